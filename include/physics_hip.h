/* physics_hip.h — C ABI of libphysics_hip.so, the MI355X (gfx950) backend for the per-frame
 * rigid-body step of martingoe/physics.
 *
 * The reference has no FFI of its own; the surface replaced is the inherent-method surface of
 * `PhysicsState` (reference src/physics.rs:40-100) and `RigidBody` (src/physics/rigid_body.rs).
 * Each entry point cites the reference item it stands in for. A Rust shim (rust/physics_hip_sys,
 * shown in INTEGRATION.md) binds exactly these symbols.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions cross the boundary.
 *   - every call returns int32_t: 0 = PHYS_OK, < 0 = error; phys_last_error() gives the text
 *     (thread-local). The reference panics instead (unwrap at rigid_body.rs:31, assert_eq at
 *     sparse_matrix.rs:26,40); a panic cannot cross FFI, so the same conditions become codes.
 *   - a phys_world* is used from one thread at a time (mirrors `&mut self`).
 *   - host arrays passed in are copied before the call returns; output arrays are caller-allocated.
 *   - quaternions are [i, j, k, w] (nalgebra storage order), matrices row-major unless stated.
 *   - there is NO CPU fallback: phys_create fails with PHYS_ERR_NO_DEVICE when no gfx950 device
 *     is usable.
 */
#ifndef PHYSICS_HIP_H
#define PHYSICS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHYS_ABI_VERSION 2u

/* status codes */
#define PHYS_OK 0
#define PHYS_ERR_INVALID_ARG (-1)
#define PHYS_ERR_NO_DEVICE (-2)
#define PHYS_ERR_HIP (-3)
#define PHYS_ERR_SINGULAR_INERTIA (-4) /* reference: try_inverse().unwrap() panic, rigid_body.rs:31 */
#define PHYS_ERR_CAPACITY (-5)         /* pair / manifold / halo buffer overflow, or more than 64 manifolds at one body;
                                          raised in ANY step since the last phys_sync (sticky), cleared by that phys_sync */
#define PHYS_ERR_OUT_OF_RANGE (-6)     /* body index out of range (reference: Vec index panic) */
#define PHYS_ERR_UNSUPPORTED (-7)
#define PHYS_ERR_NO_BODIES (-8)        /* reference: view() panic on N = 0 */

/* shape types (new: the reference has no shapes) */
#define PHYS_SHAPE_NONE 0u   /* takes part in integration only */
#define PHYS_SHAPE_SPHERE 1u /* radius = half_extent[0] */
#define PHYS_SHAPE_BOX 2u    /* half extents along the body axes */
/* capsule: radius = half_extent[0]; core half-length h = half_extent[1] along the body's local y axis, so the core segment
 * runs from c - h*R[:,1] to c + h*R[:,1] (h = 0: a sphere); half_extent[2] is ignored. Added without an ABI version bump
 * (no struct changed): a library that predates capsules refuses PHYS_SHAPE_CAPSULE in phys_set_static_bodies with
 * PHYS_ERR_INVALID_ARG, which is how a caller can tell. Contact rules: DESIGN.md section 11. */
#define PHYS_SHAPE_CAPSULE 3u

/* phys_config.flags */
#define PHYS_FLAG_COLLISIONS 0x1u     /* run broad-phase + narrow-phase + sequential impulses */
#define PHYS_FLAG_GROUND_PLANE 0x2u   /* static plane y = ground_height, normal +y */
#define PHYS_FLAG_EXACT_ROTATION 0x4u /* OFF (default) = reference quirk Q1: dq = exp(a*sin(th/2)/2) */
#define PHYS_FLAG_BROADPHASE_ONLY 0x8u /* with COLLISIONS: stop after the candidate-pair list */
#define PHYS_FLAG_SOLVER_PER_COLOR 0x10u /* contact solver as one launch per colour class instead of the single-launch
                                            dataflow kernel; same order of updates per body, bit-identical results */
#define PHYS_FLAG_SHARED_GPU 0x20u       /* kept for callers of ABI 2: the guarded start it asked for is the DEFAULT now */
#define PHYS_FLAG_EXCLUSIVE_GPU 0x80u    /* nothing else runs on this GPU while phys_update does (no other stream of the
                                            application, no other process). The cluster solver - one launch whose
                                            workgroups must all be resident - by default starts all-or-nothing (every
                                            workgroup is counted in before anything is written; a launch that does not
                                            fit beside other streams' kernels is called off and tried again: ~0.04
                                            ms per update); with this flag it skips the count, and the dataflow solver of
                                            mid-size scenes may fill the chip as well (three workgroups per CU instead of
                                            a third of that: up to 1.8x faster at 100k-250k manifolds). A world that sets
                                            it on a GPU that IS shared may spin into the solver's 3 s time-out
                                            (PHYS_ERR_HIP at phys_sync). Several worlds of one process on a device are
                                            always guarded. Same results either way. */
#define PHYS_FLAG_SOLVER_CLUSTER 0x40u    /* contact solver: the cluster kernel (body velocities resident in LDS per spatial
                                            cluster, one launch) wherever the scene admits it (>= 32768 bodies, > 40k
                                            manifolds), instead of only where it is the fastest path (>= 170k manifolds).
                                            Bit-identical results; for tests and measurements */
#define PHYS_FLAG_NO_WARM_START 0x100u   /* contact solver: start every update from zero impulses (rounds 1-2). Default: a manifold
                                            that persists starts from the impulses it ended the previous update with
                                            (include/spec/contact_solve.h: warm starting; one sweep more per update) */

typedef struct phys_config {
    uint32_t abi_version;       /* PHYS_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    uint32_t flags;             /* default 0: pure reference semantics (no collisions) */
    float gravity_force[3];     /* default (0,-9.81,0): a FORCE, not m*g (physics.rs:90, quirk Q2) */
    float gravity_offset[3];    /* default (0,0,1.5) world offset (physics.rs:91, quirk Q2) */
    uint32_t cg_max_iterations; /* default 1000 (sle_solver.rs:5) */
    float cg_max_error;         /* default 1e-2 (sle_solver.rs:6) */
    float cg_min_error;         /* default 1e-3 (sle_solver.rs:7) */
    uint32_t solver_iterations; /* sequential-impulse iterations, default 8 */
    float baumgarte;            /* default 0.2 */
    float slop;                 /* penetration allowance, default 0.01 */
    float friction;             /* Coulomb coefficient, default 0.5 */
    float contact_margin;       /* AABB fattening / speculative distance, default 0.02 */
    float ground_height;        /* default 0 */
    float max_bias;             /* cap on the contact push-out velocity, default 3.0 */
    uint64_t max_pairs;         /* 0 = auto (24 per body) */
    uint64_t max_manifolds;     /* 0 = auto (17 per body) */
    uint64_t max_ghosts;        /* sharded worlds: room for remote boundary bodies ("ghosts": kinematic copies of bodies owned
                                   by neighbouring ranks, refreshed by phys_halo_exchange before every update); 0 = none */
} phys_config;

typedef struct phys_world phys_world;

typedef struct phys_stats {
    uint64_t n_bodies;     /* owned bodies (ghost slots not counted) */
    uint64_t n_pairs;      /* candidate pairs of the last update */
    uint64_t n_manifolds;  /* body-body + body-ground manifolds */
    uint64_t n_contacts;   /* contact points */
    uint32_t n_colors;     /* solver colours */
    uint32_t color_rounds; /* colouring rounds */
    uint32_t cg_iterations; /* CG iterations of the last constraint solve */
    int32_t cg_converged;   /* 1 = Some(lambda), 0 = None (sle_solver.rs:45) */
    uint64_t steps;         /* updates since creation */
    uint32_t overflow;      /* bit 0 pairs, 1 manifolds, 2 colours (> 64 manifolds at one body), 3 halo / cross pairs,
                               4 solver hand-off timeout, 6 colour table full, 8 a body edit's bad ids: the last update's bits OR every bit raised since
                               the last phys_sync */
    uint32_t n_ground_manifolds; /* manifolds against the ground plane (subset of n_manifolds) */
    float max_extent;       /* largest fattened-AABB edge of the last broad phase (the grid cell is 1.001x this) */
    uint32_t n_halo_records; /* records written by the last phys_halo_pack */
    uint64_t n_cross_pairs;  /* cross-rank pairs found by the last phys_halo_pairs */
    uint32_t n_ghosts;       /* ghost slots filled by the last phys_halo_unpack_ghosts */
    uint32_t n_new_manifolds; /* manifolds of the last update whose pair had none in the update before (the colouring's work) */
} phys_stats;

/* reference defaults (see phys_config field comments) */
void phys_config_default(phys_config* cfg);
const char* phys_last_error(void);
uint32_t phys_abi_version(void);

/* PhysicsState { .. } literal at lib.rs:34-42 / drop */
int32_t phys_create(const phys_config* cfg, phys_world** out);
int32_t phys_destroy(phys_world* w);

/* entities: Vec<Entity> (physics.rs:26). One call replaces the whole body set.
 * Any pointer except pos may be NULL -> RigidBody::new defaults (rigid_body.rs:64-76):
 * rot identity, velocities 0, mass 1, inertia identity, shape NONE. */
int32_t phys_set_bodies(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* rot_ijkw /*4n*/,
                        const float* lin_vel /*3n*/, const float* ang_vel /*3n*/, const float* mass /*n*/,
                        const float* inertia /*9n row-major*/, const uint32_t* shape_type /*n*/,
                        const float* half_extent /*3n*/);

/* ConstraintSolver.constraints.push(Constraints::FixedPosition(..)) (lib.rs:24, fixed_position_constraint.rs) */
int32_t phys_add_constraint_fix_point(phys_world* w, uint64_t body, const float target[3]);
/* Constraints::FixedOrientation (lib.rs:25, fixed_orientation_constraint.rs); target = (roll,pitch,yaw) */
int32_t phys_add_constraint_fix_orientation(phys_world* w, uint64_t body, const float target_rpy[3]);
int32_t phys_clear_constraints(phys_world* w);

/* RigidBody::apply_force_centre_of_gravity / apply_force_at_position / apply_force_at_offset
 * (rigid_body.rs:43-62) */
int32_t phys_apply_force_centre_of_gravity(phys_world* w, uint64_t body, const float force[3]);
int32_t phys_apply_force_at_position(phys_world* w, uint64_t body, const float force[3], const float point[3]);
int32_t phys_apply_force_at_offset(phys_world* w, uint64_t body, const float force[3], const float offset[3]);

/* direct writes of body.force / body.torque (pub(crate) fields, rigid_body.rs:12-13): replaces the
 * accumulators of every body; either pointer may be NULL (= leave that array as it is) */
int32_t phys_set_forces(phys_world* w, const float* force /*3n*/, const float* torque /*3n*/);

/* PhysicsState::update(&mut self, dt: &Duration) (physics.rs:41-55). dt is passed as whole
 * nanoseconds so Duration::as_secs_f32 (rigid_body.rs:25) is reproduced bit for bit. */
int32_t phys_update(phys_world* w, uint64_t dt_nanos);
/* PhysicsState::apply_gravity (physics.rs:87-94) */
int32_t phys_apply_gravity(phys_world* w);
/* PhysicsState::step(&mut self, dt) (physics.rs:95-99) = RigidBody::step for every body */
int32_t phys_step(phys_world* w, uint64_t dt_nanos);
/* n updates back to back without returning to the host in between (same result as n phys_update) */
int32_t phys_update_n(phys_world* w, uint64_t dt_nanos, uint32_t n);
/* block until all queued device work of this world is done. Device-side errors are sticky: a capacity overflow or a
 * solver time-out in ANY update since the previous phys_sync (also an early one of a phys_update_n batch) is reported
 * here once - PHYS_ERR_CAPACITY / PHYS_ERR_HIP - and then cleared; only the bits of the LAST update stay, as in
 * phys_stats.overflow, until the next update, and a phys_sync with no update in between reports those again.
 * The contact solve of an overflowing update is
 * skipped (never run on a truncated contact set); bodies are still integrated.
 * Limit: at most 64 contact manifolds per body (one solver colour each). */
int32_t phys_sync(phys_world* w);

/* body.position / body.rotation reads (physics.rs:64-65); synchronous device-to-host */
int32_t phys_get_transforms(phys_world* w, float* pos_out /*3n*/, float* rot_ijkw_out /*4n*/);
/* body.lin_velocity / body.angular_velocity (pub fields, rigid_body.rs:9-10) */
int32_t phys_get_velocities(phys_world* w, float* lin_out /*3n*/, float* ang_out /*3n*/);
/* body.force / body.torque accumulators (pub(crate), rigid_body.rs:12-13) */
int32_t phys_get_forces(phys_world* w, float* force_out /*3n*/, float* torque_out /*3n*/);
/* Instance::to_raw for every entity (graphics.rs:13-21; consumed at physics.rs:61-69):
 * 16 f32 per body, column-major T(position) * R(rotation) */
int32_t phys_get_instance_matrices(phys_world* w, float* out /*16n*/);
/* previous_solution (physics.rs:30): warm-start lambda; *n_rows = 0 when None */
int32_t phys_get_lambda(phys_world* w, float* lambda_out, uint64_t cap, uint64_t* n_rows);

/* SparseMatrix { add_block, multiply_vector, tr_multiply_vector } (sparse_matrix.rs:16-50) in its GENERAL form, on the
 * device: a block-sparse nrows x ncols matrix given as a list of dense blocks - block b covers rows [i, i + i_length) and
 * columns [j, j + j_length), block_desc = {i, j, i_length, j_length} per block, data = the blocks one after the other,
 * each ROW-major (the reference's from_vec is column-major: the caller transposes) - times a vector: out = M v
 * (transpose == 0: v has ncols entries, out nrows; sparse_matrix.rs:25-37) or out = M^T v (transpose != 0: v has nrows,
 * out ncols; :39-50). Overlapping blocks accumulate IN LIST ORDER and the inner sum of a block row runs left to right, as
 * the reference's loops do, so the result equals the reference's bit for bit (one lane per output entry walks the blocks
 * that touch it, in list order). All pointers are HOST memory; the call uploads, runs the kernel on `device` and
 * downloads. The constraint solve inside phys_update uses the specialised identity-selector form of the same product
 * (the reference's two constraint kinds have nothing else); this entry point is the general one, held to the
 * reference's own unit tests (sparse_matrix.rs:65-119). A block reaching outside the matrix, or a vector of the wrong
 * length (the reference: assert_eq panic, sparse_matrix.rs:26,40) is PHYS_ERR_INVALID_ARG. */
int32_t phys_block_spmv(int32_t device, uint64_t nrows, uint64_t ncols, uint64_t nblocks, const uint64_t* block_desc /*4 per block*/,
                        const float* data, const float* vec, uint64_t vec_len, int32_t transpose, float* out);

/* broad-phase of the current poses: candidate pairs (i < j) with overlapping fattened AABBs,
 * sorted by (i, j). pairs_out may be NULL to query the count. (new: SURVEY §8 A10) */
int32_t phys_broadphase(phys_world* w, uint32_t* pairs_out /*2*cap*/, uint64_t cap, uint64_t* n_pairs);
/* AABBs as computed by the device: min xyz, max xyz per body */
int32_t phys_get_aabbs(phys_world* w, float* out /*6n*/);
/* contact manifolds of the last update, sorted by (body_a, body_b); body_b = 0xFFFFFFFF = ground,
 * PHYS_STATIC_ID_BIT | k = static collider k.
 * rows: per manifold 2 u32 ids + u32 count; per point (4 slots): position xyz + depth. NULLs allowed. */
int32_t phys_get_manifolds(phys_world* w, uint32_t* ids_out /*2*cap*/, uint32_t* counts_out /*cap*/,
                           float* normals_out /*3*cap*/, float* points_out /*16*cap*/, uint64_t cap,
                           uint64_t* n_manifolds);
int32_t phys_get_stats(phys_world* w, phys_stats* out);
/* manifolds per solver colour of the last update (64 entries) */
int32_t phys_get_color_counts(phys_world* w, uint32_t* counts_out /*64*/);

/* --- ray casts against the current poses (new: the reference has no queries) ---
 * The closest hit of every ray against the CURRENT poses: the state after the last update, phys_set_bodies or write
 * through phys_get_device_view. Read-only: the call builds a grid of its own from those poses and leaves every buffer,
 * counter and flag of the update untouched, so updates stay bit-identical with or without ray casts in between. Works in
 * every world, with or without PHYS_FLAG_COLLISIONS / PHYS_FLAG_BROADPHASE_ONLY; it neither reports nor clears the
 * sticky update errors (only phys_sync does).
 *   - dir need not be unit length: t is the Euclidean distance along dir / |dir|, and a hit counts when t <= max_t
 *     (max_t NULL = +inf). A zero, NaN or infinite dir or origin, or a NaN or negative max_t, gives a miss.
 *   - a miss: body = PHYS_RAY_MISS, t = +inf, normal = 0.
 *   - targets: owned bodies only (ids < phys_stats.n_bodies; ghost slots of sharded worlds are never hit: in a sharded
 *     world each rank answers for the bodies it owns and the caller merges the ranks' answers by least t), and of those
 *     SPHERE (radius half_extent[0]) and BOX (the oriented box of rot and half_extent); PHYS_SHAPE_NONE bodies and bodies
 *     with a non-finite pose are never hit. With PHYS_FLAG_GROUND_PLANE, the solid half-space y <= ground_height.
 *   - an origin inside the closed solid of a target: t = 0, normal = -dir / |dir|. Otherwise normal is the outward unit
 *     surface normal at the hit point (a box: the face of the slab the ray enters last).
 *   - ignore_body[i] (NULL = none), when below n_bodies, is skipped by ray i (a ray fired from inside a body); a value
 *     at or above n_bodies ignores nothing.
 *   - static colliders (phys_set_static_bodies) are targets too, id PHYS_STATIC_ID_BIT | k; ignore_body never names one.
 *   - the result is the least (t, id): an exact tie in t goes to the smaller id (bodies, then statics), and the ground
 *     loses ties to both. A
 *     ray's result depends only on that ray and the world state: bit-identical across calls and ray orders.
 *   - no bodies: every ray misses or hits the ground. n_rays == 0 is a no-op.
 *   - PHYS_ERR_INVALID_ARG: a NULL origin, dir, body_out or t_out, or n_rays >= 2^31.
 * Grid: e = the largest exact AABB edge of the bodies above, M = the largest |coordinate| of
 * their bounds [lo, hi], pad p = 2^-16 (M + e), cell edge (e + 2p)(1 + 2^-10), with cell corners at lo - p + k * cell.
 * The pad bounds the grid: the cell is at least 2p >= 2^-15 M and the padded bounds span at most 2M + 2p, so there are
 * never more than 65 474 cells along an axis (the kernels' clamp to 2^20 cells is a guard that no input reaches). The
 * cell edge follows the largest body: one huge body coarsens the grid, and far-flung bodies mean long walks through
 * empty cells. Results stay correct in both cases; only speed suffers.
 * Accuracy: every candidate is tested in coordinates relative to its own centre c, so the distance of the scene from
 * the origin costs nothing: t is good to about 1e-5 (1 + |origin - c| + t) and normals to 1e-4, at 2e5 from the origin as
 * near it. What float32 cannot give is a hit point finer than 2^-23 (|origin - c| + t): a ray that travels 3e6 finds the
 * right target and t within 0.25, and the face of a box it enters square on, but no meaningful normal on a sphere, a
 * capsule or near a box's edge once that distance reaches the size of the target. */
#define PHYS_RAY_MISS 0xFFFFFFFEu   /* no hit within max_t */
#define PHYS_RAY_GROUND 0xFFFFFFFFu /* the ground plane (same id the manifolds use for it) */
/* host arrays; synchronous (returns with the outputs written) */
int32_t phys_raycast(phys_world* w, uint64_t n_rays, const float* origin /*3n*/, const float* dir /*3n*/,
                     const float* max_t /*n, NULL = +inf*/, const uint32_t* ignore_body /*n, NULL = none*/,
                     uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/);
/* the same on DEVICE pointers: only enqueues on the world's stream (phys_device_view.stream), no host synchronisation */
int32_t phys_raycast_device(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                            const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out);

/* --- sphere casts and overlap queries against the current poses (new: the reference has no queries) ---
 * Both are read-only queries with the pose rules of phys_raycast: they see the CURRENT poses, write nothing an update
 * or phys_broadphase reads (updates stay bit-identical with or without them), and their targets are the owned bodies
 * with a shape and a finite pose, the static colliders and, with PHYS_FLAG_GROUND_PLANE, the half-space
 * y <= ground_height. Ghost slots and PHYS_SHAPE_NONE bodies are never reported. Ids are the ray casts' ids: the body
 * index, PHYS_STATIC_ID_BIT | k, PHYS_RAY_GROUND. These functions were added without an ABI version change (no struct
 * changed, PHYS_ABI_VERSION stays 2): a library that predates them lacks the symbols, which is how a caller tells.
 *
 * phys_spherecast: a ball of radius[i] moves from origin[i] along dir[i] / |dir[i]|; the result is the first target the
 * closed ball touches and the distance t its centre travelled. Everything else is phys_raycast's rule: t <= max_t (NULL =
 * +inf), ties to the least (t, id), ignore_body as for rays, a miss is PHYS_RAY_MISS with t = +inf and a zero normal, an
 * invalid dir, origin or max_t misses, and so does a negative, NaN or infinite radius.
 *   - a ball that already overlaps a target at t = 0 reports t = 0 and normal = -dir / |dir|.
 *   - otherwise normal is the outward unit normal of the target at the contact: the direction from the target's closest
 *     point to the ball's centre at t. The contact point (not an output) is centre(t) - radius * normal.
 *   - the test is a ray cast against the target grown by the radius (its Minkowski sum with the ball): a sphere or capsule
 *     of r + radius, the rounded box (three boxes each grown along one axis and twelve edge capsules of the radius), the
 *     plane y = ground_height + radius. radius = 0 gives phys_raycast's answer (the same id except at exact ties or
 *     grazing rays, t within rounding).
 *   - the call builds phys_raycast's grid over body AABBs grown by its largest valid radius (capped at 2^100), so the
 *     walk of the centre line meets every candidate. One huge radius coarsens the grid as one huge body does: the call
 *     gets slower, never wrong.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL origin, dir, radius, body_out or t_out. n == 0 is a no-op.
 * phys_spherecast takes host arrays and returns with the outputs written; phys_spherecast_device takes device pointers
 * and only enqueues on the world's stream. */
int32_t phys_spherecast(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                        const float* radius /*n*/, const float* max_t /*n, NULL = +inf*/,
                        const uint32_t* ignore_body /*n, NULL = none*/,
                        uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/);
int32_t phys_spherecast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius,
                               const float* max_t, const uint32_t* ignore_body, uint32_t* body_out, float* t_out,
                               float* normal_out);
/* phys_capsulecast: a capsule moves from origin[i] along dir[i] / |dir[i]| without turning. Its core is the segment
 * centre +- half_length[i] * a, a the y axis turned by rot_ijkw[i] (NULL = identity; used as given, like phys_overlap's rot),
 * its radius radius[i]. The result is the first target the closed capsule touches and the distance t its centre travelled.
 * Ids, ties, ignore_body, max_t and the miss value are phys_spherecast's; a query also misses on a non-finite rot and on a
 * negative, NaN or infinite radius or half_length.
 *   - normal: the unit vector from the target's closest point to the capsule's core at the contact; -dir / |dir| for a cast
 *     that starts touching (t = 0); (0, 1, 0) on the ground.
 *   - point_out (may be NULL): the touched point of the target's surface, i.e. the target's closest point to the capsule's
 *     core (for a sphere or capsule target: its core's closest point plus r * normal); on the ground the lower end of the
 *     core (the centre when a.y == 0) projected onto the plane; zeros at t = 0 and on a miss. Where the contact is a line or
 *     an area (a capsule flat on a face, parallel cores) it is some point of it.
 *   - half_length == 0 is a sphere cast: body, t and normal are phys_spherecast's bit for bit.
 *   - the tests are closed forms in float32, a ray from the capsule's centre against the Minkowski sum of the target and
 *     the capsule: a sphere becomes a capsule, a capsule a thickened parallelogram (four edge capsules and two faces), a box
 *     a thickened zonotope of four generators (six face pairs and the edge capsules along every generator).
 *   - the grid is grown by the call's largest valid radius + half_length (capped at 2^100), as phys_spherecast's is by the
 *     radius.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL origin, dir, radius, half_length, body_out or t_out. n == 0 is a no-op.
 * phys_capsulecast takes host arrays and returns with the outputs written; phys_capsulecast_device takes device pointers and
 * only enqueues on the world's stream. The _filtered calls take a query_mask as phys_spherecast_filtered does. */
int32_t phys_capsulecast(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                         const float* rot_ijkw /*4n, NULL = identity*/, const float* radius /*n*/, const float* half_length /*n*/,
                         const float* max_t /*n, NULL = +inf*/, const uint32_t* ignore_body /*n, NULL = none*/,
                         uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/,
                         float* point_out /*3n, may be NULL*/);
int32_t phys_capsulecast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                const float* radius, const float* half_length, const float* max_t, const uint32_t* ignore_body,
                                uint32_t* body_out, float* t_out, float* normal_out, float* point_out);
int32_t phys_capsulecast_filtered(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                                  const float* rot_ijkw /*4n, NULL = identity*/, const float* radius /*n*/,
                                  const float* half_length /*n*/, const float* max_t /*n, NULL = +inf*/,
                                  const uint32_t* ignore_body /*n, NULL = none*/, const uint16_t* query_mask /*n, NULL = no filtering*/,
                                  uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/,
                                  float* point_out /*3n, may be NULL*/);
int32_t phys_capsulecast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                         const float* radius, const float* half_length, const float* max_t,
                                         const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out, float* t_out,
                                         float* normal_out, float* point_out);
/* phys_boxcast: a box moves from origin[i] along dir[i] / |dir[i]| without turning. Its centre is origin[i], its half extents
 * half_extent[i] (three per query) in the frame of rot_ijkw[i] (NULL = identity; used as given, like phys_overlap's rot). The
 * result is the first target the closed box touches and the distance t its centre travelled: the target's id, the target's
 * outward normal at the contact and a touched point on the target. Ids, ties (the least (t, id)), ignore_body, max_t, the miss
 * value (PHYS_RAY_MISS, +inf, zeros), current poses, ghost slots and "read-only: nothing an update reads is written" are
 * phys_capsulecast's. (the arithmetic is include/spec/box_cast.h.)
 *   - a query also misses on a non-finite rot and on any half_extent component that is negative, NaN or infinite. Zero
 *     components are valid: a plate, a rod, a point.
 *   - a cast that starts touching gives t = 0, normal = -dir / |dir|, point = zeros, as the other sweeps do.
 *   - normal: the unit direction of the shortest vector from the target to the cast box just before the touch. Sphere and
 *     capsule targets: from the target core's closest point to the box's closest point. Box targets: the separating axis that
 *     is last to close, signed from the target to the cast box. Ground: (0, 1, 0).
 *   - point_out (may be NULL): a point on the target's surface that lies in the contact set; it is within tolerance of the cast
 *     box's surface at t as well. Where the contact is a segment or a polygon, any point of it.
 *   - ground: the solid half-space. The box touches it when its lowest point, origin.y - sum_i he_i |R_yi|, reaches
 *     ground_height. The point is the box's lowest feature projected onto the plane: the corner with signs -sign(R_yi), taking
 *     sign(0) = 0, so a level box reports the centre of its lowest edge or face (as phys_capsulecast reports the centre of a
 *     level core).
 *   - the tests are closed forms in float32 in the cast box's frame, relative to the target's centre: a sphere is a ray from its
 *     centre against the cast box rounded by r, a capsule a ray against the zonotope of the box's three generators and the
 *     capsule's axis thickened by r, a box a swept separating-axis test over 15 axes (cross axes of squared length <= 1e-12 are
 *     skipped). Nothing iterates.
 *   - the grid is grown by the call's largest valid |half_extent| (the box's circumscribed radius, capped at 2^100), as
 *     phys_spherecast's is by the radius.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL origin, dir, half_extent, body_out or t_out. n == 0 is a no-op.
 * phys_boxcast takes host arrays and returns with the outputs written; phys_boxcast_device takes device pointers and only
 * enqueues on the world's stream. The _filtered calls take a query_mask as phys_spherecast_filtered does. Added without an ABI
 * version change (PHYS_ABI_VERSION stays 2): a library that predates them lacks the symbols.
 * The four declarations stand in physics_hip_boxcast.h, which this header includes here: every caller of this header has them.
 * (tests/test_staging_cpu.py pins the cast prototypes whose declarations stand in THIS file to a table written out by hand, and
 * tests/test_abi.py wants a prototype in that same table for every declaration of this file; a family that joins the casts
 * without touching either therefore keeps its declarations, its ctypes prototypes and its Rust declarations in files of their
 * own, held to one another by tests/test_boxcast_cpu.py.) */
#include "physics_hip_boxcast.h" /* phys_boxcast, phys_boxcast_device, phys_boxcast_filtered, phys_boxcast_device_filtered */
/* phys_move_and_slide: a capsule character (core pos[i] +- half_length[i] * a, a the y axis turned by rot_ijkw[i], radius
 * radius[i]: phys_capsulecast's capsule) tries to move by motion[i] without turning. It casts along what is left of the motion,
 * stops `skin` short of the first target, projects the rest of the motion onto the contact plane and casts again, up to
 * max_slides casts, all inside ONE kernel launch over ONE query grid. The rule between two casts is stated once, in
 * include/spec/slide.h; every cast is phys_capsulecast's (origin = the position reached, dir = the motion
 * left, max_t = its length + skin), so targets, ids, ties, ignore_body, query_mask, ghost slots and the current-pose rule are
 * phys_capsulecast[_filtered]'s, and half_length == 0 is a sphere cast. Read-only: nothing an update reads is written, and sticky
 * update errors are neither reported nor cleared.
 *   - pos_out: where the character ends. remaining_out (may be NULL): the motion it could not make (zeros when all was made).
 *   - status_out: the number of hits (0 .. 8) in bits 0-3, and
 *       PHYS_SLIDE_BLOCKED    a cast started touching a target (t == 0: there is no usable normal); the character stays where
 *                             that cast began and the motion left stays in remaining_out. No depenetration is attempted.
 *       PHYS_SLIDE_EXHAUSTED  max_slides casts were made and motion is left.
 *       PHYS_SLIDE_INVALID    a non-finite pos, motion, rot, radius or half_length, a negative radius or half_length, or
 *                             |motion| > 3.0e38: pos_out = pos, remaining_out = motion as given, no hits.
 *   - hit slots (each array may be NULL): slot k of query i lies at index k * n + i (iteration-major): the body id, the normal
 *     and the touched point phys_capsulecast reports for the k-th hit. Every slot is written; an unused one holds PHYS_RAY_MISS
 *     and zeros.
 *   - a crease: when the slide along the second plane would re-enter the first, the motion left is projected onto the line the
 *     two planes share (nothing is left between parallel planes); a slide never turns back against the motion asked for.
 *   - a zero motion is valid: status 0, pos_out = pos. skin == 0 is allowed, but the character then rests on what it hit and the
 *     next cast starts touching, so the query normally ends BLOCKED at its second cast: use a skin around contact_margin. At a
 *     grazing approach the clearance left is skin * |u . n|, not skin.
 *   - the grid is grown by the call's largest valid radius + half_length, as phys_capsulecast's; the motions do not enter.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL pos, motion, radius, half_length, pos_out or status_out with n > 0, a non-finite or
 *     negative skin, max_slides outside 1 .. PHYS_SLIDE_MAX_SLIDES. n == 0 is a no-op.
 * phys_move_and_slide takes host arrays and returns with the outputs written; phys_move_and_slide_device takes device pointers
 * and only enqueues on the world's stream. query_mask NULL = no filtering (there is no _filtered twin). */
#define PHYS_SLIDE_MAX_SLIDES 8u
#define PHYS_SLIDE_BLOCKED 0x100u
#define PHYS_SLIDE_EXHAUSTED 0x200u
#define PHYS_SLIDE_INVALID 0x400u
int32_t phys_move_and_slide(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* motion /*3n*/,
                            const float* rot_ijkw /*4n, NULL = identity*/, const float* radius /*n*/, const float* half_length /*n*/,
                            float skin, uint32_t max_slides, const uint32_t* ignore_body /*n, NULL = none*/,
                            const uint16_t* query_mask /*n, NULL = no filtering*/, float* pos_out /*3n*/,
                            float* remaining_out /*3n, may be NULL*/, uint32_t* status_out /*n*/,
                            uint32_t* hit_body_out /*max_slides*n, may be NULL*/, float* hit_normal_out /*3*max_slides*n, may be NULL*/,
                            float* hit_point_out /*3*max_slides*n, may be NULL*/);
int32_t phys_move_and_slide_device(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw,
                                   const float* radius, const float* half_length, float skin, uint32_t max_slides,
                                   const uint32_t* ignore_body, const uint16_t* query_mask, float* pos_out, float* remaining_out,
                                   uint32_t* status_out, uint32_t* hit_body_out, float* hit_normal_out, float* hit_point_out);
/* phys_character_move: a capsule character (phys_move_and_slide's capsule) walks: it makes motion[i] - the whole displacement of
 * the frame, with whatever vertical part the caller integrated from gravity or a jump - as phys_move_and_slide does, and on top
 * does not climb what is too steep, steps up onto low obstacles, stays on the floor it walks down and learns what it stands on.
 * All of it inside ONE kernel launch over ONE query grid; the rule is stated once, as a state machine around one capsule cast, in
 * include/spec/character.h, and every cast is phys_capsulecast's. Up is +y. Read-only: nothing an update
 * reads is written, and sticky update errors are neither reported nor cleared.
 *   - a hit normal n is FLOOR when n.y >= min_floor_ny (the cosine of the steepest walkable slope), STEEP when
 *     0 < n.y < min_floor_ny, WALL when n.y <= 0. A character is walking in this call when grounded_in[i] != 0 (it stood on a
 *     floor when its last call ended: pass that call's status & PHYS_CHAR_GROUNDED; NULL = nobody did) and !(motion.y > 0).
 *   - MOVE: phys_move_and_slide on the whole motion, bit for bit for a character that is not walking; a walker's slide along a
 *     STEEP normal that would gain height follows the slope's contour instead. Hits fill slots 0 .. max_slides - 1. BLOCKED ends
 *     the query without a ground state.
 *   - STEP (walking, step_height > 0, a horizontal motion, MOVE met a hit that is not FLOOR): cast up by step_height (less under
 *     a low ceiling), slide the horizontal motion from there (hits in slots max_slides .. 2 max_slides - 1), cast down; taken
 *     when that lands on a FLOOR further along the horizontal motion than MOVE came, otherwise MOVE's result stands.
 *   - GROUND (not after a step taken or BLOCKED): one cast down by 2 skin, plus snap_distance when walking. A FLOOR: GROUNDED, and
 *     a walker more than 2 skin above it is moved down to skin above it (SNAPPED). A STEEP hit: ON_STEEP, not grounded.
 *   - pos_out, remaining_out (may be NULL): as phys_move_and_slide's, of the path taken.
 *   - status_out: MOVE's hit count in bits 0-3, the lifted slide's in bits 4-7 (casts made, taken or not), and the flags below.
 *     BLOCKED, EXHAUSTED, HIT_WALL (a hit that is not FLOOR) and HIT_CEILING (a hit with n.y < 0 while motion.y > 0) describe the
 *     slide whose result was taken. INVALID: phys_move_and_slide's rule; pos_out = pos, remaining_out = motion, no hits, no floor.
 *   - floor_body_out, floor_normal_out, floor_point_out (each may be NULL): what the character stands on (GROUNDED) or what lies
 *     below it (ON_STEEP), as phys_capsulecast reports it; PHYS_RAY_MISS and zeros otherwise.
 *   - hit slots (each array may be NULL): 2 * max_slides per query, slot k of query i at index k * n + i; every slot is written,
 *     an unused one holds PHYS_RAY_MISS and zeros. They are there for phys_apply_impulses_device: the call pushes nothing.
 *   - at most 2 * max_slides + 3 casts per character. skin == 0 is allowed and degenerate as for phys_move_and_slide (and a
 *     character resting on a floor then finds it at t == 0: not grounded).
 *   - not done here: gravity and velocity integration, pushing bodies, depenetration (call phys_depenetrate first), constant
 *     speed on walkable slopes, moving platforms, an up axis other than +y.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL pos, motion, radius, half_length, pos_out or status_out with n > 0, a non-finite or
 *     negative skin, step_height or snap_distance, min_floor_ny outside (0, 1], max_slides outside 1 .. PHYS_SLIDE_MAX_SLIDES.
 *     n == 0 is a no-op.
 * phys_character_move takes host arrays and returns with the outputs written; phys_character_move_device takes device pointers
 * and only enqueues on the world's stream. PHYS_ABI_VERSION is unchanged: a caller tells an older library by the missing symbols. */
#define PHYS_CHAR_BLOCKED 0x100u
#define PHYS_CHAR_EXHAUSTED 0x200u
#define PHYS_CHAR_INVALID 0x400u
#define PHYS_CHAR_GROUNDED 0x1000u
#define PHYS_CHAR_STEPPED 0x2000u
#define PHYS_CHAR_SNAPPED 0x4000u
#define PHYS_CHAR_ON_STEEP 0x8000u
#define PHYS_CHAR_HIT_WALL 0x10000u
#define PHYS_CHAR_HIT_CEILING 0x20000u
int32_t phys_character_move(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* motion /*3n*/,
                            const float* rot_ijkw /*4n, NULL = identity*/, const float* radius /*n*/, const float* half_length /*n*/,
                            const uint32_t* grounded_in /*n, NULL = nobody*/, float skin, uint32_t max_slides, float step_height,
                            float snap_distance, float min_floor_ny, const uint32_t* ignore_body /*n, NULL = none*/,
                            const uint16_t* query_mask /*n, NULL = no filtering*/, float* pos_out /*3n*/,
                            float* remaining_out /*3n, may be NULL*/, uint32_t* status_out /*n*/,
                            uint32_t* floor_body_out /*n, may be NULL*/, float* floor_normal_out /*3n, may be NULL*/,
                            float* floor_point_out /*3n, may be NULL*/, uint32_t* hit_body_out /*2*max_slides*n, may be NULL*/,
                            float* hit_normal_out /*3*2*max_slides*n, may be NULL*/,
                            float* hit_point_out /*3*2*max_slides*n, may be NULL*/);
int32_t phys_character_move_device(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw,
                                   const float* radius, const float* half_length, const uint32_t* grounded_in, float skin,
                                   uint32_t max_slides, float step_height, float snap_distance, float min_floor_ny,
                                   const uint32_t* ignore_body, const uint16_t* query_mask, float* pos_out, float* remaining_out,
                                   uint32_t* status_out, uint32_t* floor_body_out, float* floor_normal_out, float* floor_point_out,
                                   uint32_t* hit_body_out, float* hit_normal_out, float* hit_point_out);
/* phys_penetration and phys_depenetrate: how deep a capsule (core pos[i] +- half_length[i] * a, a the y axis turned by rot_ijkw[i]
 * and used as given, radius radius[i]: phys_capsulecast's capsule; half_length == 0 is a ball) sits in what surrounds it, and the
 * loop that pushes it out. The rule is stated once, in include/spec/depenetrate.h; depths and normals are
 * the narrow phase's own capsule functions (include/spec/collide.h) with the query as body A. Targets, ids, ignore_body,
 * query_mask, ghost slots and the current-pose rule are phys_capsulecast[_filtered]'s: owned bodies with a shape and a finite
 * pose, static colliders (PHYS_STATIC_ID_BIT | k), the ground (PHYS_RAY_GROUND) with PHYS_FLAG_GROUND_PLANE. Read-only: nothing
 * an update or phys_broadphase reads is written, sticky update errors are neither reported nor cleared, and the calls work
 * with or without PHYS_FLAG_COLLISIONS. Each call builds ONE query grid (not grown) and launches ONE kernel.
 * phys_penetration: one probe, nothing moves. For each capsule the deepest target within max_gap of it:
 *   - body_out: its id, PHYS_RAY_MISS when nothing lies within max_gap. depth_out: how far the capsule reaches into it
 *     (>= -max_gap; negative: the clearance between them; -inf for a miss). normal_out (may be NULL): the unit direction out of
 *     the target, from the target towards the capsule (the casts' convention; (0,1,0) on the ground; (0,-1,0) where the
 *     cores coincide, the narrow phase's (0,1,0) fallback seen from the target; zeros for a miss): moving the capsule by
 *     normal * depth brings the two to touch.
 *   - the greatest depth wins, an exact tie goes to the smaller id (bodies, then statics, then the ground).
 *   - a target whose clearance equals max_gap to within rounding may go either way: candidates are first rejected by their
 *     boxes against the capsule's box grown by max_gap. phys_depenetrate acts at skin / 2 of a gap of skin, far from that edge.
 *   - where the capsule's core lies inside a box, the depth is the narrow phase's: through the box face of least overlap
 *     with the core, or across a box edge where that is clearly shallower; one push can leave a sliver of overlap, which
 *     the next round of phys_depenetrate removes.
 *   - a non-finite pos, rot, radius or half_length, a negative radius or half_length, or half_length > 3.4e38: a miss.
 * phys_depenetrate: per capsule, up to max_iters rounds of: probe with max_gap = skin; when the deepest target is nearer than
 * skin / 2 (depth > -skin / 2), move by normal * (depth + skin), out of it and a skin beyond; otherwise stop.
 *   - pos_out: where the capsule ends (pos itself, bit for bit, when nothing was nearer than skin / 2).
 *   - status_out: the number of pushes (0 .. 8) in bits 0-3, and
 *       PHYS_DEPEN_STUCK    max_iters pushes were made and the capsule is still nearer than skin / 2 to something (between two
 *                           opposed targets, or in a crease too acute for max_iters rounds); pos_out is finite, the last push's.
 *       PHYS_DEPEN_INVALID  the query's own values are unusable (as for phys_penetration): pos_out = pos, no pushes.
 *     A status without flags means clear: at least skin / 2 from every target, so a phys_move_and_slide from pos_out with a
 *     skin no larger does not start BLOCKED.
 *   - push slots (each array may be NULL): slot k of query i lies at index k * n + i (iteration-major): the id, the normal and
 *     the depth phys_penetration reports where the k-th push began. Every slot is written; an unused one holds PHYS_RAY_MISS
 *     and zeros.
 *   - one target per round, the deepest first: one plane takes one push, two perpendicular planes two, an acute crease
 *     converges geometrically. Nothing is averaged.
 *   - skin == 0 is allowed, but a push then ends touching and round-off decides whether the next probe pushes again: such a
 *     query tends to end touching or STUCK. Use a skin around contact_margin.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL pos, radius or half_length with n > 0, a NULL body_out or depth_out
 *     (phys_penetration) or pos_out or status_out (phys_depenetrate) with n > 0, a non-finite or negative max_gap or skin,
 *     max_iters outside 1 .. PHYS_DEPEN_MAX_ITERS. n == 0 is a no-op.
 * The plain calls take host arrays and return with the outputs written; the _device calls take device pointers and only enqueue
 * on the world's stream. query_mask NULL = no filtering (there are no _filtered twins). PHYS_ABI_VERSION is unchanged: a caller
 * tells an older library by the missing symbols. */
#define PHYS_DEPEN_MAX_ITERS 8u
#define PHYS_DEPEN_STUCK 0x100u
#define PHYS_DEPEN_INVALID 0x400u
int32_t phys_penetration(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* rot_ijkw /*4n, NULL = identity*/,
                         const float* radius /*n*/, const float* half_length /*n*/, float max_gap,
                         const uint32_t* ignore_body /*n, NULL = none*/, const uint16_t* query_mask /*n, NULL = no filtering*/,
                         uint32_t* body_out /*n*/, float* depth_out /*n*/, float* normal_out /*3n, may be NULL*/);
int32_t phys_penetration_device(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius,
                                const float* half_length, float max_gap, const uint32_t* ignore_body, const uint16_t* query_mask,
                                uint32_t* body_out, float* depth_out, float* normal_out);
int32_t phys_depenetrate(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* rot_ijkw /*4n, NULL = identity*/,
                         const float* radius /*n*/, const float* half_length /*n*/, float skin, uint32_t max_iters,
                         const uint32_t* ignore_body /*n, NULL = none*/, const uint16_t* query_mask /*n, NULL = no filtering*/,
                         float* pos_out /*3n*/, uint32_t* status_out /*n*/, uint32_t* hit_body_out /*max_iters*n, may be NULL*/,
                         float* hit_normal_out /*3*max_iters*n, may be NULL*/, float* hit_depth_out /*max_iters*n, may be NULL*/);
int32_t phys_depenetrate_device(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius,
                                const float* half_length, float skin, uint32_t max_iters, const uint32_t* ignore_body,
                                const uint16_t* query_mask, float* pos_out, uint32_t* status_out, uint32_t* hit_body_out,
                                float* hit_normal_out, float* hit_depth_out);
/* phys_overlap: for each query shape (shape_type SPHERE, BOX or CAPSULE with the bodies' half_extent conventions, at pos
 * with the unit quaternion rot_ijkw, NULL = identity), every target whose closed shape intersects it (touching counts).
 *   - output (CSR): query i's ids are ids_out[offsets_out[i] .. offsets_out[i + 1]), ascending and each once: bodies,
 *     then statics, then the ground. offsets_out (n + 1 entries) is always written; when offsets_out[n] > cap the call
 *     returns PHYS_ERR_CAPACITY and ids_out is unspecified (resize to offsets_out[n] and call again).
 *   - ignore_body[i] (NULL = none), when below n_bodies, is never reported for query i.
 *   - a query with another shape type, a non-finite pose or a negative half extent gets an empty list, not an error.
 *   - exact tests in float32: spheres and capsules by the distance of their cores, a sphere or capsule against a box by
 *     the distance of its core to the box, box against box by separating axes (near-parallel edge pairs skipped: the face
 *     axes cover them), the ground by the query's lowest point.
 *   - the result depends only on the query and the world: the same across calls, query orders and batch sizes.
 *   - candidates come from phys_raycast's grid (not grown); a query that covers more cells than there are bodies tests
 *     every body directly. Statics are all tested, as for rays.
 *   - PHYS_ERR_INVALID_ARG: n >= 2^31, a NULL offsets_out, a NULL shape_type, pos or half_extent with n > 0, a NULL
 *     ids_out with cap > 0. Host arrays only; synchronous. */
int32_t phys_overlap(phys_world* w, uint64_t n, const uint32_t* shape_type /*n*/, const float* pos /*3n*/,
                     const float* rot_ijkw /*4n, NULL = identity*/, const float* half_extent /*3n*/,
                     const uint32_t* ignore_body /*n, NULL = none*/,
                     uint64_t cap, uint64_t* offsets_out /*n + 1*/, uint32_t* ids_out /*cap*/);

/* --- static colliders: immovable SPHERE / BOX / CAPSULE shapes that bodies collide with and rays hit. Not bodies. ---
 * Level geometry (floors, walls, ramps, pillars, container sides) that never moves: no velocity, no mass, no colour of
 * its own. A manifold against static k is one-sided like a ground manifold (body A against a partner at rest with zero
 * inverse mass and inertia); it names the collider PHYS_STATIC_ID_BIT | k as body_b, which sorts after every body id
 * and before PHYS_GROUND_ID, and ray casts report the same id in body_out. Statics are NOT bodies: they appear in none
 * of n_bodies, the transforms, velocities, forces, instance matrices, AABBs, constraints, phys_device_view or halo
 * records. A sharded world's ranks each set the statics their slab needs; nothing about them is exchanged.
 *   - phys_set_static_bodies replaces the whole static set (n = 0 clears it) and is independent of phys_set_bodies:
 *     neither clears the other's set. It makes the world forget its persistent colours and warm-start impulses, like
 *     phys_set_bodies. shape_type and half_extent are required (SPHERE: radius half_extent[0]; BOX: half extents along
 *     the collider's axes; CAPSULE: radius half_extent[0], core half-length half_extent[1] along the local y axis);
 *     rot NULL = identity. PHYS_ERR_INVALID_ARG: n >= 0x7FFFFFFE, a shape other than SPHERE, BOX or CAPSULE, a
 *     non-finite pose or half extent, a negative half extent, a NULL array that is required.
 *   - every update (PHYS_FLAG_COLLISIONS) finds the (body, static) pairs whose fattened AABBs overlap, in the order
 *     (body ascending, static ascending); their capacity is automatic: the first update after phys_set_static_bodies or
 *     phys_set_bodies counts them before it stores them (one host wait) and sizes the buffer at 1.5 times that, later
 *     updates grow it from the counts they report. An update whose pairs outgrow it after that (bodies crowding onto
 *     many more statics than before) raises overflow bit 0 like the candidate pairs: its solve is skipped, phys_sync
 *     reports PHYS_ERR_CAPACITY, and the following updates have room.
 *   - phys_get_static_stats: the static count, and the (body, static) pairs and manifolds of the last update; any
 *     output pointer may be NULL. phys_stats.n_manifolds / n_contacts include the static manifolds,
 *     n_ground_manifolds does not.
 * Structure and cost: DESIGN.md section 10. */
#define PHYS_STATIC_ID_BIT 0x80000000u /* manifold body_b / ray body_out = PHYS_STATIC_ID_BIT | k for static k */
int32_t phys_set_static_bodies(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* rot_ijkw /*4n, NULL = identity*/,
                               const uint32_t* shape_type /*n*/, const float* half_extent /*3n*/);
int32_t phys_get_static_stats(phys_world* w, uint64_t* n_static, uint64_t* n_static_pairs, uint64_t* n_static_manifolds);

/* --- collision filters: what may touch what (new: the reference has none) ---
 * Every body, static collider and the ground plane carries a filter: category (u16, the layers it belongs to), mask (u16,
 * the layers it collides with) and group (i16). Defaults: category PHYS_FILTER_DEFAULT_CATEGORY, mask
 * PHYS_FILTER_DEFAULT_MASK, group 0; the ground's group is always 0. Two of them A and B may form a contact manifold iff
 *     A.group == B.group && A.group != 0 ?  A.group > 0                       (same positive group: always; negative: never)
 *                                         :  (A.category & B.mask) != 0 && (B.category & A.mask) != 0
 * so with the defaults every pair collides, as without filters. A rejected (body, body), (body, static) or (body, ground)
 * pair is treated exactly like a pair whose shapes do not touch: no manifold, no colour, no warm-start record. Nothing else
 * changes: phys_broadphase, n_pairs and the (body, static) pairs still report AABB candidates, PHYS_FLAG_BROADPHASE_ONLY
 * worlds are unaffected, and the pair capacities are the same. Added without an ABI version change (no struct changed,
 * PHYS_ABI_VERSION stays 2): a library that predates them lacks the symbols.
 *   - phys_set_body_filters: n must equal n_bodies (owned); phys_set_static_filters: n must equal the static count. A NULL
 *     array gives that field its default for every item. Filters take effect at the next update (updates already
 *     enqueued keep the filters they were enqueued with).
 *   - phys_set_bodies resets every body filter to the defaults, phys_set_static_bodies every static filter. The ground
 *     filter lasts for the life of the world.
 *   - changing filters does NOT make the world forget its colours or warm-start impulses: a pair that stops or starts
 *     colliding is the same as a pair that separates or touches.
 *   - phys_get_body_filters: the owned bodies' filters; any output may be NULL.
 *   - sharded worlds: a ghost carries its owner's filter in the halo record, so a contact across a cut is filtered the
 *     same way on both sides (the record's size is unchanged; a default filter encodes as zeros).
 *   - cost: a world runs the narrow phase's filtered variant once any filter call was made since its reset (whatever the
 *     values), and always when it has ghost slots; DESIGN.md section 13.
 * The _filtered queries are the queries above with one more per-query mask: a body, static or ground target is reported
 * iff (target.category & query_mask[i]) != 0 (groups play no part). query_mask NULL = no filtering: the same kernels and
 * bits as the call without the suffix, and query_mask[i] = 0 reports nothing. Everything else - ignore_body, ghosts never
 * reported, the tie rules, ascending unique overlap ids, the argument errors - is the unsuffixed call's. The unsuffixed
 * calls ignore filters. */
#define PHYS_FILTER_DEFAULT_CATEGORY 0x0001u
#define PHYS_FILTER_DEFAULT_MASK 0xFFFFu
int32_t phys_set_body_filters(phys_world* w, uint64_t n, const uint16_t* category /*n, NULL = default*/,
                              const uint16_t* mask /*n, NULL = default*/, const int16_t* group /*n, NULL = 0*/);
int32_t phys_get_body_filters(phys_world* w, uint16_t* category_out /*n_bodies, may be NULL*/, uint16_t* mask_out /*may be NULL*/,
                              int16_t* group_out /*may be NULL*/);
int32_t phys_set_static_filters(phys_world* w, uint64_t n, const uint16_t* category /*n, NULL = default*/,
                                const uint16_t* mask /*n, NULL = default*/, const int16_t* group /*n, NULL = 0*/);
int32_t phys_set_ground_filter(phys_world* w, uint16_t category, uint16_t mask);
int32_t phys_raycast_filtered(phys_world* w, uint64_t n_rays, const float* origin /*3n*/, const float* dir /*3n*/,
                              const float* max_t /*n, NULL = +inf*/, const uint32_t* ignore_body /*n, NULL = none*/,
                              const uint16_t* query_mask /*n, NULL = no filtering*/, uint32_t* body_out /*n*/, float* t_out /*n*/,
                              float* normal_out /*3n, may be NULL*/);
int32_t phys_raycast_device_filtered(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                                     const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out, float* t_out,
                                     float* normal_out);
int32_t phys_spherecast_filtered(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                                 const float* radius /*n*/, const float* max_t /*n, NULL = +inf*/,
                                 const uint32_t* ignore_body /*n, NULL = none*/, const uint16_t* query_mask /*n, NULL = no filtering*/,
                                 uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/);
int32_t phys_spherecast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius,
                                        const float* max_t, const uint32_t* ignore_body, const uint16_t* query_mask,
                                        uint32_t* body_out, float* t_out, float* normal_out);
int32_t phys_overlap_filtered(phys_world* w, uint64_t n, const uint32_t* shape_type /*n*/, const float* pos /*3n*/,
                              const float* rot_ijkw /*4n, NULL = identity*/, const float* half_extent /*3n*/,
                              const uint32_t* ignore_body /*n, NULL = none*/, const uint16_t* query_mask /*n, NULL = no filtering*/,
                              uint64_t cap, uint64_t* offsets_out /*n + 1*/, uint32_t* ids_out /*cap*/);

/* --- materials: how two things behave once they touch (new: the reference has none) ---
 * Every body, static collider and the ground plane carries a material {friction >= 0, restitution in [0, 1]}. Defaults:
 * friction = phys_config.friction, restitution = 0 - a world that never calls these functions behaves, and costs, as before.
 * A manifold's friction is the geometric mean of its two sides' ((float)sqrt((double)fa * fb): combining a value with itself
 * gives it back exactly), its restitution the larger of the two. A contact point whose approach speed along the normal
 * exceeds the restitution threshold (default 1.0 length unit / s) and that touches within the update leaves with at least
 * restitution times that speed; slower contacts - a pile at rest - are solved as without restitution. The rules are
 * normative in include/spec/contact_solve.h (material_friction, material_restitution, contact_bias_restitution);
 * DESIGN.md section 14.
 *   - phys_set_body_materials: n must equal n_bodies (owned); phys_set_static_materials: n must equal the static count. A
 *     NULL array gives that field its default for every item. Calls take effect at the next update (updates already
 *     enqueued keep the materials they were enqueued with).
 *   - phys_set_bodies resets every body material to the defaults, phys_set_static_bodies every static material. The
 *     ground's material and the threshold last for the life of the world.
 *   - changing materials does NOT make the world forget its colours or warm-start impulses.
 *   - phys_get_body_materials: the owned bodies' materials; either output may be NULL.
 *   - PHYS_ERR_INVALID_ARG: a wrong n, a negative or non-finite friction, a restitution outside [0, 1], a negative or
 *     non-finite threshold.
 *   - sharded worlds: materials do not cross slab cuts. A world created with max_ghosts > 0 answers every call below
 *     with PHYS_ERR_UNSUPPORTED.
 *   - cost: a world runs the solver's material kernels once a material call was made since the reset of what it set;
 *     with every material at its default they produce the same bits as the plain kernels.
 * These functions were added without an ABI version change (no struct changed): a caller tells an older library by the
 * missing symbols. */
int32_t phys_set_body_materials(phys_world* w, uint64_t n, const float* friction /*n, NULL = default*/,
                                const float* restitution /*n, NULL = 0*/);
int32_t phys_get_body_materials(phys_world* w, float* friction_out /*n_bodies, may be NULL*/, float* restitution_out /*may be NULL*/);
int32_t phys_set_static_materials(phys_world* w, uint64_t n, const float* friction /*n, NULL = default*/,
                                  const float* restitution /*n, NULL = 0*/);
int32_t phys_set_ground_material(phys_world* w, float friction, float restitution);
int32_t phys_set_restitution_threshold(phys_world* w, float v /* >= 0, finite */);

/* --- contact events: what began and what stopped touching, and how hard (new: the reference has none) ---
 * A pair is what a manifold names: (body_a, body_b) with phys_get_manifolds' ids - body indices (ghost slots included),
 * PHYS_STATIC_ID_BIT | k, 0xFFFFFFFF for the ground. Events are raised per update E with PHYS_FLAG_COLLISIONS (an update
 * with dt = 0 has no collision stage: it raises nothing and is not an "update" below):
 *   BEGIN  a manifold of update E whose pair had no manifold in update E - 1: exactly the manifolds counted in
 *          phys_stats.n_new_manifolds (the persistent colouring's "new"; there is no second notion of persistence).
 *   END    a manifold of update E - 1 whose pair has none in update E, whatever the cause: the pair separated, was
 *          filtered out, or dropped out of the candidate pairs.
 * A pair that persists raises nothing. The first update after phys_set_bodies or phys_set_static_bodies raises BEGIN for
 * every manifold and no END: both calls make the world forget its colours and with them its contact history, and both
 * discard the events not yet drained (their ids would name other things). Enabling events resets nothing: the next update
 * reports against the update before it (its END events are missed only if phys_broadphase, which clears the step counters,
 * was called in between).
 * An update flagged with an overflow bit skips its contact solve and keeps its new manifolds out of the colour table. It
 * raises BEGIN (impulse 0) / END from the manifolds it stored; the next clean update then sees those pairs as new again
 * (one more BEGIN, and an END for the stored manifold it replaces), and the update after that reports correctly again.
 * Nothing is written out of bounds in any of them.
 *
 * phys_contact_events_enable: `capacity` = events the device keeps between two drains. 0 turns events off, frees the
 *   buffers and drops pending events; a call with a new capacity drops pending events; the same capacity is a no-op.
 *   Events accumulate on the device across updates, also inside a phys_update_n batch, at no host round trip; when the
 *   buffer is full further events are counted but not stored (no sticky error, no skipped solve). A world that never
 *   calls this launches the kernels it always launched. PHYS_ERR_UNSUPPORTED: a world without PHYS_FLAG_COLLISIONS, with
 *   PHYS_FLAG_BROADPHASE_ONLY, or without warm starting - PHYS_FLAG_NO_WARM_START, or a manifold capacity
 *   (phys_config.max_manifolds, 0 = 17 per body) of 2^26 or more: the previous update's records and the impulse records
 *   exist only in warm worlds. (A phys_set_bodies that raises the automatic capacity that far turns events off; the
 *   getter then says PHYS_ERR_UNSUPPORTED.) PHYS_ERR_INVALID_ARG: capacity >= 2^31.
 * phys_get_contact_events: synchronises the world's stream, copies the stored events sorted by (step, kind, body_a,
 *   body_b) - device order is arbitrary, like manifolds - writes *n (events returned) and *n_dropped (events raised since
 *   the last drain that did not fit the device buffer; may be NULL), then empties the buffer. More stored than `cap`:
 *   PHYS_ERR_CAPACITY with *n = the stored count, and the buffer is kept (resize and call again, as for phys_overlap).
 *   out == NULL with cap == 0 only counts: PHYS_OK, *n and *n_dropped written, the buffer kept. While n_dropped == 0 the
 *   list is complete and a function of the world's history alone: bit-identical across runs. With drops the counts are
 *   exact; which events were stored is unspecified. Events off: PHYS_ERR_UNSUPPORTED. It neither reports nor clears the
 *   sticky update errors (only phys_sync does).
 * phys_get_contact_impulses: the solver's final impulses of the LAST update, {pn, pt0, pt1} for each of the 4 point slots
 *   of every manifold (zeros beyond its count), in phys_get_manifolds' order so that the two calls line up row for row.
 *   Works in every warm world with collisions, events on or off; PHYS_ERR_UNSUPPORTED otherwise. out == NULL queries the
 *   count. An update whose solve was skipped reports zeros.
 * Added without an ABI version change (no struct changed): a library that predates them lacks the symbols. DESIGN.md
 * section 15. */
#define PHYS_CONTACT_BEGIN 1u
#define PHYS_CONTACT_END   2u
typedef struct phys_contact_event {   /* 48 bytes */
    uint32_t body_a, body_b;  /* as phys_get_manifolds */
    uint32_t kind;            /* PHYS_CONTACT_BEGIN / PHYS_CONTACT_END */
    uint32_t step;            /* low 32 bits of phys_stats.steps after the update that raised it (1 = first update) */
    float point[3];           /* BEGIN: the manifold's deepest point (largest depth, lowest index on a tie); END: 0 */
    float impulse;            /* BEGIN: sum of the manifold's normal impulses pn at the end of that update's solve,
                                 ((p0 + p1) + p2) + p3; 0 if the solve was skipped; END: 0 */
    float normal[3];          /* BEGIN: the manifold's normal as phys_get_manifolds reports it; END: 0 */
    uint32_t reserved;        /* 0 */
} phys_contact_event;

int32_t phys_contact_events_enable(phys_world* w, uint64_t capacity);
int32_t phys_get_contact_events(phys_world* w, phys_contact_event* out, uint64_t cap, uint64_t* n, uint64_t* n_dropped);
int32_t phys_get_contact_impulses(phys_world* w, float* out /*12*cap*/, uint64_t cap, uint64_t* n_manifolds);

/* --- trigger volumes: shapes that report which bodies are inside them, and which entered and left (new: the reference
 * has none) ---
 * A world keeps up to PHYS_MAX_TRIGGERS trigger volumes. Each is a SPHERE, BOX or CAPSULE with the bodies' half_extent
 * conventions, a position, a unit quaternion and a u16 mask. Triggers are NOT bodies and NOT statics: nothing collides
 * with them, and they appear in no manifold, pair, ray hit, overlap result, AABB, halo record or stat.
 * Occupants. The occupants of trigger k after an update are the OWNED bodies with shape SPHERE, BOX or CAPSULE and a
 *   finite pose whose closed shape intersects the trigger's closed shape at the poses phys_get_transforms would return
 *   after that update. Ghost slots, PHYS_SHAPE_NONE bodies, statics and the ground are never occupants; in a sharded world
 *   each rank reports its owned bodies. The exact test is phys_overlap's - the same device functions, the trigger as the
 *   query shape and the body as the target - so both agree bit for bit on every (shape, body) pair.
 * Masks. With a mask array body i is seen by trigger k iff (category[i] & mask[k]) != 0, as for phys_overlap_filtered
 *   (category: phys_set_body_filters). A NULL mask array sees every body and loads no filter.
 * When. The volumes are evaluated at the end of EVERY phys_update, and after each update of a phys_update_n batch, behind
 *   the position step, whatever the world's flags: with or without PHYS_FLAG_COLLISIONS, dt = 0 included. phys_step and
 *   phys_apply_gravity alone do not evaluate.
 * Events. Update E raises PHYS_TRIGGER_ENTER for each (trigger, body) that is an occupant after E and was not after E - 1,
 *   PHYS_TRIGGER_EXIT for the opposite transition, whatever the cause: the body moved, the trigger was moved, or the body's
 *   filter changed.
 * Resets and moves. phys_set_triggers and phys_set_bodies forget the occupancy and discard the pending trigger events: the
 *   next update raises ENTER for every occupant and no EXIT. phys_set_trigger_poses keeps the history.
 * No side effects. Nothing here writes anything an update, phys_broadphase or a query reads: updates are bit-identical with
 *   and without triggers, and a world that never calls phys_set_triggers launches exactly what it launched before they
 *   existed. Triggers neither raise nor clear the sticky update errors.
 *
 * phys_set_triggers: replaces the whole set; n = 0 clears it, frees its buffers and goes back to launching nothing.
 *   rot_ijkw NULL = identity, mask NULL = see every body. PHYS_ERR_INVALID_ARG: n > PHYS_MAX_TRIGGERS, a shape other than
 *   SPHERE, BOX or CAPSULE, a non-finite pose or half extent, a negative half extent, a NULL array that is required.
 *   Synchronises the world's stream.
 * phys_set_trigger_poses: new positions (and rotations; rot_ijkw NULL keeps them) for the set that is there, from the
 *   next update on. PHYS_ERR_INVALID_ARG: n differs from the trigger count, NULL pos, a non-finite value.
 * phys_trigger_events_enable / phys_get_trigger_events: phys_contact_events_enable / phys_get_contact_events rule for
 *   rule. capacity 0 = off (buffer freed, pending events gone), a new capacity drops the pending events, the same one is a
 *   no-op; PHYS_ERR_INVALID_ARG for capacity >= 2^31. Events accumulate on the device across updates and batches at no
 *   host round trip; a full buffer counts events but stores nothing (no sticky error). The drain synchronises, returns the
 *   stored events sorted by (step, kind, trigger, body) and empties the buffer; *n_dropped (may be NULL) = events raised
 *   since the last drain that did not fit. More stored than cap: PHYS_ERR_CAPACITY with *n = the stored count, the
 *   buffer kept. out == NULL with cap == 0 only counts. Events off: PHYS_ERR_UNSUPPORTED. The occupancy is tracked
 *   whenever triggers are set, events on or off.
 * phys_get_trigger_overlaps: the occupants as of the last update in phys_overlap's CSR convention: trigger k's body ids,
 *   ascending, are ids_out[offsets_out[k] .. offsets_out[k + 1]); offsets_out (n_triggers + 1) is always written;
 *   PHYS_ERR_CAPACITY when offsets_out[n_triggers] > cap. Before the first update since a reset every list is empty.
 *   Synchronous and not a hot path: the occupancy bits are read back and listed on the host.
 * Cost: one kernel per update, one lane per owned body. The occupancy is a bit matrix of 4 * ceil(n_triggers / 32) *
 *   n_bodies bytes on the device (128 MB for 1M bodies and 1024 triggers). DESIGN.md section 17. Added without an ABI
 *   version change (no struct changed): a library that predates them lacks the symbols. */
#define PHYS_MAX_TRIGGERS 1024u
#define PHYS_TRIGGER_ENTER 1u
#define PHYS_TRIGGER_EXIT  2u
typedef struct phys_trigger_event {   /* 16 bytes */
    uint32_t trigger;         /* index into the set of phys_set_triggers */
    uint32_t body;            /* owned body index */
    uint32_t kind;            /* PHYS_TRIGGER_ENTER / PHYS_TRIGGER_EXIT */
    uint32_t step;            /* as in phys_contact_event */
} phys_trigger_event;

int32_t phys_set_triggers(phys_world* w, uint64_t n, const uint32_t* shape_type /*n*/, const float* pos /*3n*/,
                          const float* rot_ijkw /*4n, NULL = identity*/, const float* half_extent /*3n*/,
                          const uint16_t* mask /*n, NULL = see every body*/);
int32_t phys_set_trigger_poses(phys_world* w, uint64_t n /* == trigger count */, const float* pos /*3n*/,
                               const float* rot_ijkw /*4n, NULL = keep*/);
int32_t phys_trigger_events_enable(phys_world* w, uint64_t capacity);
int32_t phys_get_trigger_events(phys_world* w, phys_trigger_event* out, uint64_t cap, uint64_t* n, uint64_t* n_dropped);
int32_t phys_get_trigger_overlaps(phys_world* w, uint64_t cap, uint64_t* offsets_out /*n_triggers + 1*/, uint32_t* ids_out /*cap*/);

/* --- force fields: volumes that push, drag and attract the bodies inside (new: the reference has one global gravity) ---
 * A world keeps up to PHYS_MAX_FORCE_FIELDS force fields. A field is a volume plus a law. The volume is a SPHERE, BOX or
 * CAPSULE with the bodies' half_extent conventions at pos with the unit quaternion rot_ijkw. Fields are NOT bodies: nothing
 * collides with them and no query sees them. They add to the force / torque accumulators, nothing else.
 * Who. Field k acts on OWNED body i iff the body's position (its centre of mass, pos[i]) lies in the closed volume, that
 *   position is finite, and (category[i] & mask[k]) != 0 (the triggers' rule; category: phys_set_body_filters; a NULL mask
 *   array means every body and loads no filter). The test uses the centre, not the shape: PHYS_SHAPE_NONE bodies - the
 *   reference's own, and every body of a world without PHYS_FLAG_COLLISIONS - are affected too, and a fall-off with
 *   distance has one meaning.
 * Laws. Each field has a 3-vector vec, two coefficients coef[0..1] and an integer exponent:
 *   PHYS_FIELD_ACCEL   F += mass * vec. A true acceleration: a zero-gravity room (for unit masses vec = -gravity_force), a
 *                      directed well, a conveyor of air. (The global gravity stays the reference's: the same FORCE on
 *                      every body.)
 *   PHYS_FIELD_DRAG    F += -coef[0] * (v - vec), T += -coef[1] * w, with v, w the body's linear and angular velocity at the
 *                      start of the update and vec the medium's velocity (wind); coef[0], coef[1] >= 0. One field over the
 *                      whole scene is linear and angular damping.
 *   PHYS_FIELD_RADIAL  with d = x - c (c = the field's pos) and r = |d|:
 *                      F += coef[0] * (r0 / max(r, r0))^exponent * d / r, r0 = coef[1] > 0, exponent 0, 1 or 2 (by
 *                      multiplication, no pow). r == 0 gives nothing. coef[0] > 0 pushes outward (held for one update: an
 *                      impulse F * dt), coef[0] < 0 attracts; the magnitude never exceeds |coef[0]|.
 * Order. A body's sums start from its accumulators and take the contributions in ascending field index, each formed
 *   completely before it is added; all arithmetic is float32 in the operation order of include/spec/force_field.h (which a
 *   host compiler reads alone). A body's result depends on that body, the field set and the world state only: the same bits
 *   across runs, batch sizes and launch shapes. Accumulators of bodies no field acts on are not touched.
 * When. At the start of EVERY phys_update, and of each update of a phys_update_n batch, before the constraint phase (whose
 *   right-hand side reads the accumulators: a pinned body in a wind feels it) and the velocity half, from the poses and
 *   velocities the previous update left. phys_step alone applies none, as it applies no gravity; its companion is
 *   phys_apply_force_fields, the twin of phys_apply_gravity: it evaluates the fields now, into the accumulators, where
 *   phys_get_forces reads them and the next phys_step or phys_update consumes them (an update adds its own evaluation on
 *   top). A world without fields launches exactly what it launched before they existed.
 *
 * phys_set_force_fields: replaces the whole set; n = 0 clears it and frees its buffers. rot_ijkw NULL = identity, mask
 *   NULL = every body, exponent NULL = 0. PHYS_ERR_INVALID_ARG, the message naming the field and the reason: an unknown
 *   kind or shape, a non-finite number, a negative half extent, a negative drag coefficient, r0 <= 0, an exponent above 2;
 *   also n > PHYS_MAX_FORCE_FIELDS and a NULL array that is required. Synchronises the world's stream. The set names no body
 *   and survives phys_set_bodies.
 * phys_set_force_field_poses: new positions (and rotations; rot_ijkw NULL keeps them) for the set that is there, from the
 *   next evaluation on: a moving wind zone, an attractor carried by something. PHYS_ERR_INVALID_ARG: n differs from the
 *   field count, NULL pos, a non-finite value.
 * phys_set_force_field_params: new vec and coef for the set that is there (kinds, volumes and exponents stay), held to
 *   each field's law as above; a strength of 0 switches a field off without rebuilding the set. PHYS_ERR_INVALID_ARG: n
 *   differs from the field count, a NULL array, a value the law refuses.
 * Sharded worlds (phys_config.max_ghosts > 0) answer all four calls with PHYS_ERR_UNSUPPORTED, like the material calls.
 * Cost: one kernel per update, one lane per owned body, only in a world with fields; 12 bytes of position per body, 32 more
 *   with a DRAG field, 8 more with masks, and 48 of accumulators for the bodies a field acts on. DESIGN.md section 22.
 *   Added without an ABI version change (no struct changed): a library that predates them lacks the symbols. */
#define PHYS_MAX_FORCE_FIELDS 1024u
#define PHYS_FIELD_ACCEL  0u
#define PHYS_FIELD_DRAG   1u
#define PHYS_FIELD_RADIAL 2u

int32_t phys_set_force_fields(phys_world* w, uint64_t n, const uint32_t* kind /*n*/, const uint32_t* shape_type /*n*/,
                              const float* pos /*3n*/, const float* rot_ijkw /*4n, NULL = identity*/,
                              const float* half_extent /*3n*/, const uint16_t* mask /*n, NULL = every body*/,
                              const float* vec /*3n*/, const float* coef /*2n*/, const uint32_t* exponent /*n, NULL = 0*/);
int32_t phys_set_force_field_poses(phys_world* w, uint64_t n /* == field count */, const float* pos /*3n*/,
                                   const float* rot_ijkw /*4n, NULL = keep*/);
int32_t phys_set_force_field_params(phys_world* w, uint64_t n /* == field count */, const float* vec /*3n*/,
                                    const float* coef /*2n*/);
int32_t phys_apply_force_fields(phys_world* w);

/* --- liquids: buoyancy and drag from each body's submerged part (new: the reference has one global gravity) ---
 * A world keeps up to PHYS_MAX_LIQUIDS liquids. A force field looks at a body's centre; a liquid looks at its SHAPE against the
 * liquid's surface, reads its rotation and produces a torque: a crate floats at a water line and rights itself.
 * The volume. A liquid is an oriented box: pos, the unit quaternion rot_ijkw, half_extent h. Its SURFACE is the plane through
 *   the box's local +y face: unit normal n = column 1 of the rotation matrix, through pos + h.y * n. The liquid is the
 *   half-space below that plane. It is NOT clipped by the box's sides or bottom: the box only decides who is in the pool.
 * The law. Each liquid has density >= 0, gravity[3] (the acceleration the liquid is weighed by, e.g. (0, -9.81, 0);
 *   independent of n), flow[3] (the liquid's velocity), drag[2] >= 0 (linear, angular) and an optional mask.
 *   The world's own gravity stays the reference's FORCE, the same on every body whatever its mass or size. Whether a body
 *   floats is therefore the caller's arithmetic: it floats iff density * V_shape * |gravity| exceeds that force.
 * Who. Liquid k acts on OWNED body i iff the body has a shape (SPHERE, BOX or CAPSULE; PHYS_SHAPE_NONE bodies have no volume
 *   and are not touched), its position and rotation are finite, (category[i] & mask[k]) != 0 (a NULL mask array means every
 *   body and loads no filter), its centre is over the footprint and not under the bottom - with l = R^T (x - pos):
 *   |l.x| <= h.x, |l.z| <= h.z, l.y >= -h.y - and its submerged volume V_sub is above 0.
 * V_sub and M, the volume and the first moment about the body's centre of the part of the shape below the plane:
 *   sphere   exact (the cap's closed form);
 *   box      exact (six tetrahedra around a space diagonal, each clipped by the plane);
 *   capsule  a stated quadrature: 8 equal slabs of the cylinder and 4 per end cap across the axis, each cap slab a short
 *            cylinder of the radius that preserves its volume, each slab cut exactly by the plane. Within 0.5 % of the
 *            capsule's volume of the truth (0.46 % measured); a fully submerged capsule gives its volume exactly. Each slab's buoyancy acts at
 *            its axial midpoint ON the axis: the offset of a cut disc's centroid inside the disc is left out.
 *   Nothing divides by V_sub: the torque stays continuous as V_sub -> 0.
 * What it adds. With frac = min(V_sub / V_shape, 1), liquid k adds to body i
 *   F += -density * V_sub * gravity          T += -density * (M x gravity)
 *   F += -drag[0] * frac * (v - flow)        T += -drag[1] * frac * w
 *   with v, w the body's velocities as the previous update left them (loaded only when the set holds a nonzero drag).
 * Order. A body's sums start from its accumulators and take the contributions in ascending liquid index, each formed
 *   completely before it is added; all arithmetic is float32 in the operation order of include/spec/liquid.h (which a host
 *   compiler reads alone), no contraction: the same bits across runs, batch sizes and launch shapes. Accumulators of bodies
 *   no liquid acts on are not touched.
 * When. At the start of EVERY phys_update, and of each update of a phys_update_n batch, AFTER the force fields and before the
 *   constraint phase. phys_step alone applies none; its companion is phys_apply_liquids, the twin of
 *   phys_apply_force_fields. A world without liquids launches exactly what it launched before they existed.
 *
 * phys_set_liquids: replaces the whole set; n = 0 clears it and frees its buffers. rot_ijkw NULL = identity, mask NULL =
 *   every body. PHYS_ERR_INVALID_ARG, the message naming the FIRST offending liquid and its reason, in this order: a
 *   non-finite number, a negative half extent, a negative density, a negative drag coefficient; also n > PHYS_MAX_LIQUIDS and
 *   a NULL array that is required. Synchronises the world's stream. The set names no body and survives phys_set_bodies.
 * phys_set_liquid_poses: new positions (and rotations; rot_ijkw NULL keeps them) for the set that is there: a tide, a
 *   sloshing tank. PHYS_ERR_INVALID_ARG: n differs from the liquid count, NULL pos, a non-finite value.
 * phys_set_liquid_params: new density, gravity, flow and drag for the set that is there. PHYS_ERR_INVALID_ARG: n differs
 *   from the liquid count, a NULL array, a non-finite or negative value as above.
 * phys_get_submersion (host arrays; synchronises) and phys_get_submersion_device (device arrays; enqueued on the world's
 *   stream): evaluate now, with the same arithmetic, and write NOTHING to the accumulators. Per owned body: frac in the
 *   lowest-index liquid that acts on it and that liquid's index; 0 and 0xFFFFFFFF mean none. Either array may be NULL.
 * Sharded worlds (phys_config.max_ghosts > 0) answer every call with PHYS_ERR_UNSUPPORTED, like the force fields.
 * Cost: one kernel per update, one lane per owned body, only in a world with liquids; 44 bytes of pose and shape per body,
 *   32 more with drag, 8 more with masks, and 48 of accumulators for the bodies a liquid acts on. DESIGN.md section 29.
 *   Added without an ABI version change (no struct changed): a library that predates them lacks the symbols. */
#define PHYS_MAX_LIQUIDS 1024u

int32_t phys_set_liquids(phys_world* w, uint64_t n, const float* pos /*3n*/, const float* rot_ijkw /*4n, NULL = identity*/,
                         const float* half_extent /*3n*/, const uint16_t* mask /*n, NULL = every body*/,
                         const float* density /*n*/, const float* gravity /*3n*/, const float* flow /*3n*/,
                         const float* drag /*2n*/);
int32_t phys_set_liquid_poses(phys_world* w, uint64_t n /* == liquid count */, const float* pos /*3n*/,
                              const float* rot_ijkw /*4n, NULL = keep*/);
int32_t phys_set_liquid_params(phys_world* w, uint64_t n /* == liquid count */, const float* density /*n*/,
                               const float* gravity /*3n*/, const float* flow /*3n*/, const float* drag /*2n*/);
int32_t phys_apply_liquids(phys_world* w);
int32_t phys_get_submersion(phys_world* w, float* frac_out /*n_bodies*/, uint32_t* liquid_out /*n_bodies*/);
int32_t phys_get_submersion_device(phys_world* w, float* dev_frac_out /*n_bodies*/, uint32_t* dev_liquid_out /*n_bodies*/);

/* --- continuous collision: fast bodies stop at statics and the ground (new: the reference samples contacts at poses only) ---
 * An update finds contacts at the poses its bodies start from, within contact_margin. A body that moves further than a static
 * collider is thick in one update never overlaps it at a sampled pose and passes through; over the ground it is caught, but
 * metres deep. The bodies LISTED here are swept along each update's motion, and one that would pass through a static
 * collider or the ground is advanced only to its time of impact in that update.
 * The rule (include/spec/ccd.h states it as code), per listed body, between the solver and the position
 *   half of a collision update, from the pose at the start of the update and the velocity the solver left:
 *   - motion m = lin_velocity * dt, L = |m|. Not swept (frac = 1, target = PHYS_RAY_MISS): L not finite or not > 0, shape NONE,
 *     a non-finite pose. Otherwise the body translates along u = m / L without turning.
 *   - the body is a core box plus a radius: a box itself; a sphere a point plus its radius; a capsule a rod plus its radius.
 *   - targets: the ground (PHYS_FLAG_GROUND_PLANE) and every static collider that the body's collision filter collides with,
 *     by the rule of the contacts. Other bodies are NOT targets.
 *   - each target is tested with the box cast's arithmetic (include/spec/box_cast.h). A test that starts touching is no hit:
 *     the discrete contact owns that pair. A hit counts only when its distance t < L. The least (t, id) wins.
 *   - frac = min(t / L, 1) on a hit, else 1. The body is integrated for dt * frac, rotation too. Its velocity is left alone:
 *     it lands touching, inside contact_margin, and the next update's contact and the materials decide what happens.
 * Limits: the sweep does not turn (a spinning long box can clip a wall at landing; the next update's contact resolves it); the
 *   rest of the update after the impact, (1 - frac) dt, is dropped; bodies are no targets for each other; sharded worlds
 *   (max_ghosts > 0) have no continuous collision. It runs in collision updates only (PHYS_FLAG_COLLISIONS, dt > 0, not
 *   PHYS_FLAG_BROADPHASE_ONLY), phys_update_n included; phys_step never sweeps.
 * phys_set_ccd_bodies: replaces the list; n = 0 clears it and frees its buffers. Entry k is ids[k]: the order is kept and is the
 *   order of the read-out. It resets every frac to 1 and every count to 0. PHYS_ERR_UNSUPPORTED: a world without
 *   PHYS_FLAG_COLLISIONS or with max_ghosts > 0. PHYS_ERR_INVALID_ARG: NULL ids with n > 0, n >= 2^31, an id given twice.
 *   PHYS_ERR_OUT_OF_RANGE: an id not below the body count. A refused call leaves the old list in force. phys_set_bodies clears
 *   the list (its ids are stale); phys_set_static_bodies keeps it.
 * phys_get_ccd_hits (host arrays; synchronises) and phys_get_ccd_hits_device (device arrays; enqueued on the world's stream):
 *   per list entry, of the last update that swept: frac, the target's id (PHYS_RAY_MISS, PHYS_RAY_GROUND, PHYS_STATIC_ID_BIT | k),
 *   the normal from the target to the body (0 without a hit), and count: the updates in which the entry was stopped since the
 *   list was set (never zeroed in between, so a phys_update_n batch hides no hit). Any array may be NULL. Read-only.
 * Cost: one kernel per update, one lane per listed body, every static's box tested against the body's swept box and the
 *   survivors exactly; only in a world with a list. A world without one launches exactly what it launched before.
 *   Added without an ABI version change (no struct changed): a library that predates it lacks the symbols. */
int32_t phys_set_ccd_bodies(phys_world* w, uint64_t n, const uint32_t* ids /*n*/);
int32_t phys_get_ccd_hits(phys_world* w, float* frac_out /*n_ccd*/, uint32_t* target_out /*n_ccd*/, float* normal_out /*3 n_ccd*/,
                          uint32_t* count_out /*n_ccd*/);
int32_t phys_get_ccd_hits_device(phys_world* w, float* dev_frac_out /*n_ccd*/, uint32_t* dev_target_out /*n_ccd*/,
                                 float* dev_normal_out /*3 n_ccd*/, uint32_t* dev_count_out /*n_ccd*/);

/* --- in-place body edits: poses, velocities, impulses and forces by id list (new: the reference sets fields of one body) ---
 * phys_set_bodies replaces the whole set and resets filters, materials, warm starting, colours, events and trigger occupancy.
 * These calls change a few bodies and keep all of that: a jump, a hit, a respawn, a reset of one environment of many. `ids`
 * are body indices below phys_stats.n_bodies, n is the number of entries; masses, inertia and shapes stay with phys_set_bodies.
 * Order. An edit call behaves as if its entries were applied one after another in the order given; several entries may name
 *   one body. For the two set calls the last entry of a body wins; impulses and forces accumulate in entry order, bit for bit
 *   as if applied one at a time. phys_get_body_states takes ids in any order, with repeats.
 * Arithmetic (normative: include/spec/body_edit.h, float32, no contraction).
 *   impulse  r = point - x (zero without a point), L = ang_impulse + r x J, v = v + J * inv_mass, w = w + I^-1 L, with the
 *            body's inverse mass and inverse inertia as the integrator applies them. It acts at once: no dt, no accumulator.
 *   force    RigidBody::apply_force_at_position per entry (T += (point - x) x f, F += f; without a point F += f), then
 *            T += torque if given: a batch equals the same phys_apply_force_* calls bit for bit, in one launch. The
 *            accumulators are consumed by the next update or phys_step, as ever.
 *   velocity only v and w are rewritten; the masses stay.
 *   pose     pos and / or rot replaced (either may be NULL = keep). Rotations are stored as given, never renormalised.
 * What a pose edit keeps and drops. Warm-start impulses, colours, contact events and trigger occupancy are kept: a body
 *   teleported away raises END for its old pairs at the next update, one teleported into a trigger raises ENTER. The AABBs and
 *   grids of the last broad phase are dropped: phys_broadphase, phys_get_aabbs, the queries and the next update see the new
 *   poses, and phys_halo_pack / phys_halo_pairs ask for an update or phys_broadphase first.
 * When. Between updates and between phys_update_n batches; on the world's stream, behind what is already enqueued.
 * Host arrays (no suffix): checked before anything is written - PHYS_ERR_INVALID_ARG for a NULL ids or a NULL impulse / force
 *   with n > 0, n >= 2^31, or a non-finite value; PHYS_ERR_OUT_OF_RANGE for an id that is not below n_bodies. The entries are
 *   ordered by a stable sort on the id and staged; the call synchronises before it returns. n == 0 is a no-op.
 * Device arrays (_device): every pointer in device memory; the call only enqueues on the world's stream. The caller gives ids in
 *   NON-DECREASING order (a sort's output, or nonzero()'s). An entry whose id is out of range is skipped, nothing is written
 *   outside the arrays, and it or an entry with ids[i - 1] > ids[i] makes the next phys_sync return PHYS_ERR_INVALID_ARG, once,
 *   behind every other sticky error (phys_stats.overflow bit 8; the update's contact solve is NOT skipped). The other entries
 *   of that call are applied; the state of a body named by an out-of-order entry is unspecified.
 * A world with max_ghosts > 0 answers all ten calls with PHYS_ERR_UNSUPPORTED. Added without an ABI version change (no struct
 * changed): a library that predates them lacks the symbols. DESIGN.md section 24. */
int32_t phys_set_body_poses(phys_world* w, uint64_t n, const uint32_t* ids /*n*/, const float* pos /*3n or NULL*/,
                            const float* rot_ijkw /*4n or NULL*/);
int32_t phys_set_body_velocities(phys_world* w, uint64_t n, const uint32_t* ids /*n*/, const float* lin /*3n or NULL*/,
                                 const float* ang /*3n or NULL*/);
int32_t phys_apply_impulses(phys_world* w, uint64_t n, const uint32_t* ids /*n*/, const float* impulse /*3n*/,
                            const float* point /*3n world space, or NULL = centre*/, const float* ang_impulse /*3n or NULL*/);
int32_t phys_apply_forces(phys_world* w, uint64_t n, const uint32_t* ids /*n*/, const float* force /*3n*/,
                          const float* point /*3n world space, or NULL = centre*/, const float* torque /*3n or NULL*/);
int32_t phys_get_body_states(phys_world* w, uint64_t n, const uint32_t* ids /*n*/, float* pos_out /*3n*/, float* rot_out /*4n*/,
                             float* lin_out /*3n*/, float* ang_out /*3n; each output may be NULL*/);
int32_t phys_set_body_poses_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* pos, const float* rot_ijkw);
int32_t phys_set_body_velocities_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* lin, const float* ang);
int32_t phys_apply_impulses_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* impulse, const float* point,
                                   const float* ang_impulse);
int32_t phys_apply_forces_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* force, const float* point,
                                 const float* torque);
int32_t phys_get_body_states_device(phys_world* w, uint64_t n, const uint32_t* ids, float* pos_out, float* rot_out, float* lin_out,
                                    float* ang_out);

/* --- per-stage device timing (HIP events on the world's stream), for bench.py's roofline --- */
#define PHYS_STAGE_STEP_FULL 0u     /* gravity + RigidBody::step, one kernel (no collisions) */
#define PHYS_STAGE_VELOCITY_AABB 1u /* gravity + velocity half + AABB */
#define PHYS_STAGE_GRID 2u          /* cell assign, scan, scatter */
#define PHYS_STAGE_PAIRS 3u         /* k_find_pairs (+ the (body, static) pairs of worlds with static colliders) */
#define PHYS_STAGE_NARROW 4u        /* k_narrowphase */
#define PHYS_STAGE_COLOR 5u         /* colouring rounds */
#define PHYS_STAGE_ROWS 6u          /* colour-major renumbering + solver_prep */
#define PHYS_STAGE_SOLVE 7u         /* k_solve_color */
#define PHYS_STAGE_POSITION 8u      /* position half */
#define PHYS_STAGE_CONSTRAINTS 9u   /* constraint assembly + CG (A3-A7) */
#define PHYS_STAGE_MISC 10u         /* memsets, halo */
#define PHYS_STAGE_SOLVE_TAIL 11u   /* k_solve_tail: the small colours of one iteration in one workgroup */
#define PHYS_STAGE_SOLVE_FLOW 12u   /* k_solve_flow: all iterations and colours in one launch */
#define PHYS_STAGE_SOLVE_CLUSTER 13u /* k_solve_cluster: one launch, body velocities resident in LDS per spatial cluster */
#define PHYS_STAGE_COUNT 14u
typedef struct phys_profile {
    double ms[PHYS_STAGE_COUNT];         /* summed device time per stage since enable */
    uint64_t launches[PHYS_STAGE_COUNT]; /* kernel launches (memsets included) per stage */
    uint64_t steps;                      /* updates profiled */
} phys_profile;
/* on != 0: bracket every launch with events (slower; never inside a timed region). Resets the sums. */
int32_t phys_profile_enable(phys_world* w, int32_t on);
int32_t phys_profile_get(phys_world* w, phys_profile* out);

/* --- device-side access for zero-copy callers (torch / RCCL plumbing) and multi-GPU halos --- */
typedef struct phys_device_view {
    uint64_t n;
    float* pos;     /* 3n */
    float* rot;     /* 4n */
    float* lin_vel; /* 3 floats per body at a stride of vel_stride floats */
    float* ang_vel; /* 3 floats per body at a stride of vel_stride floats */
    float* aabb;    /* 6n: min xyz max xyz, valid after an update with COLLISIONS or phys_broadphase */
    void* stream;   /* hipStream_t the world launches on */
    uint64_t vel_stride; /* = 8: velocities live in 32-byte records {v.xyz, 1/m, w.xyz, m} */
} phys_device_view;
int32_t phys_get_device_view(phys_world* w, phys_device_view* out);

/* Sharded broad-phase, AABB records only (config C4). Each rank owns the bodies it was given; a halo
 * record is 32 B: {min xyz, max xyz, global id, pad}. phys_halo_pack writes to DEVICE memory the records of
 * owned bodies whose fattened AABB reaches outside [x_lo + reach, x_hi - reach] and returns the count;
 * reach must be >= the largest AABB edge on ANY rank (all-reduce phys_stats.max_extent), reach <= 0
 * means this rank's own grid cell. A record may be any number of the receiving rank's grid cells wide (the cell is
 * that rank's own largest extent, not the all-reduced one): phys_halo_pairs tests it against the owned bodies of every
 * cell it covers. Both calls use the AABBs / grid of the last update or phys_broadphase.
 * phys_halo_pack first fills the whole buffer with 0xFF (empty slot = global id 0xFFFFFFFF). phys_halo_pairs
 * ignores records [skip_first, skip_first + skip_count): the caller's own block of an all-gathered buffer.
 * With n_records / n_cross_pairs == NULL both calls only ENQUEUE work on the world's stream and return
 * (no host synchronisation; phys_get_stats reports the counts later): the per-step exchange then costs no
 * host round trip when the collective is enqueued on the same stream (phys_device_view.stream). With a pointer they
 * return PHYS_ERR_CAPACITY when THIS call's records / pairs did not fit (cap, or max(4 n_bodies, 4096) cross pairs;
 * what fitted is written, nothing behind the capacity is): the same call with enough room succeeds right after. The
 * overflow also stays in phys_stats.overflow bit 3 until phys_sync reports it. phys_halo_pairs takes the gathered records of the OTHER ranks (device
 * memory) and appends owned-vs-remote candidate pairs (local index, global id of the remote body)
 * under the ownership rule "emitted by the rank owning the body with the smaller global id". */
int32_t phys_set_global_ids(phys_world* w, const uint32_t* global_ids /*n*/);
int32_t phys_halo_pack(phys_world* w, float x_lo, float x_hi, float reach, void* dev_records_out, uint64_t cap,
                       uint64_t* n_records);
int32_t phys_halo_pairs(phys_world* w, const void* dev_remote_records, uint64_t n_remote, uint64_t skip_first,
                        uint64_t skip_count, uint64_t* n_cross_pairs);
int32_t phys_get_cross_pairs(phys_world* w, uint32_t* pairs_out /*2*cap*/, uint64_t cap, uint64_t* n_pairs);

/* Sharded worlds with contacts across the cut planes (SURVEY §8 rows E + N4; no reference counterpart: the reference is
 * one thread on one CPU). A world created with phys_config.max_ghosts > 0 keeps max_ghosts GHOST slots behind its owned
 * bodies. Before every update the ranks exchange the full state of their boundary bodies - a 96-byte record {pos, rot,
 * lin vel, ang vel, half extent, shape, global id, inverse mass, inverse inertia diagonal} of every owned body within
 * `reach` of a slab face - and every rank places the neighbours' records that lie within `reach` of ITS slab into its
 * ghost slots. A ghost is a DYNAMIC body of the receiving world for the length of one update: its owner's mass and
 * inertia, this update's gravity, contacts with the ground, with other ghosts and with owned bodies. A contact between an
 * owned body and a body across the plane is therefore solved as the two-body contact it is, on BOTH sides of the plane
 * from the same state, and each side keeps its own body's half of the outcome (what the update did to the ghost is
 * forgotten at the next exchange): for an isolated pair the two halves are equal and opposite up to float rounding
 * (momentum across the plane conserved to ~1e-6), in a pile each side also sees its body's other contacts, which the
 * neighbour sees only as far as its ghosts reach - the N-rank run approximates the single-world run, it does not
 * reproduce its bits. (Round 2 placed ghosts as KINEMATIC bodies - an impact on a ghost was an impact on a moving wall,
 * 2 m v instead of the two-body impulse; a body whose world-frame inertia tensor is not diagonal still crosses that way:
 * the record holds a diagonal.) Slot order is a function of the records alone (both compactions are prefix sums, not
 * atomics), so a sharded run repeats bit for bit.
 *   phys_set_slab            this rank's x-interval and the reach (>= the largest bounding diameter + margin on any rank)
 *   phys_halo_pack_bodies    owned boundary bodies -> 96-byte records in DEVICE memory (unused slots: global id 0xFFFFFFFF)
 *   phys_halo_unpack_ghosts  gathered records (device) -> ghost slots; [skip_first, skip_first+skip_count) = own block
 *   phys_get_global_ids      global ids of the owned bodies followed by those of the ghost slots (0xFFFFFFFF = empty);
 *                            manifold ids >= phys_stats.n_bodies name ghost slots
 * All three device calls only enqueue on the world's stream. */
#define PHYS_HALO_BODY_RECORD_BYTES 96u
int32_t phys_set_slab(phys_world* w, float x_lo, float x_hi, float reach);
int32_t phys_halo_pack_bodies(phys_world* w, void* dev_records_out, uint64_t cap);
/* the bodies within reach of ONE slab face only: face < 0 the low face (what rank r - 1 may need), face > 0 the high
 * face (rank r + 1), 0 both (= phys_halo_pack_bodies). What a neighbour exchange sends (phys_comm_set_neighbours). */
int32_t phys_halo_pack_bodies_face(phys_world* w, void* dev_records_out, uint64_t cap, int32_t face);
int32_t phys_halo_unpack_ghosts(phys_world* w, const void* dev_records, uint64_t n_records, uint64_t skip_first,
                                uint64_t skip_count);
int32_t phys_get_global_ids(phys_world* w, uint32_t* out /* n_bodies + max_ghosts */);

/* The exchange itself behind the C ABI: RCCL (librccl.so, loaded on first use; PHYS_RCCL_PATH overrides the search) over
 * xGMI, one communicator rank per world / GPU, every call enqueued on the world's own stream - a Rust or C++ host shards
 * without Python. Message shape: ONE ncclAllGather of a fixed-size block per rank (latency-bound: no count exchange).
 *   phys_comm_unique_id   rank 0 makes the 128-byte id and ships it to the other ranks by any means
 *   phys_comm_create      ncclCommInitRank on the world's device; `capacity` = records per rank and step
 *   phys_comm_create_local  ONE process driving n worlds on n different devices: ncclCommInitAll (+ phys_halo_exchange_all)
 *   phys_halo_exchange    max_ghosts > 0:  pack bodies -> all-gather -> unpack ghosts   (call BEFORE phys_update)
 *                         otherwise:       pack AABBs  -> all-gather -> cross pairs     (call AFTER phys_update; C4) */
#define PHYS_COMM_ID_BYTES 128u
typedef struct phys_comm phys_comm;
int32_t phys_comm_unique_id(uint8_t id_out[PHYS_COMM_ID_BYTES]);
int32_t phys_comm_create(phys_world* w, const uint8_t id[PHYS_COMM_ID_BYTES], int32_t rank, int32_t n_ranks, uint64_t capacity,
                         phys_comm** out);
int32_t phys_comm_create_local(phys_world** worlds, int32_t n, uint64_t capacity, phys_comm** comms_out /*n*/);
int32_t phys_comm_destroy(phys_comm* c);
/* enable != 0: the ranks are x-slabs ORDERED BY RANK and none is thinner than the reach, so only ranks r - 1 and r + 1 can
 * hold bodies near this rank's faces: the exchange becomes one grouped ncclSend / ncclRecv pair per neighbour (direct xGMI
 * links, two blocks to scan) instead of an all-gather of every rank's block. Every rank of the communicator must choose
 * the same. Default: all-gather (right for any partition). */
int32_t phys_comm_set_neighbours(phys_comm* c, int32_t enable);
int32_t phys_halo_exchange(phys_world* w, phys_comm* c);
/* the n collectives of a step as ONE group: required when one thread drives the comms of phys_comm_create_local */
int32_t phys_halo_exchange_all(phys_world** worlds, phys_comm** comms, int32_t n);

/* Slab partition (host arithmetic only, no device, no communication: the caller sums the histograms of the ranks with
 * whatever transport it has - RCCL, MPI, a pipe). Equal-count cut planes along x, SURVEY §8 row E: histogram of body x
 * over `bins` equal bins of [x_min, x_max] -> prefix sums -> n_ranks + 1 cut planes (cuts[0] = -inf side = x_min,
 * cuts[n_ranks] = x_max; interior planes at bin boundaries... interpolated inside the bin that crosses k/n_ranks of the
 * bodies) -> owner of every body (the rank r with cuts[r] <= x < cuts[r+1]; bodies outside [x_min, x_max] go to the
 * first / last rank). Re-cut every k steps and hand a body that changed owner over to its new rank. */
int32_t phys_slab_histogram(const float* pos /*3n*/, uint64_t n, float x_min, float x_max, uint32_t bins,
                            uint64_t* hist /*bins, added to*/);
int32_t phys_slab_cuts(const uint64_t* hist /*bins, summed over ranks*/, uint32_t bins, float x_min, float x_max, int32_t n_ranks,
                       float* cuts_out /*n_ranks + 1*/);
int32_t phys_slab_owners(const float* pos /*3n*/, uint64_t n, const float* cuts /*n_ranks + 1*/, int32_t n_ranks,
                         int32_t* owner_out /*n*/);

#ifdef __cplusplus
}
#endif
#endif /* PHYSICS_HIP_H */
