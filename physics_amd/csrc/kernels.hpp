// kernels.hpp — shared includes and the host-side launch interface between the translation units
// of libphysics_hip.so. Every launch_* enqueues on w->stream and returns without synchronising.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <hip/hip_runtime.h>

#include "../../include/spec/collide.h"
#include "../../include/spec/contact_solve.h"
#include "../../include/spec/det_math.h"
#include "../../include/spec/vec.h"
#include "world.hpp"
#include "readout.hpp"
#include "records.hpp"
#include "staging.hpp"
#include "wave.hpp"

static_assert(PHYS_MAX_COLORS == phys::kMaxColors, "colour limit mismatch");
static_assert(PHYS_COLOR_CACHE_PERIOD == phys::kColorCachePeriod, "colour table period mismatch");

#define PHYS_PROF_CAT2(a, b) a##b
#define PHYS_PROF_CAT(a, b) PHYS_PROF_CAT2(a, b)
#define PHYS_PROF(w, st) phys::ProfScope PHYS_PROF_CAT(_prof_scope_, __LINE__)((w)->prof, (w)->stream, (st))

namespace phys {

// f(std::true_type{}) or f(std::false_type{}): a launch site names each instantiation of a kernel template once
template <class F>
inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// More than the default 64 KiB of dynamic LDS needs the function attribute: once per kernel AND DEVICE (function attributes
// are per device: a world on a second device of this process needs its own), the current device being the world's (ENTER of
// the ABI call). `done`: the launch site's own per-device flags. A refusal is returned, not left behind as the thread's error.
inline hipError_t allow_dynamic_lds(bool (&done)[64], int device, std::initializer_list<const void*> kernels, int bytes) {
    if (done[device & 63]) return hipSuccess;
    for (const void* f : kernels) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    }
    done[device & 63] = true;
    return hipSuccess;
}

// 12-byte packed attribute access as ONE dwordx3 memory instruction per lane (a wave then covers one
// contiguous 768-B span). Written as three scalar accesses hipcc emits three dword instructions, each
// touching every line of the span again.
struct alignas(4) packed3 { float x, y, z; };
__device__ __forceinline__ v3 ld3(const float* __restrict__ p, uint32_t i) {
    const packed3 t = reinterpret_cast<const packed3*>(p)[i];
    return v3_make(t.x, t.y, t.z);
}
__device__ __forceinline__ void st3(float* __restrict__ p, uint32_t i, v3 v) {
    packed3 t; t.x = v.x; t.y = v.y; t.z = v.z;
    reinterpret_cast<packed3*>(p)[i] = t;
}

// Velocity record of one body: 32 bytes {v.xyz, inv_mass, w.xyz, mass} = two dwordx4 accesses and ONE
// 32-byte sector per gather (the solver gathers it by body id 8 x colours times per step), instead of pieces
// of three separate arrays. lin_velocity / angular_velocity of the reference (rigid_body.rs:9-10) are the
// first three floats of each half.
struct BodyVel { v3 v; float inv_mass; v3 w; float mass; };
__device__ __forceinline__ BodyVel ld_vel(const float* __restrict__ vel, uint32_t i) {
    const float4 a = reinterpret_cast<const float4*>(vel)[2 * (size_t)i];
    const float4 b = reinterpret_cast<const float4*>(vel)[2 * (size_t)i + 1];
    BodyVel r;
    r.v = v3_make(a.x, a.y, a.z); r.inv_mass = a.w;
    r.w = v3_make(b.x, b.y, b.z); r.mass = b.w;
    return r;
}
__device__ __forceinline__ void st_vel(float* __restrict__ vel, uint32_t i, const BodyVel& r) {
    reinterpret_cast<float4*>(vel)[2 * (size_t)i] = make_float4(r.v.x, r.v.y, r.v.z, r.inv_mass);
    reinterpret_cast<float4*>(vel)[2 * (size_t)i + 1] = make_float4(r.w.x, r.w.y, r.w.z, r.mass);
}

// inverse inertia of one body. DIAG: every body's tensor is diagonal (the reference's only case: identity,
// rigid_body.rs:71), stored as one float4 per body = 16 B and one sector per gather instead of 36 B / two.
// The zero off-diagonals are put back, so the arithmetic is the general path's (only signed zeros can differ).
template <bool DIAG>
__device__ __forceinline__ m33 ld_inertia(const float* __restrict__ p, uint32_t i) {
    m33 M;
    if (DIAG) {
        const float4 d = reinterpret_cast<const float4*>(p)[i];
#pragma unroll
        for (int k = 0; k < 9; ++k) M.m[k] = 0.0f;
        M.m[0] = d.x; M.m[4] = d.y; M.m[8] = d.z;
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) M.m[k] = p[9 * (size_t)i + k];
    }
    return M;
}

// Persistent colouring: ONE hash table (a << 32 | b) -> {colour, update stamp} that lives across updates. Open addressing,
// linear probing, 16-byte entries {key, value word (records.hpp: stamp, manifold index, colour)} (the index of the pair's manifold in
// the update that stamped the entry: what the next update warm-starts from); at least 1.5 slots per manifold SLOT.
//   * the narrow phase of update E looks every manifold up: an exact key match whose stamp is E - 1 ("was there in the
//     previous update") keeps its colour and is re-stamped E on the spot - one 8-byte store to the line the probe has
//     just read. Entries that are not re-stamped are dead from then on.
//   * k_rows_build inserts only the manifolds that were NEW in this update (a few per cent of a steady pile), into the
//     first slot of their chain that is not live: claimed by a 64-bit CAS on the VALUE word (stamp becomes E), key stored
//     after. A slot stamped E is nobody else's business, whatever key it shows, so a half-written claim is never
//     taken for a match; pairs are unique within an update, so nobody looks for a key stamped E.
//   * a key's live entry is always the first entry of that key in its chain (a dead one before it would have been
//     reused by the insert), chains never shrink (slots go back to empty only in the reset), so a probe may stop at the
//     first empty slot or the first entry with its key.
//   * every PHYS_COLOR_CACHE_PERIOD-th update the table is REBUILT: emptied by one memset behind the narrow phase (which has
//     taken the kept colours from it by then) and refilled by k_rows_build with every manifold of that update. No colour
//     changes; the dead entries of the period are gone.
// Round 1-2a rebuilt a table per update inside k_rows_build (an atomic and two scattered stores per manifold, plus the
// sparse clear of the other table): 0.26 of k_rows_build's 0.50 ms on C5. The layout depends on arrival order, the
// answers (exact key + stamp matches) do not.
constexpr uint32_t kColorTableMaxWalk = 4096;  // slots a look-up may walk before it gives up (a full table must not hang a wave)
struct ColorTableJob {
    ulonglong2* tab;  // null: nothing to do
    uint32_t mask;
    uint32_t stamp;   // of the update whose manifolds are being inserted
    uint32_t all;     // != 0: table rebuild - the manifolds that kept their colour are inserted too
    const uint32_t* man_color; const uint64_t* man_prio;
};

__device__ __forceinline__ void color_table_insert(const ColorTableJob& job, uint32_t a, uint32_t b, uint32_t m, StepCounters* ctr) {
    const unsigned long long key = ((unsigned long long)a << 32) | b;
    const unsigned long long val = table_value_encode(job.stamp, m, table_color_field(job.man_color[m]));
    uint32_t h = (uint32_t)(job.man_prio[m] >> 20) & job.mask;
    // bounded (see the walk in k_narrowphase); a manifold that finds no slot would be coloured afresh next time where the
    // oracle keeps its colour: the update is flagged (bit 6), never a silent divergence
    for (uint32_t walked = 0; ; ++walked) {
        if (walked == 4u * kColorTableMaxWalk) { flag_overflow(ctr, kOvfColorTable); return; }
        unsigned long long* vp = &job.tab[h].y;
        const unsigned long long seen = __hip_atomic_load(vp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (table_value_stamp(seen) != job.stamp && atomicCAS(vp, seen, val) == seen) {
            job.tab[h].x = key;
            return;
        }
        if (table_value_stamp(__hip_atomic_load(vp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == job.stamp) h = (h + 1) & job.mask;
        // else: somebody else's CAS on a dead slot failed too, or the value changed under us - look at the slot again
    }
}

// ---- collision filters -------------------------------------------------------------------------
// A filter is {category | mask << 16, (uint32_t)(int32_t)group}: one 8-byte load per body or static. The defaults
// (category 0x0001, mask 0xFFFF, group 0) let everything collide. Two filters collide unless the rule says otherwise:
// the same nonzero group decides by its sign, anything else needs each category in the other's mask.
// (kFilterDefaultWord: setup.hpp)
__host__ __device__ __forceinline__ bool filter_pass(uint2 fa, uint2 fb) {
    if (fa.y == fb.y && fa.y != 0u) return (int32_t)fa.y > 0;
    return (fa.x & (fb.x >> 16)) != 0u && (fb.x & (fa.x >> 16)) != 0u;
}
// the narrow phase's filters (k_narrowphase<..., kFilters = true>)
struct NpFilters {
    const uint2* body;  // per body slot
    const uint2* st;    // per static collider (null without statics)
    uint2 ground;       // {category | mask << 16, 0}
};
// a query's filters (the _filtered query calls): a target is seen iff its category meets the query's mask
struct QueryFilters {
    const uint16_t* query_mask;  // one per query
    const uint2* body;           // per owned body
    const uint2* st;             // per static collider
    uint32_t ground;             // the ground's category
};
// ... of world `w`, for the queries whose masks are the device array query_mask
inline QueryFilters query_filters(const phys_world* w, const uint16_t* query_mask) {
    return {query_mask, reinterpret_cast<const uint2*>(w->filt.p), reinterpret_cast<const uint2*>(w->st_filt.p), w->ground_filt & 0xFFFFu};
}
// the one filter argument of a filtered kernel instance. The filter arguments travel as a parameter pack that is empty in
// the unfiltered instance, so that instance keeps the kernel arguments - and with them the offsets of the hidden
// arguments it reads - and compiles to the instructions it had before filters.
template <typename T>
__device__ __forceinline__ T filter_arg(T f) { return f; }
// what a capsule cast adds to the arguments of the cast kernel (k_rc_trace): in the same pack, in front of the filters, so
// that the ray and ball instances keep their arguments and their instructions
struct CapsuleArgs {
    const float* rot;          // [i, j, k, w] per query; null: identity
    const float* half_length;  // per query
    float* point_out;          // 3 per query; null: not wanted
};

// ---- materials ---------------------------------------------------------------------------------
// One {friction, restitution} per body slot and per static collider: one 8-byte load per side of a manifold, made by
// k_rows_build alone. The ground's material and the restitution threshold are kernel arguments.
struct RowMaterials {
    const float2* body;  // per body slot
    const float2* st;    // per static collider (null without statics)
    float2 ground;
    float threshold;     // approach speed below which nothing bounces
};
// the one material argument of k_rows_build's material instance (a parameter pack that is empty in the plain one: see filter_arg)
template <typename T>
__device__ __forceinline__ T material_arg(T m) { return m; }
// a material call was made since the reset of what it set: the solver runs its material instances
inline bool materials_active(const phys_world* w) { return w->body_materials_set || w->static_materials_set || w->ground_mat_set; }

// ---- uniform grid of the broad phase: cell -> bucket -----------------------------------------------------------------
// The table has 2^bits buckets, bits = bx + by + bz split over the axes in proportion to the scene's extent (a tower 16
// cells wide and 980 high gets x 4, y 10, z 5 instead of 7 + 7 + 7: with equal bits its 128-cell axis wrapped 7.6 times
// and every bucket held the bodies of eight different cells). Cell coordinates are taken modulo the axis size (far
// bodies alias; aliased candidates fail the overlap test, and neighbouring cells never alias: every axis has >= 4 cells).
// Buckets are numbered BRICK-major: a brick is 4 x 4 x 4 cells = 64 consecutive buckets (the low two bits of each
// coordinate interleaved), bricks x-fastest. So the bodies of a brick are one contiguous run of the bucket-sorted
// arrays, which is what lets one workgroup stage a brick and its half-shell halo in LDS (k_find_pairs_brick).
// (struct GridShape: setup.hpp)
__host__ __device__ __forceinline__ uint32_t grid_bucket_masked(uint32_t x, uint32_t y, uint32_t z, const GridShape& g) {
    const uint32_t brick = ((((z >> 2) << g.sy) | (y >> 2)) << g.sx) | (x >> 2);
    const uint32_t local = (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2) | ((x & 2u) << 2) | ((y & 2u) << 3) | ((z & 2u) << 4);
    return (brick << 6) | local;
}
__host__ __device__ __forceinline__ uint32_t grid_bucket(int cx, int cy, int cz, const GridShape& g) {
    return grid_bucket_masked((uint32_t)cx & g.mx, (uint32_t)cy & g.my, (uint32_t)cz & g.mz, g);
}
__device__ __forceinline__ int grid_cell_coord(float c, float inv_cell) {
    float t = floorf(c * inv_cell);
    t = t < -1.0e9f ? -1.0e9f : (t > 1.0e9f ? 1.0e9f : t);
    return (int)t;
}

// Cluster solver: which cluster's workgroup owns a row. A body has a HOME cluster (cluster_slot / slots) or none (ghost
// bodies of a sharded world; bodies beyond the capacity of a dynamic clustering). A row is owned by the home of its
// body A, else by the home of its body B, else - both homeless - by a cluster picked from A's id. A side whose body's
// home is the owner is served from that workgroup's LDS; every other side is "another cluster's body".
constexpr uint32_t kNoHome = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t cluster_home(const uint32_t* __restrict__ cluster_slot, uint32_t body, uint32_t slots) {
    const uint32_t s = cluster_slot[body];
    return s == kNoHome ? kNoHome : s / slots;
}
__device__ __forceinline__ uint32_t cluster_row_owner(uint32_t a, uint32_t home_a, uint32_t home_b, uint32_t clusters) {
    if (home_a != kNoHome) return home_a;
    if (home_b != kNoHome) return home_b;
    return ((a * 2654435761u) >> 7) % clusters;
}

// the step counters into the pinned host mirror w->h_counters, and wait: the one copy-and-wait of every read-out call
inline int32_t fetch_counters(phys_world* w) {
    PHYS_HIP_TRY(hipMemcpyAsync(w->h_counters, w->counters.p, sizeof(StepCounters), hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

// The one drain of phys_get_contact_events and phys_get_trigger_events (the rules: readout.hpp drain_rules). cursor_dev: the
// 64-bit count of events raised since the last drain; buf_dev: the first `capacity` of them. Only the cursor word is cleared,
// ordered on the world's stream in front of the next update's kernels.
template <class Record>
int32_t drain_events(phys_world* w, void* cursor_dev, uint64_t capacity, const void* buf_dev, Record* out, uint64_t cap, uint64_t* n,
                     uint64_t* n_dropped, const char* too_many) {
    unsigned long long cursor = 0;
    PHYS_HIP_TRY(hipMemcpyAsync(&cursor, cursor_dev, sizeof(cursor), hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    const EventDrain d = drain_rules(cursor, capacity, out != nullptr, cap);
    *n = d.stored;
    if (n_dropped) *n_dropped = d.dropped;
    if (d.count_only) return PHYS_OK;  // the buffer stays
    if (d.too_many) return fail(PHYS_ERR_CAPACITY, too_many);
    if (d.stored) {
        PHYS_HIP_TRY(hipMemcpyAsync(out, buf_dev, d.stored * sizeof(Record), hipMemcpyDeviceToHost, w->stream));
        PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
        // device order is arbitrary; a read-out convenience as in phys_get_manifolds
        std::sort(out, out + d.stored, [](const Record& x, const Record& y) { return event_before(x, y); });
    }
    if (d.clear_cursor) PHYS_HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(cursor), w->stream));
    return PHYS_OK;
}

// integrate.hip
void launch_step_full(phys_world* w, float dt, bool gravity, bool constraints = false);  // constraints: entity 0 += J^T lambda of this update
void launch_step_velocity_aabb(phys_world* w, float dt, bool gravity, bool zero_step, bool constraints = false);  // zero_step: also zero the per-step state
void launch_aabb_only(phys_world* w);
void launch_step_position(phys_world* w, float dt, bool ccd = false);  // ccd: this update's sweep ran (ccd.hip): dt * ccd_frac per body
void launch_apply_gravity(phys_world* w);
void launch_apply_force_one(phys_world* w, uint32_t body, int mode, const float f[3], const float arg[3]);
void launch_instance_matrices(phys_world* w, float* d_out);

// broadphase.hip
int32_t collision_alloc(phys_world* w);  // buffers for setup.hpp collision_sizes; the table of grid_plan is set before
void zero_step_state(phys_world* w, bool including_extent);  // ONE memset: counters + bucket counts + colouring state
void launch_broadphase(phys_world* w, const PairPlan& plan);
void build_sorted_grid(phys_world* w);  // bucket_start / sorted_ids / sorted_box from the current AABBs (bucket counts zeroed)
int32_t sorted_pairs_to_host(phys_world* w, uint32_t* pairs_out, uint64_t cap, uint64_t* n_pairs);

// narrowphase.hip / coloring.hip / solver.hip
void launch_narrowphase(phys_world* w, const NarrowPlan& plan);
// `cluster`: this update's rows go in (cluster, colour) order. On the Probe path the stage synchronises and adopts the exact
// counters as the first hint (abi.hip hint_adopt), so what follows it is planned from those.
void launch_coloring(phys_world* w, const ColorPlan& plan, bool cluster);
// `full`: the update is a full re-colouring (its round count is remembered as that)
void snapshot_counters_async(phys_world* w, bool full);  // abi.hip
StepCounters* snapshot_acquire(phys_world* w);  // abi.hip: pinned slot a kernel may fill itself ...
void snapshot_commit(phys_world* w, bool full);  // ... then mark it in flight
void poll_snapshots(phys_world* w);           // abi.hip
// The one adoption of counters as the hint (abi.hip). `full`: they are a full re-colouring's. `exact`: read by the update that
// waited for them (the Probe path), not a snapshot of an earlier one.
void hint_adopt(StepHint& hint, const StepCounters& c, bool full, bool exact);
// `table`: the colouring stage's job for k_rows_build - this update's manifolds go into the colour table (ColorPlan: stamp, rebuild)
void launch_solver(phys_world* w, float dt, const SolverPlan& plan, const ColorPlan& table);
// contact events (events.hip): two kernels behind the solve, only in a world with events on
void launch_events(phys_world* w, uint32_t step, uint32_t blocks /* plan_event_blocks */);
int32_t events_alloc(phys_world* w);  // buffers for the current event and manifold capacities (frees them when events are off)
int32_t events_reset(phys_world* w);  // forget the contact history and the pending events (a new body or static set)

// Host-built records (setup.hpp trigger_records, field_records) to `dst`, on the world's stream - behind the updates already
// enqueued - and waited for: the host vector may change as soon as the call returns.
template <typename R>
int32_t upload_records(phys_world* w, DevBuf<float>& dst, const std::vector<R>& rec) {
    PHYS_HIP_TRY(dst.resize(sizeof(R) / sizeof(float) * rec.size()));
    PHYS_HIP_TRY(hipMemcpyAsync(dst.p, rec.data(), sizeof(R) * rec.size(), hipMemcpyHostToDevice, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

// trigger volumes (trigger.hip): one kernel behind the position step of every update, only in a world with triggers
void launch_triggers(phys_world* w, uint32_t step);
// the set from its staged form (setup.hpp stage_triggers; arguments checked by the caller; empty: clears and frees); forgets the occupancy
int32_t triggers_set(phys_world* w, TriggerStaging&& staged);
int32_t triggers_rebuild(phys_world* w);  // w->tg_host was patched (poses): build the records again and send them; keeps the occupancy
int32_t triggers_reset(phys_world* w);  // forget the occupancy and the pending events (a new trigger or body set)

// force fields (fields.hip): one kernel in front of every update, only in a world with fields; it adds to the force / torque
// accumulators and marks them dirty, so the step kernels' FORCES instances read and zero them
void launch_force_fields(phys_world* w);
// the set from its staged form (setup.hpp stage_fields; arguments checked by the caller; empty: clears and frees)
int32_t fields_set(phys_world* w, FieldStaging&& staged);
int32_t fields_rebuild(phys_world* w);  // w->ff_host was patched (poses, params): build the records again and send them

// liquids (liquid.hip): one kernel in front of every update, behind the fields', only in a world with liquids; it adds to the
// force / torque accumulators and marks them dirty, as the fields' does
void launch_liquids(phys_world* w);
// frac and liquid index per owned body into device arrays (either may be null), on the world's stream; writes no accumulator
void launch_submersion(phys_world* w, float* d_frac, uint32_t* d_liquid);
// the set from its staged form (setup.hpp stage_liquids; arguments checked by the caller; empty: clears and frees)
int32_t liquids_set(phys_world* w, LiquidStaging&& staged);
int32_t liquids_rebuild(phys_world* w);  // w->lq_host was patched (poses, params): build the records again and send them

// continuous collision (ccd.hip): one kernel between the solver and the position half of every collision
// update, only in a world with a list; it writes the share of dt of every listed body into ccd_frac, which that update's
// position half then reads (launch_step_position(.., ccd = true))
void launch_ccd_sweep(phys_world* w, float dt);
// the list from its staged form (setup.hpp stage_ccd; checked by the caller; empty: clears and frees); frac to 1, counts to 0
int32_t ccd_set(phys_world* w, std::vector<uint32_t>&& ids);
// the read-out of the last sweep into arrays of n_ccd entries (each may be null; host or device ones), on the world's stream
int32_t ccd_read(phys_world* w, float* frac, uint32_t* target, float* normal, uint32_t* count, bool to_host);

// in-place body edits (edit.hip): one batch on device arrays ordered by id (EditKind, EditBatch and the
// argument checks: setup.hpp), enqueued on the world's stream; a pose edit drops the AABBs and grids kept from the last broad
// phase, a force edit marks the accumulators dirty. Nothing is launched in a world that never calls them.
int32_t launch_edit(phys_world* w, EditKind kind, const EditBatch& b);
// the states of the bodies ids[0 .. n) into device arrays (each may be null), ids in any order
int32_t launch_get_states(phys_world* w, uint64_t n, const uint32_t* ids, float* pos_out, float* rot_out, float* lin_out, float* ang_out);

// constraints.hip
int32_t constraints_alloc(phys_world* w);
void launch_constraint_phase(phys_world* w, bool gravity_pending);  // Q = accumulators (+ gravity when still pending)

// halo.hip
int32_t halo_pack(phys_world* w, float x_lo, float x_hi, float reach, void* dev_out, uint64_t cap, uint64_t* n_records);
int32_t halo_pairs(phys_world* w, const void* dev_remote, uint64_t n_remote, uint64_t skip_first, uint64_t skip_count,
                   uint64_t* n_cross);

// cluster.hip
int32_t cluster_assign(phys_world* w, const float* host_pos);
void launch_cluster_sort(phys_world* w, const ColorPlan& plan, StepCounters* snap_out /* host-mapped slot for the counters, or null */);
#ifdef __HIPCC__
// the step counters copied out to a host-mapped slot by the first workgroup of a kernel that runs after their last writer
__device__ __forceinline__ void counters_snapshot(const StepCounters* ctr, StepCounters* snap_out) {
    if (snap_out && blockIdx.x == 0) {
        constexpr uint32_t words = (uint32_t)(sizeof(StepCounters) / 4);
        for (uint32_t k = threadIdx.x; k < words; k += blockDim.x)
            reinterpret_cast<uint32_t*>(snap_out)[k] =
                __hip_atomic_load(reinterpret_cast<const uint32_t*>(ctr) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif
// scan.hip: exclusive scan of `count` (a multiple of 4) counters into out[count + 1], on the world's stream. scratch:
// scan_scratch_words(count) words of the caller's (unused by the one-launch scan)
void launch_exclusive_scan(phys_world* w, uint32_t* in, uint32_t count, uint32_t* out, bool zero_in, uint32_t* scratch,
                           uint32_t* block_used = nullptr /* as many words again: non-zero counters per block ... */,
                           StepCounters* ctr = nullptr /* ... summed into n_used_buckets */, int prof_stage = -1);
bool scan_is_one_launch(uint32_t count);  // ... in which case zero_in leaves the counters zeroed behind the scan
size_t scan_scratch_words(uint32_t count);
// cluster.hip: clusters / slots of this update (setup.hpp plan_dynamic_clusters) while the dealt homes last; false: no cluster step in this update
bool cluster_plan_dynamic(phys_world* w, const StepHint& h, const DebugSwitches& dbg);
void launch_solve_cluster(phys_world* w, const SolverPlan& plan, void* row_all, uint64_t cap, float friction, const float* inertia,
                          uint32_t stride, bool diag);

// static.hip: the static set (arguments checked by the caller), the per-update (body, static) pairs, and what k_narrowphase
// takes of them (cap 0 / null pointers: no static colliders)
int32_t static_set(phys_world* w, uint64_t n, const float* pos, const float* rot, const uint32_t* shape, const float* half_extent);
int32_t launch_static_pairs(phys_world* w);
void static_narrow_args(const phys_world* w, uint64_t* cap, const uint32_t** pairs, const float** geo);

// The query families' launchers, one overload per batch (staging.hpp; device pointers, arguments checked by the caller), all on
// w->stream: each builds the query grid once from the current poses, then runs ONE kernel with a query per lane. A query_mask
// makes it the filtered instance.
// raycast.hip: the casts. Ray: radius unused. Sphere: balls of radius[i], the grid grown by the largest valid radius. Capsule
// (DESIGN.md section 23): core origin +- half_length * (rot's y axis), radius[i], the grid grown by the largest valid radius +
// half_length; rot and point_out are read for this kind alone.
// Box goes to boxcast.hip's launch_boxcast: the box of rot and half_extent[i], the grid grown by the largest
// valid |half_extent|; radius and half_length are not read.
int32_t launch_query(phys_world* w, CastKind kind, const CastBatch& b);
int32_t launch_boxcast(phys_world* w, const CastBatch& b);
// boxcast.hip: enqueues the reduction of the n device half extents (3 each) into the query grid's grow slot (launch_query_grid calls
// it where k_sc_grow runs for the other sweeps)
void launch_box_grow(phys_world* w, const float* half_extent, uint64_t n);
// slide.hip: move-and-slide: the grid grown as for a capsule cast; every lane runs its character's whole
// cast, stop, project loop (include/spec/slide.h) against the capsule cast's own walk
int32_t launch_query(phys_world* w, const SlideBatch& b);
// character.hip: character walking: the grid grown as for a capsule cast; every lane drives its character's
// state machine (include/spec/character.h) around the capsule cast's own walk
int32_t launch_query(phys_world* w, const CharacterBatch& b);
// depen.hip: depenetration: the grid not grown; every lane probes for its capsule's deepest target (b.probe:
// that is the answer) and runs the push-out loop of include/spec/depenetrate.h, probing again from where each push left it
int32_t launch_query(phys_world* w, const DepenBatch& b);
// the query grid alone (rc_header, rc_start, rc_records), every body AABB grown by the largest valid value of the n_grow
// values of the device array grow_radius (null: not grown), plus grow_half_length's of the same query where that is given (a
// capsule reaches radius + half_length from its centre); *bits = log2 of the bucket table (rc_grid.hpp query_grid: the same
// with everything a query kernel takes of the world in one struct). grow_half_extent (a box cast's, 3 per query): grown by the
// largest valid |half_extent| instead.
int32_t launch_query_grid(phys_world* w, const float* grow_radius, const float* grow_half_length, uint64_t n_grow, uint32_t* bits,
                          const float* grow_half_extent = nullptr);
// query.hip: overlap queries on staged device arrays; writes the host offsets (n + 1) and, when they fit in cap, the ids
int32_t launch_overlap(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot, const float* half_extent,
                       const uint32_t* ignore_body, uint64_t cap, uint64_t* offsets_out, uint32_t* ids_out,
                       const uint16_t* query_mask = nullptr /* device, n; null: no filtering */);

int32_t halo_pack_bodies(phys_world* w, void* dev_out, uint64_t cap);
int32_t halo_pack_bodies_faces(phys_world* w, void* dev_out, uint64_t cap, float x_lo, float x_hi);
int32_t halo_unpack_ghosts(phys_world* w, const void* dev_records, uint64_t n_records, uint64_t skip_first, uint64_t skip_count);

}  // namespace phys
