// world.hpp — device-resident state of one phys_world (MI355X / gfx950).
//
// Layout in HBM: structure-of-arrays, one array per body attribute, so a wave reading attribute k of
// bodies [64w, 64w+64) touches one contiguous span (3-float attributes: 768 B per wave, quaternions:
// 1 KiB as dwordx4). Everything stays resident across steps; the host only sees what it asks for.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "../../include/physics_hip.h"
#include "plan.hpp"
#include "setup.hpp"

namespace phys {

void set_error(const std::string& msg);
const char* get_error();

#define PHYS_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            phys::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                     \
            return PHYS_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)
// ... and for a call of the library's own that answers a PHYS_* code (which has set the error text)
#define PHYS_TRY(expr)                                                                              \
    do {                                                                                            \
        const int32_t _rc = (expr);                                                                 \
        if (_rc != PHYS_OK) return _rc;                                                             \
    } while (0)

// host side of every extern "C" entry point: the error text and the code it returns with ...
inline int32_t fail(int32_t code, const char* msg) {
    set_error(msg);
    return code;
}
// ... and its first line: a world, and its device current
#define ENTER(w)                                                                    \
    do {                                                                            \
        if (!(w)) return phys::fail(PHYS_ERR_INVALID_ARG, "null world");            \
        PHYS_HIP_TRY(hipSetDevice((w)->device));                                    \
    } while (0)

// A device allocation and its owner: freed by the destructor, never copied. A view (point_at) is a non-owning window into
// another DevBuf's allocation (the per-step zeroed block, the solver's row planes) and frees nothing.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    bool view = false;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { free(); }
    // at least `count` elements; an allocation that is large enough stays (a view never does: it is dropped first)
    hipError_t resize(size_t count) {
        if (count <= n && p && !view) return hipSuccess;
        free();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void free() {
        if (p && !view) (void)hipFree(p);
        p = nullptr;
        n = 0;
        view = false;
    }
    void point_at(T* ptr, size_t count) { free(); p = ptr; n = count; view = true; }
};

// (struct StepCounters and its kOvf* bits: setup.hpp)
// raise overflow bits: this step's word (the solver kernels of the step look at it) and the sticky one
__device__ __forceinline__ void flag_overflow(StepCounters* ctr, uint32_t bits) {
    atomicOr(&ctr->overflow, bits);
    atomicOr(&ctr->sticky_overflow, bits);
}

// per-stage device timing with HIP events on the world's stream (phys_profile_enable)
struct Profiler {
    bool on = false;
    std::vector<hipEvent_t> ev;      // pairs: [2k] start, [2k+1] stop
    std::vector<uint32_t> stage;     // stage of pair k
    size_t used = 0;                 // pairs in flight
    double ms[PHYS_STAGE_COUNT] = {};
    uint64_t launches[PHYS_STAGE_COUNT] = {};
    uint64_t steps = 0;
    void begin(hipStream_t s, uint32_t st) {
        if (2 * used + 2 > ev.size()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            ev.push_back(a); ev.push_back(b); stage.push_back(0);
        }
        stage[used] = st;
        (void)hipEventRecord(ev[2 * used], s);
    }
    void end(hipStream_t s) { (void)hipEventRecord(ev[2 * used + 1], s); ++used; }
    void collect(hipStream_t s) {  // the stream must be idle or is synchronised here
        if (!used) return;
        (void)hipStreamSynchronize(s);
        for (size_t k = 0; k < used; ++k) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) == hipSuccess) { ms[stage[k]] += t; launches[stage[k]] += 1; }
        }
        used = 0;
    }
    void reset() { for (auto& m : ms) m = 0; for (auto& l : launches) l = 0; steps = 0; used = 0; }
    void destroy() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); stage.clear(); used = 0; }
};

struct ProfScope {
    Profiler& p; hipStream_t s;
    ProfScope(Profiler& p_, hipStream_t s_, uint32_t st) : p(p_), s(s_) { if (p.on) p.begin(s, st); }
    ~ProfScope() { if (p.on) p.end(s); }
};

// worlds alive per device in this process (abi.hip): two of them step on two streams, i.e. beside each other
int worlds_on_device(int device);
// PHYS_FLAG_EXCLUSIVE_GPU, no PHYS_FLAG_SHARED_GPU, no other world on the device: asked afresh for every update's plan (abi.hip)
bool gpu_is_exclusive(const phys_world* w);
// PHYS_DEBUG_* switches (plan.hpp DebugSwitches), parsed once per process by the first call (abi.hip)
const DebugSwitches& debug_switches();

}  // namespace phys

struct phys_world {
    // the whole teardown (abi.hip): stream drained, then events, pinned memory and the stream; every DevBuf below frees itself
    // behind it, so a buffer added here needs no second mention anywhere
    ~phys_world();
    phys_config cfg;
    int device = 0;
    int cus = 0;  // its CU count (phys_create)
    hipStream_t stream = nullptr;
    uint64_t n = 0;        // body slots the kernels run over = n_owned + max_ghosts
    uint64_t n_owned = 0;  // bodies of phys_set_bodies: every host-facing size and index check
    uint64_t max_ghosts = 0;
    float slab_lo = -3.0e38f, slab_hi = 3.0e38f, slab_reach = 0.0f;  // phys_set_slab
    phys::DevBuf<uint32_t> halo_block_counts;  // per-workgroup counts of the two ordered compactions (pack / unpack)
    uint64_t steps = 0;
    bool forces_dirty = false;      // force / torque arrays hold non-zero accumulators
    bool singular_inertia = false;  // some body's inertia tensor has det == 0 (reference panics in step)
    bool all_diag_inertia = true;
    bool uniform_inertia = true;  // all diagonal AND identical for every body
    bool body_capsules = false;   // some owned body is a PHYS_SHAPE_CAPSULE (phys_set_bodies): the narrow phase's capsule variant
    bool aabbs_valid = false;
    bool grid_valid = false;  // bucket grid + AABBs of the last broad phase are on the device (halo entry points)

    // body SoA
    phys::DevBuf<float> pos, rot, vel /* 8n: v.xyz inv_mass w.xyz mass */, force, torque, inv_inertia, inv_inertia_diag /* 4n, valid when all_diag_inertia */, half_extent, aabb;
    phys::DevBuf<uint32_t> shape;
    phys::DevBuf<uint32_t> global_id;
    // what the narrow phase needs of a body, in ONE 64-byte line: {pos.xyz, shape} {rot ijkw} {half extent xyz, lowest y of
    // the fattened AABB}; written once per update by k_step_velocity_aabb (which has it all in registers), gathered twice
    // per candidate pair - instead of four 4-to-16-byte gathers per body out of four arrays (C5: 3M pairs per update)
    phys::DevBuf<float> geo;  // 16 floats per body (48 bytes used)
    // collision filters: one {category | mask << 16, (u32)group} per body slot, owned and ghost (2n
    // words; the defaults after phys_set_bodies, ghost slots reset by k_ghost_clear and written by k_halo_unpack)
    phys::DevBuf<uint32_t> filt;
    bool body_filters_set = false;    // phys_set_body_filters since the last phys_set_bodies: the narrow phase's filtered variant
    bool static_filters_set = false;  // phys_set_static_filters since the last phys_set_static_bodies
    bool ground_filter_set = false;   // phys_set_ground_filter ever (the ground filter lasts for the life of the world)
    uint32_t ground_filt = 0xFFFF0001u;  // the ground's category | mask << 16 (its group is 0)
    // materials: one {friction, restitution} per body slot (2n floats; {cfg.friction, 0} after
    // phys_set_bodies) and per static (after phys_set_static_bodies); read by k_rows_build's material instance only
    phys::DevBuf<float> mat, st_mat;
    bool body_materials_set = false;    // phys_set_body_materials since the last phys_set_bodies
    bool static_materials_set = false;  // phys_set_static_materials since the last phys_set_static_bodies
    bool ground_mat_set = false;        // phys_set_ground_material ever (it lasts for the life of the world)
    float ground_mat[2] = {0.0f, 0.0f}; // {friction, restitution}, valid when ground_mat_set (cfg.friction, 0 otherwise)
    float restitution_threshold = 1.0f; // phys_set_restitution_threshold

    // constraints (A3-A7)
    std::vector<phys::Constraint> constraints;
    phys::DevBuf<phys::Constraint> d_constraints;
    bool constraints_dirty = false;
    phys::DevBuf<float> cg_x, cg_r, cg_p, cg_ap, cg_rhs, cg_c, cg_scratch;
    phys::DevBuf<float> cg_jl;         // J^T lambda of entity 0 (6 floats), added by the step kernel behind gravity (quirk Q3)
    phys::DevBuf<uint32_t> cg_status;  // [0] converged flag, [1] iterations, [2] previous_solution.is_some()
    phys::DevBuf<uint32_t> cg_cols;    // col_id | col_ptr | col_rows | row_cidx (constraints.hip)
    uint32_t cg_n_cols = 0;

    // collision pipeline (A10-A12)
    uint64_t max_pairs = 0, max_manifolds = 0;
    uint32_t grid_table_size = 0;  // hashed-grid buckets (power of two)
    phys::GridShape grid_shape{};  // its split over the three axes (setup.hpp grid_plan)
    // counters, bucket_count and color_state are windows into ONE allocation (step_zero) laid out
    // [bucket counts | colouring state | StepCounters], so one memset per step zeroes all three (up to, not
    // including, StepCounters::max_extent_bits at the very end)
    phys::DevBuf<uint8_t> step_zero;
    size_t step_zero_reset_bytes = 0, step_zero_full_bytes = 0;
    phys::DevBuf<phys::StepCounters> counters;
    phys::DevBuf<uint32_t> bucket_of;    // n
    phys::DevBuf<uint32_t> bucket_count, bucket_start, bucket_cursor;  // table
    phys::DevBuf<uint32_t> slot_ids;     // 4 per bucket: the slot grid of small scenes (no scan, no scatter)
    phys::DevBuf<float> slot_box;        // the AABB next to every id slot (6 floats)
    phys::DevBuf<uint32_t> grid_ovf;     // n: bodies beyond the fourth of their bucket
    bool sorted_grid_valid = false;      // bucket_start / sorted_ids / sorted_box describe the last broad phase
    phys::DevBuf<uint32_t> sorted_ids;   // n: body ids grouped by bucket
    phys::DevBuf<float> sorted_box;      // 6n: AABBs in bucket order (streamed by the pair kernel)
    phys::DevBuf<uint32_t> scan_block_sums;
    phys::DevBuf<uint32_t> pairs;        // 2 * max_pairs
    // manifolds, geometry stage (storage order = emission order, arbitrary)
    phys::DevBuf<uint32_t> man_a, man_b, man_color;  // SoA: what the colouring rounds and the row sort scan again and again
    // geometry of a manifold as ONE 128-byte record = one cache line (32 floats: {a, b, count, -} {normal, -} 4 x {point,
    // depth}, 32 bytes spare): k_rows_build reads it through the row permutation, and seven scattered 4-to-64-byte
    // accesses per row had cost it 896 bytes of line fetches for 88 useful ones
    phys::DevBuf<float> man_geo;
    // warm starting (contact_solve.h): the geometry records of the PREVIOUS update (the two buffers swap every update), the
    // accumulated impulses every manifold's solve ended with (12 floats = three float4 per manifold: {pn, pt0, pt1} x 4
    // points, packed; this update's / the previous one's), and per manifold of this update the index of the same pair's
    // manifold in the previous update (from the colour table's value word; ~0: none)
    phys::DevBuf<float> man_geo_prev, man_imp, man_imp_prev;
    phys::DevBuf<uint32_t> man_prev;
    bool warm = false;  // warm starting is on for this world (not PHYS_FLAG_NO_WARM_START, manifold indices fit the table's 26 bits)
    phys::DevBuf<uint64_t> man_prio;
    // persistent colouring: two hash tables (this update's / the previous update's), key -> colour
    phys::DevBuf<uint32_t> unc_list;  // 2 x max_manifolds: ids of the manifolds uncoloured at the start of a round (ping-pong)
    phys::DevBuf<uint64_t> ctab;  // persistent colour table: 2 words per slot {key, stamp << 32 | colour} (kernels.hpp)
    uint32_t ctab_mask = 0;     // capacity - 1 (power of two >= 1.5 * max_manifolds)
    bool ctab_valid = false;    // a table of the previous update exists
    uint64_t color_epoch = 0;   // updates with collisions since phys_set_bodies
    phys::DevBuf<uint32_t> color_block_hist;  // [colour][workgroup] histogram / offsets of the colour sort
    // colouring state
    phys::DevBuf<unsigned long long> color_state;  // 4n: used masks | three rotating per-body priority buffers
    // solver rows, colour-major, plane-major arrays of 16-byte elements (layout: records.hpp)
    phys::DevBuf<uint32_t> row_src;  // row -> manifold (the colour sort)
    // ONE allocation of 16 planes of cap float4 each (the two plane numberings: records.hpp), so a kernel can address
    // plane p of row d as all[p * cap + d] without choosing a pointer
    phys::DevBuf<float> row_all;
    // single-launch solvers: in-flight body velocities travel between workgroups as tagged granules (handoff.hpp)
    phys::DevBuf<float> flow_vel;    // kBodyGranuleBytes per body: {v.xyz, tag} {w.xyz, tag}; null = per-colour launches only
    // cluster solver (cluster.hip): spatial clusters fixed at phys_set_bodies, rows sorted by (cluster, colour) per step
    uint32_t cluster_count = 0, cluster_slots = 0;  // 0 clusters: not available for this scene (dynamic: set per update)
    bool cluster_dynamic = false;           // clusters are remade every update from the bodies that have manifolds (cluster.hip)
    uint32_t cluster_age = 0;               // cluster steps since the homes were dealt out (dynamic: remade every kClusterDynamicPeriod)
    bool cluster_homes_valid = false;
    phys::DevBuf<uint32_t> active_flag, active_rank;  // n + 4 each: flag / exclusive rank in the broad phase's bucket order
    phys::DevBuf<uint32_t> cluster_slot;   // body -> cluster * slots + slot
    phys::DevBuf<uint32_t> cluster_body;   // cluster * slots + slot -> body (0xFFFFFFFF: empty)
    phys::DevBuf<uint32_t> body_shared;    // 2 per body: 64-bit mask of the colours in which ANOTHER cluster's row updates it
    bool seg_count_dirty = false;    // the (cluster, colour) counters were left non-zero by the last cluster step (three-launch scan)
    uint32_t seg_count_bins = 0;     // ... which used this many of them
    phys::DevBuf<uint32_t> seg_start;      // exclusive scan of the rows per (cluster, colour), which are counted behind body_shared
    phys::DevBuf<uint32_t> man_rank;       // manifold -> arrival rank inside its segment
    uint32_t flow_epoch = 0;         // solves since the buffers were cleared (upper half of every tag)
    // ray-cast query (raycast.hip): its own grid, rebuilt from the current poses by every call; nothing an update reads
    phys::DevBuf<uint32_t> rc_header;    // scene bounds and largest AABB edge (order-preserving keys)
    phys::DevBuf<uint32_t> rc_count;     // insertions per bucket (left zeroed by the scatter)
    phys::DevBuf<uint32_t> rc_start;     // table + 1: exclusive scan of rc_count
    phys::DevBuf<uint32_t> rc_tile_sum;  // the scan's own scratch (scan_block_sums is the update's)
    phys::DevBuf<float> rc_records;      // 8N records of 48 bytes {centre, shape} {rot} {half extent, id}, bucket order
    // the queries on host arrays (the casts, move-and-slide, character walking, depenetration, phys_overlap): ONE staging buffer
    // for the inputs of whichever runs - each synchronises the stream before it returns, so no two are ever in flight - laid out
    // by the call's own declarations (staging.hpp StageLayout); the outputs the same way, the three buffers being the groups of
    // staging.hpp: inputs, per-query outputs, phys_character_move's hit slots
    phys::DevBuf<uint8_t> stage, rc_out, rc_slots;
    phys::DevBuf<unsigned long long> rc_stats;  // PHYS_DEBUG_RAYCAST_STATS: cells, candidates
    // overlap queries (query.hip): they walk the grid above; their own output
    phys::DevBuf<uint32_t> qr_count;     // phys_overlap: targets per query (count pass)
    phys::DevBuf<unsigned long long> qr_off;  // ... their exclusive scan (n + 1)
    phys::DevBuf<uint32_t> qr_ids;       // ... the ids in walk order, then each query's ids ascending
    // static colliders (static.hip): immovable shapes set by phys_set_static_bodies, read-only until the next such call
    uint64_t n_static = 0;
    bool static_capsules = false;        // some static is a PHYS_SHAPE_CAPSULE: the narrow phase's capsule variant
    phys::DevBuf<float> st_geo;          // 16 floats per static, the layout of `geo`: {pos, shape} {rot} {half extent, -}
    phys::DevBuf<float> st_rc;           // 12 floats per static, the ray-cast record {pos, shape} {rot} {half extent, id}
    phys::DevBuf<uint32_t> st_filt;      // 2 words per static: its filter, the layout of `filt` (defaults after phys_set_static_bodies)
    phys::DevBuf<float> st_box;          // 8 floats per static: {fattened AABB lo, packed first grid cell} {hi, -}
    phys::DevBuf<uint32_t> st_cell_start, st_cell_ids;  // uniform grid over the small statics, CSR: cell -> ascending ids
    phys::DevBuf<uint32_t> st_large;     // statics that would cover too many cells: tested by every body, ascending
    uint32_t st_n_large = 0;
    float st_org[3] = {0.0f, 0.0f, 0.0f}, st_inv_cell = 0.0f;
    uint32_t st_dim[3] = {0, 0, 0};      // cells per axis (0: no small statics), each <= 1024
    phys::DevBuf<uint32_t> st_count;     // per body slot: its static pairs (count pass), then their offsets
    phys::DevBuf<uint32_t> st_block;     // per workgroup of the count pass: pair totals, then their exclusive scan
    phys::DevBuf<uint32_t> st_pairs;     // 2 per pair: body, static index (not tagged), (body, static) ascending
    uint64_t max_static_pairs = 0;       // automatic: a per-body budget, regrown from the counts of earlier updates
    uint64_t static_pairs_seen = 0;      // the largest pair count an update has reported back (sizes the buffer)
    bool static_pairs_sized = false;     // the next update measures its pair count first (new static or body set)
    // contact events (events.hip): off unless phys_contact_events_enable gave a capacity
    uint64_t ev_capacity = 0;            // events the device keeps between two drains (0: off, nothing below is allocated)
    phys::DevBuf<uint32_t> ev_buf;       // 12 words = one phys_contact_event per slot
    phys::DevBuf<uint32_t> ev_matched;   // per manifold slot of the previous update: the stamp of the update that found its pair again
    phys::DevBuf<uint32_t> ev_state;     // 4 words: the 64-bit event cursor and the manifold counts of the last two updates (events.hip EventState)
    uint32_t ev_stamp = 0;               // updates with events so far (never 0 once one ran; wrap: launch_events)
    uint32_t ev_parity = 0;              // which of the two count words the next update writes
    // trigger volumes (trigger.hip): nothing below is allocated, and nothing launched, without triggers
    uint64_t n_triggers = 0;
    bool tg_masked = false;              // phys_set_triggers was given a mask array: the evaluation's filtered instance
    std::vector<phys::TriggerVolume> tg_host;  // the set as staged (setup.hpp stage_triggers): poses are patched here, the records built from it
    phys::DevBuf<float> tg_rec;          // 24 floats per trigger: the record the evaluation reads (include/spec/volume.h vol_record)
    phys::DevBuf<uint32_t> tg_bits;      // occupancy, plane-major: word (k / 32) of body i at [(k / 32) * n_owned + i], bit k % 32
    uint64_t tg_bits_bodies = 0;         // the n_owned tg_bits was laid out for
    uint64_t tg_capacity = 0;            // trigger events the device keeps between two drains (0: off)
    phys::DevBuf<uint32_t> tg_buf;       // 4 words = one phys_trigger_event per slot
    phys::DevBuf<unsigned long long> tg_cursor;  // trigger events raised since the last drain (allocated with the triggers or the events)
    // force fields (fields.hip): nothing below is allocated, and nothing launched, without fields
    uint64_t n_fields = 0;
    bool ff_masked = false;              // phys_set_force_fields was given a mask array: the evaluation's filtered instance
    bool ff_drag = false, ff_accel = false;  // some field is a DRAG (the velocity record is read) / an ACCEL (the mass is)
    std::vector<ff_staged> ff_host;      // the set as staged (setup.hpp stage_fields): poses and params are patched here, the records built from it
    phys::DevBuf<float> ff_rec;          // 28 floats per field: the record the evaluation reads (include/spec/force_field.h ff_record)
    // liquids (liquid.hip): nothing below is allocated, and nothing launched, without liquids
    uint64_t n_liquids = 0;
    bool lq_masked = false;              // phys_set_liquids was given a mask array: the evaluation's filtered instance
    bool lq_drag = false;                // some liquid has a nonzero drag: the velocity record is read
    std::vector<lq_staged> lq_host;      // the set as staged (setup.hpp stage_liquids): poses and params are patched here, the records built from it
    phys::DevBuf<float> lq_rec;          // 32 floats per liquid: the record the evaluation reads (include/spec/liquid.h lq_record)
    // continuous collision (ccd.hip): nothing below is allocated, and nothing launched, without a list
    uint64_t n_ccd = 0;                  // entries of phys_set_ccd_bodies
    phys::DevBuf<uint32_t> ccd_ids;      // n_ccd: entry -> body, in the caller's order
    phys::DevBuf<float> ccd_frac;        // n_owned: the share of dt each body is advanced by (1 for every body not stopped); the position half reads it
    phys::DevBuf<uint32_t> ccd_hit;      // 5 n_ccd words, the read-out of the last sweep: frac | target | normal (3 per entry)
    phys::DevBuf<uint32_t> ccd_count;    // n_ccd: updates in which the entry was stopped, since the list was set
    // multi-GPU halo
    phys::DevBuf<uint32_t> cross_pairs;
    uint64_t max_cross_pairs = 0;

    phys::StepHint hint;
    static constexpr int kSnapRing = 4;
    phys::StepCounters* h_snap[kSnapRing] = {};  // pinned snapshots of the counters
    hipEvent_t snap_event[kSnapRing] = {};
    bool snap_pending[kSnapRing] = {};
    bool snap_full[kSnapRing] = {};
    uint32_t snap_next = 0;
    phys::Profiler prof;
    uint32_t host_sticky_overflow = 0;  // overflow bits seen in counter snapshots (poll_snapshots), until phys_sync
    // pinned host mirror of the counters for read-back
    phys::StepCounters* h_counters = nullptr;
};
