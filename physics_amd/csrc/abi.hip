// abi.hip — the extern "C" surface of libphysics_hip.so (include/physics_hip.h). Host code only:
// argument checking, uploads, and the per-frame launch sequence. All compute is in HIP kernels; there
// is no CPU fallback anywhere in this library.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace phys {
static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* get_error() { return g_error.c_str(); }
}  // namespace phys

using namespace phys;

namespace phys {
void poll_snapshots(phys_world* w);
// Launch-size hints: snapshots of the step counters in a ring of pinned host slots. A slot is filled either by
// an asynchronous copy (snapshot_counters_async) or by a kernel writing the host-mapped slot itself
// (snapshot_acquire -> kernel -> snapshot_commit); an event behind it tells poll_snapshots when it is complete.
StepCounters* snapshot_acquire(phys_world* w) {
    const uint32_t k = w->snap_next;
    if (w->snap_pending[k]) {
        // ring full: the host is kSnapRing steps ahead of the device. Wait for the oldest sample, so the
        // launch-size hints never lag by more than the ring depth.
        (void)hipEventSynchronize(w->snap_event[k]);
        poll_snapshots(w);
    }
    if (!w->h_snap[k]) {
        if (hipHostMalloc((void**)&w->h_snap[k], sizeof(StepCounters), hipHostMallocDefault) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&w->snap_event[k], hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    return w->h_snap[k];
}
void snapshot_commit(phys_world* w, bool full) {
    const uint32_t k = w->snap_next;
    (void)hipEventRecord(w->snap_event[k], w->stream);
    w->snap_pending[k] = true;
    w->snap_full[k] = full;  // was this update a full re-colouring?
    w->snap_next = (k + 1) % phys_world::kSnapRing;
}
void snapshot_counters_async(phys_world* w, bool full) {
    StepCounters* slot = snapshot_acquire(w);
    if (!slot) return;
    (void)hipMemcpyAsync(slot, w->counters.p, sizeof(StepCounters), hipMemcpyDeviceToHost, w->stream);
    snapshot_commit(w, full);
}

// Counters become the hint. The colouring rounds: a full re-colouring and an incremental update need very different counts,
// and the incremental count fluctuates, so the full count is remembered by itself, and of the incremental ones the maximum
// over a ring of the last eight snapshots (with it, the most new manifolds of one update). The two callers differ in the
// ring: poll_snapshots pushes every incremental snapshot into it; the Probe path of launch_coloring (`exact`: hint invalid,
// the update has just waited for its own counters) writes color_rounds alone and leaves the ring and n_new as they are. That
// is the behaviour both had as separate copies and it is kept: an exact incremental count only arises when no snapshot has
// been adopted since phys_set_bodies (an update that overflowed leaves a colour table but no hint), the ring is empty then,
// and the next incremental snapshot replaces the count by the ring's maximum - so the exact count serves the updates in
// between and never enters the maximum.
void hint_adopt(StepHint& hint, const StepCounters& c, bool full, bool exact) {
    hint.valid = true;
    hint.n_manifolds = c.n_manifolds;
    hint.n_pairs = c.n_pairs;
    hint.n_contacts = c.n_contacts;
    if (c.max_region) hint.max_region = c.max_region;
    hint.n_used_buckets = c.n_used_buckets;
    hint.n_colors = c.n_colors;
    if (c.n_active) hint.n_active = c.n_active;  // counted only in the updates that deal out the dynamic homes
    if (full) {
        hint.full_rounds = c.color_rounds;
    } else if (exact) {
        hint.color_rounds = c.color_rounds;
    } else {
        hint.recent_new[hint.recent_pos % 8] = c.n_new_manifolds;
        hint.recent_rounds[hint.recent_pos++ % 8] = c.color_rounds;
        uint32_t mx = 0, mn = 0;
        for (int q = 0; q < 8; ++q) {
            mx = hint.recent_rounds[q] > mx ? hint.recent_rounds[q] : mx;
            mn = hint.recent_new[q] > mn ? hint.recent_new[q] : mn;
        }
        hint.color_rounds = mx;
        hint.n_new = mn;
    }
    for (int q = 0; q < kMaxColors; ++q) hint.color_count[q] = c.color_count[q];
}

// adopt every snapshot whose copy has completed (oldest first, so the newest complete one wins)
void poll_snapshots(phys_world* w) {
    for (int i = 0; i < phys_world::kSnapRing; ++i) {
        const uint32_t k = (w->snap_next + i) % phys_world::kSnapRing;
        if (!w->snap_pending[k]) continue;
        if (hipEventQuery(w->snap_event[k]) != hipSuccess) {
            (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure: do not leave it behind as the
            continue;                 // thread's sticky error for whoever calls HIP next (the host application)
        }
        const StepCounters& c = *w->h_snap[k];
        w->snap_pending[k] = false;
        w->host_sticky_overflow |= c.overflow | c.sticky_overflow;  // latched until phys_sync reports it
        if (c.n_static_pairs > w->static_pairs_seen) w->static_pairs_seen = c.n_static_pairs;  // sizes the static pairs (static.hip)
        if (c.overflow) continue;
        hint_adopt(w->hint, c, w->snap_full[k], /*exact=*/false);
    }
}
}  // namespace phys

namespace phys {
static std::atomic<int> g_worlds[64];
int worlds_on_device(int device) { return g_worlds[device & 63].load(std::memory_order_relaxed); }
bool gpu_is_exclusive(const phys_world* w) {
    return (w->cfg.flags & PHYS_FLAG_EXCLUSIVE_GPU) && !(w->cfg.flags & PHYS_FLAG_SHARED_GPU) && worlds_on_device(w->device) == 1;
}

// what the plan reads of the world (plan.hpp), as the world stands now
static PlanInputs plan_inputs(const phys_world* w) {
    PlanInputs in;
    in.flags = w->cfg.flags; in.solver_iterations = w->cfg.solver_iterations;
    in.n = w->n; in.n_owned = w->n_owned; in.max_manifolds = w->max_manifolds;
    in.grid_table_size = w->grid_table_size;
    in.cus = w->cus;
    in.exclusive = gpu_is_exclusive(w);
    in.warm = w->warm;
    in.flow_vel = w->flow_vel.p != nullptr;
    in.cluster_count = w->cluster_count; in.cluster_dynamic = w->cluster_dynamic;
    in.ctab_valid = w->ctab_valid; in.color_epoch = w->color_epoch;
    uint64_t st_cap = 0;
    const uint32_t* st_pairs = nullptr;
    const float* st_geo = nullptr;
    static_narrow_args(w, &st_cap, &st_pairs, &st_geo);
    const uint64_t n_ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? (uint32_t)w->n : 0u;
    in.statics = st_pairs != nullptr;
    // Capsules: the capsule variant wherever one can meet the narrow phase - an owned body (phys_set_bodies), a static in
    // use, or any ghost slot: ghosts arrive on the device with the shapes of another rank, which the host never sees
    in.capsules = w->body_capsules || (in.statics && w->static_capsules) || w->max_ghosts > 0;
    // Filters: the filtered variant once any filter was set since its reset (whatever the values), and
    // in every world with ghost slots: their filters arrive with the halo records, which the host never sees
    in.filters = w->body_filters_set || (in.statics && w->static_filters_set) || (n_ground && w->ground_filter_set) || w->max_ghosts > 0;
    in.materials = materials_active(w);
    in.np_items = n_ground + w->max_pairs + st_cap;
    return in;
}

// the value of a switch, parsed by `parse`; std::nullopt when the variable is not set
template <class Parse>
static auto debug_env(const char* name, Parse parse) -> std::optional<decltype(parse(""))> {
    if (const char* v = getenv(name)) return parse(v);
    return std::nullopt;
}
static bool debug_set(const char* name) { return getenv(name) != nullptr; }
static uint64_t parse_u64(const char* v) { return strtoull(v, nullptr, 10); }
static bool parse_one(const char* v) { return v[0] == '1'; }

const DebugSwitches& debug_switches() {
    static const DebugSwitches d = [] {
        DebugSwitches s;
        s.no_cluster = debug_set("PHYS_DEBUG_NO_CLUSTER");
        s.cluster_min = debug_env("PHYS_DEBUG_CLUSTER_MIN", parse_u64);
        s.clusters_per_cu = debug_env("PHYS_DEBUG_CLUSTERS_PER_CU", atoi);
        s.cluster_dynamic = debug_set("PHYS_DEBUG_CLUSTER_DYNAMIC");
        s.cluster_cap = debug_env("PHYS_DEBUG_CLUSTER_CAP", parse_u64).value_or(0);
        s.flow_max = debug_env("PHYS_DEBUG_FLOW_MAX", parse_u64);
        s.flow_quad_max = debug_env("PHYS_DEBUG_FLOW_QUAD_MAX", parse_u64).value_or(0);
        s.flow_pipeline = debug_env("PHYS_DEBUG_FLOW_PIPELINE", parse_one);
        s.np_early_probe = debug_env("PHYS_DEBUG_NP_EARLY_PROBE", parse_one);
        s.no_flow_preference = debug_set("PHYS_DEBUG_NO_FLOW_PREFERENCE");
        s.flow_stall = debug_set("PHYS_DEBUG_FLOW_STALL");
        s.flow_epoch = debug_env("PHYS_DEBUG_FLOW_EPOCH", [](const char* v) { return (uint32_t)strtoul(v, nullptr, 0); }).value_or(0u);
        s.ctab_slots = debug_env("PHYS_DEBUG_CTAB_SLOTS", parse_u64).value_or(0);
        s.color_kernel_lane = debug_env("PHYS_DEBUG_COLOR_KERNEL", [](const char* v) { return v[0] == 'l'; });
        s.np_threads = debug_env("PHYS_DEBUG_NP_THREADS", atoi).value_or(0);
        s.pair_lanes = debug_env("PHYS_DEBUG_PAIR_LANES", atoi).value_or(0);
        s.pair_kernel_brick = debug_env("PHYS_DEBUG_PAIR_KERNEL", [](const char* v) { return v[0] != 'b' || v[1] == 'r'; });
        s.brick_stage = debug_env("PHYS_DEBUG_BRICK_STAGE", atoi).value_or(0);
        s.raycast_stats = debug_set("PHYS_DEBUG_RAYCAST_STATS");
        return s;
    }();
    return d;
}
}  // namespace phys

// std::time::Duration::as_secs_f32 (used at rigid_body.rs:25)
static float duration_as_secs_f32(uint64_t nanos_total) {
    const uint64_t secs = nanos_total / 1000000000ull;
    const uint32_t nanos = (uint32_t)(nanos_total % 1000000000ull);
    return (float)secs + (float)nanos / 1.0e9f;
}

// The one teardown of a world, also of a half-made one (phys_create's failure paths): nothing is released while work on
// the stream can still touch it; the device buffers go with the members, after this body.
phys_world::~phys_world() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    prof.destroy();
    for (int k = 0; k < kSnapRing; ++k) {
        if (h_snap[k]) (void)hipHostFree(h_snap[k]);
        if (snap_event[k]) (void)hipEventDestroy(snap_event[k]);
    }
    if (h_counters) (void)hipHostFree(h_counters);
    if (stream) (void)hipStreamDestroy(stream);
}

// a {word, word} pair per item (filters, materials), up: ordered behind the updates already enqueued, which keep what they were
// enqueued with ...
template <typename T>
static int32_t upload_pairs(phys_world* w, DevBuf<T>& dst, const std::vector<T>& h, bool& set_flag) {
    if (!h.empty()) PHYS_HIP_TRY(hipMemcpyAsync(dst.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // the staging vector dies with the caller
    set_flag = true;
    return PHYS_OK;
}
// ... and the owned bodies' pairs back down
template <typename T>
static int32_t download_body_pairs(phys_world* w, const DevBuf<T>& src, std::vector<T>& h) {
    h.resize(2 * w->n_owned);
    if (!h.empty()) PHYS_HIP_TRY(hipMemcpyAsync(h.data(), src.p, sizeof(T) * h.size(), hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

// A call's host arrays in ONE device buffer of the world, laid out by the call's declarations (StageLayout, staging.hpp):
// reserve() sizes the buffer from them, copy() moves every array that is there, one hipMemcpyAsync each.
struct Staging : StageLayout {
    phys_world* w;
    DevBuf<uint8_t>& buf;
    Staging(phys_world* w, DevBuf<uint8_t>& buf) : w(w), buf(buf) {}
    int32_t reserve() {
        if (refused) return fail(PHYS_ERR_INVALID_ARG, "more arrays than a staging buffer holds");
        PHYS_HIP_TRY(buf.resize(total));
        return PHYS_OK;
    }
    // the device array of a slot, null for a null host array (valid after reserve())
    template <typename T>
    T* at(Slot<T> s) const { return StageLayout::at(buf.p, s); }
    int32_t copy(hipMemcpyKind kind) {
        for (int k = 0; k < count; ++k) {
            const Array& a = arrays[k];
            if (kind == hipMemcpyHostToDevice) PHYS_HIP_TRY(hipMemcpyAsync(buf.p + a.offset, a.host, a.bytes, kind, w->stream));
            else PHYS_HIP_TRY(hipMemcpyAsync(a.host, buf.p + a.offset, a.bytes, kind, w->stream));
        }
        return PHYS_OK;
    }
};

// The two paths of every query family that is a batch (staging.hpp): its entry points fill the batch from
// their arguments and name one of these, with the CastKind behind the batch for the casts.
// On device arrays: checked (args_error), then enqueued (launch_query, kernels.hpp)
template <class Batch, class... Kind>
static int32_t query_device(phys_world* w, const Batch& b, Kind... kind) {
    ENTER(w);
    if (const char* bad = args_error(kind..., b)) return fail(PHYS_ERR_INVALID_ARG, bad);
    if (b.n == 0) return PHYS_OK;
    return launch_query(w, kind..., b);
}

// On host arrays: checked, staged (the inputs in w->stage, the per-query outputs in w->rc_out, the character's hit slots in
// w->rc_slots: a group without arrays takes no room and no copy), run, read back; synchronises once
template <class Batch, class... Kind>
static int32_t query_host(phys_world* w, const Batch& b, Kind... kind) {
    ENTER(w);
    if (const char* bad = args_error(kind..., b)) return fail(PHYS_ERR_INVALID_ARG, bad);
    if (b.n == 0) return PHYS_OK;
    Staging st[kStageGroups] = {{w, w->stage}, {w, w->rc_out}, {w, w->rc_slots}};
    stage(b, st);
    for (Staging& s : st) PHYS_TRY(s.reserve());
    PHYS_TRY(st[kStageIn].copy(hipMemcpyHostToDevice));
    uint8_t* const bases[kStageGroups] = {st[kStageIn].buf.p, st[kStageOut].buf.p, st[kStageSlots].buf.p};
    PHYS_TRY(launch_query(w, kind..., staged(b, bases)));
    PHYS_TRY(st[kStageOut].copy(hipMemcpyDeviceToHost));
    PHYS_TRY(st[kStageSlots].copy(hipMemcpyDeviceToHost));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

extern "C" {

void phys_config_default(phys_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->abi_version = PHYS_ABI_VERSION;
    cfg->device = 0;
    cfg->flags = 0;
    cfg->gravity_force[0] = 0.0f; cfg->gravity_force[1] = -9.81f; cfg->gravity_force[2] = 0.0f;  // physics.rs:90
    cfg->gravity_offset[0] = 0.0f; cfg->gravity_offset[1] = 0.0f; cfg->gravity_offset[2] = 1.5f;  // physics.rs:91
    cfg->cg_max_iterations = 1000;  // sle_solver.rs:5
    cfg->cg_max_error = 1e-2f;      // sle_solver.rs:6
    cfg->cg_min_error = 1e-3f;      // sle_solver.rs:7
    cfg->solver_iterations = 8;
    cfg->baumgarte = 0.2f;
    cfg->slop = 0.01f;
    cfg->friction = 0.5f;
    cfg->contact_margin = 0.02f;
    cfg->ground_height = 0.0f;
    cfg->max_bias = 3.0f;
    cfg->max_pairs = 0;
    cfg->max_manifolds = 0;
    cfg->max_ghosts = 0;
}

const char* phys_last_error(void) { return get_error(); }
uint32_t phys_abi_version(void) { return PHYS_ABI_VERSION; }

int32_t phys_create(const phys_config* cfg, phys_world** out) {
    if (!cfg || !out) return fail(PHYS_ERR_INVALID_ARG, "null argument");
    if (cfg->abi_version != PHYS_ABI_VERSION) return fail(PHYS_ERR_INVALID_ARG, "phys_config.abi_version mismatch");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PHYS_ERR_NO_DEVICE, "no HIP device visible: libphysics_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= count) return fail(PHYS_ERR_NO_DEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    PHYS_HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PHYS_ERR_NO_DEVICE, "device is not gfx950 (MI355X); this library carries gfx950 code only");
    PHYS_HIP_TRY(hipSetDevice(cfg->device));
    int cus = 0;
    PHYS_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
    phys_world* w = new phys_world();
    w->cfg = *cfg;
    w->device = cfg->device;
    w->cus = cus;
    hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete w; return fail(PHYS_ERR_HIP, "hipStreamCreate failed"); }  // ~phys_world: whatever exists by then
    e = w->counters.resize(1);
    if (e == hipSuccess) e = hipHostMalloc((void**)&w->h_counters, sizeof(StepCounters), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(w->counters.p, 0, sizeof(StepCounters), w->stream);
    if (e != hipSuccess) { delete w; return fail(PHYS_ERR_HIP, "counter allocation failed"); }
    std::memset(w->h_counters, 0, sizeof(StepCounters));
    phys::g_worlds[w->device & 63].fetch_add(1);
    *out = w;
    return PHYS_OK;
}

int32_t phys_destroy(phys_world* w) {
    if (!w) return PHYS_OK;
    phys::g_worlds[w->device & 63].fetch_sub(1);
    delete w;
    return PHYS_OK;
}

int32_t phys_set_bodies(phys_world* w, uint64_t n, const float* pos, const float* rot, const float* lin,
                        const float* ang, const float* mass, const float* inertia, const uint32_t* shape_type,
                        const float* half_extent) {
    ENTER(w);
    if (n && !pos) return fail(PHYS_ERR_INVALID_ARG, "pos is required");
    if (n >= 0x7FFFFFFFull) return fail(PHYS_ERR_INVALID_ARG, "too many bodies (u32 indices)");
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    // sharded worlds: max_ghosts kinematic slots behind the owned bodies (filled by phys_halo_unpack_ghosts)
    const uint64_t G = (w->cfg.flags & PHYS_FLAG_COLLISIONS) && !(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY) ? w->cfg.max_ghosts : 0;
    const uint64_t nt = n ? n + G : 0;
    if (nt >= 0x7FFFFFFFull) return fail(PHYS_ERR_INVALID_ARG, "too many bodies + ghosts (u32 indices)");
    PHYS_HIP_TRY(w->pos.resize(3 * nt)); PHYS_HIP_TRY(w->rot.resize(4 * nt)); PHYS_HIP_TRY(w->vel.resize(8 * nt));
    PHYS_HIP_TRY(w->force.resize(3 * nt)); PHYS_HIP_TRY(w->torque.resize(3 * nt));
    PHYS_HIP_TRY(w->inv_inertia.resize(9 * nt)); PHYS_HIP_TRY(w->inv_inertia_diag.resize(4 * nt));
    PHYS_HIP_TRY(w->half_extent.resize(3 * nt)); PHYS_HIP_TRY(w->aabb.resize(6 * nt)); PHYS_HIP_TRY(w->shape.resize(nt));
    PHYS_HIP_TRY(w->global_id.resize(nt));
    PHYS_HIP_TRY(w->filt.resize(2 * nt));
    PHYS_HIP_TRY(w->mat.resize(2 * nt));
    if ((w->cfg.flags & PHYS_FLAG_COLLISIONS) && !(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY)) PHYS_HIP_TRY(w->geo.resize(16 * nt));
    w->n = nt;
    w->n_owned = n;
    w->max_ghosts = nt - n;
    w->forces_dirty = false;
    w->aabbs_valid = false;
    w->grid_valid = false;
    w->sorted_grid_valid = false;
    w->hint = StepHint();
    w->static_pairs_sized = false;  // static.hip: the next update measures its (body, static) pairs
    w->body_filters_set = false;    // every body slot gets the default filter below
    w->body_materials_set = false;  // ... and the default material
    for (int k = 0; k < phys_world::kSnapRing; ++k) w->snap_pending[k] = false;  // the stream was synchronised above
    PHYS_TRY(events_reset(w));    // contact events: history and pending events are gone
    PHYS_TRY(triggers_reset(w));  // trigger volumes: occupancy and pending events too
    PHYS_TRY(ccd_set(w, {}));     // continuous collision: the listed ids are stale
    if (n == 0) return PHYS_OK;

    // host staging with RigidBody::new defaults (setup.hpp); ghost slots: no shape, immovable
    const BodyStaging h = stage_bodies(n, nt - n, pos, rot, lin, ang, mass, inertia, shape_type, half_extent, w->cfg.friction);
    w->singular_inertia = h.singular_inertia;
    w->all_diag_inertia = h.all_diag_inertia;
    w->uniform_inertia = h.uniform_inertia;
    w->body_capsules = h.body_capsules;
    hipStream_t s = w->stream;
    PHYS_HIP_TRY(hipMemcpyAsync(w->pos.p, h.pos.data(), 12 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->rot.p, h.rot.data(), 16 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->vel.p, h.vel.data(), 32 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemsetAsync(w->force.p, 0, 12 * nt, s));
    PHYS_HIP_TRY(hipMemsetAsync(w->torque.p, 0, 12 * nt, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->inv_inertia.p, h.inv_inertia.data(), 36 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->inv_inertia_diag.p, h.inv_inertia_diag.data(), 16 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->half_extent.p, h.half_extent.data(), 12 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->shape.p, h.shape.data(), 4 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->global_id.p, h.global_id.data(), 4 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->filt.p, h.filt.data(), 8 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->mat.p, h.mat.data(), 8 * nt, hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // the staged arrays are done with
    if (w->cfg.flags & PHYS_FLAG_COLLISIONS) {
        const GridPlan grid = grid_plan(w->n, w->n_owned, pos, half_extent, w->cfg.contact_margin);
        w->grid_table_size = grid.table_size;
        w->grid_shape = grid.shape;
        PHYS_TRY(collision_alloc(w));
        if (!(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY)) {
            PHYS_TRY(cluster_assign(w, pos));  // spatial clusters of the cluster solver (large scenes only)
            // contact events follow the manifold capacity; a body set too large for warm starting turns them off
            // (phys_get_contact_events then answers PHYS_ERR_UNSUPPORTED)
            if (w->ev_capacity && !w->warm) w->ev_capacity = 0;
            PHYS_TRY(events_alloc(w));
        }
    }
    return PHYS_OK;
}

static int32_t add_constraint(phys_world* w, uint32_t kind, uint64_t body, const float t[3]) {
    ENTER(w);
    if (!t) return fail(PHYS_ERR_INVALID_ARG, "null target");
    if (body >= w->n_owned) return fail(PHYS_ERR_OUT_OF_RANGE, "body index out of range");
    Constraint c;
    c.kind = kind; c.body = (uint32_t)body;
    c.target[0] = t[0]; c.target[1] = t[1]; c.target[2] = t[2];
    w->constraints.push_back(c);
    w->constraints_dirty = true;
    return PHYS_OK;
}
int32_t phys_add_constraint_fix_point(phys_world* w, uint64_t body, const float target[3]) {
    return add_constraint(w, 0u, body, target);
}
int32_t phys_add_constraint_fix_orientation(phys_world* w, uint64_t body, const float target_rpy[3]) {
    return add_constraint(w, 1u, body, target_rpy);
}
int32_t phys_clear_constraints(phys_world* w) {
    ENTER(w);
    w->constraints.clear();
    w->constraints_dirty = true;
    return PHYS_OK;
}

static int32_t apply_force(phys_world* w, uint64_t body, int mode, const float f[3], const float arg[3]) {
    ENTER(w);
    if (!f || (mode != 0 && !arg)) return fail(PHYS_ERR_INVALID_ARG, "null argument");
    if (body >= w->n_owned) return fail(PHYS_ERR_OUT_OF_RANGE, "body index out of range");
    launch_apply_force_one(w, (uint32_t)body, mode, f, arg);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}
int32_t phys_apply_force_centre_of_gravity(phys_world* w, uint64_t body, const float force[3]) {
    return apply_force(w, body, 0, force, nullptr);
}
int32_t phys_apply_force_at_position(phys_world* w, uint64_t body, const float force[3], const float point[3]) {
    return apply_force(w, body, 1, force, point);
}
int32_t phys_apply_force_at_offset(phys_world* w, uint64_t body, const float force[3], const float offset[3]) {
    return apply_force(w, body, 2, force, offset);
}

int32_t phys_set_forces(phys_world* w, const float* force, const float* torque) {
    ENTER(w);
    if (force) PHYS_HIP_TRY(hipMemcpyAsync(w->force.p, force, 12 * w->n_owned, hipMemcpyHostToDevice, w->stream));
    if (torque) PHYS_HIP_TRY(hipMemcpyAsync(w->torque.p, torque, 12 * w->n_owned, hipMemcpyHostToDevice, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    if (force || torque) w->forces_dirty = true;
    return PHYS_OK;
}

int32_t phys_apply_gravity(phys_world* w) {
    ENTER(w);
    launch_apply_gravity(w);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

int32_t phys_step(phys_world* w, uint64_t dt_nanos) {
    ENTER(w);
    if (w->singular_inertia) return fail(PHYS_ERR_SINGULAR_INERTIA, "singular inertia tensor (reference: unwrap panic, rigid_body.rs:31)");
    launch_step_full(w, duration_as_secs_f32(dt_nanos), /*gravity=*/false);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

// one PhysicsState::update (physics.rs:41-55), enqueued without synchronising
// The collision stages in their order: poll the snapshots, plan (plan.hpp), launch. The plan is made where its inputs stand:
// the pair search and the colouring up front, the narrow phase behind the static pairs (which size its work), the solver
// behind the colouring stage (which, on its Probe path, has adopted exact counters as the hint by then).
static int32_t enqueue_update(phys_world* w, float dt) {
    // a zero-length step has no contact problem to solve (the bias terms divide by dt): plain RigidBody::step then
    const bool collisions = (w->cfg.flags & PHYS_FLAG_COLLISIONS) != 0 && dt > 0.0f;
    if (collisions) poll_snapshots(w);
    const DebugSwitches& dbg = debug_switches();
    const bool have_constraints = !w->constraints.empty();
    bool gravity_pending = true;
    if (w->n_fields) launch_force_fields(w);  // force fields: into the accumulators, from the poses and velocities as they stand
    if (w->n_liquids) launch_liquids(w);      // liquids: behind the fields, from the same poses and velocities
    if (have_constraints) {
        // the constraint right-hand side reads Q = force/torque accumulators including gravity (constraints.rs:92-104):
        // the constraint kernel adds gravity to the accumulators of the bodies it reads, and the step kernel adds
        // J^T lambda to entity 0 behind its own gravity addition - the reference's order, without a pass over all bodies
        PHYS_TRY(constraints_alloc(w));
        launch_constraint_phase(w, gravity_pending);
    }
    if (!collisions) {
        launch_step_full(w, dt, gravity_pending, have_constraints);
    } else {
        // per-step state: zeroed by the first kernel of the step itself; every 32nd step a memset in front of it
        // also restarts the running extent bound (which that kernel raises, so it cannot zero it)
        const bool restart_extent = w->steps % 32 == 0 || w->step_zero_reset_bytes % 16 != 0 || (w->step_zero_reset_bytes >> 36) != 0;
        if (restart_extent) zero_step_state(w, /*including_extent=*/true);
        launch_step_velocity_aabb(w, dt, gravity_pending, /*zero_step=*/!restart_extent, have_constraints);
        launch_broadphase(w, plan_pairs(plan_inputs(w), w->hint, dbg));
        if (!(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY)) {
            PHYS_TRY(launch_static_pairs(w));  // static colliders only (phys_set_static_bodies): nothing otherwise
            const PlanInputs in = plan_inputs(w);
            launch_narrowphase(w, plan_narrowphase(in, w->hint, dbg));
            const ColorPlan coloring = plan_coloring(in, w->hint, dbg);
            // dynamic clusters are remade from this update's bodies every few updates, and may not fit: their answer is an input
            const bool cluster = coloring.wants_cluster && (!w->cluster_dynamic || cluster_plan_dynamic(w, w->hint, dbg));
            launch_coloring(w, coloring, cluster);
            launch_solver(w, dt, plan_solver(in, w->hint, dbg, cluster), coloring);  // (the hint may be the exact one now)
            // contact events: nothing in a world without them
            if (w->ev_capacity) launch_events(w, (uint32_t)(w->steps + 1), plan_event_blocks(in, w->hint));
        } else {
            snapshot_counters_async(w, /*full=*/false);  // launch-size hints of later updates (the colouring stage takes it otherwise)
        }
        // continuous collision: nothing in a world without a list; behind the solver and the events, so the velocities are final
        const bool ccd = w->n_ccd != 0 && !(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY);
        if (ccd) launch_ccd_sweep(w, dt);
        launch_step_position(w, dt, ccd);
    }
    if (w->n_triggers) launch_triggers(w, (uint32_t)(w->steps + 1));  // trigger volumes, against the poses just written
    PHYS_HIP_TRY(hipGetLastError());
    w->steps++;
    if (w->prof.on) { w->prof.steps++; if (w->prof.used > 4096) w->prof.collect(w->stream); }
    return PHYS_OK;
}

int32_t phys_update_n(phys_world* w, uint64_t dt_nanos, uint32_t n) {
    ENTER(w);
    if (w->n == 0) return fail(PHYS_ERR_NO_BODIES, "update with no bodies (reference: index panic, physics.rs:48)");
    if (w->singular_inertia) return fail(PHYS_ERR_SINGULAR_INERTIA, "singular inertia tensor (reference: unwrap panic, rigid_body.rs:31)");
    const float dt = duration_as_secs_f32(dt_nanos);
    for (uint32_t k = 0; k < n; ++k) PHYS_TRY(enqueue_update(w, dt));
    return PHYS_OK;
}

int32_t phys_update(phys_world* w, uint64_t dt_nanos) { return phys_update_n(w, dt_nanos, 1); }

// Device-side errors are STICKY: every overflow bit raised by any step since the last phys_sync is reported here
// (StepCounters::sticky_overflow; the per-step word is zeroed by the next step), then cleared.
int32_t phys_sync(phys_world* w) {
    ENTER(w);
    PHYS_TRY(fetch_counters(w));
    poll_snapshots(w);  // the stream is idle: every snapshot in flight is adopted now, none can bring reported bits back later
    const uint32_t bits = w->h_counters->overflow | w->h_counters->sticky_overflow | w->host_sticky_overflow;
    if (w->h_counters->n_static_pairs > w->static_pairs_seen) w->static_pairs_seen = w->h_counters->n_static_pairs;
    w->host_sticky_overflow = 0;
    if (w->h_counters->sticky_overflow) {
        PHYS_HIP_TRY(hipMemsetAsync(&w->counters.p->sticky_overflow, 0, sizeof(uint32_t), w->stream));
        PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    // (a refused row keeps its note on the device) reported below: the next event may leave its own note
    if (!(bits & kOvfCorruptRow) && w->h_counters->debug[0] != 0u) {
        PHYS_HIP_TRY(hipMemsetAsync(w->counters.p->debug, 0, sizeof(w->counters.p->debug), w->stream));
        PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    const SyncError err = sync_error(bits, w->h_counters->debug);
    return err.code == PHYS_OK ? PHYS_OK : fail(err.code, err.message.c_str());
}

static int32_t d2h(phys_world* w, void* dst, const void* src, size_t bytes) {
    if (!dst || bytes == 0) return PHYS_OK;
    PHYS_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, w->stream));
    return PHYS_OK;
}

int32_t phys_get_transforms(phys_world* w, float* pos_out, float* rot_out) {
    ENTER(w);
    PHYS_TRY(d2h(w, pos_out, w->pos.p, 12 * w->n_owned));
    PHYS_TRY(d2h(w, rot_out, w->rot.p, 16 * w->n_owned));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}
int32_t phys_get_velocities(phys_world* w, float* lin_out, float* ang_out) {
    ENTER(w);
    // strided read-out of the 32-byte velocity records: 12 bytes per body from a 32-byte pitch
    if (lin_out && w->n_owned) PHYS_HIP_TRY(hipMemcpy2DAsync(lin_out, 12, w->vel.p, 32, 12, w->n_owned, hipMemcpyDeviceToHost, w->stream));
    if (ang_out && w->n_owned) PHYS_HIP_TRY(hipMemcpy2DAsync(ang_out, 12, w->vel.p + 4, 32, 12, w->n_owned, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}
int32_t phys_get_forces(phys_world* w, float* force_out, float* torque_out) {
    ENTER(w);
    PHYS_TRY(d2h(w, force_out, w->force.p, 12 * w->n_owned));
    PHYS_TRY(d2h(w, torque_out, w->torque.p, 12 * w->n_owned));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

int32_t phys_get_instance_matrices(phys_world* w, float* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    if (w->n == 0) return PHYS_OK;
    DevBuf<float> d;  // scratch of this call
    PHYS_HIP_TRY(d.resize(16 * w->n));
    launch_instance_matrices(w, d.p);
    PHYS_HIP_TRY(hipMemcpyAsync(out, d.p, 64 * w->n_owned, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

int32_t phys_get_lambda(phys_world* w, float* lambda_out, uint64_t cap, uint64_t* n_rows) {
    ENTER(w);
    if (!n_rows) return fail(PHYS_ERR_INVALID_ARG, "null n_rows");
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    uint32_t st[4] = {0, 0, 0, 0};
    if (w->cg_status.p && !w->constraints_dirty) PHYS_HIP_TRY(hipMemcpy(st, w->cg_status.p, 16, hipMemcpyDeviceToHost));
    const uint64_t rows = st[2] ? 3 * (uint64_t)w->constraints.size() : 0;  // previous_solution: Option
    *n_rows = rows;
    if (lambda_out && rows) {
        const uint64_t m = rows < cap ? rows : cap;
        PHYS_HIP_TRY(hipMemcpy(lambda_out, w->cg_x.p, 4 * m, hipMemcpyDeviceToHost));
    }
    return PHYS_OK;
}

int32_t phys_get_aabbs(phys_world* w, float* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    launch_aabb_only(w);
    PHYS_TRY(d2h(w, out, w->aabb.p, 24 * w->n_owned));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

int32_t phys_broadphase(phys_world* w, uint32_t* pairs_out, uint64_t cap, uint64_t* n_pairs) {
    ENTER(w);
    if (!n_pairs) return fail(PHYS_ERR_INVALID_ARG, "null n_pairs");
    if (!(w->cfg.flags & PHYS_FLAG_COLLISIONS)) return fail(PHYS_ERR_UNSUPPORTED, "world created without PHYS_FLAG_COLLISIONS");
    if (w->n == 0) { *n_pairs = 0; return PHYS_OK; }
    zero_step_state(w, true);
    launch_aabb_only(w);
    launch_broadphase(w, plan_pairs(plan_inputs(w), w->hint, debug_switches()));
    PHYS_HIP_TRY(hipGetLastError());
    return sorted_pairs_to_host(w, pairs_out, cap, n_pairs);
}

int32_t phys_get_manifolds(phys_world* w, uint32_t* ids_out, uint32_t* counts_out, float* normals_out,
                           float* points_out, uint64_t cap, uint64_t* n_manifolds) {
    ENTER(w);
    if (!n_manifolds) return fail(PHYS_ERR_INVALID_ARG, "null n_manifolds");
    PHYS_TRY(fetch_counters(w));
    const uint64_t m = w->h_counters->n_manifolds < w->max_manifolds ? w->h_counters->n_manifolds : w->max_manifolds;
    *n_manifolds = m;
    if (m == 0 || (!ids_out && !counts_out && !normals_out && !points_out)) return PHYS_OK;
    // read back in storage order, sort by (a, b) on the host (a read-out convenience, not the hot path)
    std::vector<uint32_t> ab(2 * m), c(m);
    std::vector<float> nrm(3 * m), pts(16 * m);
    {
        std::vector<float> geo(kManifoldFloats * m);  // the manifold records (records.hpp)
        PHYS_HIP_TRY(hipMemcpy(geo.data(), w->man_geo.p, kManifoldBytes * m, hipMemcpyDeviceToHost));
        static_assert(kManifoldWordB == kManifoldWordA + 1, "a and b are copied as one pair");
        for (uint64_t k = 0; k < m; ++k) {
            const float* g = &geo[kManifoldFloats * k];
            std::memcpy(&ab[2 * k], g + kManifoldWordA, 8); std::memcpy(&c[k], g + kManifoldWordCount, 4);
            std::memcpy(&nrm[3 * k], g + kManifoldWordNormal, 12);
            std::memcpy(&pts[16 * k], g + kManifoldWordPoints, 64);
        }
    }
    const std::vector<uint64_t> order = manifold_order(ab.data(), 2, m);
    for (uint64_t k = 0; k < m && k < cap; ++k) {
        const uint64_t s = order[k];
        if (ids_out) { ids_out[2 * k] = ab[2 * s]; ids_out[2 * k + 1] = ab[2 * s + 1]; }
        if (counts_out) counts_out[k] = c[s];
        if (normals_out) std::memcpy(normals_out + 3 * k, &nrm[3 * s], 12);
        if (points_out) std::memcpy(points_out + 16 * k, &pts[16 * s], 64);
    }
    return PHYS_OK;
}

int32_t phys_get_stats(phys_world* w, phys_stats* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    PHYS_TRY(fetch_counters(w));
    std::memset(out, 0, sizeof(*out));
    const StepCounters& c = *w->h_counters;
    out->n_bodies = w->n_owned;
    out->n_pairs = c.n_pairs;
    out->n_manifolds = c.n_manifolds;
    out->n_contacts = c.n_contacts;
    out->n_colors = c.n_colors;
    out->color_rounds = c.color_rounds;
    out->n_new_manifolds = c.n_new_manifolds;
    if (w->cg_status.p && !w->constraints.empty()) {
        uint32_t st[2] = {1, 0};
        PHYS_HIP_TRY(hipMemcpy(st, w->cg_status.p, 8, hipMemcpyDeviceToHost));
        out->cg_converged = (int32_t)st[0];
        out->cg_iterations = st[1];
    } else {
        out->cg_converged = 1;  // quirk Q8: CG on the empty system returns Some(empty) on its first check
        out->cg_iterations = w->steps ? 1u : 0u;
    }
    out->steps = w->steps;
    out->overflow = c.overflow | c.sticky_overflow | w->host_sticky_overflow;  // last step's bits + everything since the last phys_sync
    out->n_ground_manifolds = c.n_ground_manifolds;
    std::memcpy(&out->max_extent, &c.max_extent_bits, 4);
    out->n_halo_records = c.n_halo + c.n_halo_low;  // both faces of a neighbour exchange
    out->n_cross_pairs = c.n_cross_pairs;
    out->n_ghosts = c.n_ghosts;
    return PHYS_OK;
}

int32_t phys_set_static_bodies(phys_world* w, uint64_t n, const float* pos, const float* rot, const uint32_t* shape_type,
                               const float* half_extent) {
    // the arguments first: they are checked without a world or a device
    if (n >= 0x7FFFFFFEull) return fail(PHYS_ERR_INVALID_ARG, "too many static colliders (ids are PHYS_STATIC_ID_BIT | k below 0x7FFFFFFE)");
    if (n && (!pos || !shape_type || !half_extent)) return fail(PHYS_ERR_INVALID_ARG, "static colliders need pos, shape_type and half_extent");
    std::string bad;
    if (shape_set_error("static collider", n, shape_type, pos, rot, half_extent, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    ENTER(w);
    // the colour table and the warm-start records name static ids, which are stale now (as phys_set_bodies does); also
    // when the new set fails to upload below (the world then holds no statics)
    w->ctab_valid = false;
    w->color_epoch = 0;
    w->static_pairs_seen = 0;
    w->static_filters_set = false;  // the new set starts with the default filters (static_set)
    w->static_materials_set = false;  // ... and the default materials
    PHYS_TRY(events_reset(w));  // contact events name static ids too
    return static_set(w, n, pos, rot, shape_type, half_extent);
}

// ---- collision filters ----
// (pack_filters: setup.hpp)
static int32_t set_filters(phys_world* w, DevBuf<uint32_t>& dst, uint64_t expected, bool& set_flag, const char* wrong_count,
                           uint64_t n, const uint16_t* category, const uint16_t* mask, const int16_t* group) {
    if (n != expected) return fail(PHYS_ERR_INVALID_ARG, wrong_count);
    std::vector<uint32_t> h;
    pack_filters(n, category, mask, group, h);
    return upload_pairs(w, dst, h, set_flag);
}

int32_t phys_set_body_filters(phys_world* w, uint64_t n, const uint16_t* category, const uint16_t* mask, const int16_t* group) {
    ENTER(w);
    return set_filters(w, w->filt, w->n_owned, w->body_filters_set, "phys_set_body_filters: n must equal the body count", n, category, mask, group);
}

int32_t phys_set_static_filters(phys_world* w, uint64_t n, const uint16_t* category, const uint16_t* mask, const int16_t* group) {
    ENTER(w);
    return set_filters(w, w->st_filt, w->n_static, w->static_filters_set, "phys_set_static_filters: n must equal the static collider count", n,
                       category, mask, group);
}

int32_t phys_get_body_filters(phys_world* w, uint16_t* category_out, uint16_t* mask_out, int16_t* group_out) {
    ENTER(w);
    std::vector<uint32_t> h;
    PHYS_TRY(download_body_pairs(w, w->filt, h));
    for (uint64_t k = 0; k < w->n_owned; ++k) {
        if (category_out) category_out[k] = (uint16_t)(h[2 * k] & 0xFFFFu);
        if (mask_out) mask_out[k] = (uint16_t)(h[2 * k] >> 16);
        if (group_out) group_out[k] = (int16_t)(uint16_t)h[2 * k + 1];
    }
    return PHYS_OK;
}

int32_t phys_set_ground_filter(phys_world* w, uint16_t category, uint16_t mask) {
    ENTER(w);
    w->ground_filt = (uint32_t)category | ((uint32_t)mask << 16);  // read by the launches of the next update
    w->ground_filter_set = true;
    return PHYS_OK;
}

// ---- materials ----
// (pack_materials: setup.hpp)
static const char* const kMaterialRange = "a friction must be finite and >= 0, a restitution in [0, 1]";
// materials do not cross slab cuts (the halo record has no room for them): a sharded world refuses the calls
#define PHYS_NO_MATERIALS_WHEN_SHARDED(w) \
    do { if ((w)->cfg.max_ghosts > 0) return fail(PHYS_ERR_UNSUPPORTED, "materials are not supported in a world with max_ghosts > 0"); } while (0)

static int32_t set_materials(phys_world* w, DevBuf<float>& dst, uint64_t expected, bool& set_flag, const char* wrong_count, uint64_t n,
                             const float* friction, const float* restitution) {
    PHYS_NO_MATERIALS_WHEN_SHARDED(w);
    if (n != expected) return fail(PHYS_ERR_INVALID_ARG, wrong_count);
    std::vector<float> h;
    if (!pack_materials(n, friction, restitution, w->cfg.friction, h)) return fail(PHYS_ERR_INVALID_ARG, kMaterialRange);
    return upload_pairs(w, dst, h, set_flag);
}

int32_t phys_set_body_materials(phys_world* w, uint64_t n, const float* friction, const float* restitution) {
    ENTER(w);
    return set_materials(w, w->mat, w->n_owned, w->body_materials_set, "phys_set_body_materials: n must equal the body count", n, friction, restitution);
}

int32_t phys_set_static_materials(phys_world* w, uint64_t n, const float* friction, const float* restitution) {
    ENTER(w);
    return set_materials(w, w->st_mat, w->n_static, w->static_materials_set, "phys_set_static_materials: n must equal the static collider count", n,
                         friction, restitution);
}

int32_t phys_get_body_materials(phys_world* w, float* friction_out, float* restitution_out) {
    ENTER(w);
    PHYS_NO_MATERIALS_WHEN_SHARDED(w);
    std::vector<float> h;
    PHYS_TRY(download_body_pairs(w, w->mat, h));
    for (uint64_t k = 0; k < w->n_owned; ++k) {
        if (friction_out) friction_out[k] = h[2 * k];
        if (restitution_out) restitution_out[k] = h[2 * k + 1];
    }
    return PHYS_OK;
}

int32_t phys_set_ground_material(phys_world* w, float friction, float restitution) {
    ENTER(w);
    PHYS_NO_MATERIALS_WHEN_SHARDED(w);
    std::vector<float> h;
    if (!pack_materials(1, &friction, &restitution, 0.0f, h)) return fail(PHYS_ERR_INVALID_ARG, kMaterialRange);
    w->ground_mat[0] = friction; w->ground_mat[1] = restitution;  // read by the launches of the next update
    w->ground_mat_set = true;
    return PHYS_OK;
}

int32_t phys_set_restitution_threshold(phys_world* w, float v) {
    ENTER(w);
    PHYS_NO_MATERIALS_WHEN_SHARDED(w);
    if (!std::isfinite(v) || v < 0.0f) return fail(PHYS_ERR_INVALID_ARG, "phys_set_restitution_threshold: v must be finite and >= 0");
    w->restitution_threshold = v;  // read by the launches of the next update
    return PHYS_OK;
}

int32_t phys_get_static_stats(phys_world* w, uint64_t* n_static, uint64_t* n_static_pairs, uint64_t* n_static_manifolds) {
    ENTER(w);
    PHYS_TRY(fetch_counters(w));
    const StepCounters& c = *w->h_counters;
    const bool on = w->n_static != 0;  // (the counters of an update before the set was cleared say nothing about it)
    if (n_static) *n_static = w->n_static;
    if (n_static_pairs) *n_static_pairs = on ? c.n_static_pairs : 0u;
    if (n_static_manifolds) *n_static_manifolds = on ? c.n_static_manifolds : 0u;
    return PHYS_OK;
}

int32_t phys_get_color_counts(phys_world* w, uint32_t* counts_out) {
    ENTER(w);
    if (!counts_out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    PHYS_TRY(fetch_counters(w));
    for (int k = 0; k < kMaxColors; ++k) counts_out[k] = k < (int)w->h_counters->n_colors ? w->h_counters->color_count[k] : 0u;
    return PHYS_OK;
}

int32_t phys_profile_enable(phys_world* w, int32_t on) {
    ENTER(w);
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    w->prof.reset();
    w->prof.on = on != 0;
    return PHYS_OK;
}

int32_t phys_profile_get(phys_world* w, phys_profile* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    w->prof.collect(w->stream);
    for (uint32_t k = 0; k < PHYS_STAGE_COUNT; ++k) { out->ms[k] = w->prof.ms[k]; out->launches[k] = w->prof.launches[k]; }
    out->steps = w->prof.steps;
    return PHYS_OK;
}

int32_t phys_get_device_view(phys_world* w, phys_device_view* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    out->n = w->n_owned;
    out->pos = w->pos.p; out->rot = w->rot.p; out->lin_vel = w->vel.p; out->ang_vel = w->vel.p + 4;  // both with a stride of 8 floats
    out->aabb = w->aabb.p;
    out->stream = (void*)w->stream;
    out->vel_stride = 8;
    return PHYS_OK;
}

// ---- queries: casts, move-and-slide, character walking, depenetration (all through query_host / query_device above); overlaps ----
// the sixteen cast entry points: each names its kind and fills the batch from its arguments, in CastBatch's order: n, origin, dir,
// rot, radius, half_length, max_t, ignore_body on the first line; query_mask, body_out, t_out, normal_out, point_out on the second
// (and a box cast's half_extent behind them)
int32_t phys_raycast(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                     const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out) {
    return query_host(w, CastBatch{n_rays, origin, dir, nullptr, nullptr, nullptr, max_t, ignore_body,
                                   nullptr, body_out, t_out, normal_out, nullptr}, CastKind::Ray);
}

int32_t phys_raycast_filtered(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                              const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out, float* t_out,
                              float* normal_out) {
    return query_host(w, CastBatch{n_rays, origin, dir, nullptr, nullptr, nullptr, max_t, ignore_body,
                                   query_mask, body_out, t_out, normal_out, nullptr}, CastKind::Ray);
}

int32_t phys_raycast_device(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                            const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out) {
    return query_device(w, CastBatch{n_rays, origin, dir, nullptr, nullptr, nullptr, max_t, ignore_body,
                                     nullptr, body_out, t_out, normal_out, nullptr}, CastKind::Ray);
}

int32_t phys_raycast_device_filtered(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                                     const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out, float* t_out,
                                     float* normal_out) {
    return query_device(w, CastBatch{n_rays, origin, dir, nullptr, nullptr, nullptr, max_t, ignore_body,
                                     query_mask, body_out, t_out, normal_out, nullptr}, CastKind::Ray);
}

int32_t phys_spherecast(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius, const float* max_t,
                        const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out) {
    return query_host(w, CastBatch{n, origin, dir, nullptr, radius, nullptr, max_t, ignore_body,
                                   nullptr, body_out, t_out, normal_out, nullptr}, CastKind::Sphere);
}

int32_t phys_spherecast_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius,
                                 const float* max_t, const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out,
                                 float* t_out, float* normal_out) {
    return query_host(w, CastBatch{n, origin, dir, nullptr, radius, nullptr, max_t, ignore_body,
                                   query_mask, body_out, t_out, normal_out, nullptr}, CastKind::Sphere);
}

int32_t phys_spherecast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius, const float* max_t,
                               const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out) {
    return query_device(w, CastBatch{n, origin, dir, nullptr, radius, nullptr, max_t, ignore_body,
                                     nullptr, body_out, t_out, normal_out, nullptr}, CastKind::Sphere);
}

int32_t phys_spherecast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* radius,
                                        const float* max_t, const uint32_t* ignore_body, const uint16_t* query_mask,
                                        uint32_t* body_out, float* t_out, float* normal_out) {
    return query_device(w, CastBatch{n, origin, dir, nullptr, radius, nullptr, max_t, ignore_body,
                                     query_mask, body_out, t_out, normal_out, nullptr}, CastKind::Sphere);
}

// capsule casts: rot, half_length and point_out besides
int32_t phys_capsulecast(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw, const float* radius,
                         const float* half_length, const float* max_t, const uint32_t* ignore_body, uint32_t* body_out, float* t_out,
                         float* normal_out, float* point_out) {
    return query_host(w, CastBatch{n, origin, dir, rot_ijkw, radius, half_length, max_t, ignore_body,
                                   nullptr, body_out, t_out, normal_out, point_out}, CastKind::Capsule);
}

int32_t phys_capsulecast_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                  const float* radius, const float* half_length, const float* max_t, const uint32_t* ignore_body,
                                  const uint16_t* query_mask, uint32_t* body_out, float* t_out, float* normal_out, float* point_out) {
    return query_host(w, CastBatch{n, origin, dir, rot_ijkw, radius, half_length, max_t, ignore_body,
                                   query_mask, body_out, t_out, normal_out, point_out}, CastKind::Capsule);
}

int32_t phys_capsulecast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                const float* radius, const float* half_length, const float* max_t, const uint32_t* ignore_body,
                                uint32_t* body_out, float* t_out, float* normal_out, float* point_out) {
    return query_device(w, CastBatch{n, origin, dir, rot_ijkw, radius, half_length, max_t, ignore_body,
                                     nullptr, body_out, t_out, normal_out, point_out}, CastKind::Capsule);
}

int32_t phys_capsulecast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                         const float* radius, const float* half_length, const float* max_t, const uint32_t* ignore_body,
                                         const uint16_t* query_mask, uint32_t* body_out, float* t_out, float* normal_out,
                                         float* point_out) {
    return query_device(w, CastBatch{n, origin, dir, rot_ijkw, radius, half_length, max_t, ignore_body,
                                     query_mask, body_out, t_out, normal_out, point_out}, CastKind::Capsule);
}

// the box cast: half_extent is the batch's last member
int32_t phys_boxcast(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw, const float* half_extent,
                     const float* max_t, const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out,
                     float* point_out) {
    return query_host(w, CastBatch{n, origin, dir, rot_ijkw, nullptr, nullptr, max_t, ignore_body,
                                   nullptr, body_out, t_out, normal_out, point_out, half_extent}, CastKind::Box);
}

int32_t phys_boxcast_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                              const float* half_extent, const float* max_t, const uint32_t* ignore_body, const uint16_t* query_mask,
                              uint32_t* body_out, float* t_out, float* normal_out, float* point_out) {
    return query_host(w, CastBatch{n, origin, dir, rot_ijkw, nullptr, nullptr, max_t, ignore_body,
                                   query_mask, body_out, t_out, normal_out, point_out, half_extent}, CastKind::Box);
}

int32_t phys_boxcast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                            const float* half_extent, const float* max_t, const uint32_t* ignore_body, uint32_t* body_out, float* t_out,
                            float* normal_out, float* point_out) {
    return query_device(w, CastBatch{n, origin, dir, rot_ijkw, nullptr, nullptr, max_t, ignore_body,
                                     nullptr, body_out, t_out, normal_out, point_out, half_extent}, CastKind::Box);
}

int32_t phys_boxcast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                     const float* half_extent, const float* max_t, const uint32_t* ignore_body,
                                     const uint16_t* query_mask, uint32_t* body_out, float* t_out, float* normal_out,
                                     float* point_out) {
    return query_device(w, CastBatch{n, origin, dir, rot_ijkw, nullptr, nullptr, max_t, ignore_body,
                                     query_mask, body_out, t_out, normal_out, point_out, half_extent}, CastKind::Box);
}

// move-and-slide: both entry points have the same parameters, the batch from them in SlideBatch's order
#define PHYS_SLIDE_BATCH                                                                                                   \
    SlideBatch{n, pos, motion, rot_ijkw, radius, half_length, skin, max_slides, ignore_body, query_mask,                   \
               pos_out, remaining_out, status_out, hit_body_out, hit_normal_out, hit_point_out}
int32_t phys_move_and_slide_device(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw,
                                   const float* radius, const float* half_length, float skin, uint32_t max_slides,
                                   const uint32_t* ignore_body, const uint16_t* query_mask, float* pos_out, float* remaining_out,
                                   uint32_t* status_out, uint32_t* hit_body_out, float* hit_normal_out, float* hit_point_out) {
    return query_device(w, PHYS_SLIDE_BATCH);
}

int32_t phys_move_and_slide(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw, const float* radius,
                            const float* half_length, float skin, uint32_t max_slides, const uint32_t* ignore_body,
                            const uint16_t* query_mask, float* pos_out, float* remaining_out, uint32_t* status_out,
                            uint32_t* hit_body_out, float* hit_normal_out, float* hit_point_out) {
    return query_host(w, PHYS_SLIDE_BATCH);
}
#undef PHYS_SLIDE_BATCH

// character walking: likewise, in CharacterBatch's order
#define PHYS_CHARACTER_BATCH                                                                                               \
    CharacterBatch{n, pos, motion, rot_ijkw, radius, half_length, grounded_in, skin, max_slides, step_height, snap_distance, \
                   min_floor_ny, ignore_body, query_mask, pos_out, remaining_out, status_out, floor_body_out,              \
                   floor_normal_out, floor_point_out, hit_body_out, hit_normal_out, hit_point_out}
int32_t phys_character_move_device(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw,
                                   const float* radius, const float* half_length, const uint32_t* grounded_in, float skin,
                                   uint32_t max_slides, float step_height, float snap_distance, float min_floor_ny,
                                   const uint32_t* ignore_body, const uint16_t* query_mask, float* pos_out, float* remaining_out,
                                   uint32_t* status_out, uint32_t* floor_body_out, float* floor_normal_out, float* floor_point_out,
                                   uint32_t* hit_body_out, float* hit_normal_out, float* hit_point_out) {
    return query_device(w, PHYS_CHARACTER_BATCH);
}

int32_t phys_character_move(phys_world* w, uint64_t n, const float* pos, const float* motion, const float* rot_ijkw, const float* radius,
                            const float* half_length, const uint32_t* grounded_in, float skin, uint32_t max_slides, float step_height,
                            float snap_distance, float min_floor_ny, const uint32_t* ignore_body, const uint16_t* query_mask,
                            float* pos_out, float* remaining_out, uint32_t* status_out, uint32_t* floor_body_out,
                            float* floor_normal_out, float* floor_point_out, uint32_t* hit_body_out, float* hit_normal_out,
                            float* hit_point_out) {
    return query_host(w, PHYS_CHARACTER_BATCH);
}
#undef PHYS_CHARACTER_BATCH

// depenetration: both calls are one DepenBatch (probe: phys_penetration, max_iters 1, its body_out,
// normal_out and depth_out the one slot per query)
int32_t phys_penetration(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius, const float* half_length,
                         float max_gap, const uint32_t* ignore_body, const uint16_t* query_mask, uint32_t* body_out, float* depth_out,
                         float* normal_out) {
    return query_host(w, DepenBatch{n, pos, rot_ijkw, radius, half_length, max_gap, 1u, true, ignore_body, query_mask,
                                    nullptr, nullptr, body_out, normal_out, depth_out});
}

int32_t phys_penetration_device(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius,
                                const float* half_length, float max_gap, const uint32_t* ignore_body, const uint16_t* query_mask,
                                uint32_t* body_out, float* depth_out, float* normal_out) {
    return query_device(w, DepenBatch{n, pos, rot_ijkw, radius, half_length, max_gap, 1u, true, ignore_body, query_mask,
                                      nullptr, nullptr, body_out, normal_out, depth_out});
}

int32_t phys_depenetrate(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius, const float* half_length,
                         float skin, uint32_t max_iters, const uint32_t* ignore_body, const uint16_t* query_mask, float* pos_out,
                         uint32_t* status_out, uint32_t* hit_body_out, float* hit_normal_out, float* hit_depth_out) {
    return query_host(w, DepenBatch{n, pos, rot_ijkw, radius, half_length, skin, max_iters, false, ignore_body, query_mask,
                                    pos_out, status_out, hit_body_out, hit_normal_out, hit_depth_out});
}

int32_t phys_depenetrate_device(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* radius,
                                const float* half_length, float skin, uint32_t max_iters, const uint32_t* ignore_body,
                                const uint16_t* query_mask, float* pos_out, uint32_t* status_out, uint32_t* hit_body_out,
                                float* hit_normal_out, float* hit_depth_out) {
    return query_device(w, DepenBatch{n, pos, rot_ijkw, radius, half_length, skin, max_iters, false, ignore_body, query_mask,
                                      pos_out, status_out, hit_body_out, hit_normal_out, hit_depth_out});
}

static int32_t overlap_host(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot_ijkw,
                            const float* half_extent, const uint32_t* ignore_body, const uint16_t* query_mask, uint64_t cap,
                            uint64_t* offsets_out, uint32_t* ids_out) {
    ENTER(w);
    if (n >= (1ull << 31)) return fail(PHYS_ERR_INVALID_ARG, "phys_overlap: n must be below 2^31");
    if (!offsets_out) return fail(PHYS_ERR_INVALID_ARG, "phys_overlap: null offsets_out");
    if (n && (!shape_type || !pos || !half_extent)) return fail(PHYS_ERR_INVALID_ARG, "phys_overlap: null shape_type, pos or half_extent");
    if (cap && !ids_out) return fail(PHYS_ERR_INVALID_ARG, "phys_overlap: null ids_out with cap > 0");
    offsets_out[0] = 0;
    if (n == 0) return PHYS_OK;
    Staging in{w, w->stage};
    const auto s_type = in.add(shape_type, n);
    const auto s_pos = in.add(pos, 3 * n), s_he = in.add(half_extent, 3 * n);
    const auto s_ignore = in.add(ignore_body, n);
    const auto s_rot = in.add(rot_ijkw, 4 * n, /*align=*/16);  // read as float4
    const auto s_mask = in.add(query_mask, n);
    PHYS_TRY(in.reserve());
    PHYS_TRY(in.copy(hipMemcpyHostToDevice));
    return launch_overlap(w, n, in.at(s_type), in.at(s_pos), in.at(s_rot), in.at(s_he), in.at(s_ignore), cap, offsets_out, ids_out, in.at(s_mask));
}

int32_t phys_overlap(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot_ijkw,
                     const float* half_extent, const uint32_t* ignore_body, uint64_t cap, uint64_t* offsets_out, uint32_t* ids_out) {
    return overlap_host(w, n, shape_type, pos, rot_ijkw, half_extent, ignore_body, nullptr, cap, offsets_out, ids_out);
}

int32_t phys_overlap_filtered(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot_ijkw,
                              const float* half_extent, const uint32_t* ignore_body, const uint16_t* query_mask, uint64_t cap,
                              uint64_t* offsets_out, uint32_t* ids_out) {
    return overlap_host(w, n, shape_type, pos, rot_ijkw, half_extent, ignore_body, query_mask, cap, offsets_out, ids_out);
}

// ---- trigger volumes: checked and staged on the host (setup.hpp), where the records are built too ----
int32_t phys_set_triggers(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot_ijkw,
                          const float* half_extent, const uint16_t* mask) {
    // the arguments first, as phys_set_static_bodies checks them
    if (n > PHYS_MAX_TRIGGERS) return fail(PHYS_ERR_INVALID_ARG, "phys_set_triggers: more than PHYS_MAX_TRIGGERS trigger volumes");
    if (n && (!shape_type || !pos || !half_extent)) return fail(PHYS_ERR_INVALID_ARG, "trigger volumes need shape_type, pos and half_extent");
    std::string bad;
    if (shape_set_error("trigger", n, shape_type, pos, rot_ijkw, half_extent, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    ENTER(w);
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // updates in flight read the set that is replaced
    return triggers_set(w, stage_triggers(n, shape_type, pos, rot_ijkw, half_extent, mask));
}

int32_t phys_set_trigger_poses(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw) {
    ENTER(w);
    if (n != w->n_triggers) return fail(PHYS_ERR_INVALID_ARG, "phys_set_trigger_poses: n must equal the trigger count");
    if (n && !pos) return fail(PHYS_ERR_INVALID_ARG, "phys_set_trigger_poses: null pos");
    if (n == 0) return PHYS_OK;
    if (!restage_trigger_poses(w->tg_host, pos, rot_ijkw)) return fail(PHYS_ERR_INVALID_ARG, "phys_set_trigger_poses: non-finite pose");
    return triggers_rebuild(w);
}

// ---- force fields: checked and staged on the host (setup.hpp), where the records are built too ----
// who pushes a ghost is a question for a sharded scene that needs it: a sharded world refuses the calls, like the materials
#define PHYS_NO_FIELDS_WHEN_SHARDED(w) \
    do { if ((w)->cfg.max_ghosts > 0) return fail(PHYS_ERR_UNSUPPORTED, "force fields are not supported in a world with max_ghosts > 0"); } while (0)

int32_t phys_set_force_fields(phys_world* w, uint64_t n, const uint32_t* kind, const uint32_t* shape_type, const float* pos,
                              const float* rot_ijkw, const float* half_extent, const uint16_t* mask, const float* vec, const float* coef,
                              const uint32_t* exponent) {
    // the arguments first, as phys_set_triggers checks them
    if (n > PHYS_MAX_FORCE_FIELDS) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_fields: more than PHYS_MAX_FORCE_FIELDS force fields");
    if (n && (!kind || !shape_type || !pos || !half_extent || !vec || !coef))
        return fail(PHYS_ERR_INVALID_ARG, "force fields need kind, shape_type, pos, half_extent, vec and coef");
    std::string bad;
    if (field_set_error(n, kind, shape_type, pos, rot_ijkw, half_extent, vec, coef, exponent, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    ENTER(w);
    PHYS_NO_FIELDS_WHEN_SHARDED(w);
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // updates in flight read the set that is replaced
    return fields_set(w, stage_fields(n, kind, shape_type, pos, rot_ijkw, half_extent, mask, vec, coef, exponent));
}

int32_t phys_set_force_field_poses(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw) {
    ENTER(w);
    PHYS_NO_FIELDS_WHEN_SHARDED(w);
    if (n != w->n_fields) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_field_poses: n must equal the force field count");
    if (n && !pos) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_field_poses: null pos");
    if (n == 0) return PHYS_OK;
    if (!restage_field_poses(w->ff_host, pos, rot_ijkw)) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_field_poses: non-finite pose");
    return fields_rebuild(w);
}

int32_t phys_set_force_field_params(phys_world* w, uint64_t n, const float* vec, const float* coef) {
    ENTER(w);
    PHYS_NO_FIELDS_WHEN_SHARDED(w);
    if (n != w->n_fields) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_field_params: n must equal the force field count");
    if (n && (!vec || !coef)) return fail(PHYS_ERR_INVALID_ARG, "phys_set_force_field_params: null vec or coef");
    if (n == 0) return PHYS_OK;
    std::string bad;
    if (restage_field_params(w->ff_host, vec, coef, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    return fields_rebuild(w);
}

int32_t phys_apply_force_fields(phys_world* w) {
    ENTER(w);
    PHYS_NO_FIELDS_WHEN_SHARDED(w);
    launch_force_fields(w);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

// ---- liquids: checked and staged on the host (setup.hpp), where the records are built too ----
// which rank's liquid wets a ghost is a question for a sharded scene that needs it: a sharded world refuses the calls
#define PHYS_NO_LIQUIDS_WHEN_SHARDED(w) \
    do { if ((w)->cfg.max_ghosts > 0) return fail(PHYS_ERR_UNSUPPORTED, "liquids are not supported in a world with max_ghosts > 0"); } while (0)

int32_t phys_set_liquids(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw, const float* half_extent, const uint16_t* mask,
                         const float* density, const float* gravity, const float* flow, const float* drag) {
    // the arguments first, as phys_set_force_fields checks them
    if (n > PHYS_MAX_LIQUIDS) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquids: more than PHYS_MAX_LIQUIDS liquids");
    if (n && (!pos || !half_extent || !density || !gravity || !flow || !drag))
        return fail(PHYS_ERR_INVALID_ARG, "liquids need pos, half_extent, density, gravity, flow and drag");
    std::string bad;
    if (liquid_set_error(n, pos, rot_ijkw, half_extent, density, gravity, flow, drag, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // updates in flight read the set that is replaced
    return liquids_set(w, stage_liquids(n, pos, rot_ijkw, half_extent, mask, density, gravity, flow, drag));
}

int32_t phys_set_liquid_poses(phys_world* w, uint64_t n, const float* pos, const float* rot_ijkw) {
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    if (n != w->n_liquids) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquid_poses: n must equal the liquid count");
    if (n && !pos) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquid_poses: null pos");
    if (n == 0) return PHYS_OK;
    if (!restage_liquid_poses(w->lq_host, pos, rot_ijkw)) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquid_poses: non-finite pose");
    return liquids_rebuild(w);
}

int32_t phys_set_liquid_params(phys_world* w, uint64_t n, const float* density, const float* gravity, const float* flow, const float* drag) {
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    if (n != w->n_liquids) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquid_params: n must equal the liquid count");
    if (n && (!density || !gravity || !flow || !drag)) return fail(PHYS_ERR_INVALID_ARG, "phys_set_liquid_params: null density, gravity, flow or drag");
    if (n == 0) return PHYS_OK;
    std::string bad;
    if (restage_liquid_params(w->lq_host, density, gravity, flow, drag, bad)) return fail(PHYS_ERR_INVALID_ARG, bad.c_str());
    return liquids_rebuild(w);
}

int32_t phys_apply_liquids(phys_world* w) {
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    launch_liquids(w);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

int32_t phys_get_submersion_device(phys_world* w, float* dev_frac_out, uint32_t* dev_liquid_out) {
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    if (!dev_frac_out && !dev_liquid_out) return PHYS_OK;
    launch_submersion(w, dev_frac_out, dev_liquid_out);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

int32_t phys_get_submersion(phys_world* w, float* frac_out, uint32_t* liquid_out) {
    ENTER(w);
    PHYS_NO_LIQUIDS_WHEN_SHARDED(w);
    if ((!frac_out && !liquid_out) || w->n_owned == 0) return PHYS_OK;
    DevBuf<float> d;  // scratch of this call: frac, then the indices
    PHYS_HIP_TRY(d.resize(2 * w->n_owned));
    uint32_t* d_liquid = reinterpret_cast<uint32_t*>(d.p + w->n_owned);
    launch_submersion(w, d.p, d_liquid);
    PHYS_HIP_TRY(hipGetLastError());
    if (frac_out) PHYS_HIP_TRY(hipMemcpyAsync(frac_out, d.p, 4 * w->n_owned, hipMemcpyDeviceToHost, w->stream));
    if (liquid_out) PHYS_HIP_TRY(hipMemcpyAsync(liquid_out, d_liquid, 4 * w->n_owned, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

// ---- continuous collision: the list is checked on the host (setup.hpp stage_ccd), swept by ccd.hip ----
int32_t phys_set_ccd_bodies(phys_world* w, uint64_t n, const uint32_t* ids) {
    ENTER(w);
    if (!(w->cfg.flags & PHYS_FLAG_COLLISIONS)) return fail(PHYS_ERR_UNSUPPORTED, "phys_set_ccd_bodies: world created without PHYS_FLAG_COLLISIONS");
    // a ghost's step belongs to its owner's rank: a sharded world refuses the call, like the force fields
    if (w->cfg.max_ghosts > 0) return fail(PHYS_ERR_UNSUPPORTED, "continuous collision is not supported in a world with max_ghosts > 0");
    CcdStaging staged = stage_ccd(n, ids, w->n_owned);
    if (staged.code != PHYS_OK) return fail(staged.code, staged.message.c_str());  // the old list stays in force
    return ccd_set(w, std::move(staged.ids));
}

static int32_t ccd_hits(phys_world* w, float* frac_out, uint32_t* target_out, float* normal_out, uint32_t* count_out, bool to_host) {
    ENTER(w);
    PHYS_TRY(ccd_read(w, frac_out, target_out, normal_out, count_out, to_host));
    if (to_host) PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}
int32_t phys_get_ccd_hits(phys_world* w, float* frac_out, uint32_t* target_out, float* normal_out, uint32_t* count_out) {
    return ccd_hits(w, frac_out, target_out, normal_out, count_out, /*to_host=*/true);
}
int32_t phys_get_ccd_hits_device(phys_world* w, float* dev_frac_out, uint32_t* dev_target_out, float* dev_normal_out, uint32_t* dev_count_out) {
    return ccd_hits(w, dev_frac_out, dev_target_out, dev_normal_out, dev_count_out, /*to_host=*/false);
}

// ---- in-place body edits: checked and ordered on the host (setup.hpp), applied by edit.hip ----
// a ghost's state belongs to its owner's rank: a sharded world refuses the calls, like the materials and the force fields
#define PHYS_NO_EDITS_WHEN_SHARDED(w) \
    do { if ((w)->cfg.max_ghosts > 0) return fail(PHYS_ERR_UNSUPPORTED, "body edits are not supported in a world with max_ghosts > 0"); } while (0)

// edits on device arrays: checked (edit_args_error), then enqueued; ids in non-decreasing order are the caller's to give
static int32_t edit_device(phys_world* w, EditKind kind, const EditBatch& b) {
    ENTER(w);
    PHYS_NO_EDITS_WHEN_SHARDED(w);
    if (const char* bad = edit_args_error(kind, b)) return fail(PHYS_ERR_INVALID_ARG, bad);
    return launch_edit(w, kind, b);
}

// edits on host arrays: checked and ordered by id before anything is written (edit_order), staged in w->stage, applied;
// synchronises, like the queries on host arrays
static int32_t edit_host(phys_world* w, EditKind kind, const EditBatch& b) {
    ENTER(w);
    PHYS_NO_EDITS_WHEN_SHARDED(w);
    const EditOrder o = edit_order(kind, b, w->n_owned);
    if (o.code != PHYS_OK) return fail(o.code, o.message.c_str());
    if (b.n == 0) return PHYS_OK;
    std::vector<float> sorted[3];
    Staging in{w, w->stage};
    const auto s_ids = in.add(o.ids.data(), b.n);
    StageLayout::Slot<float> s_a[3];
    for (int k = 0; k < 3; ++k) {
        sorted[k] = edit_gather(o.order, b.a[k], edit_cols(kind, k));
        s_a[k] = in.add(b.a[k] ? sorted[k].data() : nullptr, sorted[k].size());
    }
    PHYS_TRY(in.reserve());
    PHYS_TRY(in.copy(hipMemcpyHostToDevice));
    PHYS_TRY(launch_edit(w, kind, {b.n, in.at(s_ids), {in.at(s_a[0]), in.at(s_a[1]), in.at(s_a[2])}}));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // the ordered arrays die with this call
    return PHYS_OK;
}

int32_t phys_set_body_poses(phys_world* w, uint64_t n, const uint32_t* ids, const float* pos, const float* rot_ijkw) {
    return edit_host(w, EditKind::Poses, {n, ids, {pos, rot_ijkw, nullptr}});
}
int32_t phys_set_body_velocities(phys_world* w, uint64_t n, const uint32_t* ids, const float* lin, const float* ang) {
    return edit_host(w, EditKind::Velocities, {n, ids, {lin, ang, nullptr}});
}
int32_t phys_apply_impulses(phys_world* w, uint64_t n, const uint32_t* ids, const float* impulse, const float* point, const float* ang_impulse) {
    return edit_host(w, EditKind::Impulses, {n, ids, {impulse, point, ang_impulse}});
}
int32_t phys_apply_forces(phys_world* w, uint64_t n, const uint32_t* ids, const float* force, const float* point, const float* torque) {
    return edit_host(w, EditKind::Forces, {n, ids, {force, point, torque}});
}
int32_t phys_set_body_poses_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* pos, const float* rot_ijkw) {
    return edit_device(w, EditKind::Poses, {n, ids, {pos, rot_ijkw, nullptr}});
}
int32_t phys_set_body_velocities_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* lin, const float* ang) {
    return edit_device(w, EditKind::Velocities, {n, ids, {lin, ang, nullptr}});
}
int32_t phys_apply_impulses_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* impulse, const float* point,
                                   const float* ang_impulse) {
    return edit_device(w, EditKind::Impulses, {n, ids, {impulse, point, ang_impulse}});
}
int32_t phys_apply_forces_device(phys_world* w, uint64_t n, const uint32_t* ids, const float* force, const float* point, const float* torque) {
    return edit_device(w, EditKind::Forces, {n, ids, {force, point, torque}});
}

// ids in any order, with repeats; an id that is not below n_owned: PHYS_ERR_OUT_OF_RANGE, nothing written
int32_t phys_get_body_states(phys_world* w, uint64_t n, const uint32_t* ids, float* pos_out, float* rot_out, float* lin_out, float* ang_out) {
    ENTER(w);
    PHYS_NO_EDITS_WHEN_SHARDED(w);
    if (n == 0) return PHYS_OK;
    if (n >= (1ull << 31)) return fail(PHYS_ERR_INVALID_ARG, "phys_get_body_states: n must be below 2^31");
    if (!ids) return fail(PHYS_ERR_INVALID_ARG, "phys_get_body_states: null ids");
    for (uint64_t k = 0; k < n; ++k)
        if (ids[k] >= w->n_owned) return fail(PHYS_ERR_OUT_OF_RANGE, "phys_get_body_states: body index out of range");
    Staging in{w, w->stage}, out{w, w->rc_out};
    const auto s_ids = in.add(ids, n);
    const auto s_pos = out.add(pos_out, 3 * n), s_rot = out.add(rot_out, 4 * n), s_lin = out.add(lin_out, 3 * n), s_ang = out.add(ang_out, 3 * n);
    PHYS_TRY(in.reserve());
    PHYS_TRY(out.reserve());
    PHYS_TRY(in.copy(hipMemcpyHostToDevice));
    PHYS_TRY(launch_get_states(w, n, in.at(s_ids), out.at(s_pos), out.at(s_rot), out.at(s_lin), out.at(s_ang)));
    PHYS_TRY(out.copy(hipMemcpyDeviceToHost));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}
int32_t phys_get_body_states_device(phys_world* w, uint64_t n, const uint32_t* ids, float* pos_out, float* rot_out, float* lin_out,
                                    float* ang_out) {
    ENTER(w);
    PHYS_NO_EDITS_WHEN_SHARDED(w);
    if (n == 0) return PHYS_OK;
    if (n >= (1ull << 31)) return fail(PHYS_ERR_INVALID_ARG, "phys_get_body_states_device: n must be below 2^31");
    if (!ids) return fail(PHYS_ERR_INVALID_ARG, "phys_get_body_states_device: null ids");
    return launch_get_states(w, n, ids, pos_out, rot_out, lin_out, ang_out);
}

int32_t phys_set_global_ids(phys_world* w, const uint32_t* global_ids) {
    ENTER(w);
    if (!global_ids) return fail(PHYS_ERR_INVALID_ARG, "null ids");
    PHYS_HIP_TRY(hipMemcpyAsync(w->global_id.p, global_ids, 4 * w->n_owned, hipMemcpyHostToDevice, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}

int32_t phys_halo_pack(phys_world* w, float x_lo, float x_hi, float reach, void* dev_records_out, uint64_t cap,
                       uint64_t* n_records) {
    ENTER(w);
    return halo_pack(w, x_lo, x_hi, reach, dev_records_out, cap, n_records);
}
int32_t phys_halo_pairs(phys_world* w, const void* dev_remote_records, uint64_t n_remote, uint64_t skip_first,
                        uint64_t skip_count, uint64_t* n_cross_pairs) {
    ENTER(w);
    return halo_pairs(w, dev_remote_records, n_remote, skip_first, skip_count, n_cross_pairs);
}
int32_t phys_set_slab(phys_world* w, float x_lo, float x_hi, float reach) {
    ENTER(w);
    if (!(x_lo < x_hi) || !(reach > 0.0f)) return fail(PHYS_ERR_INVALID_ARG, "slab needs x_lo < x_hi and reach > 0");
    w->slab_lo = x_lo; w->slab_hi = x_hi; w->slab_reach = reach;
    return PHYS_OK;
}
int32_t phys_halo_pack_bodies(phys_world* w, void* dev_records_out, uint64_t cap) {
    ENTER(w);
    return halo_pack_bodies(w, dev_records_out, cap);
}
int32_t phys_halo_pack_bodies_face(phys_world* w, void* dev_records_out, uint64_t cap, int32_t face) {
    ENTER(w);
    const float far = 3.0e38f;
    return halo_pack_bodies_faces(w, dev_records_out, cap, face > 0 ? -far : w->slab_lo, face < 0 ? far : w->slab_hi);
}
int32_t phys_halo_unpack_ghosts(phys_world* w, const void* dev_records, uint64_t n_records, uint64_t skip_first,
                                uint64_t skip_count) {
    ENTER(w);
    return halo_unpack_ghosts(w, dev_records, n_records, skip_first, skip_count);
}
int32_t phys_get_global_ids(phys_world* w, uint32_t* out) {
    ENTER(w);
    if (!out) return fail(PHYS_ERR_INVALID_ARG, "null output");
    if (w->n) PHYS_HIP_TRY(hipMemcpyAsync(out, w->global_id.p, 4 * w->n, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    return PHYS_OK;
}
int32_t phys_get_cross_pairs(phys_world* w, uint32_t* pairs_out, uint64_t cap, uint64_t* n_pairs) {
    ENTER(w);
    if (!n_pairs) return fail(PHYS_ERR_INVALID_ARG, "null n_pairs");
    PHYS_TRY(fetch_counters(w));
    const uint64_t m = w->h_counters->n_cross_pairs < w->max_cross_pairs ? w->h_counters->n_cross_pairs : w->max_cross_pairs;
    *n_pairs = m;
    if (pairs_out && m) {
        std::vector<uint32_t> raw(2 * m);
        PHYS_HIP_TRY(hipMemcpy(raw.data(), w->cross_pairs.p, 8 * m, hipMemcpyDeviceToHost));
        sort_pairs(raw.data(), m, pairs_out, cap);
    }
    return PHYS_OK;
}

}  // extern "C"
