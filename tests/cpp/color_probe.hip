// color_probe.hip — test-only read-out of the colouring stage and the row sort (coloring.hip, cluster.hip's sort) for
// tests/test_gpu_coloring.py. Built as tests/cpp/libcolor_probe.so by the `color_probe` rule of
// physics_amd/csrc/Makefile, with that Makefile's HIPFLAGS, and linked against libphysics_hip.so. It has no kernel of its
// own and nothing of it is part of libphysics_hip.so: it only copies what the world holds to host arrays, and evaluates
// plan.hpp's plan_coloring - pure host code, the very function enqueue_update calls - on the world as it stands.
//
// Every entry point returns 0, -1 for arguments it refuses, or the hipError_t of the call that failed.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../physics_amd/csrc/kernels.hpp"

using namespace phys;

namespace {
constexpr int32_t kBadArg = -1;
#define CP_TRY(expr)                                  \
    do {                                              \
        const hipError_t _e = (expr);                 \
        if (_e != hipSuccess) {                       \
            (void)hipGetLastError();                  \
            return (int32_t)_e;                       \
        }                                             \
    } while (0)

struct DeviceKeeper {
    int prev = -1;
    DeviceKeeper() { if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; } }
    ~DeviceKeeper() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

// what the Python side lays its views over (tests/color_probe.py holds the same two lists)
struct color_probe_sizes {
    uint64_t n, n_owned, max_manifolds;
    uint32_t cluster_count, cluster_slots, cluster_dynamic, counters_bytes;
};
struct color_probe_plan {
    uint32_t path;  // 0 Small, 1 Known, 2 Probe (plan.hpp ColorPath)
    uint32_t rounds, round_blocks, sort_blocks, cluster_sort_blocks, cluster_key_blocks;
    uint32_t full, rebuild, stamp, wants_cluster;
    // the hint the plan was made from
    uint32_t hint_valid, hint_n_manifolds, hint_color_rounds, hint_full_rounds, hint_n_new, hint_n_colors;
    uint64_t color_epoch;
};
// offsets of the StepCounters members the checker reads (bytes), so that Python never guesses the layout
struct color_probe_layout {
    uint32_t n_manifolds, unc_count, n_uncolored, n_colors, color_rounds, overflow, n_new_manifolds, color_count, color_start, size;
};

extern "C" {

void color_probe_layout_get(color_probe_layout* out) {
    out->n_manifolds = (uint32_t)offsetof(StepCounters, n_manifolds);
    out->unc_count = (uint32_t)offsetof(StepCounters, unc_count);
    out->n_uncolored = (uint32_t)offsetof(StepCounters, n_uncolored);
    out->n_colors = (uint32_t)offsetof(StepCounters, n_colors);
    out->color_rounds = (uint32_t)offsetof(StepCounters, color_rounds);
    out->overflow = (uint32_t)offsetof(StepCounters, overflow);
    out->n_new_manifolds = (uint32_t)offsetof(StepCounters, n_new_manifolds);
    out->color_count = (uint32_t)offsetof(StepCounters, color_count);
    out->color_start = (uint32_t)offsetof(StepCounters, color_start);
    out->size = (uint32_t)sizeof(StepCounters);
}

// plan_coloring on hand-made inputs: needs no world and no GPU (tests/test_color_ref_cpu.py holds the case tables to it)
int32_t color_probe_plan_of(uint32_t flags, uint32_t solver_iterations, uint64_t n_owned, uint64_t max_manifolds, uint32_t cluster_count,
                            uint32_t ctab_valid, uint64_t color_epoch, uint32_t hint_valid, uint32_t hint_n_manifolds,
                            uint32_t hint_color_rounds, uint32_t hint_full_rounds, uint32_t hint_n_colors, color_probe_plan* out) {
    if (!out) return kBadArg;
    PlanInputs in;
    in.flags = flags; in.solver_iterations = solver_iterations;
    in.n = n_owned; in.n_owned = n_owned; in.max_manifolds = max_manifolds;
    in.cluster_count = cluster_count; in.ctab_valid = ctab_valid != 0; in.color_epoch = color_epoch;
    StepHint h;
    h.valid = hint_valid != 0; h.n_manifolds = hint_n_manifolds; h.color_rounds = hint_color_rounds; h.full_rounds = hint_full_rounds;
    h.n_colors = hint_n_colors;
    const ColorPlan p = plan_coloring(in, h, DebugSwitches());
    std::memset(out, 0, sizeof(*out));
    out->path = p.path == ColorPath::Small ? 0u : (p.path == ColorPath::Known ? 1u : 2u);
    out->rounds = p.rounds; out->round_blocks = p.round_blocks; out->sort_blocks = p.sort_blocks;
    out->cluster_sort_blocks = p.cluster_sort_blocks; out->cluster_key_blocks = p.cluster_key_blocks;
    out->full = p.full; out->rebuild = p.rebuild; out->stamp = p.stamp; out->wants_cluster = p.wants_cluster;
    out->hint_valid = h.valid; out->hint_n_manifolds = h.n_manifolds; out->hint_color_rounds = h.color_rounds;
    out->hint_full_rounds = h.full_rounds; out->hint_n_new = h.n_new; out->hint_n_colors = h.n_colors;
    out->color_epoch = color_epoch;
    return 0;
}

int32_t color_probe_sizes_get(phys_world* w, color_probe_sizes* out) {
    if (!w || !out) return kBadArg;
    out->n = w->n; out->n_owned = w->n_owned; out->max_manifolds = w->max_manifolds;
    out->cluster_count = w->cluster_count; out->cluster_slots = w->cluster_slots; out->cluster_dynamic = w->cluster_dynamic;
    out->counters_bytes = (uint32_t)sizeof(StepCounters);
    return 0;
}

// The ColorPlan the NEXT phys_update will make, to be called on an idle stream (behind phys_sync) immediately before it: the
// snapshots in flight are adopted exactly as enqueue_update's first line does (adopting twice changes nothing), and
// plan_coloring gets the members of the world it reads - the ones abi.hip's plan_inputs copies - and the world's hint.
int32_t color_probe_next_plan(phys_world* w, color_probe_plan* out) {
    if (!w || !out) return kBadArg;
    DeviceKeeper keep;
    CP_TRY(hipSetDevice(w->device));
    CP_TRY(hipStreamSynchronize(w->stream));
    poll_snapshots(w);
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
    const StepHint& h = w->hint;
    const ColorPlan p = plan_coloring(in, h, debug_switches());
    std::memset(out, 0, sizeof(*out));
    out->path = p.path == ColorPath::Small ? 0u : (p.path == ColorPath::Known ? 1u : 2u);
    out->rounds = p.rounds; out->round_blocks = p.round_blocks; out->sort_blocks = p.sort_blocks;
    out->cluster_sort_blocks = p.cluster_sort_blocks; out->cluster_key_blocks = p.cluster_key_blocks;
    out->full = p.full; out->rebuild = p.rebuild; out->stamp = p.stamp; out->wants_cluster = p.wants_cluster;
    out->hint_valid = h.valid; out->hint_n_manifolds = h.n_manifolds; out->hint_color_rounds = h.color_rounds;
    out->hint_full_rounds = h.full_rounds; out->hint_n_new = h.n_new; out->hint_n_colors = h.n_colors;
    out->color_epoch = w->color_epoch;
    return 0;
}

// What the last update left: the counters (counters_bytes), then man_a / man_b / man_color / row_src for the first `cap`
// manifolds - the caller sizes them from a first call with cap == 0, which fills the counters only - and `used` (n words of 64
// bits). Cluster worlds: cluster_slot (n words) and seg_start (cluster_count * 64 + 1 words: k_solve_cluster reads the rows of
// cluster k and colour c as [seg_start[k * 64 + c], seg_start[k * 64 + c + 1])); both may be null.
int32_t color_probe_read(phys_world* w, void* counters, uint64_t cap, uint32_t* man_a, uint32_t* man_b, uint32_t* man_color,
                         uint32_t* row_src, unsigned long long* used, uint32_t* cluster_slot, uint32_t* seg_start) {
    if (!w || !counters) return kBadArg;
    if (cap > w->max_manifolds) return kBadArg;
    if (cap && (!man_a || !man_b || !man_color || !row_src)) return kBadArg;
    if (!w->counters.p) return kBadArg;  // a world without collisions
    DeviceKeeper keep;
    CP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    CP_TRY(hipStreamSynchronize(s));
    CP_TRY(hipMemcpyAsync(counters, w->counters.p, sizeof(StepCounters), hipMemcpyDeviceToHost, s));
    if (cap) {
        CP_TRY(hipMemcpyAsync(man_a, w->man_a.p, cap * 4, hipMemcpyDeviceToHost, s));
        CP_TRY(hipMemcpyAsync(man_b, w->man_b.p, cap * 4, hipMemcpyDeviceToHost, s));
        CP_TRY(hipMemcpyAsync(man_color, w->man_color.p, cap * 4, hipMemcpyDeviceToHost, s));
        CP_TRY(hipMemcpyAsync(row_src, w->row_src.p, cap * 4, hipMemcpyDeviceToHost, s));
    }
    if (used) {
        if (!w->color_state.p) return kBadArg;
        CP_TRY(hipMemcpyAsync(used, w->color_state.p, (size_t)w->n * 8, hipMemcpyDeviceToHost, s));
    }
    if (cluster_slot) {
        if (!w->cluster_slot.p || w->cluster_slot.n < w->n) return kBadArg;
        CP_TRY(hipMemcpyAsync(cluster_slot, w->cluster_slot.p, (size_t)w->n * 4, hipMemcpyDeviceToHost, s));
    }
    if (seg_start) {
        const size_t words = (size_t)w->cluster_count * PHYS_MAX_COLORS + 1;
        if (!w->seg_start.p || w->seg_start.n < words) return kBadArg;
        CP_TRY(hipMemcpyAsync(seg_start, w->seg_start.p, words * 4, hipMemcpyDeviceToHost, s));
    }
    CP_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
