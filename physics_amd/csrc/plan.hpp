// plan.hpp — which kernels one update launches, and how large: every such decision of the library, as pure functions of
// (PlanInputs, StepHint, DebugSwitches). Nothing of HIP in here: a host compiler reads it alone, and tests/cpp/plan_probe.cpp
// holds every threshold to a table (tests/test_plan_cpu.py). The launch_* functions take their part of the plan and only
// launch. Every path gives the same bits: a plan is a matter of speed, never of correctness.
// What is decided once per body set, static set or constraint list - and the one per-update decision that needs the cluster
// geometry, plan_dynamic_clusters - is in setup.hpp, in the same style.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <optional>

#include "../../include/physics_hip.h"

namespace phys {

constexpr int kMaxColors = 64;         // == PHYS_MAX_COLORS of include/spec/contact_solve.h
constexpr int kColorCachePeriod = 64;  // == PHYS_COLOR_CACHE_PERIOD (both held by kernels.hpp)
constexpr uint32_t kHandoffIterationsEnd = 1000;  // solver_iterations from here on: per colour only (update counts are 16-bit: records.hpp)

// launch-size hints taken from an EARLIER step's counters (asynchronous read-back); never needed for
// correctness
struct StepHint {
    bool valid = false;
    uint32_t n_manifolds = 0, n_colors = 0, n_pairs = 0, max_region = 0, n_used_buckets = 0, n_contacts = 0;
    uint32_t n_active = 0;         // owned bodies with a manifold (0 = unknown)
    uint32_t color_rounds = 0;     // max over the recent INCREMENTAL updates
    uint32_t full_rounds = 0;      // rounds of the last full re-colouring (0 = unknown)
    uint32_t recent_rounds[8] = {};
    uint32_t recent_pos = 0;
    uint32_t n_new = 0xFFFFFFFFu;  // most manifolds without a kept colour in one of the recent incremental updates (~0: unknown)
    uint32_t recent_new[8] = {};
    uint32_t color_count[kMaxColors] = {};
};

// PHYS_DEBUG_* switches, parsed once per process by the first debug_switches() (abi.hip). Unset: false / 0 / nullopt
struct DebugSwitches {
    bool no_cluster = false, cluster_dynamic = false, no_flow_preference = false, flow_stall = false;
    std::optional<uint64_t> cluster_min, flow_max;
    std::optional<int> clusters_per_cu;
    uint64_t cluster_cap = 0, flow_quad_max = 0, ctab_slots = 0;
    uint32_t flow_epoch = 0;
    int np_threads = 0, pair_lanes = 0, brick_stage = 0;
    bool raycast_stats = false;  // PHYS_DEBUG_RAYCAST_STATS: phys_raycast counts the cells and candidates its rays visit (stderr)
    std::optional<bool> flow_pipeline, np_early_probe;  // the value begins with '1'
    std::optional<bool> color_kernel_lane;              // the value begins with 'l' (four lanes otherwise)
    std::optional<bool> pair_kernel_brick;              // brick, unless the value is 'b' followed by anything but 'r'
};

// what the decisions read of the world (abi.hip plan_inputs)
struct PlanInputs {
    uint32_t flags = 0, solver_iterations = 0;  // phys_config
    uint64_t n = 0, n_owned = 0, max_manifolds = 0;
    uint32_t grid_table_size = 0;
    int cus = 0;             // CUs of the device (phys_create)
    bool exclusive = false;  // gpu_is_exclusive: PHYS_FLAG_EXCLUSIVE_GPU, no PHYS_FLAG_SHARED_GPU, no other world on the device
    bool warm = false;
    bool flow_vel = false;   // the dataflow kernels' granules exist (collision_alloc)
    uint32_t cluster_count = 0;
    bool cluster_dynamic = false;
    bool ctab_valid = false;
    uint64_t color_epoch = 0;
    // the instances this world runs. statics and np_items are the narrow phase's, so of this update only behind
    // launch_static_pairs, which sizes the (body, static) pairs
    bool statics = false, capsules = false, filters = false, materials = false;
    uint64_t np_items = 0;   // work items of k_narrowphase: ground tests + pair capacity + static pair capacity
};

// ---- kernel geometry the grids below are computed from (the kernels are written against the same constants) ----------
constexpr int kPairThreads = 256;                                                  // broadphase.hip: k_find_pairs*
constexpr int kRegX = 6, kRegY = 6, kRegZ = 5, kRegCells = kRegX * kRegY * kRegZ;  // 180: cells of a brick's region (k_find_pairs_brick)
constexpr int kColorThreads = 1024;      // coloring.hip
constexpr int kSmallTrips = 40;          // k_color_small: manifolds per thread kept in registers: 40 x 1024 = the `small` limit
constexpr int kSortBlocksMax = 512;      // most workgroups of the hist / place kernels (the plan picks nb <= this)
constexpr int kSortChunk = 4096;         // manifolds per workgroup trip of the colour sort
constexpr int kKeysItems = 4;            // cluster.hip k_cluster_keys: manifolds per lane and trip
constexpr int kQuadRowsPerGroup = 64;    // solver.hip k_solve_color_quad
constexpr int kEventThreads = 256;       // events.hip

// ---- thresholds (DESIGN.md section 19 has them in one table) --------------------------------------------------------------
constexpr uint32_t kSlotGridMaxBodies = 32768;  // beyond, streaming the sorted boxes is as fast
constexpr uint64_t kClusterMinBodies = 32768;   // below: the dataflow kernels win anyway (few launches' worth of rows)
// measured with tools/cluster_crossover.py (solve + rows, ms: cluster / four-lane dataflow kernel with statically dealt items):
// mixed piles 91k manifolds 0.518 / 0.353, 145k 0.519 / 0.486, 155k 0.535 / 0.494, 216k (C3) 0.576 / 0.696; towers 92k 0.647 /
// 0.415, 182k 0.699 / 0.700, 256k 0.712 / 0.984 - the cluster kernel's time is its chain (nearly the same at every size), the
// dataflow kernel's grows with the rows
constexpr uint64_t kClusterMinManifolds = 170000;
constexpr long long kFlowTimeoutTicks = 300000000ll;  // 3 s of the 100 MHz wall clock (fault injection: 20 ms)
constexpr uint64_t kFlowMaxManifolds = 400000;        // above: one launch per colour streams better
// below: four lanes per manifold (k_solve_flow_quad). Measured again with its statically dealt items (tools/cluster_crossover.py
// --path flow, solve ms quad / one lane): towers 92k manifolds 0.371 / 0.466, 182k 0.645 / 0.670, 256k 0.914 / 0.903; mixed piles
// 91k 0.308 / 0.405, 155k 0.444 / 0.502 (round 2, with tickets: 45k +13 %, 108k -32 %)
constexpr uint64_t kFlowQuadMaxManifolds = 200000;
constexpr uint32_t kTailMax = 512;  // manifolds per colour the single-workgroup tail should take: one trip of the workgroup
// four lanes per manifold while a colour is too small to fill the chip with one lane per manifold (measured
// crossover ~30k rows: 15k rows 10.2 vs 11.9 us per launch, 53k rows 18.3 vs 16.7, 85k rows 21.5 vs 18.7)
constexpr uint32_t kQuadColorMaxRows = 32768;
// records staged per brick: at most what one workgroup may have of a CU's LDS
constexpr uint32_t kBrickCapMax = 5000;  // 137 KiB
// persistent workgroups of the brick kernel: at most seven per CU (66 registers: seven waves per SIMD). Measured, us (C4 / 1M
// cubes in mid-fall / C5): 3 per CU 173 / 145 / 74, 4: 137 / 114 / 72, 5: 117 / 100 / 69, 6: 105 / 89 / 70, 7 (small stage):
// 103 / 83 / -; asked for 8 (not all resident: the late ones start on a drained chip) 131 / 109 / 69
constexpr size_t kBrickPerCuMax = 7;

// Which single-launch solver for a dense scene whose GPU is the world's alone (PHYS_FLAG_EXCLUSIVE_GPU: the dataflow kernel may
// then fill the chip with three workgroups per CU, like the cluster kernel). Fitted to measurements of this build, ms per
// sweep: the four-lane dataflow kernel at 672 workgroups 8.4e-8 M + 1.86e-8 K + 0.0009 C (C3 0.325 ms per solve, a 182k
// tower 0.380, the 1M cubes in mid-fall 0.405, C5 1.07); the cluster kernel max(0.0041 C, 6.9e-8 M) + 10 % (C3 0.513, the
// tower 0.636, the 1M cubes 0.235, C5 0.63): rows cost the dataflow kernel throughput, colours cost the cluster kernel
// its chain. (Both give the same bits: the choice may change from update to update.)
inline bool flow_quad_beats_cluster(uint32_t manifolds, uint32_t contacts, uint32_t colors) {
    if (!colors || !contacts) return false;
    const double flow = 8.4e-8 * manifolds + 1.86e-8 * contacts + 0.0009 * colors;
    const double cluster = 1.1 * std::max(0.0041 * colors, 6.9e-8 * manifolds);
    return flow < cluster;
}

// ---- broad phase: the pair search ---------------------------------------------------------------------------------------
enum class PairKernel { Slots, Brick128, Brick256, Lanes4, Lanes1 };
struct PairPlan {
    PairKernel kernel = PairKernel::Slots;
    uint32_t cap = 0;  // brick: records staged per brick
    size_t lds = 0;    // brick: dynamic LDS bytes
    uint32_t wgs = 0;
};
inline PairPlan plan_pairs(const PlanInputs& in, const StepHint& h, const DebugSwitches& dbg) {
    PairPlan p;
    const uint32_t n = (uint32_t)in.n;
    const uint32_t per_four_lanes = (uint32_t)(((uint64_t)n * 4 + kPairThreads - 1) / kPairThreads);
    if (n <= kSlotGridMaxBodies) {  // slot grid: two launches for the whole broad phase
        p.kernel = PairKernel::Slots;
        p.wgs = per_four_lanes;
        return p;
    }
    // small scenes are latency-bound: 4 lanes per body shorten the dependent chain; large scenes are
    // throughput-bound: one lane per body does the least total work
    // (measured: one lane per body is the faster one already at 100k bodies - C3: 0.051 against 0.089 ms)
    // PHYS_DEBUG_PAIR_LANES=1|4 and PHYS_DEBUG_PAIR_KERNEL=body / brick force one (measurements; same pair set)
    // The brick kernel wins where the grid is sparsely filled - lattices, stacks of aligned boxes: many bricks of few
    // records (C4 204 -> 119 us, C5 135 -> 73) - and loses where cells are crowded (one tumbled cube sets the cell size for
    // everybody: 1M falling cubes 89 -> 102 us, C3 51 -> 82: few bricks, each a long walk for the one workgroup that has
    // it). Crowding = bodies per bucket in use, counted by k_cell_assign of an earlier update.
    const bool crowded = h.valid && h.n_used_buckets && (uint64_t)in.n * 10ull > (uint64_t)h.n_used_buckets * 21ull;
    const bool brick = dbg.pair_kernel_brick.value_or(!crowded);
    if (brick && !dbg.pair_lanes) {
        const uint32_t n_bricks = in.grid_table_size >> 6;
        // records staged per brick: a quarter more than the largest region of an earlier update (C4: ~400 records, a pile
        // of tumbled cubes: ~1500), 1024 while nothing is known
        uint32_t cap = h.valid && h.max_region ? h.max_region + h.max_region / 4 : 1024u;
        cap = std::min(std::max((cap + 63u) & ~63u, 256u), kBrickCapMax);
        const size_t dyn = (size_t)cap * 28;
        // few pairs per body (of an earlier update): the small stage, which leaves room for a seventh workgroup per CU
        // (PHYS_DEBUG_BRICK_STAGE=128|256 forces one: measurements)
        const bool small_stage = dbg.brick_stage ? dbg.brick_stage == 128 : (h.valid && (uint64_t)h.n_pairs < 3ull * in.n);
        const size_t fixed = (kPairThreads / 64) * (small_stage ? 128 : 256) * 8 + kRegCells * 8 + 64;
        // persistent workgroups, as many as are resident at once (the LDS decides), never more than there are bricks
        const uint32_t per_cu = (uint32_t)std::min<size_t>(kBrickPerCuMax, (160 * 1024) / (((dyn + fixed) + 1023) / 1024 * 1024));
        uint32_t wgs = 256u * std::max(per_cu, 1u);
        while (wgs > n_bricks) wgs >>= 1;
        p.kernel = small_stage ? PairKernel::Brick128 : PairKernel::Brick256;
        p.cap = cap;
        p.lds = dyn;
        p.wgs = wgs;
        return p;
    }
    if (dbg.pair_lanes ? dbg.pair_lanes == 4 : n <= 65536u) {
        p.kernel = PairKernel::Lanes4;
        p.wgs = per_four_lanes;
    } else {
        p.kernel = PairKernel::Lanes1;
        p.wgs = (n + kPairThreads - 1) / kPairThreads;
    }
    return p;
}

// ---- narrow phase ---------------------------------------------------------------------------------------------------------
struct NarrowPlan {
    int threads = 512;         // 128 or 512: only the two are built
    uint32_t early_probe = 0;  // the colour-table entry of a pair is asked for ahead of the shape test
    bool statics = false, capsules = false, filters = false;  // the instance
    uint32_t blocks = 1;
};
inline NarrowPlan plan_narrowphase(const PlanInputs& in, const StepHint& h, const DebugSwitches& dbg) {
    NarrowPlan p;
    // ... where at least half of the pairs become manifolds. PHYS_DEBUG_NP_EARLY_PROBE=0 / 1 forces it (measurements; same bits)
    p.early_probe = dbg.np_early_probe.value_or(!h.valid || 2ull * h.n_manifolds >= (uint64_t)h.n_pairs);
    // 128 threads only while the whole stage is a few workgroups (C2: 10k manifolds); measured at 230k manifolds (C3):
    // 0.175 ms with 128 threads, 0.133 with 256; at 2.9M (C5): 0.86 vs 0.55 (round 2)
    const bool few = h.valid ? h.n_manifolds <= 32768u : (uint32_t)in.n <= 200000u;
    // Workgroup shape (all variants: same manifolds, emission order is arbitrary anyway). A trip ends in one reservation
    // behind two barriers, and the waves a CU holds are what hides a trip's round trips from each other; the in-place
    // clipper's LDS slice (33 dwords per lane) admits 16 waves per CU at 118 registers. Measured, ms per update
    // (C5 / 1M cubes in mid-fall / settled 1M pile / C3):
    //   256 threads, one item per lane (4 workgroups per CU)            0.251 / 0.081 / 0.812 / 0.091
    //   256 threads, two items per lane (151 registers: 12 waves)       0.230 / 0.067 / 0.917 / 0.093
    //   512 threads, one item (2 workgroups per CU, half the atomics)   0.206 / 0.069 / 0.836 / 0.075   <- the default
    //   1024 threads, one item (a barrier over 16 waves)                0.231 / 0.084 / 0.937 / 0.080
    // Only the two the library picks are built; PHYS_DEBUG_NP_THREADS=128|512 picks one by hand (any other value: 512).
    p.threads = (dbg.np_threads ? dbg.np_threads : (few ? 128 : 512)) == 128 ? 128 : 512;
    p.statics = in.statics; p.capsules = in.capsules; p.filters = in.filters;
    uint64_t blocks = (in.np_items + p.threads - 1) / p.threads;
    if (blocks > 256 * 16) blocks = 256 * 16;
    p.blocks = (uint32_t)blocks;
    return p;
}

// ---- colouring and the row sort ---------------------------------------------------------------------------------------------
enum class ColorPath {
    Small,  // one workgroup does the whole stage (k_color_small)
    Known,  // as many round launches as the last update of this kind needed, then k_color_finish
    Probe   // nothing is known about the scene yet: eight rounds at a time, and ask the device
};
struct ColorPlan {
    ColorPath path = ColorPath::Probe;
    uint32_t rounds = 0;         // Known: the round launches
    uint32_t round_blocks = 1;   // workgroups of a round
    uint32_t sort_blocks = 1;    // workgroups of the colour sort (hist / place): a power of two
    uint32_t cluster_sort_blocks = 1, cluster_key_blocks = 1;  // ... and of the cluster sort's place / keys kernels
    // a full colouring (the first update after phys_set_bodies: nothing to keep) needs far more rounds than an incremental one
    bool full = false;
    // every PHYS_COLOR_CACHE_PERIOD-th update the colour TABLE is rebuilt: emptied behind the narrow phase, which has taken
    // what it keeps from it already, and refilled by k_rows_build with every manifold of this update instead of the new ones
    // only. That purges the dead entries (chains never shrink otherwise) and changes no colour.
    bool rebuild = false;
    uint32_t stamp = 0;          // what this update's table entries are stamped with
    // the cluster solver is wanted for this update. Decided with the colouring because it decides the ORDER of the rows: by
    // (cluster, colour) instead of by colour. Dynamic clusters still have to agree (cluster_plan_dynamic).
    bool wants_cluster = false;
};
inline ColorPlan plan_coloring(const PlanInputs& in, const StepHint& h, const DebugSwitches& dbg) {
    ColorPlan p;
    uint64_t blocks64 = (in.max_manifolds + kColorThreads - 1) / kColorThreads;
    if (blocks64 > 512) blocks64 = 512;
    if (h.valid) {
        const uint64_t want = ((uint64_t)h.n_manifolds * 5 / 4 + kColorThreads) / kColorThreads;
        if (want < blocks64) blocks64 = want ? want : 1;
    }
    p.round_blocks = (uint32_t)blocks64;
    p.full = !in.ctab_valid;
    p.rebuild = p.full || (in.color_epoch % kColorCachePeriod) == 0;
    p.stamp = (uint32_t)in.color_epoch + 1u;
    const bool known = h.valid && (!p.full || h.full_rounds > 0);
    const bool small = h.valid && h.n_manifolds <= (uint32_t)(kSmallTrips * kColorThreads);
    p.path = small ? ColorPath::Small : (known ? ColorPath::Known : ColorPath::Probe);
    // as many launches as the last update of this kind needed; k_color_finish runs what is still missing over the
    // same lists (measured: handing it the second half of the rounds - one workgroup, ~10 us per round with a few
    // thousand manifolds left - is slower than the launches it saves, and far slower on a full re-colouring)
    if (p.path == ColorPath::Known) p.rounds = p.full ? h.full_rounds : h.color_rounds;
    // workgroups of the colour sort: sized from the hint (any value is correct: the kernels stride)
    uint32_t nb = kSortBlocksMax;
    if (h.valid) {
        const uint64_t want = ((uint64_t)h.n_manifolds * 5 / 4) / kSortChunk + 1;
        nb = 1;
        while (nb < want && nb < (uint32_t)kSortBlocksMax) nb <<= 1;
    }
    p.sort_blocks = nb;
    p.cluster_sort_blocks = p.round_blocks * (kColorThreads / 256);
    // (a trip of k_cluster_keys is 1024 manifolds: as many workgroups as the last known count needs, any number is correct)
    const uint64_t key_trips = h.valid ? ((uint64_t)h.n_manifolds * 5 / 4) / (256u * kKeysItems) + 1 : p.cluster_sort_blocks;
    p.cluster_key_blocks = (uint32_t)std::min<uint64_t>(p.cluster_sort_blocks, std::max<uint64_t>(1, key_trips));
    // PHYS_DEBUG_CLUSTER_MIN=<manifolds> moves the threshold (measurements; same bits either way).
    const bool cluster_forced = (in.flags & PHYS_FLAG_SOLVER_CLUSTER) != 0u;
    const uint64_t cluster_min = cluster_forced ? 0 : dbg.cluster_min.value_or(kClusterMinManifolds);
    // worth it where contacts are dense (C5: 11 rows per body): velocities stay in LDS for many rows each. Sparse piles
    // (the 1M-cube scene: 0.4-0.5 rows per body, contacts in the bottom layers only) leave most clusters idle and a few
    // overloaded - they keep the dataflow / per-colour kernels, which spread rows evenly over the chip
    // (dynamic clusters hold only the bodies that have manifolds: nothing idles, the row count alone decides)
    const bool dense = cluster_forced || dbg.cluster_min.has_value() || in.cluster_dynamic || 2ull * h.n_manifolds >= 3ull * in.n_owned;
    p.wants_cluster = (in.cluster_count > 0 || in.cluster_dynamic) && h.valid && !small && dense && h.n_manifolds >= cluster_min &&
                      !(in.flags & PHYS_FLAG_SOLVER_PER_COLOR) && in.solver_iterations > 0 && in.solver_iterations < kHandoffIterationsEnd &&
                      h.n_colors > 0;
    // ... unless the dataflow kernel is the faster one for this many rows and colours (flow_quad_beats_cluster; only where it
    // may take the whole chip: PHYS_FLAG_EXCLUSIVE_GPU, one world on the device). PHYS_DEBUG_NO_FLOW_PREFERENCE: never
    // (measurements, same bits)
    if (p.wants_cluster && !cluster_forced && !dbg.cluster_min.has_value() && !dbg.no_flow_preference && in.exclusive &&
        h.n_manifolds <= kFlowMaxManifolds && flow_quad_beats_cluster(h.n_manifolds, h.n_contacts, h.n_colors))
        p.wants_cluster = false;
    return p;
}

// ---- solver -----------------------------------------------------------------------------------------------------------------
enum class SolverPath { Cluster, FlowQuad, FlowLane, PerColor };
struct SolverPlan {
    SolverPath path = SolverPath::PerColor;
    bool materials = false;          // the material instances of every kernel of the stage
    uint32_t rows_blocks = 1;        // k_rows_build
    // fault injection for tests/test_gpu_full_size.py (PHYS_DEBUG_FLOW_STALL): one row gets a ticket nobody will ever publish, so
    // the bounded spin of the dataflow kernels must give up, flag the step (overflow bit 4) and let the launch end
    bool stall = false;
    long long timeout_ticks = kFlowTimeoutTicks;
    // Cluster: the all-or-nothing start inside the kernel, unless the GPU is this world's alone
    bool guarded = true;
    // FlowQuad / FlowLane: workgroups (the remaining items are taken by the same ones), and whether k_solve_flow looks one item ahead
    uint32_t items = 0, pipeline = 0;
    // PerColor: colours [0, big) get a launch each, four lanes per row or one; [big, n_colours) go through the single-workgroup tail
    uint32_t big = 0;
    bool color_quad[kMaxColors] = {};
    uint32_t color_blocks[kMaxColors] = {};
    bool flow() const { return path != SolverPath::PerColor; }  // the rows are built for a single-launch kernel
};
// Planned behind the colouring stage, from the hint as it is then: the first update after phys_set_bodies has adopted exact
// counters by that time. `cluster`: ColorPlan::wants_cluster, and the dynamic clusters agreed - this update's rows are in
// (cluster, colour) order.
inline SolverPlan plan_solver(const PlanInputs& in, const StepHint& h, const DebugSwitches& dbg, bool cluster) {
    SolverPlan p;
    p.materials = in.materials;
    const uint64_t cap = in.max_manifolds;
    const uint64_t m_hint = h.valid ? h.n_manifolds : cap;
    auto grid_for_count = [&](uint64_t count, uint64_t rows_per_group, uint64_t most) {
        uint64_t b = (count * 5 / 4 + rows_per_group - 1) / rows_per_group + 1;
        const uint64_t hi = (cap + rows_per_group - 1) / rows_per_group;
        if (b > hi) b = hi;
        if (b > most) b = most;
        return (uint32_t)(b ? b : 1);
    };
    p.rows_blocks = grid_for_count(m_hint, 256, 4096);
    p.stall = dbg.flow_stall;
    p.timeout_ticks = p.stall ? 2000000ll : kFlowTimeoutTicks;
    p.guarded = !in.exclusive;
    // the dataflow kernel wins while a colour class is too small to fill the chip (launch / latency bound);
    // beyond that the per-colour launches stream better. Both give the same bits, so the choice may change
    // from step to step.
    // PHYS_DEBUG_FLOW_MAX=<manifolds>: move the dataflow / per-colour crossover (measurements only; same bits either way)
    const uint64_t flow_max = dbg.flow_max.value_or(kFlowMaxManifolds);
    const bool flow = cluster || (in.flow_vel && h.valid && m_hint <= flow_max && in.solver_iterations > 0 && in.solver_iterations < kHandoffIterationsEnd);
    if (cluster) {
        p.path = SolverPath::Cluster;
        return p;
    }
    if (flow) {
        // about one wave per SIMD or less: waiting waves must not crowd out the ones that can run
        // four lanes per manifold while the hop latency is everything - and, where the launch may take the whole chip
        // (exclusive GPU: three workgroups per CU, 672 of them), all the way up: 155k manifolds 0.250 ms against 0.446 with
        // 224 workgroups, C3's 216k 0.325 (cluster kernel 0.513), the 1M cubes' 379k 0.405 (cluster kernel 0.235)
        const bool quad = m_hint <= (dbg.flow_quad_max ? dbg.flow_quad_max : (in.exclusive ? kFlowMaxManifolds : kFlowQuadMaxManifolds));
        const uint32_t sweeps = in.solver_iterations + (in.warm ? 1u : 0u);
        const uint32_t threads = 256u;
        const uint32_t rows_per_item = quad ? threads / 4 : threads;
        uint64_t items = (uint64_t)sweeps * ((m_hint * 5 / 4 + rows_per_item - 1) / rows_per_item) + 1;
        // statically dealt items need every workgroup running: a third of the chip's slots by default (beside other
        // streams' kernels), seven eighths of them - the cluster kernel's share - where the GPU is this world's alone
        // (small scenes are a chain of hand-offs, not throughput: C2's 10k manifolds 0.053 ms at 224 workgroups, 0.058 at 672)
        const uint64_t most = quad ? (in.exclusive && m_hint > 32768u ? (uint64_t)(3 * (in.cus - in.cus / 8)) : 224) : 256;
        if (items > most) items = most;
        // look one work item ahead (k_solve_flow) while a colour class keeps a good part of the launch busy; below that the
        // solve is a chain of hand-offs and an item held ahead only waits (C3: 16k rows per colour, 65k lanes: +10 %;
        // 1M cubes: 41k rows per colour: -10 %). PHYS_DEBUG_FLOW_PIPELINE=0/1 forces it (measurements; same bits).
        const uint64_t per_color = m_hint / (h.valid && h.n_colors ? h.n_colors : 1u);
        p.path = quad ? SolverPath::FlowQuad : SolverPath::FlowLane;
        p.items = (uint32_t)items;
        p.pipeline = (uint32_t)dbg.flow_pipeline.value_or(4 * per_color >= threads * items);
        return p;
    }
    p.path = SolverPath::PerColor;
    if (h.valid) {
        p.big = h.n_colors;
        while (p.big > 0 && h.color_count[p.big - 1] <= kTailMax) --p.big;
        if (h.n_colors - p.big < 2) p.big = h.n_colors;  // a tail of one colour is just a slower launch
    }
    // PHYS_DEBUG_COLOR_KERNEL=lane / quad: one of them for every colour (A/B measurements, parity tests)
    for (uint32_t col = 0; col < p.big; ++col) {
        p.color_quad[col] = !dbg.color_kernel_lane.value_or(h.color_count[col] > kQuadColorMaxRows);
        p.color_blocks[col] = p.color_quad[col] ? grid_for_count(h.color_count[col], kQuadRowsPerGroup, 16384)
                                                : grid_for_count(h.color_count[col], 256, 4096);
    }
    return p;
}

// ---- contact events: any grid is correct (the kernels stride); sized from an earlier update's count where one is known -----
inline uint32_t plan_event_blocks(const PlanInputs& in, const StepHint& h) {
    const uint64_t m_guess = h.valid ? (uint64_t)h.n_manifolds * 5 / 4 + kEventThreads : in.max_manifolds;
    const uint64_t blocks = (std::min<uint64_t>(m_guess, in.max_manifolds) + kEventThreads - 1) / kEventThreads;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, 2048));
}

}  // namespace phys
