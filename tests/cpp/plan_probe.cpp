// plan_probe.cpp — the per-update planner (physics_amd/csrc/plan.hpp) against a table of cases. Built by a host compiler
// alone (tests/test_plan_cpu.py); exits non-zero at the first mismatch. The expected values were worked out by hand from
// the launch functions as they stood before the planner existed (launch_broadphase, launch_narrowphase, launch_coloring,
// launch_solver, launch_solve_cluster, launch_events), every boundary on both sides - never by running the planner.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../physics_amd/csrc/plan.hpp"

using namespace phys;

static int g_checks = 0;
#define CHECK(what, got, want)                                                                                          \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                  \
        if (g_ != w_) {                                                                                                 \
            std::printf("MISMATCH %s:%d  %s: %s = %lld, expected %lld\n", __FILE__, __LINE__, what, #got, g_, w_);      \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)

// a dense world of n bodies on a 256-CU device, as collision_alloc sizes it; no hint, no switch
static PlanInputs world(uint64_t n) {
    PlanInputs in;
    in.flags = PHYS_FLAG_COLLISIONS | PHYS_FLAG_GROUND_PLANE;
    in.solver_iterations = 8;
    in.n = in.n_owned = n;
    in.max_manifolds = 17 * n;
    in.grid_table_size = 1u << 20;  // 16384 bricks
    in.cus = 256;
    in.warm = true;
    in.flow_vel = true;
    in.ctab_valid = true;
    in.color_epoch = 5;
    in.np_items = n + 8 * n;
    return in;
}
static StepHint hint(uint32_t manifolds) {
    StepHint h;
    h.valid = true;
    h.n_manifolds = manifolds;
    h.n_pairs = manifolds;
    h.n_contacts = 3 * manifolds;
    h.n_colors = 10;
    h.color_rounds = 5;
    return h;
}

static bool same(const PairPlan& a, const PairPlan& b) { return a.kernel == b.kernel && a.cap == b.cap && a.lds == b.lds && a.wgs == b.wgs; }
static bool same(const NarrowPlan& a, const NarrowPlan& b) {
    return a.threads == b.threads && a.early_probe == b.early_probe && a.statics == b.statics && a.capsules == b.capsules &&
           a.filters == b.filters && a.blocks == b.blocks;
}
static bool same(const ColorPlan& a, const ColorPlan& b) {
    return a.path == b.path && a.rounds == b.rounds && a.round_blocks == b.round_blocks && a.sort_blocks == b.sort_blocks &&
           a.cluster_sort_blocks == b.cluster_sort_blocks && a.cluster_key_blocks == b.cluster_key_blocks && a.full == b.full &&
           a.rebuild == b.rebuild && a.stamp == b.stamp && a.wants_cluster == b.wants_cluster;
}
static bool same(const SolverPlan& a, const SolverPlan& b) {
    return a.path == b.path && a.materials == b.materials && a.rows_blocks == b.rows_blocks && a.stall == b.stall &&
           a.timeout_ticks == b.timeout_ticks && a.guarded == b.guarded && a.items == b.items && a.pipeline == b.pipeline &&
           a.big == b.big && !std::memcmp(a.color_quad, b.color_quad, sizeof a.color_quad) &&
           !std::memcmp(a.color_blocks, b.color_blocks, sizeof a.color_blocks);
}

static void pairs() {
    const DebugSwitches off;
    const StepHint none;
    {   // the slot grid up to 32768 bodies; four lanes per body
        const PairPlan p = plan_pairs(world(32768), none, off);
        CHECK("slots", p.kernel, PairKernel::Slots); CHECK("slots", p.wgs, 512);
        // beyond, without a hint: the brick kernel, large stage, 1024 records: 28672 + 9696 bytes -> 38 KiB -> 4 per CU
        const PairPlan q = plan_pairs(world(32769), none, off);
        CHECK("brick", q.kernel, PairKernel::Brick256); CHECK("brick", q.cap, 1024); CHECK("brick", q.lds, 28672); CHECK("brick", q.wgs, 1024);
    }
    {   // crowding: bodies * 10 > buckets in use * 21
        StepHint h = hint(100000);
        h.n_pairs = 300000;  // not fewer than 3 n: the large stage
        h.n_used_buckets = 47619;
        const PairPlan p = plan_pairs(world(100000), h, off);
        CHECK("crowded", p.kernel, PairKernel::Lanes1); CHECK("crowded", p.wgs, 391);
        h.n_used_buckets = 47620;
        CHECK("not crowded", plan_pairs(world(100000), h, off).kernel, PairKernel::Brick256);
        h.n_pairs = 299999;  // brick-128 needs n_pairs < 3 n
        CHECK("small stage", plan_pairs(world(100000), h, off).kernel, PairKernel::Brick128);
        h.n_used_buckets = 0;  // unknown: not crowded
        CHECK("buckets unknown", plan_pairs(world(100000), h, off).kernel, PairKernel::Brick128);
    }
    {   // crowded: four lanes per body up to 65536 bodies
        StepHint h = hint(100000);
        h.n_used_buckets = 31207;
        const PairPlan p = plan_pairs(world(65536), h, off);
        CHECK("4 lanes", p.kernel, PairKernel::Lanes4); CHECK("4 lanes", p.wgs, 1024);
        const PairPlan q = plan_pairs(world(65537), h, off);
        CHECK("1 lane", q.kernel, PairKernel::Lanes1); CHECK("1 lane", q.wgs, 257);
    }
    {   // cap = region + 25 %, rounded up to 64, clamped to [256, 5000]
        StepHint h = hint(100000);
        h.n_pairs = 300000;
        const struct { uint32_t region, cap; } t[] = {{0, 1024}, {100, 256}, {205, 256}, {206, 320}, {1000, 1280}, {3999, 5000}, {4000, 5000}, {3949, 4992}};
        for (const auto& c : t) {
            h.max_region = c.region;
            const PairPlan p = plan_pairs(world(100000), h, off);
            CHECK("cap", p.cap, c.cap); CHECK("cap", p.lds, (size_t)c.cap * 28);
        }
        h.max_region = 4000;  // 140000 + 9696 bytes: one workgroup per CU
        CHECK("wgs", plan_pairs(world(100000), h, off).wgs, 256);
        h.max_region = 100; h.n_pairs = 0;  // small stage, 7168 + 5600 bytes: twelve would fit, seven is the most
        CHECK("wgs", plan_pairs(world(100000), h, off).wgs, 1792);
        PlanInputs in = world(100000);
        in.grid_table_size = 65536;  // 1024 bricks: never more workgroups than bricks, halved until so
        CHECK("wgs", plan_pairs(in, h, off).wgs, 896);
    }
    {   // the switches
        StepHint crowded = hint(100000);
        crowded.n_used_buckets = 1000;
        DebugSwitches d;
        d.pair_lanes = 4;
        PairPlan p = plan_pairs(world(100000), none, d);
        CHECK("PAIR_LANES=4", p.kernel, PairKernel::Lanes4); CHECK("PAIR_LANES=4", p.wgs, 1563);
        d.pair_lanes = 1;
        p = plan_pairs(world(40000), none, d);
        CHECK("PAIR_LANES=1", p.kernel, PairKernel::Lanes1); CHECK("PAIR_LANES=1", p.wgs, 157);
        CHECK("PAIR_LANES, slot grid", plan_pairs(world(32768), none, d).kernel, PairKernel::Slots);
        d = DebugSwitches();
        d.pair_kernel_brick = false;
        p = plan_pairs(world(40000), none, d);
        CHECK("PAIR_KERNEL=body", p.kernel, PairKernel::Lanes4); CHECK("PAIR_KERNEL=body", p.wgs, 625);
        d.pair_kernel_brick = true;
        CHECK("PAIR_KERNEL=brick", plan_pairs(world(100000), crowded, d).kernel, PairKernel::Brick128);
        d = DebugSwitches();
        d.brick_stage = 128;
        CHECK("BRICK_STAGE=128", plan_pairs(world(100000), none, d).kernel, PairKernel::Brick128);
        d.brick_stage = 256;
        CHECK("BRICK_STAGE=256", plan_pairs(world(100000), hint(1000), d).kernel, PairKernel::Brick256);
    }
}

// The (body count, switches) of tests/test_gpu_pairs_independent.py: which kernel each gives without a hint, with the hint of a
// sparsely filled grid and few pairs (left alone: the brick kernel, small stage) and with that of a crowded grid and many pairs
// (left alone: lanes per body) - worked out from plan_pairs as written: PAIR_LANES wins over everything above the slot grid,
// PAIR_KERNEL=brick over the crowding, BRICK_STAGE over the pair count.
static void pair_variants() {
    const StepHint none;
    StepHint sparse = hint(30000);   // 30000 pairs < 3 x 33000; 33000 x 10 <= 30000 x 21
    sparse.n_used_buckets = 30000;
    StepHint crowded = hint(30000);  // 33000 x 10 > 2000 x 21
    crowded.n_pairs = 1000000;
    crowded.n_used_buckets = 2000;
    DebugSwitches off, lanes4, lanes1, brick128, brick256;
    lanes4.pair_lanes = 4;
    lanes1.pair_lanes = 1;
    brick128.pair_kernel_brick = true; brick128.brick_stage = 128;
    brick256.pair_kernel_brick = true; brick256.brick_stage = 256;
    const struct { const char* what; uint64_t n; const DebugSwitches* d; PairKernel no_hint, sparse, crowded; } t[] = {
        {"33000, PAIR_LANES=4", 33000, &lanes4, PairKernel::Lanes4, PairKernel::Lanes4, PairKernel::Lanes4},
        {"33000, PAIR_LANES=1", 33000, &lanes1, PairKernel::Lanes1, PairKernel::Lanes1, PairKernel::Lanes1},
        {"33000, PAIR_KERNEL=brick BRICK_STAGE=128", 33000, &brick128, PairKernel::Brick128, PairKernel::Brick128, PairKernel::Brick128},
        {"33000, PAIR_KERNEL=brick BRICK_STAGE=256", 33000, &brick256, PairKernel::Brick256, PairKernel::Brick256, PairKernel::Brick256},
        {"33000, no switch", 33000, &off, PairKernel::Brick256, PairKernel::Brick128, PairKernel::Lanes4},
        {"32769, no switch", 32769, &off, PairKernel::Brick256, PairKernel::Brick128, PairKernel::Lanes4},
        {"32768, no switch", 32768, &off, PairKernel::Slots, PairKernel::Slots, PairKernel::Slots},
    };
    for (const auto& c : t) {
        PlanInputs in = world(c.n);
        in.grid_table_size = 1u << 17;  // what grid_plan gives these body counts
        CHECK(c.what, plan_pairs(in, none, *c.d).kernel, c.no_hint);
        CHECK(c.what, plan_pairs(in, sparse, *c.d).kernel, c.sparse);
        CHECK(c.what, plan_pairs(in, crowded, *c.d).kernel, c.crowded);
    }
    // a sparse grid with many pairs keeps the large stage
    sparse.n_pairs = 99000;
    CHECK("33000, 3 pairs per body", plan_pairs(world(33000), sparse, off).kernel, PairKernel::Brick256);
    sparse.n_pairs = 98999;
    CHECK("33000, fewer", plan_pairs(world(33000), sparse, off).kernel, PairKernel::Brick128);
}

static void narrow() {
    const DebugSwitches off;
    const StepHint none;
    NarrowPlan p = plan_narrowphase(world(200000), none, off);
    CHECK("no hint", p.threads, 128); CHECK("no hint", p.early_probe, 1);
    CHECK("no hint", p.blocks, 4096);  // 1.8M items / 128, capped at 256 * 16
    CHECK("no hint", plan_narrowphase(world(200001), none, off).threads, 512);
    CHECK("hint", plan_narrowphase(world(500000), hint(32768), off).threads, 128);
    CHECK("hint", plan_narrowphase(world(1000), hint(32769), off).threads, 512);
    StepHint h = hint(50);
    h.n_pairs = 100;
    CHECK("early probe", plan_narrowphase(world(1000), h, off).early_probe, 1);
    h.n_pairs = 101;
    CHECK("early probe", plan_narrowphase(world(1000), h, off).early_probe, 0);
    PlanInputs in = world(1000);
    in.np_items = 1000;
    CHECK("blocks", plan_narrowphase(in, hint(10), off).blocks, 8);
    CHECK("blocks", plan_narrowphase(in, hint(40000), off).blocks, 2);
    in.np_items = 1025;
    CHECK("blocks", plan_narrowphase(in, hint(40000), off).blocks, 3);
    in.statics = true; in.filters = true;
    p = plan_narrowphase(in, hint(10), off);
    CHECK("instance", p.statics, true); CHECK("instance", p.capsules, false); CHECK("instance", p.filters, true);
    in.statics = false; in.filters = false; in.capsules = true;
    p = plan_narrowphase(in, hint(10), off);
    CHECK("instance", p.statics, false); CHECK("instance", p.capsules, true); CHECK("instance", p.filters, false);
    DebugSwitches d;
    d.np_threads = 512;
    CHECK("NP_THREADS=512", plan_narrowphase(world(1000), hint(10), d).threads, 512);
    d.np_threads = 128;
    CHECK("NP_THREADS=128", plan_narrowphase(world(1000), hint(100000), d).threads, 128);
    d.np_threads = 256;  // not built: the 512-thread kernel, as the launch always did
    CHECK("NP_THREADS=256", plan_narrowphase(world(1000), hint(10), d).threads, 512);
    d = DebugSwitches();
    d.np_early_probe = false;
    CHECK("NP_EARLY_PROBE=0", plan_narrowphase(world(1000), none, d).early_probe, 0);
    d.np_early_probe = true;
    CHECK("NP_EARLY_PROBE=1", plan_narrowphase(world(1000), h, d).early_probe, 1);
}

static void coloring() {
    const DebugSwitches off;
    const StepHint none;
    ColorPlan p = plan_coloring(world(100000), hint(40960), off);
    CHECK("small", p.path, ColorPath::Small); CHECK("small", p.rounds, 0);
    p = plan_coloring(world(100000), hint(40961), off);
    CHECK("known", p.path, ColorPath::Known); CHECK("known", p.rounds, 5);
    p = plan_coloring(world(100000), none, off);
    CHECK("probe", p.path, ColorPath::Probe); CHECK("probe", p.rounds, 0);
    CHECK("probe", p.round_blocks, 512); CHECK("probe", p.sort_blocks, 512); CHECK("probe", p.cluster_sort_blocks, 2048); CHECK("probe", p.cluster_key_blocks, 2048);
    {   // a full colouring is known only by the rounds of an earlier full colouring
        PlanInputs in = world(100000);
        in.ctab_valid = false;
        in.color_epoch = 0;
        StepHint h = hint(50000);
        p = plan_coloring(in, h, off);
        CHECK("full", p.path, ColorPath::Probe); CHECK("full", p.full, true); CHECK("full", p.rebuild, true); CHECK("full", p.stamp, 1);
        h.full_rounds = 12;
        p = plan_coloring(in, h, off);
        CHECK("full", p.path, ColorPath::Known); CHECK("full", p.rounds, 12);
        h.n_manifolds = 40960;  // small wins over both
        CHECK("full", plan_coloring(in, h, off).path, ColorPath::Small);
        in.color_epoch = 7;  // (a table dropped later: full again, rebuilt whatever the epoch)
        p = plan_coloring(in, h, off);
        CHECK("full", p.rebuild, true); CHECK("full", p.stamp, 8);
    }
    {   // the table is rebuilt when color_epoch % PHYS_COLOR_CACHE_PERIOD == 0
        PlanInputs in = world(100000);
        const struct { uint64_t epoch; bool rebuild; } t[] = {{63, false}, {64, true}, {65, false}, {128, true}, {1, false}};
        for (const auto& c : t) {
            in.color_epoch = c.epoch;
            p = plan_coloring(in, hint(50000), off);
            CHECK("rebuild", p.rebuild, c.rebuild); CHECK("rebuild", p.full, false); CHECK("rebuild", p.stamp, c.epoch + 1);
        }
    }
    // sizes: rounds (m * 5/4 + 1024) / 1024 workgroups, at most 512 or what the capacity needs; the sort the next power of
    // two of m * 5/4 / 4096 + 1, at most 512; the cluster sort four times the rounds', its keys m * 5/4 / 1024 + 1
    p = plan_coloring(world(100000), hint(50000), off);
    CHECK("sizes", p.round_blocks, 62); CHECK("sizes", p.sort_blocks, 16); CHECK("sizes", p.cluster_sort_blocks, 248); CHECK("sizes", p.cluster_key_blocks, 62);
    p = plan_coloring(world(100000), hint(52429), off);
    CHECK("sizes", p.round_blocks, 65); CHECK("sizes", p.sort_blocks, 32); CHECK("sizes", p.cluster_key_blocks, 65);
    p = plan_coloring(world(100000), hint(0), off);
    CHECK("sizes", p.round_blocks, 1); CHECK("sizes", p.sort_blocks, 1); CHECK("sizes", p.cluster_key_blocks, 1);
    p = plan_coloring(world(1000000), hint(3000000), off);
    CHECK("sizes", p.round_blocks, 512); CHECK("sizes", p.sort_blocks, 512); CHECK("sizes", p.cluster_key_blocks, 2048);
    {
        PlanInputs in = world(100);
        in.max_manifolds = 4096;
        CHECK("sizes", plan_coloring(in, none, off).round_blocks, 4);
    }
    {   // the cluster step: a hint, not small, colours, 2 m >= 3 n_owned, m >= 170000, no PHYS_FLAG_SOLVER_PER_COLOR, clusters
        PlanInputs in = world(100000);
        in.cluster_count = 100;
        CHECK("cluster", plan_coloring(in, hint(170000), off).wants_cluster, true);
        CHECK("cluster", plan_coloring(in, hint(169999), off).wants_cluster, false);
        CHECK("cluster", plan_coloring(in, none, off).wants_cluster, false);
        in.n_owned = 113333;
        CHECK("dense", plan_coloring(in, hint(170000), off).wants_cluster, true);
        in.n_owned = 113334;
        CHECK("dense", plan_coloring(in, hint(170000), off).wants_cluster, false);
        in.n_owned = 100000;
        StepHint h = hint(170000);
        h.n_colors = 0;
        CHECK("colours", plan_coloring(in, h, off).wants_cluster, false);
        in.flags |= PHYS_FLAG_SOLVER_PER_COLOR;
        CHECK("per colour", plan_coloring(in, hint(170000), off).wants_cluster, false);
        in.flags &= ~PHYS_FLAG_SOLVER_PER_COLOR;
        in.solver_iterations = 0;
        CHECK("iterations", plan_coloring(in, hint(170000), off).wants_cluster, false);
        in.solver_iterations = 1000;
        CHECK("iterations", plan_coloring(in, hint(170000), off).wants_cluster, false);
        in.solver_iterations = 999;
        CHECK("iterations", plan_coloring(in, hint(170000), off).wants_cluster, true);
        in.cluster_count = 0;
        CHECK("no clusters", plan_coloring(in, hint(170000), off).wants_cluster, false);
        in.cluster_dynamic = true;  // dynamic clusters hold only bodies with manifolds: the row count alone decides
        in.n_owned = in.n = 1000000;
        CHECK("dynamic", plan_coloring(in, hint(170000), off).wants_cluster, true);
        CHECK("dynamic", plan_coloring(in, hint(169999), off).wants_cluster, false);
    }
    {   // PHYS_FLAG_SOLVER_CLUSTER forces it: any count, any density - but never a small update
        PlanInputs in = world(100000);
        in.cluster_count = 100;
        in.flags |= PHYS_FLAG_SOLVER_CLUSTER;
        CHECK("forced", plan_coloring(in, hint(40961), off).wants_cluster, true);
        CHECK("forced", plan_coloring(in, hint(40960), off).wants_cluster, false);
    }
    {   // it yields to flow_quad_beats_cluster only when exclusive and m <= 400000
        PlanInputs in = world(200000);
        in.cluster_count = 100;
        StepHint h = hint(400000);
        h.n_contacts = 700000; h.n_colors = 20;  // dataflow 0.0646 ms per sweep against 0.0902: it beats the cluster kernel
        CHECK("model", flow_quad_beats_cluster(400000, 700000, 20), true);
        CHECK("model", flow_quad_beats_cluster(400000, 700000, 8), false);  // 0.0538 against 0.0361
        CHECK("model", flow_quad_beats_cluster(400000, 0, 20), false);
        CHECK("model", flow_quad_beats_cluster(400000, 700000, 0), false);
        CHECK("shared GPU", plan_coloring(in, h, off).wants_cluster, true);
        in.exclusive = true;
        CHECK("exclusive", plan_coloring(in, h, off).wants_cluster, false);
        h.n_manifolds = 400001;
        CHECK("exclusive, beyond the dataflow kernels", plan_coloring(in, h, off).wants_cluster, true);
        h.n_manifolds = 400000;
        h.n_colors = 8;
        CHECK("exclusive, the cluster kernel wins", plan_coloring(in, h, off).wants_cluster, true);
        h.n_colors = 20;
        DebugSwitches d;
        d.no_flow_preference = true;
        CHECK("NO_FLOW_PREFERENCE", plan_coloring(in, h, d).wants_cluster, true);
        d = DebugSwitches();
        d.cluster_min = 1000;  // moves the threshold, counts as dense, and never yields
        CHECK("CLUSTER_MIN", plan_coloring(in, h, d).wants_cluster, true);
        in.n_owned = 10000000;
        CHECK("CLUSTER_MIN", plan_coloring(in, hint(50000), d).wants_cluster, true);
        d.cluster_min = 50001;
        CHECK("CLUSTER_MIN", plan_coloring(in, hint(50000), d).wants_cluster, false);
        in.n_owned = 200000;
        in.flags |= PHYS_FLAG_SOLVER_CLUSTER;
        CHECK("forced", plan_coloring(in, h, off).wants_cluster, true);
    }
}

static void solver() {
    const DebugSwitches off;
    const StepHint none;
    const PlanInputs in = world(100000);  // capacity 1.7M manifolds
    SolverPlan p = plan_solver(in, hint(400000), off, false);
    CHECK("flow", p.path, SolverPath::FlowLane); CHECK("flow", p.flow(), true);
    p = plan_solver(in, hint(400001), off, false);
    CHECK("per colour", p.path, SolverPath::PerColor); CHECK("per colour", p.flow(), false);
    CHECK("quad", plan_solver(in, hint(200000), off, false).path, SolverPath::FlowQuad);
    CHECK("quad", plan_solver(in, hint(200001), off, false).path, SolverPath::FlowLane);
    {
        PlanInputs ex = in;
        ex.exclusive = true;
        CHECK("quad, exclusive", plan_solver(ex, hint(400000), off, false).path, SolverPath::FlowQuad);
        CHECK("quad, exclusive", plan_solver(ex, hint(400001), off, false).path, SolverPath::PerColor);
        CHECK("guarded", plan_solver(ex, hint(200000), off, true).guarded, false);
        // statically dealt items: 224 workgroups; three per CU on seven eighths of the chip where exclusive and beyond 32768
        CHECK("items", plan_solver(ex, hint(32768), off, false).items, 224);
        CHECK("items", plan_solver(ex, hint(32769), off, false).items, 672);
        ex.cus = 64;
        CHECK("items", plan_solver(ex, hint(100000), off, false).items, 168);
    }
    {   // iterations in (0, 1000); the granules must exist; a hint
        PlanInputs q = in;
        q.solver_iterations = 0;
        CHECK("iterations", plan_solver(q, hint(1000), off, false).path, SolverPath::PerColor);
        q.solver_iterations = 1000;
        CHECK("iterations", plan_solver(q, hint(1000), off, false).path, SolverPath::PerColor);
        q.solver_iterations = 999;
        CHECK("iterations", plan_solver(q, hint(1000), off, false).path, SolverPath::FlowQuad);
        q = in;
        q.flow_vel = false;
        CHECK("no granules", plan_solver(q, hint(1000), off, false).path, SolverPath::PerColor);
        p = plan_solver(in, none, off, false);
        CHECK("no hint", p.path, SolverPath::PerColor); CHECK("no hint", p.big, 0); CHECK("no hint", p.rows_blocks, 4096);
    }
    // items = sweeps * ceil(m * 5/4 / rows per item) + 1, at most 224 (quad) / 256; rows: m * 5/4 / 256 (up) + 1, at most 4096
    p = plan_solver(in, hint(10000), off, false);
    CHECK("sizes", p.items, 224); CHECK("sizes", p.rows_blocks, 50); CHECK("sizes", p.guarded, true); CHECK("sizes", p.stall, false);
    CHECK("sizes", p.timeout_ticks, 300000000ll);
    CHECK("sizes", plan_solver(in, hint(300000), off, false).items, 256);
    {
        PlanInputs q = in;
        q.solver_iterations = 1; q.warm = false;
        CHECK("sizes", plan_solver(q, hint(10), off, false).items, 2);
        q.warm = true;  // the warm sweep counts
        CHECK("sizes", plan_solver(q, hint(10), off, false).items, 3);
        q.max_manifolds = 4096;  // the capacity bounds the rows: 16 workgroups
        CHECK("sizes", plan_solver(q, hint(100000), off, false).rows_blocks, 16);
    }
    CHECK("sizes", plan_solver(in, hint(1000000), off, false).rows_blocks, 4096);
    {   // look one item ahead while 4 * rows per colour >= 256 * items
        StepHint h = hint(300000);
        h.n_colors = 4;
        CHECK("pipeline", plan_solver(in, h, off, false).pipeline, 1);
        h.n_colors = 20;
        CHECK("pipeline", plan_solver(in, h, off, false).pipeline, 0);
        h.n_colors = 18;  // 16666 rows per colour: 66664 >= 65536
        CHECK("pipeline", plan_solver(in, h, off, false).pipeline, 1);
        h.n_colors = 19;  // 15789: 63156
        CHECK("pipeline", plan_solver(in, h, off, false).pipeline, 0);
    }
    {   // the cluster step
        p = plan_solver(in, hint(200000), off, true);
        CHECK("cluster", p.path, SolverPath::Cluster); CHECK("cluster", p.flow(), true); CHECK("cluster", p.guarded, true);
        PlanInputs q = in;
        q.materials = true;
        CHECK("materials", plan_solver(q, hint(200000), off, true).materials, true);
    }
    {   // the tail: trailing colours of <= 512 rows; a tail of one colour is no tail. Per colour: four lanes up to 32768 rows
        StepHint h = hint(500000);
        h.n_colors = 6;
        const uint32_t counts[6] = {200000, 150000, 32769, 32768, 512, 300};
        for (int k = 0; k < 6; ++k) h.color_count[k] = counts[k];
        p = plan_solver(in, h, off, false);
        CHECK("tail", p.path, SolverPath::PerColor); CHECK("tail", p.big, 4);
        CHECK("colour 0", p.color_quad[0], false); CHECK("colour 0", p.color_blocks[0], 978);
        CHECK("colour 1", p.color_quad[1], false); CHECK("colour 1", p.color_blocks[1], 734);
        CHECK("colour 2", p.color_quad[2], false); CHECK("colour 2", p.color_blocks[2], 162);
        CHECK("colour 3", p.color_quad[3], true); CHECK("colour 3", p.color_blocks[3], 641);
        CHECK("colour 4", p.color_blocks[4], 0);
        h.color_count[4] = 513;
        CHECK("tail of one", plan_solver(in, h, off, false).big, 6);
        h.color_count[5] = 513;
        CHECK("no tail", plan_solver(in, h, off, false).big, 6);
        h.color_count[4] = 512; h.color_count[5] = 0; h.color_count[3] = 1;
        CHECK("tail of three", plan_solver(in, h, off, false).big, 3);
        for (int k = 0; k < 6; ++k) h.color_count[k] = 10;
        CHECK("all tail", plan_solver(in, h, off, false).big, 0);
        for (int k = 0; k < 6; ++k) h.color_count[k] = counts[k];
        DebugSwitches d;
        d.color_kernel_lane = true;
        p = plan_solver(in, h, d, false);
        CHECK("COLOR_KERNEL=lane", p.color_quad[3], false); CHECK("COLOR_KERNEL=lane", p.color_blocks[3], 161);
        d.color_kernel_lane = false;
        p = plan_solver(in, h, d, false);
        CHECK("COLOR_KERNEL=quad", p.color_quad[0], true); CHECK("COLOR_KERNEL=quad", p.color_blocks[0], 3908); CHECK("COLOR_KERNEL=quad", p.big, 4);
    }
    {   // the switches
        DebugSwitches d;
        d.flow_max = 1000;
        CHECK("FLOW_MAX", plan_solver(in, hint(1000), d, false).path, SolverPath::FlowQuad);
        CHECK("FLOW_MAX", plan_solver(in, hint(1001), d, false).path, SolverPath::PerColor);
        d.flow_max = 1000000;
        CHECK("FLOW_MAX", plan_solver(in, hint(1000000), d, false).path, SolverPath::FlowLane);
        d = DebugSwitches();
        d.flow_quad_max = 1000;
        CHECK("FLOW_QUAD_MAX", plan_solver(in, hint(1000), d, false).path, SolverPath::FlowQuad);
        CHECK("FLOW_QUAD_MAX", plan_solver(in, hint(1001), d, false).path, SolverPath::FlowLane);
        d = DebugSwitches();
        d.flow_stall = true;
        p = plan_solver(in, hint(1000), d, false);
        CHECK("FLOW_STALL", p.stall, true); CHECK("FLOW_STALL", p.timeout_ticks, 2000000ll);
        d = DebugSwitches();
        d.flow_pipeline = true;
        StepHint h = hint(300000);
        h.n_colors = 20;
        CHECK("FLOW_PIPELINE=1", plan_solver(in, h, d, false).pipeline, 1);
        d.flow_pipeline = false;
        h.n_colors = 4;
        CHECK("FLOW_PIPELINE=0", plan_solver(in, h, d, false).pipeline, 0);
    }
    CHECK("events", plan_event_blocks(in, hint(1000)), 6);
    CHECK("events", plan_event_blocks(in, none), 2048);
    PlanInputs q = in;
    q.max_manifolds = 300;
    CHECK("events", plan_event_blocks(q, hint(1000)), 2);
    q.max_manifolds = 0;
    CHECK("events", plan_event_blocks(q, none), 1);
}

// Each switch overrides exactly the decision it names: over a spread of scenes, every plan with the switch set equals the plan
// without it, once the named fields are copied over.
struct Scene { PlanInputs in; StepHint h; bool cluster; };
template <class Set, class PatchP, class PatchN, class PatchC, class PatchS>
static void only(const char* name, Set set, PatchP pp, PatchN pn, PatchC pc, PatchS ps) {
    Scene scenes[6] = {{world(1000), StepHint(), false}, {world(10000), hint(10000), false}, {world(100000), hint(216000), false},
                       {world(100000), hint(216000), true}, {world(1000000), hint(380000), false}, {world(1000000), hint(2900000), false}};
    scenes[2].in.cluster_count = scenes[3].in.cluster_count = 600;
    scenes[4].in.exclusive = true; scenes[4].in.cluster_dynamic = true;
    scenes[5].h.n_used_buckets = 100000;
    for (int k = 0; k < 6; ++k) for (int c = 0; c < 30; ++c) scenes[k].h.color_count[c] = scenes[k].h.n_manifolds / (10u + 90u * (c > 5));
    for (int k = 0; k < 6; ++k) if (scenes[k].h.valid) scenes[k].h.n_colors = 30;
    const DebugSwitches off;
    DebugSwitches on;
    set(on);
    for (const Scene& s : scenes) {
        PairPlan p0 = plan_pairs(s.in, s.h, off), p1 = plan_pairs(s.in, s.h, on);
        NarrowPlan n0 = plan_narrowphase(s.in, s.h, off), n1 = plan_narrowphase(s.in, s.h, on);
        ColorPlan c0 = plan_coloring(s.in, s.h, off), c1 = plan_coloring(s.in, s.h, on);
        SolverPlan s0 = plan_solver(s.in, s.h, off, s.cluster), s1 = plan_solver(s.in, s.h, on, s.cluster);
        pp(p0, p1); pn(n0, n1); pc(c0, c1); ps(s0, s1);
        CHECK(name, same(p0, p1), true); CHECK(name, same(n0, n1), true); CHECK(name, same(c0, c1), true); CHECK(name, same(s0, s1), true);
    }
}
static void switches_stay_in_their_lane() {
    auto p_ = [](PairPlan&, const PairPlan&) {};
    auto n_ = [](NarrowPlan&, const NarrowPlan&) {};
    auto c_ = [](ColorPlan&, const ColorPlan&) {};
    auto s_ = [](SolverPlan&, const SolverPlan&) {};
    auto whole_pairs = [](PairPlan& a, const PairPlan& b) { a = b; };  // kernel, and the sizes that follow from the kernel
    only("PAIR_LANES", [](DebugSwitches& d) { d.pair_lanes = 1; }, whole_pairs, n_, c_, s_);
    only("PAIR_KERNEL", [](DebugSwitches& d) { d.pair_kernel_brick = false; }, whole_pairs, n_, c_, s_);
    only("BRICK_STAGE", [](DebugSwitches& d) { d.brick_stage = 128; }, [](PairPlan& a, const PairPlan& b) { a.kernel = b.kernel; a.wgs = b.wgs; }, n_, c_, s_);
    only("NP_THREADS", [](DebugSwitches& d) { d.np_threads = 128; }, p_, [](NarrowPlan& a, const NarrowPlan& b) { a.threads = b.threads; a.blocks = b.blocks; }, c_, s_);
    only("NP_EARLY_PROBE", [](DebugSwitches& d) { d.np_early_probe = false; }, p_, [](NarrowPlan& a, const NarrowPlan& b) { a.early_probe = b.early_probe; }, c_, s_);
    only("CLUSTER_MIN", [](DebugSwitches& d) { d.cluster_min = 1; }, p_, n_, [](ColorPlan& a, const ColorPlan& b) { a.wants_cluster = b.wants_cluster; }, s_);
    only("NO_FLOW_PREFERENCE", [](DebugSwitches& d) { d.no_flow_preference = true; }, p_, n_, [](ColorPlan& a, const ColorPlan& b) { a.wants_cluster = b.wants_cluster; }, s_);
    auto flow_path = [](SolverPlan& a, const SolverPlan& b) {  // the path, and what is sized per path
        a.path = b.path; a.items = b.items; a.pipeline = b.pipeline; a.big = b.big;
        std::memcpy(a.color_quad, b.color_quad, sizeof a.color_quad); std::memcpy(a.color_blocks, b.color_blocks, sizeof a.color_blocks);
    };
    only("FLOW_MAX", [](DebugSwitches& d) { d.flow_max = 250000; }, p_, n_, c_, flow_path);
    only("FLOW_QUAD_MAX", [](DebugSwitches& d) { d.flow_quad_max = 100000; }, p_, n_, c_, [](SolverPlan& a, const SolverPlan& b) { a.path = b.path; a.items = b.items; a.pipeline = b.pipeline; });
    only("FLOW_PIPELINE", [](DebugSwitches& d) { d.flow_pipeline = true; }, p_, n_, c_, [](SolverPlan& a, const SolverPlan& b) { a.pipeline = b.pipeline; });
    only("FLOW_STALL", [](DebugSwitches& d) { d.flow_stall = true; }, p_, n_, c_, [](SolverPlan& a, const SolverPlan& b) { a.stall = b.stall; a.timeout_ticks = b.timeout_ticks; });
    only("COLOR_KERNEL", [](DebugSwitches& d) { d.color_kernel_lane = false; }, p_, n_, c_, [](SolverPlan& a, const SolverPlan& b) {
        std::memcpy(a.color_quad, b.color_quad, sizeof a.color_quad); std::memcpy(a.color_blocks, b.color_blocks, sizeof a.color_blocks); });
    // the switches no per-update plan reads: set-up (cluster_assign, collision_alloc), the dynamic deal, the ray casts
    only("others", [](DebugSwitches& d) { d.no_cluster = d.cluster_dynamic = d.raycast_stats = true; d.clusters_per_cu = 1; d.cluster_cap = 64;
                                          d.ctab_slots = 64; d.flow_epoch = 65530; }, p_, n_, c_, s_);
}

int main() {
    pairs();
    pair_variants();
    narrow();
    coloring();
    solver();
    switches_stay_in_their_lane();
    std::printf("plan_probe: %d checks passed\n", g_checks);
    return 0;
}
