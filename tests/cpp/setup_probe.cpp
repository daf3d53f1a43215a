// setup_probe.cpp — the host-only set-up and read-out functions (physics_amd/csrc/setup.hpp, readout.hpp) against cases.
// Built by a host compiler alone (tests/test_setup_cpu.py); exits non-zero at the first mismatch. Where the expected values
// come from: worked out BY HAND from the functions' text as it stood inside the .hip files before the
// headers existed (grid_plan, collision_alloc, cluster_assign, cluster_plan_dynamic, phys_set_bodies, constraints_alloc, the
// validation loops, the read-outs, phys_sync) - or, for the static colliders' grid, from a BRUTE-FORCE restatement in this
// file (every static against every query box) - or, for the volume records (include/spec/volume.h), bit by bit from the float32
// arithmetic of body_aabb and quat_to_m33, the derivation written next to the case. Never from running the functions and
// pasting what they gave.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "../../physics_amd/csrc/readout.hpp"

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
#define CHECK_STR(what, got, want)                                                                                      \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const std::string g_ = (got), w_ = (want);                                                                      \
        if (g_ != w_) {                                                                                                 \
            std::printf("MISMATCH %s:%d  %s:\n  got      \"%s\"\n  expected \"%s\"\n", __FILE__, __LINE__, what, g_.c_str(), w_.c_str()); \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)
template <class T>
static void check_vec(const char* what, int line, const std::vector<T>& got, std::initializer_list<T> want) {
    ++g_checks;
    if (got != std::vector<T>(want)) {
        std::printf("MISMATCH %s:%d  %s: vector differs (size %zu, expected %zu)\n", __FILE__, line, what, got.size(), want.size());
        std::exit(1);
    }
}
#define CHECK_VEC(what, got, ...) check_vec<uint32_t>(what, __LINE__, got, {__VA_ARGS__})

static uint32_t g_seed = 1;
static void seed(uint32_t s) { g_seed = s; }
static float rnd() {  // [0, 1): a 32-bit LCG, the top 24 bits
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}
static float rnd(float lo, float hi) { return lo + (hi - lo) * rnd(); }

static void check_shape(const char* what, const GridShape& g, uint32_t bx, uint32_t by, uint32_t bz) {
    CHECK(what, g.mx, (1u << bx) - 1u); CHECK(what, g.my, (1u << by) - 1u); CHECK(what, g.mz, (1u << bz) - 1u);
    CHECK(what, g.sx, bx - 2u); CHECK(what, g.sy, by - 2u);
}

// ---- grid_plan: bits = 9 .. 27 with 2^bits >= 2 n_total; every axis starts at 2 bits, the other bits - 6 go one at a time to the
// axis with the largest cells / 2^bits (strictly: ties to the lower axis), cells = extent / cell + 1, cell = diameter * 1.05 + 0.04
static void grid() {
    const float margin = 0.02f;
    {   // no bodies: 512 buckets, every axis has one cell: x, y, z in turn
        const GridPlan p = grid_plan(0, 0, nullptr, nullptr, margin);
        CHECK("n = 0", p.table_size, 512); check_shape("n = 0", p.shape, 3, 3, 3);
    }
    {
        const float pos[3] = {5.0f, 5.0f, 5.0f};
        const GridPlan p = grid_plan(1, 1, pos, nullptr, margin);
        CHECK("one body", p.table_size, 512); check_shape("one body", p.shape, 3, 3, 3);
    }
    {   // 256 bodies on a line along x, 1 apart, no extents: cell 1.09, 234.9 cells along x, one along y and z
        std::vector<float> pos(3 * 257, 0.0f);
        for (int i = 0; i < 256; ++i) pos[3 * i] = (float)i;
        pos[3 * 256 + 1] = 1.0e6f;  // a ghost slot's stale position: never read
        GridPlan p = grid_plan(256, 256, pos.data(), nullptr, margin);
        CHECK("256 bodies", p.table_size, 512); check_shape("256 bodies", p.shape, 5, 2, 2);
        p = grid_plan(257, 257, pos.data(), nullptr, margin);  // 257 owned: the far one counts (y: 917432 cells, x: 234.9)
        CHECK("257 bodies", p.table_size, 1024); check_shape("257 bodies", p.shape, 2, 6, 2);
        p = grid_plan(257, 256, pos.data(), nullptr, margin);  // table from the total, bounds from the owned
        CHECK("256 + 1 ghost", p.table_size, 1024); check_shape("256 + 1 ghost", p.shape, 6, 2, 2);
    }
    {   // a 64 x 1 x 1 line of unit cubes: 58.8 cells along x, all three spare bits go there
        std::vector<float> pos(3 * 64, 0.0f), he(3 * 64, 0.5f);
        for (int i = 0; i < 64; ++i) pos[3 * i] = (float)i;
        const GridPlan p = grid_plan(64, 64, pos.data(), he.data(), margin);
        CHECK("line", p.table_size, 512); check_shape("line", p.shape, 5, 2, 2);
    }
    {   // a 16 x 16 x 16 block of unit cubes: 8192 buckets, 7 spare bits dealt x y z x y z x
        std::vector<float> pos, he(3 * 4096, 0.5f);
        for (int z = 0; z < 16; ++z) for (int y = 0; y < 16; ++y) for (int x = 0; x < 16; ++x) { pos.push_back((float)x); pos.push_back((float)y); pos.push_back((float)z); }
        const GridPlan p = grid_plan(4096, 4096, pos.data(), he.data(), margin);
        CHECK("block", p.table_size, 8192); check_shape("block", p.shape, 5, 4, 4);
    }
    {   // extents 3 x 1 x 0, 512 slots (4 spare bits). Without half extents the cell is 1.09: cells 3.75 / 1.92 / 1 -> x y x z;
        // with half extents 0.05 it is 0.145: cells 21.7 / 7.9 / 1 -> x x y x
        std::vector<float> pos(3 * 512, 0.0f), he(3 * 512, 0.05f);
        pos[3] = 3.0f; pos[4] = 1.0f;
        GridPlan p = grid_plan(512, 512, pos.data(), nullptr, margin);
        CHECK("no extents", p.table_size, 1024); check_shape("no extents", p.shape, 4, 3, 3);
        p = grid_plan(512, 512, pos.data(), he.data(), margin);
        check_shape("extents", p.shape, 5, 3, 2);
    }
    {   // 2^26 + 1 slots: 2^27 buckets, 21 spare bits; two owned bodies 1e9 apart along x: x stops at 20 bits, then y z y
        const float pos[6] = {0.0f, 0.0f, 0.0f, 1.0e9f, 0.0f, 0.0f};
        const GridPlan p = grid_plan((1ull << 26) + 1, 2, pos, nullptr, margin);
        CHECK("20 bits", p.table_size, 1u << 27); check_shape("20 bits", p.shape, 20, 4, 3);
        CHECK("most buckets", grid_plan(1ull << 40, 0, nullptr, nullptr, margin).table_size, 1u << 27);
    }
}

// ---- collision_sizes: collision_alloc's arithmetic -----------------------------------------------------------------------------
static phys_config config(uint32_t flags) {
    phys_config c;
    std::memset(&c, 0, sizeof c);
    c.flags = PHYS_FLAG_COLLISIONS | flags;
    return c;
}
static void sizes() {
    const DebugSwitches off;
    CollisionSizes s = collision_sizes(config(0), 1, off);  // both floors of 4096
    CHECK("n = 1", s.max_pairs, 4096); CHECK("n = 1", s.max_manifolds, 4096); CHECK("n = 1", s.ok, true);
    CHECK("n = 1", s.bucket_bytes, 2048); CHECK("n = 1", s.color_bytes, 256); CHECK("n = 1", s.counter_bytes, sizeof(StepCounters));
    CHECK("n = 1", s.ctab_slots, 8192); CHECK("n = 1", s.warm, true); CHECK("n = 1", s.flow_buffers, true);
    s = collision_sizes(config(0), 1000, off);  // 24 and 17 per body; 2048 buckets; 32 bytes of colouring state per body; 25500 -> 32768 slots
    CHECK("n = 1000", s.max_pairs, 24000); CHECK("n = 1000", s.max_manifolds, 17000);
    CHECK("n = 1000", s.bucket_bytes, 8192); CHECK("n = 1000", s.color_bytes, 32000); CHECK("n = 1000", s.ctab_slots, 32768);
    s = collision_sizes(config(0), 9, off);  // 288 bytes of colouring state: rounded up to 256s
    CHECK("n = 9", s.color_bytes, 512);
    {
        phys_config c = config(0);
        c.max_pairs = 0xFFFFFFF1ull;
        CHECK("u32 limit", collision_sizes(c, 1000, off).ok, false);
        c.max_pairs = 0xFFFFFFF0ull;
        CHECK("u32 limit", collision_sizes(c, 1000, off).ok, true);
        c.max_manifolds = 0xFFFFFFF1ull;
        CHECK("u32 limit", collision_sizes(c, 1000, off).ok, false);
    }
    {   // warm starting: the colour table's value word holds 26 bits of manifold index. 64 M below 2^32 - 1 on the same edge
        phys_config c = config(0);
        c.max_manifolds = (1ull << 26) - 1;
        s = collision_sizes(c, 1000, off);
        CHECK("warm", s.warm, true); CHECK("warm", s.flow_buffers, true); CHECK("warm", s.ctab_slots, 1ull << 27);
        c.max_manifolds = 1ull << 26;
        s = collision_sizes(c, 1000, off);
        CHECK("not warm", s.warm, false); CHECK("not warm", s.flow_buffers, false);
        c.max_manifolds = 4096; c.max_pairs = 4096;
        CHECK("32 n", collision_sizes(c, (1ull << 27) - 1, off).flow_buffers, true);
        CHECK("32 n", collision_sizes(c, 1ull << 27, off).flow_buffers, false);
        CHECK("32 n", collision_sizes(c, 1ull << 27, off).warm, true);
    }
    s = collision_sizes(config(PHYS_FLAG_NO_WARM_START), 1000, off);
    CHECK("NO_WARM_START", s.warm, false); CHECK("NO_WARM_START", s.flow_buffers, true);
    s = collision_sizes(config(PHYS_FLAG_SOLVER_PER_COLOR), 1000, off);
    CHECK("SOLVER_PER_COLOR", s.flow_buffers, false); CHECK("SOLVER_PER_COLOR", s.warm, true);
    {
        DebugSwitches d;
        d.ctab_slots = 64;
        CHECK("CTAB_SLOTS=64", collision_sizes(config(0), 1000, d).ctab_slots, 64);
        d.ctab_slots = 63;
        CHECK("CTAB_SLOTS=63", collision_sizes(config(0), 1000, d).ctab_slots, 32768);
        d.ctab_slots = 96;
        CHECK("CTAB_SLOTS=96", collision_sizes(config(0), 1000, d).ctab_slots, 32768);
        d.ctab_slots = 32;
        CHECK("CTAB_SLOTS=32", collision_sizes(config(0), 1000, d).ctab_slots, 32768);
    }
    s = collision_sizes(config(PHYS_FLAG_BROADPHASE_ONLY), 1000, off);  // no colouring block, nothing of the contact stages
    CHECK("BROADPHASE_ONLY", s.color_bytes, 0); CHECK("BROADPHASE_ONLY", s.bucket_bytes, 8192); CHECK("BROADPHASE_ONLY", s.max_pairs, 24000);
    CHECK("BROADPHASE_ONLY", s.ctab_slots, 0); CHECK("BROADPHASE_ONLY", s.warm, false); CHECK("BROADPHASE_ONLY", s.flow_buffers, false);
}

// ---- cluster_fit: 256 CUs -> 224 in use; 672 / 448 / 224 workgroups at 3 / 2 / 1 per CU. LDS of a workgroup: 64 slots + 272
// bytes, in KiB; 160 KiB per CU: at most 53 KiB each of three (832 slots), 80 KiB each of two (1216 slots), one of 2496 slots
static void check_fit(const char* what, const ClusterFit& f, int per_cu, uint32_t clusters, uint32_t slots, bool ok) {
    CHECK(what, f.per_cu, per_cu); CHECK(what, f.clusters, clusters); CHECK(what, f.slots, slots); CHECK(what, f.ok, ok);
}
static void fit() {
    const DebugSwitches off;
    CHECK("constants", kClusterSlotBytes, 64); CHECK("constants", cluster_lds_bytes(832), 53520); CHECK("constants", kClusterMaxSlots, 2496);
    CHECK("on chip", clusters_on_chip(3, 256), 672); CHECK("on chip", clusters_on_chip(1, 8), 8); CHECK("on chip", clusters_on_chip(3, 8), 21);
    CHECK("per CU", cluster_per_cu_first(cluster_per_cu_max(true), off), 3); CHECK("per CU", cluster_per_cu_first(cluster_per_cu_max(false), off), 2);
    check_fit("32768", cluster_fit(32768, 3, 256, 0), 3, 672, 64, true);  // 49 bodies each, rounded up: 512 clusters in use
    check_fit("three per CU", cluster_fit(559104, 3, 256, 0), 3, 672, 832, true);
    // one more: 896 slots are 57 KiB (three: 171), two of 1280 are 81 KiB each, one of 2560 is beyond kClusterMaxSlots
    check_fit("one too many", cluster_fit(559105, 3, 256, 0), 1, 224, 2560, false);
    check_fit("two per CU", cluster_fit(544768, 2, 256, 0), 2, 448, 1216, true);
    check_fit("two per CU + 1", cluster_fit(544769, 2, 256, 0), 1, 224, 2496, true);  // 2433 bodies each: one workgroup of 157 KiB
    check_fit("full tensors", cluster_fit(559104, 2, 256, 0), 1, 224, 2496, true);
    check_fit("full tensors + 1", cluster_fit(559105, 2, 256, 0), 1, 224, 2560, false);
    {
        DebugSwitches d;
        d.clusters_per_cu = 1;
        CHECK("CLUSTERS_PER_CU=1", cluster_per_cu_first(3, d), 1);
        d.clusters_per_cu = 7;
        CHECK("CLUSTERS_PER_CU=7", cluster_per_cu_first(3, d), 3); CHECK("CLUSTERS_PER_CU=7", cluster_per_cu_first(2, d), 2);
        d.clusters_per_cu = 0;
        CHECK("CLUSTERS_PER_CU=0", cluster_per_cu_first(3, d), 1);
        check_fit("CLUSTERS_PER_CU=1", cluster_fit(32768, 1, 256, 0), 1, 224, 192, true);  // 147 bodies each
    }
    // 8 CUs: 7 in use, but never fewer than 8 workgroups. 32768 bodies: 21 x 1600, 14 x 2368, 8 x 4096 - none fits
    check_fit("8 CUs", cluster_fit(32768, 3, 8, 0), 1, 8, 4096, false);
    check_fit("8 CUs", cluster_fit(8 * 2496, 1, 8, 0), 1, 8, 2496, true);
    // the floor of the dynamic deal: 64 slots at least; the static one has none
    check_fit("floor", cluster_fit(0, 3, 256, 64), 3, 672, 64, true);
    check_fit("no floor", cluster_fit(0, 3, 256, 0), 3, 672, 0, true);
}

// ---- plan_dynamic_clusters: cluster_plan_dynamic below its early returns ------------------------------------------------------
static StepHint active(uint32_t n_active, uint32_t manifolds = 0) {
    StepHint h;
    h.valid = true;
    h.n_active = n_active;
    h.n_manifolds = manifolds;
    return h;
}
static void check_dyn(const char* what, const std::optional<ClusterShape>& s, long long clusters, long long slots) {
    CHECK(what, s.has_value(), clusters >= 0);
    if (s) { CHECK(what, s->clusters, clusters); CHECK(what, s->slots, slots); }
}
static void dynamic() {
    const DebugSwitches off;
    const uint64_t n = 1000000;
    check_dyn("nothing known", plan_dynamic_clusters(n, true, 256, active(0, 0), off), -1, 0);
    check_dyn("manifolds known", plan_dynamic_clusters(500, true, 256, active(0, 1000), off), 672, 64);  // min(500, 1000) + 25 %: one body each
    check_dyn("manifolds known", plan_dynamic_clusters(n, true, 256, active(0, 100000), off), 672, 192);  // 125000 / 672 = 187
    // want = active * 5 / 4: 559103 fits three per CU (832 slots), 559105 does not: no cluster step
    check_dyn("inside", plan_dynamic_clusters(n, true, 256, active(447283), off), 672, 832);
    check_dyn("outside", plan_dynamic_clusters(n, true, 256, active(447284), off), -1, 0);
    check_dyn("full tensors", plan_dynamic_clusters(n, false, 256, active(435815), off), 448, 1216);  // want 544768: two per CU, just
    check_dyn("full tensors", plan_dynamic_clusters(n, false, 256, active(435816), off), -1, 0);       // 544770: only one per CU would fit
    {
        DebugSwitches d;
        d.cluster_cap = 64;
        check_dyn("CLUSTER_CAP=64", plan_dynamic_clusters(n, true, 256, active(100000), d), 672, 64);
        d.cluster_cap = 1000000;  // obeyed although it does not fit: one workgroup per CU, as many homes as its LDS holds
        check_dyn("CLUSTER_CAP=1000000", plan_dynamic_clusters(n, true, 256, active(1000000), d), 224, 2496);
        d.cluster_cap = 500000;  // 745 bodies each: 768 slots, three per CU
        check_dyn("CLUSTER_CAP=500000", plan_dynamic_clusters(n, true, 256, active(1000000), d), 672, 768);
        d.cluster_cap = 550000;  // full tensors: only one per CU fits (2456 bodies each) - refused without a cap, allowed with one
        check_dyn("CLUSTER_CAP=550000, full tensors", plan_dynamic_clusters(n, false, 256, active(1000000), d), 224, 2496);
        d = DebugSwitches();
        d.clusters_per_cu = 1;
        check_dyn("CLUSTERS_PER_CU=1", plan_dynamic_clusters(n, true, 256, active(100000), d), 224, 576);  // 125000 / 224 = 559
        check_dyn("CLUSTERS_PER_CU=1, too many", plan_dynamic_clusters(n, true, 256, active(1000000), d), -1, 0);
        d.cluster_cap = 2000000;  // with a cap as well: the fallback
        check_dyn("CLUSTERS_PER_CU=1 and a cap", plan_dynamic_clusters(n, true, 256, active(1000000), d), 224, 2496);
    }
    {   // the 33 280-body tower of tests/test_gpu_cluster_variants.py, everybody in contact, on 256 CUs: homes = clusters x slots.
        // The floor of 64 slots makes 672 x 64 = 43 008 homes of PHYS_DEBUG_CLUSTER_CAP=9000 with diagonal tensors -
        // nobody is homeless; with full tensors (two per CU) 28 672, and with one workgroup per CU 14 336, either kind
        DebugSwitches d;
        d.cluster_cap = 9000;
        check_dyn("tower, cap 9000", plan_dynamic_clusters(33280, true, 256, active(33280), d), 672, 64);
        check_dyn("tower, cap 9000, full tensors", plan_dynamic_clusters(33280, false, 256, active(33280), d), 448, 64);
        d.clusters_per_cu = 1;
        check_dyn("tower, cap 9000, one per CU", plan_dynamic_clusters(33280, true, 256, active(33280), d), 224, 64);
        check_dyn("tower, cap 9000, one per CU, full tensors", plan_dynamic_clusters(33280, false, 256, active(33280), d), 224, 64);
    }
    {   // the six scenes of plan_probe.cpp (no count of active bodies yet: min(n_owned, manifolds) + 25 %), on 256 CUs
        const struct { uint64_t n; uint32_t manifolds; long long c0, s0, c1, s1, c2, s2; } t[6] = {
            //                       no switch      CLUSTER_CAP=200000   CLUSTERS_PER_CU=1
            {1000, 0,                -1, 0,         -1, 0,               -1, 0},
            {10000, 10000,           672, 64,       672, 64,             224, 64},      // 12500
            {100000, 216000,         672, 192,      672, 192,            224, 576},     // 125000
            {100000, 216000,         672, 192,      672, 192,            224, 576},
            {1000000, 380000,        672, 768,      672, 320,            224, 2176},    // 475000 (capped: 200000 / 672 = 298)
            {1000000, 2900000,       -1, 0,         672, 320,            -1, 0}};       // 1250000
        DebugSwitches cap, per_cu;
        cap.cluster_cap = 200000;
        per_cu.clusters_per_cu = 1;
        for (const auto& c : t) {
            check_dyn("scenes", plan_dynamic_clusters(c.n, true, 256, active(0, c.manifolds), off), c.c0, c.s0);
            check_dyn("scenes, cap", plan_dynamic_clusters(c.n, true, 256, active(0, c.manifolds), cap), c.c1, c.s1);
            check_dyn("scenes, per CU", plan_dynamic_clusters(c.n, true, 256, active(0, c.manifolds), per_cu), c.c2, c.s2);
        }
    }
}

// ---- cluster_homes: Morton order z | y | x per bit; a cube's corners sort by (z, y, x) ------------------------------------------
static void homes() {
    {
        // corner c = x + 2 y + 4 z sits at body index where[c]
        const uint32_t body_of_corner[8] = {5, 2, 7, 0, 3, 6, 1, 4};
        std::vector<float> pos(3 * 10, 99.0f);  // two ghost slots behind: never read
        for (uint32_t c = 0; c < 8; ++c) {
            const uint32_t i = body_of_corner[c];
            pos[3 * i] = 2.0f + (float)(c & 1u); pos[3 * i + 1] = -1.0f + (float)((c >> 1) & 1u); pos[3 * i + 2] = 10.0f + (float)(c >> 2);
        }
        const ClusterHomes h = cluster_homes(10, 8, pos.data(), 64);
        CHECK("corners", h.clusters, 1); CHECK("corners", h.cluster_slot.size(), 10); CHECK("corners", h.cluster_body.size(), 64);
        for (uint32_t c = 0; c < 8; ++c) { CHECK("corners", h.cluster_body[c], body_of_corner[c]); CHECK("corners", h.cluster_slot[body_of_corner[c]], c); }
        for (uint32_t r = 8; r < 64; ++r) CHECK("empty homes", h.cluster_body[r], 0xFFFFFFFFu);
        CHECK("ghost", h.cluster_slot[8], 0xFFFFFFFFu); CHECK("ghost", h.cluster_slot[9], 0xFFFFFFFFu);
    }
    {
        seed(7);
        std::vector<float> pos(3 * 130);
        for (float& p : pos) p = rnd(-5.0f, 5.0f);
        const ClusterHomes h = cluster_homes(130, 130, pos.data(), 64);
        CHECK("130", h.clusters, 3); CHECK("130", h.cluster_body.size(), 192);
        std::set<uint32_t> seen;
        for (uint32_t r = 0; r < 130; ++r) { seen.insert(h.cluster_body[r]); CHECK("130", h.cluster_slot[h.cluster_body[r]], r); }
        CHECK("130: every body once", seen.size(), 130); CHECK("130", *seen.rbegin(), 129);
        for (uint32_t r = 130; r < 192; ++r) CHECK("130", h.cluster_body[r], 0xFFFFFFFFu);
    }
    {   // all at one point: the span is floored at 1e-6, every key is 0, the order is the bodies'
        std::vector<float> pos(3 * 70, 4.0f);
        const ClusterHomes h = cluster_homes(70, 70, pos.data(), 64);
        CHECK("one point", h.clusters, 2);
        for (uint32_t i = 0; i < 70; ++i) CHECK("one point", h.cluster_slot[i], i);
    }
}

// ---- build_static_set against brute force ------------------------------------------------------------------------------------
struct Box { float lo[3], hi[3]; };
static bool overlap(const float* b, const Box& q) {  // static.hip st_overlap on box[8 k ..]
    return b[0] <= q.hi[0] && q.lo[0] <= b[4] && b[1] <= q.hi[1] && q.lo[1] <= b[5] && b[2] <= q.hi[2] && q.lo[2] <= b[6];
}
// the visit rule of static.hip st_visit, restated: the large list, then the cells of the query box; a pair is kept only in
// the first cell of the intersection of the two cell ranges
static std::vector<uint32_t> visit(const StaticSet& s, const Box& q) {
    std::vector<uint32_t> out;
    for (uint32_t j = 0; j < s.n_large; ++j)
        if (overlap(&s.box[8 * (size_t)s.large[j]], q)) out.push_back(s.large[j]);
    if (s.dim[0] == 0) return out;
    uint32_t c0[3], c1[3];
    for (int a = 0; a < 3; ++a) { c0[a] = st_cell(q.lo[a], s.org[a], s.inv_cell, s.dim[a]); c1[a] = st_cell(q.hi[a], s.org[a], s.inv_cell, s.dim[a]); }
    for (uint32_t z = c0[2]; z <= c1[2]; ++z)
        for (uint32_t y = c0[1]; y <= c1[1]; ++y)
            for (uint32_t x = c0[0]; x <= c1[0]; ++x) {
                const uint32_t c = (z * s.dim[1] + y) * s.dim[0] + x;
                for (uint32_t e = s.cell_start[c]; e < s.cell_start[c + 1]; ++e) {
                    const uint32_t k = s.cell_ids[e];
                    if (!overlap(&s.box[8 * (size_t)k], q)) continue;
                    uint32_t p;
                    std::memcpy(&p, &s.box[8 * (size_t)k + 3], 4);
                    const uint32_t fx = std::max(c0[0], p & 1023u), fy = std::max(c0[1], (p >> 10) & 1023u), fz = std::max(c0[2], p >> 20);
                    if (fx == x && fy == y && fz == z) out.push_back(k);
                }
            }
    return out;
}
struct Statics { std::vector<float> pos, rot, he; std::vector<uint32_t> shape; uint64_t n() const { return shape.size(); } };
static void add(Statics& s, float x, float y, float z, float hx, float hy, float hz, uint32_t shape) {
    s.pos.insert(s.pos.end(), {x, y, z}); s.he.insert(s.he.end(), {hx, hy, hz}); s.shape.push_back(shape);
    s.rot.insert(s.rot.end(), {0.0f, 0.0f, 0.0f, 1.0f});
}
static void check_set(const char* what, const Statics& in, const StaticSet& s, float reach, float max_half) {
    const uint64_t n = in.n();
    CHECK(what, s.geo.size(), 16 * n); CHECK(what, s.rc.size(), 12 * n); CHECK(what, s.box.size(), 8 * n);
    CHECK(what, s.filt.size(), 2 * n); CHECK(what, s.mat.size(), 2 * n);
    const uint64_t cells = (uint64_t)s.dim[0] * s.dim[1] * s.dim[2];
    CHECK(what, s.cell_start.size(), cells ? cells + 1 : 2);
    CHECK(what, s.cell_ids.size(), std::max<uint64_t>(1, s.cell_start.back()));
    std::vector<uint8_t> is_large(n, 0);
    for (uint32_t j = 0; j < s.n_large; ++j) { is_large[s.large[j]] = 1; if (j) CHECK("large ascending", s.large[j - 1] < s.large[j], true); }
    for (uint64_t c = 0; c < cells; ++c)
        for (uint32_t e = s.cell_start[c] + 1; e < s.cell_start[c + 1]; ++e) CHECK("cell lists ascending", s.cell_ids[e - 1] < s.cell_ids[e], true);
    for (uint64_t k = 0; k < n; ++k) {
        uint32_t w;
        CHECK("records", std::memcmp(&s.geo[16 * k], &in.pos[3 * k], 12), 0); CHECK("records", std::memcmp(&s.rc[12 * k], &in.pos[3 * k], 12), 0);
        std::memcpy(&w, &s.geo[16 * k + 3], 4); CHECK("records", w, in.shape[k]);
        std::memcpy(&w, &s.rc[12 * k + 3], 4); CHECK("records", w, in.shape[k]);
        std::memcpy(&w, &s.rc[12 * k + 11], 4); CHECK("records", w, 0x80000000u | k);
        CHECK("records", std::memcmp(&s.geo[16 * k + 8], &in.he[3 * k], 12), 0); CHECK("records", std::memcmp(&s.rc[12 * k + 8], &in.he[3 * k], 12), 0);
        CHECK("records", s.geo[16 * k + 7] == 1.0f && s.rc[12 * k + 7] == 1.0f, true);
        CHECK("defaults", s.filt[2 * k], 0xFFFF0001u); CHECK("defaults", s.filt[2 * k + 1], 0);
        CHECK("defaults", s.mat[2 * k] == 0.5f && s.mat[2 * k + 1] == 0.0f, true);
        if (in.shape[k] == PHYS_SHAPE_BOX)  // identity rotation: the fattened box is centre -+ (half extent + margin), to rounding
            for (int a = 0; a < 3; ++a) {
                const float h = in.he[3 * k + a] + 0.02f, tol = 1e-5f * (1.0f + std::fabs(in.pos[3 * k + a]) + h);
                CHECK("fattened box", std::fabs(s.box[8 * k + a] - (in.pos[3 * k + a] - h)) <= tol && std::fabs(s.box[8 * k + 4 + a] - (in.pos[3 * k + a] + h)) <= tol, true);
            }
        if (!is_large[k] && cells) {  // the packed first cell is st_cell of the low corner
            std::memcpy(&w, &s.box[8 * k + 3], 4);
            for (int a = 0; a < 3; ++a) CHECK("first cell", (w >> (10 * a)) & 1023u, st_cell(s.box[8 * k + a], s.org[a], s.inv_cell, s.dim[a]));
        }
    }
    // 200 query boxes: the visit finds exactly the statics whose fattened box overlaps, each once
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    for (uint64_t k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], in.pos[3 * k + a]); hi[a] = std::max(hi[a], in.pos[3 * k + a]); }
    uint64_t hits = 0;
    for (int qn = 0; qn < 200; ++qn) {
        Box q;
        for (int a = 0; a < 3; ++a) {
            const float c = rnd(lo[a] - reach, hi[a] + reach), h = rnd(0.0f, max_half);
            q.lo[a] = c - h; q.hi[a] = c + h;
        }
        std::vector<uint32_t> got = visit(s, q), want;
        for (uint64_t k = 0; k < n; ++k) if (overlap(&s.box[8 * k], q)) want.push_back((uint32_t)k);
        std::sort(got.begin(), got.end());
        ++g_checks;
        if (got != want) { std::printf("MISMATCH %s: query %d finds %zu statics, brute force %zu\n", what, qn, got.size(), want.size()); std::exit(1); }
        hits += want.size();
    }
    CHECK(what, hits > 50, true);  // the queries meet statics
}
static StaticSet build(const Statics& s, bool with_rot = true) {
    return build_static_set(s.n(), s.pos.data(), with_rot ? s.rot.data() : nullptr, s.shape.data(), s.he.data(), 0.02f, 0.5f);
}
static void statics() {
    Statics plane;
    seed(11);
    for (int k = 0; k < 40; ++k) add(plane, rnd(0.0f, 20.0f), 0.0f, rnd(0.0f, 20.0f), rnd(0.3f, 0.8f), rnd(0.3f, 0.8f), rnd(0.3f, 0.8f), PHYS_SHAPE_BOX);
    {
        const StaticSet s = build(plane);
        CHECK("plane", s.n_large, 0); CHECK("plane", s.dim[0] > 1 && s.dim[1] >= 1 && s.dim[2] > 1, true); CHECK("plane", s.capsules, false);
        seed(12);
        check_set("plane", plane, s, 2.0f, 3.0f);
        const StaticSet t = build(plane, false);  // rot null: identity, the same set
        CHECK("rot null", s.geo == t.geo && s.rc == t.rc && s.box == t.box && s.cell_start == t.cell_start && s.cell_ids == t.cell_ids, true);
    }
    {
        Statics slab = plane;
        add(slab, 10.0f, -1.0f, 10.0f, 15.0f, 0.5f, 15.0f, PHYS_SHAPE_BOX);  // covers everything: 20-odd cells along x and z
        add(slab, 3.0f, 1.0f, 3.0f, 0.4f, 1.0f, 0.0f, PHYS_SHAPE_CAPSULE);
        const StaticSet s = build(slab);
        CHECK("slab", s.n_large, 1); CHECK("slab", s.large[0], 40); CHECK("slab", s.capsules, true);
        seed(13);
        check_set("slab", slab, s, 2.0f, 3.0f);
    }
    {   // 30 statics over 5000 units: 4800 cells per axis at the median edge - coarsened until <= 1024 per axis and 4096 in all
        Statics far;
        seed(14);
        for (int k = 0; k < 30; ++k) add(far, rnd(0.0f, 5000.0f), rnd(0.0f, 5000.0f), rnd(0.0f, 5000.0f), rnd(0.3f, 0.8f), rnd(0.3f, 0.8f), rnd(0.3f, 0.8f), k % 2 ? PHYS_SHAPE_BOX : PHYS_SHAPE_SPHERE);
        const StaticSet s = build(far);
        CHECK("far", s.n_large, 0);
        CHECK("far", 1.0f / s.inv_cell > 100.0f, true);  // the median edge is below 1.7
        for (int a = 0; a < 3; ++a) CHECK("far", s.dim[a] >= 2 && s.dim[a] <= kStMaxDim, true);
        CHECK("far", (uint64_t)(s.dim[0] - 1) * (s.dim[1] - 1) * (s.dim[2] - 1) <= 4096, true);  // dim = floor(span / cell) + 2 per axis
        seed(15);
        check_set("far", far, s, 100.0f, 2500.0f);
    }
    {
        Statics one;
        add(one, 1.0f, 2.0f, 3.0f, 0.5f, 0.5f, 0.5f, PHYS_SHAPE_BOX);
        const StaticSet s = build(one);
        CHECK("n = 1", s.n_large, 0); CHECK("n = 1", s.dim[0] * s.dim[1] * s.dim[2] >= 1, true);
        Box q = {{0.0f, 1.0f, 2.0f}, {2.0f, 3.0f, 4.0f}};
        CHECK("n = 1", visit(s, q).size(), 1);
        Box miss = {{5.0f, 1.0f, 2.0f}, {6.0f, 3.0f, 4.0f}};
        CHECK("n = 1", visit(s, miss).size(), 0);
    }
    {   // zero extent: the box is the margin's, the cell edge 0.04
        Statics zero;
        add(zero, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, PHYS_SHAPE_SPHERE);
        add(zero, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, PHYS_SHAPE_BOX);
        const StaticSet s = build(zero);
        CHECK("zero extent", s.n_large, 0); CHECK("zero extent", std::fabs(1.0f / s.inv_cell - 0.04f) < 1e-6f, true);
        Box q = {{-0.01f, -0.01f, -0.01f}, {0.01f, 0.01f, 0.01f}};
        CHECK_VEC("zero extent", visit(s, q), 0);
        Box both = {{-1.0f, -1.0f, -1.0f}, {2.0f, 1.0f, 1.0f}};
        CHECK("zero extent", visit(s, both).size(), 2);
    }
    {   // all large: extents whose span overflows a float (finite arguments) - no grid at all
        Statics huge;
        add(huge, 0.0f, 0.0f, 0.0f, 3.0e38f, 3.0e38f, 3.0e38f, PHYS_SHAPE_BOX);
        add(huge, 1.0f, 0.0f, 0.0f, 3.0e38f, 3.0e38f, 3.0e38f, PHYS_SHAPE_BOX);
        const StaticSet s = build(huge);
        CHECK("all large", s.n_large, 2); CHECK("all large", s.dim[0] | s.dim[1] | s.dim[2], 0); CHECK("all large", s.inv_cell == 0.0f, true);
        CHECK_VEC("all large", s.large, 0, 1); CHECK_VEC("all large", s.cell_start, 0, 0); CHECK_VEC("all large", s.cell_ids, 0);
        Box q = {{5.0f, 5.0f, 5.0f}, {6.0f, 6.0f, 6.0f}};
        CHECK("all large", visit(s, q).size(), 2);
    }
}

// ---- stage_bodies ------------------------------------------------------------------------------------------------------------
static void bodies() {
    const float inf = std::numeric_limits<float>::infinity();
    {   // every optional array null: RigidBody::new
        const float pos[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
        const BodyStaging s = stage_bodies(2, 0, pos, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.5f);
        CHECK("defaults", s.pos.size(), 6); CHECK("defaults", std::memcmp(s.pos.data(), pos, 24), 0);
        for (int i = 0; i < 2; ++i) {
            const float rot[4] = {0.0f, 0.0f, 0.0f, 1.0f}, vel[8] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
            const float eye[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, diag[4] = {1.0f, 1.0f, 1.0f, 0.0f}, zero[3] = {0.0f, 0.0f, 0.0f};
            CHECK("defaults", std::memcmp(&s.rot[4 * i], rot, 16), 0); CHECK("defaults", std::memcmp(&s.vel[8 * i], vel, 32), 0);
            for (int k = 0; k < 9; ++k) CHECK("defaults", s.inv_inertia[9 * i + k] == eye[k], true);  // (the adjugate leaves a -0)
            CHECK("defaults", std::memcmp(&s.inv_inertia_diag[4 * i], diag, 16), 0);
            CHECK("defaults", std::memcmp(&s.half_extent[3 * i], zero, 12), 0);
            CHECK("defaults", s.shape[i], PHYS_SHAPE_NONE); CHECK("defaults", s.global_id[i], i);
            CHECK("defaults", s.filt[2 * i], 0xFFFF0001u); CHECK("defaults", s.filt[2 * i + 1], 0);
            CHECK("defaults", s.mat[2 * i] == 0.5f && s.mat[2 * i + 1] == 0.0f, true);
        }
        CHECK("defaults", s.singular_inertia, false); CHECK("defaults", s.all_diag_inertia, true); CHECK("defaults", s.uniform_inertia, true);
        CHECK("defaults", s.body_capsules, false);
    }
    const float pos3[9] = {0};
    {   // given arrays are taken; a mass of 4: inverse 0.25
        const float rot[4] = {0.5f, 0.5f, 0.5f, 0.5f}, lin[3] = {1.0f, 2.0f, 3.0f}, ang[3] = {4.0f, 5.0f, 6.0f}, mass[1] = {4.0f}, he[3] = {0.1f, 0.2f, 0.3f};
        const uint32_t shape[1] = {PHYS_SHAPE_BOX};
        const BodyStaging s = stage_bodies(1, 0, pos3, rot, lin, ang, mass, nullptr, shape, he, 0.25f);
        const float vel[8] = {1.0f, 2.0f, 3.0f, 0.25f, 4.0f, 5.0f, 6.0f, 4.0f};
        CHECK("given", std::memcmp(s.vel.data(), vel, 32), 0); CHECK("given", std::memcmp(s.rot.data(), rot, 16), 0);
        CHECK("given", std::memcmp(s.half_extent.data(), he, 12), 0); CHECK("given", s.shape[0], PHYS_SHAPE_BOX); CHECK("given", s.mat[0] == 0.25f, true);
    }
    {   // a singular tensor: zero inverse, the flag; (zero differs from body 0's identity: not uniform)
        float I[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, /* body 1 */ 1, 2, 3, 2, 4, 6, 0, 0, 1};
        const BodyStaging s = stage_bodies(2, 0, pos3, nullptr, nullptr, nullptr, nullptr, I, nullptr, nullptr, 0.5f);
        CHECK("singular", s.singular_inertia, true);
        for (int k = 0; k < 9; ++k) CHECK("singular", s.inv_inertia[9 + k] == 0.0f, true);
        CHECK("singular", s.all_diag_inertia, true); CHECK("singular", s.uniform_inertia, false);
    }
    {   // one off-diagonal entry: not all diagonal, and so not uniform (both bodies have the same tensor)
        float I[18] = {2, 1, 0, 1, 2, 0, 0, 0, 1, 2, 1, 0, 1, 2, 0, 0, 0, 1};
        const BodyStaging s = stage_bodies(2, 0, pos3, nullptr, nullptr, nullptr, nullptr, I, nullptr, nullptr, 0.5f);
        CHECK("off-diagonal", s.singular_inertia, false); CHECK("off-diagonal", s.all_diag_inertia, false); CHECK("off-diagonal", s.uniform_inertia, false);
        CHECK("off-diagonal", s.inv_inertia[1] != 0.0f, true);
    }
    {   // two different diagonal tensors: 1 and 2 -> inverses 1 and 0.5 (cofactor 4 over determinant 8)
        float I[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 0, 0, 0, 2, 0, 0, 0, 2};
        const BodyStaging s = stage_bodies(2, 0, pos3, nullptr, nullptr, nullptr, nullptr, I, nullptr, nullptr, 0.5f);
        CHECK("two diagonals", s.all_diag_inertia, true); CHECK("two diagonals", s.uniform_inertia, false);
        CHECK("two diagonals", s.inv_inertia_diag[4] == 0.5f && s.inv_inertia_diag[5] == 0.5f && s.inv_inertia_diag[6] == 0.5f && s.inv_inertia_diag[7] == 0.0f, true);
        CHECK("two diagonals", s.inv_inertia[9] == 0.5f && s.inv_inertia[13] == 0.5f && s.inv_inertia[17] == 0.5f && s.inv_inertia[10] == 0.0f, true);
    }
    {
        const uint32_t shape[3] = {PHYS_SHAPE_BOX, PHYS_SHAPE_CAPSULE, PHYS_SHAPE_SPHERE};
        CHECK("capsule", stage_bodies(3, 0, pos3, nullptr, nullptr, nullptr, nullptr, nullptr, shape, nullptr, 0.5f).body_capsules, true);
        CHECK("capsule", stage_bodies(1, 0, pos3, nullptr, nullptr, nullptr, nullptr, nullptr, shape, nullptr, 0.5f).body_capsules, false);
    }
    {   // two ghost slots: identity rotation, inverse mass 0, mass +inf, zero tensors, no shape, no id; never uniform
        const uint32_t shape[1] = {PHYS_SHAPE_BOX};
        const BodyStaging s = stage_bodies(1, 2, pos3, nullptr, nullptr, nullptr, nullptr, nullptr, shape, nullptr, 0.5f);
        CHECK("ghosts", s.pos.size(), 9); CHECK("ghosts", s.vel.size(), 24); CHECK("ghosts", s.shape.size(), 3);
        for (int i = 1; i < 3; ++i) {
            const float rot[4] = {0.0f, 0.0f, 0.0f, 1.0f}, vel[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, inf};
            CHECK("ghosts", std::memcmp(&s.rot[4 * i], rot, 16), 0); CHECK("ghosts", std::memcmp(&s.vel[8 * i], vel, 32), 0);
            for (int k = 0; k < 9; ++k) CHECK("ghosts", s.inv_inertia[9 * i + k] == 0.0f, true);
            CHECK("ghosts", s.shape[i], PHYS_SHAPE_NONE); CHECK("ghosts", s.global_id[i], 0xFFFFFFFFu);
            CHECK("ghosts", s.filt[2 * i], 0xFFFF0001u); CHECK("ghosts", s.mat[2 * i] == 0.5f, true);
        }
        CHECK("ghosts", s.uniform_inertia, false); CHECK("ghosts", s.all_diag_inertia, true);
    }
}

// ---- constraint_columns: column = 6 body + 3 kind + axis, row = 3 constraint + axis -------------------------------------------
static void constraints() {
    auto c = [](uint32_t kind, uint32_t body) { Constraint x; x.kind = kind; x.body = body; x.target[0] = x.target[1] = x.target[2] = 0.0f; return x; };
    ConstraintColumns t = constraint_columns({});
    CHECK("none", t.col_id.size(), 0); CHECK_VEC("none", t.col_ptr, 0); CHECK("none", t.col_rows.size() + t.row_cidx.size(), 0);
    t = constraint_columns({c(0, 2)});
    CHECK_VEC("one", t.col_id, 12, 13, 14); CHECK_VEC("one", t.col_ptr, 0, 1, 2, 3); CHECK_VEC("one", t.col_rows, 0, 1, 2); CHECK_VEC("one", t.row_cidx, 0, 1, 2);
    t = constraint_columns({c(1, 1), c(1, 1)});  // shared columns, rows in constraint order
    CHECK_VEC("shared", t.col_id, 9, 10, 11); CHECK_VEC("shared", t.col_ptr, 0, 2, 4, 6); CHECK_VEC("shared", t.col_rows, 0, 3, 1, 4, 2, 5);
    CHECK_VEC("shared", t.row_cidx, 0, 1, 2, 0, 1, 2);
    t = constraint_columns({c(1, 0), c(0, 0)});  // orientation, then point, on body 0: six columns, the point's first
    CHECK_VEC("six", t.col_id, 0, 1, 2, 3, 4, 5); CHECK_VEC("six", t.col_ptr, 0, 1, 2, 3, 4, 5, 6); CHECK_VEC("six", t.col_rows, 3, 4, 5, 0, 1, 2);
    CHECK_VEC("six", t.row_cidx, 3, 4, 5, 0, 1, 2);
}

// ---- shape_set_error, pack_filters, pack_materials -----------------------------------------------------------------------------
static void validation() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (const char* noun : {"static collider", "trigger"}) {
        const std::string N = noun;
        std::string msg;
        uint32_t shape[4] = {PHYS_SHAPE_SPHERE, PHYS_SHAPE_BOX, PHYS_SHAPE_CAPSULE, PHYS_SHAPE_BOX};
        float pos[12] = {0}, he[12] = {0}, rot[16] = {0};
        CHECK(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg) == nullptr, true);
        CHECK(noun, shape_set_error(noun, 4, shape, pos, nullptr, he, msg) == nullptr, true);
        CHECK(noun, shape_set_error(noun, 0, nullptr, nullptr, nullptr, nullptr, msg) == nullptr, true);
        shape[3] = PHYS_SHAPE_NONE;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 3: shape is neither SPHERE nor BOX nor CAPSULE");
        shape[3] = 4u;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 3: shape is neither SPHERE nor BOX nor CAPSULE");
        he[3 * 3 + 1] = nan;  // the shape is checked first
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 3: shape is neither SPHERE nor BOX nor CAPSULE");
        shape[3] = PHYS_SHAPE_BOX;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 3: non-finite pose or half extent");
        he[3 * 3 + 1] = 0.0f; pos[3 * 2] = inf;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 2: non-finite pose or half extent");
        pos[3 * 2] = 0.0f; rot[4 * 1 + 3] = nan;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 1: non-finite pose or half extent");
        CHECK(noun, shape_set_error(noun, 4, shape, pos, nullptr, he, msg) == nullptr, true);  // rot null: not looked at
        rot[4 * 1 + 3] = 0.0f; he[3 * 2 + 2] = -0.5f;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 2: negative half extent");
        he[3 * 2 + 0] = -inf;  // both non-finite and negative: non-finite is said first
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 2: non-finite pose or half extent");
        he[3 * 2 + 0] = 0.0f; he[0] = -1.0f; shape[1] = 0u;  // several offend: the first index
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 0: negative half extent");
        he[0] = 0.0f;
        CHECK_STR(noun, shape_set_error(noun, 4, shape, pos, rot, he, msg), N + " 1: shape is neither SPHERE nor BOX nor CAPSULE");
    }
    {
        std::vector<uint32_t> f;
        pack_filters(2, nullptr, nullptr, nullptr, f);
        CHECK_VEC("filters", f, 0xFFFF0001u, 0, 0xFFFF0001u, 0);
        const uint16_t cat[2] = {2, 4}, mask[2] = {0x00FF, 0x8000};
        const int16_t group[2] = {-1, 3};
        pack_filters(2, cat, mask, group, f);
        CHECK_VEC("filters", f, 0x00FF0002u, 0xFFFFFFFFu, 0x80000004u, 3);
        std::vector<float> m;
        CHECK("materials", pack_materials(2, nullptr, nullptr, 0.5f, m), true);
        CHECK("materials", m[0] == 0.5f && m[1] == 0.0f && m[2] == 0.5f && m[3] == 0.0f, true);
        const float fr[1] = {-0.1f}, e0[1] = {1.0f}, e1[1] = {1.5f}, fn[1] = {nan};
        CHECK("materials", pack_materials(1, fr, nullptr, 0.5f, m), false); CHECK("materials", pack_materials(1, fn, nullptr, 0.5f, m), false);
        CHECK("materials", pack_materials(1, nullptr, e0, 0.5f, m), true); CHECK("materials", pack_materials(1, nullptr, e1, 0.5f, m), false);
        CHECK("materials", pack_materials(1, nullptr, fn, 0.5f, m), false);
    }
}

// ---- volumes: include/spec/volume.h vol_record_make, stage_triggers, restage_trigger_poses, trigger_records, field_records ------
// The rotation used below is 90 degrees about z: q = (0, 0, s, s) with s = float(sqrt(1/2)) = 0x3F3504F3 = 11863283 * 2^-24.
// quat_to_m33 by hand: s * s = 140737483538089 * 2^-48 = 1/2 - 0.574 * 2^-25, which rounds to a = 1/2 - 2^-25 (0x3EFFFFFF), so
// ww = kk = a and ii = jj = 0; wk = (s * s) * 2 = b = 1 - 2^-24 (0x3F7FFFFF), every other product is +0. The matrix:
//   m0 = (a + 0 - 0) - a = +0   m1 = 0 - b = -b   m2 = 0      m3 = b + 0 = b   m4 = (a - 0 + 0) - a = +0   m5 = 0
//   m6 = 0   m7 = 0   m8 = (a - 0 - 0) + a = b
static void check_words(const char* what, const void* got, std::initializer_list<uint32_t> want) {
    std::vector<uint32_t> g(want.size());
    std::memcpy(g.data(), got, 4 * want.size());
    size_t k = 0;
    for (uint32_t w : want) {
        ++g_checks;
        if (g[k] != w) { std::printf("MISMATCH %s: word %zu = %08x, expected %08x\n", what, k, g[k], w); std::exit(1); }
        ++k;
    }
}
static void volumes() {
    const uint32_t one = 0x3F800000u, m_one = 0xBF800000u, b = 0x3F7FFFFFu, m_b = 0xBF7FFFFFu, s = 0x3F3504F3u;
    const float sf = vol_u2f(s), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK("sizes", sizeof(vol_record), 96); CHECK("sizes", sizeof(ff_record), 112); CHECK("sizes", sizeof(vol_f4), 16);
    {   // a unit sphere at the origin, rot NULL and mask NULL: box -+1 (e = (1, 1, 1); (0 - 1) - 0, (0 + 1) + 0), the identity matrix
        // (ww = 1, every other term +0), mask 0xFFFF
        const uint32_t shape[1] = {PHYS_SHAPE_SPHERE};
        const float pos[3] = {0.0f, 0.0f, 0.0f}, he[3] = {1.0f, 0.0f, 0.0f};
        const TriggerStaging st = stage_triggers(1, shape, pos, nullptr, he, nullptr);
        CHECK("sphere", st.masked, false); CHECK("sphere", st.staged.size(), 1);
        CHECK("sphere", st.staged[0].q.i == 0.0f && st.staged[0].q.j == 0.0f && st.staged[0].q.k == 0.0f && st.staged[0].q.w == 1.0f, true);
        const std::vector<vol_record> rec = trigger_records(st.staged);
        CHECK("sphere", rec.size(), 1);
        check_words("sphere", rec.data(), {m_one, m_one, m_one, 1u, /**/ one, one, one, 0xFFFFu, /**/ 0, 0, 0, one,
                                           /**/ one, 0, 0, 0, /**/ 0, one, 0, 0, /**/ 0, 0, one, 0});
        CHECK("accessors", vol_word(rec[0].r[0]), PHYS_SHAPE_SPHERE); CHECK("accessors", vol_mask(rec[0].r[1]), 0xFFFFu);
        CHECK("accessors", vol_lo(rec[0].r[0]).y == -1.0f && vol_hi(rec[0].r[1]).z == 1.0f, true);
        CHECK("accessors", vol_half_extent(rec[0].r[2], rec[0].r[3], rec[0].r[4]).x == 1.0f, true);
        CHECK("accessors", vol_rotation(rec[0].r[3], rec[0].r[4], rec[0].r[5]).m[4] == 1.0f, true);
        const v3 in = v3_make(1.0f, -1.0f, 0.0f), out = v3_make(0.0f, 1.5f, 0.0f), bad = v3_make(nan, 0.0f, 0.0f);
        CHECK("box", vol_box_meets(rec[0].r[0], rec[0].r[1], in, in), 1); CHECK("box", vol_box_meets(rec[0].r[0], rec[0].r[1], out, out), 0);
        CHECK("box", vol_box_meets(rec[0].r[0], rec[0].r[1], bad, bad), 0); CHECK("box", vol_box_meets(rec[0].r[0], rec[0].r[1], in, out), 1);
        CHECK("none", stage_triggers(0, nullptr, nullptr, nullptr, nullptr, nullptr).masked, false);
    }
    // three triggers with rotations and masks: a sphere, a box (1, 2, 3) at the origin and a capsule (r 0.5, hl 1) at (10, 20, 30),
    // the last two turned 90 degrees about z.
    //   box: e.x = (0 * 1 + b * 2) + 0 * 3 = 2 - 2^-23 (0x3FFFFFFF), e.y = (b * 1 + 0) + 0 = b, e.z = (0 + 0) + b * 3 = 3 - 0.75 * 2^-22,
    //        which rounds to 3 - 2^-22 (0x403FFFFF); lo = (0 - e) - 0 = -e, hi = e: +-(2, 1, 3) to the rounding of the matrix
    //   capsule: e.x = b * 1 + 0.5 = 1.5 - 2^-24, a tie that rounds to the even 1.5; e.y = e.z = 0 * 1 + 0.5: lo = (8.5, 19.5, 29.5),
    //        hi = (11.5, 20.5, 30.5), all exact
    const uint32_t shape[3] = {PHYS_SHAPE_SPHERE, PHYS_SHAPE_BOX, PHYS_SHAPE_CAPSULE};
    const float pos[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 10.0f, 20.0f, 30.0f};
    const float rot[12] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, sf, sf, 0.0f, 0.0f, sf, sf};
    const float he[9] = {1.0f, 0.0f, 0.0f, 1.0f, 2.0f, 3.0f, 0.5f, 1.0f, 0.0f};
    const uint16_t mask[3] = {1, 0x00F0, 0x8000};
    TriggerStaging st = stage_triggers(3, shape, pos, rot, he, mask);
    CHECK("three", st.masked, true);
    std::vector<vol_record> rec = trigger_records(st.staged);
    check_words("three: sphere", &rec[0], {m_one, m_one, m_one, 1u, one, one, one, 1u, 0, 0, 0, one, one, 0, 0, 0, 0, one, 0, 0, 0, 0, one, 0});
    check_words("three: box", &rec[1], {0xBFFFFFFFu, m_b, 0xC03FFFFFu, 2u, /**/ 0x3FFFFFFFu, b, 0x403FFFFFu, 0x00F0u, /**/ 0, 0, 0, one,
                                        /**/ 0, m_b, 0, 0x40000000u, /**/ b, 0, 0, 0x40400000u, /**/ 0, 0, b, 0});
    check_words("three: capsule", &rec[2], {0x41080000u, 0x419C0000u, 0x41EC0000u, 3u, /**/ 0x41380000u, 0x41A40000u, 0x41F40000u, 0x8000u,
                                            /**/ 0x41200000u, 0x41A00000u, 0x41F00000u, 0x3F000000u, /**/ 0, m_b, 0, one, /**/ b, 0, 0, 0,
                                            /**/ 0, 0, b, 0});
    {   // new poses with rot NULL: the stored quaternions stay, and so do rows 3 to 5; the centres and the boxes move (the capsule
        // to the origin: lo = (-1.5, -0.5, -0.5), hi = (1.5, 0.5, 0.5))
        const float pos2[9] = {4.0f, 0.0f, 0.0f, 0.0f, 8.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        CHECK("poses", restage_trigger_poses(st.staged, pos2, nullptr), true);
        const std::vector<vol_record> moved = trigger_records(st.staged);
        for (int k = 0; k < 3; ++k) CHECK("poses: rows 3 to 5", std::memcmp(&moved[k].r[3], &rec[k].r[3], 48), 0);
        CHECK("poses", st.staged[1].q.k == sf && st.staged[1].q.w == sf && st.staged[1].c.y == 8.0f, true);
        check_words("poses: capsule", &moved[2], {0xBFC00000u, 0xBF000000u, 0xBF000000u, 3u, 0x3FC00000u, 0x3F000000u, 0x3F000000u, 0x8000u, 0, 0, 0, 0x3F000000u});
        check_words("poses: sphere", &moved[0], {0x40400000u, m_one, m_one, 1u, 0x40A00000u, one, one, 1u, 0x40800000u, 0, 0, one});  // 3, 5 | 4
        // a NaN in pos, or in rot, is refused and the set is what it was
        float pos3[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rot3[12] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        pos3[4] = nan;
        CHECK("poses: NaN", restage_trigger_poses(st.staged, pos3, rot3), false);
        pos3[4] = 0.0f; rot3[11] = std::numeric_limits<float>::infinity();
        CHECK("poses: inf in rot", restage_trigger_poses(st.staged, pos3, rot3), false);
        const std::vector<vol_record> after = trigger_records(st.staged);
        CHECK("poses: refused, unchanged", std::memcmp(after.data(), moved.data(), 3 * sizeof(vol_record)), 0);
        rot3[11] = 1.0f;  // identity rotations: the box's matrix is the identity now, its box (1, 2, 3) about the origin
        CHECK("poses: rot", restage_trigger_poses(st.staged, pos3, rot3), true);
        const std::vector<vol_record> turned = trigger_records(st.staged);
        check_words("poses: box", &turned[1], {m_one, 0xC0000000u, 0xC0400000u, 2u, one, 0x40000000u, 0x40400000u, 0x00F0u, 0, 0, 0, one,
                                               one, 0, 0, 0x40000000u, 0, one, 0, 0x40400000u, 0, 0, one, 0});
    }
    {   // a finite volume whose box is not: pos 3e38, half extent 3e38 - hi = 3e38 + 3e38 = +inf, the sum of the six is +inf: the
        // inverted box. And a field of the same volume: ff_record_make's first six vectors are vol_record_make's but for the two
        // words the field packs for itself; the same for the turned box above
        const uint32_t big = vol_f2u(3.0e38f), m_big = vol_f2u(-3.0e38f);
        CHECK("3e38", big, 0x7F61B1E6u);  // 3e38 / 2^127 = 1.7632415: mantissa 0.7632415 * 2^23 = 6402534 = 0x61B1E6
        const uint32_t shape1[2] = {PHYS_SHAPE_BOX, PHYS_SHAPE_BOX};
        const float pos1[6] = {3.0e38f, 3.0e38f, 3.0e38f, 0.0f, 0.0f, 0.0f}, he1[6] = {3.0e38f, 3.0e38f, 3.0e38f, 1.0f, 2.0f, 3.0f};
        const float rot1[8] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, sf, sf};
        const std::vector<vol_record> v = trigger_records(stage_triggers(2, shape1, pos1, rot1, he1, nullptr).staged);
        check_words("overflow", &v[0], {big, big, big, 2u, m_big, m_big, m_big, 0xFFFFu, big, big, big, big, one, 0, 0, big, 0, one, 0, big, 0, 0, one, 0});
        CHECK("overflow", vol_box_meets(v[0].r[0], v[0].r[1], v3_make(3.0e38f, 3.0e38f, 3.0e38f), v3_make(3.0e38f, 3.0e38f, 3.0e38f)), 0);
        CHECK("turned box", std::memcmp(&v[1], &rec[1], 28) == 0 && std::memcmp(&v[1].r[2], &rec[1].r[2], 64) == 0, true);  // (the masks differ)
        const uint32_t kind[2] = {PHYS_FIELD_DRAG, PHYS_FIELD_RADIAL}, ex[2] = {0, 2};
        const float vec[6] = {1.0f, 2.0f, 3.0f, 0.0f, 0.0f, 0.0f}, coef[4] = {0.25f, 0.5f, -4.0f, 1.5f};
        const uint16_t fmask[2] = {0x0F0F, 3};
        const FieldStaging fs = stage_fields(2, kind, shape1, pos1, rot1, he1, fmask, vec, coef, ex);
        const std::vector<ff_record> f = field_records(fs.staged);
        CHECK("fields", f.size(), 2);
        for (int k = 0; k < 2; ++k) {
            uint32_t fw[28], vw[24];
            std::memcpy(fw, &f[k], 112); std::memcpy(vw, &v[k], 96);
            for (int i = 0; i < 24; ++i)
                if (i != 3 && i != 7 && i != 23) CHECK("field = volume", fw[i], vw[i]);
            CHECK("field: mask", fw[7], fmask[k]);
            CHECK("field: word", fw[3], kind[k] | (PHYS_SHAPE_BOX << 8) | (ex[k] << 16));
            CHECK("field: coef 0", fw[23], vol_f2u(coef[2 * k])); CHECK("field: coef 1", fw[27], vol_f2u(coef[2 * k + 1]));
            CHECK("field: vec", std::memcmp(&fw[24], &vec[3 * k], 12), 0);
        }
    }
}

// ---- readout.hpp -------------------------------------------------------------------------------------------------------------
static void readout() {
    {
        const uint32_t raw[8] = {5, 9, 1, 7, 5, 2, 1, 3};
        uint32_t out[8] = {77, 77, 77, 77, 77, 77, 77, 77};
        sort_pairs(raw, 4, out, 4);
        const uint32_t all[8] = {1, 3, 1, 7, 5, 2, 5, 9};
        CHECK("sort_pairs", std::memcmp(out, all, 32), 0);
        uint32_t few[8] = {77, 77, 77, 77, 77, 77, 77, 77};
        sort_pairs(raw, 4, few, 2);  // cap < m: the first two of the sorted list, nothing behind them
        const uint32_t two[8] = {1, 3, 1, 7, 77, 77, 77, 77};
        CHECK("sort_pairs, cap < m", std::memcmp(few, two, 32), 0);
        sort_pairs(raw, 0, few, 2);
        CHECK("sort_pairs, m = 0", std::memcmp(few, two, 32), 0);
    }
    {
        const uint32_t rec[5 * 4] = {7, 1, 0, 0, /**/ 2, 9, 0, 0, /**/ 7, 0, 0, 0, /**/ 0, 0xFFFFFFFFu, 0, 0, /**/ 2, 3, 0, 0};
        const std::vector<uint64_t> o = manifold_order(rec, 4, 5);
        const uint64_t want[5] = {3, 4, 1, 2, 0};
        CHECK("manifold_order", o.size(), 5); CHECK("manifold_order", std::memcmp(o.data(), want, 40), 0);
        const uint32_t ab[6] = {3, 1, 3, 0, 1, 8};
        const std::vector<uint64_t> p = manifold_order(ab, 2, 3);
        CHECK("manifold_order, stride 2", p[0] == 2 && p[1] == 1 && p[2] == 0, true);
    }
    {   // events: by step, kind, then the two ids
        phys_contact_event a{}, b{};
        a.step = 1; b.step = 2; a.kind = 2; b.kind = 1;
        CHECK("contact order", event_before(a, b), true); CHECK("contact order", event_before(b, a), false);
        b.step = 1;
        CHECK("contact order", event_before(b, a), true);
        b.kind = 2; a.body_a = 1; b.body_a = 1; a.body_b = 4; b.body_b = 5;
        CHECK("contact order", event_before(a, b), true); CHECK("contact order", event_before(a, a), false);
        a.body_a = 2;
        CHECK("contact order", event_before(b, a), true);
        phys_trigger_event x{}, y{};
        x.step = 3; y.step = 3; x.kind = 1; y.kind = 1; x.trigger = 5; y.trigger = 5; x.body = 1; y.body = 2;
        CHECK("trigger order", event_before(x, y), true); CHECK("trigger order", event_before(y, x), false);
        y.trigger = 4;
        CHECK("trigger order", event_before(y, x), true);
        y.kind = 2;
        CHECK("trigger order", event_before(x, y), true);
        x.step = 4;
        CHECK("trigger order", event_before(y, x), true);
    }
    {
        EventDrain d = drain_rules(5, 100, false, 0);  // count query
        CHECK("count query", d.stored, 5); CHECK("count query", d.dropped, 0); CHECK("count query", d.count_only, true);
        CHECK("count query", d.too_many, false); CHECK("count query", d.clear_cursor, false);
        d = drain_rules(5, 100, true, 4);  // stored > cap: nothing drained
        CHECK("too many", d.stored, 5); CHECK("too many", d.count_only, false); CHECK("too many", d.too_many, true); CHECK("too many", d.clear_cursor, false);
        d = drain_rules(5, 100, true, 5);
        CHECK("drain", d.stored, 5); CHECK("drain", d.too_many, false); CHECK("drain", d.clear_cursor, true);
        d = drain_rules(130, 100, true, 100);  // cursor beyond the capacity: the rest was dropped
        CHECK("dropped", d.stored, 100); CHECK("dropped", d.dropped, 30); CHECK("dropped", d.too_many, false); CHECK("dropped", d.clear_cursor, true);
        d = drain_rules(0, 100, true, 10);
        CHECK("empty", d.stored, 0); CHECK("empty", d.count_only, false); CHECK("empty", d.too_many, false); CHECK("empty", d.clear_cursor, false);
        d = drain_rules(0, 100, true, 0);  // a buffer with cap 0 is a drain, not a count query
        CHECK("cap 0", d.count_only, false); CHECK("cap 0", d.too_many, false);
        d = drain_rules(3, 100, true, 0);
        CHECK("cap 0", d.too_many, true);
    }
    {   // 33 triggers (two words, the second with one valid bit), three bodies
        const uint64_t T = 33, nb = 3;
        uint32_t bits[6] = {0, 0, 0, 0, 0, 0};  // [word * nb + body]
        bits[0 * nb + 2] = (1u << 0) | (1u << 31);         // body 2 in triggers 0 and 31
        bits[0 * nb + 0] = 1u << 31;                       // body 0 in trigger 31
        bits[1 * nb + 1] = (1u << 0) | (1u << 1);          // body 1 in trigger 32; bit 33 is padding
        bits[1 * nb + 0] = 1u << 7;                        // padding only
        uint64_t off[34];
        uint32_t ids[5] = {77, 77, 77, 77, 77};
        CHECK("csr", trigger_bits_to_csr(bits, 2, nb, T, 4, off, ids), true);  // exactly enough
        CHECK("csr", off[0], 0); CHECK("csr", off[1], 1); CHECK("csr", off[31], 1); CHECK("csr", off[32], 3); CHECK("csr", off[33], 4);
        for (int k = 2; k <= 31; ++k) CHECK("csr", off[k], 1);
        CHECK("csr", ids[0] == 2 && ids[1] == 0 && ids[2] == 2 && ids[3] == 1 && ids[4] == 77, true);
        uint32_t none[5] = {77, 77, 77, 77, 77};
        uint64_t off2[34];
        CHECK("csr, one short", trigger_bits_to_csr(bits, 2, nb, T, 3, off2, none), false);
        CHECK("csr, one short", std::memcmp(off, off2, sizeof off), 0); CHECK("csr, one short", none[0], 77);
    }
    {
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, row[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        const uint32_t note[8] = {0xC1u, 5u | (672u << 16), 100, 7, 9, 3u | (4u << 16), 1u | (1u << 4) | (2u << 8), 12u | (3u << 8)};
        const std::string pairs = "pair / manifold capacity exceeded in a step since the last phys_sync (the contact solve of that step was skipped): raise "
                                  "phys_config.max_pairs / max_manifolds";
        const std::string flow = "contact solver hand-off timed out (k_solve_flow) in a step since the last phys_sync; velocities are invalid from that step on";
        const std::string colors = "a body has more than 64 contact manifolds (PHYS_MAX_COLORS): the contact solve of that step was skipped. This limit is not configurable";
        const std::string halo = "halo record / cross-pair capacity exceeded in a step since the last phys_sync";
        const std::string table = "the persistent colour table is full (a look-up or an insert gave up after thousands of slots): the contact solve of that step was "
                                  "skipped. Raise phys_config.max_manifolds";
        const std::string corrupt = "internal error: a solver row names no body of this world and was refused (row 1: a 2, b 3, points 4; colour 7 rows [5, 6), tile base 8)";
        const std::string cluster = "contact solver hand-off timed out (k_solve_cluster) in a step since the last phys_sync; velocities are invalid from that step on. "
                                    "First lane to give up: cluster 5 of 672, row 100, bodies 7 / 9, tickets 3 / 4, waiting A/B 1/0, modes 1/2, iteration 3, colour 12. "
                                    "If other work shares this GPU with phys_update, create the world WITHOUT PHYS_FLAG_EXCLUSIVE_GPU";
        SyncError e = sync_error(0, zero);
        CHECK("no bits", e.code, PHYS_OK); CHECK_STR("no bits", e.message, "");
        e = sync_error(0, note);  // a note without a bit is no error
        CHECK("no bits", e.code, PHYS_OK);
        const struct { uint32_t bits; const uint32_t* dbg; int32_t code; const std::string* text; } t[] = {
            {kOvfPairs, zero, PHYS_ERR_CAPACITY, &pairs}, {kOvfManifolds, zero, PHYS_ERR_CAPACITY, &pairs},
            {kOvfColors, zero, PHYS_ERR_CAPACITY, &colors}, {kOvfHalo, zero, PHYS_ERR_CAPACITY, &halo},
            {kOvfHandoff, zero, PHYS_ERR_HIP, &flow}, {kOvfHandoff, note, PHYS_ERR_HIP, &cluster},
            {kOvfCorruptRow, row, PHYS_ERR_HIP, &corrupt}, {kOvfColorTable, zero, PHYS_ERR_CAPACITY, &table},
            // two bits: corrupt row, hand-off, colours, halo, colour table, the rest - in this order
            {kOvfCorruptRow | kOvfHandoff, row, PHYS_ERR_HIP, &corrupt}, {kOvfHandoff | kOvfColors, zero, PHYS_ERR_HIP, &flow},
            {kOvfColors | kOvfHalo, zero, PHYS_ERR_CAPACITY, &colors}, {kOvfHalo | kOvfColorTable, zero, PHYS_ERR_CAPACITY, &halo},
            {kOvfColorTable | kOvfPairs, zero, PHYS_ERR_CAPACITY, &table}, {kOvfPairs | kOvfManifolds, zero, PHYS_ERR_CAPACITY, &pairs},
            {kOvfColors | kOvfPairs, note, PHYS_ERR_CAPACITY, &colors}, {0x80u, zero, PHYS_ERR_CAPACITY, &pairs}};
        for (const auto& c : t) {
            e = sync_error(c.bits, c.dbg);
            CHECK("sync_error", e.code, c.code); CHECK_STR("sync_error", e.message, *c.text);
        }
    }
}

int main() {
    grid();
    sizes();
    fit();
    dynamic();
    homes();
    statics();
    bodies();
    constraints();
    validation();
    volumes();
    readout();
    std::printf("setup_probe: %d checks passed\n", g_checks);
    return 0;
}
