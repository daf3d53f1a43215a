// setup.hpp — what the host computes ONCE per body set, static set or constraint list, as pure functions of host arrays and a
// few scalars: table sizes, capacities, cluster shapes and homes, the static colliders' grid, the staged body arrays, the
// constraint column tables, the staged force fields and trigger volumes with their records, the checks and the order of a body-edit
// batch, the list of continuous collision (checked by tests/cpp/ccd_probe.cpp), argument validation. Nothing of HIP in here and no phys_world: a host compiler reads it alone,
// and tests/cpp/setup_probe.cpp holds every function to hand-worked values or a brute-force restatement
// (tests/test_setup_cpu.py). The .hip files keep the allocations, the copies and the launches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/physics_hip.h"
#include "../../include/spec/collide.h"
#include "../../include/spec/contact_solve.h"
#include "../../include/spec/det_math.h"
#include "../../include/spec/body_edit.h"
#include "../../include/spec/force_field.h"
#include "../../include/spec/liquid.h"
#include "../../include/spec/vec.h"
#include "plan.hpp"

namespace phys {

// device-side counters of the collision pipeline (one 256-B block, zeroed per step by one memset)
struct StepCounters {
    // the first two words are reserved TOGETHER by the narrow phase: one 64-bit atomic per workgroup trip adds the trip's
    // manifolds to the low word and its uncoloured manifolds to the high one (same-address atomics serialise chip-wide;
    // two of them per trip was two places in that queue)
    uint32_t n_manifolds;    // manifolds written (body-body + ground)
    uint32_t unc_count[3];   // colouring rounds: length of the list of uncoloured manifolds read / written / cleared (rotating)
    uint32_t n_pairs;        // candidate pairs written
    uint32_t n_contacts;     // contact points
    uint32_t n_uncolored;    // manifolds still uncoloured (colouring loop)
    uint32_t n_colors;       // colours in use
    uint32_t color_rounds;
    uint32_t overflow;       // kOvf* bits (below)
    uint32_t n_halo;         // halo records packed
    uint32_t n_cross_pairs;
    uint32_t n_ground_manifolds;
    uint32_t flow_ticket;    // k_solve_flow: next (iteration, row chunk) item to hand to a workgroup
    uint32_t n_grid_ovf;     // slot grid: bodies that found their bucket's four slots taken
    uint32_t n_active;       // owned bodies with at least one manifold in this update (dynamic clusters, cluster.hip)
    uint32_t n_used_buckets; // buckets of the sorted grid holding at least one body (k_cell_assign)
    uint32_t max_region;     // k_find_pairs_brick: most records in the region of one brick (sizes the LDS stage of later updates)
    uint32_t n_new_manifolds;  // manifolds that kept no colour in this update (= the colouring's work; never counted down)
    uint32_t n_static_pairs;      // (body, static) pairs of this update, all of them (k_static_fill; only max_static_pairs are stored)
    uint32_t n_static_manifolds;  // manifolds against a static collider (subset of n_manifolds)
    uint32_t cluster_arrived[2][8];  // k_solve_cluster, per attempt: workgroups that have begun (eight counters: same-address
                                     // atomics serialise chip-wide) ...
    uint32_t cluster_state[2];       // ... and the launch's one decision: 0 undecided, 1 go (all are resident), 2 called off
    uint32_t color_count[kMaxColors];  // manifolds per colour
    uint32_t color_start[kMaxColors + 1];
    // LAST member: survives the per-step reset (only the bytes before it are zeroed), so a wave issues the
    // same-address atomicMax only when it RAISES the bound. It is a running upper bound of the largest
    // fattened-AABB edge (float bits; positive floats order as uints), re-derived from zero every 32 steps.
    // Any upper bound is a valid grid cell size: the pair SET does not depend on it.
    alignas(16) uint32_t max_extent_bits;
    // Every overflow bit ever raised since the host last looked (phys_sync reports and clears it). `overflow` above
    // is per step - the first kernel of the next step zeroes it - so a capacity miss or a hand-off timeout in an
    // EARLY step of a phys_update_n batch would otherwise be gone by the time the host synchronises. Zeroed by
    // neither the per-step reset nor the extent restart (both stop short of it).
    uint32_t sticky_overflow;
    uint32_t n_ghosts;   // ghost slots filled by the last phys_halo_unpack_ghosts (set before the update: not part of the per-step reset)
    uint32_t n_halo_low; // neighbour exchange: records of the LOW-face block (n_halo then counts the high-face block; the stats add them)
    uint32_t debug[8];  // what a kernel that refused a corrupt row saw (overflow bit 5); never read by device code
};
static_assert(offsetof(StepCounters, n_manifolds) % 8 == 0 && offsetof(StepCounters, unc_count) == offsetof(StepCounters, n_manifolds) + 4,
              "n_manifolds | unc_count[0] are one aligned 64-bit word");
// the bits of StepCounters::overflow / sticky_overflow (phys_stats.overflow shows them; phys_sync turns them into errors)
constexpr uint32_t kOvfPairs = 1u;        // bit 0: candidate pairs or (body, static) pairs beyond their capacity
constexpr uint32_t kOvfManifolds = 2u;    // bit 1: manifolds beyond max_manifolds
constexpr uint32_t kOvfColors = 4u;       // bit 2: more than kMaxColors manifolds at one body
constexpr uint32_t kOvfHalo = 8u;         // bit 3: halo records, ghosts or cross pairs beyond their capacity
constexpr uint32_t kOvfHandoff = 16u;     // bit 4: solver hand-off timeout
constexpr uint32_t kOvfCorruptRow = 32u;  // bit 5: corrupt solver row refused (StepCounters::debug says which)
constexpr uint32_t kOvfColorTable = 64u;  // bit 6: colour table walk given up
// bit 8, sticky word ONLY (edit.hip; the per-step word would make the next update skip its contact solve): a body edit on
// device arrays met ids out of order or out of range. phys_sync reports it as PHYS_ERR_INVALID_ARG, behind everything else.
constexpr uint32_t kOvfBadEdit = 0x100u;
constexpr size_t kCountersStepResetBytes = offsetof(StepCounters, max_extent_bits);
constexpr size_t kCountersExtentResetBytes = offsetof(StepCounters, sticky_overflow);

constexpr uint32_t kFilterDefaultWord = 0xFFFF0001u;  // category 0x0001 | mask 0xFFFF << 16 (kernels.hpp: collision filters)

struct Constraint {
    uint32_t kind;  // 0 fix point, 1 fix orientation
    uint32_t body;
    float target[3];
};

// ---- broad phase: the bucket table (phys_set_bodies) ---------------------------------------------------------------------
// split of the broad phase's bucket table over the three axes (kernels.hpp: grid_bucket)
struct GridShape {
    uint32_t mx = 7, my = 7, mz = 7;  // per-axis masks: cells per axis - 1 (each >= 3)
    uint32_t sx = 1, sy = 1;          // bits of the brick coordinates along x and y (= axis bits - 2)
};
struct GridPlan {
    uint32_t table_size = 0;  // buckets: a power of two, >= 2 per body slot
    GridShape shape;
};
inline uint32_t table_bits_for(uint64_t n) {
    uint32_t bits = 9;  // 512 buckets = 8 bricks at least
    while ((1ull << bits) < 2 * n && bits < 27) ++bits;
    return bits;
}
// Table size (>= 2 buckets per body slot, ghosts included, a power of two) and its split over the axes, from the OWNED bodies
// as uploaded: every axis starts with 2 bits (one brick of 4 cells) and the rest go, one at a time, to the axis with the most
// cells per bucket row - cells estimated as extent of the body centres / the largest bounding diameter. Any split is
// correct (cells wrap modulo the axis size); a good one keeps far-apart cells out of the same bucket. Bodies move, the
// split stays: a pile that compresses or spreads by a factor of two costs one bit of accuracy, not correctness.
inline GridPlan grid_plan(uint64_t n_total, uint64_t n_owned, const float* pos, const float* half_extent, float contact_margin) {
    const uint64_t n = n_owned;
    const uint32_t bits = table_bits_for(n_total);
    GridPlan out;
    out.table_size = 1u << bits;
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f}, diam = 0.0f;
    for (uint64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], pos[3 * i + a]); hi[a] = std::max(hi[a], pos[3 * i + a]); }
        if (half_extent) {
            const float* h = half_extent + 3 * i;
            diam = std::max(diam, 2.0f * std::max(h[0], std::max(h[1], h[2])));
        }
    }
    const float cell = (diam > 0.0f ? diam : 1.0f) * 1.05f + 2.0f * contact_margin;
    double cells[3];
    for (int a = 0; a < 3; ++a) cells[a] = n ? std::max(1.0, (double)(hi[a] - lo[a]) / cell + 1.0) : 1.0;
    uint32_t ab[3] = {2, 2, 2};
    for (uint32_t left = bits - 6; left > 0; --left) {
        int best = 0;
        double worst = -1.0;
        for (int a = 0; a < 3; ++a) {
            const double load = cells[a] / (double)(1u << ab[a]);
            if (load > worst && ab[a] < 20) { worst = load; best = a; }
        }
        ab[best] += 1;
    }
    GridShape& g = out.shape;
    g.mx = (1u << ab[0]) - 1u; g.my = (1u << ab[1]) - 1u; g.mz = (1u << ab[2]) - 1u;
    g.sx = ab[0] - 2u; g.sy = ab[1] - 2u;
    return out;
}

// ---- capacities of the collision pipeline (collision_alloc reads this and allocates) ----------------------------------------
struct CollisionSizes {
    uint64_t max_pairs = 0, max_manifolds = 0;
    bool ok = false;           // both index with 32 bits (<= 0xFFFFFFF0)
    uint64_t ctab_slots = 0;   // colour table: a power of two >= 1.5 * max_manifolds (PHYS_DEBUG_CTAB_SLOTS: a smaller one)
    bool warm = false;         // warm starting: not PHYS_FLAG_NO_WARM_START, and the table's value word holds the manifold index (26 bits)
    bool flow_buffers = false; // the dataflow solver's granules may exist: it addresses row_acc / flow_vel through 32-bit buffer offsets
    // the block zeroed by one memset per step: [bucket counts | colouring state | StepCounters]
    size_t bucket_bytes = 0, color_bytes = 0, counter_bytes = sizeof(StepCounters);
};
inline CollisionSizes collision_sizes(const phys_config& cfg, uint64_t n_total, const DebugSwitches& dbg) {
    CollisionSizes s;
    const uint64_t n = n_total;
    s.max_pairs = cfg.max_pairs ? cfg.max_pairs : std::max<uint64_t>(24 * n, 4096);
    s.max_manifolds = cfg.max_manifolds ? cfg.max_manifolds : std::max<uint64_t>(17 * n, 4096);
    s.ok = !(s.max_pairs > 0xFFFFFFF0ull || s.max_manifolds > 0xFFFFFFF0ull);
    const size_t T = (size_t)1 << table_bits_for(n);  // grid_plan's table
    const bool contacts = !(cfg.flags & PHYS_FLAG_BROADPHASE_ONLY);
    s.bucket_bytes = (T * 4 + 255) / 256 * 256;
    s.color_bytes = contacts ? ((size_t)4 * n * 8 + 255) / 256 * 256 : 0;
    if (!contacts) return s;
    const uint64_t M = s.max_manifolds;
    s.warm = !(cfg.flags & PHYS_FLAG_NO_WARM_START) && M < (1ull << 26);
    uint64_t cap = 4096;
    while (cap < M + M / 2) cap <<= 1;
    // PHYS_DEBUG_CTAB_SLOTS=<power of two>: a smaller table (tests of the bounded walks: crowded and overfull tables)
    if (dbg.ctab_slots >= 64 && (dbg.ctab_slots & (dbg.ctab_slots - 1)) == 0) cap = dbg.ctab_slots;
    s.ctab_slots = cap;
    s.flow_buffers = !(cfg.flags & PHYS_FLAG_SOLVER_PER_COLOR) && 64 * M < 0xFFFFFFFFull && 32 * n < 0xFFFFFFFFull;
    return s;
}

// ---- cluster solver: how many workgroups, how many bodies each (cluster.hip) ---------------------------------------------
constexpr uint32_t kClusterDynamicPeriod = 8;  // cluster steps between two deals of the dynamic homes (a body that became active
                                               // since has none and is served as another cluster's body: slower, never wrong)
constexpr uint32_t kClusterMaxSlots = 2496;    // bodies per cluster whose {v, w, x, I^-1} fit one CU's LDS (64 B each: 156 KiB; 13-bit slot field)
// occupancy asked for: three workgroups per CU (3 waves per SIMD, <= 168 VGPRs; at 128 the kernel spills 2) with diagonal
// tensors, two otherwise. Measured on C5, same bits: 1 per CU 3.48 ms, 2 per CU 2.70, 3 per CU 2.20
constexpr int kClusterPerCuDiag = 3, kClusterPerCuFull = 2;
constexpr size_t kClusterLdsPerCu = 160 * 1024;
constexpr uint32_t kClusterSlotBytes = 64;  // LDS per body slot: {v, tag} {w, 1/m} {x, -} {inverse inertia diagonal, -}
inline size_t cluster_lds_bytes(uint32_t slots) { return (size_t)slots * kClusterSlotBytes + (PHYS_MAX_COLORS + 1) * 4 + 12; }
// workgroups of a cluster grid of per_cu per CU, an eighth of the chip spared (at least 8)
inline uint32_t clusters_on_chip(int per_cu, int cus) { return (uint32_t)std::max(8, per_cu * (cus - cus / 8)); }
// the workgroups per CU to try first: as many as the kernel's occupancy bound admits; PHYS_DEBUG_CLUSTERS_PER_CU asks for fewer
inline int cluster_per_cu_max(bool all_diag_inertia) { return all_diag_inertia ? kClusterPerCuDiag : kClusterPerCuFull; }
inline int cluster_per_cu_first(int per_cu_max, const DebugSwitches& dbg) {
    return dbg.clusters_per_cu ? std::min(per_cu_max, std::max(1, *dbg.clusters_per_cu)) : per_cu_max;
}

// One workgroup per cluster, several per CU, and EVERY workgroup must be resident: the LDS of a CU must hold all of its
// workgroups' bodies (64 B per slot + the segment table, in 1 KiB allocation units) - fewer, larger clusters per CU, from
// per_cu_first down, until it does. ok = false: not even one workgroup per CU holds them (per_cu is 1 then, and slots is
// what would have been needed). The two callers differ in the floor of `slots`, which is the argument min_slots: the static
// deal (cluster_assign) rounds up to 64 with no floor (0), the dynamic one floors at 64. What a caller does with !ok - the
// dynamic plan's fallback to kClusterMaxSlots / 64 * 64 - stays with the caller.
struct ClusterFit {
    int per_cu = 0;
    uint32_t clusters = 0, slots = 0;  // clusters_on_chip(per_cu), bodies per cluster (a multiple of 64)
    bool ok = false;
};
inline ClusterFit cluster_fit(uint64_t want_bodies, int per_cu_first, int cus, uint32_t min_slots) {
    ClusterFit f;
    for (f.per_cu = per_cu_first;; --f.per_cu) {
        f.clusters = clusters_on_chip(f.per_cu, cus);
        f.slots = (uint32_t)((want_bodies + f.clusters - 1) / f.clusters);
        f.slots = std::max(min_slots, (f.slots + 63u) / 64u * 64u);
        const size_t per_wg = (cluster_lds_bytes(f.slots) + 1023) / 1024 * 1024;
        f.ok = per_wg * (size_t)f.per_cu <= kClusterLdsPerCu && f.slots <= kClusterMaxSlots;
        if (f.ok || f.per_cu <= 1) return f;
    }
}

// Static clusters: the homes of the owned bodies in isotropic Morton order over their bounding box, `slots` to a cluster.
// Ghost slots (sharded worlds) get no home in any cluster: a row never has one as body A, as body B it is 'another cluster's
// body' for everybody (slot ~0 maps to a cluster nobody runs), and no workgroup is spent on clusters that own no rows.
struct ClusterHomes {
    uint32_t clusters = 0;
    std::vector<uint32_t> cluster_slot;  // n_total: body -> cluster * slots + slot (0xFFFFFFFF: none)
    std::vector<uint32_t> cluster_body;  // clusters * slots: -> body (0xFFFFFFFF: empty)
};
inline uint32_t spread10(uint32_t x) {
    x &= 0x3ffu;
    x = (x ^ (x << 16)) & 0xff0000ffu;
    x = (x ^ (x << 8)) & 0x0300f00fu;
    x = (x ^ (x << 4)) & 0x030c30c3u;
    x = (x ^ (x << 2)) & 0x09249249u;
    return x;
}
inline ClusterHomes cluster_homes(uint64_t n_total, uint64_t n_owned, const float* pos, uint32_t slots) {
    ClusterHomes out;
    out.clusters = (uint32_t)((n_owned + slots - 1) / slots);
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    for (uint64_t i = 0; i < n_owned; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], pos[3 * i + a]); hi[a] = std::max(hi[a], pos[3 * i + a]); }
    const float span = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), std::max(hi[2] - lo[2], 1e-6f));
    const float scale = 1023.0f / span;
    std::vector<uint64_t> keyed(n_owned);
    for (uint64_t i = 0; i < n_owned; ++i) {
        uint32_t q[3];
        for (int a = 0; a < 3; ++a) {
            const float t = (pos[3 * i + a] - lo[a]) * scale;
            q[a] = t <= 0.0f ? 0u : (t >= 1023.0f ? 1023u : (uint32_t)t);
        }
        const uint64_t key = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
        keyed[i] = (key << 32) | i;
    }
    std::sort(keyed.begin(), keyed.end());
    out.cluster_slot.assign(n_total, 0xFFFFFFFFu);
    out.cluster_body.assign((size_t)out.clusters * slots, 0xFFFFFFFFu);
    for (uint64_t r = 0; r < n_owned; ++r) {
        const uint32_t i = (uint32_t)keyed[r];
        out.cluster_slot[i] = (uint32_t)r;  // = cluster * slots + slot
        out.cluster_body[r] = i;
    }
    return out;
}

// Dynamic clusters (the owned bodies do not fit the chip's LDS): clusters / slots of the next deal of homes, from the lagged
// count of bodies that have manifolds. A decision of an update like plan.hpp's, made only when the homes are dealt out again
// (cluster.hip cluster_plan_dynamic keeps that state). nullopt: no cluster step in this update.
struct ClusterShape { uint32_t clusters = 0, slots = 0; };
inline std::optional<ClusterShape> plan_dynamic_clusters(uint64_t n_owned, bool all_diag_inertia, int cus, const StepHint& h,
                                                         const DebugSwitches& dbg) {
    // the count of the last deal; before the first one: a pile has about as many bodies in contact as it has manifolds
    // (between half as many and twice as many; a world seeded with a mid-fall state - 1M cubes, 360k manifolds, 250k
    // active bodies - never got a first deal with the upper bound). Too low a guess leaves some bodies without a home for
    // one period (slower, never wrong), and the deal itself then counts them.
    uint64_t active = h.n_active;
    if (active == 0) active = std::min<uint64_t>(n_owned, (uint64_t)h.n_manifolds);
    if (active == 0) return std::nullopt;
    const int per_cu_max = cluster_per_cu_max(all_diag_inertia);
    // homes for a quarter more bodies than the last known count; what does not get one is served as "another cluster's
    // body" (slower, never wrong), so this is a matter of speed only
    uint64_t want = active + active / 4;
    if (dbg.cluster_cap && want > dbg.cluster_cap) want = dbg.cluster_cap;
    const ClusterFit f = cluster_fit(want, cluster_per_cu_first(per_cu_max, dbg), cus, 64u);
    // Only while the homes fit with the FULL number of workgroups per CU. Measured on the growing 1M-cube pile: the
    // moment the plan has to go to two or one larger workgroups per CU the per-colour launches are faster (2.10
    // against 2.33 ms at 430k active bodies, 2.66 against 3.30 at 500k; with half the bodies homeless 3.61 against
    // 4.08) - fewer workgroups hide less of each other's colour steps. (A capacity set for tests is obeyed.)
    if ((!f.ok || f.per_cu < per_cu_max) && !dbg.cluster_cap && !dbg.clusters_per_cu) return std::nullopt;
    // (PHYS_DEBUG_CLUSTERS_PER_CU asks for fewer, larger workgroups - never for homes that do not fit: with the
    // switch set, the growing 1M-cube pile once ran one 160 KiB workgroup per CU with half its bodies homeless and
    // ended in the hand-off time-out)
    if (!f.ok && !dbg.cluster_cap) return std::nullopt;
    ClusterShape s;
    s.clusters = f.clusters;
    s.slots = f.ok ? f.slots : kClusterMaxSlots / 64u * 64u;  // !ok: one workgroup per CU, as many homes as its LDS holds
    return s;
}

// ---- static colliders: records and grid (static.hip has the layout's story) ------------------------------------------------
constexpr uint32_t kStMaxDim = 1024;    // cells per axis: three 10-bit cell coordinates pack into one word
constexpr uint32_t kStLargeCells = 64;  // a static covering more cells than this is tested by every body instead

// cell of coordinate x along one axis, clamped to [0, dim - 1] (NaN: cell 0). Host and device run these operations
// alike (no contraction: -ffp-contract=off), and the result is monotone in x.
PHYS_HD uint32_t st_cell(float x, float org, float inv, uint32_t dim) {
    float t = floorf((x - org) * inv);
    if (!(t >= 0.0f)) t = 0.0f;
    const float top = (float)(dim - 1u);
    t = t > top ? top : t;
    return (uint32_t)t;
}

struct StaticSet {
    std::vector<float> geo;     // 16 floats per static, the layout of the bodies' `geo`: {pos, shape} {rot} {half extent, -}
    std::vector<float> rc;      // 12 floats per static, the ray-cast record {pos, shape} {rot} {half extent, id}
    std::vector<float> box;     // 8 floats per static: {fattened AABB lo, packed first grid cell} {hi, -}
    std::vector<uint32_t> cell_start, cell_ids;  // uniform grid over the small statics, CSR: cell -> ascending ids
    std::vector<uint32_t> large;                 // statics that would cover too many cells, ascending (one unused word when none)
    uint32_t n_large = 0;
    float org[3] = {0.0f, 0.0f, 0.0f}, inv_cell = 0.0f;
    uint32_t dim[3] = {0, 0, 0};  // cells per axis (0: no small statics), each <= kStMaxDim
    bool capsules = false;        // some static is a PHYS_SHAPE_CAPSULE
    std::vector<uint32_t> filt;   // 2 words per static: the default collision filter
    std::vector<float> mat;       // 2 floats per static: the default material {default_friction, 0}
};
// rot null: identity
inline quat quat_at(const float* rot, uint64_t k) {
    quat q;
    if (rot) { q.i = rot[4 * k]; q.j = rot[4 * k + 1]; q.k = rot[4 * k + 2]; q.w = rot[4 * k + 3]; }
    else { q.i = 0.0f; q.j = 0.0f; q.k = 0.0f; q.w = 1.0f; }
    return q;
}
// n > 0 statics (arguments checked by shape_set_error); rot null: identity
inline StaticSet build_static_set(uint64_t n, const float* pos, const float* rot, const uint32_t* shape, const float* he, float margin,
                                  float default_friction) {
    StaticSet out;
    std::vector<float>&geo = out.geo, &rc = out.rc, &box = out.box;
    geo.assign(16 * n, 0.0f); rc.assign(12 * n, 0.0f); box.assign(8 * n, 0.0f);
    std::vector<float> lo(3 * n), hi(3 * n), edge(n);
    for (uint64_t k = 0; k < n; ++k) {
        const quat q = quat_at(rot, k);
        const v3 c = v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
        const v3 h = v3_make(he[3 * k], he[3 * k + 1], he[3 * k + 2]);
        const uint32_t id = PHYS_STATIC_ID_BIT | (uint32_t)k;
        const float g[16] = {c.x, c.y, c.z, 0.0f, q.i, q.j, q.k, q.w, h.x, h.y, h.z, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        std::memcpy(&geo[16 * k], g, sizeof(g));
        std::memcpy(&geo[16 * k + 3], &shape[k], 4);
        std::memcpy(&rc[12 * k], g, 48);
        std::memcpy(&rc[12 * k + 3], &shape[k], 4);
        std::memcpy(&rc[12 * k + 11], &id, 4);
        if (shape[k] == PHYS_SHAPE_CAPSULE) out.capsules = true;
        // fattened by the contact margin like the bodies' boxes (a capsule's from its segment and radius, collide.h): a pair
        // is a candidate wherever body-body pairs would be
        const aabb_t b = body_aabb(c, q, h, shape[k], margin);
        lo[3 * k] = b.lo.x; lo[3 * k + 1] = b.lo.y; lo[3 * k + 2] = b.lo.z;
        hi[3 * k] = b.hi.x; hi[3 * k + 1] = b.hi.y; hi[3 * k + 2] = b.hi.z;
        edge[k] = std::max(b.hi.x - b.lo.x, std::max(b.hi.y - b.lo.y, b.hi.z - b.lo.z));
    }
    // cell edge: the median extent (a few huge statics do not coarsen the grid; they go to the large list)
    std::vector<float> sorted_edge(edge);
    std::nth_element(sorted_edge.begin(), sorted_edge.begin() + n / 2, sorted_edge.end());
    double cell = sorted_edge[n / 2];
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    auto covered = [&](uint64_t k, double cl) {  // cells of static k at edge cl (an upper bound: two partial cells per axis)
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) cells *= std::floor((double)(hi[3 * k + a] - lo[3 * k + a]) / cl) + 2.0;
        return cells;
    };
    std::vector<uint8_t> is_large(n, 0);
    std::vector<uint32_t>& large = out.large;
    double blo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bhi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    uint64_t n_small = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (covered(k, cell) > (double)kStLargeCells) { is_large[k] = 1; large.push_back((uint32_t)k); continue; }
        ++n_small;
        for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], (double)lo[3 * k + a]); bhi[a] = std::max(bhi[a], (double)hi[3 * k + a]); }
    }
    out.n_large = (uint32_t)large.size();
    std::vector<uint32_t>&cell_start = out.cell_start, &cell_ids = out.cell_ids;
    cell_start.assign(2, 0);
    uint32_t* dim = out.dim;
    float* org = out.org;
    float inv = 0.0f;
    if (n_small) {
        // at most kStMaxDim cells per axis and a few cells per small static in all: far-flung statics coarsen the grid
        const double max_cells = std::max<double>(4096.0, 8.0 * (double)n_small);
        for (int guard = 0; guard < 200; ++guard) {
            double total = 1.0;
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                const double d = std::floor((bhi[a] - blo[a]) / cell) + 1.0;
                if (d > (double)kStMaxDim) fits = false;
                total *= d;
            }
            if (fits && total <= max_cells) break;
            cell *= 1.25;
        }
        inv = (float)(1.0 / cell);
        for (int a = 0; a < 3; ++a) {
            org[a] = (float)blo[a];
            // the span at the float cell edge, +1 for rounding; clamped by st_cell anyway
            dim[a] = (uint32_t)std::min<double>(kStMaxDim, std::floor((bhi[a] - blo[a]) * (double)inv) + 2.0);
        }
        const uint64_t cells = (uint64_t)dim[0] * dim[1] * dim[2];
        std::vector<uint32_t> cnt(cells + 1, 0), range(6 * n, 0);
        for (uint64_t k = 0; k < n; ++k) {
            if (is_large[k]) continue;
            uint32_t* r = &range[6 * k];
            for (int a = 0; a < 3; ++a) {
                r[a] = st_cell(lo[3 * k + a], org[a], inv, dim[a]);
                r[3 + a] = st_cell(hi[3 * k + a], org[a], inv, dim[a]);
            }
            const uint32_t p = r[0] | (r[1] << 10) | (r[2] << 20);
            std::memcpy(&box[8 * k + 3], &p, 4);
            for (uint32_t z = r[2]; z <= r[5]; ++z)
                for (uint32_t y = r[1]; y <= r[4]; ++y)
                    for (uint32_t x = r[0]; x <= r[3]; ++x) cnt[(z * dim[1] + y) * dim[0] + x]++;
        }
        cell_start.assign(cells + 1, 0);
        for (uint64_t c = 0; c < cells; ++c) cell_start[c + 1] = cell_start[c] + cnt[c];
        cell_ids.assign(cell_start[cells] ? cell_start[cells] : 1, 0);
        std::vector<uint32_t> cur(cell_start.begin(), cell_start.end() - 1);
        for (uint64_t k = 0; k < n; ++k) {  // ascending k: every cell's list is ascending
            if (is_large[k]) continue;
            const uint32_t* r = &range[6 * k];
            for (uint32_t z = r[2]; z <= r[5]; ++z)
                for (uint32_t y = r[1]; y <= r[4]; ++y)
                    for (uint32_t x = r[0]; x <= r[3]; ++x) cell_ids[cur[(z * dim[1] + y) * dim[0] + x]++] = (uint32_t)k;
        }
    }
    out.inv_cell = inv;
    for (uint64_t k = 0; k < n; ++k) {
        box[8 * k] = lo[3 * k]; box[8 * k + 1] = lo[3 * k + 1]; box[8 * k + 2] = lo[3 * k + 2];
        box[8 * k + 4] = hi[3 * k]; box[8 * k + 5] = hi[3 * k + 1]; box[8 * k + 6] = hi[3 * k + 2];
    }
    if (cell_ids.empty()) cell_ids.assign(1, 0);
    if (large.empty()) large.assign(1, 0);  // (never read: n_large is 0)
    // every static starts with the default collision filter (phys_set_static_filters changes them) ...
    out.filt.resize(2 * n);
    for (uint64_t k = 0; k < n; ++k) { out.filt[2 * k] = kFilterDefaultWord; out.filt[2 * k + 1] = 0u; }
    // ... and the default material {default_friction, 0} (phys_set_static_materials)
    out.mat.assign(2 * n, 0.0f);
    for (uint64_t k = 0; k < n; ++k) out.mat[2 * k] = default_friction;
    return out;
}

// ---- bodies: the staged arrays of phys_set_bodies ---------------------------------------------------------------------------
struct BodyStaging {
    std::vector<float> pos, rot, vel /* 8 per slot: v.xyz inv_mass w.xyz mass */, inv_inertia, inv_inertia_diag /* 4 per slot */, half_extent;
    std::vector<uint32_t> shape, global_id, filt;
    std::vector<float> mat;
    bool singular_inertia = false;  // some body's inertia tensor has det == 0 (reference panics in step)
    bool all_diag_inertia = true;
    bool uniform_inertia = true;    // all diagonal AND identical for every body slot
    bool body_capsules = false;
};
// RigidBody::new defaults (rigid_body.rs:64-76) for every null array; ghost slots behind the owned bodies: no shape, immovable
inline BodyStaging stage_bodies(uint64_t n, uint64_t n_ghost_slots, const float* pos, const float* rot, const float* lin, const float* ang,
                                const float* mass, const float* inertia, const uint32_t* shape_type, const float* half_extent,
                                float default_friction) {
    const uint64_t nt = n + n_ghost_slots;
    BodyStaging s;
    std::vector<float>&h_pos = s.pos, &h_rot = s.rot, &h_vel = s.vel, &h_inv = s.inv_inertia, &h_diag = s.inv_inertia_diag, &h_he = s.half_extent;
    h_pos.assign(3 * nt, 0.0f); h_rot.resize(4 * nt); h_vel.resize(8 * nt); h_inv.assign(9 * nt, 0.0f); h_diag.assign(4 * nt, 0.0f);
    h_he.assign(3 * nt, 0.0f);
    std::vector<uint32_t>&h_shape = s.shape, &h_gid = s.global_id, &h_filt = s.filt;
    h_shape.assign(nt, PHYS_SHAPE_NONE); h_gid.assign(nt, 0xFFFFFFFFu); h_filt.assign(2 * nt, 0u);
    for (uint64_t i = 0; i < nt; ++i) h_filt[2 * i] = kFilterDefaultWord;
    s.mat.assign(2 * nt, 0.0f);
    for (uint64_t i = 0; i < nt; ++i) s.mat[2 * i] = default_friction;
    std::memcpy(h_pos.data(), pos, 12 * n);
    for (uint64_t i = 0; i < n; ++i) {
        if (rot) std::memcpy(&h_rot[4 * i], rot + 4 * i, 16);
        else { h_rot[4 * i] = 0.0f; h_rot[4 * i + 1] = 0.0f; h_rot[4 * i + 2] = 0.0f; h_rot[4 * i + 3] = 1.0f; }
        const float m_i = mass ? mass[i] : 1.0f;
        for (int k = 0; k < 3; ++k) { h_vel[8 * i + k] = lin ? lin[3 * i + k] : 0.0f; h_vel[8 * i + 4 + k] = ang ? ang[3 * i + k] : 0.0f; }
        h_vel[8 * i + 3] = 1.0f / m_i;  // constraints.rs:75
        h_vel[8 * i + 7] = m_i;
        m33 I, inv;
        for (int k = 0; k < 9; ++k) I.m[k] = inertia ? inertia[9 * i + k] : ((k % 4 == 0) ? 1.0f : 0.0f);
        // The reference inverts the (constant, world-frame) tensor every step (rigid_body.rs:31, quirk Q5);
        // inverting once gives the same bits.
        if (!m33_try_inverse(&I, &inv)) {
            s.singular_inertia = true;
            for (int k = 0; k < 9; ++k) inv.m[k] = 0.0f;
        }
        for (int k = 0; k < 9; ++k) {
            h_inv[9 * i + k] = inv.m[k];
            if (k % 4 != 0 && inv.m[k] != 0.0f) s.all_diag_inertia = false;
        }
        h_diag[4 * i] = inv.m[0]; h_diag[4 * i + 1] = inv.m[4]; h_diag[4 * i + 2] = inv.m[8];
        if (h_diag[4 * i] != h_diag[0] || h_diag[4 * i + 1] != h_diag[1] || h_diag[4 * i + 2] != h_diag[2]) s.uniform_inertia = false;
        if (shape_type) h_shape[i] = shape_type[i];
        if (h_shape[i] == PHYS_SHAPE_CAPSULE) s.body_capsules = true;
        if (half_extent) std::memcpy(&h_he[3 * i], half_extent + 3 * i, 12);
        h_gid[i] = (uint32_t)i;
    }
    for (uint64_t i = n; i < nt; ++i) {  // ghost slots: identity pose, inverse mass 0, mass +inf (F / m = 0), inverse inertia 0
        h_rot[4 * i + 3] = 1.0f;
        h_vel[8 * i + 3] = 0.0f;
        h_vel[8 * i + 7] = std::numeric_limits<float>::infinity();
    }
    if (nt > n) s.uniform_inertia = false;  // the ghosts' zero tensors differ from everybody's
    if (!s.all_diag_inertia) s.uniform_inertia = false;
    return s;
}

// ---- constraints: the column tables of the constraint solve (constraints.hip) -----------------------------------------------
// distinct selected columns (6 * body + 3 * kind + axis, ascending), each with its selecting rows in constraint order
struct ConstraintColumns {
    std::vector<uint32_t> col_id, col_ptr /* columns + 1 */, col_rows /* 3 per constraint */, row_cidx /* row -> index into col_id */;
};
inline ConstraintColumns constraint_columns(const std::vector<Constraint>& constraints) {
    const size_t C = constraints.size();
    const size_t n = 3 * C;
    std::vector<std::pair<uint32_t, uint32_t>> sorted(n);  // (column, row)
    for (size_t c = 0; c < C; ++c)
        for (uint32_t k = 0; k < 3; ++k) sorted[3 * c + k] = {6u * constraints[c].body + 3u * constraints[c].kind + k, (uint32_t)(3 * c + k)};
    std::stable_sort(sorted.begin(), sorted.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    ConstraintColumns out;
    out.col_rows.resize(n); out.row_cidx.resize(n);
    for (size_t k = 0; k < n; ++k) {
        if (k == 0 || sorted[k].first != sorted[k - 1].first) { out.col_id.push_back(sorted[k].first); out.col_ptr.push_back((uint32_t)k); }
        out.col_rows[k] = sorted[k].second;
        out.row_cidx[sorted[k].second] = (uint32_t)out.col_id.size() - 1;
    }
    out.col_ptr.push_back((uint32_t)n);
    return out;
}

// ---- argument checks and packing of the set calls -----------------------------------------------------------------------
// The shapes and poses of phys_set_static_bodies ("static collider") and phys_set_triggers ("trigger"): null when every item
// is a SPHERE, BOX or CAPSULE with a finite pose and a finite, non-negative half extent; else the message for the FIRST
// offending item (held by msg) - its shape first, then non-finite, then negative. rot null: not checked.
inline const char* shape_set_error(const char* kind_name, uint64_t n, const uint32_t* shape, const float* pos, const float* rot, const float* he,
                                   std::string& msg) {
    for (uint64_t k = 0; k < n; ++k) {
        const char* what = nullptr;
        if (shape[k] != PHYS_SHAPE_SPHERE && shape[k] != PHYS_SHAPE_BOX && shape[k] != PHYS_SHAPE_CAPSULE) {
            what = ": shape is neither SPHERE nor BOX nor CAPSULE";
        } else {
            bool finite = true, negative = false;
            for (int a = 0; a < 3; ++a) {
                finite = finite && std::isfinite(pos[3 * k + a]) && std::isfinite(he[3 * k + a]);
                negative = negative || he[3 * k + a] < 0.0f;
            }
            if (rot)
                for (int a = 0; a < 4; ++a) finite = finite && std::isfinite(rot[4 * k + a]);
            if (!finite) what = ": non-finite pose or half extent";
            else if (negative) what = ": negative half extent";
        }
        if (what) {
            msg = std::string(kind_name) + " " + std::to_string(k) + what;
            return msg.c_str();
        }
    }
    return nullptr;
}

// collision filters: {category | mask << 16, (u32)group} per item; a NULL array gives that field its default
inline void pack_filters(uint64_t n, const uint16_t* category, const uint16_t* mask, const int16_t* group, std::vector<uint32_t>& out) {
    out.resize(2 * n);
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t c = category ? category[k] : PHYS_FILTER_DEFAULT_CATEGORY;
        const uint32_t m = mask ? mask[k] : PHYS_FILTER_DEFAULT_MASK;
        out[2 * k] = c | (m << 16);
        out[2 * k + 1] = group ? (uint32_t)(int32_t)group[k] : 0u;
    }
}
// materials: {friction, restitution} per item; a NULL array gives that field its default. false: a value out of range
inline bool pack_materials(uint64_t n, const float* friction, const float* restitution, float default_friction, std::vector<float>& out) {
    out.resize(2 * n);
    for (uint64_t k = 0; k < n; ++k) {
        const float f = friction ? friction[k] : default_friction, e = restitution ? restitution[k] : 0.0f;
        if (!std::isfinite(f) || f < 0.0f || !(e >= 0.0f && e <= 1.0f)) return false;
        out[2 * k] = f; out[2 * k + 1] = e;
    }
    return true;
}

// ---- force fields: the checks and the staged form of phys_set_force_fields and its two updates --------
// null when every field has a known kind, a SPHERE, BOX or CAPSULE volume, finite numbers, a non-negative half extent, and
// coefficients its law admits; else the message for the FIRST offending field (held by msg): its kind first, then its shape,
// then non-finite, then a negative half extent, then the law. rot / exponent null: not checked (identity / 0).
inline const char* field_law_error(uint32_t kind, const float* coef2, uint32_t exponent) {
    if (kind == PHYS_FIELD_DRAG && (coef2[0] < 0.0f || coef2[1] < 0.0f)) return ": negative drag coefficient";
    if (kind == PHYS_FIELD_RADIAL && !(coef2[1] > 0.0f)) return ": r0 (coef[1]) must be above 0";
    if (exponent > 2u) return ": exponent above 2";
    return nullptr;
}
inline const char* field_set_error(uint64_t n, const uint32_t* kind, const uint32_t* shape, const float* pos, const float* rot, const float* he,
                                   const float* vec, const float* coef, const uint32_t* exponent, std::string& msg) {
    for (uint64_t k = 0; k < n; ++k) {
        const char* what = nullptr;
        if (kind[k] != PHYS_FIELD_ACCEL && kind[k] != PHYS_FIELD_DRAG && kind[k] != PHYS_FIELD_RADIAL) {
            what = ": kind is neither ACCEL nor DRAG nor RADIAL";
        } else if (shape[k] != PHYS_SHAPE_SPHERE && shape[k] != PHYS_SHAPE_BOX && shape[k] != PHYS_SHAPE_CAPSULE) {
            what = ": shape is neither SPHERE nor BOX nor CAPSULE";
        } else {
            bool finite = std::isfinite(coef[2 * k]) && std::isfinite(coef[2 * k + 1]), negative = false;
            for (int a = 0; a < 3; ++a) {
                finite = finite && std::isfinite(pos[3 * k + a]) && std::isfinite(he[3 * k + a]) && std::isfinite(vec[3 * k + a]);
                negative = negative || he[3 * k + a] < 0.0f;
            }
            if (rot)
                for (int a = 0; a < 4; ++a) finite = finite && std::isfinite(rot[4 * k + a]);
            if (!finite) what = ": non-finite number";
            else if (negative) what = ": negative half extent";
            else what = field_law_error(kind[k], coef + 2 * k, exponent ? exponent[k] : 0u);
        }
        if (what) {
            msg = "force field " + std::to_string(k) + what;
            return msg.c_str();
        }
    }
    return nullptr;
}

// the new poses of n staged volumes (phys_set_force_field_poses, phys_set_trigger_poses) are finite; rot null: not looked at
inline bool poses_finite(size_t n, const float* pos, const float* rot) {
    for (size_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(pos[k])) return false;
    for (size_t k = 0; rot && k < 4 * n; ++k)
        if (!std::isfinite(rot[k])) return false;
    return true;
}

// The set as the host keeps it (include/spec/force_field.h ff_staged, 80 bytes per field) and what selects the evaluation's
// instance: a mask array was given; some field is a DRAG (the velocity record is read); some field is an ACCEL (the mass is).
struct FieldStaging {
    std::vector<ff_staged> staged;
    bool masked = false, drag = false, accel = false;
};
// n fields (arguments checked by field_set_error); rot null: identity, mask null: every body, exponent null: 0
inline FieldStaging stage_fields(uint64_t n, const uint32_t* kind, const uint32_t* shape, const float* pos, const float* rot, const float* he,
                                 const uint16_t* mask, const float* vec, const float* coef, const uint32_t* exponent) {
    FieldStaging out;
    out.staged.resize(n);
    out.masked = n != 0 && mask != nullptr;
    for (uint64_t k = 0; k < n; ++k) {
        out.staged[k] = ff_staged_make(kind[k], shape[k], mask ? (uint32_t)mask[k] : 0xFFFFu, exponent ? exponent[k] : 0u,
                                       v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]), quat_at(rot, k),
                                       v3_make(he[3 * k], he[3 * k + 1], he[3 * k + 2]), v3_make(vec[3 * k], vec[3 * k + 1], vec[3 * k + 2]),
                                       coef[2 * k], coef[2 * k + 1]);
        if (kind[k] == PHYS_FIELD_DRAG) out.drag = true;
        if (kind[k] == PHYS_FIELD_ACCEL) out.accel = true;
    }
    return out;
}
// phys_set_force_field_poses: new centres and, unless rot is null, rotations of the staged set; false: a non-finite value
// (nothing changed then)
inline bool restage_field_poses(std::vector<ff_staged>& staged, const float* pos, const float* rot) {
    if (!poses_finite(staged.size(), pos, rot)) return false;
    for (size_t k = 0; k < staged.size(); ++k) {
        staged[k].s[1] = vol_f4_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2], 0.0f);
        if (rot) staged[k].s[2] = vol_f4_make(rot[4 * k], rot[4 * k + 1], rot[4 * k + 2], rot[4 * k + 3]);
    }
    return true;
}
// phys_set_force_field_params: new vec and coef of the staged set, each held to its field's law (kind and exponent stay);
// null, or the message for the first offending field (nothing changed then)
inline const char* restage_field_params(std::vector<ff_staged>& staged, const float* vec, const float* coef, std::string& msg) {
    const size_t n = staged.size();
    for (size_t k = 0; k < n; ++k) {
        const char* what = nullptr;
        if (!(std::isfinite(vec[3 * k]) && std::isfinite(vec[3 * k + 1]) && std::isfinite(vec[3 * k + 2]) && std::isfinite(coef[2 * k]) &&
              std::isfinite(coef[2 * k + 1])))
            what = ": non-finite number";
        else what = field_law_error(ff_f2u(staged[k].s[0].x), coef + 2 * k, ff_f2u(staged[k].s[0].w));
        if (what) {
            msg = "force field " + std::to_string(k) + what;
            return msg.c_str();
        }
    }
    for (size_t k = 0; k < n; ++k) {
        staged[k].s[3].w = coef[2 * k];
        staged[k].s[4] = vol_f4_make(vec[3 * k], vec[3 * k + 1], vec[3 * k + 2], coef[2 * k + 1]);
    }
    return nullptr;
}

// ---- liquids: the checks and the staged form of phys_set_liquids and its two updates ------------------
// null when every number is finite, no half extent negative, no density negative and no drag negative; else the message for
// the FIRST offending liquid (held by msg), its reasons in that order. rot null: not checked (identity).
inline bool liquid_params_finite(const float* density, const float* gravity, const float* flow, const float* drag, uint64_t k) {
    bool finite = std::isfinite(density[k]) && std::isfinite(drag[2 * k]) && std::isfinite(drag[2 * k + 1]);
    for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(gravity[3 * k + a]) && std::isfinite(flow[3 * k + a]);
    return finite;
}
inline const char* liquid_params_negative(const float* density, const float* drag, uint64_t k) {
    if (density[k] < 0.0f) return ": negative density";
    if (drag[2 * k] < 0.0f || drag[2 * k + 1] < 0.0f) return ": negative drag coefficient";
    return nullptr;
}
inline const char* liquid_set_error(uint64_t n, const float* pos, const float* rot, const float* he, const float* density, const float* gravity,
                                    const float* flow, const float* drag, std::string& msg) {
    for (uint64_t k = 0; k < n; ++k) {
        bool finite = true, negative = false;
        for (int a = 0; a < 3; ++a) {
            finite = finite && std::isfinite(pos[3 * k + a]) && std::isfinite(he[3 * k + a]);
            negative = negative || he[3 * k + a] < 0.0f;
        }
        if (rot)
            for (int a = 0; a < 4; ++a) finite = finite && std::isfinite(rot[4 * k + a]);
        const char* what = nullptr;
        if (!finite || !liquid_params_finite(density, gravity, flow, drag, k)) what = ": non-finite number";
        else if (negative) what = ": negative half extent";
        else what = liquid_params_negative(density, drag, k);
        if (what) {
            msg = "liquid " + std::to_string(k) + what;
            return msg.c_str();
        }
    }
    return nullptr;
}
// The set as the host keeps it (include/spec/liquid.h lq_staged, 96 bytes per liquid) and what selects the evaluation's
// instance: a mask array was given; some liquid has a nonzero drag (the velocity record is read).
struct LiquidStaging {
    std::vector<lq_staged> staged;
    bool masked = false, drag = false;
};
inline bool liquids_have_drag(const std::vector<lq_staged>& staged) {
    for (const lq_staged& s : staged)
        if (s.s[4].w != 0.0f || s.s[5].w != 0.0f) return true;
    return false;
}
// n liquids (arguments checked by liquid_set_error); rot null: identity, mask null: every body
inline LiquidStaging stage_liquids(uint64_t n, const float* pos, const float* rot, const float* he, const uint16_t* mask, const float* density,
                                   const float* gravity, const float* flow, const float* drag) {
    LiquidStaging out;
    out.staged.resize(n);
    out.masked = n != 0 && mask != nullptr;
    for (uint64_t k = 0; k < n; ++k)
        out.staged[k] = lq_staged_make(mask ? (uint32_t)mask[k] : 0xFFFFu, v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]), quat_at(rot, k),
                                       v3_make(he[3 * k], he[3 * k + 1], he[3 * k + 2]), density[k],
                                       v3_make(gravity[3 * k], gravity[3 * k + 1], gravity[3 * k + 2]),
                                       v3_make(flow[3 * k], flow[3 * k + 1], flow[3 * k + 2]), drag[2 * k], drag[2 * k + 1]);
    out.drag = liquids_have_drag(out.staged);
    return out;
}
// phys_set_liquid_poses: new centres and, unless rot is null, rotations of the staged set; false: a non-finite value
// (nothing changed then)
inline bool restage_liquid_poses(std::vector<lq_staged>& staged, const float* pos, const float* rot) {
    if (!poses_finite(staged.size(), pos, rot)) return false;
    for (size_t k = 0; k < staged.size(); ++k) {
        staged[k].s[1] = vol_f4_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2], 0.0f);
        if (rot) staged[k].s[2] = vol_f4_make(rot[4 * k], rot[4 * k + 1], rot[4 * k + 2], rot[4 * k + 3]);
    }
    return true;
}
// phys_set_liquid_params: new density, gravity, flow and drag of the staged set; null, or the message for the first
// offending liquid (nothing changed then)
inline const char* restage_liquid_params(std::vector<lq_staged>& staged, const float* density, const float* gravity, const float* flow,
                                         const float* drag, std::string& msg) {
    const size_t n = staged.size();
    for (size_t k = 0; k < n; ++k) {
        const char* what = liquid_params_finite(density, gravity, flow, drag, k) ? liquid_params_negative(density, drag, k) : ": non-finite number";
        if (what) {
            msg = "liquid " + std::to_string(k) + what;
            return msg.c_str();
        }
    }
    for (size_t k = 0; k < n; ++k) {
        staged[k].s[0].w = density[k];
        staged[k].s[4] = vol_f4_make(flow[3 * k], flow[3 * k + 1], flow[3 * k + 2], drag[2 * k]);
        staged[k].s[5] = vol_f4_make(gravity[3 * k], gravity[3 * k + 1], gravity[3 * k + 2], drag[2 * k + 1]);
    }
    return nullptr;
}
inline std::vector<lq_record> liquid_records(const std::vector<lq_staged>& staged) {
    std::vector<lq_record> rec(staged.size());
    for (size_t k = 0; k < staged.size(); ++k) rec[k] = lq_record_make(&staged[k]);
    return rec;
}

// ---- trigger volumes: staged like the fields - the set as the host keeps it, its poses, its records ---
struct TriggerVolume { uint32_t shape, mask; v3 c; quat q; v3 h; };
struct TriggerStaging { std::vector<TriggerVolume> staged; bool masked = false; /* a mask array was given: the filtered instance */ };
// n triggers (arguments checked by shape_set_error); rot null: identity, mask null: every body
inline TriggerStaging stage_triggers(uint64_t n, const uint32_t* shape, const float* pos, const float* rot, const float* he,
                                     const uint16_t* mask) {
    TriggerStaging out;
    out.staged.resize(n);
    out.masked = n != 0 && mask != nullptr;
    for (uint64_t k = 0; k < n; ++k)
        out.staged[k] = {shape[k], mask ? (uint32_t)mask[k] : 0xFFFFu, v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]), quat_at(rot, k),
                         v3_make(he[3 * k], he[3 * k + 1], he[3 * k + 2])};
    return out;
}
// phys_set_trigger_poses: as restage_field_poses
inline bool restage_trigger_poses(std::vector<TriggerVolume>& staged, const float* pos, const float* rot) {
    if (!poses_finite(staged.size(), pos, rot)) return false;
    for (size_t k = 0; k < staged.size(); ++k) {
        staged[k].c = v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
        if (rot) staged[k].q = quat_at(rot, k);
    }
    return true;
}
// the records the evaluations read (trigger.hip, fields.hip), built where the sets were checked
inline std::vector<vol_record> trigger_records(const std::vector<TriggerVolume>& staged) {
    std::vector<vol_record> rec(staged.size());
    for (size_t k = 0; k < staged.size(); ++k) rec[k] = vol_record_make(staged[k].shape, staged[k].mask, staged[k].c, staged[k].q, staged[k].h);
    return rec;
}
inline std::vector<ff_record> field_records(const std::vector<ff_staged>& staged) {
    std::vector<ff_record> rec(staged.size());
    for (size_t k = 0; k < staged.size(); ++k) rec[k] = ff_record_make(&staged[k]);
    return rec;
}

// ---- in-place body edits: the checks and the order of a batch on host arrays ----------------------------
// The four edit calls and the arrays of one batch, host pointers or device pointers alike, in the header's order:
//   Poses: pos, rot   Velocities: lin, ang   Impulses: impulse, point, ang_impulse   Forces: force, point, torque
enum class EditKind { Poses, Velocities, Impulses, Forces };
struct EditBatch {
    uint64_t n;
    const uint32_t* ids;
    const float* a[3];
};
// floats per entry of array `slot` (0: the kind has no such array); only the first array of an impulse or force batch is required
inline uint32_t edit_cols(EditKind kind, int slot) {
    if (kind == EditKind::Poses) return slot == 0 ? 3u : (slot == 1 ? 4u : 0u);
    if (kind == EditKind::Velocities) return slot < 2 ? 3u : 0u;
    return 3u;
}
inline bool edit_required(EditKind kind, int slot) { return slot == 0 && (kind == EditKind::Impulses || kind == EditKind::Forces); }
// what every edit entry point checks first, host or device arrays: the text of the refusal (PHYS_ERR_INVALID_ARG), null when
// the call may go on. n == 0 is a no-op whatever the pointers.
inline const char* edit_args_error(EditKind kind, const EditBatch& b) {
    if (b.n == 0) return nullptr;
    if (b.n >= (1ull << 31)) return "body edit: n must be below 2^31";
    if (!b.ids) return "body edit: null ids";
    for (int s = 0; s < 3; ++s)
        if (edit_required(kind, s) && !b.a[s]) return "body edit: null impulse / force array";
    return nullptr;
}
// The entries ordered by a STABLE sort on the id, so that the entries of one body keep the order the caller gave them and form
// one run (include/spec/body_edit.h). Checked before anything is written: code is PHYS_OK, or the refusal and its text - a
// null ids or a null required array with n > 0 (PHYS_ERR_INVALID_ARG), then an id that is not below n_owned
// (PHYS_ERR_OUT_OF_RANGE), then a non-finite value (PHYS_ERR_INVALID_ARG). n == 0: no entries, PHYS_OK.
struct EditOrder {
    int32_t code = PHYS_OK;
    std::string message;
    std::vector<uint32_t> order;  // order[k]: the caller's entry that is applied k-th
    std::vector<uint32_t> ids;    // ids[order[k]]: non-decreasing
};
inline EditOrder edit_order(EditKind kind, const EditBatch& b, uint64_t n_owned) {
    EditOrder out;
    const uint64_t n = b.n;
    const uint32_t* ids = b.ids;
    if (n == 0) return out;
    const auto refuse = [&](int32_t code, std::string msg) { out.code = code; out.message = std::move(msg); return out; };
    if (const char* bad = edit_args_error(kind, b)) return refuse(PHYS_ERR_INVALID_ARG, bad);
    for (uint64_t k = 0; k < n; ++k)
        if (ids[k] >= n_owned)
            return refuse(PHYS_ERR_OUT_OF_RANGE, "body edit: entry " + std::to_string(k) + " names body " + std::to_string(ids[k]) + ", out of range");
    for (int s = 0; s < 3; ++s) {
        const uint32_t cols = edit_cols(kind, s);
        for (uint64_t k = 0; b.a[s] && k < n * cols; ++k)
            if (!std::isfinite(b.a[s][k])) return refuse(PHYS_ERR_INVALID_ARG, "body edit: non-finite value in entry " + std::to_string(k / cols));
    }
    out.order.resize(n);
    for (uint64_t k = 0; k < n; ++k) out.order[k] = (uint32_t)k;
    std::stable_sort(out.order.begin(), out.order.end(), [&](uint32_t x, uint32_t y) { return ids[x] < ids[y]; });
    out.ids.resize(n);
    for (uint64_t k = 0; k < n; ++k) out.ids[k] = ids[out.order[k]];
    return out;
}
// an array of the batch in that order (`cols` values per entry); null stays null (an empty vector)
template <typename T>
inline std::vector<T> edit_gather(const std::vector<uint32_t>& order, const T* src, uint32_t cols) {
    std::vector<T> out;
    if (!src) return out;
    out.resize(order.size() * (size_t)cols);
    for (size_t k = 0; k < order.size(); ++k) std::memcpy(&out[k * cols], src + (size_t)order[k] * cols, sizeof(T) * cols);
    return out;
}

// ---- continuous collision: the list of phys_set_ccd_bodies ---------------------------------------------
// Entry k of the list is ids[k]: the given order is kept, the read-out of phys_get_ccd_hits is in it. Checked before anything is
// written: code is PHYS_OK, or the refusal and its text - null ids with n > 0 or n at or above 2^31 (PHYS_ERR_INVALID_ARG), then an
// id that is not below n_owned (PHYS_ERR_OUT_OF_RANGE, as a body edit answers), then an id given twice (PHYS_ERR_INVALID_ARG: two
// lanes would own one body's step). n == 0: an empty list, PHYS_OK.
struct CcdStaging {
    int32_t code = PHYS_OK;
    std::string message;
    std::vector<uint32_t> ids;
};
inline CcdStaging stage_ccd(uint64_t n, const uint32_t* ids, uint64_t n_owned) {
    CcdStaging out;
    if (n == 0) return out;
    const auto refuse = [&](int32_t code, std::string msg) { out.code = code; out.message = std::move(msg); out.ids.clear(); return out; };
    if (n >= (1ull << 31)) return refuse(PHYS_ERR_INVALID_ARG, "phys_set_ccd_bodies: n must be below 2^31");
    if (!ids) return refuse(PHYS_ERR_INVALID_ARG, "phys_set_ccd_bodies: null ids");
    for (uint64_t k = 0; k < n; ++k)
        if (ids[k] >= n_owned)
            return refuse(PHYS_ERR_OUT_OF_RANGE, "phys_set_ccd_bodies: entry " + std::to_string(k) + " names body " + std::to_string(ids[k]) + ", out of range");
    std::vector<uint32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) return refuse(PHYS_ERR_INVALID_ARG, "phys_set_ccd_bodies: body " + std::to_string(*twice) + " is listed twice");
    out.ids.assign(ids, ids + n);
    return out;
}

}  // namespace phys
