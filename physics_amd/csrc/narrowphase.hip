// narrowphase.hip — contact generation for gfx950. No reference counterpart; the arithmetic is
// the normative scalar spec of include/spec/collide.h. (The colouring that orders the solver: coloring.hip.)
//
// k_narrowphase: one lane per work item (ground test of a body, one candidate pair, or - worlds with static colliders - one
//   (body, static) pair of static.hip, B's shape and pose read from the static set); manifolds are
//   compacted per workgroup (wavefront ballot + popcount prefix, wave totals through LDS, ONE global
//   atomic per workgroup) and written as 100-byte records. Emission order is arbitrary. A manifold that
//   existed in the previous update keeps its colour (hash-table probe); the others publish round 0 of the colouring.
// Algorithmic bytes: per pair 8 + 2 x 44 (pos 12, rot 16, half 12, shape 4) = 96 B read;
//   per manifold 100 B written (ids 8, count 4, normal 12, points 64, priority 8, colour 4).
#include <cstdlib>
#include <utility>

#include "kernels.hpp"

namespace phys {

// one body as the narrow phase sees it: three 16-byte loads from ONE 64-byte line (world.hpp `geo`, written by
// k_step_velocity_aabb of this update from the same pose the AABBs were made of)
__device__ __forceinline__ geom_t load_geom(uint32_t i, const float* __restrict__ geo) {
    const float4* g = reinterpret_cast<const float4*>(geo) + 4 * (size_t)i;
    const float4 g0 = g[0], qq = g[1], g2 = g[2];
    quat q; q.i = qq.x; q.j = qq.y; q.k = qq.z; q.w = qq.w;
    return geom_make(v3_make(g0.x, g0.y, g0.z), q, v3_make(g2.x, g2.y, g2.z), __float_as_uint(g0.w));
}

// kNpThreads: 128 for small scenes (latency-bound: more workgroups in flight, the LDS slice of the clipper
// halves), 512 for everything else (launch_narrowphase). kCapsules: the full collide_pair / collide_ground of collide.h;
// without it only their sphere / box part is compiled (a world without capsules keeps the registers - and the resident
// waves - the kernel had before capsules: DESIGN.md section 11). kFilters: every work item is first tested against the
// collision filters of its two sides (one NpFilters argument, the pack `filt`); an item they reject
// is an item whose shapes do not touch. Without it the pack is empty and the kernel is the one it was before filters.
template <int kNpThreads, int kNpItems, bool kStatics, bool kCapsules, bool kFilters, typename... Filt>
__global__ __launch_bounds__(kNpThreads) void k_narrowphase(
    uint32_t n_ground /* bodies tested against the plane (0 = no ground) */, uint32_t n_owned /* pairs whose FIRST body is at
    or beyond this index are skipped (= all body slots: the ghosts of a sharded world collide like everybody else) */,
    const uint32_t* __restrict__ pairs,
    uint64_t max_pairs, const float* __restrict__ geo /* 16 floats per body: {pos, shape} {rot} {half extent, AABB lo.y} */,
    float margin, float ground, uint64_t max_manifolds, uint32_t* __restrict__ man_a, uint32_t* __restrict__ man_b,
    uint32_t* __restrict__ man_color, float* __restrict__ man_geo /* 32 floats per manifold */,
    uint64_t* __restrict__ man_prio, unsigned long long* __restrict__ used,
    unsigned long long* __restrict__ top0, ulonglong2* __restrict__ cache /* persistent colour table (kernels.hpp) */,
    uint32_t cache_mask /* 0 = keep nothing this update */, uint32_t early_probe /* ask for the table entry before the shapes
    are tested */, uint32_t stamp /* of this update */,
    uint32_t* __restrict__ unc_list /* ids of the manifolds that did not keep a colour: round 0 of the colouring */,
    const uint32_t* __restrict__ man_prev /* warm starting on (non-null; the index of the pair's previous manifold itself
    travels in the manifold record) */,
    float* __restrict__ man_imp /* ... and this update's impulse records, zeroed here (a solve that never runs leaves zeros) */,
    StepCounters* __restrict__ ctr,
    uint64_t max_static_pairs /* kStatics: (body, static) pairs of static.hip, the third kind of work item */,
    const uint32_t* __restrict__ static_pairs, const float* __restrict__ static_geo /* 16 floats per static, the layout of geo */,
    Filt... filt /* kFilters: one NpFilters */) {
    static_assert(sizeof...(Filt) == (kFilters ? 1u : 0u), "one NpFilters argument exactly in the filtered instance");
    NpFilters flt{};
    if constexpr (kFilters) flt = filter_arg(filt...);
    // per-wave totals of a trip, in two sets used alternately: a wave may start the next trip (and post its totals) while
    // another still reads this trip's to place its manifolds - there is no barrier at the end of a trip any more
    __shared__ uint32_t wtot[2][4][kNpThreads / 64];
    __shared__ uint32_t block_base, unc_base;
    // polygon-clipper scratch in LDS: one 32-dword slice per lane at an odd (33) dword stride, so the lanes of
    // a wave hit distinct banks; private scratch memory would go through L1/L2 instead
    constexpr int kWsStride = sizeof(clip_ws_t) / 4 + 1;
    __shared__ float ws_lds[kNpThreads * kWsStride];
    clip_ws_t* ws = reinterpret_cast<clip_ws_t*>(ws_lds + threadIdx.x * kWsStride);
    // nothing else of a lane is indexed at run time: the shapes and the manifold stay in registers, and the kernel
    // uses no scratch memory at all (a rule of this library - tests/test_build_rules.py)
    const uint32_t np_raw = ctr->n_pairs;
    const uint32_t n_pairs = (uint64_t)np_raw < max_pairs ? np_raw : (uint32_t)max_pairs;
    uint32_t n_static = 0;
    if (kStatics) {
        const uint32_t ns_raw = ctr->n_static_pairs;
        n_static = (uint64_t)ns_raw < max_static_pairs ? ns_raw : (uint32_t)max_static_pairs;
    }
    const uint32_t n_body_items = n_ground + n_pairs;
    const uint32_t total = n_body_items + n_static;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t trip = 0;
    uint32_t acc_pts = 0, acc_ground = 0, acc_unc = 0;  // thread 0: statistics of this workgroup's trips, added once at the end
    uint32_t acc_static = 0;  // kStatics, every wave: its static manifolds, added once at the end
    // A trip is a chain of dependent round trips - pair, shapes, [test], table entry, `used` masks, barrier, slot
    // reservation, barrier, stores - that the 12 waves a CU's LDS admits cannot hide from each other. A lane therefore
    // tests kNpItems work items per trip, one after the other, and everything behind the test - the ballots, the two
    // barriers, the workgroup's ONE reservation - is made once for all of them.
    struct Item {
        manifold_t m;
        uint32_t a, b, col, prev_m, kept_h;
        unsigned long long prio, seen, bit;
        bool has, uncolored;
    };
    for (uint64_t base = (uint64_t)blockIdx.x * (kNpThreads * kNpItems); base < total;
         base += (uint64_t)gridDim.x * (kNpThreads * kNpItems), ++trip) {
        uint32_t* wcount = wtot[trip & 1u][0];
        uint32_t* wpts = wtot[trip & 1u][1];
        uint32_t* wground = wtot[trip & 1u][2];
        uint32_t* wunc = wtot[trip & 1u][3];
        Item item[kNpItems];
#pragma unroll
        for (int j = 0; j < kNpItems; ++j) {
            Item& it = item[j];
            manifold_t& m = it.m;
            const uint64_t idx = base + (uint64_t)j * kNpThreads + threadIdx.x;
            m.count = 0;
            uint32_t a = 0, b = PHYS_GROUND_ID;
            ulonglong2 early = make_ulonglong2(0ull, 0ull);
            uint32_t early_h = 0;
            bool have_early = false;
            if (idx < n_ground) {
                a = (uint32_t)idx;
                if (kFilters && !filter_pass(flt.body[a], flt.ground)) {
                    // filtered out: no manifold, like a body clear of the plane
                } else {
                // the fattened AABB of this step (k_step_velocity_aabb; lo.y = lowest corner - margin) rules most bodies out
                // without their orientation being read or a corner being made: a million-cube drop has 1 % of its bodies on
                // the plane. Conservative: a body is kept unless its AABB clears ground + margin by more than rounding.
                const float4 g2 = reinterpret_cast<const float4*>(geo)[4 * (size_t)a + 2];
                const float lo_y = g2.w;
                if (lo_y <= (ground + margin) + 1.0e-3f * (1.0f + det_absf(lo_y))) {
                    const geom_t ga = load_geom(a, geo);
                    if (ga.type != PHYS_SPEC_SHAPE_NONE) {
                        if (kCapsules) collide_ground(&ga, ground, margin, &m, ws);
                        else collide_ground_sphere_box(&ga, ground, margin, &m, ws);
                    }
                }
                }
            } else if (idx < total) {
                // a candidate pair of two bodies, or (kStatics, behind them) a body and static collider k: B = the static
                const bool body_pair = !kStatics || idx < n_body_items;
                const uint2 pr = body_pair ? reinterpret_cast<const uint2*>(pairs)[idx - n_ground]
                                           : reinterpret_cast<const uint2*>(static_pairs)[idx - n_body_items];
                a = pr.x; b = body_pair ? pr.y : (PHYS_STATIC_ID_BIT | pr.y);
                // kFilters: the two filters before anything else of the pair is read (a rejected pair costs two 8-byte loads)
                if (a < n_owned && (!kFilters || filter_pass(flt.body[a], body_pair ? flt.body[pr.y] : flt.st[pr.y]))) {
                    // the colour-table entry this pair would keep its colour from (a random 16-byte read): asked for NOW, so
                    // that it travels while the shapes are fetched and tested instead of being one more dependent round trip
                    // behind the emission below (nearly every candidate pair of a resting pile becomes a manifold)
                    // (only where most candidate pairs DO become manifolds: a stack of aligned boxes has three sliver pairs for
                    // every contact since the sliver rule, and three wasted 64-byte line fetches out of a 100+ MB table for
                    // every useful one - launch_narrowphase decides from the counts of an earlier update)
                    if (cache_mask && early_probe) {
                        early_h = (uint32_t)(color_priority(a, b) >> 20) & cache_mask;
                        early = cache[early_h];
                        have_early = true;
                    }
                    const geom_t ga = load_geom(a, geo);
                    const geom_t gb = body_pair ? load_geom(b, geo) : load_geom(pr.y, static_geo);
                    if (kCapsules) collide_pair(&ga, &gb, margin, &m, ws);
                    else collide_pair_sphere_box(&ga, &gb, margin, &m, ws);
                }
            }
            const bool has = m.count > 0;
            // ---- everything of a manifold that does not need its slot, BEFORE the workgroup's slot reservation: the kept
            // colour (table entry asked for above; re-stamped below), the colour's mark at the two bodies, or round 0 of the
            // colouring. Their round trips then overlap the reservation's instead of following it.
            // A manifold that turns out to be beyond the capacity has then left its marks too: that update is flagged, its
            // solve skipped and its new manifolds never reach the table, so nothing of it survives.
            unsigned long long prio = 0ull, seen_a = 0ull, seen_b = 0ull, bit = 0ull;
            uint32_t col = kUncolored, prev_m = 0xFFFFFFFFu, kept_h = 0;
            bool uncolored = false;
            if (has) {
                prio = color_priority(a, b);
                // persistent colouring (contact_solve.h): a manifold that existed in the previous update keeps its
                // colour - exact 64-bit key match in the table, stamped by the previous update; re-stamped below
                if (cache_mask) {
                    const unsigned long long key = ((unsigned long long)a << 32) | b;
                    uint32_t h = (uint32_t)(prio >> 20) & cache_mask;
                    // bounded walk: the table is rebuilt every PHYS_COLOR_CACHE_PERIOD updates and holds 1.5 slots per manifold
                    // slot, but a chain of live and dead entries without an empty slot must end the walk, not hang the GPU
                    bool ended = false;
                    for (uint32_t walked = 0; walked < kColorTableMaxWalk; ++walked) {
                        const ulonglong2 e = (have_early && h == early_h) ? early : cache[h];
                        have_early = false;
                        if (e.x == key) {
                            if (table_value_stamp(e.y) + 1u == stamp) {
                                // (the fields by the header's constants, not through table_value_color / _index: with the
                                // calls hipcc loads the value word in a second, dependent round trip after the key matched)
                                col = (uint32_t)e.y & kTableColorMask;
                                prev_m = (uint32_t)e.y >> kTableColorBits;  // the pair's manifold of the previous update
                                kept_h = h;                     // re-stamped below, once this update's slot is known
                            }
                            ended = true;
                            break;  // a dead entry of this key: no live one follows
                        }
                        if (e.x == ~0ull) { ended = true; break; }  // empty slot: never seen
                        h = (h + 1) & cache_mask;
                    }
                    // a walk given up on might have passed over a colour the oracle's map keeps: never silently (bit 6: the
                    // update is flagged and its solve skipped, like any other capacity miss)
                    if (!ended) flag_overflow(ctr, kOvfColorTable);
                }
                if (col != kUncolored) {
                    bit = 1ull << col;
                    seen_a = atomicOr(&used[a], bit);  // looked at after the barrier below
                    if (!PHYS_IS_STATIC_PARTNER(b)) seen_b = atomicOr(&used[b], bit);
                } else {
                    uncolored = true;
                    // round 0 of the colouring: per-body maximum priority (order-independent u64 max)
                    atomicMax(&top0[a], prio);
                    if (!PHYS_IS_STATIC_PARTNER(b)) atomicMax(&top0[b], prio);
                }
            }
            it.a = a; it.b = b; it.col = col; it.prev_m = prev_m; it.kept_h = kept_h;
            it.prio = prio; it.seen = seen_a | seen_b; it.bit = bit; it.has = has; it.uncolored = uncolored;
        }
        // manifolds of the wave: item-major (all of item 0, then all of item 1), lanes in order inside an item
        unsigned long long mask[kNpItems], umask[kNpItems];
        uint32_t n_has = 0, n_gnd = 0, n_unc = 0, pts = 0;
#pragma unroll
        for (int j = 0; j < kNpItems; ++j) {
            mask[j] = __ballot(item[j].has);
            umask[j] = __ballot(item[j].uncolored);
            n_has += (uint32_t)__popcll(mask[j]);
            n_unc += (uint32_t)__popcll(umask[j]);
            n_gnd += (uint32_t)__popcll(__ballot(item[j].has && item[j].b == PHYS_GROUND_ID));
            if (kStatics) acc_static += (uint32_t)__popcll(__ballot(item[j].has && item[j].b != PHYS_GROUND_ID && PHYS_IS_STATIC_PARTNER(item[j].b)));
            pts += item[j].has ? (uint32_t)item[j].m.count : 0u;  // contact points (for the stats counter)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pts += (uint32_t)__shfl_xor((int)pts, off, 64);
        if (lane == 0) {
            wcount[wave] = n_has;
            wpts[wave] = pts;
            wground[wave] = n_gnd;
            wunc[wave] = n_unc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // one set of global atomics per workgroup: same-address atomics serialise chip-wide
            uint32_t t = 0, tp = 0, tg = 0, tu = 0;
            for (int k = 0; k < kNpThreads / 64; ++k) { t += wcount[k]; tp += wpts[k]; tg += wground[k]; tu += wunc[k]; }
            uint32_t bb = 0, ub = 0;
            if (t) {
                // ONE reservation for both lists: manifold slots (low word) and this workgroup's stretch of the round-0 list
                // of uncoloured manifolds (high word); see StepCounters
                const unsigned long long got = atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->n_manifolds),
                                                         ((unsigned long long)tu << 32) | t);
                bb = (uint32_t)got;
                ub = (uint32_t)(got >> 32);
                const uint64_t room = (uint64_t)bb < max_manifolds ? max_manifolds - bb : 0;
                const uint32_t stored = (uint64_t)t <= room ? t : (uint32_t)room;
                if (stored != t) flag_overflow(ctr, kOvfManifolds);
                acc_pts += tp; acc_ground += tg; acc_unc += tu;
            }
            block_base = bb;
            unc_base = ub;
        }
        __syncthreads();
        uint32_t woff = 0, uoff = 0;
        for (int k = 0; k < wave; ++k) { woff += wcount[k]; uoff += wunc[k]; }
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int j = 0; j < kNpItems; ++j) {
            const Item& it = item[j];
            if (it.has) {
                const manifold_t& m = it.m;
                const uint32_t a = it.a, b = it.b, col = it.col;
                const uint64_t slot = (uint64_t)block_base + woff + (uint32_t)__popcll(mask[j] & below);
                if (slot < max_manifolds) {
                    man_a[slot] = a;
                    man_b[slot] = b;
                    man_prio[slot] = it.prio;
                    man_color[slot] = col;
                    // a kept entry is re-stamped with this update's manifold index (one 8-byte store to the line the probe read)
                    if (col != kUncolored) cache[it.kept_h].y = table_value_encode(stamp, (uint32_t)slot, col);
                    if (man_prev) {
                        float4* imp = reinterpret_cast<float4*>(man_imp) + kImpulseVecs * slot;
                        for (uint32_t k = 0; k < kImpulseVecs; ++k) imp[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                    // (Measured and dropped: staging the records of a wave in LDS and copying them out as whole 128-byte lines -
                    // 4.5 write requests per manifold become 2 - left the kernel at 0.52 ms on C5: it waits on its chain of
                    // dependent round trips, not on the write path.)
                    float4* o = reinterpret_cast<float4*>(man_geo) + kManifoldVecs * slot;  // one 128-byte line per manifold (records.hpp)
                    // ids, count, kept colour and the previous update's index ride in the record: k_rows_build would otherwise
                    // gather them, 4 bytes out of a 64-byte sector each, from two more arrays through the row permutation
                    manifold_head_encode(ManifoldHead{a, b, (uint32_t)m.count, col}, o[kManifoldVecHead]);  // (one 16-byte store)
                    o[kManifoldVecNormal] = make_float4(m.normal.x, m.normal.y, m.normal.z, __uint_as_float(it.prev_m));
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[kManifoldVecPoint + k] = make_float4(m.pt[k].x, m.pt[k].y, m.pt[k].z, m.depth[k]);
                }
                if (it.uncolored) {
                    // (a manifold beyond the capacity - update flagged, never solved - names the last slot: the list must hold
                    // ids of stored manifolds only, whatever else happens to that update)
                    const uint32_t at = unc_base + uoff + (uint32_t)__popcll(umask[j] & below);
                    unc_list[at < max_manifolds ? at : (uint32_t)max_manifolds - 1u] =
                        slot < max_manifolds ? (uint32_t)slot : (uint32_t)max_manifolds - 1u;
                } else if ((it.seen & it.bit) != 0ull) {
                    // order-independent. A kept colour that was ALREADY in use at one of the bodies means the previous
                    // colouring was not proper (it saturated at PHYS_MAX_COLORS): two rows of one colour on one body
                    // would race in the solver, so the step is flagged like any other colour overflow (no solve)
                    flag_overflow(ctr, kOvfColors);
                }
            }
            woff += (uint32_t)__popcll(mask[j]);
            uoff += (uint32_t)__popcll(umask[j]);
        }
        // (block_base / unc_base are rewritten behind the next trip's first barrier, which every wave reaches only after it
        // has placed this trip's manifolds; the per-wave totals alternate between two sets)
    }
    if (threadIdx.x == 0) {
        if (acc_pts) atomicAdd(&ctr->n_contacts, acc_pts);
        if (acc_ground) atomicAdd(&ctr->n_ground_manifolds, acc_ground);
        if (acc_unc) { atomicAdd(&ctr->n_uncolored, acc_unc); atomicAdd(&ctr->n_new_manifolds, acc_unc); }
    }
    if (kStatics && (threadIdx.x & 63) == 0 && acc_static) atomicAdd(&ctr->n_static_manifolds, acc_static);
}

void launch_narrowphase(phys_world* w, const NarrowPlan& plan) {
    const uint32_t n = (uint32_t)w->n;
    if (n == 0) return;
    // ghost bodies of a sharded world (slots behind the owned bodies) are dynamic bodies of this world for one update
    // (halo.hip k_halo_unpack): they rest on the ground and on each other like everybody else
    const uint32_t n_owned = n;
    const uint32_t n_ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? n : 0u;
    // static colliders (static.hip): their pairs with the bodies are the third kind of work item
    uint64_t st_cap = 0;
    const uint32_t* st_pairs = nullptr;
    const float* st_geo = nullptr;
    static_narrow_args(w, &st_cap, &st_pairs, &st_geo);
    // colouring state of the step: used masks + three rotating priority buffers (one memset); the narrow
    // phase publishes round 0's per-body maxima as it emits manifolds
    // persistent colouring: colours of the previous update are kept (contact_solve.h)
    const uint32_t cache_mask = w->ctab_valid ? w->ctab_mask : 0u;
    const uint32_t stamp = (uint32_t)w->color_epoch + 1u;  // never 0xFFFFFFFF (the stamp of an empty slot) in a world's life
    if (w->warm) {  // last update's records become "previous": what this update's kept manifolds start from
        std::swap(w->man_geo.p, w->man_geo_prev.p);
        std::swap(w->man_imp.p, w->man_imp_prev.p);
    }
    NpFilters flt{};
    flt.body = reinterpret_cast<const uint2*>(w->filt.p);
    flt.st = st_pairs ? reinterpret_cast<const uint2*>(w->st_filt.p) : nullptr;
    flt.ground = make_uint2(w->ground_filt, 0u);
    PHYS_PROF(w, PHYS_STAGE_NARROW);
    // the instance of the plan (plan.hpp: worlds without static colliders run the kernel they always ran, the static work
    // items are compiled out of it; capsules wherever one can meet the narrow phase; filters once any was set)
    dispatch_bool(plan.threads == 128, [&](auto few_t) { dispatch_bool(plan.statics, [&](auto st_t) {
    dispatch_bool(plan.capsules, [&](auto cap_t) { dispatch_bool(plan.filters, [&](auto flt_t) {
        constexpr int T = decltype(few_t)::value ? 128 : 512;
        constexpr bool S = decltype(st_t)::value, CAP = decltype(cap_t)::value, FLT = decltype(flt_t)::value;
        // (the filtered instance takes `flt` as one more argument; the unfiltered one is launched exactly as before filters)
        auto launch = [&](auto... filters) {
            hipLaunchKernelGGL((k_narrowphase<T, 1, S, CAP, FLT>), dim3(plan.blocks), dim3(T), 0, w->stream, n_ground, n_owned, w->pairs.p,
                               w->max_pairs, w->geo.p, w->cfg.contact_margin, w->cfg.ground_height, w->max_manifolds, w->man_a.p, w->man_b.p,
                               w->man_color.p, w->man_geo.p, w->man_prio.p, w->color_state.p, w->color_state.p + n,
                               reinterpret_cast<ulonglong2*>(w->ctab.p), cache_mask, plan.early_probe, stamp, w->unc_list.p,
                               w->warm ? w->man_prev.p : nullptr, w->man_imp.p, w->counters.p, st_cap, st_pairs, st_geo, filters...);
        };
        if constexpr (FLT) launch(flt); else launch();
    }); }); }); });
}

}  // namespace phys
