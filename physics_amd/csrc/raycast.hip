// raycast.hip — batched ray casts and sphere casts against the current poses (phys_raycast / phys_raycast_device,
// phys_spherecast / phys_spherecast_device), and the query grid they and the overlap queries (query.hip) walk.
//
// A read-only query: it owns its acceleration structure, rebuilt on every call from the SoA poses (pos, rot, half_extent,
// shape) inside rc_* buffers of its own, and writes nothing an update or phys_broadphase reads (no counters, no bucket_*
// or sorted_* arrays, no grid_valid, no scan_block_sums, not geo: that is the pose at the START of the last update).
//
// Build (7 launches and one memset, no host round trip):
//   k_rc_bounds   one reduction over the owned bodies with a shape: scene bounds of the exact AABBs and the largest exact
//                 AABB edge e, as order-preserving integer keys under atomicMax (min / max do not depend on arrival order)
//   k_rc_insert<false>  every body into every cell its padded AABB touches (at most 2 per axis: the cell edge exceeds the
//                 padded edge), counted per bucket of a hashed table of >= 2N buckets
//   k_rc_scan_*   exclusive scan of the bucket counts (own scratch: w->scan_block_sums belongs to the update)
//   k_rc_insert<true>   the same cells again: one 48-byte record {centre, shape} {rot} {half extent, id} per insertion, in
//                 bucket order, so a candidate is one record read and no gather from four arrays
// Static colliders (static.hip) are tested one by one in front of the walk, from records phys_set_static_bodies made once:
// O(statics) per ray, nothing rebuilt per call (a world without statics runs no extra test).
// Traversal (k_rc_trace): one ray per lane, clipped to the grid box and [0, min(max_t, ground hit)], Amanatides-Woo DDA
// with the state in named scalars and the stepping axis chosen by selects (a runtime-indexed float[3] goes to scratch,
// which the build rules forbid). Every candidate of a cell is tested exactly; the walk stops once the best t is at or
// below the cell's exit t (a candidate's hit beyond the exit may still be beaten by a later cell: multi-insertion). The
// winner is the least (t, id); the order in which the scatter's atomics placed a bucket's records changes nothing.
// Sphere casts (k_rc_trace<, true>) run the same walk for the ball's centre over a grid whose body AABBs were grown by the
// call's largest valid radius (k_sc_grow writes it into the header before k_rc_bounds; ray casts leave it zero, which
// changes no arithmetic), and test each candidate with sc_test: the ray against the target grown by the ball's radius.
// Capsule casts (phys_capsulecast) are a third instance of the same kernel, chosen by a CapsuleArgs in
// its argument pack: the grid grown by the largest valid radius + half-length, every candidate tested with cc_test
// (capsule_cast.hpp); a capsule of half-length 0 is a ball and calls sc_test.
// The per-query walk itself (rc_walk) and the tests of a ray and of a ball live in cast_walk.hpp, which move-and-slide
// (slide.hip) calls too: k_rc_trace is a loader and a storer around it.
#include <cstdio>

#include "cast_walk.hpp"

namespace phys {

namespace {

constexpr int kRcScanItems = 16;                              // per thread of the scan kernels
constexpr uint32_t kRcScanTile = kRcThreads * kRcScanItems;   // 4096 buckets per workgroup; the table is a multiple of it
constexpr int kRcMaxBoundsBlocks = 1024;
// a sphere cast grows the grid by its largest valid radius, capped here so that grown bounds stay finite
constexpr float kScMaxGrow = 0x1p100f;

__global__ __launch_bounds__(kRcThreads) void k_rc_bounds(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                         const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                         RcHeader* __restrict__ hdr) {
    float k[7];  // -lo xyz, hi xyz, edge (fully unrolled: registers, not scratch)
#pragma unroll
    for (int a = 0; a < 7; ++a) k[a] = -3.0e38f;
    bool any = false;
    const float grow = __uint_as_float(hdr->grow);  // written before this launch (k_sc_grow) or zero
    for (uint32_t i = blockIdx.x * kRcThreads + threadIdx.x; i < n; i += gridDim.x * kRcThreads) {
        aabb_t b;
        if (!rc_aabb(pos, rot, he, shape, i, &b)) continue;
        b = rc_grown(b, grow);
        any = true;
        k[0] = fmaxf(k[0], -b.lo.x); k[1] = fmaxf(k[1], -b.lo.y); k[2] = fmaxf(k[2], -b.lo.z);
        k[3] = fmaxf(k[3], b.hi.x); k[4] = fmaxf(k[4], b.hi.y); k[5] = fmaxf(k[5], b.hi.z);
        k[6] = fmaxf(k[6], fmaxf(b.hi.x - b.lo.x, fmaxf(b.hi.y - b.lo.y, b.hi.z - b.lo.z)));
    }
    __shared__ float red[kRcThreads / 64][7];
    __shared__ int any_wave[kRcThreads / 64];
    const auto op_fmax = [](float a, float b) { return fmaxf(a, b); };  // (never a NaN here: either order of operands)
#pragma unroll
    for (int a = 0; a < 7; ++a) k[a] = wave_reduce(k[a], op_fmax);
    const bool wave_any = __any(any);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 7; ++a) red[wave][a] = k[a];
        any_wave[wave] = wave_any ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        float v = -3.0e38f;
        int seen = 0;
        for (int w = 0; w < kRcThreads / 64; ++w) { v = fmaxf(v, red[w][threadIdx.x]); seen |= any_wave[w]; }
        if (seen) atomicMax(&reinterpret_cast<uint32_t*>(hdr)[threadIdx.x], f2key(v));
    }
}

// pass 0 (WRITE = false): count the insertions per bucket; pass 1: place the records, counting each bucket back down to
// zero (the counts leave the call zeroed)
template <bool WRITE>
__global__ __launch_bounds__(kRcThreads) void k_rc_insert(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                         const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                         const RcHeader* __restrict__ hdr, uint32_t bits, uint32_t* __restrict__ count,
                                                         const uint32_t* __restrict__ start, float4* __restrict__ rec, uint32_t rec_cap) {
    const uint32_t i = blockIdx.x * kRcThreads + threadIdx.x;
    if (i >= n) return;
    aabb_t b;
    if (!rc_aabb(pos, rot, he, shape, i, &b)) return;
    const RcGrid g = rc_grid(hdr);
    const RcCells cl = rc_body_cells(g, rc_grown(b, __uint_as_float(hdr->grow)));
    const int x0 = cl.x0, x1 = cl.x1, y0 = cl.y0, y1 = cl.y1, z0 = cl.z0, z1 = cl.z1;
    float4 r0, r1, r2;
    if (WRITE) {
        const v3 c = ld3(pos, i), h = ld3(he, i);
        r0 = make_float4(c.x, c.y, c.z, __uint_as_float(shape[i]));
        r1 = reinterpret_cast<const float4*>(rot)[i];
        r2 = make_float4(h.x, h.y, h.z, __uint_as_float(i));
    }
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const uint32_t bk = rc_bucket(x, y, z, bits);
                if (!WRITE) {
                    atomicAdd(&count[bk], 1u);
                } else {
                    const uint32_t slot = start[bk] + atomicSub(&count[bk], 1u) - 1u;
                    if (slot < rec_cap) {
                        rec[3 * (size_t)slot] = r0;
                        rec[3 * (size_t)slot + 1] = r1;
                        rec[3 * (size_t)slot + 2] = r2;
                    }
                }
            }
}

// exclusive scan over 4096-bucket tiles: tile sums, one workgroup scans the tile sums, tiles scanned with their offsets.
// (Three small launches at every table size: the one-launch scan of scan.hip was 3 us per call slower at 32768 buckets,
// DESIGN.md section 18.) The lane's exclusive prefix over the workgroup and the workgroup's total: the wave scan, then
// the four wave totals.
__device__ __forceinline__ uint32_t rc_block_exclusive(uint32_t v, uint32_t* total) {
    __shared__ uint32_t s_tot[kRcThreads / 64];
    const uint32_t inc = wave_inclusive_scan(v), wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)(kRcThreads / 64); ++k) {
        const uint32_t t = s_tot[k];
        if (k < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;  // (one call per kernel: s_tot is not rewritten)
}

__global__ __launch_bounds__(kRcThreads) void k_rc_scan_reduce(const uint32_t* __restrict__ count, uint32_t* __restrict__ tile_sum) {
    const uint4* p = reinterpret_cast<const uint4*>(count + (size_t)blockIdx.x * kRcScanTile + threadIdx.x * kRcScanItems);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kRcScanItems / 4; ++k) { const uint4 v = p[k]; s += (v.x + v.y) + (v.z + v.w); }
    uint32_t total;
    (void)rc_block_exclusive(s, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kRcThreads) void k_rc_scan_tiles(uint32_t* __restrict__ tile_sum, uint32_t tiles) {
    const uint32_t total = block_scan_in_place<kRcThreads>(tile_sum, tiles);
    if (threadIdx.x == 0) tile_sum[tiles] = total;
}

__global__ __launch_bounds__(kRcThreads) void k_rc_scan_final(const uint32_t* __restrict__ count, const uint32_t* __restrict__ tile_sum,
                                                             uint32_t tiles, uint32_t* __restrict__ start) {
    const size_t at = (size_t)blockIdx.x * kRcScanTile + threadIdx.x * kRcScanItems;
    const uint4* p = reinterpret_cast<const uint4*>(count + at);
    uint4 v[kRcScanItems / 4];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kRcScanItems / 4; ++k) { v[k] = p[k]; s += (v[k].x + v[k].y) + (v[k].z + v[k].w); }
    uint32_t total;
    uint32_t run = tile_sum[blockIdx.x] + rc_block_exclusive(s, &total);
    uint4* o = reinterpret_cast<uint4*>(start + at);
#pragma unroll
    for (int k = 0; k < kRcScanItems / 4; ++k) {
        uint4 r;
        r.x = run; run += v[k].x;
        r.y = run; run += v[k].y;
        r.z = run; run += v[k].z;
        r.w = run; run += v[k].w;
        o[k] = r;
    }
    if (blockIdx.x == tiles - 1 && threadIdx.x == 0) start[(size_t)tiles * kRcScanTile] = tile_sum[tiles];
}

// One query per lane: loads it, walks it (rc_walk, cast_walk.hpp: the exact tests and the walk itself) and stores its answer.
// SWEEP: a sphere cast (radius per ray); otherwise a ray cast (radius unused, the arithmetic of the ray cast unchanged).
// FILT: the _filtered calls (one QueryFilters argument, the pack `filt`): a target whose category misses the query's mask
// is skipped before its exact test; without it the pack is empty and the kernel is the one it was before filters.
// A CapsuleArgs in front of the pack (SWEEP instances only) makes the instance the capsule cast: lanes with a half-length
// above 0 test with cc_test and find their contact after the walk, the others are sphere casts with a touched point.
template <bool STATS, bool SWEEP, bool FILT, typename... Filt>
__global__ __launch_bounds__(kRcThreads) void k_rc_trace(uint32_t n_rays, const float* __restrict__ origin, const float* __restrict__ dir,
                                                        const float* __restrict__ radius,
                                                        const float* __restrict__ max_t, const uint32_t* __restrict__ ignore_body,
                                                        const RcHeader* __restrict__ hdr, uint32_t bits, const uint32_t* __restrict__ start,
                                                        const float4* __restrict__ rec, uint32_t n_bodies, int ground, float ground_y,
                                                        const float4* __restrict__ st_rec, uint32_t n_static,
                                                        uint32_t* __restrict__ body_out, float* __restrict__ t_out, float* __restrict__ normal_out,
                                                        unsigned long long* __restrict__ stats, Filt... filt) {
    constexpr bool CAPS = has_capsule_args<Filt...>::value;
    static_assert(sizeof...(Filt) == (FILT ? 1u : 0u) + (CAPS ? 1u : 0u), "one QueryFilters argument exactly in the filtered instance");
    static_assert(SWEEP || !CAPS, "a capsule cast is a sweep");
    CapsuleArgs ca{};
    if constexpr (CAPS) ca = capsule_arg(filt...);
    const uint32_t r = blockIdx.x * kRcThreads + threadIdx.x;
    if (r >= n_rays) return;
    QueryFilters qf{};
    if constexpr (FILT) qf = filter_arg(filt...);
    const uint32_t qm = FILT ? (uint32_t)qf.query_mask[r] : 0xFFFFu;
    uint32_t cells = 0, cands = 0;
    const v3 o = ld3(origin, r), d = ld3(dir, r);
    const float tmax = max_t ? max_t[r] : __builtin_inff();
    const uint32_t ign = ignore_body && ignore_body[r] < n_bodies ? ignore_body[r] : 0xFFFFFFFFu;
    const float len = rc_length(d);
    const float rad = SWEEP ? radius[r] : 0.0f;
    // the capsule's core: half-length hq along a, the y axis of rot (used as given); a bad half-length or rot misses
    float hq = 0.0f, ax = 0.0f, ay = 1.0f, az = 0.0f;
    bool cap_ok = true;
    if constexpr (CAPS) {
        hq = ca.half_length[r];
        cap_ok = hq >= 0.0f && hq <= 3.4e38f;
        if (ca.rot) {
            const float4 q4 = make_float4(ca.rot[4 * (size_t)r], ca.rot[4 * (size_t)r + 1], ca.rot[4 * (size_t)r + 2], ca.rot[4 * (size_t)r + 3]);
            cap_ok = cap_ok && isfinite(q4.x) && isfinite(q4.y) && isfinite(q4.z) && isfinite(q4.w);
            rc_capsule_axis(q4, ax, ay, az);
        }
    }
    RayHit best;
    v3 point;
    rc_walk<STATS, SWEEP, FILT, CAPS>(hdr, bits, start, rec, ground, ground_y, st_rec, n_static, qf, qm, o, d, len, tmax, ign, rad, hq, ax, ay, az, cap_ok, best, point, cells, cands);
    body_out[r] = best.id;
    t_out[r] = best.t;
    if (normal_out) st3(normal_out, r, v3_make(best.nx, best.ny, best.nz));
    if constexpr (CAPS) { if (ca.point_out) st3(ca.point_out, r, point); }
    if (STATS) { atomicAdd(&stats[0], (unsigned long long)cells); atomicAdd(&stats[1], (unsigned long long)cands); }
}

// the largest valid (finite, non-negative) radius of a sphere cast into the header's grow slot, capped at kScMaxGrow:
// non-negative floats order as their bits, so one atomicMax per workgroup
// (a capsule cast: the largest radius + half-length over the queries in which both are valid)
__global__ __launch_bounds__(kRcThreads) void k_sc_grow(uint32_t n, const float* __restrict__ radius, const float* __restrict__ half_length,
                                                       RcHeader* __restrict__ hdr) {
    float m = 0.0f;
    for (uint32_t i = blockIdx.x * kRcThreads + threadIdx.x; i < n; i += gridDim.x * kRcThreads) {
        const float r = radius[i], h = half_length ? half_length[i] : 0.0f;
        if (r >= 0.0f && r <= 3.4e38f && h >= 0.0f && h <= 3.4e38f) m = fmaxf(m, fminf(half_length ? r + h : r, kScMaxGrow));
    }
    const auto op_fmax = [](float a, float b) { return fmaxf(a, b); };
    __shared__ float red[kRcThreads / 64];
    block_put(m, red, op_fmax);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&hdr->grow, __float_as_uint(block_get<kRcThreads>(red, op_fmax)));
}

}  // namespace

int32_t launch_query_grid(phys_world* w, const float* grow_radius, const float* grow_half_length, uint64_t n_grow, uint32_t* bits_out,
                          const float* grow_half_extent) {
    hipStream_t s = w->stream;
    const uint64_t n = w->n_owned;
    PHYS_HIP_TRY(w->rc_header.resize(sizeof(RcHeader) / 4));
    PHYS_HIP_TRY(hipMemsetAsync(w->rc_header.p, 0, sizeof(RcHeader), s));
    const RcHeader* hdr = reinterpret_cast<const RcHeader*>(w->rc_header.p);
    uint32_t bits = 12;
    if (n > (1ull << 29)) { set_error("query grid: more than 2^29 bodies (the query's grid indexes insertions with 32 bits)"); return PHYS_ERR_UNSUPPORTED; }
    if (n) {
        // table: a power of two >= 2N buckets (and a whole number of scan tiles); records: 8 insertions per body at most
        while ((1ull << bits) < 2 * n) ++bits;
        const uint32_t table = 1u << bits, tiles = table / kRcScanTile;
        PHYS_HIP_TRY(w->rc_count.resize(table));
        PHYS_HIP_TRY(w->rc_start.resize((size_t)table + 1));
        PHYS_HIP_TRY(w->rc_tile_sum.resize((size_t)tiles + 1));
        PHYS_HIP_TRY(w->rc_records.resize(12 * 8 * (size_t)n));  // 8 records of three float4 per body
        PHYS_HIP_TRY(hipMemsetAsync(w->rc_count.p, 0, 4 * (size_t)table, s));
        const uint32_t nn = (uint32_t)n;
        if (grow_radius && n_grow)
            hipLaunchKernelGGL(k_sc_grow, dim3(std::min<unsigned>(rc_blocks(n_grow), kRcMaxBoundsBlocks)), dim3(kRcThreads), 0, s,
                               (uint32_t)n_grow, grow_radius, grow_half_length, reinterpret_cast<RcHeader*>(w->rc_header.p));
        if (grow_half_extent && n_grow) launch_box_grow(w, grow_half_extent, n_grow);  // a box cast: boxcast.hip's own reduction
        const unsigned bb = std::min<unsigned>(rc_blocks(n), kRcMaxBoundsBlocks);
        hipLaunchKernelGGL(k_rc_bounds, dim3(bb), dim3(kRcThreads), 0, s, nn, w->pos.p, w->rot.p, w->half_extent.p, w->shape.p,
                           reinterpret_cast<RcHeader*>(w->rc_header.p));
        hipLaunchKernelGGL(k_rc_insert<false>, dim3(rc_blocks(n)), dim3(kRcThreads), 0, s, nn, w->pos.p, w->rot.p, w->half_extent.p,
                           w->shape.p, hdr, bits, w->rc_count.p, (const uint32_t*)nullptr, (float4*)nullptr, 0u);
        hipLaunchKernelGGL(k_rc_scan_reduce, dim3(tiles), dim3(kRcThreads), 0, s, w->rc_count.p, w->rc_tile_sum.p);
        hipLaunchKernelGGL(k_rc_scan_tiles, dim3(1), dim3(kRcThreads), 0, s, w->rc_tile_sum.p, tiles);
        hipLaunchKernelGGL(k_rc_scan_final, dim3(tiles), dim3(kRcThreads), 0, s, w->rc_count.p, w->rc_tile_sum.p, tiles, w->rc_start.p);
        hipLaunchKernelGGL(k_rc_insert<true>, dim3(rc_blocks(n)), dim3(kRcThreads), 0, s, nn, w->pos.p, w->rot.p, w->half_extent.p,
                           w->shape.p, hdr, bits, w->rc_count.p, w->rc_start.p, reinterpret_cast<float4*>(w->rc_records.p),
                           (uint32_t)(8 * n));
    }
    *bits_out = bits;
    return PHYS_OK;
}

// the walk shared by ray casts, sphere casts and capsule casts: the kind names the kernel instance, the arrays are the batch's
int32_t launch_query(phys_world* w, CastKind kind, const CastBatch& b) {
    if (kind == CastKind::Box) return launch_boxcast(w, b);  // a kernel of its own (boxcast.hip)
    hipStream_t s = w->stream;
    const bool sweep = kind != CastKind::Ray, capsule = kind == CastKind::Capsule;
    const float* radius = sweep ? b.radius : nullptr;
    const CapsuleArgs caps{b.rot, b.half_length, b.point_out};
    QueryGrid g;
    PHYS_TRY(query_grid(w, radius, capsule ? b.half_length : nullptr, sweep ? b.n : 0, &g));
    const bool stats = debug_switches().raycast_stats;
    if (stats) {
        PHYS_HIP_TRY(w->rc_stats.resize(2));
        PHYS_HIP_TRY(hipMemsetAsync(w->rc_stats.p, 0, 16, s));
    }
    const QueryFilters qf = query_filters(w, b.query_mask);
#define PHYS_RC_LAUNCH(SW, FILT, ...)                                                                                        \
    hipLaunchKernelGGL((k_rc_trace<kSt, SW, FILT>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, s, (uint32_t)b.n, b.origin, b.dir,   \
                       radius, b.max_t, b.ignore_body, g.hdr, g.bits, g.start, g.rec, g.n_bodies, g.ground, g.ground_y, g.st_rec,  \
                       g.n_static, b.body_out, b.t_out, b.normal_out, w->rc_stats.p, ##__VA_ARGS__)
    dispatch_bool(stats, [&](auto st) {
        constexpr bool kSt = decltype(st)::value;
        if (capsule) {
            if (b.query_mask) PHYS_RC_LAUNCH(true, true, caps, qf);
            else PHYS_RC_LAUNCH(true, false, caps);
            return;
        }
        dispatch_bool(sweep, [&](auto sw) {
            constexpr bool kSw = decltype(sw)::value;
            if (b.query_mask) PHYS_RC_LAUNCH(kSw, true, qf);
            else PHYS_RC_LAUNCH(kSw, false);
        });
    });
#undef PHYS_RC_LAUNCH
    PHYS_HIP_TRY(hipGetLastError());
    if (stats) {
        unsigned long long h[2] = {0, 0};
        PHYS_HIP_TRY(hipMemcpyAsync(h, w->rc_stats.p, 16, hipMemcpyDeviceToHost, s));
        PHYS_HIP_TRY(hipStreamSynchronize(s));
        fprintf(stderr, "%s rays=%llu cells=%llu candidates=%llu\n",
                capsule ? "PHYS_CAPSULECAST_STATS" : (sweep ? "PHYS_SPHERECAST_STATS" : "PHYS_RAYCAST_STATS"),
                (unsigned long long)b.n, h[0], h[1]);
    }
    return PHYS_OK;
}

}  // namespace phys
