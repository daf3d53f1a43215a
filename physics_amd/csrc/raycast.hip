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
#include <cstdio>

#include "capsule_cast.hpp"

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

// exact test of one record; accepted into `best` when t <= tmax and (t, id) beats it
__device__ __forceinline__ void rc_test(const float4* __restrict__ rec, uint32_t k, float ox, float oy, float oz, float ux, float uy,
                                        float uz, float tmax, uint32_t ignore, RayHit& best) {
    const float4 a = rec[3 * (size_t)k];
    const float4 c = rec[3 * (size_t)k + 2];
    const uint32_t id = __float_as_uint(c.w);
    if (id == ignore) return;
    const float px = ox - a.x, py = oy - a.y, pz = oz - a.z;  // origin relative to the centre
    float t, nx, ny, nz;
    if (__float_as_uint(a.w) == PHYS_SHAPE_SPHERE) {
        if (!ray_ball(px, py, pz, ux, uy, uz, c.x, t, nx, ny, nz)) return;
    } else if (__float_as_uint(a.w) == PHYS_SHAPE_CAPSULE) {
        // radius c.x, core c +- c.y * w, w = column 1 of R
        float wx, wy, wz;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        if (!ray_capsule(px, py, pz, ux, uy, uz, wx, wy, wz, c.x, c.y, t, nx, ny, nz)) return;
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        m33 R;
        quat_to_m33(q, &R);  // world = R * local: the local frame is R^T (the conjugate rotation)
        const float lx = (R.m[0] * px + R.m[3] * py) + R.m[6] * pz;
        const float ly = (R.m[1] * px + R.m[4] * py) + R.m[7] * pz;
        const float lz = (R.m[2] * px + R.m[5] * py) + R.m[8] * pz;
        const float dx = (R.m[0] * ux + R.m[3] * uy) + R.m[6] * uz;
        const float dy = (R.m[1] * ux + R.m[4] * uy) + R.m[7] * uz;
        const float dz = (R.m[2] * ux + R.m[5] * uy) + R.m[8] * uz;
        float sx, sy, sz;
        const int res = ray_box_local(lx, ly, lz, dx, dy, dz, c.x, c.y, c.z, t, sx, sy, sz);
        if (res == 0) return;
        if (res == 1) {  // origin inside the closed box
            nx = -ux; ny = -uy; nz = -uz;
        } else {
            // local normal of the entering slab, into the world frame
            nx = (R.m[0] * sx + R.m[1] * sy) + R.m[2] * sz;
            ny = (R.m[3] * sx + R.m[4] * sy) + R.m[5] * sz;
            nz = (R.m[6] * sx + R.m[7] * sy) + R.m[8] * sz;
            const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);  // R of a nearly-unit quaternion
            nx *= inv; ny *= inv; nz *= inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) { best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz; }
}

// a ball of radius rad swept from o along u against one record: the ray against the record's shape grown by rad (its
// Minkowski sum with the ball). Sphere r: the ball of r + rad. Capsule r: the capsule of r + rad. Box: the rounded box,
// the union of three boxes each grown by rad along one axis (its flat faces) and of the twelve edge capsules of radius
// rad (the cylinders along the edges; their end balls are the rounded corners): the least t over the fifteen. The normal
// runs from the target's closest point to the centre at t; from inside (t = 0) it is -u.
__device__ __forceinline__ void sc_test(const float4* __restrict__ rec, uint32_t k, float ox, float oy, float oz, float ux, float uy,
                                        float uz, float rad, float tmax, uint32_t ignore, RayHit& best) {
    const float4 a = rec[3 * (size_t)k];
    const float4 c = rec[3 * (size_t)k + 2];
    const uint32_t id = __float_as_uint(c.w);
    if (id == ignore) return;
    const float px = ox - a.x, py = oy - a.y, pz = oz - a.z;
    float t, nx, ny, nz;
    if (__float_as_uint(a.w) == PHYS_SHAPE_SPHERE) {
        if (!ray_ball(px, py, pz, ux, uy, uz, c.x + rad, t, nx, ny, nz)) return;
    } else if (__float_as_uint(a.w) == PHYS_SHAPE_CAPSULE) {
        float wx, wy, wz;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        if (!ray_capsule(px, py, pz, ux, uy, uz, wx, wy, wz, c.x + rad, c.y, t, nx, ny, nz)) return;
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        m33 R;
        quat_to_m33(q, &R);
        const float lx = (R.m[0] * px + R.m[3] * py) + R.m[6] * pz;
        const float ly = (R.m[1] * px + R.m[4] * py) + R.m[7] * pz;
        const float lz = (R.m[2] * px + R.m[5] * py) + R.m[8] * pz;
        const float dx = (R.m[0] * ux + R.m[3] * uy) + R.m[6] * uz;
        const float dy = (R.m[1] * ux + R.m[4] * uy) + R.m[7] * uz;
        const float dz = (R.m[2] * ux + R.m[5] * uy) + R.m[8] * uz;
        float sx, sy, sz;
        // the rounded box lies inside the box grown by rad along every axis: a ray that misses that misses it
        if (ray_box_local(lx, ly, lz, dx, dy, dz, c.x + rad, c.y + rad, c.z + rad, t, sx, sy, sz) == 0) return;
        const float gx = fmaxf(fabsf(lx) - c.x, 0.0f), gy = fmaxf(fabsf(ly) - c.y, 0.0f), gz = fmaxf(fabsf(lz) - c.z, 0.0f);
        bool inside = (gx * gx + gy * gy) + gz * gz <= rad * rad;  // the centre starts within rad of the box
        float mx = 0.0f, my = 0.0f, mz = 0.0f;  // local normal of the best part
        t = __builtin_inff();
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            float tb, bx, by, bz;
            const int res = ray_box_local(lx, ly, lz, dx, dy, dz, c.x + (ax == 0 ? rad : 0.0f), c.y + (ax == 1 ? rad : 0.0f),
                                          c.z + (ax == 2 ? rad : 0.0f), tb, bx, by, bz);
            inside = inside || res == 1;
            if (res == 2 && tb < t) { t = tb; mx = bx; my = by; mz = bz; }
        }
        // radius 0: the rounded box is the box (and a zero-radius cylinder is ill-conditioned), so no edges
#pragma unroll
        for (int e = 0; e < (rad > 0.0f ? 12 : 0); ++e) {
            // edge e along axis e / 4, at the corner signs of bits 0 and 1 of e on the other two axes
            const int ax = e >> 2;
            const float s1 = (e & 1) ? 1.0f : -1.0f, s2 = (e & 2) ? 1.0f : -1.0f;
            const float ex = ax == 0 ? 0.0f : s1 * c.x;
            const float ey = ax == 1 ? 0.0f : (ax == 0 ? s1 : s2) * c.y;
            const float ez = ax == 2 ? 0.0f : s2 * c.z;
            const float hl = ax == 0 ? c.x : (ax == 1 ? c.y : c.z);
            float te, ex_n, ey_n, ez_n;
            if (ray_capsule(lx - ex, ly - ey, lz - ez, dx, dy, dz, ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f,
                            rad, hl, te, ex_n, ey_n, ez_n) &&
                te < t) {
                t = te; mx = ex_n; my = ey_n; mz = ez_n;
            }
        }
        if (inside) {
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            if (!(t < __builtin_inff())) return;
            // the normal runs from the box's closest point to the centre at t: a face and the cylinder beside it give
            // nearly equal t near their seam, and this does not depend on which of them rounding picked (the part's own
            // normal stays for a centre that rounding put within rad / 2 of the box)
            const float cx = lx + t * dx, cy = ly + t * dy, cz = lz + t * dz;
            const float vx = cx - fminf(fmaxf(cx, -c.x), c.x), vy = cy - fminf(fmaxf(cy, -c.y), c.y), vz = cz - fminf(fmaxf(cz, -c.z), c.z);
            if ((vx * vx + vy * vy) + vz * vz > 0.25f * (rad * rad)) { mx = vx; my = vy; mz = vz; }
            nx = (R.m[0] * mx + R.m[1] * my) + R.m[2] * mz;
            ny = (R.m[3] * mx + R.m[4] * my) + R.m[5] * mz;
            nz = (R.m[6] * mx + R.m[7] * my) + R.m[8] * mz;
            const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
            nx *= inv; ny *= inv; nz *= inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) { best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz; }
}

__device__ __forceinline__ float rc_plane_t(int i, bool up, float lo, float cell, float o, float inv_u) {
    return ((lo + (float)(i + (up ? 1 : 0)) * cell) - o) * inv_u;
}

// SWEEP: a sphere cast (radius per ray; the grid was grown by the largest valid radius, so the walk of the centre line
// meets every target the ball can touch); otherwise a ray cast (radius unused, the arithmetic of the ray cast unchanged).
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
    RayHit best;
    best.t = __builtin_inff(); best.id = kRayMiss; best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f;
    uint32_t cells = 0, cands = 0;
    const v3 o = ld3(origin, r), d = ld3(dir, r);
    const float tmax = max_t ? max_t[r] : __builtin_inff();
    const uint32_t ign = ignore_body && ignore_body[r] < n_bodies ? ignore_body[r] : 0xFFFFFFFFu;
    const float len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    const float sum = ((o.x + o.y) + (o.z + d.x)) + (d.y + d.z);
    const float rad = SWEEP ? radius[r] : 0.0f;
    const bool rad_ok = !SWEEP || (rad >= 0.0f && rad <= 3.4e38f);  // a negative, NaN or infinite radius misses
    // the capsule's core: half-length hq along a, the y axis of rot (used as given); a bad half-length or rot misses
    float hq = 0.0f, ax = 0.0f, ay = 1.0f, az = 0.0f;
    bool cap_ok = true, best_st = false;
    uint32_t best_k = 0;
    v3 point = v3_make(0.0f, 0.0f, 0.0f);
    if constexpr (CAPS) {
        hq = ca.half_length[r];
        cap_ok = hq >= 0.0f && hq <= 3.4e38f;
        if (ca.rot) {
            const float4 q4 = make_float4(ca.rot[4 * (size_t)r], ca.rot[4 * (size_t)r + 1], ca.rot[4 * (size_t)r + 2], ca.rot[4 * (size_t)r + 3]);
            cap_ok = cap_ok && isfinite(q4.x) && isfinite(q4.y) && isfinite(q4.z) && isfinite(q4.w);
            rc_capsule_axis(q4, ax, ay, az);
        }
    }
    if (len > 0.0f && len <= 3.0e38f && isfinite(sum) && tmax >= 0.0f && rad_ok && cap_ok) {
        const float ux = d.x / len, uy = d.y / len, uz = d.z / len;
        // the ground: the solid half-space y <= ground_y (for a ball: its centre reaches y = ground_y + rad; for a capsule:
        // its lowest point, hq |a.y| + rad below the centre)
        float gy = SWEEP ? ground_y + rad : ground_y;
        if (CAPS && hq > 0.0f) gy = ground_y + (rad + hq * fabsf(ay));
        if (ground && (!FILT || (qf.ground & qm) != 0u)) {
            float tg = -1.0f;
            if (o.y <= gy) { tg = 0.0f; best.nx = -ux; best.ny = -uy; best.nz = -uz; }
            else if (uy < 0.0f) { tg = (gy - o.y) / uy; best.nx = 0.0f; best.ny = 1.0f; best.nz = 0.0f; }
            if (tg >= 0.0f && tg <= tmax) { best.t = tg; best.id = kRayGround; }
            else { best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f; }
        }
        // static colliders (records of phys_set_static_bodies, id PHYS_STATIC_ID_BIT | k): every one tested, before the bodies'
        // walk so that a static hit shortens it; bodies still win exact ties (smaller ids), the ground loses them
        for (uint32_t k = 0; k < n_static; ++k) {
            if (FILT && (qf.st[k].x & qm) == 0u) continue;
            if (CAPS && hq > 0.0f) cc_test(st_rec, k, true, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, tmax, 0xFFFFFFFFu, best, best_k, best_st);
            else if (SWEEP) sc_test(st_rec, k, o.x, o.y, o.z, ux, uy, uz, rad, tmax, 0xFFFFFFFFu, best);
            else rc_test(st_rec, k, o.x, o.y, o.z, ux, uy, uz, tmax, 0xFFFFFFFFu, best);
        }
        const RcGrid g = rc_grid(hdr);
        // clip to the grid box and to [0, min(max_t, best)] (bodies win ties with the ground: best.t itself stays in)
        const float iux = 1.0f / ux, iuy = 1.0f / uy, iuz = 1.0f / uz;  // +-inf on a zero component
        const float hx = g.lox + (float)g.nx * g.cell, hy = g.loy + (float)g.ny * g.cell, hz = g.loz + (float)g.nz * g.cell;
        float t0 = 0.0f, t1 = fminf(tmax, best.t);
        bool hit_box = g.valid;
        if (ux == 0.0f) hit_box = hit_box && o.x >= g.lox && o.x <= hx;
        else { const float a = (g.lox - o.x) * iux, b = (hx - o.x) * iux; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (uy == 0.0f) hit_box = hit_box && o.y >= g.loy && o.y <= hy;
        else { const float a = (g.loy - o.y) * iuy, b = (hy - o.y) * iuy; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (uz == 0.0f) hit_box = hit_box && o.z >= g.loz && o.z <= hz;
        else { const float a = (g.loz - o.z) * iuz, b = (hz - o.z) * iuz; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (hit_box && t0 <= t1) {
            const float tlim = fminf(tmax, best.t);
            int ix = rc_coord(o.x + t0 * ux, g.lox, g.inv, g.nx);
            int iy = rc_coord(o.y + t0 * uy, g.loy, g.inv, g.ny);
            int iz = rc_coord(o.z + t0 * uz, g.loz, g.inv, g.nz);
            const bool upx = ux > 0.0f, upy = uy > 0.0f, upz = uz > 0.0f;
            const int sx = upx ? 1 : (ux < 0.0f ? -1 : 0), sy = upy ? 1 : (uy < 0.0f ? -1 : 0), sz = upz ? 1 : (uz < 0.0f ? -1 : 0);
            const float inf = __builtin_inff();
            float tx = sx ? rc_plane_t(ix, upx, g.lox, g.cell, o.x, iux) : inf;
            float ty = sy ? rc_plane_t(iy, upy, g.loy, g.cell, o.y, iuy) : inf;
            float tz = sz ? rc_plane_t(iz, upz, g.loz, g.cell, o.z, iuz) : inf;
            // a walk never takes more steps than the grid has cells along the three axes (also bounds a NaN walk)
            for (int steps = g.nx + g.ny + g.nz + 3; steps > 0; --steps) {
                const float texit = fminf(tx, fminf(ty, tz));
                const uint32_t bk = rc_bucket(ix, iy, iz, bits);
                const uint32_t b0 = start[bk], b1 = start[bk + 1];
                if (STATS) { cells += 1; cands += b1 - b0; }
                for (uint32_t k = b0; k < b1; ++k) {
                    if (FILT && (qf.body[__float_as_uint(rec[3 * (size_t)k + 2].w)].x & qm) == 0u) continue;
                    if (CAPS && hq > 0.0f) cc_test(rec, k, false, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, tlim, ign, best, best_k, best_st);
                    else if (SWEEP) sc_test(rec, k, o.x, o.y, o.z, ux, uy, uz, rad, tlim, ign, best);
                    else rc_test(rec, k, o.x, o.y, o.z, ux, uy, uz, tlim, ign, best);
                }
                if (best.t <= texit || texit > t1) break;
                const bool ax = tx <= ty && tx <= tz, ay = !ax && ty <= tz, az = !ax && !ay;
                ix += ax ? sx : 0; iy += ay ? sy : 0; iz += az ? sz : 0;
                if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) break;
                tx = ax ? rc_plane_t(ix, upx, g.lox, g.cell, o.x, iux) : tx;
                ty = ay ? rc_plane_t(iy, upy, g.loy, g.cell, o.y, iuy) : ty;
                tz = az ? rc_plane_t(iz, upz, g.loz, g.cell, o.z, iuz) : tz;
            }
        }
        if constexpr (CAPS) {
            // the contact, once per query: the touched point and, for a capsule, the normal from the closest points at t
            if (best.id == kRayGround && best.t > 0.0f) {
                // the lower end of the core (the centre for a level one) at t, projected onto the plane
                const float e = ay > 0.0f ? -hq : (ay < 0.0f ? hq : 0.0f);
                point = v3_make((o.x + best.t * ux) + e * ax, ground_y, (o.z + best.t * uz) + e * az);
            } else if (best.id != kRayMiss && best.t > 0.0f) {
                if (hq > 0.0f) cc_contact(best_st ? st_rec : rec, best_k, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, best.t, best.nx, best.ny, best.nz, point);
                else point = v3_make(o.x + (best.t * ux - rad * best.nx), o.y + (best.t * uy - rad * best.ny), o.z + (best.t * uz - rad * best.nz));
            }
        }
    }
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

unsigned rc_blocks(uint64_t n) { return (unsigned)((n + kRcThreads - 1) / kRcThreads); }

int32_t launch_query_grid(phys_world* w, const float* grow_radius, const float* grow_half_length, uint64_t n_grow, uint32_t* bits_out) {
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
int32_t launch_cast(phys_world* w, CastKind kind, const CastBatch& b) {
    hipStream_t s = w->stream;
    const uint64_t n = w->n_owned;
    const bool sweep = kind != CastKind::Ray, capsule = kind == CastKind::Capsule;
    const float* radius = sweep ? b.radius : nullptr;
    const CapsuleArgs caps{b.rot, b.half_length, b.point_out};
    uint32_t bits = 12;
    PHYS_TRY(launch_query_grid(w, radius, capsule ? b.half_length : nullptr, sweep ? b.n : 0, &bits));
    const RcHeader* hdr = reinterpret_cast<const RcHeader*>(w->rc_header.p);
    const bool stats = debug_switches().raycast_stats;
    if (stats) {
        PHYS_HIP_TRY(w->rc_stats.resize(2));
        PHYS_HIP_TRY(hipMemsetAsync(w->rc_stats.p, 0, 16, s));
    }
    const int ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? 1 : 0;
    const QueryFilters qf = query_filters(w, b.query_mask);
#define PHYS_RC_LAUNCH(SW, FILT, ...)                                                                                        \
    hipLaunchKernelGGL((k_rc_trace<kSt, SW, FILT>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, s, (uint32_t)b.n, b.origin, b.dir,   \
                       radius, b.max_t, b.ignore_body, hdr, bits, (const uint32_t*)w->rc_start.p,                                  \
                       reinterpret_cast<const float4*>(w->rc_records.p), (uint32_t)n, ground, w->cfg.ground_height,               \
                       reinterpret_cast<const float4*>(w->st_rc.p), (uint32_t)w->n_static, b.body_out, b.t_out, b.normal_out,     \
                       w->rc_stats.p, ##__VA_ARGS__)
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
