// raycast.hip — batched ray casts against the current poses (phys_raycast / phys_raycast_device).
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
#include <cstdio>

#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kRcThreads = 256;
constexpr int kRcScanItems = 16;                              // per thread of the scan kernels
constexpr uint32_t kRcScanTile = kRcThreads * kRcScanItems;   // 4096 buckets per workgroup; the table is a multiple of it
constexpr int kRcMaxBoundsBlocks = 1024;
constexpr uint32_t kRcMaxCellsPerAxis = 1u << 20;
constexpr uint32_t kRayMiss = PHYS_RAY_MISS, kRayGround = PHYS_RAY_GROUND;

// k_rc_bounds' result: order-preserving keys (0 = nothing seen, which no finite float maps to); the low corner as the
// key of -x so that every slot is a max and one memset to zero resets them all
struct RcHeader {
    uint32_t neg_lo[3];
    uint32_t hi[3];
    uint32_t edge;
    uint32_t pad;
};

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the grid every kernel derives from the header (same arithmetic everywhere, so insertion and walk agree on every cell)
struct RcGrid {
    float lox, loy, loz;  // grid origin = scene bounds - pad
    float cell, inv, pad;
    int nx, ny, nz;       // cells per axis
    bool valid;           // some owned body has a shape
};

__device__ __forceinline__ int rc_dim(float span, float inv) {
    float c = floorf(span * inv) + 1.0f;
    c = c < 1.0f ? 1.0f : (c > (float)kRcMaxCellsPerAxis + 1.0f ? (float)kRcMaxCellsPerAxis + 1.0f : c);
    return (int)c;
}

__device__ __forceinline__ RcGrid rc_grid(const RcHeader* __restrict__ h) {
    RcGrid g;
    g.valid = h->hi[0] != 0u;
    const float lx = -key2f(h->neg_lo[0]), ly = -key2f(h->neg_lo[1]), lz = -key2f(h->neg_lo[2]);
    const float hx = key2f(h->hi[0]), hy = key2f(h->hi[1]), hz = key2f(h->hi[2]);
    const float e = g.valid ? key2f(h->edge) : 0.0f;
    float m = fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fmaxf(fabsf(ly), fabsf(hy)), fmaxf(fabsf(lz), fabsf(hz))));
    if (!g.valid) m = 0.0f;
    // pad: float rounding of an AABB, of a cell coordinate and of the walk's plane crossings is a few ulp of the scene's
    // coordinates; 2^-16 of them is hundreds of ulp. The cell exceeds the padded edge, so a body touches <= 2 cells per axis
    g.pad = 0x1p-16f * (m + e);
    g.lox = lx - g.pad; g.loy = ly - g.pad; g.loz = lz - g.pad;
    const float sx = (hx + g.pad) - g.lox, sy = (hy + g.pad) - g.loy, sz = (hz + g.pad) - g.loz;
    float cell = (e + 2.0f * g.pad) * (1.0f + 0x1p-10f);
    const float span = fmaxf(sx, fmaxf(sy, sz));
    if (span * 0x1p-20f > cell) cell = span * 0x1p-20f;  // at most 2^20 cells per axis (far-flung scenes: coarser cells)
    g.cell = fmaxf(cell, 1.0e-30f);
    g.inv = 1.0f / g.cell;
    g.nx = g.valid ? rc_dim(sx, g.inv) : 1;
    g.ny = g.valid ? rc_dim(sy, g.inv) : 1;
    g.nz = g.valid ? rc_dim(sz, g.inv) : 1;
    return g;
}

__device__ __forceinline__ int rc_coord(float x, float lo, float inv, int n) {
    float c = floorf((x - lo) * inv);
    c = c < 0.0f ? 0.0f : (c > (float)(n - 1) ? (float)(n - 1) : c);  // NaN stays NaN -> (int) 0 on gfx950, still in range
    const int i = (int)c;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// multiplicative hash of the cell, top `bits` bits
__device__ __forceinline__ uint32_t rc_bucket(int x, int y, int z, uint32_t bits) {
    const uint32_t h = ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
    return (h * 0x9E3779B1u) >> (32u - bits);
}

__device__ __forceinline__ bool rc_aabb(const float* __restrict__ pos, const float* __restrict__ rot, const float* __restrict__ he,
                                        const uint32_t* __restrict__ shape, uint32_t i, aabb_t* out) {
    const uint32_t type = shape[i];
    if (type != PHYS_SHAPE_SPHERE && type != PHYS_SHAPE_BOX && type != PHYS_SHAPE_CAPSULE) return false;
    const float4 q4 = reinterpret_cast<const float4*>(rot)[i];
    quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
    const aabb_t b = body_aabb(ld3(pos, i), q, ld3(he, i), type, 0.0f);
    // a non-finite pose is never inserted (and so never hit)
    const float s = ((b.lo.x + b.lo.y) + (b.lo.z + b.hi.x)) + (b.hi.y + b.hi.z);
    if (!isfinite(s)) return false;
    *out = b;
    return true;
}

__global__ __launch_bounds__(kRcThreads) void k_rc_bounds(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                         const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                         RcHeader* __restrict__ hdr) {
    float k[7];  // -lo xyz, hi xyz, edge (fully unrolled: registers, not scratch)
#pragma unroll
    for (int a = 0; a < 7; ++a) k[a] = -3.0e38f;
    bool any = false;
    for (uint32_t i = blockIdx.x * kRcThreads + threadIdx.x; i < n; i += gridDim.x * kRcThreads) {
        aabb_t b;
        if (!rc_aabb(pos, rot, he, shape, i, &b)) continue;
        any = true;
        k[0] = fmaxf(k[0], -b.lo.x); k[1] = fmaxf(k[1], -b.lo.y); k[2] = fmaxf(k[2], -b.lo.z);
        k[3] = fmaxf(k[3], b.hi.x); k[4] = fmaxf(k[4], b.hi.y); k[5] = fmaxf(k[5], b.hi.z);
        k[6] = fmaxf(k[6], fmaxf(b.hi.x - b.lo.x, fmaxf(b.hi.y - b.lo.y, b.hi.z - b.lo.z)));
    }
    __shared__ float red[kRcThreads / 64][7];
    __shared__ int any_wave[kRcThreads / 64];
#pragma unroll
    for (int a = 0; a < 7; ++a)
        for (int off = 32; off > 0; off >>= 1) k[a] = fmaxf(k[a], __shfl_xor(k[a], off));
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
    const int x0 = rc_coord(b.lo.x - g.pad, g.lox, g.inv, g.nx), x1 = min(rc_coord(b.hi.x + g.pad, g.lox, g.inv, g.nx), x0 + 1);
    const int y0 = rc_coord(b.lo.y - g.pad, g.loy, g.inv, g.ny), y1 = min(rc_coord(b.hi.y + g.pad, g.loy, g.inv, g.ny), y0 + 1);
    const int z0 = rc_coord(b.lo.z - g.pad, g.loz, g.inv, g.nz), z1 = min(rc_coord(b.hi.z + g.pad, g.loz, g.inv, g.nz), z0 + 1);
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

// exclusive scan over 4096-bucket tiles: tile sums, one workgroup scans the tile sums, tiles scanned with their offsets
__device__ __forceinline__ uint32_t rc_block_exclusive(uint32_t v, uint32_t* total) {
    __shared__ uint32_t s[kRcThreads];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kRcThreads; off <<= 1) {
        const uint32_t add = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0u;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t incl = s[threadIdx.x];
    *total = s[kRcThreads - 1];
    __syncthreads();
    return incl - v;
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
    uint32_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += kRcThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_sum[i] : 0u;
        uint32_t total;
        const uint32_t ex = rc_block_exclusive(v, &total);
        if (i < tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[tiles] = carry;
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

struct RayHit {
    float t;
    uint32_t id;
    float nx, ny, nz;
};

__device__ __forceinline__ bool rc_better(float t, uint32_t id, const RayHit& b) { return t < b.t || (t == b.t && id < b.id); }

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
        const float r = c.x;
        const float bb = (px * ux + py * uy) + pz * uz;
        const float cc = ((px * px + py * py) + pz * pz) - r * r;
        if (cc <= 0.0f) {  // origin inside the closed ball
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            if (bb >= 0.0f) return;  // outside and moving away
            // distance of the line from the centre without cancellation: |p - (p.u) u|^2
            const float lx = px - bb * ux, ly = py - bb * uy, lz = pz - bb * uz;
            const float disc = r * r - ((lx * lx + ly * ly) + lz * lz);
            if (disc < 0.0f) return;
            const float q = -bb + sqrtf(disc);  // the far root (> 0); the near one is cc / q (no cancellation)
            t = cc / q;
            const float hx = px + t * ux, hy = py + t * uy, hz = pz + t * uz;
            const float inv = 1.0f / sqrtf((hx * hx + hy * hy) + hz * hz);
            nx = hx * inv; ny = hy * inv; nz = hz * inv;
        }
    } else if (__float_as_uint(a.w) == PHYS_SHAPE_CAPSULE) {
        // radius c.x, core c +- c.y * w, w = column 1 of R: the finite cylinder's side, then the two end balls; the first hit
        // of the union is the least of their first hits (a ray that enters through a flat end of the cylinder has hit the
        // ball there already)
        const float4 q4 = rec[3 * (size_t)k + 1];
        const float qi = q4.x, qj = q4.y, qk = q4.z, qw = q4.w;
        const float wx = (qi * qj * 2.0f) - (qw * qk * 2.0f);            // R.m[1] of quat_to_m33
        const float wy = (((qw * qw) - (qi * qi)) + (qj * qj)) - (qk * qk);  // R.m[4]
        const float wz = (qw * qi * 2.0f) + (qj * qk * 2.0f);            // R.m[7]
        const float r = c.x, hl = c.y, rr = r * r;
        const float pd = (px * wx + py * wy) + pz * wz;
        const float sp = fminf(fmaxf(pd, -hl), hl);
        const float qx = px - sp * wx, qy = py - sp * wy, qz = pz - sp * wz;
        if ((qx * qx + qy * qy) + qz * qz <= rr) {  // origin inside the closed capsule
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            t = __builtin_inff();
            // side: the components of p and u across the axis
            const float ud = (ux * wx + uy * wy) + uz * wz;
            const float ax = ux - ud * wx, ay = uy - ud * wy, az = uz - ud * wz;
            const float bx = px - pd * wx, by = py - pd * wy, bz = pz - pd * wz;
            const float A = (ax * ax + ay * ay) + az * az;
            const float B = (ax * bx + ay * by) + az * bz;
            const float C = ((bx * bx + by * by) + bz * bz) - rr;
            if (A > 1.0e-12f && B < 0.0f) {
                const float disc = B * B - A * C;
                if (disc >= 0.0f) {
                    const float q = -B + sqrtf(disc);  // > 0; the near root is C / q (no cancellation)
                    const float tc = C / q;
                    if (tc >= 0.0f && fabsf(pd + tc * ud) <= hl) t = tc;
                }
            }
            // end balls at -hl w and +hl w (the existing ray-ball test of the sphere branch)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float s = e == 0 ? -hl : hl;
                const float ex = px - s * wx, ey = py - s * wy, ez = pz - s * wz;
                const float bb = (ex * ux + ey * uy) + ez * uz;
                const float cc = ((ex * ex + ey * ey) + ez * ez) - rr;
                if (bb < 0.0f) {
                    const float lx = ex - bb * ux, ly = ey - bb * uy, lz = ez - bb * uz;
                    const float disc = rr - ((lx * lx + ly * ly) + lz * lz);
                    if (disc >= 0.0f) t = fminf(t, cc / (-bb + sqrtf(disc)));
                }
            }
            if (!(t < __builtin_inff())) return;  // missed
            // normal: from the closest point of the core to the hit
            const float hx = px + t * ux, hy = py + t * uy, hz = pz + t * uz;
            const float sh = fminf(fmaxf((hx * wx + hy * wy) + hz * wz, -hl), hl);
            const float dx = hx - sh * wx, dy = hy - sh * wy, dz = hz - sh * wz;
            const float inv = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);
            nx = dx * inv; ny = dy * inv; nz = dz * inv;
        }
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
        if (fabsf(lx) <= c.x && fabsf(ly) <= c.y && fabsf(lz) <= c.z) {  // origin inside the closed box
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            // slabs; an axis the ray is parallel to either always holds the ray (|l| <= h) or never (the box is missed)
            const bool px0 = dx == 0.0f, py0 = dy == 0.0f, pz0 = dz == 0.0f;
            if ((px0 && fabsf(lx) > c.x) || (py0 && fabsf(ly) > c.y) || (pz0 && fabsf(lz) > c.z)) return;
            const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
            // entering face of each slab: the one facing the ray (-sign(d) h)
            const float ex = px0 ? -3.0e38f : (dx > 0.0f ? (-c.x - lx) : (c.x - lx)) * ix;
            const float fx = px0 ? 3.0e38f : (dx > 0.0f ? (c.x - lx) : (-c.x - lx)) * ix;
            const float ey = py0 ? -3.0e38f : (dy > 0.0f ? (-c.y - ly) : (c.y - ly)) * iy;
            const float fy = py0 ? 3.0e38f : (dy > 0.0f ? (c.y - ly) : (-c.y - ly)) * iy;
            const float ez = pz0 ? -3.0e38f : (dz > 0.0f ? (-c.z - lz) : (c.z - lz)) * iz;
            const float fz = pz0 ? 3.0e38f : (dz > 0.0f ? (c.z - lz) : (-c.z - lz)) * iz;
            const float tn = fmaxf(ex, fmaxf(ey, ez));
            const float tf = fminf(fx, fminf(fy, fz));
            if (!(tn <= tf) || tf < 0.0f || tn < 0.0f) return;
            t = tn;
            // local normal of the entering slab (ties: x, then y, then z), then into the world frame
            const bool ax = ex == tn, ay = !ax && ey == tn, az = !ax && !ay;
            const float sx = ax ? (dx > 0.0f ? -1.0f : 1.0f) : 0.0f;
            const float sy = ay ? (dy > 0.0f ? -1.0f : 1.0f) : 0.0f;
            const float sz = az ? (dz > 0.0f ? -1.0f : 1.0f) : 0.0f;
            nx = (R.m[0] * sx + R.m[1] * sy) + R.m[2] * sz;
            ny = (R.m[3] * sx + R.m[4] * sy) + R.m[5] * sz;
            nz = (R.m[6] * sx + R.m[7] * sy) + R.m[8] * sz;
            const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);  // R of a nearly-unit quaternion
            nx *= inv; ny *= inv; nz *= inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) { best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz; }
}

__device__ __forceinline__ float rc_plane_t(int i, bool up, float lo, float cell, float o, float inv_u) {
    return ((lo + (float)(i + (up ? 1 : 0)) * cell) - o) * inv_u;
}

template <bool STATS>
__global__ __launch_bounds__(kRcThreads) void k_rc_trace(uint32_t n_rays, const float* __restrict__ origin, const float* __restrict__ dir,
                                                        const float* __restrict__ max_t, const uint32_t* __restrict__ ignore_body,
                                                        const RcHeader* __restrict__ hdr, uint32_t bits, const uint32_t* __restrict__ start,
                                                        const float4* __restrict__ rec, uint32_t n_bodies, int ground, float ground_y,
                                                        const float4* __restrict__ st_rec, uint32_t n_static,
                                                        uint32_t* __restrict__ body_out, float* __restrict__ t_out, float* __restrict__ normal_out,
                                                        unsigned long long* __restrict__ stats) {
    const uint32_t r = blockIdx.x * kRcThreads + threadIdx.x;
    if (r >= n_rays) return;
    RayHit best;
    best.t = __builtin_inff(); best.id = kRayMiss; best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f;
    uint32_t cells = 0, cands = 0;
    const v3 o = ld3(origin, r), d = ld3(dir, r);
    const float tmax = max_t ? max_t[r] : __builtin_inff();
    const uint32_t ign = ignore_body && ignore_body[r] < n_bodies ? ignore_body[r] : 0xFFFFFFFFu;
    const float len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    const float sum = ((o.x + o.y) + (o.z + d.x)) + (d.y + d.z);
    if (len > 0.0f && len <= 3.0e38f && isfinite(sum) && tmax >= 0.0f) {
        const float ux = d.x / len, uy = d.y / len, uz = d.z / len;
        // the ground: the solid half-space y <= ground_y
        if (ground) {
            float tg = -1.0f;
            if (o.y <= ground_y) { tg = 0.0f; best.nx = -ux; best.ny = -uy; best.nz = -uz; }
            else if (uy < 0.0f) { tg = (ground_y - o.y) / uy; best.nx = 0.0f; best.ny = 1.0f; best.nz = 0.0f; }
            if (tg >= 0.0f && tg <= tmax) { best.t = tg; best.id = kRayGround; }
            else { best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f; }
        }
        // static colliders (records of phys_set_static_bodies, id PHYS_STATIC_ID_BIT | k): every one tested, before the bodies'
        // walk so that a static hit shortens it; bodies still win exact ties (smaller ids), the ground loses them
        for (uint32_t k = 0; k < n_static; ++k) rc_test(st_rec, k, o.x, o.y, o.z, ux, uy, uz, tmax, 0xFFFFFFFFu, best);
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
                for (uint32_t k = b0; k < b1; ++k) rc_test(rec, k, o.x, o.y, o.z, ux, uy, uz, tlim, ign, best);
                if (best.t <= texit || texit > t1) break;
                const bool ax = tx <= ty && tx <= tz, ay = !ax && ty <= tz, az = !ax && !ay;
                ix += ax ? sx : 0; iy += ay ? sy : 0; iz += az ? sz : 0;
                if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) break;
                tx = ax ? rc_plane_t(ix, upx, g.lox, g.cell, o.x, iux) : tx;
                ty = ay ? rc_plane_t(iy, upy, g.loy, g.cell, o.y, iuy) : ty;
                tz = az ? rc_plane_t(iz, upz, g.loz, g.cell, o.z, iuz) : tz;
            }
        }
    }
    body_out[r] = best.id;
    t_out[r] = best.t;
    if (normal_out) st3(normal_out, r, v3_make(best.nx, best.ny, best.nz));
    if (STATS) { atomicAdd(&stats[0], (unsigned long long)cells); atomicAdd(&stats[1], (unsigned long long)cands); }
}

}  // namespace

unsigned rc_blocks(uint64_t n) { return (unsigned)((n + kRcThreads - 1) / kRcThreads); }

int32_t launch_raycast(phys_world* w, uint64_t n_rays, const float* origin, const float* dir, const float* max_t,
                       const uint32_t* ignore_body, uint32_t* body_out, float* t_out, float* normal_out) {
    hipStream_t s = w->stream;
    const uint64_t n = w->n_owned;
    PHYS_HIP_TRY(w->rc_header.resize(sizeof(RcHeader) / 4));
    PHYS_HIP_TRY(hipMemsetAsync(w->rc_header.p, 0, sizeof(RcHeader), s));
    const RcHeader* hdr = reinterpret_cast<const RcHeader*>(w->rc_header.p);
    uint32_t bits = 12;
    if (n > (1ull << 29)) { set_error("phys_raycast: more than 2^29 bodies (the query's grid indexes insertions with 32 bits)"); return PHYS_ERR_UNSUPPORTED; }
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
    const bool stats = debug_switches().raycast_stats;
    if (stats) {
        PHYS_HIP_TRY(w->rc_stats.resize(2));
        PHYS_HIP_TRY(hipMemsetAsync(w->rc_stats.p, 0, 16, s));
    }
    const int ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? 1 : 0;
#define PHYS_RC_TRACE(S)                                                                                                       \
    hipLaunchKernelGGL(k_rc_trace<S>, dim3(rc_blocks(n_rays)), dim3(kRcThreads), 0, s, (uint32_t)n_rays, origin, dir, max_t,  \
                       ignore_body, hdr, bits, (const uint32_t*)w->rc_start.p, reinterpret_cast<const float4*>(w->rc_records.p), \
                       (uint32_t)n, ground, w->cfg.ground_height, reinterpret_cast<const float4*>(w->st_rc.p), (uint32_t)w->n_static, \
                       body_out, t_out, normal_out, w->rc_stats.p)
    if (stats) PHYS_RC_TRACE(true);
    else PHYS_RC_TRACE(false);
#undef PHYS_RC_TRACE
    PHYS_HIP_TRY(hipGetLastError());
    if (stats) {
        unsigned long long h[2] = {0, 0};
        PHYS_HIP_TRY(hipMemcpyAsync(h, w->rc_stats.p, 16, hipMemcpyDeviceToHost, s));
        PHYS_HIP_TRY(hipStreamSynchronize(s));
        fprintf(stderr, "PHYS_RAYCAST_STATS rays=%llu cells=%llu candidates=%llu\n", (unsigned long long)n_rays, h[0], h[1]);
    }
    return PHYS_OK;
}

}  // namespace phys
