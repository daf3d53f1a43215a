// query.hip — overlap queries against the current poses (phys_overlap): for each query shape, every target whose closed
// shape it intersects, as ascending ids in CSR form. Read-only like the ray casts: it walks the query grid that raycast.hip
// builds (launch_query_grid, not grown) and writes only qr_* buffers of its own.
//
//   launch_query_grid   the ray casts' grid over the exact AABBs
//   k_ov_query<false>   one query per lane: the cells its padded AABB covers (or every body, when it covers more cells than
//                       there are bodies), every static, the ground; counts the targets it intersects
//   (host)              exclusive scan of the counts into offsets_out (u64); PHYS_ERR_CAPACITY when the total exceeds cap
//   k_ov_query<true>    the same walk again, writing each query's ids into its segment (bucket order)
//   k_ov_order          one wave per query: its segment ascending (copied when already ascending; bitonic sort in LDS up
//                       to kOvSortLds ids; rank by counting through LDS tiles above that)
// A bucket can hold a body's records of other cells and, when two of its cells hash to one bucket, two records of the same
// body. A record counts only in the first cell the body shares with the query (componentwise larger low corner of the two
// cell ranges) and only if no earlier record of its bucket names the same body: every id appears once.
#include <vector>

#include "rc_grid.hpp"

namespace phys {

namespace {

constexpr int kOvThreads = 256;
constexpr int kOvSortThreads = 64;       // one wave per query segment
constexpr uint32_t kOvSortLds = 2048;    // ids sorted in LDS (8 KB per wave)
constexpr unsigned kOvMaxSortBlocks = 1u << 16;
constexpr float kSatParallel = 1.0e-6f;  // edge cross axes with |a x b|^2 below this (unit axes) are skipped

// a query or target shape in world space; rotation as the matrix of quat_to_m33
struct QShape {
    uint32_t type;
    v3 c, h;
    m33 R;
};

__device__ __forceinline__ QShape qs_make(uint32_t type, v3 c, float4 q4, v3 h) {
    QShape s;
    s.type = type; s.c = c; s.h = h;
    quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
    quat_to_m33(q, &s.R);
    return s;
}

// the core of a sphere (a point) or capsule (a segment c +- hl * w) and its radius
__device__ __forceinline__ void qs_core(const QShape& s, v3* w, float* hl, float* r) {
    const bool cap = s.type == PHYS_SHAPE_CAPSULE;
    *w = cap ? v3_make(s.R.m[1], s.R.m[4], s.R.m[7]) : v3_make(0.0f, 1.0f, 0.0f);
    *hl = cap ? s.h.y : 0.0f;
    *r = s.h.x;
}

// squared distance from p to the segment c +- hl * w
__device__ __forceinline__ float qr_point_seg_d2(v3 p, v3 c, v3 w, float hl) {
    const float s = segment_param(c, w, hl, p);
    const v3 d = v3_sub(p, v3_add(c, v3_scale(w, s)));
    return v3_dot(d, d);
}

// squared distance of the segments ca +- ha * ua and cb +- hb * ub, exact for parallel ones too: the least of the four
// end-point distances and, when the lines cross at parameters inside both segments, the distance there (otherwise the
// minimum lies at an end point of one of them)
__device__ __forceinline__ float qr_seg_seg_d2(v3 ca, v3 ua, float ha, v3 cb, v3 ub, float hb) {
    float d2 = fminf(fminf(qr_point_seg_d2(v3_add(ca, v3_scale(ua, ha)), cb, ub, hb), qr_point_seg_d2(v3_sub(ca, v3_scale(ua, ha)), cb, ub, hb)),
                     fminf(qr_point_seg_d2(v3_add(cb, v3_scale(ub, hb)), ca, ua, ha), qr_point_seg_d2(v3_sub(cb, v3_scale(ub, hb)), ca, ua, ha)));
    const v3 r = v3_sub(ca, cb);
    const float a = v3_dot(ua, ua), e = v3_dot(ub, ub), b = v3_dot(ua, ub);
    const float c = v3_dot(ua, r), f = v3_dot(ub, r);
    const float den = a * e - b * b;
    if (den > 1.0e-12f * (a * e)) {
        const float s = (b * f - c * e) / den, t = (a * f - b * c) / den;
        if (fabsf(s) <= ha && fabsf(t) <= hb) {
            const v3 d = v3_sub(v3_add(ca, v3_scale(ua, s)), v3_add(cb, v3_scale(ub, t)));
            d2 = fminf(d2, v3_dot(d, d));
        }
    }
    return d2;
}

// a sphere or capsule S against a box B: the core segment in B's frame; 0 if it crosses the box (slab test), otherwise the
// least of its end points' distances to the box and its distances to the box's 12 edges (exact for a segment against a
// convex box), compared with the radius
__device__ __forceinline__ bool qr_round_box(const QShape& S, const QShape& B) {
    v3 w; float hl, r;
    qs_core(S, &w, &hl, &r);
    const v3 p = m33_tmul_v3(&B.R, v3_sub(S.c, B.c));
    const v3 d = m33_tmul_v3(&B.R, w);
    const v3 h = B.h;
    // slabs over the segment's parameter range [-hl, hl]
    float lo = -hl, hi = hl;
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pa = a == 0 ? p.x : (a == 1 ? p.y : p.z);
        const float da = a == 0 ? d.x : (a == 1 ? d.y : d.z);
        const float ha = a == 0 ? h.x : (a == 1 ? h.y : h.z);
        if (da == 0.0f) {
            miss = miss || fabsf(pa) > ha;
        } else {
            const float t0 = (-ha - pa) / da, t1 = (ha - pa) / da;
            lo = fmaxf(lo, fminf(t0, t1));
            hi = fminf(hi, fmaxf(t0, t1));
        }
    }
    if (!miss && lo <= hi) return true;
    float d2 = 3.0e38f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const v3 q = v3_add(p, v3_scale(d, k == 0 ? -hl : hl));
        const float gx = fmaxf(fabsf(q.x) - h.x, 0.0f), gy = fmaxf(fabsf(q.y) - h.y, 0.0f), gz = fmaxf(fabsf(q.z) - h.z, 0.0f);
        d2 = fminf(d2, (gx * gx + gy * gy) + gz * gz);
    }
    if (hl > 0.0f) {
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            // edge e along axis e / 4, at the corner signs of bits 0 and 1 of e on the other two axes
            const int ax = e >> 2;
            const float s1 = (e & 1) ? 1.0f : -1.0f, s2 = (e & 2) ? 1.0f : -1.0f;
            const v3 ec = v3_make(ax == 0 ? 0.0f : s1 * h.x, ax == 1 ? 0.0f : (ax == 0 ? s1 : s2) * h.y, ax == 2 ? 0.0f : s2 * h.z);
            const v3 eu = v3_make(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f);
            const float eh = ax == 0 ? h.x : (ax == 1 ? h.y : h.z);
            d2 = fminf(d2, qr_seg_seg_d2(p, d, hl, ec, eu, eh));
        }
    }
    return d2 <= r * r;
}

// box against box: separating axes over the 6 face normals and the 9 edge cross products (near-parallel ones skipped: the
// face axes cover them). Touching (|t.L| == ra + rb) counts as overlapping.
__device__ __forceinline__ bool qr_box_box(const QShape& A, const QShape& B) {
    float C[3][3], Cb[3][3];  // C[i][j] = A_i . B_j (indices are compile-time after unrolling: registers)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            C[i][j] = (A.R.m[i] * B.R.m[j] + A.R.m[3 + i] * B.R.m[3 + j]) + A.R.m[6 + i] * B.R.m[6 + j];
            Cb[i][j] = fabsf(C[i][j]);
        }
    const v3 tw = m33_tmul_v3(&A.R, v3_sub(B.c, A.c));
    const float t[3] = {tw.x, tw.y, tw.z};
    const float ha[3] = {A.h.x, A.h.y, A.h.z}, hb[3] = {B.h.x, B.h.y, B.h.z};
    bool sep = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // A's faces
        const float rb = (hb[0] * Cb[i][0] + hb[1] * Cb[i][1]) + hb[2] * Cb[i][2];
        sep = sep || fabsf(t[i]) > ha[i] + rb;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // B's faces
        const float ra = (ha[0] * Cb[0][j] + ha[1] * Cb[1][j]) + ha[2] * Cb[2][j];
        const float tj = (t[0] * C[0][j] + t[1] * C[1][j]) + t[2] * C[2][j];
        sep = sep || fabsf(tj) > ra + hb[j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // A_i x B_j
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            if (1.0f - C[i][j] * C[i][j] < kSatParallel) continue;
            const float ra = ha[i1] * Cb[i2][j] + ha[i2] * Cb[i1][j];
            const float rb = hb[j1] * Cb[i][j2] + hb[j2] * Cb[i][j1];
            sep = sep || fabsf(t[i2] * C[i1][j] - t[i1] * C[i2][j]) > ra + rb;
        }
    return !sep;
}

// the closed query shape Q against the closed target T
__device__ __forceinline__ bool qr_overlap(const QShape& Q, const QShape& T) {
    const bool qb = Q.type == PHYS_SHAPE_BOX, tb = T.type == PHYS_SHAPE_BOX;
    if (qb && tb) return qr_box_box(Q, T);
    if (!qb && !tb) {
        v3 wq, wt; float hq, ht, rq, rt;
        qs_core(Q, &wq, &hq, &rq);
        qs_core(T, &wt, &ht, &rt);
        const float rr = rq + rt;
        return qr_seg_seg_d2(Q.c, wq, hq, T.c, wt, ht) <= rr * rr;
    }
    return qb ? qr_round_box(T, Q) : qr_round_box(Q, T);
}

__device__ __forceinline__ bool aabb_touch(const aabb_t& a, const aabb_t& b) {
    return a.lo.x <= b.hi.x && b.lo.x <= a.hi.x && a.lo.y <= b.hi.y && b.lo.y <= a.hi.y && a.lo.z <= b.hi.z && b.lo.z <= a.hi.z;
}

// FILL = false: count[q] = the number of targets query q intersects. FILL = true: their ids into ids[offsets[q] ...]
// FILT: phys_overlap_filtered (one QueryFilters argument, the pack `filt`): a target whose category misses the query's mask
// is skipped before its exact test; without it the pack is empty and the kernel is the one it was before filters
template <bool FILL, bool FILT, typename... Filt>
__global__ __launch_bounds__(kOvThreads) void k_ov_query(uint32_t nq, const uint32_t* __restrict__ qtype, const float* __restrict__ qpos,
                                                        const float* __restrict__ qrot, const float* __restrict__ qhe,
                                                        const uint32_t* __restrict__ ignore_body, const RcHeader* __restrict__ hdr,
                                                        uint32_t bits, const uint32_t* __restrict__ start, const float4* __restrict__ rec,
                                                        uint32_t n_bodies, const float* __restrict__ pos, const float* __restrict__ rot,
                                                        const float* __restrict__ he, const uint32_t* __restrict__ shape, int ground,
                                                        float ground_y, const float4* __restrict__ st_rec, uint32_t n_static,
                                                        uint32_t* __restrict__ count, const unsigned long long* __restrict__ offsets,
                                                        uint32_t* __restrict__ ids, Filt... filt) {
    static_assert(sizeof...(Filt) == (FILT ? 1u : 0u), "one QueryFilters argument exactly in the filtered instance");
    const uint32_t q = blockIdx.x * kOvThreads + threadIdx.x;
    if (q >= nq) return;
    QueryFilters qf{};
    if constexpr (FILT) qf = filter_arg(filt...);
    const uint32_t qm = FILT ? (uint32_t)qf.query_mask[q] : 0xFFFFu;
    uint32_t cnt = 0;
    const unsigned long long base = FILL ? offsets[q] : 0ull;
    const uint32_t room = FILL ? (uint32_t)(offsets[q + 1] - base) : 0u;
    auto emit = [&](uint32_t id) {
        if (FILL && cnt < room) ids[base + cnt] = id;
        ++cnt;
    };
    const uint32_t type = qtype[q];
    const v3 c = ld3(qpos, q), h = ld3(qhe, q);
    const float4 q4 = qrot ? reinterpret_cast<const float4*>(qrot)[q] : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    const uint32_t ign = ignore_body && ignore_body[q] < n_bodies ? ignore_body[q] : 0xFFFFFFFFu;
    const float sum = ((c.x + c.y) + (c.z + h.x)) + ((h.y + h.z) + ((q4.x + q4.y) + (q4.z + q4.w)));
    aabb_t qa;
    // an invalid query (other shape, non-finite pose, negative extent) intersects nothing
    if (isfinite(sum) && h.x >= 0.0f && h.y >= 0.0f && h.z >= 0.0f && rc_aabb_of(c, q4, h, type, &qa)) {
        const QShape Q = qs_make(type, c, q4, h);
        const RcGrid g = rc_grid(hdr);
        if (g.valid && n_bodies) {
            aabb_t qp;  // padded like the bodies' cells
            qp.lo = v3_make(qa.lo.x - g.pad, qa.lo.y - g.pad, qa.lo.z - g.pad);
            qp.hi = v3_make(qa.hi.x + g.pad, qa.hi.y + g.pad, qa.hi.z + g.pad);
            const int x0 = rc_coord(qp.lo.x, g.lox, g.inv, g.nx), x1 = rc_coord(qp.hi.x, g.lox, g.inv, g.nx);
            const int y0 = rc_coord(qp.lo.y, g.loy, g.inv, g.ny), y1 = rc_coord(qp.hi.y, g.loy, g.inv, g.ny);
            const int z0 = rc_coord(qp.lo.z, g.loz, g.inv, g.nz), z1 = rc_coord(qp.hi.z, g.loz, g.inv, g.nz);
            const unsigned long long cells = (unsigned long long)(x1 - x0 + 1) * (unsigned long long)(y1 - y0 + 1) *
                                             (unsigned long long)(z1 - z0 + 1);
            if (cells > n_bodies) {
                // more cells than bodies: every owned body directly, in ascending order
                for (uint32_t i = 0; i < n_bodies; ++i) {
                    aabb_t b;
                    if (i == ign || (FILT && (qf.body[i].x & qm) == 0u) || !rc_aabb(pos, rot, he, shape, i, &b) || !aabb_touch(b, qp)) continue;
                    if (qr_overlap(Q, qs_make(shape[i], ld3(pos, i), reinterpret_cast<const float4*>(rot)[i], ld3(he, i)))) emit(i);
                }
            } else {
                for (int z = z0; z <= z1; ++z)
                    for (int y = y0; y <= y1; ++y)
                        for (int x = x0; x <= x1; ++x) {
                            const uint32_t bk = rc_bucket(x, y, z, bits);
                            const uint32_t b0 = start[bk], b1 = start[bk + 1];
                            for (uint32_t k = b0; k < b1; ++k) {
                                const float4 r0 = rec[3 * (size_t)k], r1 = rec[3 * (size_t)k + 1], r2 = rec[3 * (size_t)k + 2];
                                const uint32_t id = __float_as_uint(r2.w);
                                const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
                                aabb_t b;
                                if (id == ign || (FILT && (qf.body[id].x & qm) == 0u) || !rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) ||
                                    !aabb_touch(b, qp))
                                    continue;
                                // only in the first cell the body shares with the query: the record may be another cell's
                                const RcCells bcl = rc_body_cells(g, b);
                                if (x > bcl.x1 || y > bcl.y1 || z > bcl.z1 || max(bcl.x0, x0) != x || max(bcl.y0, y0) != y ||
                                    max(bcl.z0, z0) != z)
                                    continue;
                                // two cells of the body hashed to this bucket: only its first record here counts
                                bool dup = false;
                                for (uint32_t k2 = b0; k2 < k && !dup; ++k2) dup = __float_as_uint(rec[3 * (size_t)k2 + 2].w) == id;
                                if (dup) continue;
                                if (qr_overlap(Q, qs_make(__float_as_uint(r0.w), bc, r1, bh))) emit(id);
                            }
                        }
            }
        }
        // static colliders, ascending (ids PHYS_STATIC_ID_BIT | k above every body id)
        for (uint32_t k = 0; k < n_static; ++k) {
            if (FILT && (qf.st[k].x & qm) == 0u) continue;
            const float4 r0 = st_rec[3 * (size_t)k], r1 = st_rec[3 * (size_t)k + 1], r2 = st_rec[3 * (size_t)k + 2];
            const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
            aabb_t b;
            if (!rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) || !aabb_touch(b, qa)) continue;
            if (qr_overlap(Q, qs_make(__float_as_uint(r0.w), bc, r1, bh))) emit(__float_as_uint(r2.w));
        }
        // the ground half-space y <= ground_y: the query's lowest point is its AABB's low y
        if (ground && (!FILT || (qf.ground & qm) != 0u) && qa.lo.y <= ground_y) emit(kRayGround);
    }
    if (!FILL) count[q] = cnt;
}

// each query's segment of tmp, ascending, into out (ids of a segment are distinct)
__global__ __launch_bounds__(kOvSortThreads) void k_ov_order(uint32_t nq, const unsigned long long* __restrict__ offsets,
                                                            const uint32_t* __restrict__ tmp, uint32_t* __restrict__ out) {
    __shared__ uint32_t s[kOvSortLds];
    const uint32_t lane = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const unsigned long long b = offsets[q];
        const uint32_t len = (uint32_t)(offsets[q + 1] - b);
        bool desc = false;
        for (uint32_t j = lane; j + 1 < len; j += kOvSortThreads) desc = desc || tmp[b + j] > tmp[b + j + 1];
        if (!__any(desc)) {  // already ascending (every direct-path list, the single ids, the statics and the ground)
            for (uint32_t j = lane; j < len; j += kOvSortThreads) out[b + j] = tmp[b + j];
            continue;
        }
        if (len <= kOvSortLds) {
            uint32_t p = 1;
            while (p < len) p <<= 1;
            for (uint32_t j = lane; j < p; j += kOvSortThreads) s[j] = j < len ? tmp[b + j] : 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k = 2; k <= p; k <<= 1)
                for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
                    for (uint32_t i = lane; i < p; i += kOvSortThreads) {
                        const uint32_t l = i ^ jj;
                        if (l > i) {
                            const uint32_t x = s[i], y = s[l];
                            if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t j = lane; j < len; j += kOvSortThreads) out[b + j] = s[j];
            __syncthreads();
        } else {
            // long lists: the rank of an id is the number of ids below it, counted through LDS tiles
            for (uint32_t j0 = 0; j0 < len; j0 += kOvSortThreads) {
                const uint32_t j = j0 + lane;
                const uint32_t x = j < len ? tmp[b + j] : 0u;
                uint32_t rank = 0;
                for (uint32_t t0 = 0; t0 < len; t0 += kOvSortLds) {
                    const uint32_t tl = min(kOvSortLds, len - t0);
                    for (uint32_t m = lane; m < tl; m += kOvSortThreads) s[m] = tmp[b + t0 + m];
                    __syncthreads();
                    for (uint32_t m = 0; m < tl; ++m) rank += s[m] < x ? 1u : 0u;
                    __syncthreads();
                }
                if (j < len && rank < len) out[b + rank] = x;
            }
        }
    }
}

}  // namespace

int32_t launch_overlap(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot, const float* half_extent,
                       const uint32_t* ignore_body, uint64_t cap, uint64_t* offsets_out, uint32_t* ids_out, const uint16_t* query_mask) {
    hipStream_t s = w->stream;
    uint32_t bits = 12;
    int32_t rc = launch_query_grid(w, nullptr, 0, &bits); if (rc) return rc;
    const RcHeader* hdr = reinterpret_cast<const RcHeader*>(w->rc_header.p);
    PHYS_HIP_TRY(w->qr_count.resize(n));
    PHYS_HIP_TRY(w->qr_off.resize(n + 1));
    const unsigned blocks = (unsigned)((n + kOvThreads - 1) / kOvThreads);
    const int ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? 1 : 0;
    const uint32_t nb = (uint32_t)w->n_owned;
    const float4* st = reinterpret_cast<const float4*>(w->st_rc.p);
    const float4* rec = reinterpret_cast<const float4*>(w->rc_records.p);
    QueryFilters qf{};
    qf.query_mask = query_mask;
    qf.body = reinterpret_cast<const uint2*>(w->filt.p);
    qf.st = reinterpret_cast<const uint2*>(w->st_filt.p);
    qf.ground = w->ground_filt & 0xFFFFu;
    // (the filtered instances take `qf` as one more argument; the unfiltered ones are launched exactly as before filters)
#define PHYS_OV_LAUNCH(FILL, FILT, count, offsets, ids, ...)                                                                 \
    hipLaunchKernelGGL((k_ov_query<FILL, FILT>), dim3(blocks), dim3(kOvThreads), 0, s, (uint32_t)n, shape_type, pos, rot, half_extent, \
                       ignore_body, hdr, bits, (const uint32_t*)w->rc_start.p, rec, nb, w->pos.p, w->rot.p, w->half_extent.p,      \
                       w->shape.p, ground, w->cfg.ground_height, st, (uint32_t)w->n_static, count, offsets, ids, ##__VA_ARGS__)
    if (query_mask) PHYS_OV_LAUNCH(false, true, w->qr_count.p, (const unsigned long long*)nullptr, (uint32_t*)nullptr, qf);
    else PHYS_OV_LAUNCH(false, false, w->qr_count.p, (const unsigned long long*)nullptr, (uint32_t*)nullptr);
    PHYS_HIP_TRY(hipGetLastError());
    // exclusive scan on the host: the offsets are an output of the call anyway
    std::vector<uint32_t> cnt((size_t)n);
    PHYS_HIP_TRY(hipMemcpyAsync(cnt.data(), w->qr_count.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));
    uint64_t run = 0;
    for (size_t i = 0; i < (size_t)n; ++i) { offsets_out[i] = run; run += cnt[i]; }
    offsets_out[n] = run;
    if (run > cap) {
        set_error("phys_overlap: the ids need offsets_out[n] slots, more than cap");
        return PHYS_ERR_CAPACITY;
    }
    if (run == 0) return PHYS_OK;
    PHYS_HIP_TRY(w->qr_ids.resize(2 * (size_t)run));
    uint32_t* tmp = w->qr_ids.p;
    uint32_t* out = w->qr_ids.p + run;
    PHYS_HIP_TRY(hipMemcpyAsync(w->qr_off.p, offsets_out, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    if (query_mask) PHYS_OV_LAUNCH(true, true, (uint32_t*)nullptr, (const unsigned long long*)w->qr_off.p, tmp, qf);
    else PHYS_OV_LAUNCH(true, false, (uint32_t*)nullptr, (const unsigned long long*)w->qr_off.p, tmp);
#undef PHYS_OV_LAUNCH
    hipLaunchKernelGGL(k_ov_order, dim3((unsigned)std::min<uint64_t>(n, kOvMaxSortBlocks)), dim3(kOvSortThreads), 0, s, (uint32_t)n,
                       (const unsigned long long*)w->qr_off.p, (const uint32_t*)tmp, out);
    PHYS_HIP_TRY(hipGetLastError());
    PHYS_HIP_TRY(hipMemcpyAsync(ids_out, out, 4 * (size_t)run, hipMemcpyDeviceToHost, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));
    return PHYS_OK;
}

}  // namespace phys
