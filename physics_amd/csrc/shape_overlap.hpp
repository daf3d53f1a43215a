// shape_overlap.hpp — the exact intersection test of two closed shapes (sphere, box, capsule), shared by the overlap
// queries (query.hip: the query shape against a target) and the trigger volumes (trigger.hip: the trigger against a
// body). One set of device functions, so that both report the same bits for the same two shapes in the same order.
#pragma once
#include "rc_grid.hpp"

namespace phys {
namespace {

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
        // relative to the target's centre, like the two box tests: the end points c +- hl w rounded to the ulp of world
        // coordinates (1/64 at 2e5 from the origin) would cost the distance its digits
        return qr_seg_seg_d2(v3_sub(Q.c, T.c), wq, hq, v3_make(0.0f, 0.0f, 0.0f), wt, ht) <= rr * rr;
    }
    return qb ? qr_round_box(T, Q) : qr_round_box(Q, T);
}

__device__ __forceinline__ bool aabb_touch(const aabb_t& a, const aabb_t& b) {
    return a.lo.x <= b.hi.x && b.lo.x <= a.hi.x && a.lo.y <= b.hi.y && b.lo.y <= a.hi.y && a.lo.z <= b.hi.z && b.lo.z <= a.hi.z;
}

}  // namespace
}  // namespace phys
