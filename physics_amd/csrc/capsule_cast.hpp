// capsule_cast.hpp — the exact tests of a capsule cast (phys_capsulecast): a capsule of core
// o +- hq * a and radius rad, translated along u without turning, against one record of the query grid or one static.
//
// Each test is a ray from the capsule's centre against the Minkowski sum of the target and the reflected capsule, in
// coordinates relative to the target's centre (as rc_test and sc_test work):
//   sphere r         the capsule of axis a, half-length hq and radius r + rad around the target's centre (ray_capsule)
//   capsule (b, k, r)  the parallelogram {s b - sigma a} thickened by rho = r + rad: its four edges as capsules of radius
//                    rho (they alone cover parallel cores) and its two faces, the planes at +-rho along a x b
//   box              in the box frame a zonotope of four generators (hx e_x, hy e_y, hz e_z, hq a) thickened by rad: the
//                    faces of its six generator pairs, offset by rad, and the edge capsules of radius rad along every
//                    generator (their end balls are the rounded vertices)
// The walk keeps the least (t, id) and the part's own normal; cc_contact then finds the closest points of the two cores
// at that t once per query, for the normal and the touched point.
// Nothing here indexes private memory at run time: the generator loops are unrolled or choose by selects (no scratch).
#pragma once
#include <type_traits>

#include "shape_overlap.hpp"

namespace phys {
namespace {

constexpr float kCcParallel = 1.0e-12f;  // |di x dj|^2 (unit axes) below this: the pair spans no face
constexpr float kCcCoplanar = 1.0e-6f;   // |n . d| below this: the generator d lies in the face of normal n

// is the kernel's argument pack the capsule cast's (CapsuleArgs first)?
template <typename... T> struct has_capsule_args : std::false_type {};
template <typename... R> struct has_capsule_args<CapsuleArgs, R...> : std::true_type {};
template <typename... R>
__device__ __forceinline__ CapsuleArgs capsule_arg(CapsuleArgs c, R...) { return c; }
__device__ __forceinline__ QueryFilters filter_arg(CapsuleArgs, QueryFilters f) { return f; }

__device__ __forceinline__ float cc_clamp(float x, float h) { return fminf(fmaxf(x, -h), h); }

// closest points of the segments c1 + s u1 (|s| <= h1) and c2 + t u2 (|t| <= h2), unit axes: the lines' closest points
// clamped, then each parameter projected onto the other segment in turn (parallel axes start from s = 0)
__device__ __forceinline__ void cc_seg_seg(v3 c1, v3 u1, float h1, v3 c2, v3 u2, float h2, float& s, float& t) {
    const v3 r = v3_sub(c1, c2), x = v3_cross(u1, u2);
    const float b = v3_dot(u1, u2), c = v3_dot(u1, r), f = v3_dot(u2, r);
    const float den = v3_dot(x, x);  // 1 - b^2 without its cancellation
    s = den > kCcParallel ? cc_clamp((b * f - c) / den, h1) : 0.0f;
    t = cc_clamp(b * s + f, h2);
    s = cc_clamp(b * t - c, h1);
    t = cc_clamp(b * s + f, h2);
}

// closest points of the segment l + s d (|s| <= hl, hl > 0) and the box [-h, h], all in the box frame: q on the segment, p
// on the box, the squared distance returned. A segment that crosses the box gives 0 and q = p = a crossing point.
// Otherwise the least over the two end points against the box and the segment against the twelve edges (exact for a
// segment and a convex box, shape_overlap.hpp qr_round_box).
__device__ __forceinline__ float cc_seg_box(v3 l, v3 d, float hl, v3 h, v3& q, v3& p) {
    float lo = -hl, hi = hl;
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pa = a == 0 ? l.x : (a == 1 ? l.y : l.z);
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
    if (!miss && lo <= hi) {
        q = v3_add(l, v3_scale(d, 0.5f * (lo + hi)));
        p = q;
        return 0.0f;
    }
    float d2 = 3.0e38f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const v3 e = v3_add(l, v3_scale(d, k == 0 ? -hl : hl));
        const v3 c = v3_make(cc_clamp(e.x, h.x), cc_clamp(e.y, h.y), cc_clamp(e.z, h.z));
        const v3 g = v3_sub(e, c);
        const float gg = v3_dot(g, g);
        if (gg < d2) { d2 = gg; q = e; p = c; }
    }
#pragma clang loop unroll(disable)
    for (int e = 0; e < 12; ++e) {
        // edge e along axis e / 4, at the corner signs of bits 0 and 1 of e on the other two axes
        const int ax = e >> 2;
        const float s1 = (e & 1) ? 1.0f : -1.0f, s2 = (e & 2) ? 1.0f : -1.0f;
        const v3 ec = v3_make(ax == 0 ? 0.0f : s1 * h.x, ax == 1 ? 0.0f : (ax == 0 ? s1 : s2) * h.y, ax == 2 ? 0.0f : s2 * h.z);
        const v3 eu = v3_make(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f);
        const float eh = ax == 0 ? h.x : (ax == 1 ? h.y : h.z);
        float s, t;
        cc_seg_seg(l, d, hl, ec, eu, eh, s, t);
        const v3 qq = v3_add(l, v3_scale(d, s)), pp = v3_add(ec, v3_scale(eu, t));
        const v3 g = v3_sub(qq, pp);
        const float gg = v3_dot(g, g);
        if (gg < d2) { d2 = gg; q = qq; p = pp; }
    }
    return d2;
}

// One face pair of a thickened zonotope, against the ray l + t dl: the generators di * li and dj * lj (unit axes) span
// the face, the other two (d1 * l1, d2 * l2) place it. Of the two opposite faces only the one that faces the ray can be
// entered. The hit is accepted where it lies inside the parallelogram; a generator that lies in the face's plane makes the
// true face a hexagon, which the parallelograms at both of its ends cover together. Accepted when it beats t.
__device__ __forceinline__ void cc_face(v3 l, v3 dl, v3 di, float li, v3 dj, float lj, v3 d1, float l1, v3 d2, float l2, float rad,
                                        float& t, v3& nrm) {
    const v3 m = v3_cross(di, dj);
    const float mm = v3_dot(m, m);
    if (!(mm > kCcParallel)) return;  // no face: the edge capsules along the two generators coincide there
    const float inv = 1.0f / mm;
    const v3 n = v3_scale(m, 1.0f / sqrtf(mm));
    const float nu = v3_dot(n, dl);
    if (nu == 0.0f) return;
    const float s = nu < 0.0f ? 1.0f : -1.0f;  // the outward normal s n faces the ray
    const float n1 = v3_dot(n, d1), n2 = v3_dot(n, d2);
    const float dist = s * v3_dot(n, l) - ((l1 * fabsf(n1) + l2 * fabsf(n2)) + rad);
    if (!(dist >= 0.0f)) return;  // the origin is behind this face's plane: the sum is entered elsewhere
    const float tf = dist / fabsf(nu);
    if (!(tf < t)) return;
    const v3 x = v3_add(l, v3_scale(dl, tf));
    // x = alpha di + beta dj + (the rest along m): alpha = (x x dj) . m / |m|^2, beta = (di x x) . m / |m|^2
    const float ax = v3_dot(v3_cross(x, dj), m) * inv, bx = v3_dot(v3_cross(di, x), m) * inv;
    const float a1 = l1 * (v3_dot(v3_cross(d1, dj), m) * inv), b1 = l1 * (v3_dot(v3_cross(di, d1), m) * inv);
    const float a2 = l2 * (v3_dot(v3_cross(d2, dj), m) * inv), b2 = l2 * (v3_dot(v3_cross(di, d2), m) * inv);
    const bool c1 = fabsf(n1) <= kCcCoplanar, c2 = fabsf(n2) <= kCcCoplanar;
    const float s1 = n1 >= 0.0f ? s : -s, s2 = n2 >= 0.0f ? s : -s;  // the supporting end of each placing generator
    bool in = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (((k & 1) && !c1) || ((k & 2) && !c2)) continue;
        const float e1 = (k & 1) ? -s1 : s1, e2 = (k & 2) ? -s2 : s2;
        const float al = (ax - e1 * a1) - e2 * a2, be = (bx - e1 * b1) - e2 * b2;
        in = in || (fabsf(al) <= li && fabsf(be) <= lj);
    }
    if (in) { t = tf; nrm = v3_scale(n, s); }
}

// the capsule (o +- hq a, rad), hq > 0, swept along u against one record; accepted into `best` when t <= tmax and (t, id)
// beats it. best keeps the normal of the part that was hit (-u from inside); best_k / best_st remember the record for
// cc_contact.
__device__ __forceinline__ void cc_test(const float4* __restrict__ rec, uint32_t k, bool is_static, float ox, float oy, float oz, float ux,
                                        float uy, float uz, float ax, float ay, float az, float hq, float rad, float tmax,
                                        uint32_t ignore, RayHit& best, uint32_t& best_k, bool& best_st) {
    const float4 a4 = rec[3 * (size_t)k];
    const float4 c4 = rec[3 * (size_t)k + 2];
    const uint32_t id = __float_as_uint(c4.w);
    if (id == ignore) return;
    const float px = ox - a4.x, py = oy - a4.y, pz = oz - a4.z;
    float t, nx, ny, nz;
    if (__float_as_uint(a4.w) == PHYS_SHAPE_SPHERE) {
        if (!ray_capsule(px, py, pz, ux, uy, uz, ax, ay, az, c4.x + rad, hq, t, nx, ny, nz)) return;
    } else if (__float_as_uint(a4.w) == PHYS_SHAPE_CAPSULE) {
        float wx, wy, wz;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        const float rho = c4.x + rad, kk = c4.y;
        const v3 p = v3_make(px, py, pz), u = v3_make(ux, uy, uz), a = v3_make(ax, ay, az), w = v3_make(wx, wy, wz);
        if (qr_seg_seg_d2(p, a, hq, v3_make(0.0f, 0.0f, 0.0f), w, kk) <= rho * rho) {  // the cast starts touching
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            t = __builtin_inff();
            // the parallelogram's edges: along w at -+hq a, along a at +-kk w (none at rho == 0, as sc_test at radius 0)
#pragma unroll
            for (int e = 0; e < (rho > 0.0f ? 4 : 0); ++e) {
                const float sg = (e & 1) ? -1.0f : 1.0f;
                const v3 ec = e < 2 ? v3_scale(a, sg * hq) : v3_scale(w, sg * kk);
                const v3 eu = e < 2 ? w : a;
                float te, ex, ey, ez;
                if (ray_capsule(px - ec.x, py - ec.y, pz - ec.z, ux, uy, uz, eu.x, eu.y, eu.z, rho, e < 2 ? kk : hq, te, ex, ey, ez) &&
                    te < t) {
                    t = te; nx = ex; ny = ey; nz = ez;
                }
            }
            // its two faces (skipped for parallel cores: a sliver the edges cover)
            const v3 m = v3_cross(a, w);
            const float mm = v3_dot(m, m);
            if (mm > kCcParallel) {
                const v3 n = v3_scale(m, 1.0f / sqrtf(mm));
                const float np = v3_dot(n, p), nu = v3_dot(n, u);
                const float s = np > 0.0f ? 1.0f : -1.0f;
                const float dist = fabsf(np) - rho;
                if (dist >= 0.0f && s * nu < 0.0f) {
                    const float tf = dist / fabsf(nu);
                    const v3 x = v3_add(p, v3_scale(u, tf));
                    // x = tau a + sb w + (the rest along m)
                    const float tau = v3_dot(v3_cross(x, w), m) / mm, sb = v3_dot(v3_cross(a, x), m) / mm;
                    if (fabsf(tau) <= hq && fabsf(sb) <= kk && tf < t) { t = tf; nx = s * n.x; ny = s * n.y; nz = s * n.z; }
                }
            }
            if (!(t < __builtin_inff())) return;
        }
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        m33 R;
        quat_to_m33(q, &R);
        const v3 l = m33_tmul_v3(&R, v3_make(px, py, pz)), dl = m33_tmul_v3(&R, v3_make(ux, uy, uz));
        const v3 al = m33_tmul_v3(&R, v3_make(ax, ay, az));
        const v3 h = v3_make(c4.x, c4.y, c4.z);
        float sx, sy, sz;
        // the thickened zonotope lies inside the box grown by rad + hq along every axis: a ray that misses that misses it
        const float grow = rad + hq;
        if (ray_box_local(l.x, l.y, l.z, dl.x, dl.y, dl.z, h.x + grow, h.y + grow, h.z + grow, t, sx, sy, sz) == 0) return;
        v3 cq, cp;
        if (cc_seg_box(l, al, hq, h, cq, cp) <= rad * rad) {  // the cast starts touching
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            t = __builtin_inff();
            v3 mn = v3_make(0.0f, 0.0f, 0.0f);  // local normal of the best part
            const v3 e0 = v3_make(1.0f, 0.0f, 0.0f), e1 = v3_make(0.0f, 1.0f, 0.0f), e2 = v3_make(0.0f, 0.0f, 1.0f);
            // the box's own faces, pushed out by the capsule's extent along them
            cc_face(l, dl, e1, h.y, e2, h.z, e0, h.x, al, hq, rad, t, mn);
            cc_face(l, dl, e2, h.z, e0, h.x, e1, h.y, al, hq, rad, t, mn);
            cc_face(l, dl, e0, h.x, e1, h.y, e2, h.z, al, hq, rad, t, mn);
            // the side faces: a box edge swept along the capsule's axis
            cc_face(l, dl, e0, h.x, al, hq, e1, h.y, e2, h.z, rad, t, mn);
            cc_face(l, dl, e1, h.y, al, hq, e2, h.z, e0, h.x, rad, t, mn);
            cc_face(l, dl, e2, h.z, al, hq, e0, h.x, e1, h.y, rad, t, mn);
            // the edge capsules: generator e / 8 (x, y, z, a) at the ends of the other three chosen by the bits of e. The
            // two whose ends all point back into the sum are no edges and are left out. (rad == 0: the zonotope itself)
            if (rad > 0.0f) {
                const float gx = al.x >= 0.0f ? 1.0f : -1.0f, gy = al.y >= 0.0f ? 1.0f : -1.0f, gz = al.z >= 0.0f ? 1.0f : -1.0f;
#pragma clang loop unroll(disable)
                for (int e = 0; e < 32; ++e) {
                    const int gen = e >> 3;
                    const float b0 = (e & 1) ? 1.0f : -1.0f, b1 = (e & 2) ? 1.0f : -1.0f, b2 = (e & 4) ? 1.0f : -1.0f;
                    const float ex = gen == 0 ? 0.0f : b0;
                    const float ey = gen == 0 ? b0 : (gen == 1 ? 0.0f : b1);
                    const float ez = gen == 3 ? b2 : (gen == 2 ? 0.0f : b1);
                    const float ea = gen == 3 ? 0.0f : b2;
                    const float pa = ex * gx, pb = ey * gy, pc = ez * gz;
                    const float v = gen == 3 ? pa : -ea;
                    if ((pa == 0.0f || pa == v) && (pb == 0.0f || pb == v) && (pc == 0.0f || pc == v)) continue;
                    const float cx = ex * h.x + (ea * hq) * al.x, cy = ey * h.y + (ea * hq) * al.y, cz = ez * h.z + (ea * hq) * al.z;
                    const float wx = gen == 0 ? 1.0f : (gen == 3 ? al.x : 0.0f);
                    const float wy = gen == 1 ? 1.0f : (gen == 3 ? al.y : 0.0f);
                    const float wz = gen == 2 ? 1.0f : (gen == 3 ? al.z : 0.0f);
                    const float hl = gen == 0 ? h.x : (gen == 1 ? h.y : (gen == 2 ? h.z : hq));
                    float te, ex_n, ey_n, ez_n;
                    if (ray_capsule(l.x - cx, l.y - cy, l.z - cz, dl.x, dl.y, dl.z, wx, wy, wz, rad, hl, te, ex_n, ey_n, ez_n) && te < t) {
                        t = te; mn = v3_make(ex_n, ey_n, ez_n);
                    }
                }
            }
            if (!(t < __builtin_inff())) return;
            const v3 nw = m33_mul_v3(&R, mn);
            const float inv = 1.0f / sqrtf(v3_dot(nw, nw));
            nx = nw.x * inv; ny = nw.y * inv; nz = nw.z * inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) {
        best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz;
        best_k = k; best_st = is_static;
    }
}

// the contact of the winning record at t > 0: the closest points of the capsule's core at t and of the target (its core,
// or the box). The normal runs from the target's point to the capsule's, which does not depend on the part rounding chose
// near a seam (the part's own normal, in n on entry, stays where rounding left the two within half of r + rad, and for
// r + rad == 0); the touched point is the target's point plus r * normal. Relative to the target's centre, which is added
// last.
__device__ __forceinline__ void cc_contact(const float4* __restrict__ rec, uint32_t k, float ox, float oy, float oz, float ux, float uy,
                                           float uz, float ax, float ay, float az, float hq, float rad, float t, float& nx, float& ny,
                                           float& nz, v3& point) {
    const float4 a4 = rec[3 * (size_t)k];
    const float4 c4 = rec[3 * (size_t)k + 2];
    const v3 a = v3_make(ax, ay, az);
    const v3 x = v3_make((ox - a4.x) + t * ux, (oy - a4.y) + t * uy, (oz - a4.z) + t * uz);  // the capsule's centre at t
    v3 q, tp;
    float r = c4.x;
    if (__float_as_uint(a4.w) == PHYS_SHAPE_SPHERE) {
        tp = v3_make(0.0f, 0.0f, 0.0f);
        q = v3_add(x, v3_scale(a, cc_clamp(-v3_dot(x, a), hq)));
    } else if (__float_as_uint(a4.w) == PHYS_SHAPE_CAPSULE) {
        float wx, wy, wz, s, tt;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        const v3 w = v3_make(wx, wy, wz);
        cc_seg_seg(x, a, hq, v3_make(0.0f, 0.0f, 0.0f), w, c4.y, s, tt);
        q = v3_add(x, v3_scale(a, s));
        tp = v3_scale(w, tt);
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat qq; qq.i = q4.x; qq.j = q4.y; qq.k = q4.z; qq.w = q4.w;
        m33 R;
        quat_to_m33(qq, &R);
        v3 ql, pl;
        (void)cc_seg_box(m33_tmul_v3(&R, x), m33_tmul_v3(&R, a), hq, v3_make(c4.x, c4.y, c4.z), ql, pl);
        q = m33_mul_v3(&R, ql);
        tp = m33_mul_v3(&R, pl);
        r = 0.0f;
    }
    const v3 v = v3_sub(q, tp);
    const float vv = v3_dot(v, v), rho = r + rad;
    if (rho > 0.0f && vv > 0.25f * (rho * rho)) {
        const float inv = 1.0f / sqrtf(vv);
        nx = v.x * inv; ny = v.y * inv; nz = v.z * inv;
    }
    point = v3_make(a4.x + (tp.x + r * nx), a4.y + (tp.y + r * ny), a4.z + (tp.z + r * nz));
}

}  // namespace
}  // namespace phys
