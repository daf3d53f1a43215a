/* liquid.h — normative scalar definition of the liquid volumes (physics_hip.h, phys_set_liquids):
 * an oriented box whose local +y face is a liquid's surface, and buoyancy and drag from the part of each body's SHAPE that
 * lies below that surface. A force field (force_field.h) looks at a body's centre; a liquid looks at its shape and rotation
 * and produces a torque.
 *
 * The reference (martingoe/physics) has one global gravity force and no liquid, so this header is the specification itself:
 * the submerged volume and first moment of a sphere, a box and a capsule below a plane, the record, one liquid on one body,
 * and the per-body accumulation, as scalar f32 functions with a fixed operation order. The HIP kernels (physics_amd/csrc/
 * liquid.hip) call exactly these functions, and a host compiler reads the header alone (tests/cpp/liquid_probe.cpp), so a GPU
 * run and a sequential CPU run agree bit for bit. Build with -ffp-contract=off; no libm beyond the correctly rounded sqrt and
 * det_math.h's asin.
 *
 * Geometry. With R the liquid's rotation matrix and h its half extents, the surface is the plane through pos + h.y * n with
 * unit normal n = column 1 of R; the liquid is the half-space below it, NOT clipped by the box's sides or bottom. The box only
 * decides who is in the pool: with l = R^T (x - pos), |l.x| <= h.x, |l.z| <= h.z and l.y >= -h.y. s = l.y - h.y is the height
 * of the body's centre above the surface.
 *
 * Every rule gives V, the submerged volume, and M, the first moment of the submerged part about the body's centre (the
 * integral of p - x over it). Nothing divides by V: the torque -density * (M x gravity) stays continuous as V -> 0.
 *
 * Order: a body's sums start from its accumulators and take the liquids' contributions in ascending liquid index, each
 * contribution formed completely before it is added. Nothing depends on any other body.
 */
#ifndef PHYS_SPEC_LIQUID_H
#define PHYS_SPEC_LIQUID_H

#include <stdint.h>

#include "volume.h"

#define LQ_PI 3.14159274f /* float(pi) */
#define LQ_NONE 0xFFFFFFFFu

/* the capsule's quadrature: slabs across its axis, kLiqCylSlabs equal ones of the cylinder and kLiqCapSlabs per end cap */
#define kLiqCylSlabs 8
#define kLiqCapSlabs 4
/* A slab whose axis is nearly parallel to the surface, |cu| * (t1 - t0) < kLiqFlat * a, takes the midpoint value instead of
 * the antiderivative's difference. With q = |cu| * (t1 - t0) / a, the difference H(s1) - H(s0) carries an absolute error of
 * about eps * a and is divided by cu: eps / q of the slab. The midpoint rule's error is about q^2 / 24 of it. The two meet at
 * q^3 = 24 eps, q = 0.0142 for eps = 2^-23; 1/64 is the power of two next to it, and both branches are then good to about
 * 1e-5 of the slab's volume. */
#define kLiqFlat 0.015625f

/* One liquid as the evaluation reads it, 128 bytes: the box's volume record (volume.h) with the density in r[5].w, followed by
 * flow = {flow, drag[0]} and grav = {gravity, drag[1]}. */
#define LQ_REC_VEC (VOL_REC_VEC + 2)
typedef struct { vol_record vol; vol_f4 flow; vol_f4 grav; } lq_record;

/* What the host stages and keeps per liquid (phys_set_liquids; poses and params are patched here), 96 bytes:
 *   {mask, -, -, density} {pos, -} {rot ijkw} {half extent, -} {flow, drag[0]} {gravity, drag[1]} */
#define LQ_STAGE_VEC 6
typedef struct { vol_f4 s[LQ_STAGE_VEC]; } lq_staged;

/* what a liquid reads of one body. shape == PHYS_SPEC_SHAPE_NONE: no liquid touches it (no shape, or a non-finite pose).
 * volume and bound follow from shape and h (lq_body_make). v, w are read only with drag. */
typedef struct {
    v3 x, v, w;
    m33 R;
    v3 h;
    uint32_t shape, category;
    float volume; /* V_shape */
    float bound;  /* bounding radius b: r, |h|, 9/8 r + L */
} lq_body;

/* a body's running sums; acted == 0: no liquid has acted yet and F, T are not loaded */
typedef struct {
    v3 F, T;
    int acted;
} lq_sum;

/* submerged volume V and first moment M about the centre */
typedef struct {
    float V;
    v3 M;
} lq_wet;

PHYS_HD float lq_u2f(uint32_t u) { return vol_u2f(u); }
PHYS_HD uint32_t lq_f2u(float f) { return vol_f2u(f); }

/* ---- sphere, exact: cap of height hc = clamp(r - s, 0, 2r). V = pi hc^2 (3r - hc) / 3; the cap's centroid lies
 * 3 (2r - hc)^2 / (4 (3r - hc)) below the centre along n, so M = -n * pi/4 * hc^2 (2r - hc)^2, without the division. ---- */
PHYS_HD lq_wet lq_wet_sphere(float r, float s, v3 n) {
    const float hc = det_minf(det_maxf(r - s, 0.0f), 2.0f * r);
    const float hh = hc * hc, e = 2.0f * r - hc;
    lq_wet o;
    o.V = (LQ_PI * hh) * (3.0f * r - hc) / 3.0f;
    o.M = v3_scale(n, -((LQ_PI * 0.25f) * (hh * (e * e))));
    return o;
}

/* ---- the body: each V_shape in the operations of its rule's fully wet answer, so that frac is exactly 1 there ---- */
PHYS_HD float lq_shape_volume(uint32_t shape, v3 h) {
    if (shape == PHYS_SPEC_SHAPE_SPHERE) return lq_wet_sphere(h.x, -2.0f * h.x, v3_make(0.0f, 0.0f, 0.0f)).V;
    if (shape == PHYS_SPEC_SHAPE_BOX) return ((2.0f * h.x) * (2.0f * h.y)) * (2.0f * h.z);
    if (shape == PHYS_SPEC_SHAPE_CAPSULE) return (LQ_PI * (h.x * h.x)) * (2.0f * h.y + 4.0f / 3.0f * h.x);
    return 0.0f;
}
PHYS_HD float lq_shape_bound(uint32_t shape, v3 h) {
    if (shape == PHYS_SPEC_SHAPE_SPHERE) return h.x;
    if (shape == PHYS_SPEC_SHAPE_BOX) return v3_norm(h);
    /* the rim of the capsule rule's outermost cap slab lies 1.109 r from the cap's centre: 9/8 keeps the reject conservative */
    if (shape == PHYS_SPEC_SHAPE_CAPSULE) return 1.125f * h.x + h.y;
    return 0.0f;
}
PHYS_HD lq_body lq_body_make(uint32_t shape, v3 x, quat q, v3 h, v3 v, v3 w, uint32_t category) {
    lq_body b;
    const float sum = ((det_absf(x.x) + det_absf(x.y)) + (det_absf(x.z) + det_absf(q.i))) + ((det_absf(q.j) + det_absf(q.k)) + det_absf(q.w));
    const int known = shape == PHYS_SPEC_SHAPE_SPHERE || shape == PHYS_SPEC_SHAPE_BOX || shape == PHYS_SPEC_SHAPE_CAPSULE;
    b.shape = (known && sum <= 3.0e38f) ? shape : PHYS_SPEC_SHAPE_NONE; /* NaN or infinite: not touched */
    b.x = x; b.v = v; b.w = w; b.h = h;
    quat_to_m33(q, &b.R);
    b.category = category;
    b.volume = lq_shape_volume(b.shape, h);
    b.bound = lq_shape_bound(b.shape, h);
    return b;
}

/* ---- box, exact: six tetrahedra around the space diagonal from corner (-,-,-) to corner (+,+,+), each clipped by the plane.
 * Everything in the body's frame: nl = R_body^T n, a point p has height s + nl . p and is wet where that is negative. ---- */
#define LQ_SWAP_IF(c, da, db, pa, pb)                    \
    do {                                                 \
        const int c_ = (c);                              \
        const float td_ = da; const v3 tp_ = pa;         \
        da = c_ ? db : da; db = c_ ? td_ : db;           \
        pa.x = c_ ? pb.x : pa.x; pb.x = c_ ? tp_.x : pb.x; \
        pa.y = c_ ? pb.y : pa.y; pb.y = c_ ? tp_.y : pb.y; \
        pa.z = c_ ? pb.z : pa.z; pb.z = c_ ? tp_.z : pb.z; \
    } while (0)

/* the point on edge a -> b at ratio t */
PHYS_HD v3 lq_lerp(v3 a, v3 b, float t) { return v3_add(a, v3_scale(v3_sub(b, a), t)); }
/* adds a tetrahedron of volume vol with vertices a, b, c, e: its first moment is vol * (a + b + c + e) / 4 */
PHYS_HD void lq_add_tet(lq_wet* o, float vol, v3 a, v3 b, v3 c, v3 e) {
    o->V = o->V + vol;
    o->M = v3_add(o->M, v3_scale(v3_add(v3_add(a, b), v3_add(c, e)), 0.25f * vol));
}

/* One tetrahedron of volume vt, vertices p0..p3 at heights d0..d3, added to *o. The vertices are sorted by height first
 * (a five-comparator network of selects: no indexed table), so the wet ones come first and the case is their count:
 *   1 wet: the small tetrahedron at p0 with edge ratios d0 / (d0 - dj);
 *   3 wet: the whole minus the dry small tetrahedron at p3;
 *   2 wet: the prism between the cut triangles (p0, p0p2, p0p3) and (p1, p1p2, p1p3) as the tetrahedra
 *          (p0, p0p2, p0p3, p1), (p1, p1p2, p1p3, p0p2), (p1, p0p2, p0p3, p1p3); the prism's quadrilateral faces lie in the
 *          tetrahedron's faces and in the plane, so they are planar and this is exact. Their volumes are vt times products of
 *          the edge ratios: t02 t03, t12 t13 (1 - t02), t13 t02 (1 - t03).
 * A ratio's denominator is a dry height minus a wet one: above zero. */
PHYS_HD void lq_clip_tet(lq_wet* o, float vt, v3 p0, v3 p1, v3 p2, v3 p3, float d0, float d1, float d2, float d3) {
    LQ_SWAP_IF(d1 < d0, d0, d1, p0, p1);
    LQ_SWAP_IF(d3 < d2, d2, d3, p2, p3);
    LQ_SWAP_IF(d2 < d0, d0, d2, p0, p2);
    LQ_SWAP_IF(d3 < d1, d1, d3, p1, p3);
    LQ_SWAP_IF(d2 < d1, d1, d2, p1, p2);
    if (!(d0 < 0.0f)) return; /* dry */
    if (d3 < 0.0f) {          /* wet */
        lq_add_tet(o, vt, p0, p1, p2, p3);
        return;
    }
    if (!(d1 < 0.0f)) { /* 1 wet */
        const float t1 = d0 / (d0 - d1), t2 = d0 / (d0 - d2), t3 = d0 / (d0 - d3);
        lq_add_tet(o, vt * ((t1 * t2) * t3), p0, lq_lerp(p0, p1, t1), lq_lerp(p0, p2, t2), lq_lerp(p0, p3, t3));
        return;
    }
    if (d2 < 0.0f) { /* 3 wet */
        const float t0 = d3 / (d3 - d0), t1 = d3 / (d3 - d1), t2 = d3 / (d3 - d2);
        lq_add_tet(o, vt, p0, p1, p2, p3);
        lq_add_tet(o, -(vt * ((t0 * t1) * t2)), p3, lq_lerp(p3, p0, t0), lq_lerp(p3, p1, t1), lq_lerp(p3, p2, t2));
        return;
    }
    /* 2 wet */
    const float t02 = d0 / (d0 - d2), t03 = d0 / (d0 - d3), t12 = d1 / (d1 - d2), t13 = d1 / (d1 - d3);
    const v3 a2 = lq_lerp(p0, p2, t02), a3 = lq_lerp(p0, p3, t03), b2 = lq_lerp(p1, p2, t12), b3 = lq_lerp(p1, p3, t13);
    lq_add_tet(o, vt * (t02 * t03), p0, a2, a3, p1);
    lq_add_tet(o, vt * ((t12 * t13) * (1.0f - t02)), p1, b2, b3, a2);
    lq_add_tet(o, vt * ((t13 * t02) * (1.0f - t03)), p1, a2, a3, b3);
}

/* corner j of the box in its own frame: bit 0, 1, 2 of j choose +h.x, +h.y, +h.z */
#define LQ_CORNER(j) v3_make(((j) & 1) ? h.x : -h.x, ((j) & 2) ? h.y : -h.y, ((j) & 4) ? h.z : -h.z)
#define LQ_TET(a, b, c, e) lq_clip_tet(&o, vt, LQ_CORNER(a), LQ_CORNER(b), LQ_CORNER(c), LQ_CORNER(e), d##a, d##b, d##c, d##e)

/* R: the box's rotation; s: its centre's height above the surface; n: the surface normal (world). All eight corners wet or all
 * dry are answered without the clip. */
PHYS_HD lq_wet lq_wet_box(const m33* R, v3 h, float s, v3 n) {
    lq_wet o;
    o.V = 0.0f;
    o.M = v3_make(0.0f, 0.0f, 0.0f);
    const v3 nl = m33_tmul_v3(R, n);
    const float ex = nl.x * h.x, ey = nl.y * h.y, ez = nl.z * h.z;
    const float reach = (det_absf(ex) + det_absf(ey)) + det_absf(ez);
    if (s - reach >= 0.0f) return o; /* all dry */
    const float vol = ((2.0f * h.x) * (2.0f * h.y)) * (2.0f * h.z);
    if (s + reach <= 0.0f) { /* all wet: the moment about the centre is zero */
        o.V = vol;
        return o;
    }
    const float d0 = ((s - ex) - ey) - ez, d1 = ((s + ex) - ey) - ez, d2 = ((s - ex) + ey) - ez, d3 = ((s + ex) + ey) - ez;
    const float d4 = ((s - ex) - ey) + ez, d5 = ((s + ex) - ey) + ez, d6 = ((s - ex) + ey) + ez, d7 = ((s + ex) + ey) + ez;
    const float vt = vol / 6.0f;
    LQ_TET(0, 1, 3, 7);
    LQ_TET(0, 1, 5, 7);
    LQ_TET(0, 2, 3, 7);
    LQ_TET(0, 2, 6, 7);
    LQ_TET(0, 4, 5, 7);
    LQ_TET(0, 4, 6, 7);
    o.M = m33_mul_v3(R, o.M);
    return o;
}

/* ---- capsule, a stated quadrature (an obliquely cut hemisphere has no closed form in det_math.h's vocabulary): slabs across
 * the axis u, each a cylinder of radius rho from t0 to t1 along it, cut exactly by the plane. cu = n . u, st = sqrt(1 - cu^2),
 * a = rho * st, and the disc at t has its centre at height s(t) = s0 + t * cu. The wet fraction of a disc whose centre is at
 * height x * a is f(x) = (acos x - x sqrt(1 - x^2)) / pi, and H(s, a) = s (s <= -a), 0 (s >= a), a G(s / a) between, with
 * G(x) = (x acos x - sqrt(1 - x^2) + (1 - x^2)^(3/2) / 3) / pi, is an antiderivative of it in s. Nothing divides by a, so a
 * vertical capsule (a == 0) is handled. ---- */
PHYS_HD float lq_acos(float x) { return 1.57079637f - det_asinf(x); }
PHYS_HD float lq_seg_f(float x) {
    if (x <= -1.0f) return 1.0f;
    if (x >= 1.0f) return 0.0f;
    return (lq_acos(x) - x * det_sqrtf(1.0f - x * x)) / LQ_PI;
}
PHYS_HD float lq_seg_H(float s, float a) {
    if (s <= -a) return s;
    if (s >= a) return 0.0f;
    const float x = s / a; /* -a < s < a: a > 0 */
    const float c2 = det_maxf(1.0f - x * x, 0.0f), c = det_sqrtf(c2);
    return a * (((x * lq_acos(x) - c) + (c2 * c) / 3.0f) / LQ_PI);
}
/* the wet volume of the slab [t0, t1] of radius^2 rho2 */
PHYS_HD float lq_slab(float rho2, float st, float cu, float s0, float t0, float t1) {
    const float a = det_sqrtf(rho2) * st, dt = t1 - t0;
    if (det_absf(cu) * dt < kLiqFlat * a) return ((LQ_PI * rho2) * lq_seg_f((s0 + (0.5f * (t0 + t1)) * cu) / a)) * dt;
    return (LQ_PI * rho2) * ((lq_seg_H(s0 + t1 * cu, a) - lq_seg_H(s0 + t0 * cu, a)) / cu);
}
/* Each slab's buoyancy acts at its axial midpoint ON the axis: the offset of a cut disc's centroid inside the disc is left out
 * (DESIGN.md section 29 gives the measured cost). Slab j of an end cap spans r j/4 .. r (j+1)/4 beyond the cylinder's end and
 * has the radius^2 r^2 (1 - (3 j^2 + 3 j + 1) / 48) that preserves its true volume. */
#if defined(__HIPCC__)
#define LQ_ROLLED _Pragma("unroll 1") /* one slab's code, not sixteen copies: the asin alone is a few hundred instructions */
#else
#define LQ_ROLLED
#endif
PHYS_HD lq_wet lq_wet_capsule(const m33* R, float r, float L, float s, v3 n) {
    lq_wet o;
    o.V = 0.0f;
    o.M = v3_make(0.0f, 0.0f, 0.0f);
    const v3 u = v3_make(R->m[1], R->m[4], R->m[7]);
    const float cu = v3_dot(n, u);
    const float st = det_sqrtf(det_maxf(1.0f - cu * cu, 0.0f));
    /* the cylinder around all slabs (a cap slab's rim lies outside the true cap): clear of the surface, every slab is */
    const float reach = det_absf(cu) * (L + r) + r * st;
    if (s - reach >= 0.0f) return o; /* dry */
    if (s + reach <= 0.0f) {          /* wet: the moment about the centre is zero */
        o.V = (LQ_PI * (r * r)) * (2.0f * L + 4.0f / 3.0f * r);
        return o;
    }
    const float rr = r * r, q = 0.25f * r, w = 2.0f * L / (float)kLiqCylSlabs;
    float mt = 0.0f; /* the moment along the axis */
    /* from the lower tip up: the lower cap's slabs, the cylinder's, the upper cap's */
    LQ_ROLLED
    for (int j = 0; j < 2 * kLiqCapSlabs + kLiqCylSlabs; ++j) {
        const int cyl = j >= kLiqCapSlabs && j < kLiqCapSlabs + kLiqCylSlabs;
        const int up = j >= kLiqCapSlabs + kLiqCylSlabs;
        const int k = cyl ? j - kLiqCapSlabs : (up ? j - (kLiqCapSlabs + kLiqCylSlabs) : kLiqCapSlabs - 1 - j);
        const float k0 = (float)k, k1 = (float)(k + 1);
        const float rho2 = cyl ? rr : rr * (1.0f - (float)(3 * k * k + 3 * k + 1) / 48.0f);
        const float t0 = cyl ? -L + w * k0 : (up ? L + q * k0 : -L - q * k1);
        const float t1 = cyl ? -L + w * k1 : (up ? L + q * k1 : -L - q * k0);
        const float v = lq_slab(rho2, st, cu, s, t0, t1);
        o.V = o.V + v;
        mt = mt + v * (0.5f * (t0 + t1));
    }
    o.M = v3_scale(u, mt);
    return o;
}

/* ---- records ---- */
PHYS_HD lq_staged lq_staged_make(uint32_t mask, v3 c, quat q, v3 h, float density, v3 gravity, v3 flow, float drag0, float drag1) {
    lq_staged s;
    s.s[0] = vol_f4_make(lq_u2f(mask), 0.0f, 0.0f, density);
    s.s[1] = vol_f4_make(c.x, c.y, c.z, 0.0f);
    s.s[2] = vol_f4_make(q.i, q.j, q.k, q.w);
    s.s[3] = vol_f4_make(h.x, h.y, h.z, 0.0f);
    s.s[4] = vol_f4_make(flow.x, flow.y, flow.z, drag0);
    s.s[5] = vol_f4_make(gravity.x, gravity.y, gravity.z, drag1);
    return s;
}

PHYS_HD lq_record lq_record_make(const lq_staged* s) {
    quat q;
    q.i = s->s[2].x; q.j = s->s[2].y; q.k = s->s[2].z; q.w = s->s[2].w;
    lq_record r;
    r.vol = vol_record_make(PHYS_SPEC_SHAPE_BOX, lq_f2u(s->s[0].x), v3_make(s->s[1].x, s->s[1].y, s->s[1].z), q,
                            v3_make(s->s[3].x, s->s[3].y, s->s[3].z));
    r.vol.r[5].w = s->s[0].w;
    r.flow = s->s[4];
    r.grav = s->s[5];
    return r;
}

/* ---- one liquid on one body: 1, its complete contribution and frac = V_sub / V_shape, or 0 (no shape, filtered, outside the
 * pool, dry). masked == 0: the set has no masks and the category is not looked at. drag == 0: the set has no nonzero drag
 * and the velocities are not looked at. A non-finite centre fails the AABB comparisons. ---- */
PHYS_HD int lq_contribution(const lq_record* rec, const lq_body* b, int masked, int drag, v3* dF, v3* dT, float* frac) {
    if (b->shape == PHYS_SPEC_SHAPE_NONE) return 0;
    const vol_f4 a0 = rec->vol.r[0], a1 = rec->vol.r[1];
    if (masked && (b->category & vol_mask(a1)) == 0u) return 0;
    const v3 x = b->x;
    const v3 bb = v3_make(b->bound, b->bound, b->bound);
    if (!vol_box_meets(a0, a1, v3_sub(x, bb), v3_add(x, bb))) return 0;
    const vol_f4 r2 = rec->vol.r[2], r3 = rec->vol.r[3], r4 = rec->vol.r[4], r5 = rec->vol.r[5];
    const m33 R = vol_rotation(r3, r4, r5);
    const v3 h = vol_half_extent(r2, r3, r4);
    const v3 l = m33_tmul_v3(&R, v3_sub(x, vol_centre(r2)));
    if (!(det_absf(l.x) <= h.x && det_absf(l.z) <= h.z && l.y >= -h.y)) return 0; /* over the footprint, not under the bottom */
    const v3 n = v3_make(R.m[1], R.m[4], R.m[7]);
    const float s = l.y - h.y;
    lq_wet wet;
    if (b->shape == PHYS_SPEC_SHAPE_SPHERE) wet = lq_wet_sphere(b->h.x, s, n);
    else if (b->shape == PHYS_SPEC_SHAPE_BOX) wet = lq_wet_box(&b->R, b->h, s, n);
    else wet = lq_wet_capsule(&b->R, b->h.x, b->h.y, s, n);
    if (!(wet.V > 0.0f)) return 0;
    const float f = det_minf(wet.V / b->volume, 1.0f);
    const float density = r5.w;
    const v3 g = v3_make(rec->grav.x, rec->grav.y, rec->grav.z);
    v3 F = v3_scale(g, -(density * wet.V));
    v3 T = v3_scale(v3_cross(wet.M, g), -density);
    if (drag) {
        const v3 flow = v3_make(rec->flow.x, rec->flow.y, rec->flow.z);
        F = v3_add(F, v3_scale(v3_sub(b->v, flow), -(rec->flow.w * f)));
        T = v3_add(T, v3_scale(b->w, -(rec->grav.w * f)));
    }
    *dF = F;
    *dT = T;
    *frac = f;
    return 1;
}

/* ---- the per-body accumulation over records [0, n): the sums start from the body's accumulators *acc_F, *acc_T, which are
 * read when the first liquid acts and not before. Called once per tile with the same `sum`, a tiled walk gives the bits of one
 * walk over the whole array. ---- */
PHYS_HD void lq_accumulate(const lq_record* rec, uint32_t n, const lq_body* b, int masked, int drag, const v3* acc_F, const v3* acc_T,
                           lq_sum* sum) {
    for (uint32_t k = 0; k < n; ++k) {
        v3 dF, dT;
        float frac;
        if (!lq_contribution(rec + k, b, masked, drag, &dF, &dT, &frac)) continue;
        if (!sum->acted) {
            sum->F = *acc_F;
            sum->T = *acc_T;
            sum->acted = 1;
        }
        sum->F = v3_add(sum->F, dF);
        sum->T = v3_add(sum->T, dT);
    }
}

/* ---- the read-out (phys_get_submersion): frac in the lowest-index liquid that acts on the body and that liquid's index;
 * *liquid == LQ_NONE on entry means none was found yet, and `first` is the index of rec[0] in the set. ---- */
PHYS_HD void lq_submersion(const lq_record* rec, uint32_t n, uint32_t first, const lq_body* b, int masked, float* frac, uint32_t* liquid) {
    for (uint32_t k = 0; k < n && *liquid == LQ_NONE; ++k) {
        v3 dF, dT;
        float f;
        if (!lq_contribution(rec + k, b, masked, 0, &dF, &dT, &f)) continue;
        *frac = f;
        *liquid = first + k;
    }
}

#endif /* PHYS_SPEC_LIQUID_H */
