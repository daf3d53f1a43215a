/* force_field.h — normative scalar definition of the force fields (physics_hip.h, phys_set_force_fields; DESIGN.md
 * section 22): a volume plus a law that adds to the force / torque accumulators of the bodies whose centre lies inside.
 *
 * The reference (martingoe/physics) has one global gravity force and nothing local, so this header is the specification
 * itself: the point-in-volume tests, the three laws, what a field adds to the volume record of volume.h, and the per-body
 * accumulation over a record array, as scalar f32 functions with a fixed operation order. The HIP kernel (physics_amd/csrc/
 * fields.hip) calls exactly these functions, and a host compiler reads the header alone (tests/cpp/field_probe.cpp), so a GPU run and a
 * sequential CPU run agree bit for bit. Build with -ffp-contract=off; no pow, no libm beyond the correctly rounded sqrt.
 *
 * Order: a body's sums start from its accumulators and take the fields' contributions in ascending field index, each
 * contribution formed completely before it is added. Nothing depends on any other body.
 */
#ifndef PHYS_SPEC_FORCE_FIELD_H
#define PHYS_SPEC_FORCE_FIELD_H

#include <stdint.h>

#include "volume.h"

#define PHYS_SPEC_FIELD_ACCEL 0u
#define PHYS_SPEC_FIELD_DRAG 1u
#define PHYS_SPEC_FIELD_RADIAL 2u

/* One field as the evaluation reads it, 112 bytes: the volume's record (volume.h) with kind | shape << 8 | exponent << 16 in
 * its word r[0].w and coef[0] in r[5].w, followed by law = {vec, coef[1]}. */
#define FF_REC_VEC (VOL_REC_VEC + 1)
typedef struct { vol_record vol; vol_f4 law; } ff_record;

/* What the host stages and keeps per field (phys_set_force_fields; poses and params are patched here), 80 bytes = 20 words:
 *   {kind, shape, mask, exponent} {pos, -} {rot ijkw} {half extent, coef[0]} {vec, coef[1]} */
#define FF_STAGE_VEC 5
typedef struct { vol_f4 s[FF_STAGE_VEC]; } ff_staged;

/* what a field reads of one body: centre, velocities at the start of the update, mass, filter category */
typedef struct {
    v3 x, v, w;
    float mass;
    uint32_t category;
} ff_body;

/* a body's running sums; acted == 0: no field has acted yet and F, T are not loaded */
typedef struct {
    v3 F, T;
    int acted;
} ff_sum;

PHYS_HD float ff_u2f(uint32_t u) { return vol_u2f(u); }
PHYS_HD uint32_t ff_f2u(float f) { return vol_f2u(f); }

/* ---- the closed volumes: d = point - centre (world), R the volume's rotation matrix, h its half extents ---- */
PHYS_HD int ff_in_sphere(v3 d, v3 h) { return v3_dot(d, d) <= h.x * h.x; }
PHYS_HD int ff_in_box(const m33* R, v3 d, v3 h) {
    const v3 l = m33_tmul_v3(R, d);
    return det_absf(l.x) <= h.x && det_absf(l.y) <= h.y && det_absf(l.z) <= h.z;
}
/* within h.x of the core segment +- h.y * u, u = column 1 of R */
PHYS_HD int ff_in_capsule(const m33* R, v3 d, v3 h) {
    const v3 u = v3_make(R->m[1], R->m[4], R->m[7]);
    const float t = det_minf(det_maxf(v3_dot(d, u), -h.y), h.y);
    const v3 q = v3_sub(d, v3_scale(u, t));
    return v3_dot(q, q) <= h.x * h.x;
}
PHYS_HD int ff_in_volume(uint32_t shape, const m33* R, v3 d, v3 h) {
    if (shape == PHYS_SPEC_SHAPE_SPHERE) return ff_in_sphere(d, h);
    if (shape == PHYS_SPEC_SHAPE_BOX) return ff_in_box(R, d, h);
    if (shape == PHYS_SPEC_SHAPE_CAPSULE) return ff_in_capsule(R, d, h);
    return 0;
}

/* ---- the laws ---- */
/* ACCEL: F = mass * vec */
PHYS_HD v3 ff_law_accel(float mass, v3 vec) { return v3_scale(vec, mass); }
/* DRAG: F = -coef0 * (v - vec), T = -coef1 * w */
PHYS_HD v3 ff_law_drag_force(v3 v, v3 vec, float coef0) { return v3_scale(v3_sub(v, vec), -coef0); }
PHYS_HD v3 ff_law_drag_torque(v3 w, float coef1) { return v3_scale(w, -coef1); }
/* RADIAL: F = coef0 * (r0 / max(r, r0))^exponent * d / r with d = x - centre, r = |d|; 0: r == 0, nothing */
PHYS_HD int ff_law_radial(v3 d, float coef0, float r0, uint32_t exponent, v3* F) {
    const float r = v3_norm(d);
    if (!(r > 0.0f)) return 0;
    const float s = r0 / det_maxf(r, r0);
    const float g = exponent == 0u ? 1.0f : (exponent == 1u ? s : s * s);
    *F = v3_scale(v3_div(d, r), coef0 * g);
    return 1;
}

/* ---- records ---- */
PHYS_HD ff_staged ff_staged_make(uint32_t kind, uint32_t shape, uint32_t mask, uint32_t exponent, v3 c, quat q, v3 h, v3 vec, float coef0,
                           float coef1) {
    ff_staged s;
    s.s[0] = vol_f4_make(ff_u2f(kind), ff_u2f(shape), ff_u2f(mask), ff_u2f(exponent));
    s.s[1] = vol_f4_make(c.x, c.y, c.z, 0.0f);
    s.s[2] = vol_f4_make(q.i, q.j, q.k, q.w);
    s.s[3] = vol_f4_make(h.x, h.y, h.z, coef0);
    s.s[4] = vol_f4_make(vec.x, vec.y, vec.z, coef1);
    return s;
}

PHYS_HD ff_record ff_record_make(const ff_staged* s) {
    const uint32_t kind = ff_f2u(s->s[0].x), shape = ff_f2u(s->s[0].y), mask = ff_f2u(s->s[0].z), exponent = ff_f2u(s->s[0].w);
    quat q;
    q.i = s->s[2].x; q.j = s->s[2].y; q.k = s->s[2].z; q.w = s->s[2].w;
    ff_record r;
    r.vol = vol_record_make(shape, mask, v3_make(s->s[1].x, s->s[1].y, s->s[1].z), q, v3_make(s->s[3].x, s->s[3].y, s->s[3].z));
    r.vol.r[0].w = ff_u2f(kind | (shape << 8) | (exponent << 16));
    r.vol.r[5].w = s->s[3].w;
    r.law = s->s[4];
    return r;
}

/* ---- one field on one body: 1 and its complete contribution, or 0 (filtered, outside, non-finite centre, r == 0).
 * masked == 0: the set has no masks and the category is not looked at. A non-finite centre fails the AABB comparisons. */
PHYS_HD int ff_contribution(const ff_record* rec, const ff_body* b, int masked, v3* dF, v3* dT) {
    const vol_f4 a0 = rec->vol.r[0], a1 = rec->vol.r[1];
    if (masked && (b->category & vol_mask(a1)) == 0u) return 0;
    const v3 x = b->x;
    if (!vol_box_meets(a0, a1, x, x)) return 0;
    const vol_f4 r2 = rec->vol.r[2], r3 = rec->vol.r[3], r4 = rec->vol.r[4], r5 = rec->vol.r[5], r6 = rec->law;
    const uint32_t word = vol_word(a0);
    const uint32_t kind = word & 0xFFu, shape = (word >> 8) & 0xFFu, exponent = word >> 16;
    const m33 R = vol_rotation(r3, r4, r5);
    const v3 d = v3_sub(x, vol_centre(r2));
    if (!ff_in_volume(shape, &R, d, vol_half_extent(r2, r3, r4))) return 0;
    const v3 vec = v3_make(r6.x, r6.y, r6.z);
    *dT = v3_make(0.0f, 0.0f, 0.0f);
    if (kind == PHYS_SPEC_FIELD_ACCEL) {
        *dF = ff_law_accel(b->mass, vec);
        return 1;
    }
    if (kind == PHYS_SPEC_FIELD_DRAG) {
        *dF = ff_law_drag_force(b->v, vec, r5.w);
        *dT = ff_law_drag_torque(b->w, r6.w);
        return 1;
    }
    if (kind == PHYS_SPEC_FIELD_RADIAL) return ff_law_radial(d, r5.w, r6.w, exponent, dF);
    return 0;
}

/* ---- the per-body accumulation over records [0, n): the sums start from the body's accumulators *acc_F, *acc_T, which
 * are read when the first field acts and not before. Called once per tile with the same `sum`, a tiled walk gives the
 * bits of one walk over the whole array. */
PHYS_HD void ff_accumulate(const ff_record* rec, uint32_t n, const ff_body* b, int masked, const v3* acc_F, const v3* acc_T, ff_sum* sum) {
    for (uint32_t k = 0; k < n; ++k) {
        v3 dF, dT;
        if (!ff_contribution(rec + k, b, masked, &dF, &dT)) continue;
        if (!sum->acted) {
            sum->F = *acc_F;
            sum->T = *acc_T;
            sum->acted = 1;
        }
        sum->F = v3_add(sum->F, dF);
        sum->T = v3_add(sum->T, dT);
    }
}

#endif /* PHYS_SPEC_FORCE_FIELD_H */
