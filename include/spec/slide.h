/* slide.h — normative scalar definition of move-and-slide (physics_hip.h, phys_move_and_slide): what a
 * capsule character does with the answer of one capsule cast, and when its loop of casts ends.
 *
 * The reference (martingoe/physics) has no queries, so this header is the specification itself. The HIP kernel
 * (physics_amd/csrc/slide.hip) calls exactly these functions for the arithmetic between two casts, and a host compiler reads
 * the header alone (tests/cpp/slide_probe.cpp), so one launch and a host loop of phys_capsulecast calls with these functions
 * between them agree bit for bit. Build with -ffp-contract=off.
 *
 * Per query: pos, motion, rot (or identity), R, h, ignore, mask; per call: skin (finite, >= 0) and max_slides
 * (1 .. PHYS_SLIDE_MAX_SLIDES).
 *
 *   if !sl_valid(...): status = INVALID, pos_out = pos, remaining_out = motion, every slot empty
 *   sl_begin(&s, pos, motion)
 *   for k in 0 .. max_slides - 1:
 *       L = sl_length(s.m);  if !(L > 0): break
 *       (id, t, n, point) = capsule cast(origin s.p, dir s.m, rot, R, h, max_t = sl_max_t(L, skin), ignore, mask)
 *       if id == PHYS_RAY_MISS: sl_miss(&s); break            the whole of m is free: p += m, m = 0
 *       slot k = (id, n, point)
 *       if !sl_hit(&s, L, skin, t, n): break                  t == 0, the cast starts touching: BLOCKED, m stays
 *   if k ran out: sl_ran_out(&s)                              EXHAUSTED when motion is left
 *   pos_out = s.p, remaining_out = s.m, status_out = s.status
 *
 * sl_hit stops the character `skin` short of the contact, projects what is left of the motion onto the contact plane, in a
 * crease (the slide would re-enter the previous plane) onto the line both planes share, and never lets it turn back against
 * the motion that was asked for.
 *
 * skin == 0 is allowed, but the character then rests ON the surface it hit, and the next cast starts touching: the query
 * normally ends BLOCKED at its second cast with the slide unspent. Use a skin around the world's contact_margin.
 */
#ifndef PHYS_SPEC_SLIDE_H
#define PHYS_SPEC_SLIDE_H

#include <stdint.h>

#include "vec.h"

#define SL_MAX_SLIDES 8u
#define SL_BLOCKED 0x100u   /* a cast started touching (t == 0): no usable normal */
#define SL_EXHAUSTED 0x200u /* max_slides casts were made and motion is left */
#define SL_INVALID 0x400u   /* the query's own values are unusable */
#define SL_HITS_MASK 0xFu   /* the number of hits, 0 .. 8 */
/* |a x b|^2 of two unit normals at or below this: the planes are parallel, a crease between them has no line */
#define SL_PARALLEL 1.0e-12f
/* the cast's own rule for the length of a direction */
#define SL_MAX_LENGTH 3.0e38f

typedef struct {
    v3 p;      /* where the character is */
    v3 m;      /* the motion that is left */
    v3 m0;     /* the motion that was asked for */
    v3 n_prev; /* the normal of the previous hit (have_prev) */
    int have_prev;
    uint32_t status;
} sl_state;

PHYS_HD int sl_finite(float x) { return x >= -3.4028235e38f && x <= 3.4028235e38f; }
PHYS_HD int sl_finite3(v3 a) { return sl_finite(a.x) && sl_finite(a.y) && sl_finite(a.z); }

/* the cast's own expression for the length of its direction */
PHYS_HD float sl_length(v3 m) { return det_sqrtf((m.x * m.x + m.y * m.y) + m.z * m.z); }

/* every value finite, R and h >= 0, |motion| <= 3.0e38 (a zero motion is valid); rot is looked at when has_rot (else identity) */
PHYS_HD int sl_valid(v3 pos, v3 motion, int has_rot, quat rot, float R, float h) {
    if (!sl_finite3(pos) || !sl_finite3(motion) || !sl_finite(R) || !sl_finite(h)) return 0;
    if (has_rot && !(sl_finite(rot.i) && sl_finite(rot.j) && sl_finite(rot.k) && sl_finite(rot.w))) return 0;
    if (!(R >= 0.0f) || !(h >= 0.0f)) return 0;
    return sl_length(motion) <= SL_MAX_LENGTH;
}

PHYS_HD void sl_begin(sl_state* s, v3 pos, v3 motion) {
    s->p = pos; s->m = motion; s->m0 = motion;
    s->n_prev = v3_make(0.0f, 0.0f, 0.0f);
    s->have_prev = 0;
    s->status = 0u;
}

/* how far the cast of a motion of length L looks: the skin beyond it, so that the character stops short of what lies there */
PHYS_HD float sl_max_t(float L, float skin) { return L + skin; }

/* the cast met nothing: the whole motion is made */
PHYS_HD void sl_miss(sl_state* s) {
    s->p = v3_add(s->p, s->m);
    s->m = v3_make(0.0f, 0.0f, 0.0f);
}

/* the cast of s->m (length L > 0) met a target at t with the normal n. Returns 1 when the loop goes on, 0 when it ends here. */
PHYS_HD int sl_hit(sl_state* s, float L, float skin, float t, v3 n) {
    s->status += 1u;
    if (t == 0.0f) { s->status |= SL_BLOCKED; return 0; }
    const v3 u = v3_div(s->m, L);
    float a = t - skin;
    a = a > 0.0f ? a : 0.0f;
    a = a < L ? a : L;
    s->p = v3_add(s->p, v3_scale(u, a));
    const v3 r = v3_scale(u, L - a);
    v3 sl = v3_sub(r, v3_scale(n, v3_dot(r, n)));
    if (s->have_prev && v3_dot(sl, s->n_prev) < 0.0f) {
        const v3 c = v3_cross(s->n_prev, n);
        const float cc = v3_dot(c, c);
        sl = cc > SL_PARALLEL ? v3_scale(c, v3_dot(r, c) / cc) : v3_make(0.0f, 0.0f, 0.0f);
    }
    if (!(v3_dot(sl, s->m0) > 0.0f)) sl = v3_make(0.0f, 0.0f, 0.0f);
    s->n_prev = n;
    s->have_prev = 1;
    s->m = sl;
    return 1;
}

/* max_slides casts were made: EXHAUSTED when motion is left */
PHYS_HD void sl_ran_out(sl_state* s) {
    if (s->m.x != 0.0f || s->m.y != 0.0f || s->m.z != 0.0f) s->status |= SL_EXHAUSTED;
}

#endif /* PHYS_SPEC_SLIDE_H */
