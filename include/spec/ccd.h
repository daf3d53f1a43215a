/* ccd.h — normative scalar definition of continuous collision (physics_hip.h, phys_set_ccd_bodies): a listed
 * body whose step would carry it through a static collider or the ground is advanced only to its time of impact.
 *
 * The reference (martingoe/physics) detects contacts at the sampled poses alone, so this header is the specification itself.
 * The HIP kernel (physics_amd/csrc/ccd.hip, k_ccd_sweep) calls exactly these functions, and a host compiler reads the header
 * alone (tests/cpp/ccd_probe.cpp), so a host probe runs what the kernel runs. Build with -ffp-contract=off. It uses det_math.h,
 * vec.h and box_cast.h and nothing else.
 *
 * Where it runs: behind the solver (and the contact events), in front of the position half, so the velocity it reads is final.
 *
 *   motion   m = v dt component by component, L = |m|. A body is NOT swept (frac = 1.0f exactly, target = CCD_MISS) when L is
 *            not finite or not > 0, its shape is NONE or its pose is not finite. Otherwise u = m (1 / L).
 *   mover    a core box hc in the body's frame plus a radius rho: BOX hc = he, rho = 0; SPHERE hc = 0, rho = he.x; CAPSULE
 *            hc = (0, he.y, 0), rho = he.x. It translates along u without turning.
 *   targets  the ground (if the world has one) and every static, each behind ccd_filter_pass(body's filter, target's filter):
 *            the rule of the narrow phase. Other bodies are no targets.
 *              round static (r [, k])   bx_test of the core box along u against the static with its radius grown to r + rho
 *              box static, box mover    bx_test as it stands
 *              box static, round mover  the roles exchanged: the static's box cast along -u at the body as a round target of
 *                                       h = (rho, k); the same t, the normal negated
 *              ground                   gap = ((x.y - bx_ground_reach(core)) - rho) - ground_y; gap <= 0 touches at t = 0;
 *                                       otherwise, with u.y < 0, t = gap / (-u.y); the normal is +y
 *   hits     a test that starts touching (bx_test's 1, gap <= 0) is NO hit: the discrete contact owns that pair and the solver
 *            has limited the approach already. A hit counts only when t < L. The least (t, id) wins; ids are
 *            PHYS_STATIC_ID_BIT | k and PHYS_RAY_GROUND: the casts' tie rule.
 *   result   frac = min(t / L, 1.0f) on a hit, else 1.0f: the body is integrated for dt * frac, rotation too. The velocity stays:
 *            the body lands touching, the next update's narrow phase makes the manifold. dt * 1.0f == dt, so a body that hits
 *            nothing moves by the bits it moved by without this stage.
 *
 * The cheap reject in front of bx_test (ccd_swept_aabb against the static's fattened box) is part of the rule only in that it
 * must never drop a hit: the box of the mover at x joined with its box at x + m, every side pushed out by CCD_PAD times
 * (1 + the largest coordinate magnitude of the box), which is some hundred float32 spacings there.
 * Nothing here indexes an array at run time.
 */
#ifndef PHYS_SPEC_CCD_H
#define PHYS_SPEC_CCD_H

#include <stdint.h>

#include "det_math.h"
#include "vec.h"
#include "box_cast.h"

#define CCD_SHAPE_NONE 0u         /* PHYS_SHAPE_NONE */
#define CCD_MISS 0xFFFFFFFEu      /* PHYS_RAY_MISS */
#define CCD_GROUND 0xFFFFFFFFu    /* PHYS_RAY_GROUND */
#define CCD_STATIC_BIT 0x80000000u /* PHYS_STATIC_ID_BIT */
#define CCD_PAD 1.0e-5f

typedef struct {
    int swept;    /* 0: the body is not swept (frac 1, no target) */
    int round;    /* the mover has a radius (SPHERE, CAPSULE) */
    v3 m;         /* v dt */
    float L;      /* |m| */
    float rho, k; /* radius and half length of the round mover (0 for a box) */
    quat q;       /* the body's rotation, as stored */
    bx_query core; /* the core box at the pose, along u */
} ccd_mover;

typedef struct {
    float frac;      /* 1.0f: nothing hit */
    uint32_t target; /* CCD_MISS, CCD_GROUND or PHYS_STATIC_ID_BIT | k */
    v3 n;            /* from the target to the body; 0 without a hit */
    float t;         /* the winner's distance along u (inf without a hit) */
} ccd_result;

/* filter_pass of the narrow phase (a filter is {category | mask << 16, group}): the same nonzero group decides by its sign,
 * anything else needs each category in the other's mask */
PHYS_HD int ccd_filter_pass(uint32_t ax, uint32_t ay, uint32_t bx, uint32_t by) {
    if (ay == by && ay != 0u) return (int32_t)ay > 0;
    return (ax & (bx >> 16)) != 0u && (bx & (ax >> 16)) != 0u;
}

/* a ? x : y component by component (of whole structs it would be a choice of addresses, which ends in private memory) */
PHYS_HD v3 ccd_sel3(int a, v3 x, v3 y) { return v3_make(a ? x.x : y.x, a ? x.y : y.y, a ? x.z : y.z); }
PHYS_HD quat ccd_selq(int a, quat x, quat y) {
    quat r;
    r.i = a ? x.i : y.i; r.j = a ? x.j : y.j; r.k = a ? x.k : y.k; r.w = a ? x.w : y.w;
    return r;
}

PHYS_HD ccd_mover ccd_mover_make(uint32_t shape, v3 x, quat q, v3 he, v3 v, float dt) {
    ccd_mover mv;
    mv.m = v3_make(v.x * dt, v.y * dt, v.z * dt);
    mv.L = det_sqrtf((mv.m.x * mv.m.x + mv.m.y * mv.m.y) + mv.m.z * mv.m.z);
    const int pose = bx_finite(x.x) && bx_finite(x.y) && bx_finite(x.z) && bx_finite(q.i) && bx_finite(q.j) && bx_finite(q.k) && bx_finite(q.w);
    mv.swept = bx_finite(mv.L) && mv.L > 0.0f && shape != CCD_SHAPE_NONE && pose;
    const float inv = 1.0f / mv.L;
    const v3 zero = v3_make(0.0f, 0.0f, 0.0f);
    const v3 u = ccd_sel3(mv.swept, v3_scale(mv.m, inv), zero);
    mv.round = shape != BX_SHAPE_BOX;
    mv.rho = mv.round ? he.x : 0.0f;
    mv.k = shape == BX_SHAPE_CAPSULE ? he.y : 0.0f;
    const v3 hc = ccd_sel3(mv.round, v3_make(0.0f, mv.k, 0.0f), he);
    quat id;
    id.i = 0.0f; id.j = 0.0f; id.k = 0.0f; id.w = 1.0f;
    mv.q = ccd_selq(mv.swept, q, id);
    mv.core = bx_query_make(ccd_sel3(mv.swept, x, zero), u, 1, mv.q, hc);
    return mv;
}

/* the mover's box at x joined with its box at x + m, padded (see the head of the file) */
PHYS_HD void ccd_swept_aabb(const ccd_mover* mv, v3* lo, v3* hi) {
    const m33* R = &mv->core.R;
    const v3 h = mv->core.h, o = mv->core.o;
    const float ex = ((h.x * det_absf(R->m[0]) + h.y * det_absf(R->m[1])) + h.z * det_absf(R->m[2])) + mv->rho;
    const float ey = ((h.x * det_absf(R->m[3]) + h.y * det_absf(R->m[4])) + h.z * det_absf(R->m[5])) + mv->rho;
    const float ez = ((h.x * det_absf(R->m[6]) + h.y * det_absf(R->m[7])) + h.z * det_absf(R->m[8])) + mv->rho;
    const v3 e = v3_add(o, mv->m);
    const v3 a = v3_make(det_minf(o.x, e.x) - ex, det_minf(o.y, e.y) - ey, det_minf(o.z, e.z) - ez);
    const v3 b = v3_make(det_maxf(o.x, e.x) + ex, det_maxf(o.y, e.y) + ey, det_maxf(o.z, e.z) + ez);
    const float big = det_maxf(det_maxf(det_maxf(det_absf(a.x), det_absf(a.y)), det_absf(a.z)),
                               det_maxf(det_maxf(det_absf(b.x), det_absf(b.y)), det_absf(b.z)));
    const float pad = CCD_PAD * (1.0f + big);
    *lo = v3_make(a.x - pad, a.y - pad, a.z - pad);
    *hi = v3_make(b.x + pad, b.y + pad, b.z + pad);
}
/* closed boxes; written so that a NaN side keeps the static (the exact test decides) */
PHYS_HD int ccd_aabb_apart(v3 lo, v3 hi, v3 slo, v3 shi) {
    return slo.x > hi.x || lo.x > shi.x || slo.y > hi.y || lo.y > shi.y || slo.z > hi.z || lo.z > shi.z;
}

/* the swept mover against one static (its ray-cast record as a bx_target): bx_test's answer, *n from the static to the body.
 * One bx_test whichever way the roles go: the query and the target are chosen first. */
PHYS_HD int ccd_static_test(const ccd_mover* mv, const bx_target* st, float* t, v3* n) {
    const int box = st->shape == BX_SHAPE_BOX;
    const int exchange = box && mv->round;
    /* chosen value by value, the frame made once behind the choice */
    const bx_query q = bx_query_make(ccd_sel3(exchange, st->c, mv->core.o), ccd_sel3(exchange, v3_neg(mv->core.u), mv->core.u), 1,
                                     ccd_selq(exchange, st->q, mv->q), ccd_sel3(exchange, st->h, mv->core.h));
    bx_target tg;
    tg.shape = exchange ? BX_SHAPE_CAPSULE : st->shape; /* (a capsule of k == 0: bx_test takes it as a sphere) */
    tg.c = ccd_sel3(exchange, mv->core.o, st->c);
    tg.q = ccd_selq(exchange, mv->q, st->q);
    tg.h = ccd_sel3(exchange, v3_make(mv->rho, mv->k, 0.0f), v3_make(box ? st->h.x : st->h.x + mv->rho, st->h.y, st->h.z));
    v3 tn = v3_make(0.0f, 0.0f, 0.0f);
    const int res = bx_test(&q, &tg, t, &tn);
    *n = exchange ? v3_neg(tn) : tn;
    return res;
}

/* the ground y <= ground_y: 0 no approach, 1 touching at the start, 2 reached at *t */
PHYS_HD int ccd_ground_test(const ccd_mover* mv, float ground_y, float* t) {
    const float gap = ((mv->core.o.y - bx_ground_reach(&mv->core)) - mv->rho) - ground_y;
    if (gap <= 0.0f) { *t = 0.0f; return 1; }
    if (!(mv->core.u.y < 0.0f)) return 0;
    *t = gap / (-mv->core.u.y);
    return 2;
}

PHYS_HD ccd_result ccd_result_none(void) {
    ccd_result r;
    r.frac = 1.0f; r.target = CCD_MISS; r.n = v3_make(0.0f, 0.0f, 0.0f); r.t = BX_INF;
    return r;
}
/* one test's answer (res: bx_test's or ccd_ground_test's) into the least (t, id) so far */
PHYS_HD void ccd_take(ccd_result* best, const ccd_mover* mv, int res, float t, v3 n, uint32_t id) {
    if (res == 2 && t < mv->L && (t < best->t || (t == best->t && id < best->target))) {
        best->t = t; best->target = id; best->n = n;
    }
}
/* frac of the winner, once per body */
PHYS_HD void ccd_finish(ccd_result* best, const ccd_mover* mv) {
    best->frac = best->target != CCD_MISS ? det_minf(best->t / mv->L, 1.0f) : 1.0f;
}

#endif /* PHYS_SPEC_CCD_H */
