/* depenetrate.h — normative scalar definition of depenetration (physics_hip.h, phys_penetration and phys_depenetrate; DESIGN.md
 * section 27): how deep a capsule sits in the targets around it, and how it is pushed out of them.
 *
 * The reference (martingoe/physics) has no queries, so this header is the specification itself. The HIP kernel
 * (physics_amd/csrc/depen.hip) calls exactly these functions, and a host compiler reads the header alone
 * (tests/cpp/depen_probe.cpp), so one launch and a host loop of phys_penetration calls with dp_step between them agree bit for
 * bit. The depths and normals are collide.h's (collide_capsule_any, collide_capsule_ground): nothing of the narrow phase is
 * restated. Build with -ffp-contract=off.
 *
 * The query capsule: core p +- h * a, radius R; a is the y axis turned by rot (dp_axis: the casts' expression, used as given),
 * (0,1,0) without a rot. h == 0 is a ball.
 *
 * The probe (dp_deepest in the prose; the kernel and the host probe drive it with their own loops) at a position p, with a
 * gap (finite, >= 0):
 *
 *   Q = dp_capsule(p, a, R, h);  best = dp_none()
 *   for every target T (bodies, statics; never ghost slots, NONE shapes, ignore_body or a category the mask misses):
 *       dp_target(&Q, &T, id, gap, &best)           collide_capsule_any(Q, T, gap): counts when it has a point
 *   with a ground plane: dp_ground(&Q, ground_height, gap, &best)
 *
 * A target's depth is the larger of its points' depths (>= -gap; negative: a clearance), its normal -m.normal: from the
 * target to the capsule, the casts' convention ((0,1,0) on the ground). The answer is the greatest depth, an exact tie going
 * to the smaller id (dp_better): bodies, then statics, then the ground. A maximum with an id tie-break does not mind a target
 * met twice. A miss is PHYS_RAY_MISS, depth -inf, normal 0.
 *
 * The loop, per query; per call: skin (finite, >= 0) and max_iters (1 .. DP_MAX_ITERS):
 *
 *   if !dp_valid(pos, rot, R, h): status = INVALID, pos_out = pos, every slot empty
 *   dp_begin(&s, pos)
 *   for k in 0 .. max_iters:
 *       best = the probe at s.p with gap = skin
 *       if !dp_step(&s, k, max_iters, skin, &best): break
 *       slot k = (best.id, best.n, best.depth)
 *   pos_out = s.p, status_out = s.status
 *
 * dp_step ends the loop when the capsule is clear (a miss, or the deepest target at least skin / 2 away: !(d > -skin / 2)),
 * or when max_iters pushes were made and it still is not (STUCK); otherwise it counts a push and moves the capsule by
 * n * (d + skin): out of the target and a skin beyond. skin / 2 lies between the clearance a push leaves (skin) and zero, so
 * round-off in the next probe never asks for another push, and a clear capsule is clear for phys_move_and_slide's first cast.
 * One target per round, the deepest first: one plane takes one push, two perpendicular planes two, an acute crease converges
 * geometrically, and a capsule between two opposed targets ends STUCK at a finite position.
 *
 * skin == 0 is allowed: the loop then acts on d > 0 alone and a push ends touching, so the next probe's round-off decides
 * whether it pushes again: such a query tends to end touching or STUCK. Use a skin around the world's contact_margin.
 */
#ifndef PHYS_SPEC_DEPENETRATE_H
#define PHYS_SPEC_DEPENETRATE_H

#include <stdint.h>

#include "vec.h"
#include "collide.h"

#define DP_MAX_ITERS 8u
#define DP_STUCK 0x100u    /* max_iters pushes were made and the capsule is still not clear */
#define DP_INVALID 0x400u  /* the query's own values are unusable (the bit of SL_INVALID; 0x200 stays unused) */
#define DP_PUSHES_MASK 0xFu /* the number of pushes, 0 .. 8 */
#define DP_MISS 0xFFFFFFFEu   /* PHYS_RAY_MISS */
#define DP_GROUND 0xFFFFFFFFu /* PHYS_RAY_GROUND: above every body and static id, so the ground loses exact ties */
/* the capsule cast's bound on a half-length */
#define DP_MAX_HALF_LENGTH 3.4e38f

/* the deepest target so far */
typedef struct {
    uint32_t id; /* DP_MISS: none */
    float depth; /* -inf for none */
    v3 n;        /* from the target to the capsule */
} dp_best;

typedef struct {
    v3 p;            /* where the capsule is */
    uint32_t status; /* pushes made | flags */
} dp_state;

PHYS_HD int dp_finite(float x) { return x >= -3.4028235e38f && x <= 3.4028235e38f; }
PHYS_HD int dp_finite3(v3 a) { return dp_finite(a.x) && dp_finite(a.y) && dp_finite(a.z); }

/* the casts' own expression for a capsule's core axis: column 1 of the rotation matrix of rot, not normalised */
PHYS_HD v3 dp_axis(quat q) {
    const float qi = q.i, qj = q.j, qk = q.k, qw = q.w;
    return v3_make((qi * qj * 2.0f) - (qw * qk * 2.0f), (((qw * qw) - (qi * qi)) + (qj * qj)) - (qk * qk),
                   (qw * qi * 2.0f) + (qj * qk * 2.0f));
}

/* every value finite, R and h >= 0, h <= 3.4e38; rot is looked at when has_rot (else identity) */
PHYS_HD int dp_valid(v3 pos, int has_rot, quat rot, float R, float h) {
    if (!dp_finite3(pos) || !dp_finite(R) || !dp_finite(h)) return 0;
    if (has_rot && !(dp_finite(rot.i) && dp_finite(rot.j) && dp_finite(rot.k) && dp_finite(rot.w))) return 0;
    if (!(R >= 0.0f) || !(h >= 0.0f)) return 0;
    return h <= DP_MAX_HALF_LENGTH;
}

/* the query as collide.h's capsule A: centre p, column 1 of R the axis a, h = (R, h, 0). The capsule functions read nothing
 * else of it; the other columns are the identity's */
PHYS_HD geom_t dp_capsule(v3 p, v3 a, float R, float h) {
    geom_t g;
    g.c = p;
    g.R.m[0] = 1.0f; g.R.m[1] = a.x; g.R.m[2] = 0.0f;
    g.R.m[3] = 0.0f; g.R.m[4] = a.y; g.R.m[5] = 0.0f;
    g.R.m[6] = 0.0f; g.R.m[7] = a.z; g.R.m[8] = 1.0f;
    g.h = v3_make(R, h, 0.0f);
    g.type = PHYS_SPEC_SHAPE_CAPSULE;
    return g;
}

PHYS_HD dp_best dp_none(void) {
    dp_best b;
    b.id = DP_MISS;
    b.depth = -__builtin_inff();
    b.n = v3_make(0.0f, 0.0f, 0.0f);
    return b;
}

/* deeper wins; an exact tie goes to the smaller id */
PHYS_HD int dp_better(float depth, uint32_t id, float best_depth, uint32_t best_id) {
    return depth > best_depth || (depth == best_depth && id < best_id);
}

/* a manifold of the query (as A) against target `id` into best: its deepest point, the normal turned to point at the capsule */
PHYS_HD void dp_take(const manifold_t* m, uint32_t id, dp_best* best) {
    if (m->count <= 0) return;
    float d = m->depth[0];
    if (m->count > 1 && m->depth[1] > d) d = m->depth[1];
    if (dp_better(d, id, best->depth, best->id)) { best->id = id; best->depth = d; best->n = v3_neg(m->normal); }
}

/* one body or static collider T (SPHERE, BOX or CAPSULE; anything else never counts) */
PHYS_HD void dp_target(const geom_t* Q, const geom_t* T, uint32_t id, float gap, dp_best* best) {
    manifold_t m;
    manifold_clear(&m);
    collide_capsule_any(Q, T, gap, &m);
    dp_take(&m, id, best);
}

/* the ground plane y = ground_y */
PHYS_HD void dp_ground(const geom_t* Q, float ground_y, float gap, dp_best* best) {
    manifold_t m;
    manifold_clear(&m);
    m.normal = v3_make(0.0f, -1.0f, 0.0f);
    collide_capsule_ground(Q, ground_y, gap, &m);
    dp_take(&m, DP_GROUND, best);
}

PHYS_HD void dp_begin(dp_state* s, v3 pos) {
    s->p = pos;
    s->status = 0u;
}

/* round k (0 .. max_iters) of the loop with the probe's answer at s->p (gap = skin). Returns 1 when a push was made: the
 * caller records slot k and probes again; 0 when the loop ends here. */
PHYS_HD int dp_step(dp_state* s, uint32_t k, uint32_t max_iters, float skin, const dp_best* best) {
    if (best->id == DP_MISS || !(best->depth > -0.5f * skin)) return 0; /* clear: at least skin / 2 from everything */
    if (k >= max_iters) { s->status |= DP_STUCK; return 0; }            /* max_iters pushes made and still not clear */
    s->status += 1u;
    s->p = v3_add(s->p, v3_scale(best->n, best->depth + skin));
    return 1;
}

#endif /* PHYS_SPEC_DEPENETRATE_H */
