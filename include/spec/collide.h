/* collide.h — normative scalar definition of the collision-stage arithmetic.
 *
 * The reference (martingoe/physics) has NO shapes, broad-phase or narrow-phase ("parity unpinned"
 * for these rows). This header is therefore the specification itself: per-body AABB, per-pair
 * overlap test and per-pair contact manifold, written as scalar f32 functions with a fixed
 * operation order. The HIP kernels (physics_amd/csrc) and the CPU oracle (oracle/) both compile
 * these functions (-ffp-contract=off) and drive them with independent loops, so a parallel GPU run
 * and a sequential CPU run agree bit for bit. tests/test_collide_kat.py pins the functions
 * themselves with closed-form known answers.
 *
 * Conventions: manifold normal points from body A to body B; depth > 0 is penetration, depth < 0 a
 * speculative gap inside the contact margin. Body B may be the ground plane (PHYS_GROUND_ID) or a static collider
 * (PHYS_STATIC_ID_BIT | k: collide_pair with B's shape and pose read from the static set).
 */
#ifndef PHYS_SPEC_COLLIDE_H
#define PHYS_SPEC_COLLIDE_H

#include <stdint.h>

#include "vec.h"

#define PHYS_GROUND_ID 0xFFFFFFFFu
/* body B of a one-sided manifold: the ground (PHYS_GROUND_ID) or a static collider (PHYS_STATIC_ID_BIT | k). Body and
 * ghost ids stay below 2^31, so for a world without static colliders this is exactly b == PHYS_GROUND_ID. */
#ifndef PHYS_STATIC_ID_BIT
#define PHYS_STATIC_ID_BIT 0x80000000u
#endif
#define PHYS_IS_STATIC_PARTNER(b) (((b) & PHYS_STATIC_ID_BIT) != 0u)
#define PHYS_SPEC_SHAPE_NONE 0u
#define PHYS_SPEC_SHAPE_SPHERE 1u
#define PHYS_SPEC_SHAPE_BOX 2u
/* capsule: radius h.x, core half-length h.y along the body's local y axis (column 1 of R); h.z unused */
#define PHYS_SPEC_SHAPE_CAPSULE 3u

typedef struct { v3 lo, hi; } aabb_t;

typedef struct {
    v3 c;          /* centre (world) */
    m33 R;         /* rotation matrix of the (unnormalised, quirk Q6) quaternion */
    v3 h;          /* half extents; sphere radius in h.x; capsule radius h.x, core half-length h.y */
    uint32_t type;
} geom_t;

typedef struct {
    v3 normal;     /* A -> B */
    int count;     /* 0..4 */
    v3 pt[4];      /* world contact points */
    float depth[4];
} manifold_t;

/* per-lane scratch of the polygon clipper: 128 bytes - ONE polygon of up to 8 vertices, clipped in place (clip_poly), and
 * the depths of the candidate points. The HIP narrow phase keeps it in LDS (one slice per lane, odd dword stride)
 * instead of private scratch memory; the oracle puts it on the stack. At 33 dwords per lane four 256-thread workgroups
 * fit a CU's LDS (two at 192 bytes and two polygons, three at 48 dwords): the narrow phase is bound by how many dependent
 * memory round trips its resident waves can overlap. */
typedef struct {
    v3 poly[8];
    float depth[8];
} clip_ws_t;

PHYS_HD geom_t geom_make(v3 c, quat q, v3 h, uint32_t type) {
    geom_t g;
    g.c = c; g.h = h; g.type = type;
    quat_to_m33(q, &g.R);
    return g;
}

/* column c of a row-major 3x3. Selections, not indexing: a matrix (or any small array) indexed by a run-time value
 * is put into per-lane scratch memory by the GPU compiler, and nothing of this header may live there (DESIGN.md:
 * kernels that used scratch lost data whenever a scratch-using kernel of another stream ran beside them). */
PHYS_HD v3 m33_col(const m33* R, int c) {
    const float m0 = R->m[0], m1 = R->m[1], m2 = R->m[2], m3 = R->m[3], m4 = R->m[4], m5 = R->m[5], m6 = R->m[6],
                m7 = R->m[7], m8 = R->m[8]; /* all nine read first: the selections below are between values */
    return v3_make(c == 0 ? m0 : (c == 1 ? m1 : m2), c == 0 ? m3 : (c == 1 ? m4 : m5),
                   c == 0 ? m6 : (c == 1 ? m7 : m8));
}
PHYS_HD float sel3(const float* a, int i) {
    const float a0 = a[0], a1 = a[1], a2 = a[2];
    return i == 0 ? a0 : (i == 1 ? a1 : a2);
}
/* R^T * v (world -> local for an orthonormal R) */
PHYS_HD v3 m33_tmul_v3(const m33* R, v3 v) {
    return v3_make((R->m[0] * v.x + R->m[3] * v.y) + R->m[6] * v.z,
                   (R->m[1] * v.x + R->m[4] * v.y) + R->m[7] * v.z,
                   (R->m[2] * v.x + R->m[5] * v.y) + R->m[8] * v.z);
}
PHYS_HD float v3_get(v3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

/* ---- A10: fattened world AABB of one body. NONE shapes get an inverted box (never overlaps). */
PHYS_HD aabb_t body_aabb(v3 c, quat q, v3 h, uint32_t type, float margin) {
    aabb_t b;
    v3 e;
    if (type == PHYS_SPEC_SHAPE_SPHERE) {
        e = v3_make(h.x, h.x, h.x);
    } else if (type == PHYS_SPEC_SHAPE_BOX) {
        m33 R;
        quat_to_m33(q, &R);
        e.x = (det_absf(R.m[0]) * h.x + det_absf(R.m[1]) * h.y) + det_absf(R.m[2]) * h.z;
        e.y = (det_absf(R.m[3]) * h.x + det_absf(R.m[4]) * h.y) + det_absf(R.m[5]) * h.z;
        e.z = (det_absf(R.m[6]) * h.x + det_absf(R.m[7]) * h.y) + det_absf(R.m[8]) * h.z;
    } else if (type == PHYS_SPEC_SHAPE_CAPSULE) {
        /* the core segment's extent |h.y * R[:,1]| per axis, plus the radius */
        m33 R;
        quat_to_m33(q, &R);
        e.x = det_absf(R.m[1]) * h.y + h.x;
        e.y = det_absf(R.m[4]) * h.y + h.x;
        e.z = det_absf(R.m[7]) * h.y + h.x;
    } else {
        b.lo = v3_make(3.0e38f, 3.0e38f, 3.0e38f);
        b.hi = v3_make(-3.0e38f, -3.0e38f, -3.0e38f);
        return b;
    }
    b.lo = v3_make((c.x - e.x) - margin, (c.y - e.y) - margin, (c.z - e.z) - margin);
    b.hi = v3_make((c.x + e.x) + margin, (c.y + e.y) + margin, (c.z + e.z) + margin);
    return b;
}

PHYS_HD int aabb_overlap(aabb_t a, aabb_t b) {
    return a.lo.x <= b.hi.x && b.lo.x <= a.hi.x && a.lo.y <= b.hi.y && b.lo.y <= a.hi.y && a.lo.z <= b.hi.z &&
           b.lo.z <= a.hi.z;
}

/* ---- A11: narrow phase -------------------------------------------------------------------- */

PHYS_HD void manifold_clear(manifold_t* m) {
    m->count = 0;
    m->normal = v3_make(0.0f, 1.0f, 0.0f);
    PHYS_UNROLL
    for (int k = 0; k < 4; ++k) { m->pt[k] = v3_make(0.0f, 0.0f, 0.0f); m->depth[k] = 0.0f; }
}

PHYS_HD void collide_sphere_sphere(const geom_t* A, const geom_t* B, float margin, manifold_t* m) {
    const v3 d = v3_sub(B->c, A->c);
    const float dist2 = v3_dot(d, d);
    const float r = A->h.x + B->h.x;
    const float reach = r + margin;
    if (dist2 > reach * reach) return;
    const float dist = det_sqrtf(dist2);
    v3 n = v3_make(0.0f, 1.0f, 0.0f);
    if (dist > 1.0e-12f) n = v3_div(d, dist);
    const float depth = r - dist;
    m->normal = n;
    m->count = 1;
    m->pt[0] = v3_add(A->c, v3_scale(n, A->h.x - 0.5f * depth));
    m->depth[0] = depth;
}

/* sphere S against box X; normal written S -> X */
PHYS_HD void collide_sphere_box_raw(const geom_t* S, const geom_t* X, float margin, manifold_t* m) {
    const v3 p = m33_tmul_v3(&X->R, v3_sub(S->c, X->c)); /* sphere centre in box frame */
    v3 q;
    q.x = det_maxf(-X->h.x, det_minf(p.x, X->h.x));
    q.y = det_maxf(-X->h.y, det_minf(p.y, X->h.y));
    q.z = det_maxf(-X->h.z, det_minf(p.z, X->h.z));
    const float r = S->h.x;
    v3 nl; /* box -> sphere, box frame */
    float depth;
    if (q.x == p.x && q.y == p.y && q.z == p.z) {
        /* centre inside the box: leave through the nearest face */
        const float fx = X->h.x - det_absf(p.x), fy = X->h.y - det_absf(p.y), fz = X->h.z - det_absf(p.z);
        if (fx <= fy && fx <= fz) { nl = v3_make(p.x < 0.0f ? -1.0f : 1.0f, 0.0f, 0.0f); depth = fx + r; q.x = p.x < 0.0f ? -X->h.x : X->h.x; }
        else if (fy <= fz)        { nl = v3_make(0.0f, p.y < 0.0f ? -1.0f : 1.0f, 0.0f); depth = fy + r; q.y = p.y < 0.0f ? -X->h.y : X->h.y; }
        else                      { nl = v3_make(0.0f, 0.0f, p.z < 0.0f ? -1.0f : 1.0f); depth = fz + r; q.z = p.z < 0.0f ? -X->h.z : X->h.z; }
    } else {
        const v3 dl = v3_sub(p, q);
        const float dist2 = v3_dot(dl, dl);
        const float reach = r + margin;
        if (dist2 > reach * reach) return;
        const float dist = det_sqrtf(dist2);
        nl = v3_div(dl, dist);
        depth = r - dist;
    }
    const v3 nw = m33_mul_v3(&X->R, nl);           /* box -> sphere, world */
    m->normal = v3_neg(nw);                        /* sphere -> box */
    m->count = 1;
    m->pt[0] = v3_add(X->c, m33_mul_v3(&X->R, q)); /* on the box surface */
    m->depth[0] = depth;
}

/* Sutherland-Hodgman clip of a convex polygon (<= 8 verts) against  dot(p - c, u) <= lim, IN PLACE. Vertex k is the
 * `a` of edge k and the `b` of edge k - 1: it travels in registers from one edge to the next, and so does its distance (the
 * same expression on the same vertex: the same value), and the first vertex, which the last edge needs again. The output
 * never passes the vertex that is read next: before edge k at most k points are out - or k + 1 right behind a LEAVING edge
 * (two points out for one vertex in), whose next vertex is outside and puts out at most one. A convex polygon leaves a
 * half-plane once; should rounding ever make a degenerate one leave twice, a vertex is overwritten before it is read -
 * deterministically, inside the array, and alike in the oracle and on the device. */
PHYS_HD int clip_poly(v3* p, int n_in, v3 c, v3 u, float lim) {
    int n_out = 0;
    if (n_in <= 0) return 0;
    const v3 first = p[0];
    v3 a = first;
    float da = v3_dot(v3_sub(a, c), u) - lim;
    for (int k = 0; k < 8; ++k) {
        if (k >= n_in) break;
        v3 b = first;
        if (k + 1 != n_in) b = p[k + 1];
        const float db = v3_dot(v3_sub(b, c), u) - lim;
        if (da <= 0.0f) {
            if (n_out < 8) p[n_out++] = a;
            if (db > 0.0f) {
                const float t = da / (da - db);
                if (n_out < 8) p[n_out++] = v3_add(a, v3_scale(v3_sub(b, a), t));
            }
        } else if (db <= 0.0f) {
            const float t = da / (da - db);
            if (n_out < 8) p[n_out++] = v3_add(a, v3_scale(v3_sub(b, a), t));
        }
        a = b; da = db;
    }
    return n_out;
}

/* keep at most 4 of n candidate points: deepest, farthest from it, then the two extreme signed
 * areas. Ties resolve to the lowest index (strict comparisons). */
PHYS_HD void manifold_reduce(const v3* p, const float* depth, int n, v3 normal, manifold_t* m) {
    if (n <= 4) {
        m->count = n;
        PHYS_UNROLL
        for (int k = 0; k < 4; ++k) if (k < n) { m->pt[k] = p[k]; m->depth[k] = depth[k]; }
        return;
    }
    int i0 = 0;
    for (int k = 1; k < 8; ++k) if (k < n && depth[k] > depth[i0]) i0 = k;
    int i1 = -1; float best = -1.0f;
    for (int k = 0; k < 8; ++k) if (k < n && k != i0) {
        const v3 d = v3_sub(p[k], p[i0]);
        const float dd = v3_dot(d, d);
        if (dd > best) { best = dd; i1 = k; }
    }
    int i2 = -1, i3 = -1; float amax = 0.0f, amin = 0.0f;
    const v3 e = v3_sub(p[i1], p[i0]);
    for (int k = 0; k < 8; ++k) if (k < n && k != i0 && k != i1) {
        const float area = v3_dot(v3_cross(e, v3_sub(p[k], p[i0])), normal);
        if (area > amax) { amax = area; i2 = k; }
        if (area < amin) { amin = area; i3 = k; }
    }
    m->pt[0] = p[i0]; m->depth[0] = depth[i0];
    m->pt[1] = p[i1]; m->depth[1] = depth[i1];
    /* the area extremes follow in that order; each manifold slot is written at a fixed index (no run-time
     * indexing of the manifold: it stays in registers on the GPU) */
    const int has2 = i2 >= 0, has3 = i3 >= 0;
    const int s2 = has2 ? i2 : i3;
    if (has2 || has3) { m->pt[2] = p[s2]; m->depth[2] = depth[s2]; }
    if (has2 && has3) { m->pt[3] = p[i3]; m->depth[3] = depth[i3]; }
    m->count = 2 + has2 + has3;
}

/* face contact: Ref's face (axis r, side sgn) against the most anti-parallel face of Inc.
 * Writes points and depths; manifold normal is set by the caller. */
PHYS_HD void box_face_contact(const geom_t* Ref, const geom_t* Inc, int r, float sgn, float margin, v3 n_ab,
                              manifold_t* m, clip_ws_t* ws) {
    const v3 nref = v3_scale(m33_col(&Ref->R, r), sgn);
    /* incident face: axis of Inc most anti-parallel to nref */
    const float d0 = v3_dot(nref, m33_col(&Inc->R, 0));
    const float d1 = v3_dot(nref, m33_col(&Inc->R, 1));
    const float d2 = v3_dot(nref, m33_col(&Inc->R, 2));
    int j = 0; float dj = d0;
    if (det_absf(d1) > det_absf(dj)) { j = 1; dj = d1; }
    if (det_absf(d2) > det_absf(dj)) { j = 2; dj = d2; }
    const float jsgn = dj > 0.0f ? -1.0f : 1.0f;
    const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    const v3 fc = v3_add(Inc->c, v3_scale(m33_col(&Inc->R, j), jsgn * v3_get(Inc->h, j)));
    const v3 e1 = v3_scale(m33_col(&Inc->R, j1), v3_get(Inc->h, j1));
    const v3 e2 = v3_scale(m33_col(&Inc->R, j2), v3_get(Inc->h, j2));
    v3* polyA = ws->poly;
    polyA[0] = v3_add(v3_add(fc, e1), e2);
    polyA[1] = v3_add(v3_sub(fc, e1), e2);
    polyA[2] = v3_sub(v3_sub(fc, e1), e2);
    polyA[3] = v3_sub(v3_add(fc, e1), e2);
    int n = 4;
    const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
    const v3 u1 = m33_col(&Ref->R, r1), u2 = m33_col(&Ref->R, r2);
    const float l1 = v3_get(Ref->h, r1), l2 = v3_get(Ref->h, r2);
    n = clip_poly(polyA, n, Ref->c, u1, l1);
    n = clip_poly(polyA, n, Ref->c, v3_neg(u1), l1);
    n = clip_poly(polyA, n, Ref->c, u2, l2);
    n = clip_poly(polyA, n, Ref->c, v3_neg(u2), l2);
    /* extent of the contact patch (the incident face inside the reference face's side planes) along the two
     * in-plane axes of the reference face: the sliver rule below */
    float lo1 = 3.0e38f, hi1 = -3.0e38f, lo2 = 3.0e38f, hi2 = -3.0e38f;
    /* keep points at or below the reference face (+ margin): compacted in place (nc <= k) */
    v3* cand = ws->poly; float* cdep = ws->depth; int nc = 0;
    const float hr = v3_get(Ref->h, r);
    float deepest = -3.0e38f;
    for (int k = 0; k < 8; ++k) {
        if (k >= n) break;
        const v3 rel = v3_sub(polyA[k], Ref->c);
        const float c1 = v3_dot(rel, u1), c2 = v3_dot(rel, u2);
        lo1 = det_minf(lo1, c1); hi1 = det_maxf(hi1, c1);
        lo2 = det_minf(lo2, c2); hi2 = det_maxf(hi2, c2);
        const float dep = hr - v3_dot(rel, nref);
        if (dep >= -margin) { cand[nc] = polyA[k]; cdep[nc] = dep; deepest = det_maxf(deepest, dep); ++nc; }
    }
    /* SLIVER RULE. Two boxes that touch along an edge or at a corner (diagonal neighbours of a stack: face separation 0
     * on two or three axes at once) come out of the clipper with a patch of no width - up to four points on a line or on
     * one spot, all at depth ~0. Such a manifold carries no load (bias 0, and friction is bounded by a normal impulse
     * that stays 0), yet a stack of boxes has four of them for every manifold that does (C5: 11.4 manifolds and 45
     * points per box, of which 3 x 4 bear weight; 33 solver colours instead of 8). So: a face contact whose patch is
     * narrower than kSliverRel of the smallest half extent of the two faces, and whose deepest point penetrates by no
     * more than kSliverDepth margins, is NOT a contact. A sliver that does penetrate (a box balanced on a thin strip
     * sinks by a quarter of the margin first) is kept, and so is every line contact of a tilted edge on a face (its
     * patch, taken before the depth filter, is as wide as the incident face). */
    {
        const float kSliverRel = 0.1f, kSliverDepth = 0.25f;
        const float width = det_minf(hi1 - lo1, hi2 - lo2);
        const float face = det_minf(det_minf(l1, l2), det_minf(v3_get(Inc->h, j1), v3_get(Inc->h, j2)));
        if (nc > 0 && width < kSliverRel * face && deepest <= kSliverDepth * margin) nc = 0;
    }
    manifold_reduce(cand, cdep, nc, n_ab, m);
}

PHYS_HD void collide_box_box(const geom_t* A, const geom_t* B, float margin, manifold_t* m, clip_ws_t* ws) {
    const v3 d = v3_sub(B->c, A->c);
    float C[3][3], absC[3][3], tA[3], tB[3], hA[3], hB[3];
    hA[0] = A->h.x; hA[1] = A->h.y; hA[2] = A->h.z;
    hB[0] = B->h.x; hB[1] = B->h.y; hB[2] = B->h.z;
    PHYS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const v3 ai = m33_col(&A->R, i);
        tA[i] = v3_dot(d, ai);
        PHYS_UNROLL
        for (int j = 0; j < 3; ++j) {
            C[i][j] = v3_dot(ai, m33_col(&B->R, j));
            absC[i][j] = det_absf(C[i][j]) + 1.0e-6f;
        }
    }
    PHYS_UNROLL
    for (int j = 0; j < 3; ++j) tB[j] = v3_dot(d, m33_col(&B->R, j));

    /* face axes of A */
    float aMax = -3.0e38f; int aAxis = 0;
    PHYS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const float s = det_absf(tA[i]) - (hA[i] + ((absC[i][0] * hB[0] + absC[i][1] * hB[1]) + absC[i][2] * hB[2]));
        if (s > margin) return;
        if (s > aMax) { aMax = s; aAxis = i; }
    }
    /* face axes of B */
    float bMax = -3.0e38f; int bAxis = 0;
    PHYS_UNROLL
    for (int j = 0; j < 3; ++j) {
        const float s = det_absf(tB[j]) - (hB[j] + ((absC[0][j] * hA[0] + absC[1][j] * hA[1]) + absC[2][j] * hA[2]));
        if (s > margin) return;
        if (s > bMax) { bMax = s; bAxis = j; }
    }
    /* edge axes a_i x b_j */
    float eMax = -3.0e38f; int eI = -1, eJ = -1;
    PHYS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        PHYS_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const float len2 = 1.0f - C[i][j] * C[i][j];
            if (len2 < 1.0e-4f) continue; /* near-parallel edges: covered by the face axes */
            const float ra = hA[i1] * absC[i2][j] + hA[i2] * absC[i1][j];
            const float rb = hB[j1] * absC[i][j2] + hB[j2] * absC[i][j1];
            const float dist = det_absf(tA[i2] * C[i1][j] - tA[i1] * C[i2][j]);
            const float s = (dist - (ra + rb)) / det_sqrtf(len2);
            if (s > margin) return;
            if (s > eMax) { eMax = s; eI = i; eJ = j; }
        }
    }
    /* prefer faces (frame coherence): an edge axis must beat the faces clearly. The tolerance scales the FACE side:
     * with separations negative (penetration) `eMax > kRel * faceMax + kAbs` asks the edge axis to be shallower than
     * the shallowest face by 5 % + 0.01. (Round 1 had the factor on the edge side, `kRel * eMax > faceMax + kAbs`,
     * which for penetrations beyond 0.2 let an edge axis EQUAL to a face axis win - two axis-aligned boxes in deep
     * face contact got one edge-edge point instead of a four-point face manifold; found by the brute-force SAT check
     * of tests/test_gpu_independent.py.) */
    const float kRel = 0.95f, kAbs = 0.01f;
    const float faceMax = det_maxf(aMax, bMax);
    if (eI >= 0 && eMax > kRel * faceMax + kAbs) {
        /* edge-edge */
        const v3 ai = m33_col(&A->R, eI), bj = m33_col(&B->R, eJ);
        v3 n = v3_cross(ai, bj);
        const float nl = v3_norm(n);
        n = v3_div(n, nl);
        if (v3_dot(n, d) < 0.0f) n = v3_neg(n);
        /* supporting edges */
        v3 pA = A->c, pB = B->c;
        PHYS_UNROLL
        for (int k = 0; k < 3; ++k) {
            if (k != eI) {
                const v3 ak = m33_col(&A->R, k);
                const float sg = v3_dot(n, ak) > 0.0f ? 1.0f : -1.0f;
                pA = v3_add(pA, v3_scale(ak, sg * hA[k]));
            }
            if (k != eJ) {
                const v3 bk = m33_col(&B->R, k);
                const float sg = v3_dot(n, bk) > 0.0f ? -1.0f : 1.0f;
                pB = v3_add(pB, v3_scale(bk, sg * hB[k]));
            }
        }
        /* closest points of the two lines pA + s*ai, pB + t*bj */
        const v3 w = v3_sub(pA, pB);
        const float b = v3_dot(ai, bj); /* == C[eI][eJ], recomputed so that C is never indexed at run time */
        const float dd = v3_dot(ai, w), ee = v3_dot(bj, w);
        const float den = 1.0f - b * b;
        const float sa = (b * ee - dd) / den;
        const float tb = (ee - b * dd) / den;
        const v3 qa = v3_add(pA, v3_scale(ai, sa));
        const v3 qb = v3_add(pB, v3_scale(bj, tb));
        m->normal = n;
        m->count = 1;
        m->pt[0] = v3_scale(v3_add(qa, qb), 0.5f);
        m->depth[0] = -eMax;
        return;
    }
    if (bMax > kRel * aMax + kAbs) {
        /* reference = B; its face looks back toward A */
        const float sgn = sel3(tB, bAxis) > 0.0f ? -1.0f : 1.0f;
        const v3 nref = v3_scale(m33_col(&B->R, bAxis), sgn); /* B -> A */
        m->normal = v3_neg(nref);
        box_face_contact(B, A, bAxis, sgn, margin, m->normal, m, ws);
    } else {
        const float sgn = sel3(tA, aAxis) < 0.0f ? -1.0f : 1.0f;
        m->normal = v3_scale(m33_col(&A->R, aAxis), sgn); /* A -> B */
        box_face_contact(A, B, aAxis, sgn, margin, m->normal, m, ws);
    }
}

/* body-body manifold of two spheres / boxes (A = lower index, B = higher index); any other shape gives no contact.
 * collide_pair below is the full definition; this is the part the narrow phase of a world without capsules compiles. */
PHYS_HD void collide_pair_sphere_box(const geom_t* A, const geom_t* B, float margin, manifold_t* m, clip_ws_t* ws) {
    manifold_clear(m);
    if (A->type == PHYS_SPEC_SHAPE_SPHERE && B->type == PHYS_SPEC_SHAPE_SPHERE) {
        collide_sphere_sphere(A, B, margin, m);
    } else if (A->type == PHYS_SPEC_SHAPE_SPHERE && B->type == PHYS_SPEC_SHAPE_BOX) {
        collide_sphere_box_raw(A, B, margin, m);
    } else if (A->type == PHYS_SPEC_SHAPE_BOX && B->type == PHYS_SPEC_SHAPE_SPHERE) {
        collide_sphere_box_raw(B, A, margin, m);
        m->normal = v3_neg(m->normal);
    } else if (A->type == PHYS_SPEC_SHAPE_BOX && B->type == PHYS_SPEC_SHAPE_BOX) {
        collide_box_box(A, B, margin, m, ws);
    }
}

/* body against the ground plane y = ground (normal +y). Manifold has A = body, B = ground, so the
 * A -> B normal is (0,-1,0). Spheres and boxes only: collide_ground below adds capsules. */
PHYS_HD void collide_ground_sphere_box(const geom_t* A, float ground, float margin, manifold_t* m, clip_ws_t* ws) {
    manifold_clear(m);
    m->normal = v3_make(0.0f, -1.0f, 0.0f);
    if (A->type == PHYS_SPEC_SHAPE_SPHERE) {
        const float bottom = A->c.y - A->h.x;
        const float depth = ground - bottom;
        if (depth < -margin) return;
        m->count = 1;
        m->pt[0] = v3_make(A->c.x, bottom + 0.5f * depth, A->c.z);
        m->depth[0] = depth;
    } else if (A->type == PHYS_SPEC_SHAPE_BOX) {
        v3* cand = ws->poly; float* cdep = ws->depth; int nc = 0;
        const v3 ex = v3_scale(m33_col(&A->R, 0), A->h.x);
        const v3 ey = v3_scale(m33_col(&A->R, 1), A->h.y);
        const v3 ez = v3_scale(m33_col(&A->R, 2), A->h.z);
        for (int k = 0; k < 8; ++k) {
            v3 p = A->c;
            p = (k & 1) ? v3_add(p, ex) : v3_sub(p, ex);
            p = (k & 2) ? v3_add(p, ey) : v3_sub(p, ey);
            p = (k & 4) ? v3_add(p, ez) : v3_sub(p, ez);
            const float depth = ground - p.y;
            if (depth >= -margin) { cand[nc] = p; cdep[nc] = depth; ++nc; }
        }
        if (nc == 0) return;
        manifold_reduce(cand, cdep, nc, v3_make(0.0f, 1.0f, 0.0f), m);
    }
}


/* ---- capsules ------------------------------------------------------------------------------
 * A capsule is the set of points within h.x of its core segment c +- h.y * u, u = column 1 of R. Every capsule test
 * reduces to spheres on that segment: no polygon clipping, no clip_ws_t, at most two points. Points sit in the middle
 * of the overlap (the sphere-sphere convention); the normal points A -> B. */

/* core axis u (column 1 of R) */
PHYS_HD v3 capsule_axis(const geom_t* A) { return v3_make(A->R.m[1], A->R.m[4], A->R.m[7]); }

/* a sphere of radius r at p: what collide_sphere_sphere / collide_sphere_box_raw take */
PHYS_HD geom_t capsule_ball(v3 p, float r) {
    geom_t g;
    g.c = p;
    g.R.m[0] = 1.0f; g.R.m[1] = 0.0f; g.R.m[2] = 0.0f;
    g.R.m[3] = 0.0f; g.R.m[4] = 1.0f; g.R.m[5] = 0.0f;
    g.R.m[6] = 0.0f; g.R.m[7] = 0.0f; g.R.m[8] = 1.0f;
    g.h = v3_make(r, r, r);
    g.type = PHYS_SPEC_SHAPE_SPHERE;
    return g;
}

/* parameter s in [-hl, hl] of the point c + s*u closest to p */
PHYS_HD float segment_param(v3 c, v3 u, float hl, v3 p) {
    const float uu = v3_dot(u, u);
    float s = 0.0f;
    if (uu > 1.0e-12f) s = v3_dot(v3_sub(p, c), u) / uu;
    return det_maxf(-hl, det_minf(s, hl));
}

/* Closest points of the segments ca + s*ua (|s| <= ha) and cb + t*ub (|t| <= hb), clamped as in Ericson, Real-Time
 * Collision Detection 5.1.9. Near-parallel segments (sin^2 of the angle below 1e-4) start from s = 0. */
PHYS_HD void segment_closest(v3 ca, v3 ua, float ha, v3 cb, v3 ub, float hb, float* s_out, float* t_out) {
    const v3 r = v3_sub(ca, cb);
    const float a = v3_dot(ua, ua), e = v3_dot(ub, ub), b = v3_dot(ua, ub);
    const float c = v3_dot(ua, r), f = v3_dot(ub, r);
    const float denom = a * e - b * b;
    float s = 0.0f, t = 0.0f;
    if (denom > 1.0e-4f * (a * e)) s = det_maxf(-ha, det_minf((b * f - c * e) / denom, ha));
    if (e > 1.0e-12f) t = (b * s + f) / e;
    if (t < -hb || t > hb) {
        t = t < -hb ? -hb : hb;
        s = a > 1.0e-12f ? det_maxf(-ha, det_minf((b * t - c) / a, ha)) : 0.0f;
    }
    *s_out = s;
    *t_out = t;
}

/* capsule A against sphere B: the sphere on A's segment closest to B's centre, then sphere-sphere. One point. */
PHYS_HD void collide_capsule_sphere(const geom_t* A, const geom_t* B, float margin, manifold_t* m) {
    const v3 u = capsule_axis(A);
    const float s = segment_param(A->c, u, A->h.y, B->c);
    const geom_t S = capsule_ball(v3_add(A->c, v3_scale(u, s)), A->h.x);
    collide_sphere_sphere(&S, B, margin, m);
}

/* capsule A against capsule B. Near-parallel segments whose projections overlap (along A's axis, strictly) give the
 * two ends of the overlap, with the normal of the two axes' offset - (0,1,0) for coincident axes; anything else is
 * sphere-sphere at the segments' closest points. */
PHYS_HD void collide_capsule_capsule(const geom_t* A, const geom_t* B, float margin, manifold_t* m) {
    const v3 ua = capsule_axis(A), ub = capsule_axis(B);
    const float ra = A->h.x, rb = B->h.x;
    const float a = v3_dot(ua, ua), e = v3_dot(ub, ub), b = v3_dot(ua, ub);
    if (a > 1.0e-12f && e > 1.0e-12f && a * e - b * b <= 1.0e-4f * (a * e)) {
        const v3 d = v3_sub(B->c, A->c);
        const float sb = v3_dot(d, ua) / a;                    /* B's centre along A's axis */
        const float pb = B->h.y * (det_absf(b) / a);           /* B's half-length along A's axis */
        const float lo = det_maxf(-A->h.y, sb - pb), hi = det_minf(A->h.y, sb + pb);
        if (lo < hi) {
            const v3 perp = v3_sub(d, v3_scale(ua, sb));
            const float dist = v3_norm(perp);
            v3 n = v3_make(0.0f, 1.0f, 0.0f);
            if (dist > 1.0e-12f) n = v3_div(perp, dist);
            const float r = ra + rb;
            int nc = 0;
            PHYS_UNROLL
            for (int k = 0; k < 2; ++k) {
                const float s = k == 0 ? lo : hi;
                const v3 pa = v3_add(A->c, v3_scale(ua, s));
                const float t = segment_param(B->c, ub, B->h.y, pa);
                const v3 qb = v3_add(B->c, v3_scale(ub, t));
                const float depth = r - v3_dot(v3_sub(qb, pa), n);
                if (depth >= -margin) {
                    const v3 p = v3_add(pa, v3_scale(n, ra - 0.5f * depth));
                    if (nc == 0) { m->pt[0] = p; m->depth[0] = depth; }
                    else { m->pt[1] = p; m->depth[1] = depth; }
                    ++nc;
                }
            }
            m->normal = n;
            m->count = nc;
            return;
        }
    }
    float s, t;
    segment_closest(A->c, ua, A->h.y, B->c, ub, B->h.y, &s, &t);
    const geom_t SA = capsule_ball(v3_add(A->c, v3_scale(ua, s)), ra);
    const geom_t SB = capsule_ball(v3_add(B->c, v3_scale(ub, t)), rb);
    collide_sphere_sphere(&SA, &SB, margin, m);
}

/* the segment (pc, dl, hl) and the box edge qe + t*ue (|t| <= he), in the box frame: keeps the closer pair in (*bp, *bq) */
PHYS_HD void capsule_edge_closest(v3 pc, v3 dl, float hl, v3 qe, v3 ue, float he, float* best, v3* bp, v3* bq) {
    float s, t;
    segment_closest(pc, dl, hl, qe, ue, he, &s, &t);
    const v3 p = v3_add(pc, v3_scale(dl, s)), q = v3_add(qe, v3_scale(ue, t));
    const v3 d = v3_sub(p, q);
    const float d2 = v3_dot(d, d);
    if (d2 < *best) { *best = d2; *bp = p; *bq = q; }
}

/* the nearest of the four edges of box face (axis f, side sg) to the segment (pc, dl, hl), box frame; each edge runs
 * along one in-plane axis at +-e of the other */
PHYS_HD void capsule_face_edges(v3 pc, v3 dl, float hl, int f, float sg, v3 e, float* best, v3* bp, v3* bq) {
    const int ja = f == 0 ? 1 : 0, ka = f == 2 ? 1 : 2;  /* the two axes of the face */
    const float ef = f == 0 ? e.x : (f == 1 ? e.y : e.z);
    PHYS_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int along = k < 2 ? ka : ja, across = k < 2 ? ja : ka;  /* along ka at +-e_ja, then along ja at +-e_ka */
        const float side = (k & 1) ? 1.0f : -1.0f;
        const float ec = across == 0 ? e.x : (across == 1 ? e.y : e.z);
        const float qx = f == 0 ? sg * ef : (across == 0 ? side * ec : 0.0f);
        const float qy = f == 1 ? sg * ef : (across == 1 ? side * ec : 0.0f);
        const float qz = f == 2 ? sg * ef : (across == 2 ? side * ec : 0.0f);
        const v3 ue = v3_make(along == 0 ? 1.0f : 0.0f, along == 1 ? 1.0f : 0.0f, along == 2 ? 1.0f : 0.0f);
        const float he = along == 0 ? e.x : (along == 1 ? e.y : e.z);
        capsule_edge_closest(pc, dl, hl, v3_make(qx, qy, qz), ue, he, best, bp, bq);
    }
}

/* one point of capsule A against box B from the closest points p (on A's core) and q (on B's surface), box frame. Where
 * an axis separates the core from the box (sep_f > 0) their distance is the separation; otherwise the core touches or
 * enters the box, and nf (box -> capsule) with its separation sep_f gives normal and depth */
PHYS_HD void capsule_box_point(const geom_t* A, const geom_t* B, v3 p, v3 q, v3 nf, float sep_f, float margin, manifold_t* m) {
    const float r = A->h.x;
    const v3 d = v3_sub(p, q);
    const float dist = v3_norm(d);
    v3 n = nf;
    float depth = r - sep_f;
    if (sep_f > 0.0f && dist > 1.0e-6f) { n = v3_div(d, dist); depth = r - dist; }
    if (depth < -margin) return;
    m->normal = v3_neg(m33_mul_v3(&B->R, n));
    m->count = 1;
    m->pt[0] = v3_add(B->c, m33_mul_v3(&B->R, v3_sub(p, v3_scale(n, r - 0.5f * depth))));
    m->depth[0] = depth;
}

/* capsule A against box B, at most 2 points. SAT in the box frame over the box's 3 face axes and the 3 axes
 * segment x box edge, the segment taken with zero radius and the radius subtracted afterwards. The faces are preferred
 * as in collide_box_box. A face axis clips the segment to the face rectangle; each end of the clipped part within the
 * margin is a point. An edge axis gives one point, at the closest point of the segment to that box edge. A face axis
 * whose rectangle the segment misses (it passes beside an edge or a corner) falls back to sphere-box at the segment
 * point nearest the box (two alternating projections). */
PHYS_HD void collide_capsule_box(const geom_t* A, const geom_t* B, float margin, manifold_t* m) {
    const float r = A->h.x, hl = A->h.y;
    const v3 pc = m33_tmul_v3(&B->R, v3_sub(A->c, B->c)); /* segment centre in the box frame */
    const v3 dl = m33_tmul_v3(&B->R, capsule_axis(A));   /* segment axis in the box frame */
    const float ex = B->h.x, ey = B->h.y, ez = B->h.z;
    /* face axes */
    const float fx = det_absf(pc.x) - (ex + hl * det_absf(dl.x));
    const float fy = det_absf(pc.y) - (ey + hl * det_absf(dl.y));
    const float fz = det_absf(pc.z) - (ez + hl * det_absf(dl.z));
    if (fx - r > margin || fy - r > margin || fz - r > margin) return;
    int fAxis = 0; float fMax = fx;
    if (fy > fMax) { fAxis = 1; fMax = fy; }
    if (fz > fMax) { fAxis = 2; fMax = fz; }
    /* edge axes dl x e_i (local): (0, dl.z, -dl.y), (-dl.z, 0, dl.x), (dl.y, -dl.x, 0) */
    float eMax = -3.0e38f; int eAxis = -1;
    PHYS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const v3 n = i == 0 ? v3_make(0.0f, dl.z, -dl.y) : (i == 1 ? v3_make(-dl.z, 0.0f, dl.x) : v3_make(dl.y, -dl.x, 0.0f));
        const float len2 = v3_dot(n, n);
        if (len2 < 1.0e-4f) continue; /* segment (nearly) parallel to this edge: covered by the face axes */
        const float rb = (ex * det_absf(n.x) + ey * det_absf(n.y)) + ez * det_absf(n.z);
        const float s = (det_absf(v3_dot(pc, n)) - rb) / det_sqrtf(len2);
        if (s - r > margin) return;
        if (s > eMax) { eMax = s; eAxis = i; }
    }
    /* an edge axis must beat the faces clearly; the separations of a zero-radius segment are mostly positive, so the
     * tolerance grows with |fMax| (an edge axis that IS a face normal - a segment across a face - never wins) */
    v3 nl; /* box -> capsule, box frame */
    if (eAxis >= 0 && eMax > fMax + (0.05f * det_absf(fMax) + 0.01f)) {
        v3 n = eAxis == 0 ? v3_make(0.0f, dl.z, -dl.y) : (eAxis == 1 ? v3_make(-dl.z, 0.0f, dl.x) : v3_make(dl.y, -dl.x, 0.0f));
        n = v3_div(n, v3_norm(n));
        if (v3_dot(n, pc) < 0.0f) n = v3_neg(n);
        /* the box edge along axis eAxis on the side n faces */
        const float sx = n.x > 0.0f ? ex : -ex, sy = n.y > 0.0f ? ey : -ey, sz = n.z > 0.0f ? ez : -ez;
        const v3 qe = v3_make(eAxis == 0 ? 0.0f : sx, eAxis == 1 ? 0.0f : sy, eAxis == 2 ? 0.0f : sz);
        const v3 ue = v3_make(eAxis == 0 ? 1.0f : 0.0f, eAxis == 1 ? 1.0f : 0.0f, eAxis == 2 ? 1.0f : 0.0f);
        const float he = eAxis == 0 ? ex : (eAxis == 1 ? ey : ez);
        float best = 3.0e38f;
        v3 p = pc, q = qe;
        capsule_edge_closest(pc, dl, hl, qe, ue, he, &best, &p, &q);
        capsule_box_point(A, B, p, q, n, eMax, margin, m);  /* eMax > fMax: the largest separation */
        return;
    }
    /* face fAxis: the part of the segment inside the face rectangle, s in [lo, hi] */
    const float pf = fAxis == 0 ? pc.x : (fAxis == 1 ? pc.y : pc.z);
    const float sg = pf < 0.0f ? -1.0f : 1.0f;
    float lo = -hl, hi = hl;
    PHYS_UNROLL
    for (int j = 0; j < 3; ++j) {
        if (j == fAxis) continue;
        const float pj = j == 0 ? pc.x : (j == 1 ? pc.y : pc.z);
        const float dj = j == 0 ? dl.x : (j == 1 ? dl.y : dl.z);
        const float ej = j == 0 ? ex : (j == 1 ? ey : ez);
        if (dj == 0.0f) {
            if (det_absf(pj) > ej) { lo = 1.0f; hi = -1.0f; }
        } else {
            const float t0 = (-ej - pj) / dj, t1 = (ej - pj) / dj;
            lo = det_maxf(lo, det_minf(t0, t1));
            hi = det_minf(hi, det_maxf(t0, t1));
        }
    }
    if (lo <= hi) {
        nl = v3_make(fAxis == 0 ? sg : 0.0f, fAxis == 1 ? sg : 0.0f, fAxis == 2 ? sg : 0.0f);
        const float ef = fAxis == 0 ? ex : (fAxis == 1 ? ey : ez);
        const int ends = lo < hi ? 2 : 1;
        int nc = 0;
        PHYS_UNROLL
        for (int k = 0; k < 2; ++k) {
            if (k >= ends) break;
            const float s = k == 0 ? lo : hi;
            const v3 pa = v3_add(pc, v3_scale(dl, s));
            const float paf = fAxis == 0 ? pa.x : (fAxis == 1 ? pa.y : pa.z);
            const float depth = r - (sg * paf - ef);
            if (depth >= -margin) {
                const v3 p = v3_add(B->c, m33_mul_v3(&B->R, v3_sub(pa, v3_scale(nl, r - 0.5f * depth))));
                if (nc == 0) { m->pt[0] = p; m->depth[0] = depth; }
                else { m->pt[1] = p; m->depth[1] = depth; }
                ++nc;
            }
        }
        m->normal = v3_neg(m33_mul_v3(&B->R, nl));
        m->count = nc;
        /* a core outside the box that leans over an edge of the face comes closest beyond the clipped part: where an edge
         * of the face is nearer than the deepest clipped end, that edge's one point is the contact */
        const float sep = det_maxf(fMax, eMax);
        if (sep > 0.0f) {
            float best = 3.0e38f;
            v3 p = pc, q = pc;
            capsule_face_edges(pc, dl, hl, fAxis, sg, B->h, &best, &p, &q);
            const float edge_depth = r - det_sqrtf(best);
            const float deepest = nc == 0 ? -3.0e38f : (nc == 1 ? m->depth[0] : det_maxf(m->depth[0], m->depth[1]));
            if (edge_depth > deepest + 1.0e-6f) {
                manifold_clear(m);
                capsule_box_point(A, B, p, q, nl, sep, margin, m);
            }
        }
        return;
    }
    /* the segment misses the face rectangle */
    float best = 3.0e38f;
    v3 p = pc, q = pc;
    capsule_face_edges(pc, dl, hl, fAxis, sg, B->h, &best, &p, &q);
    capsule_box_point(A, B, p, q, v3_make(fAxis == 0 ? sg : 0.0f, fAxis == 1 ? sg : 0.0f, fAxis == 2 ? sg : 0.0f),
                      det_maxf(fMax, eMax), margin, m);
}

/* capsule A against anything; B a capsule too, a sphere or a box */
PHYS_HD void collide_capsule_any(const geom_t* A, const geom_t* B, float margin, manifold_t* m) {
    if (B->type == PHYS_SPEC_SHAPE_SPHERE) collide_capsule_sphere(A, B, margin, m);
    else if (B->type == PHYS_SPEC_SHAPE_CAPSULE) collide_capsule_capsule(A, B, margin, m);
    else if (B->type == PHYS_SPEC_SHAPE_BOX) collide_capsule_box(A, B, margin, m);
}

/* body-body manifold for the ordered pair (A = lower index, B = higher index), every shape. Pairs with a capsule
 * are tested with the capsule as A (swapped and the normal negated, as sphere/box does). */
PHYS_HD void collide_pair(const geom_t* A, const geom_t* B, float margin, manifold_t* m, clip_ws_t* ws) {
    if (A->type == PHYS_SPEC_SHAPE_CAPSULE) {
        manifold_clear(m);
        collide_capsule_any(A, B, margin, m);
    } else if (B->type == PHYS_SPEC_SHAPE_CAPSULE) {
        manifold_clear(m);
        if (A->type != PHYS_SPEC_SHAPE_NONE) {
            collide_capsule_any(B, A, margin, m);
            m->normal = v3_neg(m->normal);
        }
    } else {
        collide_pair_sphere_box(A, B, margin, m, ws);
    }
}

/* capsule against the ground: one point for each end of the core segment whose sphere reaches the plane within the
 * margin, placed as for a sphere (the middle of the overlap). Coinciding ends (h.y = 0) give one point. */
PHYS_HD void collide_capsule_ground(const geom_t* A, float ground, float margin, manifold_t* m) {
    const v3 ax = v3_scale(capsule_axis(A), A->h.y);
    const v3 p0 = v3_sub(A->c, ax), p1 = v3_add(A->c, ax);
    const float b0 = p0.y - A->h.x, b1 = p1.y - A->h.x;
    const float d0 = ground - b0, d1 = ground - b1;
    const int k0 = d0 >= -margin;
    const int k1 = d1 >= -margin && !(p0.x == p1.x && p0.y == p1.y && p0.z == p1.z);
    const v3 q0 = v3_make(p0.x, b0 + 0.5f * d0, p0.z), q1 = v3_make(p1.x, b1 + 0.5f * d1, p1.z);
    if (k0) { m->pt[0] = q0; m->depth[0] = d0; }
    if (k1) {
        if (k0) { m->pt[1] = q1; m->depth[1] = d1; }
        else { m->pt[0] = q1; m->depth[0] = d1; }
    }
    m->count = k0 + k1;
}

/* body against the ground plane, every shape (see collide_ground_sphere_box) */
PHYS_HD void collide_ground(const geom_t* A, float ground, float margin, manifold_t* m, clip_ws_t* ws) {
    if (A->type == PHYS_SPEC_SHAPE_CAPSULE) {
        manifold_clear(m);
        m->normal = v3_make(0.0f, -1.0f, 0.0f);
        collide_capsule_ground(A, ground, margin, m);
    } else {
        collide_ground_sphere_box(A, ground, margin, m, ws);
    }
}

#endif /* PHYS_SPEC_COLLIDE_H */
