"""Float64 brute force of the box cast (include/physics_hip.h, phys_boxcast), written for the tests: every query against
every target, numpy only. It shares nothing with the kernel: the kernel casts a ray at a Minkowski sum or sweeps separating
axes; this reference walks the exact distance of the cast box to the target, capsulecast_ref's method with the cast box in
place of the core.

    h = boxcast(origins, dirs, rot, half_extent, targets, max_t=None, ignore=None, ground=None, centre=None)

targets, ground, centre: as in query_ref. Per query: body, t, t2 (the second-best t), normal, point, valid, and o, u, R, he
(origin, unit direction, frame and half extents, measured from the centre), which (the winning target's row), tg.

separation(t) = distance(cast box at o + t u, target's core or box) - r is convex in t (the distance of two convex sets under
a translation), so a golden section finds its minimum and a bisection the first t with separation <= 0. The distances are
exact closed forms: a point against a box (clamp), a segment against a box (capsulecast_ref.seg_box_closest with the cast box
as the box), and two boxes as the least over each box's twelve edges against the other box (checked against nested golden
sections in tests/test_boxcast_cpu.py). The normal is the shortest vector a little before the touch, the point comes from the
closest pair."""
import numpy as np

import query_ref
from capsulecast_ref import seg_box_closest
from query_ref import SHAPE_BOX, SHAPE_CAPSULE, SHAPE_SPHERE
from raycast_ref import GROUND, MISS, rotation_matrices

_EDGES = [(ax, s1, s2) for ax in range(3) for s1 in (-1.0, 1.0) for s2 in (-1.0, 1.0)]


def _edges_box(ca, Ra, ha, cb, Rb, hb):
    """The closest pair over the twelve edges of box a (centres ca, frames Ra, half extents ha: rows) against box b: (point
    on a, point on b, distance), world frame. (The twelve edges of every pair go through seg_box_closest as rows of one call.)"""
    n = len(ca)
    rel = np.einsum("pj,pjk->pk", ca - cb, Rb)      # a's centre in b's frame
    A = np.einsum("pji,pjk->pik", Ra, Rb)            # A[p, i] = a's axis i in b's frame
    cs, ws, hs = [], [], []
    for ax, s1, s2 in _EDGES:
        o1, o2 = [a for a in range(3) if a != ax]
        cs.append(rel + (s1 * ha[:, o1])[:, None] * A[:, o1] + (s2 * ha[:, o2])[:, None] * A[:, o2])
        ws.append(A[:, ax])
        hs.append(ha[:, ax])
    q, p, d = seg_box_closest(np.concatenate(cs), np.concatenate(ws), np.concatenate(hs), np.tile(hb, (12, 1)))
    k = d.reshape(12, n).argmin(0)
    idx = k * n + np.arange(n)
    q = np.einsum("pjk,pk->pj", Rb, q[idx]) + cb
    p = np.einsum("pjk,pk->pj", Rb, p[idx]) + cb
    return q, p, d[idx]


def box_box_closest(ca, Ra, ha, cb, Rb, hb):
    """Closest points (q on box a, p on box b) and distance of two boxes, rows: the least over each box's twelve edges
    against the other box (0 where they overlap)."""
    q1, p1, d1 = _edges_box(ca, Ra, ha, cb, Rb, hb)
    p2, q2, d2 = _edges_box(cb, Rb, hb, ca, Ra, ha)
    first = d1 <= d2
    return np.where(first[:, None], q1, q2), np.where(first[:, None], p1, p2), np.where(first, d1, d2)


def closest(c, Rq, hq, pos, R, he, shape):
    """Rows of pairs: the cast box (centre c, frame Rq, half extents hq) against the target (pos, R, he, shape). Returns (q on
    the cast box, p on the target's core or box, their distance, the target's radius), world frame."""
    n = len(c)
    q, p, d, r = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, np.inf), np.zeros(n)
    sph = (shape == SHAPE_SPHERE) | ((shape == SHAPE_CAPSULE) & (he[:, 1] == 0))
    if sph.any():
        l = np.einsum("pj,pjk->pk", pos[sph] - c[sph], Rq[sph])
        cl = np.clip(l, -hq[sph], hq[sph])
        q[sph] = np.einsum("pjk,pk->pj", Rq[sph], cl) + c[sph]
        p[sph] = pos[sph]
        d[sph] = np.linalg.norm(l - cl, axis=1)
        r[sph] = he[sph, 0]
    cap = (shape == SHAPE_CAPSULE) & ~sph
    if cap.any():
        l = np.einsum("pj,pjk->pk", pos[cap] - c[cap], Rq[cap])
        w = np.einsum("pj,pjk->pk", R[cap][:, :, 1], Rq[cap])
        pp, qq, dd = seg_box_closest(l, w, he[cap, 1].copy(), hq[cap])
        q[cap] = np.einsum("pjk,pk->pj", Rq[cap], qq) + c[cap]
        p[cap] = np.einsum("pjk,pk->pj", Rq[cap], pp) + c[cap]
        d[cap] = dd
        r[cap] = he[cap, 0]
    box = shape == SHAPE_BOX
    if box.any():
        q[box], p[box], d[box] = box_box_closest(c[box], Rq[box], hq[box], pos[box], R[box], he[box])
    return q, p, d, r


def inputs(origins, dirs, rot, half_extent, tg, max_t=None, ignore=None, ground=None, centre=None):
    """What the answer carries of the call itself, measured from the centre: o, u, R, he, valid, tg, ground (and mt, ig for
    boxcast below). Cheap; the stored answers of tests/golden/boxcast hold the rest."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    dv = np.asarray(dirs, np.float64).reshape(-1, 3)
    if centre is not None:
        c, tg, ground = query_ref._centred(tg, centre, ground)
        o = o - c
    n = len(o)
    hq = np.broadcast_to(np.asarray(half_extent, np.float64).reshape(-1, 3), (n, 3)).copy()
    q4 = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rot is None else np.asarray(rot, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(dv, axis=1)
        valid = np.isfinite(o).all(1) & np.isfinite(dv).all(1) & (ln > 0) & np.isfinite(ln) & np.isfinite(q4).all(1) \
            & (hq >= 0).all(1) & np.isfinite(hq).all(1)
        u = np.where(valid[:, None], dv / np.where(valid, ln, 1.0)[:, None], 0.0)
        Rq = rotation_matrices(np.where(valid[:, None], q4, [0.0, 0.0, 0.0, 1.0])) if n else np.zeros((0, 3, 3))
    mt = np.full(n, np.inf) if max_t is None else np.asarray(max_t, np.float64).reshape(-1)
    ig = np.full(n, -1, np.int64) if ignore is None else np.asarray(ignore, np.int64).reshape(-1)
    valid &= mt >= 0
    hq = np.where(valid[:, None], hq, 0.0)
    return dict(o=o, u=u, R=Rq, he=hq, valid=valid, tg=tg, ground=ground, mt=mt, ig=ig)


def boxcast(origins, dirs, rot, half_extent, tg, max_t=None, ignore=None, ground=None, centre=None, iters=56):
    base = inputs(origins, dirs, rot, half_extent, tg, max_t, ignore, ground, centre)
    o, u, Rq, hq, valid, tg, ground, mt, ig = (base[k] for k in ("o", "u", "R", "he", "valid", "tg", "ground", "mt", "ig"))
    n = len(o)
    reach_q = np.linalg.norm(hq, axis=1)
    m = len(tg["pos"])
    R = query_ref._frames(tg)
    b = query_ref._bound(tg["half_extent"], tg["shape"]) if m else np.zeros(0)
    shaped = np.isin(tg["shape"], (SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE)) if m else np.zeros(0, bool)
    ri, mi = np.nonzero(valid[:, None] & shaped[None, :]) if m else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    # cull by the swept bounding sphere
    rel = tg["pos"][mi] - o[ri]
    along = (rel * u[ri]).sum(-1)
    perp = np.linalg.norm(rel - along[:, None] * u[ri], axis=1)
    reach = b[mi] + reach_q[ri] + 1e-9
    keep = (perp <= reach) & ((along >= -reach) | (np.linalg.norm(rel, axis=1) <= reach)) & (tg["id"][mi] != ig[ri])
    ri, mi = ri[keep], mi[keep]
    pos, Rm, he, sh = tg["pos"][mi], R[mi], tg["half_extent"][mi], tg["shape"][mi]
    oo, uu, RR, hh = o[ri], u[ri], Rq[ri], hq[ri]

    def f(t, sel):
        _, _, d, r = closest(oo[sel] + t[:, None] * uu[sel], RR[sel], hh[sel], pos[sel], Rm[sel], he[sel], sh[sel])
        return d - r

    k = len(ri)
    t = np.full(k, np.inf)
    f0 = f(np.zeros(k), np.arange(k))
    t[f0 <= 0] = 0.0
    todo = np.nonzero(f0 > 0)[0]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    lo_t = np.zeros(len(todo))
    hi_t = np.maximum(np.linalg.norm(pos[todo] - oo[todo], axis=1) + b[mi[todo]] + reach_q[ri[todo]] + 1.0, 1.0)
    for _ in range(iters):
        m1, m2 = hi_t - g * (hi_t - lo_t), lo_t + g * (hi_t - lo_t)
        left = f(m1, todo) <= f(m2, todo)
        hi_t = np.where(left, m2, hi_t)
        lo_t = np.where(left, lo_t, m1)
    tmin = 0.5 * (lo_t + hi_t)
    # (1e-9: two sets of no thickness touch at one t, where the distance is a V the search has found to 1e-10)
    touches = f(tmin, todo) <= 1e-9
    touch, lo_t, hi_t = todo[touches], np.zeros(int(touches.sum())), tmin[touches]
    for _ in range(iters):
        mid = 0.5 * (lo_t + hi_t)
        inside = f(mid, touch) <= 0
        hi_t = np.where(inside, mid, hi_t)
        lo_t = np.where(inside, lo_t, mid)
    t[touch] = hi_t
    t[t > mt[ri]] = np.inf
    ids = tg["id"][mi]
    if ground is not None:
        gy = ground + (hq * np.abs(Rq[:, 1, :])).sum(1)
        with np.errstate(all="ignore"):
            tgr = np.where(o[:, 1] <= gy, 0.0, np.where(u[:, 1] < 0, (gy - o[:, 1]) / u[:, 1], np.inf))
        tgr = np.where(valid & (tgr <= mt), tgr, np.inf)
        ri = np.concatenate([ri, np.arange(n)])
        mi = np.concatenate([mi, np.full(n, -1)])
        ids = np.concatenate([ids, np.full(n, GROUND, np.int64)])
        t = np.concatenate([t, tgr])
    fin = np.isfinite(t)
    ri, mi, ids, t = ri[fin], mi[fin], ids[fin], t[fin]
    order = np.lexsort((ids, t, ri))
    ri, mi, ids, t = ri[order], mi[order], ids[order], t[order]
    first = np.ones(len(ri), bool)
    first[1:] = ri[1:] != ri[:-1]
    second = np.zeros(len(ri), bool)
    second[1:] = ~first[1:] & first[:-1]
    body = np.full(n, MISS, np.int64)
    tb, t2 = np.full(n, np.inf), np.full(n, np.inf)
    which = np.full(n, -1, np.int64)
    body[ri[first]], tb[ri[first]], which[ri[first]] = ids[first], t[first], mi[first]
    t2[ri[second]] = t[second]
    out = dict(body=body, t=tb, t2=t2, valid=valid, u=u, o=o, R=Rq, he=hq, which=which, tg=tg, ground=ground)
    normal, point = np.zeros((n, 3)), np.zeros((n, 3))
    for i in np.nonzero((body != MISS) & (tb > 0))[0]:
        normal[i], point[i] = contact(out, i, tb[i])
    t0 = (body != MISS) & (tb == 0)
    normal[t0] = -u[t0]
    out.update(normal=normal, point=point)
    return out


def _pair(h, i, t, k):
    tg = h["tg"]
    one = lambda x: np.asarray(x)[k:k + 1]
    return closest((h["o"][i] + t * h["u"][i])[None], h["R"][i][None], h["he"][i][None], one(tg["pos"]),
                   query_ref._frames(tg)[k:k + 1], one(tg["half_extent"]), one(tg["shape"]))


def contact(h, i, t, target=None):
    """(normal, point) of query i touching its target (default: the winner) with the centre at t > 0. The normal is the
    direction of the shortest vector from the target to the cast box; where the target has (nearly) no radius the two closest
    points coincide at the contact, and the direction is taken a little before it."""
    tg = h["tg"]
    o, u, R, he = h["o"][i], h["u"][i], h["R"][i], h["he"][i]
    k = h["which"][i] if target is None else target
    if k < 0:  # the ground: the lowest feature (corner; centre of a level edge or face) projected onto the plane
        c = o + t * u
        e = c - R @ (np.sign(R[1, :]) * he)
        return np.array([0.0, 1.0, 0.0]), np.array([e[0], h["ground"], e[2]])
    r = 0.0 if tg["shape"][k] == SHAPE_BOX else tg["half_extent"][k][0]
    te = t if r > 1e-4 else max(t - 1e-6, 0.0)
    q, p, d, _ = _pair(h, i, te, k)
    nrm = (q[0] - p[0]) / d[0] if d[0] > 0 else -u
    q, p, d, _ = _pair(h, i, t, k)
    return nrm, p[0] + r * nrm


def separation_at(h, i, t, k):
    """separation of query i with its centre at t from target row k (<= 0: touching)"""
    _, _, d, r = _pair(h, i, t, k)
    return float(d[0] - r[0])
