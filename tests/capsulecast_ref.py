"""Float64 brute force of the capsule cast (include/physics_hip.h, phys_capsulecast), written for the tests: every query
against every target, numpy only. An independent restatement: the kernel casts a ray at the Minkowski sum of the target
and the capsule; this reference walks the exact distance of the capsule's core to the target instead, as
query_ref.spherecast does for a ball.

    h = capsulecast(origins, dirs, rot, radius, half_length, targets, max_t=None, ignore=None, ground=None, centre=None)

targets, ground, centre: as in query_ref. Per query: body, t, t2 (the second-best t), normal, point, valid, and o, u, a
(origin, unit direction and unit axis, measured from the centre), which (the winning target's row), tg.

separation(t) = distance(core at o + t u, target's core or box) - (r + R) is convex in t (the distance of two convex sets
under a translation), so a golden section finds its minimum and a bisection the first t with separation <= 0. The
distances are exact closed forms over the features of a segment and of a box (end points, edges), checked against nested
golden sections in tests/test_capsulecast_cpu.py; the normal and the point come from the closest pair."""
import numpy as np

import query_ref
from query_ref import SHAPE_BOX, SHAPE_CAPSULE, SHAPE_SPHERE
from raycast_ref import GROUND, MISS, rotation_matrices


def _dot(a, b):
    return (a * b).sum(-1)


def _on_seg(p, c, w, hl):
    """closest point of the segment c +- hl w to p (rows)"""
    return c + np.clip(_dot(p - c, w), -hl, hl)[:, None] * w


def seg_seg_closest(c1, u1, h1, c2, u2, h2):
    """Closest points (q on segment 1, p on segment 2) of c1 +- h1 u1 and c2 +- h2 u2, rows of unit axes: the least of the
    four end points against the other segment and, where it lies inside both, the crossing of the two lines."""
    n = len(c1)
    qs, ps = [], []
    for sg in (-1.0, 1.0):
        e = c1 + sg * h1[:, None] * u1
        qs.append(e); ps.append(_on_seg(e, c2, u2, h2))
        e = c2 + sg * h2[:, None] * u2
        qs.append(_on_seg(e, c1, u1, h1)); ps.append(e)
    r = c1 - c2
    b, c, f = _dot(u1, u2), _dot(u1, r), _dot(u2, r)
    x = np.cross(u1, u2)
    den = _dot(x, x)
    with np.errstate(all="ignore"):
        s, t = (b * f - c) / den, (f - b * c) / den
    ok = (den > 1e-14) & (np.abs(s) <= h1) & (np.abs(t) <= h2)
    s, t = np.where(ok, s, 0.0), np.where(ok, t, 0.0)
    qs.append(c1 + s[:, None] * u1); ps.append(c2 + t[:, None] * u2)
    q, p = np.stack(qs), np.stack(ps)  # (5, n, 3)
    d = np.linalg.norm(q - p, axis=2)
    d[4, ~ok] = np.inf
    k = d.argmin(0)
    idx = np.arange(n)
    return q[k, idx], p[k, idx], d[k, idx]


def seg_box_closest(c, w, hl, he):
    """Closest points (q on the segment c +- hl w, p on the box [-he, he]) in the box frame, rows: 0 where the segment
    crosses the box, otherwise the least of its end points against the box and of the segment against the twelve edges."""
    n = len(c)
    lo, hi = -hl.copy(), hl.copy()
    miss = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            par = w[:, a] == 0
            t0, t1 = (-he[:, a] - c[:, a]) / w[:, a], (he[:, a] - c[:, a]) / w[:, a]
            miss |= par & (np.abs(c[:, a]) > he[:, a])
            lo = np.where(par, lo, np.maximum(lo, np.minimum(t0, t1)))
            hi = np.where(par, hi, np.minimum(hi, np.maximum(t0, t1)))
    cross = ~miss & (lo <= hi)
    qs, ps = [], []
    for sg in (-1.0, 1.0):
        e = c + sg * hl[:, None] * w
        qs.append(e); ps.append(np.clip(e, -he, he))
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        eu = np.zeros((n, 3)); eu[:, ax] = 1.0
        for s1 in (-1.0, 1.0):
            for s2 in (-1.0, 1.0):
                ec = np.zeros((n, 3)); ec[:, o1] = s1 * he[:, o1]; ec[:, o2] = s2 * he[:, o2]
                q, p, _ = seg_seg_closest(c, w, hl, ec, eu, he[:, ax])
                qs.append(q); ps.append(p)
    q, p = np.stack(qs), np.stack(ps)
    d = np.linalg.norm(q - p, axis=2)
    k = d.argmin(0)
    idx = np.arange(n)
    q, p, d = q[k, idx], p[k, idx], d[k, idx]
    mid = c + (0.5 * (lo + hi))[:, None] * w
    q, p, d = np.where(cross[:, None], mid, q), np.where(cross[:, None], mid, p), np.where(cross, 0.0, d)
    return q, p, d


def closest(c, a, hl, pos, R, he, shape):
    """Rows of pairs: the query core c +- hl a against the target (pos, R, he, shape). Returns (q on the query's core, p on
    the target's core or box, their distance, the target's radius), world frame."""
    n = len(c)
    q, p, d, r = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, np.inf), np.zeros(n)
    rel = c - pos
    zero = np.zeros((n, 3))
    rnd = (shape == SHAPE_SPHERE) | (shape == SHAPE_CAPSULE)
    if rnd.any():
        w = R[rnd][:, :, 1]
        k = np.where(shape[rnd] == SHAPE_CAPSULE, he[rnd, 1], 0.0)
        qq, pp, dd = seg_seg_closest(rel[rnd], a[rnd], hl[rnd], zero[rnd], w, k)
        q[rnd], p[rnd], d[rnd], r[rnd] = qq + pos[rnd], pp + pos[rnd], dd, he[rnd, 0]
    box = shape == SHAPE_BOX
    if box.any():
        Rb = R[box]
        l = np.einsum("pj,pjk->pk", rel[box], Rb)
        al = np.einsum("pj,pjk->pk", a[box], Rb)
        qq, pp, dd = seg_box_closest(l, al, hl[box], he[box])
        q[box] = np.einsum("pjk,pk->pj", Rb, qq) + pos[box]
        p[box] = np.einsum("pjk,pk->pj", Rb, pp) + pos[box]
        d[box] = dd
    return q, p, d, r


def capsulecast(origins, dirs, rot, radius, half_length, tg, max_t=None, ignore=None, ground=None, centre=None, iters=56):
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    dv = np.asarray(dirs, np.float64).reshape(-1, 3)
    if centre is not None:
        c, tg, ground = query_ref._centred(tg, centre, ground)
        o = o - c
    n = len(o)
    rad = np.broadcast_to(np.asarray(radius, np.float64), (n,)).copy()
    hq = np.broadcast_to(np.asarray(half_length, np.float64), (n,)).copy()
    q4 = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rot is None else np.asarray(rot, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(dv, axis=1)
        valid = np.isfinite(o).all(1) & np.isfinite(dv).all(1) & (ln > 0) & np.isfinite(ln) & np.isfinite(q4).all(1) \
            & (rad >= 0) & np.isfinite(rad) & (hq >= 0) & np.isfinite(hq)
        u = np.where(valid[:, None], dv / np.where(valid, ln, 1.0)[:, None], 0.0)
        a = rotation_matrices(np.where(valid[:, None], q4, [0.0, 0.0, 0.0, 1.0]))[:, :, 1] if n else np.zeros((0, 3))
    mt = np.full(n, np.inf) if max_t is None else np.asarray(max_t, np.float64).reshape(-1)
    ig = np.full(n, -1, np.int64) if ignore is None else np.asarray(ignore, np.int64).reshape(-1)
    valid &= mt >= 0
    rad, hq = np.where(valid, rad, 0.0), np.where(valid, hq, 0.0)
    m = len(tg["pos"])
    R = query_ref._frames(tg)
    b = query_ref._bound(tg["half_extent"], tg["shape"]) if m else np.zeros(0)
    shaped = np.isin(tg["shape"], (SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE)) if m else np.zeros(0, bool)
    ri, mi = np.nonzero(valid[:, None] & shaped[None, :]) if m else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    rel = tg["pos"][mi] - o[ri]
    along = _dot(rel, u[ri])
    perp = np.linalg.norm(rel - along[:, None] * u[ri], axis=1)
    reach = b[mi] + rad[ri] + hq[ri] + 1e-9
    keep = (perp <= reach) & ((along >= -reach) | (np.linalg.norm(rel, axis=1) <= reach)) & (tg["id"][mi] != ig[ri])
    ri, mi = ri[keep], mi[keep]
    pos, Rm, he, sh = tg["pos"][mi], R[mi], tg["half_extent"][mi], tg["shape"][mi]
    oo, uu, aa, rr, hh = o[ri], u[ri], a[ri], rad[ri], hq[ri]

    def f(t, sel):
        _, _, d, r = closest(oo[sel] + t[:, None] * uu[sel], aa[sel], hh[sel], pos[sel], Rm[sel], he[sel], sh[sel])
        return d - (r + rr[sel])

    k = len(ri)
    t = np.full(k, np.inf)
    f0 = f(np.zeros(k), np.arange(k))
    t[f0 <= 0] = 0.0
    # the minimum over [0, T] for the pairs that start apart: past the closest approach the distance only grows
    todo = np.nonzero(f0 > 0)[0]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    lo_t = np.zeros(len(todo))
    hi_t = np.maximum(np.linalg.norm(pos[todo] - oo[todo], axis=1) + b[mi[todo]] + rr[todo] + hh[todo] + 1.0, 1.0)
    for _ in range(iters):
        m1, m2 = hi_t - g * (hi_t - lo_t), lo_t + g * (hi_t - lo_t)
        left = f(m1, todo) <= f(m2, todo)
        hi_t = np.where(left, m2, hi_t)
        lo_t = np.where(left, lo_t, m1)
    tmin = 0.5 * (lo_t + hi_t)
    # (1e-9: two cores that cross at r + R = 0 touch at one t, where the distance is a V the search has found to 1e-10;
    # the bisection then keeps that t)
    reach = f(tmin, todo) <= 1e-9
    touch, lo_t, hi_t = todo[reach], np.zeros(int(reach.sum())), tmin[reach]
    for _ in range(iters):
        mid = 0.5 * (lo_t + hi_t)
        inside = f(mid, touch) <= 0
        hi_t = np.where(inside, mid, hi_t)
        lo_t = np.where(inside, lo_t, mid)
    t[touch] = hi_t
    t[t > mt[ri]] = np.inf
    ids = tg["id"][mi]
    if ground is not None:
        gy = ground + rad + hq * np.abs(a[:, 1])
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
    out = dict(body=body, t=tb, t2=t2, valid=valid, u=u, o=o, a=a, rad=rad, hq=hq, which=which, tg=tg, ground=ground)
    normal, point = np.zeros((n, 3)), np.zeros((n, 3))
    for i in np.nonzero((body != MISS) & (tb > 0))[0]:
        normal[i], point[i] = contact(out, i, tb[i])
    t0 = (body != MISS) & (tb == 0)
    normal[t0] = -u[t0]
    out.update(normal=normal, point=point)
    return out


def contact(h, i, t, target=None):
    """(normal, point) of query i touching its target (default: the winner) with the centre at t > 0. Where r + R is
    (nearly) zero the two closest points coincide at the contact: the direction is taken a little before it."""
    tg = h["tg"]
    o, u, a = h["o"][i], h["u"][i], h["a"][i]
    k = h["which"][i] if target is None else target
    if k < 0:  # the ground: the lower end of the core (the centre for a level one) projected onto the plane
        c = o + t * u
        e = c - np.sign(a[1]) * h["hq"][i] * a
        return np.array([0.0, 1.0, 0.0]), np.array([e[0], h["ground"], e[2]])
    one = lambda x: np.asarray(x)[k:k + 1]
    Rk = query_ref._frames(tg)[k:k + 1]
    rho = h["rad"][i] + (0.0 if tg["shape"][k] == SHAPE_BOX else tg["half_extent"][k][0])
    te = t if rho > 1e-4 else max(t - 1e-6, 0.0)
    q, p, d, r = closest((o + te * u)[None], a[None], h["hq"][i:i + 1], one(tg["pos"]), Rk, one(tg["half_extent"]), one(tg["shape"]))
    nrm = (q[0] - p[0]) / d[0] if d[0] > 0 else -u
    q, p, d, r = closest((o + t * u)[None], a[None], h["hq"][i:i + 1], one(tg["pos"]), Rk, one(tg["half_extent"]), one(tg["shape"]))
    return nrm, p[0] + r[0] * nrm


def separation_at(h, i, t, k):
    """separation of query i with its centre at t from target row k (<= 0: touching)"""
    tg = h["tg"]
    one = lambda x: np.asarray(x)[k:k + 1]
    _, _, d, r = closest((h["o"][i] + t * h["u"][i])[None], h["a"][i][None], h["hq"][i:i + 1], one(tg["pos"]),
                         query_ref._frames(tg)[k:k + 1], one(tg["half_extent"]), one(tg["shape"]))
    return float(d[0] - r[0] - h["rad"][i])
