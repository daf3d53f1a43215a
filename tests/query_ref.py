"""Float64 brute force of the sphere-cast and overlap queries (include/physics_hip.h, phys_spherecast / phys_overlap),
written for the tests: every query against every target, numpy only. An independent restatement: the kernel grows the
targets and casts a ray; this reference walks the exact distance of the ball's centre to each target instead.

    hits = spherecast(origins, dirs, radius, targets, max_t=None, ignore=None, ground=None, centre=None)
    sets = overlap(shape_type, pos, rot, half_extent, targets, ignore=None, ground=None, centre=None)

targets = dict(pos (m, 3), rot (m, 4) [i, j, k, w], half_extent (m, 3), shape (m,), id (m,)): bodies and statics
together, each with the id the query reports (body index or STATIC_ID_BIT | k). ground = the plane height or None.
centre = a point subtracted in float64 from every query and target position (and its height from the ground) before
anything else: exact for float32 inputs, so that a scene far from the origin costs the reference no digits; the o of the
result and its targets (tg) are measured from it."""
import numpy as np

from raycast_ref import GROUND, MISS, rotation_matrices

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, 1, 2, 3
STATIC_ID_BIT = 0x80000000


def targets(bodies=None, statics=None):
    """bodies / statics: dicts of pos, rot, half_extent, shape (rot may be None). One target dict with their ids."""
    parts = []
    for d, base in ((bodies, 0), (statics, STATIC_ID_BIT)):
        if d is None or len(np.asarray(d["pos"]).reshape(-1, 3)) == 0:
            continue
        pos = np.asarray(d["pos"], np.float64).reshape(-1, 3)
        m = len(pos)
        rot = np.tile([0.0, 0.0, 0.0, 1.0], (m, 1)) if d.get("rot") is None else np.asarray(d["rot"], np.float64).reshape(-1, 4)
        parts.append(dict(pos=pos, rot=rot, half_extent=np.asarray(d["half_extent"], np.float64).reshape(-1, 3),
                          shape=np.asarray(d["shape"]).reshape(-1).astype(np.int64), id=base + np.arange(m, dtype=np.int64)))
    if not parts:
        return dict(pos=np.zeros((0, 3)), rot=np.zeros((0, 4)), half_extent=np.zeros((0, 3)), shape=np.zeros(0, np.int64),
                    id=np.zeros(0, np.int64))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _frames(t):
    R = rotation_matrices(t["rot"]) if len(t["pos"]) else np.zeros((0, 3, 3))
    return R


def point_dist(p, pos, R, he, shape):
    """Distance of points p (P, 3) to the closed shapes of PAIRS (arrays of length P); 0 inside."""
    d = p - pos
    out = np.full(len(p), np.inf)
    sph = shape == SHAPE_SPHERE
    out[sph] = np.linalg.norm(d[sph], axis=1) - he[sph, 0]
    cap = shape == SHAPE_CAPSULE
    if cap.any():
        w = R[cap][:, :, 1]
        hl = he[cap, 1]
        s = np.clip((d[cap] * w).sum(1), -hl, hl)
        out[cap] = np.linalg.norm(d[cap] - s[:, None] * w, axis=1) - he[cap, 0]
    box = shape == SHAPE_BOX
    if box.any():
        l = np.einsum("pj,pjk->pk", d[box], R[box])
        g = np.maximum(np.abs(l) - he[box], 0.0)
        out[box] = np.linalg.norm(g, axis=1)
    return np.maximum(out, 0.0)


def closest_normal(p, pos, R, he, shape):
    """Unit direction from the shape's closest point to p (p outside the shape)."""
    d = p - pos
    if shape == SHAPE_SPHERE:
        v = d
    elif shape == SHAPE_CAPSULE:
        w = R[:, 1]
        v = d - np.clip(d @ w, -he[1], he[1]) * w
    else:
        l = R.T @ d
        v = R @ (l - np.clip(l, -he, he))
    return v / np.linalg.norm(v)


def _bound(he, shape):
    return np.where(shape == SHAPE_SPHERE, he[:, 0],
                    np.where(shape == SHAPE_CAPSULE, he[:, 0] + he[:, 1], np.linalg.norm(he, axis=1)))


def _centred(tg, centre, ground):
    c = np.asarray(centre, np.float64).reshape(3)
    return c, dict(tg, pos=np.asarray(tg["pos"], np.float64) - c), None if ground is None else ground - c[1]


def spherecast(origins, dirs, radius, tg, max_t=None, ignore=None, ground=None, iters=80, centre=None):
    """Per ball: dict(body, t, normal, t2 = second-best t, valid). The first t with dist(centre(t), target) <= radius:
    the distance along a line is convex, so a golden-section search finds its minimum and a bisection the first touch."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    dv = np.asarray(dirs, np.float64).reshape(-1, 3)
    if centre is not None:
        c, tg, ground = _centred(tg, centre, ground)
        o = o - c
    n = len(o)
    rad = np.broadcast_to(np.asarray(radius, np.float64), (n,)).copy()
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(dv, axis=1)
        valid = np.isfinite(o).all(1) & np.isfinite(dv).all(1) & (ln > 0) & np.isfinite(ln) & (rad >= 0) & np.isfinite(rad)
        u = np.where(valid[:, None], dv / np.where(valid, ln, 1.0)[:, None], 0.0)
    mt = np.full(n, np.inf) if max_t is None else np.asarray(max_t, np.float64).reshape(-1)
    ig = np.full(n, -1, np.int64) if ignore is None else np.asarray(ignore, np.int64).reshape(-1)
    valid &= mt >= 0
    R = _frames(tg)
    m = len(tg["pos"])
    b = _bound(tg["half_extent"], tg["shape"]) if m else np.zeros(0)
    shaped = np.isin(tg["shape"], (SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE)) if m else np.zeros(0, bool)
    # candidate pairs: the centre line passes within bound + radius of the target's centre
    ri, mi = np.nonzero(valid[:, None] & shaped[None, :]) if m else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    rel = tg["pos"][mi] - o[ri]
    along = (rel * u[ri]).sum(1)
    perp = np.linalg.norm(rel - along[:, None] * u[ri], axis=1)
    reach = b[mi] + rad[ri] + 1e-9
    keep = (perp <= reach) & ((along >= -reach) | (np.linalg.norm(rel, axis=1) <= reach)) & (tg["id"][mi] != ig[ri])
    ri, mi = ri[keep], mi[keep]
    pos, Rm, he, sh = tg["pos"][mi], R[mi], tg["half_extent"][mi], tg["shape"][mi]
    oo, uu, rr = o[ri], u[ri], rad[ri]
    f = lambda t: point_dist(oo + t[:, None] * uu, pos, Rm, he, sh) - rr
    t = np.full(len(ri), np.inf)
    f0 = f(np.zeros(len(ri)))
    t[f0 <= 0] = 0.0
    todo = f0 > 0
    # minimum on [0, T]: past the closest approach of the centre the distance only grows
    lo = np.zeros(len(ri))
    hi = np.maximum(np.linalg.norm(pos - oo, axis=1) + b[mi] + rr + 1.0, 1.0)
    g = (np.sqrt(5.0) - 1.0) / 2.0
    a, c = lo.copy(), hi.copy()
    for _ in range(iters):
        m1, m2 = c - g * (c - a), a + g * (c - a)
        left = f(m1) <= f(m2)
        c = np.where(left, m2, c)
        a = np.where(left, a, m1)
    tmin = 0.5 * (a + c)
    touch = todo & (f(tmin) <= 1e-12)
    a, c = np.zeros(len(ri)), tmin.copy()
    for _ in range(iters):
        mid = 0.5 * (a + c)
        inside = f(mid) <= 0
        c = np.where(inside, mid, c)
        a = np.where(inside, a, mid)
    t[touch] = c[touch]
    t[t > mt[ri]] = np.inf
    ids = tg["id"][mi]
    if ground is not None:
        gy = ground + rad
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
    tb = np.full(n, np.inf)
    t2 = np.full(n, np.inf)
    which = np.full(n, -1, np.int64)
    body[ri[first]], tb[ri[first]], which[ri[first]] = ids[first], t[first], mi[first]
    t2[ri[second]] = t[second]
    normal = np.zeros((n, 3))
    for i in np.nonzero(body != MISS)[0]:
        if tb[i] == 0:
            normal[i] = -u[i]
        elif body[i] == GROUND:
            normal[i] = (0.0, 1.0, 0.0)
        else:
            k = which[i]
            normal[i] = closest_normal(o[i] + tb[i] * u[i], tg["pos"][k], R[k], tg["half_extent"][k], tg["shape"][k])
    return dict(body=body, t=tb, normal=normal, t2=t2, valid=valid, u=u, o=o, which=which, tg=tg)


def _seg(pos, R, he, shape):
    """core segment (centre, unit axis, half-length) and radius of a sphere or capsule"""
    if shape == SHAPE_CAPSULE:
        return pos, R[:, 1], he[1], he[0]
    return pos, np.array([0.0, 1.0, 0.0]), 0.0, he[0]


def _golden(fn, lo, hi, iters=100):
    g = (np.sqrt(5.0) - 1.0) / 2.0
    a, c = lo, hi
    for _ in range(iters):
        m1, m2 = c - g * (c - a), a + g * (c - a)
        if fn(m1) <= fn(m2):
            c = m2
        else:
            a = m1
    return fn(0.5 * (a + c))


def _seg_point(c, w, hl, p):
    s = np.clip((p - c) @ w, -hl, hl)
    return np.linalg.norm(p - c - s * w)


def _seg_seg(ca, ua, ha, cb, ub, hb):
    return _golden(lambda s: _seg_point(cb, ub, hb, ca + s * ua), -ha, ha) if ha > 0 else _seg_point(cb, ub, hb, ca)


def _seg_box(c, w, hl, bpos, R, he):
    def dist(s):
        l = R.T @ (c + s * w - bpos)
        return np.linalg.norm(np.maximum(np.abs(l) - he, 0.0))
    return _golden(dist, -hl, hl) if hl > 0 else dist(0.0)


def _box_gap(pa, Ra, ha, pb, Rb, hb):
    """the largest separating-axis gap over the 15 axes (> 0: separated; its sign is exact, SAT)"""
    t = pb - pa
    axes = [Ra[:, i] for i in range(3)] + [Rb[:, j] for j in range(3)]
    for i in range(3):
        for j in range(3):
            a = np.cross(Ra[:, i], Rb[:, j])
            nrm = np.linalg.norm(a)
            if nrm > 1e-9:
                axes.append(a / nrm)
    best = -np.inf
    for L in axes:
        ra = np.abs(Ra.T @ L) @ ha
        rb = np.abs(Rb.T @ L) @ hb
        best = max(best, abs(t @ L) - ra - rb)
    return best


def separation(qs, qp, qR, qh, ts, tp, tR, th):
    """Signed separation of two closed shapes: > 0 apart, <= 0 touching or overlapping (a gap for the near-touch count,
    exact in sign)."""
    if qs == SHAPE_BOX and ts == SHAPE_BOX:
        return _box_gap(qp, qR, qh, tp, tR, th)
    if qs != SHAPE_BOX and ts != SHAPE_BOX:
        ca, ua, ha, ra = _seg(qp, qR, qh, qs)
        cb, ub, hb, rb = _seg(tp, tR, th, ts)
        return _seg_seg(ca, ua, ha, cb, ub, hb) - ra - rb
    if qs == SHAPE_BOX:
        qs, qp, qR, qh, ts, tp, tR, th = ts, tp, tR, th, qs, qp, qR, qh
    c, w, hl, r = _seg(qp, qR, qh, qs)
    return _seg_box(c, w, hl, tp, tR, th) - r


def lowest(shape, pos, R, he):
    if shape == SHAPE_SPHERE:
        return pos[1] - he[0]
    if shape == SHAPE_CAPSULE:
        return pos[1] - abs(R[1, 1]) * he[1] - he[0]
    return pos[1] - np.abs(R[1]) @ he


def overlap(shape_type, pos, rot, half_extent, tg, ignore=None, ground=None, centre=None):
    """Per query: (sorted list of ids, dict id -> separation of the pairs within 1e-3 of touching, both sides)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    if centre is not None:
        c, tg, ground = _centred(tg, centre, ground)
        pos = pos - c
    n = len(pos)
    st = np.broadcast_to(np.asarray(shape_type), (n,))
    he = np.broadcast_to(np.asarray(half_extent, np.float64).reshape(-1, 3), (n, 3))
    rot = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rot is None else np.asarray(rot, np.float64).reshape(-1, 4)
    ig = np.full(n, -1, np.int64) if ignore is None else np.asarray(ignore, np.int64).reshape(-1)
    Rq = rotation_matrices(rot) if n else np.zeros((0, 3, 3))
    Rt = _frames(tg)
    m = len(tg["pos"])
    bt = _bound(tg["half_extent"], tg["shape"]) if m else np.zeros(0)
    out = []
    for i in range(n):
        ids, near = [], {}
        ok = st[i] in (SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE) and np.isfinite(pos[i]).all() and np.isfinite(he[i]).all() \
            and np.isfinite(rot[i]).all() and (he[i] >= 0).all()
        if not ok:
            out.append((ids, near))
            continue
        bq = _bound(he[i:i + 1], np.asarray([st[i]]))[0]
        close = np.nonzero(np.linalg.norm(tg["pos"] - pos[i], axis=1) <= bq + bt + 1e-3)[0] if m else []
        for k in close:
            if tg["shape"][k] not in (SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE) or tg["id"][k] == ig[i]:
                continue
            s = separation(st[i], pos[i], Rq[i], he[i], tg["shape"][k], tg["pos"][k], Rt[k], tg["half_extent"][k])
            if s <= 0:
                ids.append(int(tg["id"][k]))
            if abs(s) <= 1e-3:
                near[int(tg["id"][k])] = s
        if ground is not None:
            s = lowest(st[i], pos[i], Rq[i], he[i]) - ground
            if s <= 0:
                ids.append(GROUND)
            if abs(s) <= 1e-3:
                near[GROUND] = s
        out.append((sorted(ids), near))
    return out
