"""Float64 brute force of the ray-cast query (include/physics_hip.h, phys_raycast), written for the tests: every ray
against every body, with the header's semantics. numpy only.

    hits = cast(origins, dirs, bodies, max_t=None, ignore=None, ground=None, statics=None, centre=None)

bodies = dict(pos (m, 3), rot (m, 4) [i, j, k, w], half_extent (m, 3), shape (m,)): spheres, boxes and capsules (radius
half_extent[0], core half-length half_extent[1] along the local y axis); statics = the same for the static colliders
(rot may be None), further targets with the ids STATIC_ID_BIT | k that ignore never names; ground = the plane height or
None; centre = a point subtracted in float64 from every origin and position (and its height from the ground) before
anything else: exact for float32 inputs, so a scene far from the origin costs the reference no digits, and o, pos and
|o| of the result are measured from it.
Returns a dict of per-ray arrays: body (MISS / GROUND / id), t (+inf on a miss), normal (zero on a miss), t2 (the
second-best t over every target, +inf if none), span (length of the best target's interval along the ray: short =
grazing) and valid (direction and origin usable); and the targets (pos, R, he, shape, ids: row k of a body is k, of
static k it is n_bodies + k)."""
import numpy as np

MISS = 0xFFFFFFFE
GROUND = 0xFFFFFFFF
SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, 1, 2, 3
STATIC_ID_BIT = 0x80000000


def rotation_matrices(rot):
    """World = R @ local for quaternions [i, j, k, w] (normalised here)."""
    q = np.asarray(rot, np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    i, j, k, w = q.T
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (j * j + k * k); R[:, 0, 1] = 2 * (i * j - w * k); R[:, 0, 2] = 2 * (i * k + w * j)
    R[:, 1, 0] = 2 * (i * j + w * k); R[:, 1, 1] = 1 - 2 * (i * i + k * k); R[:, 1, 2] = 2 * (j * k - w * i)
    R[:, 2, 0] = 2 * (i * k - w * j); R[:, 2, 1] = 2 * (j * k + w * i); R[:, 2, 2] = 1 - 2 * (i * i + j * j)
    return R


def _unit(origins, dirs):
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        n = np.linalg.norm(d, axis=1)
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (n > 0) & np.isfinite(n)
        u = np.where(valid[:, None], d / np.where(valid, n, 1.0)[:, None], 0.0)
    return o, u, valid


def _intersect(o, u, pos, R, he, shape):
    """(t, span) of ray-body PAIRS (arrays of equal length P): t = inf where missed, span = length of the pair's interval
    along the ray (short: a grazing ray)."""
    p = o - pos
    t = np.full(len(p), np.inf)
    span = np.zeros(len(p))
    with np.errstate(all="ignore"):
        sph = shape == SHAPE_SPHERE
        if sph.any():
            ps, us = p[sph], u[sph]
            rad = he[sph, 0]
            b = (ps * us).sum(1)
            cc = (ps * ps).sum(1) - rad * rad
            l = ps - b[:, None] * us
            disc = rad * rad - (l * l).sum(1)
            inside = cc <= 0
            hit = inside | ((b < 0) & (disc >= 0))
            ts = np.where(inside, 0.0, cc / (-b + np.sqrt(np.maximum(disc, 0))))
            t[sph] = np.where(hit, ts, np.inf)
            span[sph] = np.where(hit, 2 * np.sqrt(np.maximum(disc, 0)), 0.0)
        box = shape == SHAPE_BOX
        if box.any():
            Rb = R[box]
            pl = np.einsum("pj,pjk->pk", p[box], Rb)  # R^T p
            dl = np.einsum("pj,pjk->pk", u[box], Rb)
            h = he[box]
            par = dl == 0
            a = (-h - pl) / np.where(par, 1.0, dl)
            c = (h - pl) / np.where(par, 1.0, dl)
            lo = np.where(par, np.where(np.abs(pl) <= h, -np.inf, np.inf), np.minimum(a, c))
            hi = np.where(par, np.where(np.abs(pl) <= h, np.inf, -np.inf), np.maximum(a, c))
            tn, tf = lo.max(1), hi.min(1)
            inside = (np.abs(pl) <= h).all(1)
            hit = inside | ((tn <= tf) & (tn >= 0))
            t[box] = np.where(hit, np.where(inside, 0.0, tn), np.inf)
            span[box] = np.where(hit, tf - np.maximum(tn, 0), 0.0)
        cap = shape == SHAPE_CAPSULE
        if cap.any():
            pc, uc, w, r, hl = p[cap], u[cap], R[cap][:, :, 1], he[cap, 0], he[cap, 1]
            tin = _capsule_entry(pc, uc, w, r, hl)
            # the capsule is convex: its interval ends where the reversed ray, started beyond it, enters
            far = np.linalg.norm(pc, axis=1) + r + hl + 1.0
            tout = far - _capsule_entry(pc + far[:, None] * uc, -uc, w, r, hl)
            t[cap] = tin
            span[cap] = np.where(np.isfinite(tin) & np.isfinite(tout), np.maximum(tout - tin, 0.0), 0.0)
    return t, span


def _capsule_entry(p, u, w, r, hl):
    """First t >= 0 at which the ray p + t u (u unit, p relative to the centre) is inside the closed capsule of radius r
    around the core +- hl w: 0 from inside, else the least of the closed-form roots of the cylinder's side (kept where the
    hit lies between the end planes) and of the two end balls; inf on a miss."""
    pd, ud = (p * w).sum(1), (u * w).sum(1)
    s = np.clip(pd, -hl, hl)
    inside = np.linalg.norm(p - s[:, None] * w, axis=1) <= r
    t = np.full(len(p), np.inf)
    a, b = u - ud[:, None] * w, p - pd[:, None] * w
    A, B, C = (a * a).sum(1), (a * b).sum(1), (b * b).sum(1) - r * r
    disc = B * B - A * C
    ok = (A > 1e-24) & (disc >= 0)
    ts = (-B - np.sqrt(np.where(ok, disc, 0.0))) / np.where(ok, A, 1.0)
    ok &= (ts >= 0) & (np.abs(pd + ts * ud) <= hl)
    t = np.where(ok, ts, t)
    for end in (-1.0, 1.0):
        pe = p - (end * hl)[:, None] * w
        bb, cc = (pe * u).sum(1), (pe * pe).sum(1) - r * r
        disc = bb * bb - cc
        te = -bb - np.sqrt(np.maximum(disc, 0.0))
        t = np.where((disc >= 0) & (te >= 0), np.minimum(t, te), t)
    return np.where(inside, 0.0, t)


def normal_of(o, u, t, pos, R, he, shape):
    """Outward normal(s) of one hit: a list of acceptable unit normals (several at a box edge or corner: every face whose
    plane the hit point lies within 1e-4 of; -u for an origin inside)."""
    if t == 0:
        return [-u]
    hp = o + t * u - pos
    if shape == SHAPE_SPHERE:
        return [hp / np.linalg.norm(hp)]
    if shape == SHAPE_CAPSULE:  # from the closest point of the core to the hit
        w = R[:, 1]
        v = hp - np.clip(hp @ w, -he[1], he[1]) * w
        return [v / np.linalg.norm(v)]
    l = R.T @ hp
    out = []
    for a in range(3):
        if abs(abs(l[a]) - he[a]) <= 1e-4:
            out.append(R[:, a] * np.sign(l[a]))
    if not out:  # numerically deepest face
        a = int(np.argmax(np.abs(l) / np.maximum(he, 1e-30)))
        out.append(R[:, a] * np.sign(l[a]))
    return out


def _targets(bodies, statics):
    """bodies then statics as one set of targets: pos, rot, half_extent, shape, ids"""
    parts = []
    for d, base in ((bodies, 0), (statics, STATIC_ID_BIT)):
        if d is None:
            continue
        pos = np.asarray(d["pos"], np.float64).reshape(-1, 3)
        k = len(pos)
        rot = np.tile([0.0, 0.0, 0.0, 1.0], (k, 1)) if d.get("rot") is None else np.asarray(d["rot"], np.float64).reshape(-1, 4)
        parts.append((pos, rot, np.asarray(d["half_extent"], np.float64).reshape(-1, 3),
                      np.asarray(d["shape"]).reshape(-1).astype(np.int64), base + np.arange(k, dtype=np.int64)))
    return [np.concatenate(x) for x in zip(*parts)]


def cast(origins, dirs, bodies, max_t=None, ignore=None, ground=None, chunk_elems=4_000_000, statics=None, centre=None):
    o, u, valid = _unit(origins, dirs)
    n = len(o)
    pos, rot, he, shape, ids = _targets(bodies, statics)
    m = len(pos)
    n_bodies = len(np.asarray(bodies["pos"]).reshape(-1, 3))
    if centre is not None:
        c = np.asarray(centre, np.float64).reshape(3)
        o, pos = o - c, pos - c
        ground = None if ground is None else ground - c[1]
    R = rotation_matrices(rot) if m else np.zeros((0, 3, 3))
    mt = np.full(n, np.inf) if max_t is None else np.asarray(max_t, np.float64).reshape(-1)
    ig = np.full(n, -1, np.int64) if ignore is None else np.asarray(ignore, np.int64).reshape(-1)
    ig = np.where(ig < n_bodies, ig, -1)  # names a body or nothing
    ok = valid & (mt >= 0)
    # candidates: rays passing within the bounding sphere of a body (two matrix products per chunk of rays), then the
    # exact test on those pairs only
    rad = np.where(shape == SHAPE_SPHERE, he[:, 0], np.where(shape == SHAPE_CAPSULE, he[:, 0] + he[:, 1], np.linalg.norm(he, axis=1)))
    rad = np.where((shape == SHAPE_SPHERE) | (shape == SHAPE_BOX) | (shape == SHAPE_CAPSULE), rad, -1.0)
    cc = (pos * pos).sum(1)
    ri_all, mi_all = [], []
    step = max(1, chunk_elems // max(m, 1))
    for s in range(0, n if m else 0, step):
        e = min(n, s + step)
        oo, uu = np.where(ok[s:e, None], o[s:e], 0.0), u[s:e]
        b = (oo * uu).sum(1)[:, None] - uu @ pos.T  # (o - c).u: > 0 moving away from the centre
        pp = (oo * oo).sum(1)[:, None] - 2 * (oo @ pos.T) + cc[None, :]  # |o - c|^2
        d2 = pp - b * b
        # (the expanded square is good to a few ulp of |o|^2 + |c|^2: far-flung targets keep their candidates)
        slack = 1e-9 * (pp + 1.0) + 1e-6 + 1e-14 * ((oo * oo).sum(1)[:, None] + cc[None, :])
        cand = (rad[None, :] >= 0) & (d2 <= (rad * 1.001)[None, :] ** 2 + slack) & ((b <= 0) | (pp <= (rad * 1.001)[None, :] ** 2 + slack))
        cand &= ok[s:e, None]
        r_, m_ = np.nonzero(cand)
        ri_all.append(r_ + s)
        mi_all.append(m_)
    ri = np.concatenate(ri_all) if ri_all else np.zeros(0, np.int64)
    mi = np.concatenate(mi_all) if mi_all else np.zeros(0, np.int64)
    t, span = _intersect(o[ri], u[ri], pos[mi], R[mi], he[mi], shape[mi])
    tid = ids[mi]
    t[(t > mt[ri]) | (ig[ri] == tid)] = np.inf
    # the ground as one more target, id GROUND (larger than every body id: it loses ties)
    if ground is not None:
        with np.errstate(all="ignore"):
            tg = np.where(o[:, 1] <= ground, 0.0, np.where(u[:, 1] < 0, (ground - o[:, 1]) / u[:, 1], np.inf))
        tg = np.where(ok & (tg <= mt), tg, np.inf)
        ri = np.concatenate([ri, np.arange(n)])
        mi = np.concatenate([mi, np.full(n, -1, np.int64)])
        tid = np.concatenate([tid, np.full(n, GROUND, np.int64)])
        t = np.concatenate([t, tg])
        span = np.concatenate([span, np.full(n, np.inf)])
    keep = np.isfinite(t)
    ri, mi, tid, t, span = ri[keep], mi[keep], tid[keep], t[keep], span[keep]
    order = np.lexsort((tid, t, ri))
    ri, mi, tid, t, span = ri[order], mi[order], tid[order], t[order], span[order]
    first = np.ones(len(ri), bool)
    first[1:] = ri[1:] != ri[:-1]
    second = np.zeros(len(ri), bool)
    second[1:] = ~first[1:] & first[:-1]
    body = np.full(n, MISS, np.int64)
    tb = np.full(n, np.inf)
    t2 = np.full(n, np.inf)
    sp = np.zeros(n)
    row = np.full(n, -1, np.int64)
    body[ri[first]], tb[ri[first]], sp[ri[first]], row[ri[first]] = tid[first], t[first], span[first], mi[first]
    t2[ri[second]] = t[second]
    normal = np.zeros((n, 3))
    for i in np.nonzero(body != MISS)[0]:
        if body[i] == GROUND:
            normal[i] = -u[i] if tb[i] == 0 else (0.0, 1.0, 0.0)
        else:
            k = row[i]
            normal[i] = normal_of(o[i], u[i], tb[i], pos[k], R[k], he[k], shape[k])[0]
    return dict(body=body, t=tb, normal=normal, t2=t2, span=sp, valid=valid, u=u, o=o, R=R, pos=pos, he=he, shape=shape, ids=ids,
                n_bodies=n_bodies, ground=ground)


def row_of(hits, target_id):
    """Row of a body or static id in the hits' target arrays (pos, R, he, shape)."""
    return int(target_id) if target_id < STATIC_ID_BIT else hits["n_bodies"] + (int(target_id) - STATIC_ID_BIT)


def t_of(hits, ray, body_id):
    """Float64 t of ray `ray` against body `body_id` (inf on a miss), for judging a different id."""
    o, u = hits["o"][ray:ray + 1], hits["u"][ray:ray + 1]
    b = row_of(hits, body_id)
    t, _ = _intersect(o, u, hits["pos"][b:b + 1], hits["R"][b:b + 1], hits["he"][b:b + 1], hits["shape"][b:b + 1])
    return float(t[0])


def near_body(hits, ray, body_id, t, tol):
    """The point at t on the ray lies within tol of body `body_id` (a grazing hit the float64 test calls a miss)."""
    b = row_of(hits, body_id)
    q = hits["o"][ray] + t * hits["u"][ray] - hits["pos"][b]
    if hits["shape"][b] == SHAPE_SPHERE:
        return abs(np.linalg.norm(q) - hits["he"][b, 0]) <= tol or np.linalg.norm(q) <= hits["he"][b, 0]
    if hits["shape"][b] == SHAPE_CAPSULE:
        w = hits["R"][b][:, 1]
        return np.linalg.norm(q - np.clip(q @ w, -hits["he"][b, 1], hits["he"][b, 1]) * w) <= hits["he"][b, 0] + tol
    return bool((np.abs(hits["R"][b].T @ q) <= hits["he"][b] + tol).all())
