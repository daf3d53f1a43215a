"""float64 reference of capsule geometry (numpy only): contacts of a capsule with the ground, a sphere, a capsule and a
box, and ray-capsule hits. An independent restatement of the rules of include/spec/collide.h section "capsules" (and of
the ray test of raycast.hip), for comparison within a tolerance: same rules, other arithmetic."""
import numpy as np

SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 1, 2, 3


def rot(q):
    """rotation matrix of a quaternion [i, j, k, w] (not renormalised, as the spec)"""
    i, j, k, w = (float(x) for x in q)
    return np.array([[w * w + i * i - j * j - k * k, 2 * (i * j - w * k), 2 * (w * j + i * k)],
                     [2 * (w * k + i * j), w * w - i * i + j * j - k * k, 2 * (j * k - w * i)],
                     [2 * (i * k - w * j), 2 * (w * i + j * k), w * w - i * i - j * j + k * k]])


def segment(c, q, he):
    """(centre, axis, half-length, radius) of a capsule"""
    return np.asarray(c, np.float64), rot(q)[:, 1], float(he[1]), float(he[0])


def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def closest_param(c, u, hl, p):
    uu = u @ u
    return _clamp((p - c) @ u / uu if uu > 1e-12 else 0.0, -hl, hl)


def segments_closest(ca, ua, ha, cb, ub, hb):
    """exact closest parameters of two segments (brute force refinement of the clamped solution is not needed: the
    problem is convex and the clamped two-step rule is exact for non-parallel segments)"""
    r = ca - cb
    a, e, b, c, f = ua @ ua, ub @ ub, ua @ ub, ua @ r, ub @ r
    den = a * e - b * b
    s = _clamp((b * f - c * e) / den, -ha, ha) if den > 1e-4 * a * e else 0.0
    t = (b * s + f) / e
    if t < -hb or t > hb:
        t = _clamp(t, -hb, hb)
        s = _clamp((b * t - c) / a, -ha, ha)
    return s, t


def _balls(pa, ra, pb, rb, margin):
    d = pb - pa
    dist = np.linalg.norm(d)
    if dist > ra + rb + margin:
        return None
    n = d / dist if dist > 1e-12 else np.array([0.0, 1.0, 0.0])
    depth = ra + rb - dist
    return n, [(pa + n * (ra - 0.5 * depth), depth)]


def ground(c, q, he, ground_y, margin):
    """list of (point, depth) of a capsule on the plane y = ground_y (normal of the manifold (0, -1, 0))"""
    c, u, hl, r = segment(c, q, he)
    ends = [c - hl * u, c + hl * u] if hl > 0 else [c]
    out = []
    for p in ends:
        depth = ground_y - (p[1] - r)
        if depth >= -margin:
            out.append((np.array([p[0], p[1] - r + 0.5 * depth, p[2]]), depth))
    return out


def capsule_sphere(cap, sph, margin):
    c, u, hl, r = segment(*cap)
    cs, rs = np.asarray(sph[0], np.float64), float(sph[2][0])
    p = c + closest_param(c, u, hl, cs) * u
    return _balls(p, r, cs, rs, margin)


def capsule_capsule(A, B, margin):
    ca, ua, ha, ra = segment(*A)
    cb, ub, hb, rb = segment(*B)
    a, e, b = ua @ ua, ub @ ub, ua @ ub
    if a * e - b * b <= 1e-4 * a * e:
        d = cb - ca
        sb = d @ ua / a
        pb = hb * abs(b) / a
        lo, hi = max(-ha, sb - pb), min(ha, sb + pb)
        if lo < hi:
            perp = d - ua * sb
            dist = np.linalg.norm(perp)
            n = perp / dist if dist > 1e-12 else np.array([0.0, 1.0, 0.0])
            pts = []
            for s in (lo, hi):
                pa = ca + s * ua
                qb = cb + closest_param(cb, ub, hb, pa) * ub
                depth = ra + rb - (qb - pa) @ n
                if depth >= -margin:
                    pts.append((pa + n * (ra - 0.5 * depth), depth))
            return (n, pts) if pts else None
    s, t = segments_closest(ca, ua, ha, cb, ub, hb)
    return _balls(ca + s * ua, ra, cb + t * ub, rb, margin)


def capsule_box(cap, box, margin):
    """the deepest point of the capsule against the box: the exact distance of the segment to the box (a convex
    minimisation by golden section over the segment parameter). Returns (normal capsule -> box, depth), or None
    beyond the margin. Only for pairs whose closest point is outside the box (dist > 0)."""
    c, u, hl, r = segment(*cap)
    cb, R, e = np.asarray(box[0], np.float64), rot(box[1]), np.asarray(box[2], np.float64)

    def dist(s):
        pl = R.T @ (c + s * u - cb)
        q = np.clip(pl, -e, e)
        return np.linalg.norm(pl - q), pl, q

    lo, hi = -hl, hl
    g = (np.sqrt(5.0) - 1.0) / 2.0
    for _ in range(200):
        m1, m2 = hi - g * (hi - lo), lo + g * (hi - lo)
        if dist(m1)[0] <= dist(m2)[0]:
            hi = m2
        else:
            lo = m1
    d, pl, q = dist(0.5 * (lo + hi))
    if d - r > margin or d <= 1e-9:
        return None
    return -(R @ ((pl - q) / d)), r - d


def ray_capsule(o, d, cap):
    """first hit (t, normal) of the ray o + t d (d unit) on a capsule, or None; t = 0 and -d from inside"""
    c, u, hl, r = segment(*cap)
    p = o - c
    s = closest_param(np.zeros(3), u, hl, p)
    if np.linalg.norm(p - s * u) <= r:
        return 0.0, -d
    best = np.inf
    pd, ud = p @ u, d @ u
    a_, b_ = d - ud * u, p - pd * u
    A, B, C = a_ @ a_, a_ @ b_, b_ @ b_ - r * r
    if A > 1e-12:
        disc = B * B - A * C
        if disc >= 0:
            t = (-B - np.sqrt(disc)) / A
            if t >= 0 and abs(pd + t * ud) <= hl:
                best = t
    for end in (-hl, hl):
        pe = p - end * u
        bb, cc = pe @ d, pe @ pe - r * r
        disc = bb * bb - cc
        if disc >= 0:
            t = -bb - np.sqrt(disc)
            if t >= 0:
                best = min(best, t)
    if not np.isfinite(best):
        return None
    h = p + best * d
    sh = closest_param(np.zeros(3), u, hl, h)
    n = h - sh * u
    return best, n / np.linalg.norm(n)


def raycast(origins, dirs, caps, ids):
    """brute force over capsules: (id, t, normal, gap to the second-best t) per ray; id None on a miss"""
    out = []
    for o, d in zip(np.asarray(origins, np.float64), np.asarray(dirs, np.float64)):
        d = d / np.linalg.norm(d)
        hits = []
        for cap, k in zip(caps, ids):
            h = ray_capsule(o, d, cap)
            if h is not None:
                hits.append((h[0], k, h[1]))
        hits.sort(key=lambda x: (x[0], x[1]))
        if not hits:
            out.append((None, np.inf, None, np.inf))
        else:
            gap = hits[1][0] - hits[0][0] if len(hits) > 1 else np.inf
            out.append((hits[0][1], hits[0][0], hits[0][2], gap))
    return out
