"""Float64 reference of the liquids (include/physics_hip.h, phys_set_liquids ...), written for the tests in numpy alone from
the header's text: submerged volume and first moment of a sphere (the cap's closed form), of a box (its six faces clipped by
the surface and closed by the cut polygon, summed as pyramids over the centre - NOT the library's six tetrahedra) and of a
capsule (the header's slab rule, with the antiderivative throughout), buoyancy and drag from them, the per-body sum in
ascending liquid order and the submersion read-out. It shares no code with the library's own statement of the arithmetic.

capsule_truth is what the slab rule approximates: a fine quadrature of true discs across the axis, each cut exactly, with
the cut disc's own centroid in the moment.

Also the committed scene of the tests: the bodies of trigger_ref.soup(seed=7, n) and liquids from a seeded generator."""
import numpy as np

NONE, SPHERE, BOX, CAPSULE = 0, 1, 2, 3
NO_LIQUID = 0xFFFFFFFF
CYL_SLABS, CAP_SLABS = 8, 4


def rot_matrix(q):
    """Rotation matrix of the quaternion [i, j, k, w] (not normalised first: the library does not either)."""
    i, j, k, w = (float(x) for x in q)
    return np.array([[w * w + i * i - j * j - k * k, 2 * (i * j - w * k), 2 * (w * j + i * k)],
                     [2 * (w * k + i * j), w * w - i * i + j * j - k * k, 2 * (j * k - w * i)],
                     [2 * (i * k - w * j), 2 * (w * i + j * k), w * w - i * i - j * j + k * k]])


def shape_volume(shape, he):
    he = np.asarray(he, np.float64)
    if shape == SPHERE:
        return 4.0 / 3.0 * np.pi * he[0] ** 3
    if shape == BOX:
        return 8.0 * he[0] * he[1] * he[2]
    if shape == CAPSULE:
        return np.pi * he[0] ** 2 * (2.0 * he[1] + 4.0 / 3.0 * he[0])
    return 0.0


def shape_bound(shape, he):
    he = np.asarray(he, np.float64)
    return {SPHERE: he[0], BOX: float(np.linalg.norm(he)), CAPSULE: 1.125 * he[0] + he[1]}.get(shape, 0.0)


def shape_reach(shape, R, he, n):
    """How far the shape extends along +-n from its centre."""
    he = np.asarray(he, np.float64)
    if shape == SPHERE:
        return he[0]
    if shape == BOX:
        return float(np.abs(R.T @ n) @ he)
    # the capsule rule's slabs, not the true capsule: a cap slab's rim lies a little outside the cap
    cu = abs(float(n @ R[:, 1]))
    st = np.sqrt(max(1.0 - cu * cu, 0.0))
    return max(cu * max(abs(t0), abs(t1)) + np.sqrt(rho2) * st for rho2, t0, t1 in capsule_slabs(he[0], he[1]))


# ---- submerged volume V and first moment M about the centre; s: the centre's height above the surface, n: its unit normal ----
def wet_sphere(r, s, n):
    hc = min(max(r - s, 0.0), 2.0 * r)
    V = np.pi * hc * hc * (3.0 * r - hc) / 3.0
    if V == 0.0:
        return 0.0, np.zeros(3)
    below = 3.0 * (2.0 * r - hc) ** 2 / (4.0 * (3.0 * r - hc))  # the cap's centroid, below the centre
    return V, -n * V * below


def _clip_polygon(poly, n, s):
    """The part of the convex polygon (k, 3) with height s + n.p <= 0, and the points where its outline crosses 0."""
    out, cuts = [], []
    d = s + poly @ n
    for a in range(len(poly)):
        b = (a + 1) % len(poly)
        if d[a] <= 0.0:
            out.append(poly[a])
        if (d[a] <= 0.0) != (d[b] <= 0.0):
            p = poly[a] + (poly[b] - poly[a]) * (d[a] / (d[a] - d[b]))
            out.append(p)
            cuts.append(p)
    return np.array(out).reshape(-1, 3), cuts


def _pyramids(poly, outward):
    """Volume and first moment about the origin of the pyramid from the origin over the planar polygon, signed by which side
    of the polygon's plane (outward normal `outward`) the origin lies on."""
    V, M = 0.0, np.zeros(3)
    for k in range(1, len(poly) - 1):
        a, b, c = poly[0], poly[k], poly[k + 1]
        v = float(outward @ a) * float(np.linalg.norm(np.cross(b - a, c - a))) / 6.0
        V += v
        M += v * (a + b + c) / 4.0
    return V, M


def wet_box(R, he, s, n):
    """By clipping the box's faces (world axes through the centre): the wet part is bounded by the clipped faces and by the cut
    polygon in the surface; each bounding polygon spans a pyramid with the centre."""
    he = np.asarray(he, np.float64)
    V, M, cuts = 0.0, np.zeros(3), []
    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            corners = []
            for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis], p[a1], p[a2] = sign * he[axis], s1 * he[a1], s2 * he[a2]
                corners.append(R @ p)
            poly, c = _clip_polygon(np.array(corners), n, s)
            cuts += c
            if len(poly) >= 3:
                v, m = _pyramids(poly, sign * R[:, axis])
                V += v
                M += m
    if len(cuts) >= 3:  # the lid: the cut points in order around their mean, in the surface
        pts = np.array(cuts)
        mid = pts.mean(0)
        e1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(n, e1)
        order = np.argsort(np.arctan2((pts - mid) @ e2, (pts - mid) @ e1))
        v, m = _pyramids(pts[order], n)
        V += v
        M += m
    return V, M


def _acos(x):
    return np.arccos(np.clip(x, -1.0, 1.0))


def _H(s, a):
    """An antiderivative in s of the wet fraction of a disc whose centre is at height s and whose lowest point is a below it."""
    if s <= -a:
        return s
    if s >= a:
        return 0.0
    x = s / a
    c2 = max(1.0 - x * x, 0.0)
    return a * (x * _acos(x) - np.sqrt(c2) + c2 ** 1.5 / 3.0) / np.pi


def _slab(rho2, st, cu, s0, t0, t1):
    a = np.sqrt(rho2) * st
    # (the antiderivative throughout; where the axis is parallel to the surface to 1e-5 of the slab its difference is 0 / 0 and
    # the limit is taken: float64 leaves both forms good to 1e-11 there)
    if abs(cu) * (t1 - t0) < 1e-5 * a:
        x = np.clip((s0 + 0.5 * (t0 + t1) * cu) / a, -1.0, 1.0)
        return np.pi * rho2 * (_acos(x) - x * np.sqrt(1.0 - x * x)) / np.pi * (t1 - t0)
    if t1 == t0:
        return 0.0
    return np.pi * rho2 * (_H(s0 + t1 * cu, a) - _H(s0 + t0 * cu, a)) / cu


def capsule_slabs(r, L):
    """(rho^2, t0, t1) of the header's slabs: 8 equal ones of the cylinder, 4 per end cap whose radius preserves their volume."""
    out = []
    for j in range(CAP_SLABS):
        z0, z1 = r * j / CAP_SLABS, r * (j + 1) / CAP_SLABS
        rho2 = r * r - (z1 * z1 + z1 * z0 + z0 * z0) / 3.0
        out += [(rho2, L + z0, L + z1), (rho2, -L - z1, -L - z0)]
    for j in range(CYL_SLABS):
        out.append((r * r, -L + 2.0 * L * j / CYL_SLABS, -L + 2.0 * L * (j + 1) / CYL_SLABS))
    return out


def wet_capsule(R, r, L, s, n):
    u = R[:, 1]
    cu = float(n @ u)
    st = np.sqrt(max(1.0 - cu * cu, 0.0))
    V, mt = 0.0, 0.0
    for rho2, t0, t1 in capsule_slabs(r, L):
        v = _slab(rho2, st, cu, s, t0, t1)
        V += v
        mt += v * 0.5 * (t0 + t1)  # at the slab's axial midpoint, on the axis
    return V, u * mt


def capsule_truth(R, r, L, s, n, discs=20000):
    """(V, M) of the capsule below the surface by `discs` true discs across the axis, each cut exactly, the cut disc's centroid
    included."""
    u = R[:, 1]
    cu = float(n @ u)
    st = np.sqrt(max(1.0 - cu * cu, 0.0))
    e = (n - cu * u) / st if st > 1e-12 else np.zeros(3)
    edges = np.linspace(-(L + r), L + r, discs + 1)
    t = 0.5 * (edges[1:] + edges[:-1])
    dt = edges[1] - edges[0]
    z = np.maximum(np.abs(t) - L, 0.0)
    rho = np.sqrt(np.maximum(r * r - z * z, 0.0))
    h = s + t * cu  # the disc centre's height
    if st > 1e-12:
        y0 = np.clip(-h / st, -rho, rho)  # wet: in-disc coordinate along e below y0
        x = -y0 / np.maximum(rho, 1e-300)
        area = rho * rho * (_acos(x) - x * np.sqrt(np.maximum(1.0 - x * x, 0.0)))
        my = -(2.0 / 3.0) * np.maximum(rho * rho - y0 * y0, 0.0) ** 1.5
    else:
        area = np.where(h < 0.0, np.pi * rho * rho, 0.0)
        my = np.zeros_like(t)
    return float(area.sum() * dt), u * float((area * t).sum() * dt) + e * float(my.sum() * dt)


def wet(shape, R, he, s, n):
    he = np.asarray(he, np.float64)
    if shape == SPHERE:
        return wet_sphere(he[0], s, n)
    if shape == BOX:
        return wet_box(R, he, s, n)
    if shape == CAPSULE:
        return wet_capsule(R, he[0], he[1], s, n)
    return 0.0, np.zeros(3)


def evaluate(liquids, bodies, category=None, force=None, torque=None):
    """The liquids on the bodies. liquids: dict of pos, rot (or None), half_extent, mask (or None), density, gravity, flow, drag.
    bodies: dict of shape, pos, rot, half_extent and optionally vel, ang. Returns a dict: F, T (n, 3) float64 from the starting
    accumulators; K (n,) liquids acting per body; frac, liquid (n,): the read-out; S (n,): the sum over the acting liquids of
    density * V_shape * |gravity|; b (n,) bounding radii; pairs, the set of acting (liquid, body); margin, the smallest
    distance of any unfiltered shaped pair to changing whether it acts: the footprint's edges, the bottom, first touching the
    surface."""
    pos = np.asarray(bodies["pos"], np.float64).reshape(-1, 3)
    n = len(pos)
    rot = np.asarray(bodies["rot"], np.float64).reshape(-1, 4)
    he = np.asarray(bodies["half_extent"], np.float64).reshape(-1, 3)
    shape = np.asarray(bodies["shape"]).reshape(-1)
    vel = np.zeros((n, 3)) if bodies.get("vel") is None else np.asarray(bodies["vel"], np.float64)
    ang = np.zeros((n, 3)) if bodies.get("ang") is None else np.asarray(bodies["ang"], np.float64)
    cat = np.full(n, 1, np.int64) if category is None else np.broadcast_to(np.asarray(category, np.int64), (n,))
    T = len(liquids["density"])
    lpos = np.asarray(liquids["pos"], np.float64).reshape(-1, 3)
    lhe = np.asarray(liquids["half_extent"], np.float64).reshape(-1, 3)
    lR = [np.eye(3) if liquids.get("rot") is None else rot_matrix(liquids["rot"][k]) for k in range(T)]
    dens = np.asarray(liquids["density"], np.float64)
    grav = np.asarray(liquids["gravity"], np.float64).reshape(-1, 3)
    flow = np.asarray(liquids["flow"], np.float64).reshape(-1, 3)
    drag = np.asarray(liquids["drag"], np.float64).reshape(-1, 2)
    F = np.zeros((n, 3)) if force is None else np.array(force, np.float64)
    Tq = np.zeros((n, 3)) if torque is None else np.array(torque, np.float64)
    S, K, b = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    frac, liquid = np.zeros(n), np.full(n, NO_LIQUID, np.uint32)
    pairs, margin = set(), np.inf
    for i in range(n):
        sh = int(shape[i])
        if sh not in (SPHERE, BOX, CAPSULE) or not (np.isfinite(pos[i]).all() and np.isfinite(rot[i]).all()):
            continue
        R = rot_matrix(rot[i])
        Vs = shape_volume(sh, he[i])
        b[i] = shape_bound(sh, he[i])
        for k in range(T):
            m = 0xFFFF if liquids.get("mask") is None else int(np.broadcast_to(liquids["mask"], (T,))[k])
            if not cat[i] & m:
                continue
            l = lR[k].T @ (pos[i] - lpos[k])
            nrm = lR[k][:, 1]
            s = l[1] - lhe[k][1]
            # the four conditions, each as a distance that is positive where it holds; a pair that acts is as far from not
            # acting as its tightest one, a pair that does not is as far from acting as its most violated one
            cond = np.array([lhe[k][0] - abs(l[0]), lhe[k][2] - abs(l[2]), l[1] + lhe[k][1], shape_reach(sh, R, he[i], nrm) - s])
            margin = min(margin, float(cond.min() if (cond >= 0.0).all() else -cond.min()))
            if (cond[:3] < 0.0).any():
                continue
            V, M = wet(sh, R, he[i], s, nrm)
            if not V > 0.0:
                continue
            f = min(V / Vs, 1.0)
            F[i] += -dens[k] * V * grav[k] - drag[k][0] * f * (vel[i] - flow[k])
            Tq[i] += -dens[k] * np.cross(M, grav[k]) - drag[k][1] * f * ang[i]
            S[i] += dens[k] * Vs * np.linalg.norm(grav[k])
            K[i] += 1
            pairs.add((k, i))
            if liquid[i] == NO_LIQUID:
                frac[i], liquid[i] = f, k
    return dict(F=F, T=Tq, K=K, S=S, b=b, frac=frac, liquid=liquid, pairs=pairs, margin=margin)


def scene_liquids(n_liquids, seed=233):
    """n_liquids pools from np.random.default_rng(seed): centres in +-6, half extents 1.5 to 5, tilted up to about 30 degrees
    from the y axis, densities 400 to 1600, gravities near (0, -9.81, 0) and not along the normals, flows and drags."""
    rng = np.random.default_rng(seed)
    T = n_liquids
    pos = rng.uniform(-6.0, 6.0, (T, 3)).astype(np.float32)
    axis = rng.normal(size=(T, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.0, 0.55, T)
    rot = np.concatenate([axis * np.sin(half)[:, None], np.cos(half)[:, None]], axis=1).astype(np.float32)
    he = rng.uniform(1.5, 5.0, (T, 3)).astype(np.float32)
    density = rng.uniform(400.0, 1600.0, T).astype(np.float32)
    gravity = (np.array([0.0, -9.81, 0.0]) + rng.normal(size=(T, 3)) * 0.8).astype(np.float32)
    flow = rng.uniform(-2.0, 2.0, (T, 3)).astype(np.float32)
    drag = rng.uniform(0.0, 4.0, (T, 2)).astype(np.float32)
    return dict(pos=pos, rot=rot, half_extent=he, mask=None, density=density, gravity=gravity, flow=flow, drag=drag)


def scene(n_bodies, n_liquids):
    """The committed scene: (bodies, liquids). Bodies: trigger_ref.soup(seed=7, n_bodies) with spins added."""
    import trigger_ref
    sc = trigger_ref.soup(seed=7, n=n_bodies)
    rng = np.random.default_rng(7029)
    bodies = dict(pos=sc["pos"], rot=sc["rot"], vel=sc["vel"], ang=rng.normal(size=(n_bodies, 3)).astype(np.float32),
                  shape=sc["shape"], half_extent=sc["half_extent"])
    return bodies, scene_liquids(n_liquids)
