"""Float64 reference of the force fields (include/physics_hip.h, phys_set_force_fields ...), written for the tests in numpy
alone: signed distances of a point to the three volumes, the three laws, and the per-body sum in ascending field order. It
shares no code with the library's own statement of the arithmetic.

Also the committed scene of the tests: the bodies of trigger_ref.soup(seed=7, n) and fields drawn from
np.random.default_rng(107). No (field, body) pair of it lies within 1e-3 of a volume's boundary (tests/test_field_cpu.py
asserts the figures), so float32 and float64 agree on who is inside and a comparison needs no exclusions."""
import numpy as np

SPHERE, BOX, CAPSULE = 1, 2, 3
ACCEL, DRAG, RADIAL = 0, 1, 2


def rot_matrix(q):
    """Rotation matrix of the quaternion [i, j, k, w] (not normalised first: the library does not either)."""
    i, j, k, w = (float(x) for x in q)
    return np.array([[w * w + i * i - j * j - k * k, 2 * (i * j - w * k), 2 * (w * j + i * k)],
                     [2 * (w * k + i * j), w * w - i * i + j * j - k * k, 2 * (j * k - w * i)],
                     [2 * (i * k - w * j), 2 * (w * i + j * k), w * w - i * i - j * j + k * k]])


def signed_distance(shape, centre, rot, he, x):
    """Distance of point x to the volume's surface, negative inside. rot None: identity."""
    d = np.asarray(x, np.float64) - np.asarray(centre, np.float64)
    he = np.asarray(he, np.float64)
    R = np.eye(3) if rot is None else rot_matrix(rot)
    if shape == SPHERE:
        return float(np.linalg.norm(d) - he[0])
    if shape == BOX:
        q = np.abs(R.T @ d) - he
        return float(np.linalg.norm(np.maximum(q, 0.0)) + min(q.max(), 0.0))
    if shape == CAPSULE:
        u = R[:, 1]
        t = min(max(float(d @ u), -he[1]), he[1])
        return float(np.linalg.norm(d - t * u) - he[0])
    raise ValueError(shape)


def law(kind, vec, coef, exponent, centre, x, v, w, mass):
    """(F, T) of one field on one body inside it, or None (RADIAL at r == 0)."""
    vec = np.asarray(vec, np.float64)
    c0, c1 = float(coef[0]), float(coef[1])
    if kind == ACCEL:
        return float(mass) * vec, np.zeros(3)
    if kind == DRAG:
        return -c0 * (np.asarray(v, np.float64) - vec), -c1 * np.asarray(w, np.float64)
    if kind == RADIAL:
        d = np.asarray(x, np.float64) - np.asarray(centre, np.float64)
        r = float(np.linalg.norm(d))
        if r == 0.0:
            return None
        return c0 * (c1 / max(r, c1)) ** int(exponent) * d / r, np.zeros(3)
    raise ValueError(kind)


def evaluate(fields, pos, vel=None, ang=None, mass=None, category=None, force=None, torque=None):
    """The fields on the bodies. fields: dict of kind, shape, pos, rot (or None), half_extent, mask (or None), vec, coef,
    exponent (or None). Returns a dict: F, T (n, 3) float64 from the starting accumulators force / torque (None: zeros);
    K (n,) fields acting per body; S (n,) the sum of the magnitudes of the contributions (force and torque) and of the starting
    accumulators; pairs, the set of acting (field, body); margin, the smallest |signed distance| of any unfiltered pair."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    T = len(fields["kind"])
    vel = np.zeros((n, 3)) if vel is None else np.asarray(vel, np.float64)
    ang = np.zeros((n, 3)) if ang is None else np.asarray(ang, np.float64)
    mass = np.ones(n) if mass is None else np.asarray(mass, np.float64)
    cat = np.full(n, 1, np.int64) if category is None else np.broadcast_to(np.asarray(category, np.int64), (n,))
    F = np.zeros((n, 3)) if force is None else np.array(force, np.float64)
    Tq = np.zeros((n, 3)) if torque is None else np.array(torque, np.float64)
    S = np.linalg.norm(F, axis=1) + np.linalg.norm(Tq, axis=1)
    K = np.zeros(n, np.int64)
    pairs, margin = set(), np.inf
    for i in range(n):
        if not np.isfinite(pos[i]).all():
            continue
        for k in range(T):
            m = 0xFFFF if fields.get("mask") is None else int(np.broadcast_to(fields["mask"], (T,))[k])
            if not cat[i] & m:
                continue
            rot = None if fields.get("rot") is None else fields["rot"][k]
            sd = signed_distance(int(fields["shape"][k]), fields["pos"][k], rot, fields["half_extent"][k], pos[i])
            margin = min(margin, abs(sd))
            if sd > 0.0:
                continue
            ex = 0 if fields.get("exponent") is None else int(fields["exponent"][k])
            ft = law(int(fields["kind"][k]), fields["vec"][k], fields["coef"][k], ex, fields["pos"][k], pos[i], vel[i], ang[i], mass[i])
            if ft is None:
                continue
            F[i] += ft[0]
            Tq[i] += ft[1]
            S[i] += np.linalg.norm(ft[0]) + np.linalg.norm(ft[1])
            K[i] += 1
            pairs.add((k, i))
    return dict(F=F, T=Tq, K=K, S=S, pairs=pairs, margin=margin)


def bound(res):
    """(n, 1): what float32 may differ by, per body and component: (16 + K) * 2^-23 * S - at most 16 roundings per
    contribution and K additions, with a factor 2."""
    return ((16 + res["K"]) * 2.0 ** -23 * res["S"])[:, None]


def scene_fields(n_fields):
    """n_fields fields from np.random.default_rng(107): mixed kinds and shapes, centres in +-7, half extents 0.8 to 3.5,
    random rotations, every law's coefficients in its range."""
    rng = np.random.default_rng(107)
    T = n_fields
    shape = rng.integers(1, 4, T).astype(np.uint32)
    pos = rng.uniform(-7.0, 7.0, (T, 3)).astype(np.float32)
    q = rng.normal(size=(T, 4))
    rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    he = rng.uniform(0.8, 3.5, (T, 3)).astype(np.float32)
    kind = rng.integers(0, 3, T).astype(np.uint32)
    vec = rng.uniform(-4.0, 4.0, (T, 3)).astype(np.float32)
    coef = np.stack([rng.uniform(-6.0, 6.0, T), rng.uniform(0.3, 2.5, T)], axis=1).astype(np.float32)
    coef[kind == DRAG, 0] = np.abs(coef[kind == DRAG, 0])
    exponent = rng.integers(0, 3, T).astype(np.uint32)
    return dict(kind=kind, shape=shape, pos=pos, rot=rot, half_extent=he, mask=None, vec=vec, coef=coef, exponent=exponent)


def scene(n_bodies, n_fields):
    """The committed scene: (bodies, fields). Bodies: trigger_ref.soup(seed=7, n_bodies) with spins and unequal masses added."""
    import trigger_ref
    sc = trigger_ref.soup(seed=7, n=n_bodies)
    rng = np.random.default_rng(7007)
    bodies = dict(pos=sc["pos"], rot=sc["rot"], vel=sc["vel"], ang=rng.normal(size=(n_bodies, 3)).astype(np.float32),
                  mass=rng.uniform(0.5, 3.0, n_bodies).astype(np.float32), shape=sc["shape"], half_extent=sc["half_extent"])
    return bodies, scene_fields(n_fields)
