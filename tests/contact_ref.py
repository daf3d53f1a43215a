"""Float64 reference of the contact solver and of the manifold colouring that orders it (include/spec/contact_solve.h,
include/physics_hip.h), written for the tests from the documented definitions. numpy only: it shares no code with the
spec, the oracle or the kernels.

    ref = SolverRef(n_bodies, Params(dt, baumgarte, slop, friction, max_bias), iterations, warm=True)
    out = ref.update(manifolds, pos, lin, ang, inv_mass, inv_inertia, force)

`manifolds` is what World.get_manifolds() returns (ids, counts, normals, points), sorted by pair; pos / lin / ang are
the bodies at the START of the update. One call is one update with collisions and gravity_offset = 0:
  * pre-solve velocities: v + dt F / m (gravity is a force, quirk Q2), angular velocity unchanged;
  * persistent colouring: a pair that had a manifold in the previous call keeps its colour, the new ones go through
    Jones-Plassmann rounds on priority = splitmix64 finaliser of (a << 32 | b) against `used` masks seeded with the kept
    colours (the ground is no body, and neither is a static collider - a partner id with STATIC_ID_BIT set: its rows are
    one-sided, it has no entry in `used` or `top`, and the priority still hashes the full pair; colours capped at 63);
  * warm starting: each point takes the impulses of the first untaken remembered point within 0.05 (normal impulse if
    the normals agree to a cosine of 0.999, friction only if both tangents do too); sweep 0 applies them unclamped;
  * `iterations` Gauss-Seidel sweeps, colour by colour ascending, per point in index order: tangent 1, tangent 2,
    normal. Friction is a box clamp: each tangent to +-mu * pn of that point at that moment. Effective masses use the
    inverse inertia as given (world frame, never rotated: quirk Q5); the ground and a static collider are a static body B.
The returned dict holds lin / ang after the solve, colours, n_colors, color_rounds, n_new_manifolds, the final impulses
(m, 4, 3) in the order (t1, t2, n) and per-manifold `ambiguous` flags: a warm-start decision within 1e-5 of its
threshold, or a normal within 1e-6 of the tangent-basis switch, where float32 rounding may decide the other way."""
import numpy as np

GROUND = 0xFFFFFFFF
STATIC_ID_BIT = 0x80000000  # partner STATIC_ID_BIT | k: static collider k (the ground's id has the bit as well)
MAX_COLORS = 64
WARM_DIST2 = 0.05 ** 2
WARM_DOT = 0.999
BASIS_SWITCH = np.float32(0.57735)
WARM_BAND = 1e-5
BASIS_BAND = 1e-6


class Params:
    def __init__(self, dt, baumgarte=0.2, slop=0.01, friction=0.5, max_bias=3.0):
        self.dt, self.baumgarte, self.slop, self.friction, self.max_bias = (float(dt), float(baumgarte), float(slop),
                                                                           float(friction), float(max_bias))


def is_body(b):
    """The partner of a manifold is a body that moves: neither the ground nor a static collider."""
    return (np.asarray(b, np.int64) & STATIC_ID_BIT) == 0


# ---------------------------------------------------------------- colouring
def color_priority(a, b):
    """splitmix64's finaliser of (a << 32 | b), uint64 with wrap-around."""
    z = (np.asarray(a, np.uint64) << np.uint64(32)) | np.asarray(b, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pair_keys(a, b):
    return (np.asarray(a, np.uint64) << np.uint64(32)) | np.asarray(b, np.uint64)


def _lowest_free(mask):
    """Lowest colour whose bit is clear in mask, capped at MAX_COLORS - 1."""
    free = ~mask
    with np.errstate(over="ignore"):
        low = free & (~free + np.uint64(1))
    _, e = np.frexp(low.astype(np.float64))  # low is a power of two (exact in float64): 2^c has exponent c + 1
    return np.where(free == 0, MAX_COLORS - 1, np.minimum(e - 1, MAX_COLORS - 1)).astype(np.int64)


def color_manifolds(a, b, n_bodies, prev_keys=None, prev_colors=None):
    """Colours of manifolds (a[m], b[m]). prev_keys (sorted) / prev_colors: the previous update's pairs and colours
    (persistent mode), or None. Returns (colors, n_colors, color_rounds, n_new)."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    M = len(a)
    dyn = is_body(b)
    bb = np.where(dyn, b, 0)
    prio = color_priority(a, b)
    color = np.full(M, -1, np.int64)
    used = np.zeros(n_bodies, np.uint64)
    if prev_keys is not None and len(prev_keys) and M:
        keys = pair_keys(a, b)
        at = np.minimum(np.searchsorted(prev_keys, keys), len(prev_keys) - 1)
        kept = prev_keys[at] == keys
        color[kept] = prev_colors[at[kept]]
        bits = np.uint64(1) << color[kept].astype(np.uint64)
        np.bitwise_or.at(used, a[kept], bits)
        np.bitwise_or.at(used, bb[kept & dyn], bits[dyn[kept]])
    n_new = int((color < 0).sum())
    rounds = 0
    while (color < 0).any():
        unc = np.flatnonzero(color < 0)
        top = np.zeros(n_bodies, np.uint64)
        np.maximum.at(top, a[unc], prio[unc])
        ud = unc[dyn[unc]]
        np.maximum.at(top, bb[ud], prio[ud])
        win = unc[(prio[unc] == top[a[unc]]) & (~dyn[unc] | (prio[unc] == top[bb[unc]]))]
        # a winner is the top manifold at each of its bodies, so no two winners of a round share a body
        mask = used[a[win]] | np.where(dyn[win], used[bb[win]], np.uint64(0))
        c = _lowest_free(mask)
        color[win] = c
        bits = np.uint64(1) << c.astype(np.uint64)
        np.bitwise_or.at(used, a[win], bits)
        np.bitwise_or.at(used, bb[win][dyn[win]], bits[dyn[win]])
        rounds += 1
    n_colors = int(color.max()) + 1 if M else 0
    return color, n_colors, rounds, n_new


# ---------------------------------------------------------------- rows
def tangent_basis(normal32):
    """(t1, t2, ambiguous) of float32 unit normals (m, 3): |n.x| >= 0.57735f -> t1 ~ (n.y, -n.x, 0), otherwise
    t1 ~ (0, n.z, -n.y); t2 = n x t1. The branch is decided on the float32 value, as the device does."""
    n32 = np.asarray(normal32, np.float32).reshape(-1, 3)
    n = n32.astype(np.float64)
    ax = np.abs(n32[:, 0])
    first = ax >= BASIS_SWITCH
    t = np.where(first[:, None], np.stack([n[:, 1], -n[:, 0], np.zeros(len(n))], 1),
                 np.stack([np.zeros(len(n)), n[:, 2], -n[:, 1]], 1))
    t1 = t / np.linalg.norm(t, axis=1, keepdims=True)
    t2 = np.cross(n, t1)
    ambiguous = np.abs(ax.astype(np.float64) - float(BASIS_SWITCH)) < BASIS_BAND
    return t1, t2, ambiguous


def contact_bias(depth, p):
    depth = np.asarray(depth, np.float64)
    push = np.minimum(p.baumgarte / p.dt * (depth - p.slop), p.max_bias)
    return np.where(depth > p.slop, push, np.where(depth < 0.0, depth / p.dt, 0.0))


def warm_match(cur, prev):
    """Starting impulses (m, 4, 3) of the manifolds `cur` from the remembered `prev` (dicts of keys (sorted), normal32,
    count, pts, imp), and per-manifold ambiguity flags."""
    M = len(cur["keys"])
    P0 = np.zeros((M, 4, 3))
    amb = np.zeros(M, bool)
    if prev is None or not len(prev["keys"]) or not M:
        return P0, amb
    at = np.minimum(np.searchsorted(prev["keys"], cur["keys"]), len(prev["keys"]) - 1)
    has = (prev["keys"][at] == cur["keys"]) & (prev["count"][at] > 0)
    pn32 = prev["normal32"][at]
    dot = (cur["normal32"].astype(np.float64) * pn32.astype(np.float64)).sum(1)
    ok = has & (dot >= WARM_DOT)
    amb |= has & (np.abs(dot - WARM_DOT) < WARM_BAND)
    a1, a2, amb_a = tangent_basis(cur["normal32"])
    b1, b2, amb_b = tangent_basis(pn32)
    d1, d2 = (a1 * b1).sum(1), (a2 * b2).sum(1)
    same = (d1 >= WARM_DOT) & (d2 >= WARM_DOT)
    amb |= ok & ((np.abs(d1 - WARM_DOT) < WARM_BAND) | (np.abs(d2 - WARM_DOT) < WARM_BAND) | amb_a | amb_b)
    wpts = prev["pts"][at]
    wimp = prev["imp"][at]
    wcount = prev["count"][at]
    taken = np.zeros((M, 4), bool)
    for k in range(4):
        found = np.zeros(M, bool)
        for j in range(4):
            cand = ok & (k < cur["count"]) & (j < wcount) & ~taken[:, j] & ~found
            d = cur["pts"][:, k] - wpts[:, j]
            d2 = (d * d).sum(1)
            hit = cand & (d2 <= WARM_DIST2)
            amb |= cand & (np.abs(d2 - WARM_DIST2) < WARM_BAND)
            taken[hit, j] = True
            found |= hit
            P0[hit, k, 2] = wimp[hit, j, 2]
            hs = hit & same
            P0[hs, k, :2] = wimp[hs, j, :2]
    return P0, amb


def build_rows(a, b, count, normal32, pts, depth, x, inv_mass, inv_inertia, p):
    """Velocity-independent part of every row: directions D (m, 3 [t1, t2, n], 3), angular Jacobians aA / aB and their
    images under the inverse inertia mA / mB (m, 4, 3, 3), inverse masses, row masses (m, 4, 3), bias (m, 4)."""
    M = len(a)
    dyn = is_body(b)
    bb = np.where(dyn, b, 0)
    t1, t2, amb = tangent_basis(normal32)
    n = normal32.astype(np.float64)
    D = np.stack([t1, t2, n], 1)
    active = np.arange(4)[None, :] < count[:, None]
    rA = np.where(active[:, :, None], pts - x[a][:, None, :], 0.0)
    rB = np.where((active & dyn[:, None])[:, :, None], pts - x[bb][:, None, :], 0.0)
    aA = np.cross(rA[:, :, None, :], D[:, None, :, :])
    aB = np.cross(rB[:, :, None, :], D[:, None, :, :])
    mA = np.einsum("mij,mkdj->mkdi", inv_inertia[a], aA)
    mB = np.einsum("mij,mkdj->mkdi", inv_inertia[bb], aB) * dyn[:, None, None, None]
    imA = inv_mass[a]
    imB = np.where(dyn, inv_mass[bb], 0.0)
    k = imA[:, None, None] + (mA * aA).sum(-1) + (imB[:, None, None] + (mB * aB).sum(-1)) * dyn[:, None, None]
    with np.errstate(divide="ignore"):
        mass = np.where(active[:, :, None] & (k > 0), 1.0 / np.where(k > 0, k, 1.0), 0.0)
    bias = np.where(active, contact_bias(depth, p), 0.0)
    return dict(D=D, aA=aA, aB=aB, mA=mA, mB=mB, imA=imA, imB=imB, mass=mass, bias=bias, active=active, basis_amb=amb)


def solve(a, b, count, colors, n_colors, rows, lin, ang, friction, iterations, P0=None):
    """Gauss-Seidel in colour order. lin / ang (n, 3) are the pre-solve velocities (modified copies are returned).
    With P0 (warm start) sweep 0 applies those impulses unclamped before the `iterations` relaxation sweeps."""
    v = np.array(lin, np.float64)
    w = np.array(ang, np.float64)
    M = len(a)
    P = np.zeros((M, 4, 3)) if P0 is None else np.array(P0, np.float64)
    dyn = is_body(b)
    bb = np.where(dyn, b, 0)
    groups = []
    for c in range(n_colors):
        idx = np.flatnonzero(colors == c)
        if not len(idx):
            continue
        g = {key: rows[key][idx] for key in ("D", "aA", "aB", "mA", "mB", "imA", "imB", "mass", "bias", "active")}
        g.update(idx=idx, A=a[idx], B=bb[idx], dyn=dyn[idx])
        groups.append(g)
    for sweep in range(0 if P0 is not None else 1, iterations + 1):
        for g in groups:
            # the manifolds of one colour share no dynamic body: one vector operation per row, bodies gathered once
            idx, A, B, hb = g["idx"], g["A"], g["B"], g["dyn"][:, None]
            vA, wA = v[A], w[A]
            vB, wB = v[B] * hb, w[B] * hb
            Pc = P[idx]
            for k in range(4):
                act = g["active"][:, k]
                if not act.any():
                    continue
                for d in range(3):
                    dirv = g["D"][:, d]
                    aA, aB, mA, mB = g["aA"][:, k, d], g["aB"][:, k, d], g["mA"][:, k, d], g["mB"][:, k, d]
                    if sweep == 0:
                        lam = np.where(act, Pc[:, k, d], 0.0)
                    else:
                        vrel = ((dirv * vB).sum(1) + (aB * wB).sum(1)) - ((dirv * vA).sum(1) + (aA * wA).sum(1))
                        old = Pc[:, k, d]
                        if d < 2:
                            lim = friction * Pc[:, k, 2]
                            new = np.maximum(-lim, np.minimum(old - g["mass"][:, k, d] * vrel, lim))
                        else:
                            new = np.maximum(old + g["mass"][:, k, d] * (g["bias"][:, k] - vrel), 0.0)
                        new = np.where(act, new, 0.0)
                        lam = new - old
                        Pc[:, k, d] = new
                    vA = vA - dirv * (g["imA"] * lam)[:, None]
                    wA = wA - mA * lam[:, None]
                    vB = vB + dirv * (g["imB"] * lam)[:, None]
                    wB = wB + mB * lam[:, None]
            P[idx] = Pc
            v[A], w[A] = vA, wA
            h = g["dyn"]
            v[B[h]], w[B[h]] = vB[h], wB[h]
    return v, w, P


def unpack_manifolds(manifolds):
    ids, counts, normals, points = manifolds
    ids = np.asarray(ids).reshape(-1, 2)
    a = ids[:, 0].astype(np.int64)
    b = ids[:, 1].astype(np.int64)
    pts = np.asarray(points, np.float32).reshape(-1, 4, 4)
    return dict(a=a, b=b, keys=pair_keys(a, b), count=np.asarray(counts, np.int64),
                normal32=np.asarray(normals, np.float32).reshape(-1, 3),
                pts=pts[:, :, :3].astype(np.float64), depth=pts[:, :, 3].astype(np.float64))


class SolverRef:
    """The state one world carries between updates: the previous update's colours and the impulses its solve ended
    with (this reference's own float64 values). warm=False: no sweep 0, nothing carried (PHYS_FLAG_NO_WARM_START)."""

    def __init__(self, n_bodies, params, iterations, warm=True):
        self.n = int(n_bodies)
        self.p = params
        self.iterations = int(iterations)
        self.warm = warm
        self.prev = None

    def update(self, manifolds, pos, lin, ang, inv_mass, inv_inertia, force=None):
        m = unpack_manifolds(manifolds)
        assert (m["keys"][1:] > m["keys"][:-1]).all(), "manifolds must be sorted by pair"
        prev = self.prev
        colors, n_colors, rounds, n_new = color_manifolds(m["a"], m["b"], self.n, None if prev is None else prev["keys"],
                                                          None if prev is None else prev["colors"])
        inv_mass = np.broadcast_to(np.asarray(inv_mass, np.float64), (self.n,))
        inv_inertia = np.broadcast_to(np.asarray(inv_inertia, np.float64), (self.n, 3, 3))
        x = np.asarray(pos, np.float64).reshape(-1, 3)
        rows = build_rows(m["a"], m["b"], m["count"], m["normal32"], m["pts"], m["depth"], x, inv_mass, inv_inertia, self.p)
        v = np.asarray(lin, np.float64).reshape(-1, 3)
        if force is not None:
            v = v + self.p.dt * np.asarray(force, np.float64) * inv_mass[:, None]
        w = np.asarray(ang, np.float64).reshape(-1, 3)
        P0, amb = warm_match(m, prev) if self.warm else (None, np.zeros(len(m["a"]), bool))
        v, w, P = solve(m["a"], m["b"], m["count"], colors, n_colors, rows, v, w, self.p.friction, self.iterations, P0)
        self.prev = dict(keys=m["keys"], colors=colors, normal32=m["normal32"], count=m["count"], pts=m["pts"], imp=P)
        return dict(lin=v, ang=w, colors=colors, n_colors=n_colors, color_rounds=rounds, n_new_manifolds=n_new, impulses=P,
                    ambiguous=amb | rows["basis_amb"], a=m["a"], b=m["b"], count=m["count"], P0=P0)


def color_counts(colors):
    return np.bincount(np.asarray(colors, np.int64), minlength=MAX_COLORS)[:MAX_COLORS]


# ---------------------------------------------------------------- scenes shared by the CPU and GPU tests
SHAPE_SPHERE, SHAPE_BOX = 1, 2


def _small_tilts(rng, n, angle):
    """Quaternions [i, j, k, w] of rotations by up to `angle` radians about random axes."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.0, angle, n)
    return np.concatenate([axis * np.sin(half)[:, None], np.cos(half)[:, None]], 1).astype(np.float32)


def _inertia(rng, n, kind):
    if kind == "identity":
        return None  # every body the same identity tensor (the solver reads one shared entry)
    if kind == "diag":
        return np.stack([np.diag(d) for d in rng.uniform(0.3, 3.0, size=(n, 3))]).reshape(n, 9).astype(np.float32)
    A = rng.normal(size=(n, 3, 3))
    return (A @ A.transpose(0, 2, 1) + 1.5 * np.eye(3)).reshape(n, 9).astype(np.float32)  # SPD, not diagonal


def friction_pairs(seed, n_groups, inertia="identity"):
    """Isolated manifolds with friction engaged: per group, a box resting on a box, a sphere resting on a box and a box
    on the ground, 12 units from every other group. Contacts start 0.09 deep to 0.015 apart (the slop, the max_bias cap
    and speculative points all occur); the upper body approaches at up to 2 units/s and slides at 0 to 6 units/s, so
    friction ends in stick for some rows and at the +-mu pn box for others. Returns the set_bodies arguments."""
    rng = np.random.default_rng(seed)
    n = 5 * n_groups
    pos = np.zeros((n, 3))
    he = rng.uniform(0.5, 1.2, size=(n, 3))
    shape = np.full(n, SHAPE_BOX, np.uint32)
    rot = _small_tilts(rng, n, 0.15)
    lin = np.zeros((n, 3))
    ang = rng.normal(scale=0.3, size=(n, 3))
    side = int(np.ceil(n_groups ** 0.5))
    for g in range(n_groups):
        base = np.array([(g % side - 0.5 * side) * 12.0, 0.0, (g // side - 0.5 * side) * 12.0])
        lo, up, s_lo, s, gb = 5 * g, 5 * g + 1, 5 * g + 2, 5 * g + 3, 5 * g + 4
        rot[[lo, s_lo]] = (0, 0, 0, 1)
        pos[lo] = base + (0, 8.0, 0)
        pos[up] = pos[lo] + (rng.uniform(-0.3, 0.3), he[lo, 1] + he[up, 1] - rng.uniform(-0.015, 0.09), rng.uniform(-0.3, 0.3))
        shape[s] = SHAPE_SPHERE
        he[s] = he[s, 0]
        pos[s_lo] = base + (5.0, 8.0, 0)
        pos[s] = pos[s_lo] + (rng.uniform(-0.3, 0.3), he[s_lo, 1] + he[s, 0] - rng.uniform(-0.015, 0.09), rng.uniform(-0.3, 0.3))
        R = quat_matrices(rot[gb:gb + 1])[0]
        pos[gb] = base + (0, float(np.abs(R[1]) @ he[gb]) - rng.uniform(-0.015, 0.09), 5.0)
        for body in (up, s, gb):
            slide = rng.normal(size=3)
            slide[1] = 0.0
            slide *= rng.uniform(0.0, 6.0) / np.linalg.norm(slide)
            lin[body] = slide + (0, -rng.uniform(0.0, 2.0), 0)
    mass = rng.uniform(0.5, 4.0, n).astype(np.float32)
    return dict(pos=pos.astype(np.float32), rot=rot, lin_vel=lin.astype(np.float32), ang_vel=ang.astype(np.float32),
                mass=mass, inertia=_inertia(rng, n, inertia), shape_type=shape, half_extent=he.astype(np.float32))


def random_heap(seed, n=512):
    """About 500 boxes and spheres of mixed sizes and orientations on a jittered lattice of spacing 1.9 on the ground:
    most touch several neighbours at once from the first update."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil((n / 4) ** 0.5))
    idx = np.arange(n)
    pos = np.stack([(idx % side) * 1.9, 1.0 + (idx // (side * side)) * 1.9, ((idx // side) % side) * 1.9], 1)
    pos = pos + rng.uniform(-0.15, 0.15, size=(n, 3))
    shape = np.where(rng.random(n) < 0.4, SHAPE_SPHERE, SHAPE_BOX).astype(np.uint32)
    he = rng.uniform(0.75, 1.05, size=(n, 3))
    he[shape == SHAPE_SPHERE] = he[shape == SHAPE_SPHERE, :1]
    lin = rng.normal(scale=0.5, size=(n, 3))
    return dict(pos=pos.astype(np.float32), rot=_small_tilts(rng, n, np.pi), lin_vel=lin.astype(np.float32),
                ang_vel=rng.normal(scale=0.5, size=(n, 3)).astype(np.float32), mass=rng.uniform(0.5, 3.0, n).astype(np.float32),
                inertia=None, shape_type=shape, half_extent=he.astype(np.float32))


def body_boxes(bodies):
    """Float64 boxes [lo, hi] (n, 6) of boxes and spheres as set_bodies takes them, without a margin."""
    R = np.abs(quat_matrices(bodies["rot"]))
    he = np.asarray(bodies["half_extent"], np.float64)
    e = np.where((np.asarray(bodies["shape_type"]) == SHAPE_SPHERE)[:, None], he[:, :1], np.einsum("nab,nb->na", R, he))
    c = np.asarray(bodies["pos"], np.float64)
    return np.concatenate([c - e, c + e], 1)


CONTAINER_GAP = 0.004  # of a wall segment to the nearest body: inside the contact margin of 0.02, and no overlap


def heap_container(bodies, pitch=1.9, top=0.0):
    """A static container for random_heap's bodies: a floor slab whose top is the plane y = `top`, and four walls of one
    box segment per lattice column (1 long, 0.5 thick, as high as the heap). Each segment's face stands CONTAINER_GAP
    outside the farthest-reaching body among those it faces, so no body starts in overlap with a wall and the nearest
    body of every segment starts with a speculative manifold against it; bodies of the lowest layer among those touch
    floor and wall. Returns (pos, shape_type, half_extent) of set_static_bodies (identity rotations); the slab is static 0."""
    box = body_boxes(bodies)
    lo, hi = box[:, :3].min(0), box[:, 3:].max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pos = [[mid[0], top - 0.5, mid[2]]]
    he = [[half[0] + 3.0, 0.5, half[2] + 3.0]]
    centres = np.asarray(bodies["pos"], np.float64)
    height = 0.5 * (hi[1] - top) + 0.5
    for axis, along in ((0, 2), (2, 0)):
        cols = np.unique(np.round(centres[:, along] / pitch).astype(np.int64))
        for c in cols * pitch:
            faces = (box[:, along] <= c + 0.5) & (box[:, 3 + along] >= c - 0.5)
            for side in (-1.0, 1.0):
                reach = box[faces, axis].min() if side < 0 else box[faces, 3 + axis].max()
                p = [0.0, top + height - 0.5, 0.0]
                p[axis], p[along] = reach + side * (CONTAINER_GAP + 0.25), c
                h = [0.0, height, 0.0]
                h[axis], h[along] = 0.25, 0.5
                pos.append(p); he.append(h)
    return dict(pos=np.asarray(pos, np.float32), shape_type=np.full(len(pos), SHAPE_BOX, np.uint32), half_extent=np.asarray(he, np.float32))


def static_boxes(seed=21, n_st=120):
    """Sliding and spinning boxes and spheres on static boxes 12 apart, ONE body on each static (a third of the boxes with
    a second box on top). Returns (set_bodies arguments, set_static_bodies arguments)."""
    rng = np.random.default_rng(seed)
    st_pos = np.column_stack([np.arange(n_st) % 12 * 12.0, np.zeros(n_st), np.arange(n_st) // 12 * 12.0])
    st_he = np.column_stack([rng.uniform(1.5, 2.5, n_st), np.full(n_st, 0.5), rng.uniform(1.5, 2.5, n_st)])
    pos, rot, shape, he = [], [], [], []
    for k in range(n_st):
        c = st_pos[k]
        sphere = k % 4 == 3
        r = rng.uniform(0.4, 0.7)
        h = np.array([r, r, r]) if sphere else rng.uniform(0.4, 0.7, 3)
        off = rng.uniform(-0.6, 0.6, 2)
        pos.append([c[0] + off[0], 0.5 + h[1] - rng.uniform(-0.015, 0.03), c[2] + off[1]])
        q = np.array([*(rng.normal(size=3) * 0.02), 1.0]) if not sphere else np.array([0, 0, 0, 1.0])
        rot.append(q / np.linalg.norm(q)); shape.append(SHAPE_SPHERE if sphere else SHAPE_BOX); he.append(h)
        if k % 3 == 0 and not sphere:  # a box on top: a body-body manifold coloured against the static one
            h2 = rng.uniform(0.3, 0.5, 3)
            pos.append([pos[-1][0] + rng.uniform(-0.2, 0.2), pos[-1][1] + h[1] + h2[1] - 0.01, pos[-1][2]])
            rot.append(np.array([0, 0, 0, 1.0])); shape.append(SHAPE_BOX); he.append(h2)
    pos, rot, he = (np.asarray(x, np.float32) for x in (pos, rot, he))
    n = len(pos)
    lin = np.column_stack([rng.uniform(-4, 4, n), np.zeros(n), rng.uniform(-4, 4, n)]).astype(np.float32)
    ang = (rng.normal(size=(n, 3)) * 0.5).astype(np.float32)
    bodies = dict(pos=pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=np.asarray(shape, np.uint32), half_extent=he)
    statics = dict(pos=st_pos.astype(np.float32), shape_type=np.full(n_st, SHAPE_BOX, np.uint32), half_extent=st_he.astype(np.float32))
    return bodies, statics


SHAPE_CAPSULE = 3
TOWER_MU = 0.5  # the default friction, which varied_tower's census of friction rows is taken with


def varied_tower(seed, inertia, dims=(16, 130, 16), p_sphere=0.25, p_capsule=0.2, p_tilt=0.3, tilt=0.02, slide=3.0, spin=0.6):
    """A tower whose bodies are all different, for the kernels that move body constants about: the 16 x 130 x 16 lattice of
    spacing 2 (x fastest, then z, then y; lowest centres at y = 1: resting contact all round), 33 280 bodies.
      masses   log-uniform in [0.25, 4], independent per body;
      inertia  "uniform": one diagonal tensor (0.6, 1.7, 2.9) for everybody; "diag": three distinct entries per body;
               "full": symmetric positive definite with off-diagonal entries (_inertia);
      shapes   boxes of half extent 1, spheres of radius 1 and capsules (radius 1, core half-length 0.05) lying along x or
               z; some boxes tilted by up to `tilt` radians: manifolds of 1, 2 and 4 points;
      motion   horizontal speeds of 0 to `slide` units/s, up to 0.3 up or down, angular velocities of scale `spin`: some
               friction rows end at the +-mu pn box, others inside it.
    Returns the set_bodies arguments. Seeds and amplitudes are pinned by tests/test_contact_ref_cpu.py's censuses."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    n = nx * ny * nz
    idx = np.arange(n)
    pos = np.stack([(idx % nx - (nx - 1) / 2.0) * 2.0, 1.0 + (idx // (nx * nz)) * 2.0, ((idx // nx) % nz - (nz - 1) / 2.0) * 2.0], 1)
    u = rng.random(n)
    shape = np.where(u < p_sphere, SHAPE_SPHERE, np.where(u < p_sphere + p_capsule, SHAPE_CAPSULE, SHAPE_BOX)).astype(np.uint32)
    he = np.ones((n, 3))
    he[shape == SHAPE_CAPSULE] = (1.0, 0.05, 0.0)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 3] = 1.0
    tilted = (shape == SHAPE_BOX) & (rng.random(n) < p_tilt)
    rot[tilted] = _small_tilts(rng, int(tilted.sum()), tilt)
    s = np.float32(np.sqrt(0.5))
    caps = np.flatnonzero(shape == SHAPE_CAPSULE)
    along_x = rng.random(len(caps)) < 0.5
    rot[caps] = (0, 0, 0, s)
    rot[caps[along_x], 2] = s   # 90 degrees about z: the core (local y) along -x
    rot[caps[~along_x], 0] = s  # 90 degrees about x: the core along +z
    heading = rng.uniform(0.0, 2.0 * np.pi, n)
    speed = rng.uniform(0.0, slide, n)
    lin = np.stack([speed * np.cos(heading), rng.uniform(-0.3, 0.3, n), speed * np.sin(heading)], 1)
    ang = rng.normal(scale=spin, size=(n, 3))
    mass = np.exp(rng.uniform(np.log(0.25), np.log(4.0), n))
    if inertia == "uniform":
        tensor = np.tile(np.diag([0.6, 1.7, 2.9]).reshape(1, 9), (n, 1)).astype(np.float32)
    else:
        tensor = _inertia(rng, n, inertia)
    return dict(pos=pos.astype(np.float32), rot=rot, lin_vel=lin.astype(np.float32), ang_vel=ang.astype(np.float32),
                mass=mass.astype(np.float32), inertia=tensor, shape_type=shape, half_extent=he.astype(np.float32))


VARIED_SEED = 11
VARIED_UPDATES = 4
# id -> (inertia, warm start, iterations): the solves the cluster kernel is held to on the varied tower (CPU: the float32
# solve of the host, tests/test_contact_ref_cpu.py; GPU: tests/test_gpu_solver_independent.py, tests/test_gpu_cluster_variants.py)
VARIED_CASES = {"diag": ("diag", True, 8), "uniform": ("uniform", True, 8), "full": ("full", True, 8),
                "diag_cold": ("diag", False, 8), "diag_cold_1": ("diag", False, 1), "diag_warm_1": ("diag", True, 1),
                "full_warm_2": ("full", True, 2), "full_cold_2": ("full", False, 2)}
# the worst float32-against-float64 velocity error of the host's float32 solve over every case above, four updates each: measured
# 3.33e-6 (diag, update 4; uniform 2.32e-6, full 3.09e-6, diag_cold 1.43e-6, diag_cold_1 7.66e-7, diag_warm_1 1.32e-6,
# full_warm_2 1.26e-6, full_cold_2 9.25e-7), rounded up to two digits. tests/test_contact_ref_cpu.py prints each
# and asserts that none exceeds this figure; the kernels get 4 x (the margin of tests/dynamics_ref.py)
MEASURED_VARIED = 3.4e-6
TOL_VARIED = 4.0 * MEASURED_VARIED


def point_count_shares(count):
    """Shares of the manifolds with 1, 2 and 4 points."""
    count = np.asarray(count)
    return tuple(float((count == k).mean()) for k in (1, 2, 4))


def quat_matrices(rot):
    """World = R @ local for quaternions [i, j, k, w]."""
    q = np.asarray(rot, np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    i, j, k, w = q.T
    return np.stack([np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - w * k), 2 * (i * k + w * j)], 1),
                     np.stack([2 * (i * j + w * k), 1 - 2 * (i * i + k * k), 2 * (j * k - w * i)], 1),
                     np.stack([2 * (i * k - w * j), 2 * (j * k + w * i), 1 - 2 * (i * i + j * j)], 1)], 1)


def body_inverses(n, mass=None, inertia=None):
    """Inverse masses (n,) and inverse inertia tensors (n, 3, 3) in float64 of set_bodies' arrays (None: 1 / identity)."""
    inv_m = np.ones(n) if mass is None else 1.0 / np.asarray(mass, np.float64).reshape(n)
    if inertia is None:
        inv_I = np.broadcast_to(np.eye(3), (n, 3, 3))
    else:
        inv_I = np.linalg.inv(np.asarray(inertia, np.float64).reshape(n, 3, 3))
    return inv_m, inv_I


def friction_row_states(out, friction, tol=1e-9):
    """(clamped, inside) counts of the friction rows of active points with pn > 0, from the reference's final impulses."""
    P = out["impulses"]
    act = (np.arange(4)[None, :] < out["count"][:, None]) & (P[:, :, 2] > 1e-6)
    lim = friction * P[:, :, 2]
    pt = np.abs(P[:, :, :2])
    clamped = act[:, :, None] & (pt >= lim[:, :, None] - tol * (1 + lim[:, :, None]))
    return int(clamped.sum()), int((act[:, :, None] & ~clamped).sum())


def velocity_error(out, lin, ang):
    """Largest |device - reference| over the velocities of every body, leaving out the bodies of ambiguous manifolds;
    and the number of those manifolds."""
    skip = np.zeros(len(lin), bool)
    amb = out["ambiguous"]
    skip[out["a"][amb]] = True
    bb = out["b"][amb]
    skip[bb[is_body(bb)]] = True
    keep = ~skip
    err = max(np.abs(np.asarray(lin, np.float64)[keep] - out["lin"][keep]).max(initial=0.0),
              np.abs(np.asarray(ang, np.float64)[keep] - out["ang"][keep]).max(initial=0.0))
    return float(err), int(amb.sum())


def spinning_pairs(seed, n_pairs, turn_deg, start_deg, dt):
    """Pairs (heavy box A, sphere B) whose contact normal turns: box A (mass and inertia x 1000, so the contacts hardly
    slow it) spins about z at turn_deg per update (with PHYS_FLAG_EXACT_ROTATION), and the sphere rests on the face whose normal starts start_deg (one
    value, or a (lo, hi) range) from +y towards -x, sliding along z so that friction carries impulses of its own."""
    rng = np.random.default_rng(seed)
    n = 2 * n_pairs
    side = int(np.ceil(n_pairs ** 0.5))
    k = np.arange(n_pairs)
    base = np.stack([(k % side) * 10.0, np.full(n_pairs, 20.0), (k // side) * 10.0], 1)
    lo, hi = (start_deg, start_deg) if np.isscalar(start_deg) else start_deg
    theta = np.radians(rng.uniform(lo, hi, n_pairs))
    normal = np.stack([-np.sin(theta), np.cos(theta), np.zeros(n_pairs)], 1)
    he = np.ones((n, 3))
    he[0::2] = rng.uniform(0.8, 1.2, size=(n_pairs, 3))
    he[1::2] = rng.uniform(0.4, 0.7, size=(n_pairs, 1))
    pos = np.zeros((n, 3))
    pos[0::2] = base
    pos[1::2] = base + normal * (he[0::2, 1] + he[1::2, 0] - rng.uniform(0.0, 0.01, n_pairs))[:, None]
    rot = np.zeros((n, 4))
    rot[:, 3] = 1.0
    rot[0::2, 2], rot[0::2, 3] = np.sin(theta / 2), np.cos(theta / 2)  # about z: the box's +y face normal becomes `normal`
    lin = np.zeros((n, 3))
    lin[1::2] = -0.5 * normal + np.stack([np.zeros(n_pairs), np.zeros(n_pairs), rng.uniform(0.5, 2.0, n_pairs)], 1)
    ang = np.zeros((n, 3))
    ang[0::2, 2] = np.radians(turn_deg) / dt
    mass = np.ones(n)
    mass[0::2] = 1000.0
    inertia = np.tile(np.eye(3).reshape(1, 9), (n, 1))
    inertia[0::2] *= 1000.0
    shape = np.where(np.arange(n) % 2 == 0, SHAPE_BOX, SHAPE_SPHERE).astype(np.uint32)
    return dict(pos=pos.astype(np.float32), rot=rot.astype(np.float32), lin_vel=lin.astype(np.float32),
                ang_vel=ang.astype(np.float32), mass=mass.astype(np.float32), inertia=inertia.astype(np.float32),
                shape_type=shape, half_extent=he.astype(np.float32))
