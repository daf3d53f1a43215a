"""The seeded inputs of the box-cast tests with their float64 answers (tests/boxcast_ref.py), computed once per process and
shared, unchanged, by tests/test_boxcast_cpu.py (which counts the reference's own near ties and holds the host probe to them)
and tests/test_gpu_boxcast.py (which holds the kernel to them). numpy and the references only.

A case: dict(label, bodies, statics, ground, centre, o, d, rot, he, max_t, ignore, tg, h)."""
import functools
import hashlib
import math
import os
import sys

import numpy as np

import boxcast_ref as ref
import capsulecast_cases as cc
import query_ref
import query_scenes as qs
from raycast_ref import rotation_matrices

SPHERE, BOX, CAPSULE = qs.SPHERE, qs.BOX, qs.CAPSULE
SOUP_SEEDS = (1, 2)
GRID_SCENES = cc.GRID_SCENES
IDENT = cc.IDENT
quats, axis_quat, outside = cc.quats, cc.axis_quat, cc.outside


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxcast")
STORED = ("body", "t", "t2", "which", "normal", "point")  # what a stored answer holds: the float64 brute force's arrays


def _digest(arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return np.frombuffer(m.digest(), np.uint8)


def golden_path(label):
    return os.path.join(GOLDEN, label.replace(" ", "_") + ".npz")


def _case(label, bodies, statics, o, d, rot, he, ground=0.0, centre=None, max_t=None, ignore=None, tg=None, recompute=False):
    """The brute force takes a minute for a soup, so the answers of the larger cases are stored under tests/golden/boxcast
    (arrays only, with a digest of the inputs they answer; `python tests/boxcast_cases.py --store` writes them). A
    stored answer is used where its digest matches; tests/test_boxcast_cpu.py recomputes stored cases and compares."""
    f = np.float32
    n = len(o)
    o, d = np.asarray(o, f).reshape(-1, 3), np.asarray(d, f).reshape(-1, 3)
    rot = None if rot is None else np.asarray(rot, f).reshape(-1, 4)
    he = np.broadcast_to(np.asarray(he, f).reshape(-1, 3), (n, 3)).copy()
    bodies = {k: np.asarray(v, np.uint32 if k == "shape" else f) for k, v in bodies.items()}
    if tg is None:
        tg = query_ref.targets(bodies, statics)
    digest = _digest([o, d, rot, he, max_t, ignore, tg["pos"], tg["rot"], tg["half_extent"], tg["shape"], tg["id"],
                      np.float64(np.nan if ground is None else ground), None if centre is None else np.asarray(centre, np.float64)])
    path = golden_path(label)
    stored = False
    h = None
    if not recompute and os.path.exists(path):
        with np.load(path) as z:
            if np.array_equal(z["digest"], digest):
                h = ref.inputs(o, d, rot, he, tg, max_t=max_t, ignore=ignore, ground=ground, centre=centre)
                h.update({k: z[k] for k in STORED})
                stored = True
    if h is None:
        h = ref.boxcast(o, d, rot, he, tg, max_t=max_t, ignore=ignore, ground=ground, centre=centre)
    return cc._frozen(dict(label=label, bodies=bodies, statics=statics, ground=ground, centre=centre, o=o, d=d, rot=rot, he=he,
                           max_t=max_t, ignore=ignore, tg=tg, h=h, stored=stored, digest=digest))


def sizes(rng, n, lo=0.1, hi=1.2):
    """half extents uniform in [lo, hi]^3, one component zeroed for a tenth (plates)"""
    he = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    flat = rng.random(n) < 0.1
    he[flat, rng.integers(0, 3, n)[flat]] = 0.0
    return he


# ---- random soups: capsulecast_cases' bodies, statics, origins and directions -------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup(seed, n_bodies=300, n_casts=300, extent=15.0):
    rng = np.random.default_rng(100 + seed)
    bodies = cc.soup_bodies(rng, n_bodies, extent)
    statics = cc.soup_statics(rng)
    o, d, rot, _, _ = cc.soup_casts(rng, n_casts, extent)  # starts >= 3 outside the scene: a box of reach <= 2.08 touches nothing
    return _case(f"soup seed {seed}", bodies, statics, o, d, rot, sizes(rng, n_casts))


# ---- degenerate sets: one call each -----------------------------------------------------------------------------------------
DEGENERATE = ("box_parallel", "box_near_parallel", "box_shared_axis", "plate", "rod", "point", "capsule_axis", "capsule_perpendicular",
              "zero_radius_targets", "long_thin", "wide_cube", "corner_reach")


def _turn(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return list(np.append(math.sin(0.5 * angle) * a, math.cos(0.5 * angle)))


def _qmul(a, b):
    ai, aj, ak, aw = a
    bi, bj, bk, bw = b
    return [aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi, aw * bk + ai * bj - aj * bi + ak * bw,
            aw * bw - ai * bi - aj * bj - ak * bk]


@functools.lru_cache(maxsize=None)
def degenerate(name, n=60):
    rng = np.random.default_rng(600 + DEGENERATE.index(name))
    c = np.array([0.0, 6.0, 0.0])
    tilt = axis_quat([0.3, 1.0, -0.2])  # the targets' own turn
    Rt = rotation_matrices(np.array([tilt]))[0]
    box = dict(pos=[c], rot=[tilt], shape=[BOX], half_extent=[[1.0, 0.6, 0.8]])
    cap = dict(pos=[c], rot=[tilt], shape=[CAPSULE], half_extent=[[0.4, 1.1, 0.0]])
    three = dict(pos=[c, c + [4.0, 0, 0], c - [4.0, 0, 0]], rot=[tilt, tilt, IDENT], shape=[BOX, CAPSULE, SPHERE],
                 half_extent=[[1.0, 0.6, 0.8], [0.4, 1.1, 0.0], [0.9, 0.0, 0.0]])
    o, d = cc._fan(rng, n, c, 7.0)
    he = rng.uniform(0.2, 1.0, (n, 3))
    if name == "box_parallel":  # the cast box's axes exactly the target's (some with the axes permuted): all nine cross axes vanish
        perm = [tilt, _qmul(tilt, _turn([0, 0, 1], math.pi / 2)), _qmul(tilt, _turn([1, 0, 0], math.pi / 2))]
        return _case(name, box, None, o, d, [perm[0]] * (n // 2) + [perm[k % 3] for k in range(n - n // 2)], he, ground=None)
    if name == "box_near_parallel":  # 1e-3 rad from parallel, about a random axis
        rot = [_qmul(tilt, _turn(rng.normal(size=3), 1e-3)) for _ in range(n)]
        return _case(name, box, None, o, d, rot, he, ground=None)
    if name == "box_shared_axis":  # one axis shared (the target's x, y or z), turned about it
        rot = [_qmul(tilt, _turn([[1, 0, 0], [0, 1, 0], [0, 0, 1]][k % 3], rng.uniform(0.2, 1.3))) for k in range(n)]
        return _case(name, box, None, o, d, rot, he, ground=None)
    if name in ("plate", "rod", "point"):
        o, d = cc._fan(rng, n, c, 9.0)
        d = (np.asarray(three["pos"], np.float64)[np.arange(n) % 3] + rng.uniform(-0.8, 0.8, (n, 3)) - o).astype(np.float32)
        zero = {"plate": 1, "rod": 2, "point": 3}[name]
        for k in range(n):
            he[k, rng.permutation(3)[:zero]] = 0.0
        return _case(name, three, None, o, d, quats(rng, n), he, ground=None)
    if name in ("capsule_axis", "capsule_perpendicular"):
        w = Rt[:, 1]
        if name == "capsule_axis":  # a box axis (x, y, z in turn) along the capsule's axis
            base = [_qmul(tilt, q) for q in (_turn([0, 0, 1], -math.pi / 2), IDENT, _turn([1, 0, 0], math.pi / 2))]
            rot = [_qmul(base[k % 3], _turn([[1, 0, 0], [0, 1, 0], [0, 0, 1]][k % 3], rng.uniform(0, 3))) for k in range(n)]
        else:  # the box's y axis in the plane perpendicular to the capsule's axis
            p = np.cross(w, [1.0, 0.0, 0.0])
            rot = [_qmul(_turn(w, rng.uniform(0, 6)), axis_quat(p)) for _ in range(n)]
        return _case(name, cap, None, o, d, rot, he, ground=None)
    if name == "zero_radius_targets":  # a box, a segment (a capsule of radius 0) and a point (a sphere of radius 0: missed)
        o, d = cc._fan(rng, n, c, 9.0)
        d = (np.asarray(three["pos"], np.float64)[np.arange(n) % 3] + rng.uniform(-0.5, 0.5, (n, 3)) - o).astype(np.float32)
        three = dict(three, half_extent=[[1.0, 0.6, 0.8], [0.0, 1.1, 0.0], [0.0, 0.0, 0.0]])
        return _case(name, three, None, o, d, quats(rng, n), he, ground=None)
    if name == "long_thin":
        # long thin boxes across a sparse field of small balls: most contacts lie far from the centre line, in cells that only
        # a grid grown by |he| (not by its largest component) lets the walk meet
        m = 150
        field = dict(pos=np.column_stack([rng.uniform(-15, 15, m), rng.uniform(2, 20, m), rng.uniform(-15, 15, m)]),
                     rot=[IDENT] * m, shape=[SPHERE] * m, half_extent=np.column_stack([rng.uniform(0.1, 0.25, m), np.zeros(m), np.zeros(m)]))
        o = outside(rng, n, [-15, 2, -15], [15, 20, 15], 5.0, 6.0)
        d = rng.uniform([-15, 2, -15], [15, 20, 15], (n, 3)) - o
        return _case(name, field, None, o, d, quats(rng, n), [0.05, 4.5, 0.05], ground=None)
    if name == "wide_cube":
        # cubes of half extent 3 across the same kind of field: their corners reach |he| = 5.2 from the centre line, which a grid
        # grown by the largest component (3) does not cover (long_thin's largest component is its |he| to four digits)
        m = 150
        field = dict(pos=np.column_stack([rng.uniform(-15, 15, m), rng.uniform(2, 20, m), rng.uniform(-15, 15, m)]),
                     rot=[IDENT] * m, shape=[SPHERE] * m, half_extent=np.column_stack([rng.uniform(0.1, 0.25, m), np.zeros(m), np.zeros(m)]))
        o = outside(rng, n, [-15, 2, -15], [15, 20, 15], 7.0, 8.0)
        d = rng.uniform([-15, 2, -15], [15, 20, 15], (n, 3)) - o
        return _case(name, field, None, o, d, quats(rng, n), [3.0, 3.0, 3.0], ground=None)
    if name == "corner_reach":
        # cubes of half extent 3 with a body diagonal along x pass a sheet of small balls in the plane x = 0 at 4.8 from it: only
        # the corner, |he| = 5.2 from the centre, reaches the balls. A grid grown by the largest component (3) ends 3.25 from the
        # sheet and the centre line never enters it; grown by |he| it does
        m = 400
        field = dict(pos=np.column_stack([np.zeros(m), rng.uniform(2, 20, m), rng.uniform(-15, 15, m)]),
                     rot=[IDENT] * m, shape=[SPHERE] * m, half_extent=np.column_stack([rng.uniform(0.1, 0.25, m), np.zeros(m), np.zeros(m)]))
        o = np.column_stack([np.full(n, -4.8), rng.uniform(4, 18, n), np.full(n, -22.0)])
        d = np.column_stack([np.zeros(n), rng.uniform(-0.1, 0.1, n), np.ones(n)])
        diag = np.array([1.0, 1.0, 1.0]) / math.sqrt(3.0)
        q = _turn(np.cross(diag, [1.0, 0.0, 0.0]), math.acos(diag[0]))
        return _case(name, field, None, o, d, [q] * n, [3.0, 3.0, 3.0], ground=None)
    raise ValueError(name)


# ---- the grid's edges: scenes of tests/query_scenes.py ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case(name, kind):
    """kind `mixed`: half extents in [0, 1.2]^3, invalid ones among them; `huge`: one call of 48 whose |he| reaches four times
    the scene's extent"""
    sc = qs.scene(name)
    rng = np.random.default_rng(800 + GRID_SCENES.index(name))
    n = 48 if kind == "huge" else (120 if name == "crowd" else 200)
    lo, hi = qs.bounds(sc)
    ext = float((hi - lo).max())
    rel = outside(rng, n, lo, hi, 5.0, 3.0)
    aim = rng.uniform(lo, hi, (n, 3))
    aim[: n // 8, 1] = -1.0
    he = sizes(rng, n, 0.0, 1.2)
    he[0, 0], he[1, 1], he[2, 2], he[3, 0], he[4, 1], he[5, 2] = -1.0, np.nan, np.inf, np.nan, -0.5, np.inf
    if kind == "huge":
        big = np.arange(8, 10)  # (two: the reference tests each of them against every body at every step)
        he[big] = rng.uniform(0.2, 2.0, (2, 3)).astype(np.float32) * np.float32(ext)
        he[big[0]] = np.float32(4.0 * ext / math.sqrt(3.0))
        v = rng.normal(size=(2, 3))
        v[:, 1] = np.abs(v[:, 1]) + 1.5
        rel[big] = 0.5 * (lo + hi) + 12.0 * ext * v / np.linalg.norm(v, axis=1, keepdims=True)
    o = qs._place(sc, rel)
    d = (aim - rel).astype(np.float32)
    return _case(f"{name} {kind}", dict(sc["bodies"]), sc["statics"], o, d, quats(rng, n), he, ground=sc["ground"], centre=sc["centre"])


# ---- ignore and max_t ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rules_case():
    base = soup(1)
    rng = np.random.default_rng(900)
    n = 200
    o, d, rot, he = (base[k][:n] for k in ("o", "d", "rot", "he"))
    first = base["h"]["body"][:n]
    ig = np.where((first < len(base["bodies"]["pos"])) & (rng.random(n) < 0.67), first, 0xFFFFFFFF).astype(np.uint32)
    t = base["h"]["t"][:n]
    mt = np.where(np.isfinite(t) & (rng.random(n) < 0.5), t * rng.uniform(0.5, 1.5, n), np.inf).astype(np.float32)
    return _case("ignore and max_t", base["bodies"], base["statics"], o, d, rot, he, max_t=mt, ignore=ig)


def all_cases():
    """every seeded input the GPU tests hold against the reference, for the CPU count of near ties"""
    yield from (soup(s) for s in SOUP_SEEDS)
    yield from (degenerate(k) for k in DEGENERATE)
    yield from (grid_case(n, k) for n in GRID_SCENES for k in ("mixed", "huge"))
    yield rules_case()
    yield from (c for _, c in filter_case()[3].values())


# ---- filters: random categories, per-query masks ---------------------------------------------------------------------------
MASKS = (1, 2, 5, 6)
GROUND_CATEGORY = 4


@functools.lru_cache(maxsize=None)
def filter_case():
    """soup 2's first 160 casts under per-query masks: (categories of bodies and statics, masks, {mask: (rows, case)}), each
    case the reference over the targets that mask leaves (the others lose their shape and keep their ids)"""
    base = soup(2)
    rng = np.random.default_rng(950)
    n = 160
    cat = rng.choice([1, 2, 4], len(base["bodies"]["pos"])).astype(np.uint16)
    scat = np.array([1, 2, 4, 2], np.uint16)
    masks = rng.choice(MASKS, n).astype(np.uint16)
    per = {}
    for mask in MASKS:
        k = np.nonzero(masks == mask)[0]
        b = dict(base["bodies"], shape=np.where((cat & mask) != 0, base["bodies"]["shape"], 0).astype(np.uint32))
        s = dict(base["statics"], shape=np.where((scat & mask) != 0, base["statics"]["shape"], 0).astype(np.uint32))
        per[mask] = (k, _case(f"mask {mask}", b, s, base["o"][k], base["d"][k], base["rot"][k], base["he"][k],
                              ground=0.0 if mask & GROUND_CATEGORY else None))
    return cat, scat, masks, per


# ---- a hand scene with closed-form answers ---------------------------------------------------------------------------------
def hand_scene():
    """(bodies, casts): casts a list of dict(name, o, d, rot, he, body, t, normal, point); a None component of point is free
    (the contact is a segment or a polygon: some point of it, see FREE_RANGE)"""
    s2, s3 = math.sqrt(2.0), math.sqrt(3.0)
    bodies = dict(pos=[[0, 5, 0], [10, 5, 0], [20, 5, 0], [30, 5, 0]],
                  rot=[IDENT, _turn([0, 1, 0], math.pi / 4), IDENT, axis_quat([0, 0, 1])],
                  shape=[BOX, BOX, SPHERE, CAPSULE],
                  half_extent=[[1, 1, 1], [1, 1, 1], [1, 0, 0], [0.5, 1, 0]])
    ground = 0xFFFFFFFF
    he = 0.5
    c = []
    add = lambda name, o, d, rot, body, t, normal, point, h=(he, he, he): c.append(
        dict(name=name, o=o, d=d, rot=rot, he=list(h), body=body, t=t, normal=normal, point=point))
    # onto the unit box at (0, 5, 0): t = gap - 1 - reach
    add("cube face to face", [-6, 5.2, 0.3], [1, 0, 0], IDENT, 0, 6 - 1 - he, [-1, 0, 0], [-1, None, None])
    add("cube turned 45 deg about z: edge onto a face", [-6, 5.2, 0.3], [2, 0, 0], _turn([0, 0, 1], math.pi / 4), 0, 6 - 1 - he * s2,
        [-1, 0, 0], [-1, 5.2, None])
    # a body diagonal along u = x: the shortest turn of (1, 1, 1) / sqrt 3 onto x
    diag = np.array([1.0, 1.0, 1.0]) / s3
    ax = np.cross(diag, [1.0, 0.0, 0.0])
    qd = _turn(ax, math.acos(diag[0]))
    add("cube with a body diagonal along u: corner onto a face", [-6, 5.2, 0.3], [1, 0, 0], qd, 0, 6 - 1 - he * s3, [-1, 0, 0], [-1, 5.2, 0.3])
    # crossed edges: the target at (10, 5, 0) is turned 45 deg about y, so its vertical edge x = 10 - sqrt 2 faces -x; the cast
    # cube is turned 45 deg about z, so its edge along z leads: the edges cross at one point, the normal is -x
    add("crossed edges", [4, 5.2, 0.3], [1, 0, 0], _turn([0, 0, 1], math.pi / 4), 1, (6 - s2) - he * s2, [-1, 0, 0], [10 - s2, 5.2, 0])
    add("face-on to a sphere", [20.2, 10, 0.1], [0, -1, 0], IDENT, 2, 5 - 1 - he, [0, 1, 0], [20, 6, 0])
    add("side-on to a capsule", [30.2, 10, 0.1], [0, -1, 0], IDENT, 3, 5 - 0.5 - he, [0, 1, 0], [30, 5.5, None])
    add("end-on to a capsule", [30, 5.1, 6], [0, 0, -1], IDENT, 3, 6 - 1.5 - he, [0, 0, 1], [30, 5, 1.5])
    tilt = _turn([0, 0, 1], math.atan2(0.6, 0.8))  # the box's y axis (-0.6, 0.8, 0): the corner (+x, -y) is lowest
    add("tilted onto the ground", [40, 5, 0], [0, -1, 0], tilt, ground, 5 - (0.8 * 0.3 + 0.6 * 0.3 + 0.0) - 0.0, [0, 1, 0], None,
        h=(0.3, 0.3, 0.2))
    add("level onto the ground", [50, 5, 0], [0, -2, 0], IDENT, ground, 5 - 0.3, [0, 1, 0], [50, 0, 0], h=(0.4, 0.3, 0.2))
    add("starts inside", [0, 5, 0.5], [0, 0, 1], qd, 0, 0.0, [0, 0, -1], [0, 0, 0])
    # the tilted box's lowest feature: signs (-, -, 0): centre - 0.3 * x_axis - 0.3 * y_axis, x_axis = (0.8, 0.6, 0), y_axis = (-0.6, 0.8, 0)
    c[7]["point"] = [40 - 0.3 * 0.8 + 0.3 * 0.6, 0, 0]
    return bodies, c


# the free components of hand_scene's segment and polygon contacts: cast name -> [(component, lo, hi)]
FREE_RANGE = {"cube face to face": [(1, 4.7, 5.7), (2, -0.2, 0.8)],
              "cube turned 45 deg about z: edge onto a face": [(2, -0.2, 0.8)],
              "side-on to a capsule": [(2, -0.4, 0.6)]}


# the cases whose answers are stored (the brute force takes more than about ten seconds for each)
def stored_cases():
    yield from (soup(s) for s in SOUP_SEEDS)
    yield from (grid_case(n, k) for n in GRID_SCENES for k in ("mixed", "huge"))
    yield rules_case()
    yield from (c for _, c in filter_case()[3].values())


if __name__ == "__main__" and sys.argv[1:] == ["--store"]:
    os.makedirs(GOLDEN, exist_ok=True)
    for c in stored_cases():
        if not c["stored"]:
            np.savez_compressed(golden_path(c["label"]), digest=c["digest"], **{k: c["h"][k] for k in STORED})
            print("stored", c["label"])
