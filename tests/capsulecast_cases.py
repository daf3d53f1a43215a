"""The seeded inputs of the capsule-cast tests with their float64 answers (tests/capsulecast_ref.py), computed once per
process and shared, unchanged, by tests/test_capsulecast_cpu.py (which counts the reference's own near ties) and
tests/test_gpu_capsulecast.py (which holds the kernel to them). numpy and the references only.

A case: dict(label, bodies, statics, ground, centre, o, d, rot, rad, hq, max_t, ignore, tg, h)."""
import functools
import math

import numpy as np

import capsulecast_ref as ref
import query_ref
import query_scenes as qs
from raycast_ref import rotation_matrices

SPHERE, BOX, CAPSULE = qs.SPHERE, qs.BOX, qs.CAPSULE
SOUP_SEEDS = (1, 2)
GRID_SCENES = ("near", "farther", "crowd")
IDENT = [0.0, 0.0, 0.0, 1.0]


def quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def axis_quat(axis):
    """the shortest turn of the y axis onto `axis`, [i, j, k, w]"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    y = np.array([0.0, 1.0, 0.0])
    c = float(y @ a)
    if c < -1.0 + 1e-12:
        return [1.0, 0.0, 0.0, 0.0]
    v = np.cross(y, a)
    q = np.array([v[0], v[1], v[2], 1.0 + c])
    return list(q / np.linalg.norm(q))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _case(label, bodies, statics, o, d, rot, rad, hq, ground=0.0, centre=None, max_t=None, ignore=None, tg=None):
    f = np.float32
    n = len(o)
    o, d = np.asarray(o, f).reshape(-1, 3), np.asarray(d, f).reshape(-1, 3)
    rot = None if rot is None else np.asarray(rot, f).reshape(-1, 4)
    rad, hq = np.broadcast_to(np.asarray(rad, f), (n,)).copy(), np.broadcast_to(np.asarray(hq, f), (n,)).copy()
    bodies = {k: np.asarray(v, np.uint32 if k == "shape" else f) for k, v in bodies.items()}
    if tg is None:
        tg = query_ref.targets(bodies, statics)
    h = ref.capsulecast(o, d, rot, rad, hq, tg, max_t=max_t, ignore=ignore, ground=ground, centre=centre)
    return _frozen(dict(label=label, bodies=bodies, statics=statics, ground=ground, centre=centre, o=o, d=d, rot=rot, rad=rad,
                        hq=hq, max_t=max_t, ignore=ignore, tg=tg, h=h))


# ---- random soups: all three shapes plus NONE, the four statics of test_gpu_query.py, the ground ---------------------------
def soup_bodies(rng, n, extent):
    pos = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.0, extent, n)
    shape = rng.choice([1, 2, 3, 0], n, p=[0.3, 0.35, 0.3, 0.05]).astype(np.uint32)
    he = rng.uniform(0.2, 1.2, (n, 3)).astype(np.float32)
    return dict(pos=pos, rot=quats(rng, n), shape=shape, half_extent=he)


def soup_statics(rng):
    # a raised platform (its top 0.3 above the ground: no exact ties with the ground plane), a ball, a capsule, a box
    pos = np.array([[0, -0.2, 0], [6, 2, -4], [-5, 1, 5], [3, 4, 8]], np.float32)
    shape = np.array([2, 1, 3, 2], np.uint32)
    he = np.array([[10, 0.5, 10], [1.5, 0, 0], [0.7, 2, 0], [1, 2, 0.5]], np.float32)
    rot = np.concatenate([np.array([IDENT], np.float32), quats(rng, 3)])
    return dict(pos=pos, rot=rot, shape=shape, half_extent=he)


def outside(rng, n, lo, hi, clear, floor):
    """n points in the box lo - clear - 6 .. hi + clear + 6 that lie at least `clear` outside lo..hi and above `floor`: a
    capsule of reach R + h <= clear that starts there touches nothing yet (a cast that starts touching several targets
    is an exact tie at t = 0, which says nothing about the sweep)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.zeros((0, 3))
    while len(out) < n:
        p = rng.uniform(lo - clear - 6.0, hi + clear + 6.0, (4 * n, 3))
        p[:, 1] = np.maximum(p[:, 1], floor)
        keep = ((p < lo - clear) | (p > hi + clear)).any(1)
        out = np.concatenate([out, p[keep]])
    return out[:n]


def soup_casts(rng, n, extent):
    lo, hi = np.array([-extent, 0.0, -extent]), np.array([extent, extent, extent])
    o = outside(rng, n, lo, hi, 3.0, 3.0).astype(np.float32)
    aim = rng.uniform(lo, hi, (n, 3))
    aim[: n // 6, 1] = -1.0  # some at the platform and the ground beside it
    d = (aim - o).astype(np.float32)
    d[n // 6: n // 4] = rng.normal(size=(n // 4 - n // 6, 3))
    rad = rng.uniform(0.0, 1.0, n).astype(np.float32)
    hq = rng.uniform(0.0, 1.5, n).astype(np.float32)
    hq[rng.random(n) < 0.1] = 0.0
    rad[rng.random(n) < 0.1] = 0.0
    return o, d, quats(rng, n), rad, hq


@functools.lru_cache(maxsize=None)
def soup(seed, n_bodies=300, n_casts=600, extent=15.0):
    rng = np.random.default_rng(100 + seed)
    bodies = soup_bodies(rng, n_bodies, extent)
    statics = soup_statics(rng)
    o, d, rot, rad, hq = soup_casts(rng, n_casts, extent)
    return _case(f"soup seed {seed}", bodies, statics, o, d, rot, rad, hq)


# ---- degenerate orientations: one call each ---------------------------------------------------------------------------------
def _fan(rng, n, centre, reach):
    """n casts from a shell around `centre` aimed at points near it"""
    v = rng.normal(size=(n, 3))
    o = np.asarray(centre) + reach * v / np.linalg.norm(v, axis=1, keepdims=True)
    aim = np.asarray(centre) + rng.uniform(-1.2, 1.2, (n, 3))
    return o.astype(np.float32), (aim - o).astype(np.float32)


DEGENERATE = ("box_axis", "box_face_plane", "capsule_parallel", "capsule_antiparallel", "capsule_perpendicular",
              "capsule_near_parallel", "segment", "zero_radii", "long_thin")


@functools.lru_cache(maxsize=None)
def degenerate(name, n=120):
    rng = np.random.default_rng(500 + DEGENERATE.index(name))
    c = np.array([0.0, 6.0, 0.0])
    tilt = axis_quat([0.3, 1.0, -0.2])  # the target capsule's own turn
    w = rotation_matrices(np.array([tilt]))[0][:, 1]
    box = dict(pos=[c], rot=[IDENT], shape=[BOX], half_extent=[[1.0, 0.6, 0.8]])
    cap = dict(pos=[c], rot=[tilt], shape=[CAPSULE], half_extent=[[0.4, 1.1, 0.0]])
    three = dict(pos=[c, c + [4.0, 0, 0], c - [4.0, 0, 0]], rot=[IDENT, tilt, IDENT], shape=[BOX, CAPSULE, SPHERE],
                 half_extent=[[1.0, 0.6, 0.8], [0.0, 1.1, 0.0], [0.0, 0.0, 0.0]])
    o, d = _fan(rng, n, c, 7.0)
    rad = rng.uniform(0.05, 0.6, n)
    hq = rng.uniform(0.2, 1.4, n)
    if name == "box_axis":  # a exactly along a box axis: x, y and z in turn
        rot = [axis_quat(e) for e in ([1, 0, 0], [0, 1, 0], [0, 0, 1])] * (n // 3)
        return _case(name, box, None, o, d, rot, rad, hq, ground=None)
    if name == "box_face_plane":  # a in a face plane of the box (no component along one axis), not along an axis
        rot = []
        for k in range(n):
            ang = rng.uniform(0.2, 1.3)
            e = [[math.cos(ang), math.sin(ang), 0], [0, math.cos(ang), math.sin(ang)], [math.sin(ang), 0, math.cos(ang)]][k % 3]
            rot.append(axis_quat(e))
        # the turn is exact only for some: the box frame is the world's, so a's third component is zero or one rounding
        return _case(name, box, None, o, d, rot, rad, hq, ground=None)
    if name.startswith("capsule_"):
        if name == "capsule_parallel":
            a = w
        elif name == "capsule_antiparallel":
            a = -w
        elif name == "capsule_perpendicular":
            a = np.cross(w, [1.0, 0.0, 0.0])
        else:
            p = np.cross(w, [0.0, 0.0, 1.0])
            a = w + 1e-3 * p / np.linalg.norm(p)  # 1e-3 rad from parallel
        rot = [tilt if name == "capsule_parallel" else axis_quat(a)] * n
        return _case(name, cap, None, o, d, rot, rad, hq, ground=None)
    if name == "long_thin":
        # long thin capsules across a sparse field of small balls: most contacts lie far from the centre line, in cells
        # that only a grid grown by R + h (not by R) lets the walk meet
        m = 150
        field = dict(pos=np.column_stack([rng.uniform(-15, 15, m), rng.uniform(2, 20, m), rng.uniform(-15, 15, m)]),
                     rot=[IDENT] * m, shape=[SPHERE] * m, half_extent=np.column_stack([rng.uniform(0.1, 0.25, m), np.zeros(m), np.zeros(m)]))
        o = outside(rng, n, [-15, 2, -15], [15, 20, 15], 5.0, 6.0)
        d = rng.uniform([-15, 2, -15], [15, 20, 15], (n, 3)) - o
        return _case(name, field, None, o, d, quats(rng, n), 0.05, 4.5, ground=None)
    if name == "segment":  # R = 0: a swept segment against a box, a capsule and a sphere
        o, d = _fan(rng, n, c, 9.0)
        d = (np.asarray(three["pos"], np.float64)[np.arange(n) % 3] + rng.uniform(-0.8, 0.8, (n, 3)) - o).astype(np.float32)
        three = dict(three, half_extent=[[1.0, 0.6, 0.8], [0.4, 1.1, 0.0], [0.9, 0.0, 0.0]])
        return _case(name, three, None, o, d, quats(rng, n), 0.0, hq, ground=None)
    if name == "zero_radii":  # r + R = 0: a swept segment against a box, a segment (a capsule of radius 0: crossed where
        # the swept parallelogram meets it) and a point (a sphere of radius 0: a set of measure zero, missed)
        o, d = _fan(rng, n, c, 9.0)
        d = (np.asarray(three["pos"], np.float64)[np.arange(n) % 3] + rng.uniform(-0.5, 0.5, (n, 3)) - o).astype(np.float32)
        return _case(name, three, None, o, d, quats(rng, n), 0.0, hq, ground=None)
    raise ValueError(name)


# ---- the grid's edges: scenes of tests/query_scenes.py ---------------------------------------------------------------------
def _mixed_sizes(rng, n):
    rad = rng.uniform(0.0, 1.0, n).astype(np.float32)
    hq = rng.uniform(0.0, 1.5, n).astype(np.float32)
    hq[rng.random(n) < 0.1] = 0.0
    bad = np.array([-1.0, np.nan, np.inf], np.float32)
    rad[:3] = bad       # one of each whatever the draw gives
    hq[3:6] = bad
    return rad, hq


@functools.lru_cache(maxsize=None)
def grid_case(name, kind):
    """kind `mixed`: R in [0, 1], h in [0, 1.5], invalid ones among them; `huge`: one call of 48 whose R + h reaches four
    times the scene's extent"""
    sc = qs.scene(name)
    rng = np.random.default_rng(700 + GRID_SCENES.index(name))
    n = 48 if kind == "huge" else (160 if name == "crowd" else 300)
    lo, hi = qs.bounds(sc)
    ext = float((hi - lo).max())
    # origins outside the bodies' bounds by more than the largest R + h (2.5) plus the largest body, above the ground
    rel = outside(rng, n, lo, hi, 5.0, 3.0)
    aim = rng.uniform(lo, hi, (n, 3))
    aim[: n // 8, 1] = -1.0
    rad, hq = _mixed_sizes(rng, n)
    if kind == "huge":
        # R + h up to four times the scene's extent, from twelve extents away and high above the ground
        big = np.arange(8, 10)  # (two: the reference tests each of them against every body at every step)
        rad[big] = rng.uniform(0.2, 2.0, 2).astype(np.float32) * np.float32(ext)
        hq[big] = rng.uniform(0.2, 2.0, 2).astype(np.float32) * np.float32(ext)
        rad[big[0]], hq[big[0]] = np.float32(2.0 * ext), np.float32(2.0 * ext)
        v = rng.normal(size=(2, 3))
        v[:, 1] = np.abs(v[:, 1]) + 1.5
        rel[big] = 0.5 * (lo + hi) + 12.0 * ext * v / np.linalg.norm(v, axis=1, keepdims=True)
    o = qs._place(sc, rel)
    d = (aim - rel).astype(np.float32)
    return _case(f"{name} {kind}", dict(sc["bodies"]), sc["statics"], o, d, quats(rng, n), rad, hq, ground=sc["ground"],
                 centre=sc["centre"])


# ---- ignore and max_t ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rules_case():
    base = soup(1)
    rng = np.random.default_rng(900)
    n = 300
    o, d, rot, rad, hq = (base[k][:n] for k in ("o", "d", "rot", "rad", "hq"))
    first = base["h"]["body"][:n]
    # ignore what the plain call hit (where that is a body), for two thirds; a max_t around the plain t for half
    ig = np.where((first < len(base["bodies"]["pos"])) & (rng.random(n) < 0.67), first, 0xFFFFFFFF).astype(np.uint32)
    t = base["h"]["t"][:n]
    mt = np.where(np.isfinite(t) & (rng.random(n) < 0.5), t * rng.uniform(0.5, 1.5, n), np.inf).astype(np.float32)
    return _case("ignore and max_t", base["bodies"], base["statics"], o, d, rot, rad, hq, max_t=mt, ignore=ig)


def all_cases():
    """every seeded input the GPU tests hold against the reference, for the CPU count of near ties"""
    yield from (soup(s) for s in SOUP_SEEDS)
    yield from (degenerate(k) for k in DEGENERATE)
    yield from (grid_case(n, k) for n in GRID_SCENES for k in ("mixed", "huge"))
    yield rules_case()


# ---- filters: random categories, per-query masks ---------------------------------------------------------------------------
MASKS = (1, 2, 5, 6)
GROUND_CATEGORY = 4


@functools.lru_cache(maxsize=None)
def filter_case():
    """soup 2's first 200 casts under per-query masks: (categories of bodies and statics, masks, {mask: (rows, case)}), each
    case the reference over the targets that mask leaves (the others lose their shape and keep their ids)"""
    base = soup(2)
    rng = np.random.default_rng(950)
    n = 200
    cat = rng.choice([1, 2, 4], len(base["bodies"]["pos"])).astype(np.uint16)
    scat = np.array([1, 2, 4, 2], np.uint16)
    masks = rng.choice(MASKS, n).astype(np.uint16)
    per = {}
    for mask in MASKS:
        k = np.nonzero(masks == mask)[0]
        b = dict(base["bodies"], shape=np.where((cat & mask) != 0, base["bodies"]["shape"], 0).astype(np.uint32))
        s = dict(base["statics"], shape=np.where((scat & mask) != 0, base["statics"]["shape"], 0).astype(np.uint32))
        per[mask] = (k, _case(f"mask {mask}", b, s, base["o"][k], base["d"][k], base["rot"][k], base["rad"][k], base["hq"][k],
                              ground=0.0 if mask & GROUND_CATEGORY else None))
    return cat, scat, masks, per


# ---- a hand scene with closed-form answers ---------------------------------------------------------------------------------
def hand_scene():
    """(bodies, casts): casts a list of dict(name, o, d, axis, rad, hq, body, t, normal, point); a None component of point is
    free (the contact is a line: some point of it, see free_range)"""
    s2 = math.sqrt(0.5)
    bodies = dict(pos=[[0, 5, 0], [10, 5, 0], [20, 5, 0], [30, 5, 0]],
                  rot=[IDENT, axis_quat([0, 0, 1]), IDENT, IDENT],
                  shape=[BOX, CAPSULE, SPHERE, CAPSULE],
                  half_extent=[[1, 1, 1], [0.5, 1, 0], [1, 0, 0], [0.5, 1, 0]])
    ground = 0xFFFFFFFF
    c = []
    add = lambda name, o, d, axis, body, t, normal, point, rad=0.5, hq=1.0: c.append(
        dict(name=name, o=o, d=d, axis=axis, rad=rad, hq=hq, body=body, t=t, normal=normal, point=point))
    add("upright, side-on to a box face", [-5, 5.2, 0.3], [1, 0, 0], [0, 1, 0], 0, 3.5, [-1, 0, 0], [-1, None, 0.3])
    add("end ball on a box face", [-6, 5.2, 0.3], [1, 0, 0], [1, 0, 0], 0, 3.5, [-1, 0, 0], [-1, 5.2, 0.3])
    add("core across a box edge", [-5, 6.3, 0], [1, 0, 0], [0, 0, 1], 0, 3.6, [-0.8, 0.6, 0], [-1, 6, None])
    add("core across a box corner", [-5, 6 + 0.3 * s2, 1 + 0.3 * s2], [1, 0, 0], [0, s2, -s2], 0, 3.6, [-0.8, 0.6 * s2, 0.6 * s2],
        [-1, 6, 1])
    add("crossed capsules: the sum's face, t = gap - (r + R)", [5, 5.3, 0.2], [1, 0, 0], [0, 1, 0], 1, 4.0, [-1, 0, 0], [9.5, 5, 0.2])
    add("parallel capsules", [25, 5.5, 0], [1, 0, 0], [0, 1, 0], 3, 4.0, [-1, 0, 0], [29.5, None, 0])
    add("collinear capsules", [30, 12, 0], [0, -1, 0], [0, 1, 0], 3, 4.0, [0, 1, 0], [30, 6.5, 0])
    add("a sphere target under the core", [20.5, 10, 0], [0, -1, 0], [1, 0, 0], 2, 3.5, [0, 1, 0], [20, 6, 0])
    add("tilted onto the ground", [40, 5, 0], [0, -1, 0], [0.6, 0.8, 0], ground, 3.7, [0, 1, 0], [39.4, 0, 0])
    add("level onto the ground", [50, 5, 0], [0, -2, 0], [1, 0, 0], ground, 4.5, [0, 1, 0], [None, 0, 0])
    add("starts overlapping", [0, 5, 0], [0, 0, 1], [0.6, 0.8, 0], 0, 0.0, [0, 0, -1], [0, 0, 0])
    return bodies, c


# the free components of hand_scene's line contacts: cast name -> (component, lo, hi)
FREE_RANGE = {"upright, side-on to a box face": (1, 4.2, 6.0), "core across a box edge": (2, -1.0, 1.0),
              "parallel capsules": (1, 4.5, 6.0), "level onto the ground": (0, 49.0, 51.0)}
