"""Reference of the static-collider pair search (physics_amd/csrc/static.hip) for tests/test_gpu_static_independent.py,
and the scenes of those tests. numpy and pair_ref only; shares no code with the collision header, the grid build or the
CPU checker.

    static_pairs(body_box, static_box)   sorted (i, k): the closed intervals of body box i and static box k overlap on all
                                         three axes (<=: touching counts), in float32 as given, by dense comparison (at
                                         most 1000 x 600 here). A NaN or inverted body box meets nothing.
    static_boxes64(static, margin)       pair_ref.aabbs of the static set: the float64 definition of the fattened boxes.

The body boxes are the world's own (get_aabbs()); the float32 static boxes are the ones the world uploads, written out by
tests/cpp/static_set_cli.cpp, which also reports the grid build_static_set gives a scene. tests/test_static_ref_cpu.py holds
those boxes to static_boxes64 (measured worst deviation 2.45 ulps; tolerance pair_ref.AABB_TOL_ULPS) and every
scene to the case it is named for, from the figures below.

Scenes (each a function of a seed; SEEDS are the committed ones; margin 0.02 unless stated):
  tiles(n)     24 x 24 box tiles, half extents (0.3, 0.25, 0.3), pitch 0.6, tops at y = 0; n bodies of all three shapes,
               random rotations, half extents 0.3 - 0.7, centres at y = 0.49 scattered over and beyond the floor.
               n in TILES_N: either side of a wave, one past a 256-thread workgroup.
  mixed(n)     240 small statics (half extents 0.2 - 0.6) and 50 mid ones (0.3 - 2.5), all shapes, random rotations, in a
               30 x 6 x 30 volume; a floor slab, four walls and a long capsule along x. Bodies in a volume 12 wider on
               every side, half extents 0.2 - 1.5, every fiftieth 3 - 5, 5 % without a shape.
  line(axis)   600 small statics strung over 3000 units along the axis (centred on the origin); 257 bodies, 253 near
               randomly chosen statics - every other one near a static within 95 of the origin - and four far beyond
               both ends (their cells are clamped).
  touching     contact_margin 2^-5; axis-aligned boxes with identity rotations on dyadic coordinates inside [8, 16), where
               every fattened face is exact in float32 (all are multiples of 2^-5, or one ulp = 2^-20 off). The statics'
               fattened boxes are 1 wide, so the cell edge is exactly 1 and the grid's origin 9: every fattened static face
               lies on a cell boundary or half way. Per face of a static: a body whose box touches it exactly (a pair) and
               the same body one float32 ulp farther (no pair); then statics across a cell boundary with bodies whose
               face lies exactly on that boundary inside them.
  only_large   no static set with sane coordinates has every static on the LARGE list: the cell edge is the median of
               the largest box edges, and a static no larger than the cell covers at most 3 x 3 x 3 = 27 <= 64 cells
               (setup.hpp `covered`). So: a floor slab and two walls on the LARGE list, and four small statics 200 units
               away from every body, which give the grid its cell and never meet a body's box: every pair comes from the list.
  one          a single static box under three bodies.

SCENE_TABLE, held by test_static_ref_cpu.py (pairs from the CPU checker's body boxes, bit-equal to the device's; the other
figures from static_set_cli): pairs, n_large, grid, longest cell list, largest span of a small static in cells, largest
first cell, small statics in more than one cell, most pairs of one body; then whether the scene's pairs meet
shape_pair_ref's floors of 25 % contacts and 25 % clear misses (the GPU test asserts them only where they hold here).

    scene       pairs large   grid          list   span   first cell  multi per body contacts / misses  floors
    tiles_1         9     0   24 x 2 x 24      9   2 1 2  21 0 21       576       9        5 /    4   yes
    tiles_63      549     0   24 x 2 x 24      9   2 1 2  21 0 21       576      20      274 /  272   yes
    tiles_64      558     0   24 x 2 x 24      9   2 1 2  21 0 21       576      20      280 /  275   yes
    tiles_65      564     0   24 x 2 x 24      9   2 1 2  21 0 21       576      20      282 /  279   yes
    tiles_257    2093     0   24 x 2 x 24      9   2 1 2  21 0 21       576      20      980 / 1102   yes
    mixed_257      67    32   22 x 7 x 21      6   4 4 4  19 3 18       253       6       41 /   26   yes
    mixed_1000    455    32   22 x 7 x 21      6   4 4 4  19 3 18       253      61      226 /  229   yes
    line_x        251     0   984 x 3 x 3      2   2 2 2  982 0 0       385       1      218 /   27   no
    line_y        251     0   3 x 984 x 3      2   2 2 2  0 982 0       372       1      218 /   27   no
    line_z        251     0   3 x 3 x 984      2   2 2 2  0 0 982       359       1      218 /   27   no
    touching       12     0   7 x 7 x 7        1   2 2 2  4 4 4          18       1        6 /    6   yes
    only_large    134     3   4 x 4 x 4        2   2 2 2  1 1 1           4       3      130 /    3   no
    one             2     0   3 x 2 x 2        1   2 2 2  0 0 0           1       1        2 /    0   no
"""
import numpy as np

import pair_ref as pr

STATIC_ID_BIT = 0x80000000
MARGIN = pr.MARGIN
TOUCH_MARGIN = 2.0 ** -5
TILES_N = (1, 63, 64, 65, 257)
MIXED_N = (257, 1000)
AXES = ("x", "y", "z")
SEEDS = {"tiles": 1, "mixed": 4, "line": 1, "touching": 1, "only_large": 1, "one": 1}
MEASURED_STATIC_BOX_ULPS = 2.45

# name -> (pairs, n_large, grid, longest cell list, span, first cell, multi-cell statics, most pairs of a body, shares hold)
SCENE_TABLE = {
    "tiles_1": (9, 0, (24, 2, 24), 9, (2, 1, 2), (21, 0, 21), 576, 9, True),
    "tiles_63": (549, 0, (24, 2, 24), 9, (2, 1, 2), (21, 0, 21), 576, 20, True),
    "tiles_64": (558, 0, (24, 2, 24), 9, (2, 1, 2), (21, 0, 21), 576, 20, True),
    "tiles_65": (564, 0, (24, 2, 24), 9, (2, 1, 2), (21, 0, 21), 576, 20, True),
    "tiles_257": (2093, 0, (24, 2, 24), 9, (2, 1, 2), (21, 0, 21), 576, 20, True),
    "mixed_257": (67, 32, (22, 7, 21), 6, (4, 4, 4), (19, 3, 18), 253, 6, True),
    "mixed_1000": (455, 32, (22, 7, 21), 6, (4, 4, 4), (19, 3, 18), 253, 61, True),
    "line_x": (251, 0, (984, 3, 3), 2, (2, 2, 2), (982, 0, 0), 385, 1, False),
    "line_y": (251, 0, (3, 984, 3), 2, (2, 2, 2), (0, 982, 0), 372, 1, False),
    "line_z": (251, 0, (3, 3, 984), 2, (2, 2, 2), (0, 0, 982), 359, 1, False),
    "touching": (12, 0, (7, 7, 7), 1, (2, 2, 2), (4, 4, 4), 18, 1, True),
    "only_large": (134, 3, (4, 4, 4), 2, (2, 2, 2), (1, 1, 1), 4, 3, False),
    "one": (2, 0, (3, 2, 2), 1, (2, 2, 2), (0, 0, 0), 1, 1, False),
}


# ------------------------------------------------------------------------------------------------ the reference
def static_pairs(body_box, static_box):
    b = np.asarray(body_box, np.float32).reshape(-1, 6)
    s = np.asarray(static_box, np.float32).reshape(-1, 6)
    live = (b[:, :3] <= b[:, 3:]).all(axis=1)  # False for an inverted box and for a NaN
    meet = live[:, None]
    for a in range(3):
        meet = meet & (b[:, None, a] <= s[None, :, 3 + a]) & (s[None, :, a] <= b[:, None, 3 + a])
    i, k = np.nonzero(meet)  # row-major: sorted by (i, k)
    return np.stack([i, k], axis=1).astype(np.uint32)


def static_boxes64(static, margin):
    return pr.aabbs(static["pos"], static["rot"], static["shape"], static["he"], margin)


def box_gaps64(body_box64, static_box64, pairs):
    """Per pair the largest per-axis separation of the two float64 boxes (negative: they overlap by that much on every
    axis), and the float32 ulp it is to be judged in (of the largest coordinate involved, at least 1)."""
    b, s = np.asarray(body_box64)[pairs[:, 0]], np.asarray(static_box64)[pairs[:, 1]]
    gap = np.maximum(b[:, :3] - s[:, 3:], s[:, :3] - b[:, 3:])
    unit = np.spacing(np.maximum(1.0, np.maximum(np.abs(b), np.abs(s)).max(axis=1)).astype(np.float32)).astype(np.float64)
    return gap.max(axis=1), unit


# ------------------------------------------------------------------------------------------------ the scenes
def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _identity(n):
    q = np.zeros((n, 4))
    q[:, 3] = 1.0
    return q


def _set(pos, rot, shape, he):
    return dict(pos=np.asarray(pos, np.float64).reshape(-1, 3).astype(np.float32), rot=np.asarray(rot, np.float64).reshape(-1, 4).astype(np.float32),
                shape=np.asarray(shape).astype(np.uint32).reshape(-1), he=np.asarray(he, np.float64).reshape(-1, 3).astype(np.float32))


def _scene(static, body, margin=MARGIN):
    return dict(static=static, body=body, margin=float(margin))


def tiles(n, seed=SEEDS["tiles"]):
    rng = np.random.default_rng(seed)
    side = 24
    ix, iz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pos = np.stack([(ix.ravel() - 0.5 * (side - 1)) * 0.6, np.full(side * side, -0.25), (iz.ravel() - 0.5 * (side - 1)) * 0.6], axis=1)
    static = _set(pos, _identity(side * side), np.full(side * side, pr.SHAPE_BOX), np.tile([0.3, 0.25, 0.3], (side * side, 1)))
    # (drawn for the largest n and cut, so that the first bodies of every n are the same)
    m = max(TILES_N)
    bpos = np.stack([rng.uniform(-8.0, 8.0, m), np.full(m, 0.49), rng.uniform(-8.0, 8.0, m)], axis=1)
    bpos[0, [0, 2]] = (0.21, -0.33)  # n = 1: the one body stands on the floor
    body = _set(bpos[:n], _quats(rng, m)[:n], rng.integers(1, 4, m)[:n], rng.uniform(0.3, 0.7, (m, 3))[:n])
    return _scene(static, body)


def _container(half, height, wall=0.5):
    """floor slab and four walls around [-half, half]^2 x [0, height]: (pos, he), boxes with identity rotations"""
    w = half + wall
    pos = [(0, -wall, 0), (-w, height / 2, 0), (w, height / 2, 0), (0, height / 2, -w), (0, height / 2, w)]
    he = [(w + wall, wall, w + wall), (wall, height / 2 + wall, w), (wall, height / 2 + wall, w), (w, height / 2 + wall, wall), (w, height / 2 + wall, wall)]
    return np.array(pos, np.float64), np.array(he, np.float64)


def mixed(n, seed=SEEDS["mixed"]):
    rng = np.random.default_rng(seed)
    vol_lo, vol_hi = np.array([-15.0, 0.0, -15.0]), np.array([15.0, 6.0, 15.0])
    ns, nm = 240, 50
    pos = rng.uniform(vol_lo, vol_hi, (ns + nm, 3))
    he = np.concatenate([rng.uniform(0.2, 0.6, (ns, 3)), rng.uniform(0.3, 2.5, (nm, 3))])
    shape = rng.integers(1, 4, ns + nm)
    rot = _quats(rng, ns + nm)
    cpos, che = _container(15.0, 6.0)
    s = np.sqrt(0.5)
    pos = np.concatenate([pos, cpos, [[0.0, 3.0, 0.0]]])
    he = np.concatenate([he, che, [[0.4, 14.0, 0.0]]])  # the capsule: radius 0.4, core half-length 14 ...
    rot = np.concatenate([rot, _identity(5), [[0.0, 0.0, -s, s]]])  # ... its local y turned onto x
    shape = np.concatenate([shape, np.full(5, pr.SHAPE_BOX), [pr.SHAPE_CAPSULE]])
    order = rng.permutation(len(pos))  # the large ones anywhere in the id range
    static = _set(pos[order], rot[order], shape[order], he[order])
    bpos = rng.uniform(vol_lo - 12.0, vol_hi + 12.0, (n, 3))
    bhe = rng.uniform(0.2, 1.5, (n, 3))
    bhe[::50] = rng.uniform(3.0, 5.0, (len(bhe[::50]), 3))
    bshape = rng.integers(1, 4, n)
    bshape[rng.permutation(n)[: n // 20]] = pr.SHAPE_NONE
    return _scene(static, _set(bpos, _quats(rng, n), bshape, bhe))


def line(axis, seed=SEEDS["line"]):
    a = AXES.index(axis)
    rng = np.random.default_rng(seed)
    ns, nb = 600, 257
    pos = rng.uniform(-1.0, 1.0, (ns, 3))
    pos[:, a] = np.linspace(-1500.0, 1500.0, ns) + rng.uniform(-1.0, 1.0, ns)
    static = _set(pos, _quats(rng, ns), rng.integers(1, 4, ns), rng.uniform(0.2, 0.6, (ns, 3)))
    near = rng.integers(0, ns, nb)
    mid = np.flatnonzero(np.abs(pos[:, a]) < 95.0)  # every other body within 100 of the origin, where shape_pair_ref's
    near[::2] = mid[rng.integers(0, len(mid), len(near[::2]))]  # tolerances hold: their manifolds are checked in full
    bpos = pos[near] + rng.uniform(-0.8, 0.8, (nb, 3))
    far = np.zeros((4, 3))
    far[:, a] = (-2600.0, -1600.0, 1600.0, 2600.0)
    bpos[[0, 100, 200, 256]] = far  # far beyond both ends
    return _scene(static, _set(bpos, _quats(rng, nb), rng.integers(1, 4, nb), rng.uniform(0.3, 0.7, (nb, 3))))


def touching(seed=SEEDS["touching"]):
    """See the module docstring. Returns the scene with two more entries: `touch` and `apart`, the (body, static) pairs whose
    boxes touch exactly and lie one ulp apart."""
    rng = np.random.default_rng(seed)
    m = TOUCH_MARGIN
    hs, hb = 0.5 - m, 0.25  # the fattened static is 1 wide, the fattened body 0.5625
    slots = [(9.5 + 2.0 * x, 9.5 + 2.0 * y, 9.5 + 2.0 * z) for z in range(3) for y in range(3) for x in range(3)]
    order = rng.permutation(len(slots))
    spos, bpos, touch, apart = [], [], [], []
    for f in range(6):            # the six faces: the body on the -x, +x, -y, ... side of its static
        a, sign = f // 2, (-1.0 if f % 2 == 0 else 1.0)
        for ulp in (0, 1):
            c = np.array(slots[order[len(spos)]], np.float32)
            b = c.copy()
            b[a] = np.float32(c[a] + sign * (0.5 + hb + m))   # exact: multiples of 2^-5 inside [8, 16)
            if ulp:
                b[a] = np.nextafter(b[a], np.float32(sign * 100.0))
            (apart if ulp else touch).append((len(bpos), len(spos)))
            spos.append(c); bpos.append(b)
    for f in range(6):            # statics across a cell boundary of that axis, a body face exactly on the boundary inside them
        a, sign = f // 2, (-1.0 if f % 2 == 0 else 1.0)
        c = np.array(slots[order[len(spos)]], np.float32)
        c[a] += np.float32(0.5)                         # fattened [c - 0.5, c + 0.5]: the boundary c (an integer) in its middle
        b = c.copy()
        b[a] = np.float32(c[a] + sign * (hb + m))       # the body's near face on the boundary
        touch.append((len(bpos), len(spos)))
        spos.append(c); bpos.append(b)
    ns, nb = len(spos), len(bpos)
    static = _set(spos, _identity(ns), np.full(ns, pr.SHAPE_BOX), np.full((ns, 3), hs))
    body = _set(bpos, _identity(nb), np.full(nb, pr.SHAPE_BOX), np.full((nb, 3), hb))
    sc = _scene(static, body, m)
    sc["touch"], sc["apart"] = np.array(touch[:6], np.uint32), np.array(apart, np.uint32)
    sc["inside"] = np.array(touch[6:], np.uint32)
    return sc


def only_large(seed=SEEDS["only_large"]):
    rng = np.random.default_rng(seed)
    cpos, che = _container(8.0, 4.0)
    big = [0, 1, 3]  # the slab and two walls that meet in a corner
    small = np.array([[200.0, 0.0, 0.0], [201.0, 0.0, 0.0], [200.0, 1.0, 0.0], [200.0, 0.0, 1.0]])
    pos = np.concatenate([small[:2], cpos[big], small[2:]])
    he = np.concatenate([np.full((2, 3), 0.3), che[big], np.full((2, 3), 0.3)])
    static = _set(pos, _identity(7), np.full(7, pr.SHAPE_BOX), he)
    n = 130
    bpos = rng.uniform((-8.0, 0.2, -8.0), (8.0, 4.0, 8.0), (n, 3))
    bpos[:40, 1] = rng.uniform(0.2, 0.6, 40)                    # on the floor
    bpos[40:70, 0] = rng.uniform(-8.0, -7.4, 30)                # at the -x wall
    bpos[70:90, 2] = rng.uniform(-8.0, -7.4, 20)                # at the -z wall
    bpos[90:100, [0, 2]] = rng.uniform(-8.0, -7.4, (10, 2))     # in the corner
    bpos[90:100, 1] = rng.uniform(0.2, 0.6, 10)
    return _scene(static, _set(bpos, _quats(rng, n), rng.integers(1, 4, n), rng.uniform(0.3, 0.7, (n, 3))))


def one(seed=SEEDS["one"]):
    rng = np.random.default_rng(seed)
    static = _set([[1.0, 2.0, 3.0]], _identity(1), [pr.SHAPE_BOX], [[0.5, 0.5, 0.5]])
    bpos = np.array([[1.2, 2.9, 3.1], [1.0, 4.5, 3.0], [0.2, 2.0, 3.6]])
    return _scene(static, _set(bpos, _quats(rng, 3), [pr.SHAPE_SPHERE, pr.SHAPE_BOX, pr.SHAPE_CAPSULE], rng.uniform(0.3, 0.6, (3, 3))))


SCENES = {}
for _n in TILES_N:
    SCENES[f"tiles_{_n}"] = (lambda n=_n: tiles(n))
for _n in MIXED_N:
    SCENES[f"mixed_{_n}"] = (lambda n=_n: mixed(n))
for _a in AXES:
    SCENES[f"line_{_a}"] = (lambda a=_a: line(a))
SCENES["touching"] = touching
SCENES["only_large"] = only_large
SCENES["one"] = one


def scene(name):
    return SCENES[name]()


def write_static_file(path, static):
    """The input of tests/cpp/static_set_cli.cpp."""
    with open(path, "wb") as f:
        f.write(np.uint64(len(static["pos"])).tobytes() + static["pos"].tobytes() + static["rot"].tobytes()
                + static["shape"].astype(np.uint32).tobytes() + static["he"].tobytes())


def parse_cli(text):
    """The figures static_set_cli prints, as a dict."""
    t = text.split()
    i = [int(x) for x in t[:4] + t[5:13]]
    return dict(n_large=i[0], dim=tuple(i[1:4]), cell=float(t[4]), longest=i[4], span=tuple(i[5:8]), first=tuple(i[8:11]), multi=i[11],
                org=tuple(float(x) for x in t[13:16]), cells=int(t[16]))
