"""Scenes for the query grid's edges (tests/test_gpu_query_grid.py, tests/test_query_grid_cpu.py), numpy only: what the
grid of physics_amd/csrc/rc_grid.hpp depends on and a compact soup near the origin never varies - the distance from the
origin (the pad is 2^-16 of the largest coordinate), the number of cells along an axis, the table and scan sizes, the
crowding of one bucket, the scale of the lengths.

    sc = scene(name)        dict(name, bodies, statics or None, ground, centre): arrays are float32 / uint32, read-only
    g = grid_of(bodies, grow=0.0)   the header's grid rule restated in float32: pad, cell, lo, dims, bits, valid
    o, d = rays(sc, n, seed) ...    the query sets of the tests, made around the scene's centre

A scene's centre is a float32-exact offset added to a near-origin soup whose coordinates are multiples of 2^-6: `far`
and `farther` are `near` translated without rounding, so relative to the centre they hold the same numbers."""
import functools

import numpy as np

NONE, SPHERE, BOX, CAPSULE = 0, 1, 2, 3
GROUND_HEIGHT = 0.0
NAMES = ("near", "near2048", "far", "farther", "flung", "one", "flat", "crowd", "tiny", "statics_only")
FLUNG_TARGETS = 60
Q = 64.0  # coordinates of the near soup are multiples of 1 / Q: exact in float32 up to 2^18


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _snap(x):
    return (np.round(np.asarray(x, np.float64) * Q) / Q).astype(np.float32)


def _sizes(rng, shape, lo, hi):
    """half extents of sizes lo..hi: sphere radius lo..hi, box half extents lo..0.8 hi, capsule radius lo..0.55 hi and core
    half-length lo..hi (the largest AABB edge stays below 3.2 hi)"""
    n = len(shape)
    he = rng.uniform(lo, hi, (n, 3))
    he[shape == BOX] = rng.uniform(lo, 0.8 * hi, (int((shape == BOX).sum()), 3))
    he[shape == CAPSULE, 0] = rng.uniform(lo, 0.55 * hi, int((shape == CAPSULE).sum()))
    return he.astype(np.float32)


def _soup(rng, n, half, height, lo=0.2, hi=1.5, none=0.05):
    pos = rng.uniform(-half, half, (n, 3))
    pos[:, 1] = rng.uniform(2.0, height, n)  # above the ground plane: no exact ties with it
    shape = rng.choice([SPHERE, BOX, CAPSULE, NONE], n, p=[0.3, 0.35, 0.35 - none, none]).astype(np.uint32)
    return dict(pos=_snap(pos), rot=_quats(rng, n), half_extent=_sizes(rng, shape, lo, hi), shape=shape)


def _statics(rng):
    """one per shape plus a platform (its top a quarter above the ground: no exact ties with the ground plane; its faces off
    the lattice of the positions, like those of every hand-placed box here: no query origin lies exactly on one)"""
    pos = np.array([[0, -0.25, 0], [6, 2, -4], [-5, 1.5, 5], [3, 4, 8]], np.float32)
    shape = np.array([BOX, SPHERE, CAPSULE, BOX], np.uint32)
    he = np.array([[12.003, 0.503, 12.003], [1.5, 0, 0], [0.75, 2, 0], [1, 2, 0.5]], np.float32)
    rot = np.concatenate([np.array([[0, 0, 0, 1]], np.float32), _quats(rng, 3)])
    return dict(pos=pos, rot=rot, half_extent=he, shape=shape)


def _moved(d, centre):
    """d translated by a float32-exact centre (float32 arithmetic: exact for the snapped soups)"""
    if d is None:
        return None
    out = dict(d)
    out["pos"] = (d["pos"] + np.asarray(centre, np.float32)).astype(np.float32)
    return out


def _head(d, n):
    return {k: v[:n].copy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _near():
    rng = np.random.default_rng(4711)
    return _soup(rng, 2049, 40.0, 32.0), _statics(rng)  # more cells (about 2 900) than bodies


def _build(name):
    zero = np.zeros(3, np.float32)
    bodies, statics = _near()
    if name == "near":
        return bodies, statics, zero
    if name == "near2048":
        return _head(bodies, 2048), statics, zero
    if name in ("far", "farther"):
        c = np.array([60_000.0, 0.0, -60_000.0] if name == "far" else [200_000.0, 0.0, -200_000.0], np.float32)
        return _moved(bodies, c), _moved(statics, c), c
    if name == "flung":
        # two clumps 3e6 apart and a few bodies between: about 61 000 cells of edge 49 along x (the pad alone is 23)
        rng = np.random.default_rng(4712)
        parts = []
        for x in (-1.5e6, 1.5e6):
            s = _soup(rng, 300, 10.0, 20.0, hi=0.8)
            s["pos"] = (s["pos"].astype(np.float64) + [x, 0.0, 0.0]).astype(np.float32)
            # the first FLUNG_TARGETS of a clump: boxes that are not turned, for rays along x from the other clump. From 3e6
            # away float32 places a hit within 0.25: enough for which box and which face, not for where on a curved one
            s["shape"][:FLUNG_TARGETS] = BOX
            s["rot"][:FLUNG_TARGETS] = [0.0, 0.0, 0.0, 1.0]
            s["half_extent"][:FLUNG_TARGETS] = rng.uniform(0.3, 0.6, (FLUNG_TARGETS, 3))
            parts.append(s)
        s = _soup(rng, 40, 10.0, 20.0, hi=0.8)
        s["pos"][:, 0] = np.round(rng.uniform(-1.4e6, 1.4e6, 40))
        parts.append(s)
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, None, zero
    if name == "one":
        return dict(pos=np.array([[3.0, 2.0, -1.0]], np.float32), rot=np.array([[0, 0, 0, 1]], np.float32),
                    half_extent=np.array([[1.003, 0.503, 0.753]], np.float32), shape=np.array([BOX], np.uint32)), None, zero
    if name == "flat":
        g = np.stack(np.meshgrid(np.arange(32), [0], np.arange(32), indexing="ij"), -1).reshape(-1, 3)
        pos = (g * 1.5 + [0.0, 2.0, 0.0]).astype(np.float32)
        n = len(pos)
        return dict(pos=pos, rot=np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)),
                    half_extent=np.tile(np.array([0.5, 0, 0], np.float32), (n, 1)), shape=np.full(n, SPHERE, np.uint32)), None, zero
    if name == "crowd":
        # 3000 small bodies in the cube [0, 4] x [1, 5] x [0, 4] and one box of half extent 30 beside it: the cell is the
        # box's edge, so the cube lies in one cell and its records in one bucket
        rng = np.random.default_rng(4713)
        s = _soup(rng, 3000, 2.0, 5.0, lo=0.05, hi=0.2, none=0.02)
        s["pos"] = _snap(np.column_stack([rng.uniform(0, 4, 3000), rng.uniform(1, 5, 3000), rng.uniform(0, 4, 3000)]))
        big = dict(pos=np.array([[36.0, 30.5, 2.0]], np.float32), rot=np.array([[0, 0, 0, 1]], np.float32),
                   half_extent=np.full((1, 3), 30.003, np.float32), shape=np.array([BOX], np.uint32))
        return {k: np.concatenate([s[k], big[k]]) for k in s}, statics, zero
    if name == "tiny":
        b = _head(bodies, 500)
        b["pos"] = (b["pos"] * np.float32(1e-3)).astype(np.float32)
        b["half_extent"] = (b["half_extent"] * np.float32(1e-3)).astype(np.float32)
        return b, None, zero
    if name == "statics_only":
        b = _head(bodies, 64)
        b["shape"] = np.zeros(64, np.uint32)
        return b, statics, zero
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def scene(name):
    bodies, statics, centre = _build(name)
    for d in (bodies, statics):
        if d is not None:
            for k in d:
                d[k] = np.ascontiguousarray(d[k])
                d[k].setflags(write=False)
    centre = centre.copy()
    centre.setflags(write=False)
    return dict(name=name, bodies=bodies, statics=statics, ground=GROUND_HEIGHT, centre=centre,
                scale=1e-3 if name == "tiny" else 1.0)


# ---- the grid rule of rc_grid.hpp in float32 ---------------------------------------------------------------------------
def _rot_f32(rot):
    """quat_to_m33 of include/spec/vec.h, operation by operation in float32 (the build never fuses a * b + c)"""
    f = np.float32
    i, j, k, w = (rot[:, a].astype(f) for a in range(4))
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj = i * j * f(2), w * k * f(2), w * j * f(2)
    ik, jk, wi = i * k * f(2), j * k * f(2), w * i * f(2)
    return [((ww + ii) - jj) - kk, ij - wk, wj + ik, wk + ij, ((ww - ii) + jj) - kk, jk - wi, ik - wj, wi + jk, ((ww - ii) - jj) + kk]


def aabbs(d):
    """(lo, hi, shaped) of the exact float32 AABBs (body_aabb of include/spec/collide.h with margin 0); shaped: a sphere,
    box or capsule with a finite box"""
    f = np.float32
    pos = np.asarray(d["pos"], f).reshape(-1, 3)
    n = len(pos)
    he = np.asarray(d["half_extent"], f).reshape(-1, 3)
    shape = np.asarray(d["shape"]).reshape(-1)
    rot = np.tile(np.array([0, 0, 0, 1], f), (n, 1)) if d.get("rot") is None else np.asarray(d["rot"], f).reshape(-1, 4)
    m = _rot_f32(rot)
    e = np.zeros((n, 3), f)
    for a in range(3):
        box = (np.abs(m[3 * a]) * he[:, 0] + np.abs(m[3 * a + 1]) * he[:, 1]) + np.abs(m[3 * a + 2]) * he[:, 2]
        cap = np.abs(m[3 * a + 1]) * he[:, 1] + he[:, 0]
        e[:, a] = np.where(shape == SPHERE, he[:, 0], np.where(shape == BOX, box, cap))
    lo, hi = (pos - e).astype(f), (pos + e).astype(f)
    with np.errstate(all="ignore"):
        shaped = np.isin(shape, (SPHERE, BOX, CAPSULE)) & np.isfinite(lo.sum(1) + hi.sum(1))
    return lo, hi, shaped


def grid_rule(lo, hi, e, valid=True):
    """rc_grid of rc_grid.hpp from the header's values (scene bounds lo, hi and largest AABB edge e, float32): pad, cell,
    inv, grid origin, cells per axis, and whether the 2^20 coarsening branch was taken"""
    f = np.float32
    lo, hi, e = np.asarray(lo, f), np.asarray(hi, f), f(e)
    if not valid:
        lo, hi, e = np.zeros(3, f), np.zeros(3, f), f(0)
    m = f(max(np.abs(lo).max(), np.abs(hi).max())) if valid else f(0)
    with np.errstate(all="ignore"):
        pad = f(2.0 ** -16) * (m + e)
        glo = (lo - pad).astype(f)
        span3 = ((hi + pad) - glo).astype(f)
        cell = (e + f(2) * pad) * f(1 + 2.0 ** -10)
        span = f(span3.max())
        coarse = bool(span * f(2.0 ** -20) > cell)
        if coarse:
            cell = span * f(2.0 ** -20)
        cell = f(max(cell, f(1.0e-30)))
        inv = f(1) / cell
        c = np.floor(span3 * inv) + f(1)
        dims = np.clip(c, 1, 2 ** 20 + 1).astype(np.int64) if valid else np.ones(3, np.int64)
    return dict(pad=pad, cell=cell, inv=inv, lo=glo, dims=dims, coarse=coarse, valid=bool(valid), edge=e)


def grid_of(bodies, grow=0.0):
    """The grid a query call builds over `bodies` (every AABB grown by `grow`, a sphere cast's largest valid radius), and
    bits: the hashed table has 2^bits buckets (a power of two >= 2 n, 4096 at least)."""
    f = np.float32
    lo, hi, shaped = aabbs(bodies)
    n = len(lo)
    bits = 12
    while (1 << bits) < 2 * n:
        bits += 1
    if not shaped.any():
        g = grid_rule(np.zeros(3), np.zeros(3), 0.0, valid=False)
    else:
        lo, hi = (lo[shaped] - f(grow)).astype(f), (hi[shaped] + f(grow)).astype(f)
        g = grid_rule(lo.min(0), hi.max(0), (hi - lo).max())
    g.update(bits=bits, n_bodies=n, body_lo=lo, body_hi=hi, shaped=shaped)
    return g


def coord(g, x, axis):
    """rc_coord: the cell of coordinate x along an axis (clamped to the grid)"""
    f = np.float32
    with np.errstate(all="ignore"):
        c = np.floor((np.asarray(x, f) - g["lo"][axis]) * g["inv"])
    return np.clip(np.nan_to_num(c, nan=0.0), 0, g["dims"][axis] - 1).astype(np.int64)


def cells_of(g, lo, hi):
    """rc_body_cells for AABBs lo, hi (n, 3): the low cell per axis and the high one (at most one further)"""
    f = np.float32
    c0 = np.stack([coord(g, np.asarray(lo, f)[:, a] - g["pad"], a) for a in range(3)], 1)
    c1 = np.stack([coord(g, np.asarray(hi, f)[:, a] + g["pad"], a) for a in range(3)], 1)
    return c0, np.minimum(c1, c0 + 1)


def covered_cells(g, lo, hi):
    """the number of cells an overlap query with the exact AABB lo, hi covers (k_ov_query: above n_bodies it tests every
    body directly instead of walking the grid)"""
    f = np.float32
    n = 1
    for a in range(3):
        n *= int(coord(g, f(hi[a]) + g["pad"], a)) - int(coord(g, f(lo[a]) - g["pad"], a)) + 1
    return n


def bucket(x, y, z, bits):
    h = ((x * 73856093) ^ (y * 19349663) ^ (z * 83492791)) & 0xFFFFFFFF
    return ((h * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)


def bucket_loads(g):
    """records per bucket: every shaped body once per cell it occupies"""
    c0, c1 = cells_of(g, g["body_lo"], g["body_hi"])
    load = np.zeros(1 << g["bits"], np.int64)
    cells = set()
    for a, b in zip(c0, c1):
        for z in range(a[2], b[2] + 1):
            for y in range(a[1], b[1] + 1):
                for x in range(a[0], b[0] + 1):
                    load[bucket(int(x), int(y), int(z), g["bits"])] += 1
                    cells.add((int(x), int(y), int(z)))
    return load, cells


# ---- query sets ----------------------------------------------------------------------------------------------------------
def bounds(sc):
    """(lo, hi) of the shaped bodies' centres (of the statics' where no body has a shape), relative to the centre"""
    b = sc["bodies"]
    keep = b["shape"] != NONE
    pos = b["pos"][keep] if keep.any() else sc["statics"]["pos"]
    rel = pos.astype(np.float64) - sc["centre"]
    return rel.min(0), rel.max(0)


def _place(sc, rel):
    """centre + rel in float32, with rel snapped to the soup's lattice (scaled) so that a translated scene gets the
    translated query exactly"""
    s = sc["scale"]
    return (np.round(np.asarray(rel, np.float64) / s * Q) / Q * s + sc["centre"].astype(np.float64)).astype(np.float32)


def rays_in(sc, rng, n, lo, hi):
    """the recipe of tests/test_gpu_raycast.py (_rays) in the box lo..hi relative to the centre: a third inside the
    bounds, a third from far outside aimed into them, a third along the ground; random lengths"""
    k = n // 3
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, size = (lo + hi) / 2, float((hi - lo).max())
    o1 = rng.uniform(lo, hi, (k, 3))
    d1 = rng.normal(size=(k, 3))
    v = rng.normal(size=(k, 3))
    o2 = c + 2.0 * size * v / np.linalg.norm(v, axis=1, keepdims=True)
    d2 = rng.uniform(lo, hi, (k, 3)) - o2
    m = n - 2 * k
    s = sc["scale"]
    o3 = np.column_stack([rng.uniform(lo[0], hi[0], m), rng.uniform(0.02, 0.5, m) * s + sc["ground"], rng.uniform(lo[2], hi[2], m)])
    d3 = np.column_stack([rng.normal(size=m), rng.uniform(-0.2, 0.2, m), rng.normal(size=m)])
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    d *= rng.uniform(0.1, 10.0, (n, 1))
    return _place(sc, o), d.astype(np.float32)


def rays(sc, n=3000, seed=1):
    """(origins, dirs, max_t, ignore): n rays around the scene's centre, and the max_t / ignore of the second run"""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(sc)
    m = 2.0 * sc["scale"]
    lo, hi = lo - m, hi + m
    lo[1] = max(lo[1], sc["ground"] + 0.02 * sc["scale"])  # origins above the ground plane (the platform lies in it)
    o, d = rays_in(sc, rng, n, lo, hi)
    size = float((hi - lo).max())
    mt = np.where(rng.random(n) < 0.3, rng.uniform(0, 1.5 * size, n), np.inf).astype(np.float32)
    nb = len(sc["bodies"]["pos"])
    ig = np.where(rng.random(n) < 0.1, rng.integers(0, nb, n), 0xFFFFFFFF).astype(np.uint32)
    return o, d, mt, ig


def casts(sc, n, seed=2, lo=None, hi=None):
    """ball casts: origins in and around the box lo..hi (default: the bounds), three quarters aimed into it"""
    rng = np.random.default_rng(seed)
    if lo is None:
        lo, hi = bounds(sc)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    m = 3.0 * sc["scale"]
    o = rng.uniform(lo - m, hi + m, (n, 3))
    o[:, 1] = rng.uniform(sc["ground"], hi[1] + m, n)
    aim = rng.uniform(lo, hi, (n, 3))
    d = aim - o
    d[: n // 4] = rng.normal(size=(n // 4, 3))
    return _place(sc, o), d.astype(np.float32)


def overlap_queries(sc, n=1500, seed=3, lo=None, hi=None, size=(0.1, 2.0)):
    """(shape, pos, rot, half_extent) of n query shapes of all three kinds in lo..hi (default: the bounds, one size out)"""
    rng = np.random.default_rng(seed)
    s = sc["scale"]
    if lo is None:
        lo, hi = bounds(sc)
        lo, hi = lo - size[1] * s, hi + size[1] * s
        lo[1] = sc["ground"] - 0.5 * s
    qp = rng.uniform(lo, hi, (n, 3))
    qs = rng.choice([SPHERE, BOX, CAPSULE], n).astype(np.uint32)
    qh = (rng.uniform(size[0], size[1], (n, 3)) * s).astype(np.float32)
    return qs, _place(sc, qp), _quats(rng, n), qh


def sweep_rays(sc, n=4):
    """n rays along +x from outside the grid, in the gap between the highest AABB and the grid's top (half the pad above
    the bodies), spread over z: they miss every body and pass through every cell of a row"""
    f = np.float32
    g = grid_of(sc["bodies"])
    top = f(g["body_hi"][:, 1].max())  # (body_lo, body_hi: the shaped bodies only)
    y = top + f(0.5) * g["pad"]
    z0, z1 = f(g["body_lo"][:, 2].min()), f(g["body_hi"][:, 2].max())
    o = np.array([[g["lo"][0] - f(3) * g["cell"], y, z0 + (z1 - z0) * f((k + 0.5) / n)] for k in range(n)], f)
    return o, np.tile(np.array([1.0, 0.0, 0.0], f), (n, 1))
