"""The query sets of the grid-edge scenes (tests/query_scenes.py) with their float64 answers, computed once per process
and shared, unchanged, by tests/test_query_grid_cpu.py (which counts the references' own ambiguous cases) and
tests/test_gpu_query_grid.py (which holds the kernels to them). numpy and the two references only."""
import functools

import numpy as np

import query_ref
import query_scenes as qs
import raycast_ref

N_RAYS = 3000
N_OVERLAPS = 1500
N_CASTS = {"near": 1500, "farther": 1500, "flung": 1500, "crowd": 400}
CAST_SCENES = tuple(N_CASTS)
PLANE_SCENES = ("one", "flat", "statics_only")
CLUMPS = {"left": np.array([-1.5e6, 0.0, 0.0], np.float32), "right": np.array([1.5e6, 0.0, 0.0], np.float32)}
# crossing rays of `flung`: t is 3e6 there, where float32 resolves 0.25; a ray is kept where its float64 answer stands
# clear of that (see ray_sets)
CROSS_MIN_SPAN, CROSS_MIN_GAP = 0.25, 2.0


def targets(sc):
    return query_ref.targets(sc["bodies"], sc["statics"])


def _cast(sc, o, d, mt, ig, centre=None):
    return raycast_ref.cast(o, d, sc["bodies"], mt, ig, sc["ground"], statics=sc["statics"],
                            centre=sc["centre"] if centre is None else centre)


def plane_rays(sc):
    """rays lying in grid planes, along grid edges and from grid corners (the recipe of
    test_rays_in_grid_planes_and_through_grid_corners) for the grid the scene's bodies give"""
    f = np.float32
    g = qs.grid_of(sc["bodies"])
    lo, cell, dims = g["lo"], g["cell"], g["dims"]
    if not g["valid"]:  # no grid: unit planes above the platform instead
        lo, cell = np.asarray(sc["centre"], f) + np.array([0.5, 1.0, 0.5], f), f(1.0)
    ks = [sorted({0, 1, int(dims[a]) // 2, int(dims[a]) - 1, int(dims[a])}) for a in range(3)]
    top = f(lo[1] + f(dims[1] + 20) * cell)
    o, d = [], []
    for a in ks[1]:
        for b in ks[2]:
            for c in ks[0]:
                px, py, pz = lo[0] + f(c) * cell, lo[1] + f(a) * cell, lo[2] + f(b) * cell
                o.append([lo[0] - f(5) * cell, py, pz]); d.append([1.0, 0.0, 0.0])   # along a grid edge (two planes)
                o.append([px, top, pz]); d.append([0.0, -1.0, 0.3])                  # inside one plane
                o.append([px, py, pz]); d.append([1.0, 1.0, 1.0])                    # from a grid corner, diagonal
                o.append([px, py, pz]); d.append([-1.0, 0.5, 0.0])
    return np.array(o, f), np.array(d, f)


def _crossing(sc):
    """at most 64 rays of `flung` along exactly +-x from beside one clump at the unturned boxes of the other: they walk
    every cell along x. Exact directions and float32 origins: float32 and float64 see the same line. Kept where the float64
    answer is such a box of the other clump with a chord >= CROSS_MIN_SPAN and no second target within CROSS_MIN_GAP."""
    b = sc["bodies"]
    o, d = [], []
    for k in list(range(qs.FLUNG_TARGETS)) + list(range(300, 300 + qs.FLUNG_TARGETS)):
        x, y, z = (float(v) for v in b["pos"][k])
        start = -1.5e6 - 64.0 if x > 0 else 1.5e6 + 64.0
        o.append([start, y, z]); d.append([1.0 if x > 0 else -1.0, 0.0, 0.0])
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    h = _cast(sc, o, d, None, None)
    other = (h["body"] % 300 < qs.FLUNG_TARGETS) & (h["body"] < 600) & (np.sign(b["pos"][np.minimum(h["body"], 599), 0]) != np.sign(o[:, 0]))
    keep = np.nonzero(other & (h["span"] >= CROSS_MIN_SPAN) & (h["t2"] - h["t"] >= CROSS_MIN_GAP))[0][:64]
    return o[keep], d[keep]


@functools.lru_cache(maxsize=None)
def ray_sets(name):
    """the ray query sets of a scene: a list of dict(label, o, d, max_t, ignore, centre, h = the float64 answer). Every
    scene: N_RAYS rays around the centre, plain and with max_t + ignore. `flung`: as many around each clump (centre: the
    clump's), the crossing rays, and short rays (max_t = 5) that start in the empty middle. `one`, `flat`, `statics_only`:
    rays in grid planes and along grid edges."""
    sc = qs.scene(name)
    out = []

    def add(label, o, d, mt=None, ig=None, centre=None):
        out.append(dict(label=f"{name} {label}", o=o, d=d, max_t=mt, ignore=ig, centre=sc["centre"] if centre is None else centre,
                        h=_cast(sc, o, d, mt, ig, centre)))

    # drawn an eighth over, and the first N_RAYS kept whose float64 answer is not ambiguous either way (origins inside two
    # bodies at once, grazing chords): the aims change, not the caps
    o, d, mt, ig = qs.rays(sc, N_RAYS + N_RAYS // 8)
    keep = np.nonzero(~ambiguous_rays(_cast(sc, o, d, None, None)) & ~ambiguous_rays(_cast(sc, o, d, mt, ig)))[0][:N_RAYS]
    assert len(keep) == N_RAYS, (name, len(keep))
    o, d, mt, ig = o[keep], d[keep], mt[keep], ig[keep]
    add("plain", o, d)
    add("max_t + ignore", o, d, mt, ig)
    if name == "flung":
        for side, c in CLUMPS.items():
            clump = dict(sc, centre=c)
            rng = np.random.default_rng(11)
            oo, dd = qs.rays_in(clump, rng, N_RAYS, [-12.0, 0.0, -12.0], [12.0, 22.0, 12.0])
            add(f"{side} clump", oo, dd, centre=c)
        oo, dd = _crossing(sc)
        add("crossing", oo, dd)
        rng = np.random.default_rng(12)
        mid = dict(sc, centre=np.zeros(3, np.float32))
        oo, dd = qs.rays_in(mid, rng, 300, [-1.0e6, 0.0, -12.0], [1.0e6, 22.0, 12.0])
        add("short rays in the middle", oo, dd, np.full(len(oo), 5.0, np.float32))
    if name in PLANE_SCENES:
        add("grid planes", *plane_rays(sc))
    return out


def ambiguous_rays(h):
    """the reference's own ambiguous rays: a hit whose chord is within the tolerance 1e-5 (1 + |o|_inf + t), or with a
    second target within it"""
    hit = np.isfinite(h["t"])
    tol = 1e-5 * (1.0 + np.abs(h["o"]).max(1) + np.where(hit, h["t"], 0.0))
    return hit & ((h["span"] <= tol) | (h["t2"] - np.where(hit, h["t"], 0.0) <= tol))


def _clear(want, margin=2e-4):
    return np.array([not any(abs(s) <= margin for s in close.values()) for _, close in want])


@functools.lru_cache(maxsize=None)
def overlap_set(name):
    """N_OVERLAPS random queries of all three shapes and their float64 lists. `crowd`: a sixth of them small and inside the
    crowded cube. `tiny` (lengths of 1e-3, where 1e-4 is a tenth of a body) and `crowd` (dozens of neighbours around
    every query): drawn over, and the first N_OVERLAPS kept that have no pair within 2e-4 of touching (the aims change,
    not the cap)."""
    sc = qs.scene(name)
    tg = targets(sc)
    n = N_OVERLAPS
    spare = n // 2 if name == "tiny" else (n // 8 if name == "crowd" else 0)
    if name == "crowd":
        k = (n + spare) // 6
        a = qs.overlap_queries(sc, n + spare - k, seed=3)
        b = qs.overlap_queries(sc, k, seed=4, lo=np.array([0.0, 1.0, 0.0]), hi=np.array([4.0, 5.0, 4.0]), size=(0.02, 0.1))
        order = np.random.default_rng(5).permutation(n + spare)  # the two kinds mixed before any is dropped
        q = tuple(np.concatenate([x, y])[order] for x, y in zip(a, b))
    elif name == "flung":  # a third over the whole scene (the ground at most), a third in each clump
        parts = [qs.overlap_queries(sc, n - 2 * (n // 3), seed=3)]
        for k, c in enumerate(CLUMPS.values()):
            c = c.astype(np.float64)
            parts.append(qs.overlap_queries(sc, n // 3, seed=4 + k, lo=c + [-12.0, -0.5, -12.0], hi=c + [12.0, 22.0, 12.0]))
        q = tuple(np.concatenate(x) for x in zip(*parts))
    else:
        q = qs.overlap_queries(sc, n + spare, seed=3)
    want = query_ref.overlap(q[0], q[1], q[2], q[3], tg, ground=sc["ground"], centre=sc["centre"])
    if spare:
        keep = np.nonzero(_clear(want))[0][:n]
        assert len(keep) == n, len(keep)
        q = tuple(x[keep] for x in q)
        want = [want[i] for i in keep]
    return dict(label=f"{name} overlaps", q=q, want=want, tg=tg)


def ambiguous_overlaps(want):
    return sum(1 for _, close in want for s in close.values() if abs(s) <= 1e-4)


def cast_radii(name, kind, n):
    """the radii of a sphere-cast call: 0, 0.25, `mixed` in [0, 1.5] with 2 % invalid, `huge`: a few valid radii up to four
    times the scene's extent among small ones and invalid ones"""
    sc = qs.scene(name)
    rng = np.random.default_rng(31)
    if kind in ("0", "0.25"):
        return np.full(n, float(kind), np.float32)
    rad = rng.uniform(0.0, 1.5, n).astype(np.float32)
    bad = rng.random(n) < 0.02
    rad[bad] = rng.choice(np.array([-1.0, np.nan, np.inf], np.float32), int(bad.sum()))
    if kind == "huge":
        lo, hi = qs.bounds(sc)
        ext = float((hi - lo).max())
        big = rng.choice(np.nonzero(~bad)[0], 6, replace=False)
        rad[big] = rng.uniform(1.0, 4.0, 6).astype(np.float32) * np.float32(ext)
        rad[big[0]] = np.float32(4.0 * ext)
        rest = np.setdiff1d(np.arange(n), big)
        rad[rest[:3]] = np.array([-1.0, np.nan, np.inf], np.float32)  # one of each whatever the draw gave
    return rad


@functools.lru_cache(maxsize=None)
def cast_set(name, kind):
    sc = qs.scene(name)
    n = N_CASTS[name] if kind != "huge" else 48
    centre = sc["centre"]
    if name == "flung":  # around the right clump, measured from it
        centre = CLUMPS["right"]
        o, d = qs.casts(dict(sc, centre=centre), n, lo=[-12.0, 0.0, -12.0], hi=[12.0, 22.0, 12.0])
    else:
        o, d = qs.casts(sc, n)
    rad = cast_radii(name, kind, n)
    tg = targets(sc)
    h = query_ref.spherecast(o, d, rad, tg, ground=sc["ground"], centre=centre)
    return dict(label=f"{name} radius {kind}", o=o, d=d, rad=rad, tg=tg, h=h, centre=centre)
