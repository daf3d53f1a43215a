"""The seeded scenes and characters of the character walking tests, and the float64 walk of every character
(tests/character_ref.py over tests/capsulecast_ref.py), computed once per process and shared, unchanged, by
tests/test_character_cpu.py (which counts the reference's own near ties) and tests/test_gpu_character.py. numpy and the
references only.

The slide scenes are tests/slide_cases.py's (soup, statics, empty: 600 characters, a seeded half of them grounded_in). The
terrain scene is statics only plus the ground, in lanes along x, 8 apart in z:
  lane 0  stairs with risers of 0.2 (below step_height)        lane 1  stairs with risers of 0.5 (above it)
  lane 2  a ramp of 30 degrees (walkable)                      lane 3  a ramp of 60 degrees (too steep)
  lane 4  a platform 0.1 high (a ledge below snap_distance)    lane 5  a platform 0.5 high (a ledge above it)
  lane 6  a riser of 0.2 under a low ceiling
Terrain characters are upright and start `skin` above a floor by construction (the ground, a platform, a stair's tread, the
30 degree ramp), or in the air above one.

A case: dict(label, bodies, statics, ground, tg, pos, motion, rot, rad, hq, grounded, skin, params)."""
import functools
import math

import numpy as np

import capsulecast_ref as ref
import character_ref
import query_ref
import slide_cases

SKIN = 0.02
STEP_HEIGHT, SNAP_DISTANCE = 0.3, 0.2
MIN_FLOOR_NY = float(np.float32(math.cos(math.radians(45.0))))
MAX_SLIDES = 4
SCENES = ("soup", "statics", "empty", "terrain")
N_TERRAIN = 600
LANE = 8.0
BOX = 2
MISS, GROUND = 0xFFFFFFFE, 0xFFFFFFFF


def params(max_slides=MAX_SLIDES):
    """(skin, max_slides, step_height, snap_distance, min_floor_ny) as float32 sees them"""
    f = lambda x: float(np.float32(x))
    return f(SKIN), max_slides, f(STEP_HEIGHT), f(SNAP_DISTANCE), MIN_FLOOR_NY


def _zquat(deg):
    a = math.radians(deg) / 2.0
    return [0.0, 0.0, math.sin(a), math.cos(a)]


def ramp(x0, z0, deg, length=8.0, half_width=3.0, thick=0.5):
    """a box turned about z whose top face rises from the line (x0, 0, z0 +- half_width) towards +x: (pos, rot, half extent)"""
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    corner = np.array([-length / 2 * c - thick * s, -length / 2 * s + thick * c])  # R (-length / 2, thick)
    return [x0 - corner[0], 0.0 - corner[1], z0], _zquat(deg), [length / 2, thick, half_width]


@functools.lru_cache(maxsize=None)
def terrain():
    """(statics, regions): regions are where characters may stand: (lane, x range, floor height at x as (y0, slope), cos of the
    floor's angle)"""
    pos, rot, he = [], [], []
    regions = []

    def box(lo, hi):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        pos.append((lo + hi) / 2); rot.append([0.0, 0.0, 0.0, 1.0]); he.append((hi - lo) / 2)

    for lane, rise in ((0, 0.2), (1, 0.5)):
        z0 = lane * LANE
        for k in range(4):
            x = 2.0 + 0.6 * k
            box([x, -1.0, z0 - 3.0 - 0.05 * k], [8.0 + 0.1 * k, rise * (k + 1), z0 + 3.0 + 0.05 * k])
            regions.append((lane, (x + 0.05, x + 0.55 if k < 3 else 7.5), (rise * (k + 1), 0.0), 1.0))
        regions.append((lane, (-3.0, 1.9), (0.0, 0.0), 1.0))
    for lane, deg in ((2, 30.0), (3, 60.0)):
        p, q, h = ramp(2.0, lane * LANE, deg)
        pos.append(p); rot.append(q); he.append(h)
        regions.append((lane, (-3.0, 1.9), (0.0, 0.0), 1.0))
        if deg == 30.0:
            regions.append((lane, (2.5, 2.0 + 7.0 * math.cos(math.radians(deg))), (-2.0 * math.tan(math.radians(deg)), math.tan(math.radians(deg))),
                            math.cos(math.radians(deg))))
    for lane, height in ((4, 0.1), (5, 0.5)):
        z0 = lane * LANE
        box([-6.0, -1.0, z0 - 3.0], [0.0, height, z0 + 3.0])
        regions.append((lane, (-5.5, -0.02), (height, 0.0), 1.0))
        regions.append((lane, (0.3, 3.0), (0.0, 0.0), 1.0))
    z0 = 6 * LANE
    box([2.0, -1.0, z0 - 3.0], [8.0, 0.2, z0 + 3.0])
    box([-2.0, 1.75, z0 - 3.2], [8.5, 2.5, z0 + 3.2])
    regions.append((6, (-1.5, 1.9), (0.0, 0.0), 1.0))
    regions.append((6, (2.3, 7.0), (0.2, 0.0), 1.0))
    m = len(pos)
    statics = dict(pos=np.array(pos, np.float32), rot=np.array(rot, np.float32), shape=np.full(m, BOX, np.uint32), half_extent=np.array(he, np.float32))
    return slide_cases._frozen(statics), tuple(regions)


def scene(name):
    """(bodies or None, statics or None, ground height or None)"""
    if name == "terrain":
        return None, terrain()[0], 0.0
    return slide_cases.scene(name)


def _terrain_characters(rng, n):
    f = np.float32
    _, regions = terrain()
    got = {k: [] for k in ("pos", "rad", "hq", "motion", "grounded")}
    have = 0
    tg = query_ref.targets(None, terrain()[0])
    while have < n:
        m = 2 * n
        which = rng.integers(0, len(regions), m)
        rad = rng.uniform(0.2, 0.3, m).astype(f)
        hq = rng.uniform(0.4, 0.55, m).astype(f)
        x = np.array([rng.uniform(*regions[k][1]) for k in which])
        z = np.array([regions[k][0] * LANE for k in which]) + rng.uniform(-2.0, 2.0, m)
        floor = np.array([regions[k][2][0] + regions[k][2][1] * xx for k, xx in zip(which, x)])
        cosine = np.array([regions[k][3] for k in which])
        airborne = rng.random(m) < 0.2
        # the lowest point of an upright capsule is its lower ball's: skin clear of a plane of angle a it stands (R + skin) / cos a
        # above the plane's point below its centre
        y = floor + (rad + SKIN) / cosine + hq + np.where(airborne, rng.uniform(0.1, 0.6, m), 0.0)
        pos = np.stack([x, y, z], axis=1).astype(f)
        ang = np.radians(rng.uniform(-50.0, 50.0, m)) + np.where(rng.random(m) < 0.75, 0.0, math.pi)
        length = rng.uniform(0.3, 1.5, m)
        kind = rng.random(m)
        my = np.where(airborne, rng.uniform(-1.0, -0.3, m), np.where(kind < 0.6, 0.0, np.where(kind < 0.8, -0.05, np.where(kind < 0.9, 0.5, 0.0))))
        motion = np.stack([length * np.cos(ang), my, length * np.sin(ang)], axis=1).astype(f)
        motion[(kind >= 0.9) & ~airborne] = [0.0, -0.05, 0.0]  # standing still under gravity
        rot = np.tile(np.array([0, 0, 0, 1], f), (m, 1))
        keep = slide_cases.separation(pos, rot, rad, hq, tg, 0.0) >= 0.5 * SKIN
        for k, v in (("pos", pos), ("rad", rad), ("hq", hq), ("motion", motion), ("grounded", (~airborne).astype(np.uint32))):
            got[k].append(v[keep])
        have += int(keep.sum())
    return {k: np.concatenate(v)[:n] for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    bodies, statics, ground = scene(name)
    if name == "terrain":
        tg = query_ref.targets(None, statics)
        c = _terrain_characters(np.random.default_rng(5200), N_TERRAIN)
        n = N_TERRAIN
        rot = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))
        return slide_cases._frozen(dict(label="character terrain", bodies=None, statics=statics, ground=ground, tg=tg, pos=c["pos"], motion=c["motion"],
                                        rot=rot, rad=c["rad"], hq=c["hq"], grounded=c["grounded"], skin=SKIN))
    s = slide_cases.case(name)
    grounded = (np.random.default_rng(5100 + slide_cases.SCENES.index(name)).random(len(s["pos"])) < 0.5).astype(np.uint32)
    return slide_cases._frozen(dict(label=f"character {name}", bodies=s["bodies"], statics=s["statics"], ground=s["ground"], tg=s["tg"], pos=s["pos"],
                                    motion=s["motion"], rot=s["rot"], rad=s["rad"], hq=s["hq"], grounded=grounded, skin=SKIN))


def ref_cast_many(c, trace=None):
    """the float64 capsule cast of case c's characters, as character_ref.walk_many takes it. trace: a list that receives, per
    cast, (character, the reference's t, its second-best t, the cast's tolerance)"""
    def cast_many(rows, p, d, max_t):
        h = ref.capsulecast(p, d, c["rot"][rows], c["rad"][rows], c["hq"][rows], c["tg"], max_t=max_t, ground=c["ground"])
        out = []
        for j, i in enumerate(rows):
            if trace is not None:
                tol = 1e-5 * (1.0 + float(np.abs(p[j]).max()) + float(c["hq"][i]) + (float(h["t"][j]) if math.isfinite(h["t"][j]) else 0.0))
                trace.append((int(i), float(h["t"][j]), float(h["t2"][j]), tol))
            out.append(None if h["body"][j] == MISS else (int(h["body"][j]), float(h["t"][j]), h["normal"][j]))
        return out
    return cast_many


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the float64 walk of every character of case(name), which characters are near ties). A near tie: a reference cast whose
    two best candidates lie within 4 tol, a classified |n.y - min_floor_ny| below 1e-4, or a progress comparison within tol."""
    c = case(name)
    trace = []
    f64 = lambda a: np.asarray(a, np.float64)
    walks = character_ref.walk_many(ref_cast_many(c, trace), f64(c["pos"]), f64(c["motion"]), c["grounded"], *params())
    n = len(c["pos"])
    tie = np.zeros(n, bool)
    for i, t, t2, tol in trace:
        if math.isfinite(t2) and t2 - t <= 4 * tol:
            tie[i] = True
    for i, w in enumerate(walks):
        tol = 1e-5 * (1.0 + float(np.abs(c["pos"][i]).max()) + float(c["hq"][i]) + float(np.linalg.norm(c["motion"][i])))
        if any(x < 1e-4 for x in w["audit"]["ny"]):
            tie[i] = True
        pr = w["audit"]["progress"]
        if pr is not None and abs(pr[0] - pr[1]) <= 4 * tol * max(1.0, float(np.linalg.norm(c["motion"][i]))):
            tie[i] = True
    return walks, tie


def tie_cap(n):
    """the GPU property test may skip at most 2 % of the characters as near ties"""
    return n // 50
