"""CPU: character walking's rule. The spec header alone (include/spec/character.h through tests/cpp/character_probe.cpp, built
once plain and once under the address and undefined-behaviour sanitizers) against the float64 statement of
tests/character_ref.py, case by case over analytic casts (half-spaces, boxes, wedges; scripted answers where no geometry
reaches a path); the reference's own count of near ties over every seeded scene of tests/test_gpu_character.py; the declared
symbols and the Python surface's argument errors."""
import math
import os
import re

import numpy as np
import pytest

import character_cases as cases
import character_probe as probe
import character_ref as ref
import slide_ref

F = np.float32
MISS = probe.MISS
SKIN, STEP, SNAP, NY = 0.02, 0.3, 0.2, cases.MIN_FLOOR_NY


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("character") / "character_probe"), sanitize=request.param == "sanitized")


# ---- analytic casts for a point character: convex solids as lists of (unit normal n, c): inside where n . x <= c everywhere ------
def halfspace(n, c):
    return [(np.asarray(n, np.float64), float(c))]


def box(lo, hi):
    out = []
    for a in range(3):
        e = np.zeros(3); e[a] = 1.0
        out += [(e, float(hi[a])), (-e, -float(lo[a]))]
    return out


GROUND = halfspace([0, 1, 0], 0.0)


def slope(ny, x0=2.0, sign=1.0):
    """a wedge whose face rises towards +x from the line x = x0, y = 0, with the unit normal (-sqrt(1 - ny^2), ny, 0) rounded to
    float32 (sign -1: an overhang, the normal's y negated and the solid above it)"""
    n = np.array([-math.sqrt(1.0 - ny * ny), sign * ny, 0.0]).astype(F).astype(np.float64)
    return [(n, float(n @ [x0, 0.0, 0.0])), (np.array([1.0, 0, 0]), x0 + 10.0), (np.array([0, -sign, 0.0]), 1.0 if sign > 0 else 5.0)]


def solid_cast(solids):
    """cast(p, d, max_t) of a point against convex solids (ids in order): the first entry, t = 0 with the normal -u from inside
    or on a solid; t and the normal as float32 sees them, so that both sides decide on the same numbers"""
    def cast(p, d, max_t):
        p, d = np.asarray(p, np.float64), np.asarray(d, np.float64)
        u = d / np.linalg.norm(d)
        best = None
        for k, planes in enumerate(solids):
            t_in, t_out, n_in = -np.inf, np.inf, None
            for n, c in planes:
                dist, den = n @ p - c, n @ u
                if den == 0:
                    if dist > 0:
                        t_in = np.inf
                elif den < 0:
                    if -dist / den > t_in:
                        t_in, n_in = -dist / den, n
                else:
                    t_out = min(t_out, -dist / den)
            if t_in > t_out or t_out < 0:
                continue
            t, n = (0.0, -u) if t_in <= 0 else (float(F(t_in)), n_in)
            if t <= max_t and (best is None or t < best[1]):
                best = (k, t, np.asarray(n, F).astype(np.float64))
        return best
    return cast


def script(*answers):
    """a cast that gives the listed answers in order, whatever is asked"""
    left = list(answers)
    return lambda p, d, max_t: left.pop(0)


RISER_LOW, RISER_HIGH = box([2, -1, -50], [12, 0.2, 50]), box([2, -1, -50], [12, 0.5, 50])
STEEP_N, FLOOR_N = math.cos(math.radians(60.0)), math.cos(math.radians(30.0))
# a point character standing inside the 2 skin band above the ground
Y0 = 0.75 * SKIN
UPN, WALLN = [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]

# (name, the cast (a factory, since scripts are consumed), pos, motion, grounded, overrides of the call's values, what the
# reference's branches must contain, flags that must be set, flags that must be clear)
G, S, N, O, W, C, B, E = ref.GROUNDED, ref.STEPPED, ref.SNAPPED, ref.ON_STEEP, ref.HIT_WALL, ref.HIT_CEILING, ref.BLOCKED, ref.EXHAUSTED
CASES = [
    # the three classes at and around min_floor_ny (walking into a slope whose normal's y is set to the float32 next to the limit)
    ("class: floor at the limit", lambda: solid_cast([GROUND, slope(NY)]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["plane", "ground:"], 0, W | S),
    ("class: floor above the limit", lambda: solid_cast([GROUND, slope(float(np.nextafter(F(NY), F(1))))]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["plane"], 0, W),
    ("class: steep below the limit", lambda: solid_cast([GROUND, slope(float(np.nextafter(F(NY), F(0))))]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["noclimb"], W, 0),
    ("class: wall", lambda: solid_cast([GROUND, RISER_HIGH]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["plane", "step:no progress"], W | G, S),
    ("class: overhang", lambda: solid_cast([GROUND, slope(STEEP_N, sign=-1.0)]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["plane"], W | G, C),
    # the no-climb rule: rising keeps the true normal and climbs, level follows the contour, falling slides down
    ("no climb: rising", lambda: solid_cast([GROUND, slope(STEEP_N)]), [1, Y0, 0], [2, 0.2, 0.3], 1, {}, ["move:plane"], W, S | C),
    ("no climb: level", lambda: solid_cast([GROUND, slope(STEEP_N)]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["plane+noclimb"], W, 0),
    ("no climb: level, head on", lambda: solid_cast([GROUND, slope(STEEP_N)]), [1, Y0, 0], [2, 0, 0], 1, {}, ["plane+noclimb"], W | G, S),
    ("no climb: falling onto it", lambda: solid_cast([GROUND, slope(STEEP_N)]), [3, 2.5, 0], [0.3, -1.5, 0.2], 0, {}, ["move:plane", "ground:steep"], W | O, G),
    ("no climb: walking down onto it", lambda: solid_cast([GROUND, slope(STEEP_N)]), [3, 2.5, 0], [0.3, -1.5, 0.2], 1, {}, ["move:plane"], W, 0),
    # each way the step is given up, and both sides of the acceptance
    ("step: taken", lambda: solid_cast([GROUND, RISER_LOW]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["step:taken"], G | S, W | N),
    ("step: no progress", lambda: solid_cast([GROUND, RISER_HIGH]), [1, Y0, 0], [2, 0, 0], 1, {}, ["step:no progress", "ground:grounded"], G | W, S),
    ("step: no room", lambda: solid_cast([GROUND, RISER_LOW, halfspace([0, -1, 0], -(Y0 + 0.015))]), [1, Y0, 0], [2, 0, 0], 1, {}, ["step:no room"], G | W, S),
    ("step: lift clamped", lambda: solid_cast([GROUND, RISER_LOW, halfspace([0, -1, 0], -(Y0 + 0.27))]), [1, Y0, 0], [2, 0, 0], 1, {}, ["step:taken"], G | S, 0),
    ("step: no landing", lambda: solid_cast([box([-10, -1, -50], [2.1, 0, 50]), box([2, -1, -50], [2.1, 0.2, 50])]), [1, Y0, 0], [2, 0, 0], 1, {},
     ["step:no landing", "ground:grounded"], G | W, S),
    ("step: not a floor", lambda: solid_cast([GROUND, box([2, -1, -50], [2.1, 0.2, 50]), slope(STEEP_N, x0=2.1)]), [1, Y0, 0], [2, 0, 0], 1, {},
     ["step:not a floor"], W, S),
    ("step: no step height", lambda: solid_cast([GROUND, RISER_LOW]), [1, Y0, 0], [2, 0, 0.3], 1, dict(step_height=0.0), ["move:plane", "ground:grounded"], G | W, S),
    ("step: not grounded_in", lambda: solid_cast([GROUND, RISER_LOW]), [1, Y0, 0], [2, 0, 0.3], 0, {}, ["move:plane", "ground:grounded"], G | W, S),
    ("step: no horizontal motion", lambda: solid_cast([GROUND, slope(STEEP_N, x0=0.99)]), [1, 0.5, 0], [0, -1, 0], 1, {}, ["move:plane"], W, S),
    # BLOCKED in each phase (scripted where no geometry starts a later cast touching)
    ("blocked: move", lambda: solid_cast([GROUND]), [1, -0.1, 0], [1, 0, 0], 1, {}, ["move:blocked"], B, G | S | O),
    ("blocked: up cast", lambda: script((1, 0.5, WALLN), (2, 0.0, [0, -1.0, 0]), (0, SKIN, UPN)), [1, Y0, 0], [1, 0, 0], 1, {},
     ["step:no room", "ground:grounded"], G | W, S | B),
    ("blocked: lifted slide", lambda: script((1, 0.5, WALLN), None, None, (2, 0.0, WALLN), (0, SKIN, UPN)), [1, Y0, 0], [1, 0, 0.5], 1, {},
     ["step:blocked", "ground:grounded"], G | W, S | B),
    ("blocked: down cast", lambda: script((1, 0.5, WALLN), None, None, (0, 0.0, UPN), (0, SKIN, UPN)), [1, Y0, 0], [1, 0, 0], 1, {},
     ["step:no landing", "ground:grounded"], G | W, S),
    ("blocked: ground cast", lambda: script(None, (0, 0.0, UPN)), [1, Y0, 0], [1, 0, 0], 1, {}, ["move:miss", "ground:none"], 0, G | N | O),
    # the 2 skin band, the snap, ledges
    ("band: inside, walking", lambda: solid_cast([GROUND]), [1, 1.5 * SKIN, 0], [1, 0, 0], 1, {}, ["ground:grounded"], G, N),
    ("band: beyond, walking", lambda: solid_cast([GROUND]), [1, 2.5 * SKIN, 0], [1, 0, 0], 1, {}, ["ground:snapped"], G | N, 0),
    ("band: inside, airborne", lambda: solid_cast([GROUND]), [1, 1.5 * SKIN, 0], [1, 0, 0], 0, {}, ["ground:grounded"], G, N),
    ("band: beyond, airborne", lambda: solid_cast([GROUND]), [1, 2.5 * SKIN, 0], [1, 0, 0], 0, {}, ["ground:none"], 0, G | N),
    ("ledge: below snap_distance", lambda: solid_cast([GROUND, box([-10, -1, -50], [0, 0.1, 50])]), [-0.5, 0.1 + Y0, 0], [1, 0, 0.2], 1, {},
     ["move:miss", "ground:snapped"], G | N, W),
    ("ledge: above snap_distance", lambda: solid_cast([GROUND, box([-10, -1, -50], [0, 0.5, 50])]), [-0.5, 0.5 + Y0, 0], [1, 0, 0.2], 1, {},
     ["move:miss", "ground:none"], 0, G | N),
    ("ramp: walking up 30 degrees", lambda: solid_cast([GROUND, slope(FLOOR_N)]), [1, Y0, 0], [2, 0, 0.3], 1, {}, ["move:plane", "ground:grounded"], G, W | S),
    ("ramp: walking down 30 degrees", lambda: solid_cast([GROUND, slope(FLOOR_N)]), [4, 2 * math.tan(math.radians(30)) + Y0 / FLOOR_N, 0], [-0.3, 0, 0.1], 1, {},
     ["move:miss", "ground:snapped"], G | N, W),
    ("on steep: standing on it", lambda: solid_cast([GROUND, slope(STEEP_N)]), [3, math.tan(math.radians(60)) + Y0 / STEEP_N, 0], [0, 0, 0.2], 1, {},
     ["ground:steep"], O, G | N),
    ("ceiling: a jump", lambda: solid_cast([GROUND, halfspace([0, -1, 0], -1.0)]), [1, Y0, 0], [0.5, 2, 0], 1, {}, ["move:plane"], C | W, G),
    ("zero motion", lambda: solid_cast([GROUND]), [1, Y0, 0], [0, 0, 0], 1, {}, ["move:", "ground:grounded"], G, N | W),
    ("zero reach", lambda: solid_cast([GROUND]), [1, Y0, 0], [1, 0, 0], 0, dict(skin=0.0), ["ground:no reach"], 0, G),
    # max_slides running out in either slide
    ("exhausted: move", lambda: solid_cast([GROUND, RISER_HIGH]), [1, Y0, 0], [2, 0, 1], 1, dict(max_slides=1), ["step:no progress"], E | W | G, S),
    ("exhausted: lifted slide", lambda: solid_cast([GROUND, RISER_LOW, box([3, -1, -50], [12, 0.9, 50])]), [1, Y0, 0], [3, 0, 1], 1, dict(max_slides=1),
     ["step:taken"], E | W | G | S, 0),
]


def _call_values(over):
    v = dict(skin=SKIN, max_slides=4, step_height=STEP, snap_distance=SNAP, min_floor_ny=NY)
    v.update(over)
    return tuple(float(F(v[k])) if k != "max_slides" else v[k] for k in ("skin", "max_slides", "step_height", "snap_distance", "min_floor_ny"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_probe_walk_matches_the_float64_rule(exe, case):
    name, make, pos, motion, grounded, over, branches, flags_set, flags_clear = case
    values = _call_values(over)
    pos32, motion32 = np.array([pos], F), np.array([motion], F)
    want = ref.walk(make(), pos32[0].astype(np.float64), motion32[0].astype(np.float64), grounded, *values)
    one = make()

    def cast32(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        hit = one(origins[0], dirs[0], float(max_t[0]))
        if hit is None:
            return np.array([MISS], np.uint32), np.array([np.inf], F), np.zeros((1, 3), F), np.zeros((1, 3), F)
        return np.array([hit[0]], np.uint32), np.array([hit[1]], F), np.array([hit[2]], F), np.zeros((1, 3), F)

    p, m, status, fbody, fnrm, _, body, _, _ = probe.host_loop(exe, cast32, pos32, motion32, 0.0, 0.0, None, [grounded], *values)
    print(name, want["branch"], hex(int(status[0])), hex(want["status"]), p[0], want["p"], m[0], want["m"])
    for b in branches:
        assert any(b in x for x in want["branch"]), (b, want["branch"])
    # the branch taken is the reference's: every flag and both hit counts, the hits themselves, and the floor
    assert int(status[0]) == want["status"], (hex(int(status[0])), hex(want["status"]))
    assert want["status"] & flags_set == flags_set and not want["status"] & flags_clear
    k = values[1]
    assert [int(b) for b in body[:k, 0] if b != MISS] == [h[0] for h in want["hits"]]
    assert [int(b) for b in body[k:, 0] if b != MISS] == [h[0] for h in want["lifted"]]
    if want["floor"] is None:
        assert fbody[0] == MISS and not fnrm[0].any()
    else:
        assert int(fbody[0]) == want["floor"][0] and np.abs(fnrm[0] - want["floor"][1]).max() <= 1e-6
    # positions to the tolerance tests/test_slide_cpu.py uses for whole loops
    assert np.abs(p[0] - want["p"]).max() <= 1e-5 and np.abs(m[0] - want["m"]).max() <= 1e-5
    assert m[0].any() == bool(want["m"].any())


def test_cast_budget_and_requests(exe):
    """the machine's own requests: unit vertical directions with the lengths the rule names, slots in their ranges, and never
    more than 2 max_slides + 3 casts"""
    seen = []

    def cast32(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        seen.append((origins[0].copy(), dirs[0].copy(), float(max_t[0])))
        hit = solid(origins[0], dirs[0], float(max_t[0]))
        if hit is None:
            return np.array([MISS], np.uint32), np.array([np.inf], F), np.zeros((1, 3), F), np.zeros((1, 3), F)
        return np.array([hit[0]], np.uint32), np.array([hit[1]], F), np.array([hit[2]], F), np.zeros((1, 3), F)

    solid = solid_cast([GROUND, RISER_LOW])
    out = probe.host_loop(exe, cast32, np.array([[1, Y0, 0]], F), np.array([[2, 0, 0.3]], F), 0.0, 0.0, None, [1], *_call_values({}))
    assert out[2][0] & ref.STEPPED
    kinds = [tuple(d) for _, d, _ in seen]
    assert (0.0, 1.0, 0.0) in kinds and (0.0, -1.0, 0.0) in kinds and len(seen) <= 2 * 4 + 3
    up = [mt for _, d, mt in seen if tuple(d) == (0.0, 1.0, 0.0)]
    assert up == [float(F(F(STEP) + F(SKIN)))]
    # the most casts: both slides use every cast (a script of oblique wall hits), then up, down and no ground cast after a step
    n1, n2 = [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]
    answers = [(1, 0.1, n1), (2, 0.1, n2)] + [None] + [(1, 0.3, n1), (2, 0.3, n2)] + [(0, 0.1, UPN)]
    left = list(answers)
    seen.clear()
    solid = lambda p, d, max_t: left.pop(0)
    out = probe.host_loop(exe, cast32, np.array([[1, Y0, 0]], F), np.array([[1, 0, 1]], F), 0.0, 0.0, None, [1], *_call_values(dict(max_slides=2)))
    assert len(seen) == 2 * 2 + 2 and not left and int(out[2][0]) & 0xFF == 0x22


BAD = [np.nan, np.inf, -np.inf]


def test_invalid_inputs(exe):
    base = dict(pos=[1.0, 2.0, 3.0], motion=[0.5, 0.0, -0.5], rot=[0.0, 0.0, 0.0, 1.0], R=0.25, h=0.5)
    rows = [("fine", dict(base), True), ("no rot", dict(base, rot=None), True), ("zero motion", dict(base, motion=[0, 0, 0]), True),
            ("R negative", dict(base, R=-0.1), False), ("h negative", dict(base, h=-0.1), False),
            ("motion too long", dict(base, motion=[2e38, 2e38, 2e38]), False)]
    for v in BAD:
        for key, at in (("pos", 1), ("motion", 2), ("rot", 3)):
            x = list(base[key]); x[at] = v
            rows.append((f"{key}[{at}] = {v}", dict(base, **{key: x}), False))
        rows += [(f"R = {v}", dict(base, R=v), False), (f"h = {v}", dict(base, h=v), False)]
    for name, q, want in rows:
        rot = None if q["rot"] is None else np.array([q["rot"]], F)
        with np.errstate(all="ignore"):
            got = probe.valid(exe, np.array([q["pos"]], F), np.array([q["motion"]], F), rot, np.array([q["R"]], F), np.array([q["h"]], F))[0]
            assert slide_ref.valid(np.array(q["pos"], F), np.array(q["motion"], F), None if rot is None else rot[0], F(q["R"]), F(q["h"])) == want, name
        assert got == want, name
    # an invalid query among valid ones: INVALID, nothing moves, no slot, no floor, and no cast is made for it
    asked = []

    def cast32(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        asked.append(ignore.copy())
        n = len(origins)
        return np.full(n, MISS, np.uint32), np.full(n, np.inf, F), np.zeros((n, 3), F), np.zeros((n, 3), F)

    pos, motion = np.array([[1, 2, 3], [np.nan, 0, 0], [4, 5, 6]], F), np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    with np.errstate(all="ignore"):
        p, m, status, fbody, _, _, body, _, _ = probe.host_loop(exe, cast32, pos, motion, 0.25, 0.5, None, [1, 1, 0], *_call_values({}),
                                                                ignore=np.arange(3, dtype=np.uint32))
    assert list(status) == [0, probe.INVALID, 0] and np.array_equal(p[1].view(np.uint32), pos[1].view(np.uint32)) and np.array_equal(m[1], motion[1])
    assert (body == MISS).all() and (fbody == MISS).all() and all(1 not in a for a in asked)
    assert np.array_equal(p[0], pos[0] + motion[0]) and np.array_equal(p[2], pos[2] + motion[2])


@pytest.mark.parametrize("name", cases.SCENES)
def test_near_ties_of_the_gpu_scenes_stay_under_half_the_cap(name):
    """The GPU property test may skip at most 2 % of the characters as near ties. That is a condition on the inputs: the
    float64 walk's own near ties (a cast whose two best candidates lie within 4 tol, a classified normal within 1e-4 of the
    slope limit, a progress comparison within tolerance) number at most half of that in every seeded scene."""
    c = cases.case(name)
    walks, tie = cases.reference(name)
    n = len(c["pos"])
    status = np.array([w["status"] for w in walks])
    count = lambda bit: int((status & bit != 0).sum())
    print(f"{c['label']}: {n} characters, near ties {int(tie.sum())}, cap {cases.tie_cap(n)}; grounded {count(G)}, stepped {count(S)}, "
          f"snapped {count(N)}, on steep {count(O)}, wall {count(W)}, ceiling {count(C)}, blocked {count(B)}")
    assert 2 * int(tie.sum()) <= cases.tie_cap(n)
    assert 0.3 < c["grounded"].mean() < 0.9
    if name == "terrain":
        # a phase nobody reaches is untested: the terrain reaches them all, and its characters start clear
        for bit in (G, S, N, O, W, C):
            assert count(bit) >= 3, hex(bit)
        assert count(B) == 0
        taken = [w["branch"] for w in walks]
        for what in ("noclimb", "step:taken", "step:not a floor", "ground:snapped", "ground:steep", "ground:none"):
            assert sum(1 for b in taken if any(what in x for x in b)) >= 3, what
    if name == "empty":
        assert not status.any()


def test_symbols_and_python_surface():
    import physics_amd
    from physics_amd import _abi
    from physics_amd.state import PhysicsState
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "physics_hip.h")).read()
    rust = open(os.path.join(root, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    spec = open(os.path.join(root, "include", "spec", "character.h")).read()
    lib = _abi.load_library()
    for name in ("phys_character_move", "phys_character_move_device"):
        assert f"{name}(" in header and f"fn {name}(" in rust and hasattr(lib, name)
    assert re.search(r"#define PHYS_ABI_VERSION 2u?\b", header)
    for macro, value in (("GROUNDED", 0x1000), ("STEPPED", 0x2000), ("SNAPPED", 0x4000), ("ON_STEEP", 0x8000), ("HIT_WALL", 0x10000),
                         ("HIT_CEILING", 0x20000)):
        assert int(re.search(rf"#define PHYS_CHAR_{macro} (\w+?)u\b", header).group(1), 0) == value == getattr(_abi, "CHAR_" + macro)
        assert int(re.search(rf"#define CH_{macro} (\w+?)u\b", spec).group(1), 0) == value == getattr(probe, macro) == getattr(ref, macro)
        assert int(re.search(rf"pub const PHYS_CHAR_{macro}: u32 = (\w+);", rust).group(1), 0) == value
        assert getattr(physics_amd, "CHAR_" + macro) == value
    for macro, value in (("BLOCKED", 0x100), ("EXHAUSTED", 0x200), ("INVALID", 0x400)):
        assert int(re.search(rf"#define PHYS_CHAR_{macro} (\w+?)u\b", header).group(1), 0) == value == getattr(_abi, "CHAR_" + macro)
    # the header includes vec.h and slide.h alone
    assert re.findall(r'#include [<"]([^>"]+)[>"]', spec) == ["vec.h", "slide.h"]
    for cls in (physics_amd.World, PhysicsState):
        assert callable(getattr(cls, "character_move", None))
    assert callable(getattr(physics_amd.World, "character_move_device", None))
    E = _abi.PHYS_ERR_INVALID_ARG
    a = np.zeros(3, F)
    st = np.zeros(1, np.uint32)
    p = lambda x, t=_abi.f32p: x.ctypes.data_as(t)
    assert lib.phys_character_move(None, 1, p(a), p(a), None, p(a), p(a), None, 0.02, 4, 0.3, 0.2, 0.7, None, None, p(a), None, p(st, _abi.u32p),
                                   None, None, None, None, None, None) == E
    assert lib.phys_character_move_device(None, 1, *[None] * 6, 0.02, 4, 0.3, 0.2, 0.7, *[None] * 11) == E


def test_argument_errors_raise_before_the_library_is_called():
    import physics_amd

    class Dead:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    w = object.__new__(physics_amd.World)
    w.lib, w.h, w.n = Dead(), None, 0
    two, ones = np.zeros((2, 3)), np.ones((2, 3))
    bad = (math.nan, math.inf, -0.1)
    cases_ = [dict(motion=np.zeros((3, 3))), dict(radius=[0.5, 0.5, 0.5]), dict(half_length=[1.0, 1.0, 1.0]), dict(rot=np.zeros((3, 4))),
              dict(ignore=[1, 2, 3]), dict(grounded=[1, 0, 1]), dict(mask=[1, 2, 3]), dict(mask=0x10000), dict(max_slides=0), dict(max_slides=9),
              dict(min_floor_ny=0.0), dict(min_floor_ny=1.01), dict(min_floor_ny=math.nan), dict(min_floor_ny=-0.5)]
    cases_ += [{k: v} for k in ("skin", "step_height", "snap_distance") for v in bad]
    for kw in cases_:
        args = dict(pos=two, motion=ones, radius=0.5, half_length=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            w.character_move(**args)
