"""CPU: move-and-slide's rule. The spec header alone (include/spec/slide.h through tests/cpp/slide_probe.cpp, built once plain
and once under the address and undefined-behaviour sanitizers) against the float64 statement of tests/slide_ref.py, case by
case; the reference cast's own count of near ties over every seeded scene of tests/test_gpu_slide.py; the declared symbols and
the Python surface's argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_cases as cases
import slide_probe as probe
import slide_ref as ref
from capsulecast_accept import near_ties
from query_accept import cast_cap

F = np.float32
MISS = probe.MISS


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("slide") / "slide_probe"), sanitize=request.param == "sanitized")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _wall(deg):
    """the unit normal of a vertical wall that meets the wall of normal (-1, 0, 0) at an inner angle of 180 - deg degrees"""
    a = np.radians(deg)
    return np.array([-np.cos(a), 0.0, -np.sin(a)])


WALL = [-1.0, 0.0, 0.0]
# one step each: (name, m, m0 (None: m), n_prev (None: no previous hit), t, n, skin, the branch the reference must take).
# Inputs lie away from the thresholds: dots of order 0.1 or more where a sign decides (or a sign that is exact in both
# precisions), |c|^2 of order 1 or far below 1e-12.
STEPS = [
    ("plane slide", [1.0, 0.0, 0.5], None, None, 0.7, [-1.0, 0.0, 0.0], 0.02, "plane"),
    ("plane slide, oblique normal", [0.8, -0.3, 0.5], None, None, 0.4, _unit([-1.0, 0.5, 0.2]), 0.02, "plane"),
    # a crease: the slide along the second wall points back into the first (n_prev). Walls meeting at 60, 90 and 120 degrees.
    ("acute crease", [0.3, 0.4, 0.9], [1.0, 0.4, 0.3], WALL, 0.2, _wall(120), 0.02, "crease"),
    ("right crease", [0.2, 0.3, 0.9], [1.0, 0.3, 0.9], WALL, 0.3, _wall(90), 0.02, "crease"),
    ("obtuse crease", [0.8, 0.3, 0.5], [1.0, 0.3, 0.5], WALL, 0.25, _wall(60), 0.02, "crease"),
    ("crease that turns back", [0.3, -0.4, 0.9], [1.0, 0.4, 0.3], WALL, 0.2, _wall(120), 0.02, "crease+turnback"),
    # parallel normals: |n_prev x n|^2 = 2.5e-13; the slide's sign against n_prev is the sign of m.z, exactly
    ("parallel normals", [0.5, 0.0, -0.5], [1.0, 0.0, -1.0], [1.0, 0.0, 5e-7], 0.2, [-1.0, 0.0, 0.0], 0.02, "parallel+turnback"),
    ("turn-back stop", [-0.2, 0.0, 1.0], [-1.0, 0.0, 0.5], None, 0.3, _unit([0.3, 0.0, -1.0]), 0.02, "plane+turnback"),
    ("previous plane, no crease", [0.0, 0.0, 1.0], [0.2, 0.0, 1.0], WALL, 0.5, _unit([-0.5, 0.0, -1.0]), 0.02, "plane"),
    ("t below skin", [1.0, 0.0, 0.5], None, None, 0.005, [-1.0, 0.0, 0.0], 0.02, "plane"),
    ("t beyond L", [0.3, 0.0, 0.1], None, None, 0.33, [-1.0, 0.0, 0.0], 0.02, "plane"),
    ("skin zero", [1.0, 0.2, 0.5], None, None, 0.6, [-1.0, 0.0, 0.0], 0.0, "plane"),
    ("starts touching", [1.0, 0.0, 0.5], None, None, 0.0, _unit([-1.0, 0.0, -0.5]), 0.02, "blocked"),
]


def _state(m, m0, n_prev, p=(3.0, 1.5, -2.0), status=0):
    one = lambda v: np.asarray(v, F).reshape(1, 3)
    return dict(p=one(p), m=one(m), m0=one(m if m0 is None else m0), n_prev=one([0, 0, 0] if n_prev is None else n_prev),
                have_prev=np.array([0 if n_prev is None else 1], np.uint32), status=np.array([status], np.uint32))


def _ref_state(s):
    """the float64 reference's state from the float32 operands the probe was given"""
    d = lambda k: s[k][0].astype(np.float64)
    return dict(p=d("p"), m=d("m"), m0=d("m0"), n_prev=d("n_prev") if s["have_prev"][0] else None, status=int(s["status"][0]))


@pytest.mark.parametrize("step", STEPS, ids=[s[0] for s in STEPS])
def test_probe_step_matches_the_float64_rule(exe, step):
    name, m, m0, n_prev, t, n, skin, branch = step
    s = _state(m, m0, n_prev, status=1 if n_prev is not None else 0)
    n32, t32, skin32 = np.asarray(n, F).reshape(1, 3), np.array([t], F), F(skin)
    got, go = probe.after_cast(exe, s, skin32, np.array([7], np.uint32), t32, n32)
    want, want_go, took = ref.step(_ref_state(s), float(skin32), (7, float(t32[0]), n32[0].astype(np.float64)))
    print(name, took, got["p"][0], got["m"][0], want["p"], want["m"])
    assert took == branch
    assert bool(go[0]) == want_go and int(got["status"][0]) == want["status"]
    # float32 rounding of operands of order 1 through a dozen operations (2^-24 each, relative): 4e-6 absolute at these sizes
    scale = 1.0 + np.abs(s["p"]).max() + np.abs(s["m"]).max()
    assert np.abs(got["p"][0] - want["p"]).max() <= 4e-6 * scale
    assert np.abs(got["m"][0] - want["m"]).max() <= 4e-6 * scale
    # branch decisions are equal: a stopped slide is exactly zero on both sides, a slide that goes on is not
    assert got["m"][0].any() == bool(want["m"].any())
    if took != "blocked":
        assert np.array_equal(got["n_prev"][0], n32[0]) and got["have_prev"][0] == 1
        assert np.array_equal(got["m0"], s["m0"])
    else:
        assert np.array_equal(got["p"], s["p"]) and np.array_equal(got["m"], s["m"])


def test_miss_zero_motion_and_running_out(exe):
    s = _state([1.0, 0.25, -0.5], None, None)
    got, go = probe.after_cast(exe, s, F(0.02), np.array([MISS], np.uint32), np.array([np.inf], F), np.zeros((1, 3), F))
    want, _, took = ref.step(_ref_state(s), 0.02, None)
    assert took == "miss" and not go[0] and got["status"][0] == 0
    assert np.array_equal(got["p"][0], (s["p"] + s["m"])[0]) and not got["m"].any() and np.allclose(got["p"][0], want["p"])
    # a zero motion: there is no cast, and nothing is left when the casts run out
    z = probe.begin(exe, np.array([[1, 2, 3]], F), np.zeros((1, 3), F))
    L, max_t, go = probe.before_cast(exe, z, F(0.02))
    assert L[0] == 0 and not go[0] and z["status"][0] == 0 and np.array_equal(z["p"][0], [1, 2, 3])
    assert probe.ran_out(exe, z)["status"][0] == 0
    # motion left when the casts run out: EXHAUSTED, and only then
    left = _state([0.0, 0.0, 0.3], [1, 0, 1], [-1, 0, 0], status=2)
    assert probe.ran_out(exe, left)["status"][0] == 2 | probe.EXHAUSTED
    # before a cast: L by the cast's own expression in float32, max_t = L + skin
    s = _state([0.3, -0.4, 1.2], None, None)
    L, max_t, go = probe.before_cast(exe, s, F(0.02))
    m = s["m"][0]
    assert L[0] == np.sqrt(F(F(m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])) and max_t[0] == F(L[0] + F(0.02)) and go[0]
    assert abs(float(L[0]) - np.linalg.norm(m.astype(np.float64))) <= 2e-7 * float(L[0])


BAD = [np.nan, np.inf, -np.inf]


def _invalid_inputs():
    base = dict(pos=[1.0, 2.0, 3.0], motion=[0.5, 0.0, -0.5], rot=[0.0, 0.0, 0.0, 1.0], R=0.25, h=0.5)
    out = [("fine", dict(base), True), ("no rot", dict(base, rot=None), True), ("zero motion", dict(base, motion=[0, 0, 0]), True),
           ("R and h zero", dict(base, R=0.0, h=0.0), True), ("long but finite", dict(base, motion=[1e19, 0, 0]), True),
           ("R negative", dict(base, R=-0.1), False), ("h negative", dict(base, h=-0.1), False),
           ("motion too long", dict(base, motion=[2e38, 2e38, 2e38]), False),
           ("motion squares overflow", dict(base, motion=[1e20, 0, 0]), False)]
    for v in BAD:
        for key, at in (("pos", 1), ("motion", 2), ("rot", 0), ("rot", 3)):
            x = list(base[key])
            x[at] = v
            out.append((f"{key}[{at}] = {v}", dict(base, **{key: x}), False))
        out.append((f"R = {v}", dict(base, R=v), False))
        out.append((f"h = {v}", dict(base, h=v), False))
    return out


def test_every_invalid_input(exe):
    rows = _invalid_inputs()
    for name, q, want in rows:
        rot = None if q["rot"] is None else np.array([q["rot"]], F)
        with np.errstate(all="ignore"):
            got = probe.valid(exe, np.array([q["pos"]], F), np.array([q["motion"]], F), rot, np.array([q["R"]], F), np.array([q["h"]], F))[0]
            assert ref.valid(np.array(q["pos"], F), np.array(q["motion"], F), None if rot is None else rot[0], F(q["R"]), F(q["h"])) == want, name
        assert got == want, name
    assert sum(1 for r in rows if not r[2]) >= 22


def test_whole_loops_against_the_float64_rule(exe):
    """the loop itself, over casts against two analytic walls (x = 2 facing -x, z = 2 facing -z) for a point character: the
    probe's loop and the float64 loop take the same hits and end within rounding of each other"""
    def wall_cast(p, m, max_t):
        p, m = np.asarray(p, np.float64), np.asarray(m, np.float64)
        u = m / np.linalg.norm(m)
        best = None
        for ax, n in ((0, [-1.0, 0, 0]), (2, [0, 0, -1.0])):
            if p[ax] >= 2.0:
                return (ax, 0.0, -u)
            if u[ax] > 0:
                t = (2.0 - p[ax]) / u[ax]
                if t <= max_t and (best is None or t < best[1]):
                    best = (ax, t, np.array(n))
        return best

    def cast32(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        n = len(origins)
        b, t, nn = np.full(n, MISS, np.uint32), np.full(n, np.inf, F), np.zeros((n, 3), F)
        for i in range(n):
            hit = wall_cast(origins[i], dirs[i], float(max_t[i]))
            if hit is not None:
                b[i], t[i], nn[i] = hit[0], F(hit[1]), hit[2]
        return b, t, nn, np.zeros((n, 3), F)

    rng = np.random.default_rng(5)
    n = 40
    pos = rng.uniform(0.0, 1.5, (n, 3)).astype(F)
    motion = rng.uniform(-1.0, 4.0, (n, 3)).astype(F)
    seen = {}
    for max_slides in (1, 2, 4):
        p, m, status, body, _, _ = probe.host_loop(exe, cast32, pos, motion, 0.0, 0.0, None, F(0.02), max_slides)
        kinds = set()
        for i in range(n):
            rp, rm, rstatus, hits = ref.slide(wall_cast, pos[i], motion[i], float(F(0.02)), max_slides)
            assert status[i] == rstatus, (i, hex(status[i]), hex(rstatus))
            assert [int(b) for b in body[:, i] if b != MISS] == [h[0] for h in hits]
            assert np.abs(p[i] - rp).max() <= 1e-5 and np.abs(m[i] - rm).max() <= 1e-5
            kinds.add(int(status[i]))
        seen[max_slides] = kinds
        print(max_slides, sorted(hex(k) for k in kinds))
    # one cast leaves slides unspent, two leave the run up the corner; four finish everything (a free third cast)
    assert 1 | probe.EXHAUSTED in seen[1] and 2 | probe.EXHAUSTED in seen[2] and not any(k & probe.EXHAUSTED for k in seen[4])
    assert {0, 1, 2} <= seen[4]


@pytest.mark.parametrize("name", cases.SCENES)
def test_near_ties_of_the_gpu_scenes_stay_under_half_the_cap(name):
    """The cap on other ids is a condition on the inputs: the reference's own near ties (t2 - t <= 4 tol) along the requested
    motion number at most half of it in every seeded scene the GPU tests use. The starts are clear of everything."""
    c = cases.case(name)
    n, ties = len(c["pos"]), near_ties(c["h"])
    print(f"{c['label']}: {n} characters, near ties {ties}, cap {cast_cap(n)}")
    assert 2 * ties <= cast_cap(n)
    sep = cases.separation(c["pos"], c["rot"], c["rad"], c["hq"], c["tg"], c["ground"])
    assert (sep >= c["skin"]).all() and (c["hq"] == 0).sum() >= n // 20 and (c["rad"] == 0).sum() >= n // 20
    L = np.linalg.norm(c["motion"].astype(np.float64), axis=1)
    if name != "empty":
        assert (c["h"]["t"] < L).sum() > (n // 2 if name == "soup" else n // 20)
    else:
        assert (c["h"]["body"] == MISS).all()


def test_symbols_and_python_surface():
    import physics_amd
    from physics_amd import _abi
    from physics_amd.state import PhysicsState
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "physics_hip.h")).read()
    rust = open(os.path.join(root, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    spec = open(os.path.join(root, "include", "spec", "slide.h")).read()
    lib = _abi.load_library()
    for name in ("phys_move_and_slide", "phys_move_and_slide_device"):
        assert f"{name}(" in header and f"fn {name}(" in rust and hasattr(lib, name)
    assert re.search(r"#define PHYS_ABI_VERSION 2u?\b", header)
    for macro, value in (("SLIDE_MAX_SLIDES", 8), ("SLIDE_BLOCKED", 0x100), ("SLIDE_EXHAUSTED", 0x200), ("SLIDE_INVALID", 0x400)):
        assert int(re.search(rf"#define PHYS_{macro} (\w+?)u\b", header).group(1), 0) == value == getattr(_abi, macro)
        assert int(re.search(rf"#define SL_{macro[6:]} (\w+?)u\b", spec).group(1), 0) == value
        assert getattr(physics_amd, macro) == value
    assert (probe.BLOCKED, probe.EXHAUSTED, probe.INVALID, probe.MISS) == (0x100, 0x200, 0x400, physics_amd.RAY_MISS)
    for cls in (physics_amd.World, PhysicsState):
        assert callable(getattr(cls, "move_and_slide", None))
    assert callable(getattr(physics_amd.World, "move_and_slide_device", None))
    E = _abi.PHYS_ERR_INVALID_ARG
    a = np.zeros(3, F)
    st = np.zeros(1, np.uint32)
    p = lambda x, t=_abi.f32p: x.ctypes.data_as(t)
    assert lib.phys_move_and_slide(None, 1, p(a), p(a), None, p(a), p(a), 0.02, 4, None, None, p(a), None, p(st, _abi.u32p),
                                   None, None, None) == E
    assert lib.phys_move_and_slide_device(None, 1, None, None, None, None, None, 0.02, 4, None, None, None, None, None, None, None, None) == E


def test_argument_errors_raise_before_the_library_is_called():
    import physics_amd

    class Dead:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    w = object.__new__(physics_amd.World)
    w.lib, w.h, w.n = Dead(), None, 0
    two, ones = np.zeros((2, 3)), np.ones((2, 3))
    for kw in (dict(motion=np.zeros((3, 3))), dict(radius=[0.5, 0.5, 0.5]), dict(half_length=[1.0, 1.0, 1.0]), dict(rot=np.zeros((3, 4))),
               dict(ignore=[1, 2, 3]), dict(mask=[1, 2, 3]), dict(mask=0x10000), dict(max_slides=0), dict(max_slides=9), dict(skin=-0.1),
               dict(skin=float("nan")), dict(skin=float("inf"))):
        args = dict(pos=two, motion=ones, radius=0.5, half_length=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            w.move_and_slide(**args)
