"""CPU: the float64 reference of the capsule cast (tests/capsulecast_ref.py) on closed forms and against nested golden
sections; the reference's own count of near ties over every seeded input of tests/test_gpu_capsulecast.py; the Python
surface's argument errors and the declared symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import capsulecast_accept as acc
import capsulecast_cases as cases
import capsulecast_ref as ref
import query_ref
from query_accept import cast_cap
from raycast_ref import MISS


def test_reference_on_closed_forms():
    bodies, casts = cases.hand_scene()
    tg = query_ref.targets(bodies)
    rot = [cases.axis_quat(c["axis"]) for c in casts]
    h = ref.capsulecast([c["o"] for c in casts], [c["d"] for c in casts], rot, [c["rad"] for c in casts],
                        [c["hq"] for c in casts], tg, ground=0.0)
    for i, c in enumerate(casts):
        assert h["body"][i] == c["body"], (c["name"], h["body"][i])
        assert abs(h["t"][i] - c["t"]) < 1e-9, (c["name"], h["t"][i])
        assert np.allclose(h["normal"][i], c["normal"], atol=1e-7), (c["name"], h["normal"][i])
        for a in range(3):
            if c["point"][a] is not None:
                assert abs(h["point"][i][a] - c["point"][a]) < 1e-7, (c["name"], h["point"][i])
        if c["name"] in cases.FREE_RANGE:  # the free component of a line contact lies on the line
            a, lo, hi = cases.FREE_RANGE[c["name"]]
            assert lo - 1e-9 <= h["point"][i][a] <= hi + 1e-9, (c["name"], h["point"][i])


def test_reference_rules():
    bodies, casts = cases.hand_scene()
    tg = query_ref.targets(bodies)
    o, d = [casts[0]["o"]] * 9, [casts[0]["d"]] * 8 + [[0, 0, 0]]
    rot = np.tile(np.array(cases.IDENT), (9, 1))
    rot[6] = np.nan
    rad = [-1, np.nan, np.inf, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    hq = [1, 1, 1, -1, np.nan, np.inf, 1, 1, 1]
    h = ref.capsulecast(o, d, rot, rad, hq, tg, max_t=[9] * 7 + [-1, 9], ground=0.0)
    assert (h["body"] == MISS).all() and np.isinf(h["t"]).all() and not h["normal"].any() and not h["point"].any()
    # max_t, ignore, and the second-best t
    h = ref.capsulecast([[-5, 5.2, 0.3]] * 4, [[1, 0, 0]] * 4, None, 0.5, 1.0, tg, max_t=[3.4, 3.6, 100, 100], ignore=[7, 7, 0, 7],
                        ground=0.0)
    assert list(h["body"]) == [MISS, 0, 1, 0] and abs(h["t"][2] - (15 - 0.5 - 0.5)) < 1e-9
    assert np.isinf(h["t2"][1]) and abs(h["t2"][3] - 14.0) < 1e-9
    # half-length 0 is query_ref's sphere cast
    c = cases.soup(1)
    k = slice(0, 80)
    a = ref.capsulecast(c["o"][k], c["d"][k], c["rot"][k], c["rad"][k], 0.0, c["tg"], ground=0.0)
    b = query_ref.spherecast(c["o"][k], c["d"][k], c["rad"][k], c["tg"], ground=0.0)
    assert np.array_equal(a["body"], b["body"]) and np.allclose(a["t"], b["t"], rtol=0, atol=1e-9)


def test_distances_against_nested_golden_sections():
    rng = np.random.default_rng(9)
    n = 60
    c1, c2 = rng.uniform(-2, 2, (n, 3)), rng.uniform(-2, 2, (n, 3))
    u1, u2 = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (rng.normal(size=(n, 3)), rng.normal(size=(n, 3))))
    u2[:6] = u1[:6]  # parallel ones
    h1, h2 = rng.uniform(0.1, 1.5, n), rng.uniform(0.1, 1.5, n)
    q, p, d = ref.seg_seg_closest(c1, u1, h1, c2, u2, h2)
    he = rng.uniform(0.2, 1.2, (n, 3))
    qb, pb, db = ref.seg_box_closest(c1 * 1.5, u1, h1, he)
    for i in range(n):
        assert abs(d[i] - query_ref._seg_seg(c1[i], u1[i], h1[i], c2[i], u2[i], h2[i])) < 1e-7
        assert abs(np.linalg.norm(q[i] - p[i]) - d[i]) < 1e-12
        assert abs(db[i] - query_ref._seg_box(c1[i] * 1.5, u1[i], h1[i], np.zeros(3), np.eye(3), he[i])) < 1e-7
        assert abs(np.linalg.norm(qb[i] - pb[i]) - db[i]) < 1e-12 and (np.abs(pb[i]) <= he[i] + 1e-12).all()


def _all_labels():
    return [f"soup{s}" for s in cases.SOUP_SEEDS] + list(cases.DEGENERATE) + \
        [f"{n}:{k}" for n in cases.GRID_SCENES for k in ("mixed", "huge")] + ["rules", "filters"]


def _cases_of(label):
    if label.startswith("soup"):
        return [cases.soup(int(label[4:]))]
    if label in cases.DEGENERATE:
        return [cases.degenerate(label)]
    if label == "rules":
        return [cases.rules_case()]
    if label == "filters":
        return [c for _, c in cases.filter_case()[3].values()]
    return [cases.grid_case(*label.split(":"))]


@pytest.mark.parametrize("label", _all_labels())
def test_near_ties_of_the_gpu_inputs_stay_under_half_the_cap(label):
    """The cap on other ids is a condition, not a measurement: the reference's own near ties (t2 - t <= 4 tol) number at
    most half of it in every seeded input the GPU tests use."""
    for c in _cases_of(label):
        n, ties = len(c["o"]), acc.near_ties(c["h"])
        print(f"{c['label']}: {n} casts, near ties {ties}, cap {cast_cap(n)}")
        assert 2 * ties <= cast_cap(n), (c["label"], ties)


def test_the_gpu_inputs_reach_every_kind_of_target():
    for seed in cases.SOUP_SEEDS:
        c = cases.soup(seed)
        body = c["h"]["body"]
        assert (body < len(c["bodies"]["pos"])).sum() > 200 and ((body & 0x80000000 != 0) & (body < MISS)).sum() > 0
        assert (body == 0xFFFFFFFF).sum() > 0 and (c["hq"] == 0).sum() > 20 and (c["rad"] == 0).sum() > 20
        shapes = c["tg"]["shape"][c["h"]["which"][c["h"]["which"] >= 0]]
        assert all((shapes == s).sum() > 30 for s in (1, 2, 3))


def test_symbols_and_python_surface():
    import physics_amd
    from physics_amd import _abi
    names = {"phys_capsulecast", "phys_capsulecast_device", "phys_capsulecast_filtered", "phys_capsulecast_device_filtered"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "physics_hip.h")).read()
    rust = open(os.path.join(root, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    lib = _abi.load_library()
    for name in names:
        assert f"{name}(" in header and f"fn {name}(" in rust and hasattr(lib, name)
    assert re.search(r"#define PHYS_ABI_VERSION 2u?\b", header)
    from physics_amd.state import PhysicsState
    for cls in (physics_amd.World, PhysicsState):
        assert callable(getattr(cls, "capsulecast", None))
    assert callable(getattr(physics_amd.World, "capsulecast_device", None))
    E = _abi.PHYS_ERR_INVALID_ARG
    f32 = C.POINTER(C.c_float)
    o = np.zeros(3, np.float32)
    body = np.zeros(1, np.uint32)
    p = lambda a, t=f32: a.ctypes.data_as(t)
    assert lib.phys_capsulecast(None, 1, p(o), p(o), None, p(o), p(o), None, None, p(body, C.POINTER(C.c_uint32)), p(o), p(o), p(o)) == E
    assert lib.phys_capsulecast_device(None, 1, None, None, None, None, None, None, None, None, None, None, None) == E
    assert lib.phys_capsulecast_filtered(None, 1, p(o), p(o), None, p(o), p(o), None, None, None, p(body, C.POINTER(C.c_uint32)),
                                         p(o), p(o), p(o)) == E
    assert lib.phys_capsulecast_device_filtered(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == E


def test_argument_errors_raise_before_the_library_is_called():
    import physics_amd

    class Dead:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    w = object.__new__(physics_amd.World)
    w.lib, w.h, w.n = Dead(), None, 0
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.zeros((3, 3)), 0.5, 1.0)
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), [0.5, 0.5, 0.5], 1.0)
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, 1.0, rot=np.zeros((3, 4)))
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, 1.0, max_t=[1.0])
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, 1.0, ignore=[1, 2, 3])
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, 1.0, mask=[1, 2, 3])
    with pytest.raises(ValueError):
        w.capsulecast(np.zeros((2, 3)), np.ones((2, 3)), 0.5, 1.0, mask=0x10000)
