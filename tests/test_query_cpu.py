"""CPU: the float64 brute force of the sphere-cast and overlap queries (tests/query_ref.py) on closed-form cases, and the
queries' surface - header declarations, exported symbols, the Python methods and the argument errors that need no
device. No GPU needed."""
import math
import os
import re

import numpy as np
import pytest

import physics_amd
from physics_amd import _abi

import query_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "physics_hip.h")


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([a * math.sin(angle / 2), [math.cos(angle / 2)]])


def _tg(pos, shape, he, rot=None):
    return ref.targets(dict(pos=pos, rot=rot, half_extent=he, shape=shape))


def _cast(o, d, r, tg, **kw):
    h = ref.spherecast([o], [d], [r], tg, **kw)
    return int(h["body"][0]), float(h["t"][0]), h["normal"][0]


UNIT_BOX = dict(pos=[[0, 0, 0]], shape=[ref.SHAPE_BOX], he=[[1, 1, 1]])


def test_spherecast_box_face():
    body, t, n = _cast([-5, 0.2, 0.3], [2, 0, 0], 0.5, _tg(**UNIT_BOX))
    assert body == 0 and abs(t - 3.5) < 1e-9 and np.allclose(n, [-1, 0, 0], atol=1e-7)


def test_spherecast_box_edge_cylinder_part():
    body, t, n = _cast([-5, 1.3, 0], [1, 0, 0], 0.5, _tg(**UNIT_BOX))
    assert body == 0 and abs(t - 3.6) < 1e-9 and np.allclose(n, [-0.8, 0.6, 0], atol=1e-7)


def test_spherecast_box_corner_ball_part():
    body, t, n = _cast([-5, 1.3, 1.2], [1, 0, 0], 0.5, _tg(**UNIT_BOX))
    s = math.sqrt(0.12)
    assert body == 0 and abs(t - (4 - s)) < 1e-9
    assert np.allclose(n, np.array([-s, 0.3, 0.2]) / 0.5, atol=1e-7)


def test_spherecast_turned_box_face():
    tg = _tg([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 1, 1]], rot=[_rot([0, 1, 0], math.pi / 4)])
    body, t, n = _cast([-5, 0, 0], [1, 0, 0], 0.25, tg)  # onto the (-x) edge of the diamond: the cylinder part
    assert body == 0 and abs(t - (5 - math.sqrt(2) - 0.25)) < 1e-9 and np.allclose(n, [-1, 0, 0], atol=1e-7)


def test_spherecast_capsule_side_and_end():
    tg = _tg([[0, 0, 0]], [ref.SHAPE_CAPSULE], [[0.5, 1, 0]])
    body, t, n = _cast([-5, 0.5, 0], [1, 0, 0], 0.25, tg)
    assert body == 0 and abs(t - 4.25) < 1e-9 and np.allclose(n, [-1, 0, 0], atol=1e-7)
    body, t, n = _cast([0.3, 5, 0], [0, -1, 0], 0.25, tg)
    h = math.sqrt(0.75 ** 2 - 0.3 ** 2)
    assert body == 0 and abs(t - (4 - h)) < 1e-9 and np.allclose(n, [0.3 / 0.75, h / 0.75, 0], atol=1e-7)


def test_spherecast_ground_and_initial_overlap():
    tg = ref.targets()
    body, t, n = _cast([0, 3, 0], [0, -2, 0], 0.5, tg, ground=0.0)
    assert body == ref.GROUND and t == 2.5 and np.allclose(n, [0, 1, 0])
    body, t, n = _cast([0, 0.4, 0], [1, 0, 0], 0.5, tg, ground=0.0)  # the ball already touches the ground
    assert body == ref.GROUND and t == 0.0 and np.allclose(n, [-1, 0, 0])
    body, t, n = _cast([0.5, 1.2, 0], [0, 0, 3], 0.5, _tg(**UNIT_BOX))  # overlaps the box: t = 0, normal -dir
    assert body == 0 and t == 0.0 and np.allclose(n, [0, 0, -1])


def test_spherecast_rules():
    tg = _tg([[0, 0, 0], [5, 0, 0]], [ref.SHAPE_BOX, ref.SHAPE_SPHERE], [[1, 1, 1], [1, 0, 0]])
    assert _cast([-5, 0, 0], [1, 0, 0], 0.5, tg, ignore=[0])[:2] == (1, 8.5)
    assert _cast([-5, 0, 0], [1, 0, 0], 0.5, tg, max_t=[3.4])[0] == ref.MISS
    assert _cast([-5, 0, 0], [1, 0, 0], 0.5, tg, max_t=[3.5])[:2] == (0, 3.5)
    for r in (-1.0, math.nan, math.inf):
        body, t, n = _cast([-5, 0, 0], [1, 0, 0], r, tg, ground=0.0)
        assert body == ref.MISS and t == math.inf and not n.any()
    # radius 0 is the ray cast
    import raycast_ref
    o, d = [[-5, 0.3, 0.2], [0.2, 9, 0.1]], [[1, 0.01, 0], [0, -1, 0.02]]
    a = ref.spherecast(o, d, 0.0, tg)
    b = raycast_ref.cast(o, d, dict(pos=tg["pos"], rot=tg["rot"], half_extent=tg["half_extent"], shape=tg["shape"]))
    assert list(a["body"]) == list(b["body"]) and np.allclose(a["t"], b["t"], atol=1e-9)


def _ov(shape, pos, he, tg, rot=None, ground=None):
    return ref.overlap([shape], [pos], None if rot is None else [rot], [he], tg, ground=ground)[0][0]


def test_overlap_edge_edge_sat():
    # A turned 45 degrees about z (top edge along z at y = sqrt 2), B about x (bottom edge along x): only the cross axis
    # of the two edges, y, separates them
    tg = _tg([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 1, 1]], rot=[_rot([0, 0, 1], math.pi / 4)])
    rb = _rot([1, 0, 0], math.pi / 4)
    c = 2 * math.sqrt(2)
    assert _ov(ref.SHAPE_BOX, [0, c - 1e-3, 0], [1, 1, 1], tg, rot=rb) == [0]
    assert _ov(ref.SHAPE_BOX, [0, c + 1e-3, 0], [1, 1, 1], tg, rot=rb) == []
    Ra = ref.rotation_matrices([_rot([0, 0, 1], math.pi / 4)])[0]
    Rb = ref.rotation_matrices([rb])[0]
    gap = ref._box_gap(np.zeros(3), Ra, np.ones(3), np.array([0, c + 1e-3, 0]), Rb, np.ones(3))
    assert abs(gap - 1e-3) < 1e-9


def test_overlap_capsule_by_a_box_edge():
    tg = _tg(**UNIT_BOX)
    along_z = _rot([1, 0, 0], math.pi / 2)  # the core (local y) along z
    for d, want in ((0.5 - 1e-3, [0]), (0.5 + 1e-3, [])):
        c = 1 + d / math.sqrt(2)
        assert _ov(ref.SHAPE_CAPSULE, [c, c, 0], [0.5, 2, 0], tg, rot=along_z) == want
    # a core skew to the edge, along (1, -1, 1) / sqrt 3: their common perpendicular is (1, 1, 0), length d
    tilted = _rot([1, 0, -1], math.acos(-1 / math.sqrt(3)))
    for d, want in ((0.5 - 1e-3, [0]), (0.5 + 1e-3, [])):
        c = 1 + d / math.sqrt(2)
        assert _ov(ref.SHAPE_CAPSULE, [c, c, 0.3], [0.5, 2, 0], tg, rot=tilted) == want


def test_overlap_shapes_ground_statics_and_order():
    bodies = dict(pos=[[0, 0, 0], [3, 0, 0]], shape=[ref.SHAPE_SPHERE, ref.SHAPE_CAPSULE], half_extent=[[1, 0, 0], [0.5, 1, 0]])
    statics = dict(pos=[[0, -1, 0]], shape=[ref.SHAPE_BOX], half_extent=[[10, 0.5, 10]])
    tg = ref.targets(bodies, statics)
    got = _ov(ref.SHAPE_SPHERE, [1.5, 0, 0], [1, 0, 0], tg, ground=-1.5)
    assert got == [0, 1, ref.STATIC_ID_BIT]
    got = _ov(ref.SHAPE_SPHERE, [1.5, 0, 0], [2, 0, 0], tg, ground=-1.5)
    assert got == [0, 1, ref.STATIC_ID_BIT, ref.GROUND]
    assert ref.overlap([7], [[0, 0, 0]], None, [[1, 1, 1]], tg)[0][0] == []  # not a shape: empty
    assert ref.overlap([ref.SHAPE_BOX], [[0, 0, 0]], None, [[1, -1, 1]], tg)[0][0] == []  # negative extent: empty


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(phys_[a-z0-9_]+)\s*\(", text))


def test_queries_declared_and_exported():
    names = {"phys_spherecast", "phys_spherecast_device", "phys_overlap"}
    assert names <= _declared()
    lib = _abi.load_library()
    for nm in names:
        assert hasattr(lib, nm)
    text = open(HEADER).read()
    assert re.search(r"#define PHYS_ABI_VERSION 2u?\b", text)


def test_python_surface():
    for cls in (physics_amd.World, __import__("physics_amd.state", fromlist=["PhysicsState"]).PhysicsState):
        assert callable(getattr(cls, "spherecast", None)) and callable(getattr(cls, "overlap", None))
    assert callable(getattr(physics_amd.World, "spherecast_device", None))


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    f32, u32, u64 = _abi.f32p, _abi.u32p, _abi.u64p
    o = np.zeros(3, np.float32)
    r = np.ones(1, np.float32)
    body = np.zeros(1, np.uint32)
    t = np.zeros(1, np.float32)
    rc = lib.phys_spherecast(None, 1, o.ctypes.data_as(f32), o.ctypes.data_as(f32), r.ctypes.data_as(f32), None, None,
                             body.ctypes.data_as(u32), t.ctypes.data_as(f32), None)
    assert rc == _abi.PHYS_ERR_INVALID_ARG
    rc = lib.phys_spherecast_device(None, 1, None, None, None, None, None, None, None, None)
    assert rc == _abi.PHYS_ERR_INVALID_ARG
    off = np.zeros(2, np.uint64)
    rc = lib.phys_overlap(None, 1, None, None, None, None, None, 0, off.ctypes.data_as(u64), None)
    assert rc == _abi.PHYS_ERR_INVALID_ARG
    # the Python layer checks shapes before it reaches the library
    w = physics_amd.World.__new__(physics_amd.World)
    with pytest.raises(ValueError):
        w.spherecast(np.zeros((2, 3)), np.zeros((3, 3)), 1.0)
    with pytest.raises(ValueError):
        w.spherecast(np.zeros((2, 3)), np.ones((2, 3)), 1.0, max_t=[1.0])
    with pytest.raises(ValueError):
        w.overlap(physics_amd.SHAPE_SPHERE, np.zeros((2, 3)))
    with pytest.raises(ValueError):
        w.overlap(physics_amd.SHAPE_BOX, np.zeros((2, 3)), rot=np.zeros((3, 4)), half_extent=[1, 1, 1])
