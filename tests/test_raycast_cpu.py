"""CPU: the float64 brute force of the ray-cast query (tests/raycast_ref.py) on hand cases with known answers, and the
query's surface - header declarations, exported symbols, the Python constants and World.raycast. No GPU needed."""
import math
import os
import re

import numpy as np

import physics_amd
from physics_amd import _abi

import raycast_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "physics_hip.h")


def _bodies(pos, shape, he, rot=None):
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    rot = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rot is None else np.asarray(rot, np.float64).reshape(-1, 4)
    return dict(pos=pos, rot=rot, half_extent=np.asarray(he, np.float64).reshape(-1, 3), shape=np.asarray(shape).reshape(-1))


def _one(o, d, bodies, **kw):
    h = ref.cast([o], [d], bodies, **kw)
    return int(h["body"][0]), float(h["t"][0]), h["normal"][0]


def test_reference_axis_aligned_box():
    b = _bodies([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 2, 3]])
    body, t, n = _one([-5, 0.5, 0.5], [2, 0, 0], b)
    assert body == 0 and t == 4.0 and np.allclose(n, [-1, 0, 0])
    body, t, n = _one([0.2, 10, 0], [0, -1, 0], b)
    assert body == 0 and t == 8.0 and np.allclose(n, [0, 1, 0])


def test_reference_box_turned_45_degrees_about_y():
    s = math.sin(math.pi / 8)
    b = _bodies([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 1, 1]], rot=[[0, s, 0, math.cos(math.pi / 8)]])
    body, t, n = _one([-5, 0, 0.3], [1, 0, 0], b)  # the diamond's face facing (-x, +z)
    assert body == 0 and abs(t - (5.3 - math.sqrt(2))) < 1e-12
    assert np.allclose(n, [-math.sqrt(0.5), 0, math.sqrt(0.5)])


def test_reference_sphere():
    b = _bodies([[0, 0, 0]], [ref.SHAPE_SPHERE], [[2, 0, 0]])
    body, t, n = _one([0, 0, -10], [0, 0, 3], b)
    assert body == 0 and t == 8.0 and np.allclose(n, [0, 0, -1])
    body, t, n = _one([0, 1, -10], [0, 0, 1], b)
    assert body == 0 and abs(t - (10 - math.sqrt(3))) < 1e-12 and np.allclose(n, [0, 0.5, -math.sqrt(0.75)])


def test_reference_origin_inside():
    b = _bodies([[0, 0, 0], [10, 0, 0]], [ref.SHAPE_BOX, ref.SHAPE_SPHERE], [[1, 1, 1], [1, 0, 0]])
    for o, want in (([0.5, 0, 0], 0), ([10, 0.5, 0], 1), ([1, 1, 1], 0)):  # the last: a corner, the closed solid
        body, t, n = _one(o, [0, 0, 2], b)
        assert body == want and t == 0.0 and np.allclose(n, [0, 0, -1])


def test_reference_parallel_miss():
    b = _bodies([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 1, 1]])
    body, t, n = _one([-5, 1.5, 0], [1, 0, 0], b)
    assert body == ref.MISS and t == math.inf and not n.any()
    body, t, _ = _one([-5, 1.0, 0], [1, 0, 0], b)  # along a face plane: the closed box is hit
    assert body == 0 and t == 4.0


def test_reference_max_t_and_ignore():
    b = _bodies([[0, 0, 0], [5, 0, 0]], [ref.SHAPE_BOX, ref.SHAPE_BOX], [[1, 1, 1], [1, 1, 1]])
    assert _one([-5, 0, 0], [1, 0, 0], b, max_t=[3.9])[0] == ref.MISS
    assert _one([-5, 0, 0], [1, 0, 0], b, max_t=[4.0])[:2] == (0, 4.0)
    assert _one([-5, 0, 0], [1, 0, 0], b, ignore=[0])[:2] == (1, 9.0)
    assert _one([-5, 0, 0], [1, 0, 0], b, ignore=[7])[:2] == (0, 4.0)


def test_reference_ground_and_its_tie_rule():
    b = _bodies([[10, -1, 0], [20, 2, 0], [20.5, 2, 0]], [ref.SHAPE_BOX] * 3, [[1, 1, 1]] * 3)
    body, t, n = _one([0, 5, 0], [0, -1, 0], b, ground=0.0)
    assert body == ref.GROUND and t == 5.0 and np.allclose(n, [0, 1, 0])
    body, t, _ = _one([10, 5, 0], [0, -1, 0], b, ground=0.0)  # the box's top is the ground plane: the body wins
    assert body == 0 and t == 5.0
    body, t, _ = _one([20.25, 5, 0], [0, -1, 0], b, ground=0.0)  # two bodies at the same t: the smaller id
    assert body == 1 and t == 2.0
    body, t, n = _one([0, -1, 0], [1, 0, 0], b, ground=0.0)  # origin inside the ground half-space
    assert body == ref.GROUND and t == 0.0 and np.allclose(n, [-1, 0, 0])
    assert _one([0, 5, 0], [0, 1, 0], b, ground=0.0)[0] == ref.MISS


def test_reference_bad_rays_miss():
    b = _bodies([[0, 0, 0]], [ref.SHAPE_BOX], [[1, 1, 1]])
    for o, d in (([-5, 0, 0], [0, 0, 0]), ([-5, 0, 0], [np.nan, 0, 0]), ([np.inf, 0, 0], [1, 0, 0])):
        assert _one(o, d, b, ground=0.0)[0] == ref.MISS


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(phys_[a-z0-9_]+)\s*\(", text))


def test_raycast_declared_and_exported():
    assert {"phys_raycast", "phys_raycast_device"} <= _declared()
    lib = _abi.load_library()
    assert hasattr(lib, "phys_raycast") and hasattr(lib, "phys_raycast_device")


def test_ray_constants_match_the_header():
    text = open(HEADER).read()
    vals = dict(re.findall(r"#define (PHYS_RAY_MISS|PHYS_RAY_GROUND)\s+(0x[0-9A-Fa-f]+)u", text))
    assert int(vals["PHYS_RAY_MISS"], 16) == physics_amd.RAY_MISS == ref.MISS
    assert int(vals["PHYS_RAY_GROUND"], 16) == physics_amd.RAY_GROUND == ref.GROUND == physics_amd.GROUND_ID


def test_world_has_raycast():
    assert callable(getattr(physics_amd.World, "raycast", None))
    assert callable(getattr(physics_amd.World, "raycast_device", None))
