"""CPU: the liquids without a GPU. The six symbols in the library, the ctypes table and the Rust shim; the constants against
the C compiler; the Python wrapper's checks, which raise before the library is called; known answers worked out by hand, for
the float64 reference (tests/liquid_ref.py) and for the library's own arithmetic (tests/cpp/liquid_probe.cpp compiles
include/spec/liquid.h and the setup.hpp staging with the host compiler alone, once under the address and undefined-behaviour
sanitizers); the probe against float64 on the committed scene; the capsule's slab rule against a fine quadrature; each shape
lowered through a surface; the validation messages."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import liquid_probe as lp
import liquid_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phys_set_liquids", "phys_set_liquid_poses", "phys_set_liquid_params", "phys_apply_liquids", "phys_get_submersion",
         "phys_get_submersion_device")
EPS = 2.0 ** -23
# The bounds of the probe against float64, C * 2^-23 * S with S = density * V_shape * |gravity| summed over the acting liquids
# (S * b for torques): four times the largest ratio measured on the committed scene (257 bodies, 40 liquids; zero and nonzero
# accumulators, plain and masked). Measured: spheres and boxes 8.52, capsules 6.50 (test_spec_against_float64 prints them).
C_SPHERE_BOX = 4 * 8.52
C_CAPSULE = 4 * 6.50


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return lp.build(str(tmp_path_factory.mktemp("liquid_probe") / "liquid_probe"))


@pytest.fixture(scope="module")
def probe_sanitized(tmp_path_factory):
    return lp.build(str(tmp_path_factory.mktemp("liquid_probe_san") / "liquid_probe"), sanitize=True)


def bound(res, shape, force=None, torque=None):
    """((n, 1), (n, 1)): what float32 may differ by in force and in torque, per body; the starting accumulators count as part
    of the sum that is rounded."""
    c = np.where(np.asarray(shape) == lr.CAPSULE, C_CAPSULE, C_SPHERE_BOX)
    f0 = 0.0 if force is None else np.linalg.norm(force, axis=1)
    t0 = 0.0 if torque is None else np.linalg.norm(torque, axis=1)
    return (c * EPS * (res["S"] + f0))[:, None], (c * EPS * (res["S"] * res["b"] + t0))[:, None]


# ---- symbols, constants, wrapper ------------------------------------------------------------------------------------------
def test_symbols_exported_bound_and_declared_in_the_rust_shim():
    from physics_amd import World, _abi
    lib = _abi.load_library()
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    header = open(os.path.join(ROOT, "include", "physics_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _abi.PROTOTYPES and len(re.findall(rf"pub fn {name}\s*\(", rust)) == 1
        assert re.search(rf"int32_t {name}\(", header)
    assert len(_abi.PROTOTYPES["phys_set_liquids"][1]) == 10
    for method in ("set_liquids", "set_liquid_poses", "set_liquid_params", "apply_liquids", "get_submersion", "get_submersion_device"):
        assert callable(getattr(World, method))


def test_constants_agree_with_the_header(tmp_path):
    import physics_amd
    from physics_amd import _abi
    src = '#include <stdio.h>\n#include "physics_hip.h"\nint main(){printf("%u", PHYS_MAX_LIQUIDS);}'
    exe = str(tmp_path / "liquid_constants")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = int(subprocess.check_output([exe]))
    assert got == 1024 == _abi.MAX_LIQUIDS == physics_amd.MAX_LIQUIDS
    assert _abi.NO_LIQUID == lr.NO_LIQUID == 0xFFFFFFFF
    assert f"pub const PHYS_MAX_LIQUIDS: u32 = {got};" in open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    header = open(os.path.join(ROOT, "include", "spec", "liquid.h")).read()
    assert re.search(r"#define kLiqCylSlabs 8\b", header) and re.search(r"#define kLiqCapSlabs 4\b", header)
    assert (lr.CYL_SLABS, lr.CAP_SLABS) == (8, 4)


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_validates_before_the_library_is_called():
    from physics_amd import World
    w = World.__new__(World)  # no phys_create: there is no GPU here, and the checks under test come before any call
    w.lib, w.h, w.n, w.n_liquids = _NoLibrary(), None, 0, 3
    pos = np.zeros((3, 3), np.float32)
    he = np.ones((3, 3), np.float32)
    ok = dict(half_extent=he, density=1000.0, gravity=[0, -9.81, 0])
    bad = [
        dict(density=1000.0, gravity=[0, -9.81, 0]),                                  # no half extents
        dict(half_extent=he, gravity=[0, -9.81, 0]),                                  # no density
        dict(half_extent=he, density=1000.0),                                         # no gravity
        dict(half_extent=np.ones((2, 3)), density=1000.0, gravity=[0, -9.81, 0]),     # wrong length
        dict(half_extent=-he, density=1000.0, gravity=[0, -9.81, 0]),                 # negative half extent
        dict(half_extent=he * np.inf, density=1000.0, gravity=[0, -9.81, 0]),
        dict(half_extent=he, density=[1.0, 2.0], gravity=[0, -9.81, 0]),              # two densities for three liquids
        dict(half_extent=he, density=-1.0, gravity=[0, -9.81, 0]),                    # negative density
        dict(half_extent=he, density=np.nan, gravity=[0, -9.81, 0]),
        dict(half_extent=he, density=1.0, gravity=np.zeros((2, 3))),
        dict(half_extent=he, density=1.0, gravity=[0, np.inf, 0]),
        dict(flow=np.zeros((2, 3)), **ok),
        dict(flow=[np.nan, 0, 0], **ok),
        dict(drag=[-1.0, 0.0], **ok),                                                 # negative linear drag
        dict(drag=[0.0, -1.0], **ok),                                                 # negative angular drag
        dict(drag=np.ones((2, 2)), **ok),
        dict(rot=np.zeros((2, 4), np.float32), **ok),                                 # rot length
        dict(rot=np.full((3, 4), np.nan, np.float32), **ok),
        dict(mask=[1, 2], **ok),                                                      # mask length
        dict(mask=0x10000, **ok),                                                     # mask range
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            w.set_liquids(pos, **kw)
    with pytest.raises(ValueError):
        w.set_liquids(np.full((3, 3), np.nan, np.float32), **ok)                      # NaN position
    with pytest.raises(ValueError):
        w.set_liquids(np.zeros((1025, 3), np.float32), half_extent=[1, 1, 1], density=1.0, gravity=[0, -1, 0])  # more than MAX_LIQUIDS
    with pytest.raises(ValueError):
        w.set_liquid_poses(np.zeros((2, 3), np.float32))                              # the world has three
    with pytest.raises(ValueError):
        w.set_liquid_poses(pos, rot=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        w.set_liquid_poses(np.full((3, 3), np.inf, np.float32))
    with pytest.raises(ValueError):
        w.set_liquid_params([1.0, 2.0], [0, -1, 0])
    with pytest.raises(ValueError):
        w.set_liquid_params(-1.0, [0, -1, 0])
    with pytest.raises(ValueError):
        w.set_liquid_params(1.0, [0, np.nan, 0])
    with pytest.raises(ValueError):
        w.set_liquid_params(1.0, [0, -1, 0], drag=[0.0, -2.0])
    w.h = None  # (nothing to destroy)


# ---- the spec header and the probe ----------------------------------------------------------------------------------------
def test_spec_header_needs_no_hip():
    header = os.path.join(ROOT, "include", "spec", "liquid.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", "-"], input=f'#include "{header}"\n', text=True,
                   check=True)
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-x", "c", "-"],
                   input=f'#include "{header}"\n', text=True, check=True)


def test_probe_holds_the_validation_messages(probe):
    r = subprocess.run([probe, "--messages"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout


def test_validation_messages_through_the_abi():
    """phys_set_liquids checks its arguments before it looks at the world, as phys_set_force_fields does."""
    from physics_amd import _abi
    lib = _abi.load_library()
    E = _abi.PHYS_ERR_INVALID_ARG
    n = 2
    pos, he = (C.c_float * (3 * n))(), (C.c_float * (3 * n))(*([1.0] * (3 * n)))
    density = (C.c_float * n)(1000.0, 800.0)
    gravity, flow = (C.c_float * (3 * n))(0, -9.81, 0, 0, -9.81, 0), (C.c_float * (3 * n))()
    drag = (C.c_float * (2 * n))(0.5, 0.5, 0.0, 1.0)

    def run(count=n, **kw):
        a = dict(pos=pos, rot=None, he=he, mask=None, density=density, gravity=gravity, flow=flow, drag=drag)
        a.update(kw)
        rc = lib.phys_set_liquids(None, count, a["pos"], a["rot"], a["he"], a["mask"], a["density"], a["gravity"], a["flow"], a["drag"])
        return rc, lib.phys_last_error().decode()

    assert run() == (E, "null world")  # every liquid passes: the world is looked at next
    assert run(count=1025) == (E, "phys_set_liquids: more than PHYS_MAX_LIQUIDS liquids")
    for missing in ("pos", "he", "density", "gravity", "flow", "drag"):
        assert run(**{missing: None}) == (E, "liquids need pos, half_extent, density, gravity, flow and drag")
    flow[4] = float("nan")
    he[1] = -1.0
    assert run() == (E, "liquid 0: negative half extent")  # the first offender, whatever the second one's reason
    he[1] = 1.0
    assert run() == (E, "liquid 1: non-finite number")
    flow[4] = 0.0
    he[4] = -1.0
    density[1] = -1.0
    drag[3] = -1.0
    assert run() == (E, "liquid 1: negative half extent")
    he[4] = 1.0
    assert run() == (E, "liquid 1: negative density")
    density[1] = 800.0
    assert run() == (E, "liquid 1: negative drag coefficient")
    drag[3] = 1.0
    drag[0] = -0.5
    assert run() == (E, "liquid 0: negative drag coefficient")
    for name in NAMES[1:]:
        args = {"phys_set_liquid_poses": (None, 0, None, None), "phys_set_liquid_params": (None, 0, None, None, None, None),
                "phys_apply_liquids": (None,), "phys_get_submersion": (None, None, None), "phys_get_submersion_device": (None, None, None)}[name]
        assert getattr(lib, name)(*args) == E and lib.phys_last_error().decode() == "null world"


# ---- known answers by hand ----------------------------------------------------------------------------------------------
S2 = float(np.sqrt(0.5))
RZ45 = [0.0, 0.0, float(np.sin(np.pi / 8)), float(np.cos(np.pi / 8))]  # 45 degrees about z
RZ90 = [0.0, 0.0, S2, S2]                                              # a quarter turn about z: local y -> world -x
ID = [0.0, 0.0, 0.0, 1.0]
G = 10.0
# a pool of +-4 x +-4 whose surface is y = 0 and whose bottom is y = -6, density 2, weighed by (0, -10, 0)
POOL = dict(pos=[0, -3, 0], rot=None, he=[4, 3, 4], density=2.0, gravity=[0, -G, 0], flow=[0, 0, 0], drag=[0, 0])
V_SPHERE = 4.0 / 3.0 * np.pi * 0.5 ** 3
V_BOX = 8 * 0.5 * 0.25 * 0.75
V_CAPS = np.pi * 0.25 ** 2 * (2 * 0.5 + 4.0 / 3.0 * 0.25)
# (label, liquid overrides, shape, half extent, position, rotation, velocity, spin, force or None, torque or None (not checked), frac)
HAND = [
    ("sphere fully submerged", {}, lr.SPHERE, [0.5, 0, 0], [1, -2, 1], ID, None, None, [0, 2 * V_SPHERE * G, 0], [0, 0, 0], 1.0),
    ("box fully submerged, turned", {}, lr.BOX, [0.5, 0.25, 0.75], [1, -2, 1], RZ45, None, None, [0, 2 * V_BOX * G, 0], [0, 0, 0], 1.0),
    ("capsule fully submerged, turned", {}, lr.CAPSULE, [0.25, 0.5, 0], [1, -2, 1], RZ45, None, None, [0, 2 * V_CAPS * G, 0], [0, 0, 0], 1.0),
    ("sphere dry", {}, lr.SPHERE, [0.5, 0, 0], [1, 0.75, 1], ID, None, None, None, None, 0.0),
    ("box dry", {}, lr.BOX, [0.5, 0.25, 0.75], [1, 1.0, 1], RZ45, None, None, None, None, 0.0),
    ("capsule dry", {}, lr.CAPSULE, [0.25, 0.5, 0], [1, 1.0, 1], ID, None, None, None, None, 0.0),
    ("sphere outside the footprint", {}, lr.SPHERE, [0.5, 0, 0], [4.25, -2, 1], ID, None, None, None, None, 0.0),
    ("box outside the footprint in z", {}, lr.BOX, [0.5, 0.25, 0.75], [1, -2, -4.25], ID, None, None, None, None, 0.0),
    ("capsule under the bottom", {}, lr.CAPSULE, [0.25, 0.5, 0], [1, -6.25, 1], ID, None, None, None, None, 0.0),
    ("sphere, the surface through its centre: half", {}, lr.SPHERE, [0.5, 0, 0], [1, 0, 1], ID, None, None, [0, V_SPHERE * G, 0], [0, 0, 0], 0.5),
    ("axis-aligned box at depth d = 0.125: 4 h.x h.z d", {}, lr.BOX, [0.5, 0.25, 0.75], [1, 0.125, 1], ID, None, None,
     [0, 2 * (4 * 0.5 * 0.75 * 0.125) * G, 0], [0, 0, 0], 0.25),
    ("box turned 45 degrees, the surface through its centre: half", {}, lr.BOX, [0.5, 0.25, 0.75], [1, 0, 1], RZ45, None, None,
     [0, V_BOX * G, 0], None, 0.5),
    ("horizontal capsule, the surface through its axis: half", {}, lr.CAPSULE, [0.25, 0.5, 0], [1, 0, 1], RZ90, None, None,
     [0, V_CAPS * G, 0], [0, 0, 0], 0.5),
    ("vertical capsule wet to the middle of its cylinder: half", {}, lr.CAPSULE, [0.25, 0.5, 0], [1, 0, 1], ID, None, None,
     [0, V_CAPS * G, 0], [0, 0, 0], 0.5),
    ("drag scaled by frac: the half-wet sphere", dict(drag=[3.0, 5.0], flow=[1, 0, 0]), lr.SPHERE, [0.5, 0, 0], [1, 0, 1], ID, [3, 2, -4], [0, 2, 4],
     [-3.0, V_SPHERE * G - 3.0, 6.0], [0, -5.0, -10.0], 0.5),
    ("a tilted liquid: n is not gravity's direction; the sphere is still under the slanted surface",
     dict(pos=[0, 0, 0], rot=RZ45, he=[4, 1, 4]), lr.SPHERE, [0.5, 0, 0], [0.5, -0.5, 0], ID, None, None, [0, 2 * V_SPHERE * G, 0], [0, 0, 0], 1.0),
    ("a tilted liquid: half of the sphere below the slanted surface, pushed along -gravity and not along n",
     dict(pos=[0, 0, 0], rot=RZ45, he=[4, 1, 4]), lr.SPHERE, [0.5, 0, 0], [-S2, S2, 0], ID, None, None, [0, V_SPHERE * G, 0], None, 0.5),
]


def _liquids(*overrides):
    rows = [dict(POOL, **o) for o in overrides]
    rot = None if all(r["rot"] is None for r in rows) else np.array([ID if r["rot"] is None else r["rot"] for r in rows], np.float32)
    return dict(pos=np.array([r["pos"] for r in rows], np.float32), rot=rot, half_extent=np.array([r["he"] for r in rows], np.float32),
                mask=None, density=np.array([r["density"] for r in rows], np.float32), gravity=np.array([r["gravity"] for r in rows], np.float32),
                flow=np.array([r["flow"] for r in rows], np.float32), drag=np.array([r["drag"] for r in rows], np.float32))


def _body(shape, he, x, q, v=None, w=None):
    z = [0, 0, 0]
    return dict(shape=np.array([shape], np.uint32), pos=np.array([x], np.float32), rot=np.array([q], np.float32),
                half_extent=np.array([he], np.float32), vel=np.array([z if v is None else v], np.float32),
                ang=np.array([z if w is None else w], np.float32))


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_known_answers_by_hand(case, probe, tmp_path):
    """One body in one liquid; the starting accumulators are (1, 2, 3) and (-1, -2, -3), and a liquid that does not act leaves
    them as they are and reads out (0, none)."""
    _, over, shape, he, x, q, v, w, F, T, frac = case
    liquids, body = _liquids(over), _body(shape, he, x, q, v, w)
    acc_f, acc_t = np.array([[1, 2, 3]], np.float32), np.array([[-1, -2, -3]], np.float32)
    res = lr.evaluate(liquids, body, force=acc_f, torque=acc_t)
    acted, got_f, got_t, got_frac, got_liquid = lp.evaluate(probe, tmp_path, liquids, body, force=acc_f, torque=acc_t)
    assert res["K"][0] == (F is not None) and acted[0] == (F is not None)
    # (the reference reads the float32 inputs the library gets: a quaternion of sines is not unit to more than 2^-24)
    assert res["frac"][0] == pytest.approx(frac, abs=1e-6) and got_frac[0] == pytest.approx(frac, abs=1e-6)
    if F is None:
        assert got_f.tobytes() == acc_f.tobytes() and got_t.tobytes() == acc_t.tobytes()
        assert got_liquid[0] == lr.NO_LIQUID and res["liquid"][0] == lr.NO_LIQUID and got_frac[0] == 0.0
        return
    assert got_liquid[0] == 0 and res["liquid"][0] == 0
    tol_f, tol_t = bound(res, [shape], acc_f, acc_t)
    assert np.allclose(res["F"][0], acc_f[0] + np.array(F), rtol=0, atol=1e-5)
    assert (np.abs(got_f[0] - res["F"][0]) <= tol_f[0]).all(), (got_f, res["F"])
    assert (np.abs(got_t[0] - res["T"][0]) <= tol_t[0]).all(), (got_t, res["T"])
    if T is not None:
        assert np.allclose(res["T"][0], acc_t[0] + np.array(T), rtol=0, atol=1e-5)


@pytest.mark.parametrize("shape,he", [(lr.BOX, [0.5, 0.125, 0.25]), (lr.CAPSULE, [0.125, 0.5, 0])], ids=["box", "capsule"])
def test_a_tilted_half_wet_body_is_righted(shape, he, probe, tmp_path):
    """A plank (box: thin in y, long in x; capsule: long in y) with the surface through its centre, turned by +-0.3 about z from
    the attitude it floats in (box: flat; capsule: lying, its axis along world x): the torque about z has the sign that turns
    it back, in the reference and in the probe, and vanishes at that attitude."""
    flat = 0.0 if shape == lr.BOX else np.pi / 2
    for tilt in (0.3, -0.3, 0.0):
        a = flat + tilt
        q = [0.0, 0.0, float(np.sin(a / 2)), float(np.cos(a / 2))]
        body = _body(shape, he, [0, 0, 0], q)
        res = lr.evaluate(_liquids({}), body)
        _, _, got_t, got_frac, _ = lp.evaluate(probe, tmp_path, _liquids({}), body)
        tol = bound(res, [shape])[1][0]
        assert abs(got_t[0][2] - res["T"][0][2]) <= tol and got_frac[0] == pytest.approx(0.5, abs=1e-6)
        if tilt:
            assert np.sign(res["T"][0][2]) == -np.sign(tilt) and np.sign(got_t[0][2]) == -np.sign(tilt)
            assert abs(res["T"][0][2]) > 1e-3 * res["S"][0] * res["b"][0]
        else:
            assert abs(res["T"][0][2]) < 1e-9 and abs(got_t[0][2]) <= tol


def test_masks_and_two_overlapping_liquids_in_index_order(probe, tmp_path):
    """Two pools over the same place, the second denser and flowing: both act, in index order (the read-out names the first);
    a body whose category only the second one's mask has gets the second alone, and one that neither has gets nothing."""
    liquids = _liquids({}, dict(density=5.0, drag=[2.0, 0.0], flow=[1, 0, 0]))
    body = _body(lr.SPHERE, [0.5, 0, 0], [1, 0, 1], ID)
    both = V_SPHERE * G * (2.0 + 5.0) / 2
    for masks, cat, fy, fx, first in ((None, 1, both, 1.0, 0), ([1, 2], 2, 5.0 * V_SPHERE * G / 2, 1.0, 1), ([1, 2], 3, both, 1.0, 0),
                                      ([1, 2], 4, None, None, lr.NO_LIQUID)):
        lq = dict(liquids, mask=None if masks is None else np.array(masks, np.uint16))
        res = lr.evaluate(lq, body, category=cat)
        acted, got_f, _, got_frac, got_liquid = lp.evaluate(probe, tmp_path, lq, body, category=cat)
        assert got_liquid[0] == first == res["liquid"][0] and acted[0] == (fy is not None)
        if fy is None:
            assert not got_f.any() and got_frac[0] == 0.0
            continue
        assert res["F"][0] == pytest.approx([fx, fy, 0.0], abs=1e-6)  # drag 2 * frac 0.5 * (0 - (-1))
        assert (np.abs(got_f[0] - res["F"][0]) <= bound(res, [lr.SPHERE])[0][0]).all()
    # index order: float32 sums are not associative, and the probe's are those of liquid 0 first
    swapped = {k: (None if v is None else v[::-1].copy()) for k, v in liquids.items()}
    a = lp.evaluate(probe, tmp_path, liquids, body, force=np.array([[0.1, 0.3, 0.7]], np.float32))
    b = lp.evaluate(probe, tmp_path, swapped, body, force=np.array([[0.1, 0.3, 0.7]], np.float32))
    assert a[4][0] == 0 and b[4][0] == 0 and np.allclose(a[1], b[1], rtol=1e-6)


# ---- the committed scene ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bodies,n_liquids,pairs,most,untouched,closest", [(65, 33, 183, 9, 14, 4.05e-3), (257, 40, 880, 10, 36, 1.88e-3)])
def test_committed_scene_figures(n_bodies, n_liquids, pairs, most, untouched, closest):
    """No (liquid, body) pair of the committed scene lies within 1e-3 of a footprint or bottom boundary or of first touching the
    surface, so float32 and float64 agree on who is acted on and the comparisons need no exclusions."""
    bodies, liquids = lr.scene(n_bodies, n_liquids)
    res = lr.evaluate(liquids, bodies)
    part = (res["frac"] > 0) & (res["frac"] < 1)
    print(f"scene ({n_bodies}, {n_liquids}): closest {res['margin']:.3e}, {len(res['pairs'])} pairs, most {res['K'].max()}, "
          f"untouched {(res['K'] == 0).sum()}, partly wet by shape {[int((part & (bodies['shape'] == k)).sum()) for k in (1, 2, 3)]}")
    assert res["margin"] > 1e-3 and res["margin"] == pytest.approx(closest, rel=0.02)
    assert (len(res["pairs"]), int(res["K"].max()), int((res["K"] == 0).sum())) == (pairs, most, untouched)
    assert all((part & (bodies["shape"] == k)).sum() > 0 for k in (1, 2, 3))


@pytest.mark.parametrize("n_bodies", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_liquids", [1, 32, 33, 40])
def test_every_size_of_the_gpu_comparison_keeps_clear_of_the_boundaries(n_bodies, n_liquids):
    bodies, liquids = lr.scene(n_bodies, n_liquids)
    lr_wet, lr.wet = lr.wet, lambda *a: (1.0, np.zeros(3))  # (the margins do not need the volumes)
    try:
        assert lr.evaluate(liquids, bodies)["margin"] > 1e-3
    finally:
        lr.wet = lr_wet


def test_spec_against_float64_on_the_committed_scene(probe, probe_sanitized, tmp_path):
    """The probe on the committed scene (257 bodies, 40 liquids), zero and nonzero starting accumulators, plain and masked:
    within C * 2^-23 * S (S * b for torques) of the float64 reference per body and component, no exclusions; untouched bodies
    keep their bits; the read-out agrees; and the build under -fsanitize=address,undefined prints the same bits and reports
    nothing."""
    bodies, liquids = lr.scene(257, 40)
    rng = np.random.default_rng(11)
    acc = rng.normal(size=(2, 257, 3)).astype(np.float32) * 5
    cat = (1 << rng.integers(0, 4, 257)).astype(np.uint16)
    masks = rng.integers(1, 16, 40).astype(np.uint16)
    sh = bodies["shape"]
    worst = {"sphere and box": 0.0, "capsule": 0.0}
    for label, f, t, masked in (("zero", None, None, False), ("nonzero", acc[0], acc[1], False), ("masked", acc[0], acc[1], True)):
        lq = dict(liquids, mask=masks if masked else None)
        acted, got_f, got_t, got_frac, got_liquid = lp.evaluate(probe, tmp_path, lq, bodies, category=cat, force=f, torque=t)
        res = lr.evaluate(lq, bodies, category=cat, force=f, torque=t)
        assert (acted == (res["K"] > 0)).all() and (got_liquid == res["liquid"]).all()
        assert np.abs(got_frac - res["frac"]).max() <= 64 * EPS
        tol_f, tol_t = bound(res, sh, f, t)
        err_f, err_t = np.abs(got_f - res["F"]), np.abs(got_t - res["T"])
        c = np.where(sh == lr.CAPSULE, C_CAPSULE, C_SPHERE_BOX)[:, None]
        ratio = np.maximum(err_f / np.maximum(tol_f, 1e-300), err_t / np.maximum(tol_t, 1e-300)) * c
        for name, sel in (("sphere and box", acted & (sh != lr.CAPSULE)), ("capsule", acted & (sh == lr.CAPSULE))):
            worst[name] = max(worst[name], float(ratio[sel].max()))
        assert (err_f <= tol_f).all() and (err_t <= tol_t).all(), label
        start_f, start_t = (np.zeros((257, 3), np.float32) if f is None else f), (np.zeros((257, 3), np.float32) if t is None else t)
        assert got_f[~acted].tobytes() == start_f[~acted].tobytes() and got_t[~acted].tobytes() == start_t[~acted].tobytes()
        if label == "masked":
            san = lp.evaluate(probe_sanitized, tmp_path, lq, bodies, category=cat, force=f, torque=t)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(san, (acted, got_f, got_t, got_frac, got_liquid)))
    print(f"largest error / (2^-23 S): {worst}; the bounds are four times the figures in this file's head")
    assert worst["sphere and box"] > C_SPHERE_BOX / 16 and worst["capsule"] > C_CAPSULE / 16  # (the bounds are not slack)
    r = subprocess.run([probe_sanitized, "--messages"], capture_output=True, text=True)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr


# ---- the capsule's slab rule against the truth ----------------------------------------------------------------------------------
def test_capsule_slab_rule_against_a_fine_quadrature():
    """The reference's statement of the slab rule against 20 000 true discs, float64, 320 seeded capsules: random attitudes and
    depths, and every tenth one vertical, every tenth horizontal. The volume is within 1 % of V_shape (a condition); the moment
    error, as a fraction of V_shape * (r + L), is reported with a bound at twice what was measured: 0.1589 (the in-disc offset
    of a cut disc's centroid is what the rule leaves out: 4 / (3 pi) of the radius for a half-wet lying capsule)."""
    rng = np.random.default_rng(2029)
    worst_v = worst_m = 0.0
    n = np.array([0.0, 1.0, 0.0])
    for k in range(320):
        r, L = rng.uniform(0.1, 0.6), rng.uniform(0.0, 1.2)
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if k % 10 == 0:
            q = np.array(ID)
        elif k % 10 == 5:
            a = rng.uniform(0, 2 * np.pi)  # horizontal: the axis turned into the x-z plane
            q = np.array([np.sin(a) * S2, 0.0, np.cos(a) * S2, S2]) if k % 20 == 5 else np.array(RZ90)
        R = lr.rot_matrix(q)
        reach = abs(R[1, 1]) * L + r
        s = rng.uniform(-reach, reach)
        V, M = lr.wet_capsule(R, r, L, s, n)
        Vt, Mt = lr.capsule_truth(R, r, L, s, n)
        Vs = lr.shape_volume(lr.CAPSULE, [r, L, 0])
        worst_v = max(worst_v, abs(V - Vt) / Vs)
        worst_m = max(worst_m, float(np.linalg.norm(M - Mt)) / (Vs * (r + L)))
    print(f"capsule slab rule vs 20000 discs: volume {worst_v:.4%} of V_shape, moment {worst_m:.4%} of V_shape (r + L)")
    assert worst_v < 0.01
    assert worst_m < 2 * 0.1589
    full = lr.wet_capsule(np.eye(3), 0.3, 0.7, -5.0, n)
    assert full[0] == pytest.approx(lr.shape_volume(lr.CAPSULE, [0.3, 0.7, 0]), rel=1e-14) and np.abs(full[1]).max() < 1e-15


# ---- monotone and continuous -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,he", [(lr.SPHERE, [0.4, 0, 0]), (lr.BOX, [0.5, 0.2, 0.35]), (lr.CAPSULE, [0.2, 0.45, 0])],
                         ids=["sphere", "box", "capsule"])
def test_lowered_through_the_surface_the_volume_is_monotone_and_continuous(shape, he, probe, tmp_path):
    """Each shape lowered through the surface in 512 steps at three attitudes (as given, about 33 degrees off, and a random
    one): V_sub from the probe never decreases by more than the float32 tolerance, no step changes it by more than 2 / 512 of
    V_shape plus that tolerance, and it runs from 0 to V_shape. A staircase rule fails this."""
    Vs = lr.shape_volume(shape, he)
    tol = (C_CAPSULE if shape == lr.CAPSULE else C_SPHERE_BOX) * EPS * Vs
    rng = np.random.default_rng(3)
    qr = rng.normal(size=4)
    for q in (ID, [0.0, 0.0, float(np.sin(0.29)), float(np.cos(0.29))], list(qr / np.linalg.norm(qr))):
        reach = lr.shape_reach(shape, lr.rot_matrix(q), he, np.array([0.0, 1.0, 0.0])) * 1.02
        ys = np.linspace(reach, -reach, 513)
        n = len(ys)
        bodies = dict(shape=np.full(n, shape, np.uint32), pos=np.stack([np.zeros(n), ys, np.zeros(n)], 1).astype(np.float32),
                      rot=np.tile(np.array(q, np.float32), (n, 1)), half_extent=np.tile(np.array(he, np.float32), (n, 1)))
        lq = _liquids(dict(density=1.0, gravity=[0, -1, 0]))
        _, F, _, frac, _ = lp.evaluate(probe, tmp_path, lq, bodies)
        V = F[:, 1].astype(np.float64)
        step = np.diff(V)
        assert step.min() >= -tol, step.min()
        assert step.max() <= 2.0 / 512 * Vs + tol, (step.max() / Vs * 512)
        assert V[0] == 0.0 and V[-1] == pytest.approx(Vs, rel=1e-6) and frac[-1] == 1.0
