"""CPU: the force fields without a GPU. The four symbols in the library, the ctypes table and the Rust shim; the constants
against the C compiler; the Python wrapper's checks, which raise before the library is called; the float64 reference
(tests/field_ref.py) on its own and the figures of the committed scene; known answers worked out by hand, for the reference and
for the library's own arithmetic (tests/cpp/field_probe.cpp compiles include/spec/force_field.h and the setup.hpp staging with
the host compiler alone, once under the address and undefined-behaviour sanitizers); the validation messages."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import field_probe as fp
import field_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phys_set_force_fields", "phys_set_force_field_poses", "phys_set_force_field_params", "phys_apply_force_fields")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return fp.build(str(tmp_path_factory.mktemp("field_probe") / "field_probe"))


@pytest.fixture(scope="module")
def probe_sanitized(tmp_path_factory):
    return fp.build(str(tmp_path_factory.mktemp("field_probe_san") / "field_probe"), sanitize=True)


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
    assert len(_abi.PROTOTYPES["phys_set_force_fields"][1]) == 11
    for method in ("set_force_fields", "set_force_field_poses", "set_force_field_params", "apply_force_fields"):
        assert callable(getattr(World, method))


def test_constants_agree_with_the_header(tmp_path):
    import physics_amd
    from physics_amd import _abi
    src = ('#include <stdio.h>\n#include "physics_hip.h"\nint main(){printf("%u %u %u %u", PHYS_MAX_FORCE_FIELDS, PHYS_FIELD_ACCEL, '
           'PHYS_FIELD_DRAG, PHYS_FIELD_RADIAL);}')
    exe = str(tmp_path / "field_constants")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [1024, 0, 1, 2]
    assert got == [_abi.MAX_FORCE_FIELDS, _abi.FIELD_ACCEL, _abi.FIELD_DRAG, _abi.FIELD_RADIAL]
    assert got == [physics_amd.MAX_FORCE_FIELDS, physics_amd.FIELD_ACCEL, physics_amd.FIELD_DRAG, physics_amd.FIELD_RADIAL]
    assert (fr.ACCEL, fr.DRAG, fr.RADIAL) == (0, 1, 2)
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    for name, value in zip(("MAX_FORCE_FIELDS", "FIELD_ACCEL", "FIELD_DRAG", "FIELD_RADIAL"), got):
        assert f"pub const PHYS_{name}: u32 = {value};" in rust


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_validates_before_the_library_is_called():
    from physics_amd import FIELD_ACCEL, FIELD_DRAG, FIELD_RADIAL, World
    w = World.__new__(World)  # no phys_create: there is no GPU here, and the checks under test come before any call
    w.lib, w.h, w.n, w.n_static, w.n_triggers = _NoLibrary(), None, 0, 0, 0
    w.n_fields, w._field_kinds = 3, np.array([FIELD_ACCEL, FIELD_DRAG, FIELD_RADIAL], np.uint32)
    pos = np.zeros((3, 3), np.float32)
    he = np.ones((3, 3), np.float32)
    kinds = [FIELD_ACCEL, FIELD_DRAG, FIELD_RADIAL]
    ok = dict(half_extent=he, vec=np.zeros(3), coef=[1.0, 1.0])
    bad = [
        dict(kind=[0, 1], shape_type=2, **ok),                                        # two kinds for three fields
        dict(kind=3, shape_type=2, **ok),                                             # an unknown kind
        dict(kind=kinds, shape_type=0, **ok),                                         # an unknown shape
        dict(kind=kinds, shape_type=[2, 2], **ok),                                    # wrong length
        dict(kind=kinds, shape_type=2, vec=np.zeros(3), coef=[1.0, 1.0]),             # no half extents
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros(3)),              # no coefficients
        dict(kind=kinds, shape_type=2, half_extent=np.ones((2, 3)), vec=np.zeros(3), coef=[1.0, 1.0]),
        dict(kind=kinds, shape_type=2, half_extent=-he, vec=np.zeros(3), coef=[1.0, 1.0]),  # negative half extent
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros((2, 3)), coef=[1.0, 1.0]),
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros(3), coef=np.ones((2, 2))),
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros(3), coef=[-1.0, 1.0]),  # negative linear drag
        dict(kind=FIELD_DRAG, shape_type=2, half_extent=he, vec=np.zeros(3), coef=[1.0, -1.0]),  # negative angular drag
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros(3), coef=[1.0, 0.0]),   # r0 == 0
        dict(kind=FIELD_RADIAL, shape_type=1, half_extent=he, vec=np.zeros(3), coef=[1.0, -2.0]),  # r0 < 0
        dict(kind=kinds, shape_type=2, exponent=3, **ok),                             # exponent 3
        dict(kind=kinds, shape_type=2, exponent=[0, 1], **ok),
        dict(kind=kinds, shape_type=2, half_extent=he, vec=[np.nan, 0, 0], coef=[1.0, 1.0]),  # NaN
        dict(kind=kinds, shape_type=2, half_extent=he, vec=np.zeros(3), coef=[np.nan, 1.0]),
        dict(kind=kinds, shape_type=2, half_extent=he * np.inf, vec=np.zeros(3), coef=[1.0, 1.0]),
        dict(kind=kinds, shape_type=2, rot=np.zeros((2, 4), np.float32), **ok),       # rot length
        dict(kind=kinds, shape_type=2, rot=np.full((3, 4), np.nan, np.float32), **ok),
        dict(kind=kinds, shape_type=2, mask=[1, 2], **ok),                            # mask length
        dict(kind=kinds, shape_type=2, mask=0x10000, **ok),                           # mask range
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            w.set_force_fields(pos=pos, **kw)
    with pytest.raises(ValueError):
        w.set_force_fields(kinds, 2, np.full((3, 3), np.nan, np.float32), **ok)       # NaN position
    with pytest.raises(ValueError):
        w.set_force_fields(0, 2, np.zeros((1025, 3), np.float32), **ok)               # more than MAX_FORCE_FIELDS
    with pytest.raises(ValueError):
        w.set_force_field_poses(np.zeros((2, 3), np.float32))                         # the world has three
    with pytest.raises(ValueError):
        w.set_force_field_poses(pos, rot=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        w.set_force_field_poses(np.full((3, 3), np.inf, np.float32))
    with pytest.raises(ValueError):
        w.set_force_field_params(np.zeros((2, 3)), np.ones((3, 2)))
    with pytest.raises(ValueError):
        w.set_force_field_params(np.zeros(3), [-1.0, 1.0])                            # field 1 is a DRAG
    with pytest.raises(ValueError):
        w.set_force_field_params(np.zeros(3), [1.0, 0.0])                             # field 2 is a RADIAL: r0
    with pytest.raises(ValueError):
        w.set_force_field_params([0, np.nan, 0], [1.0, 1.0])
    w.h = None  # (nothing to destroy)


# ---- the spec header and the probe ----------------------------------------------------------------------------------------
def test_spec_header_needs_no_hip():
    header = os.path.join(ROOT, "include", "spec", "force_field.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", "-"], input=f'#include "{header}"\n', text=True,
                   check=True)
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-x", "c", "-"],
                   input=f'#include "{header}"\n', text=True, check=True)


def test_probe_holds_the_validation_messages(probe):
    r = subprocess.run([probe, "--messages"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout


def test_validation_messages_through_the_abi():
    """phys_set_force_fields checks its arguments before it looks at the world, as phys_set_triggers does."""
    from physics_amd import _abi
    lib = _abi.load_library()
    E = _abi.PHYS_ERR_INVALID_ARG
    n = 2
    kind = (C.c_uint32 * n)(1, 2)
    shape = (C.c_uint32 * n)(2, 1)
    pos, he, vec = (C.c_float * (3 * n))(), (C.c_float * (3 * n))(*([1.0] * (3 * n))), (C.c_float * (3 * n))()
    coef = (C.c_float * (2 * n))(0.5, 0.5, -4.0, 1.0)
    ex = (C.c_uint32 * n)(0, 2)

    def run(count=n, **kw):
        a = dict(kind=kind, shape=shape, pos=pos, rot=None, he=he, mask=None, vec=vec, coef=coef, ex=ex)
        a.update(kw)
        rc = lib.phys_set_force_fields(None, count, a["kind"], a["shape"], a["pos"], a["rot"], a["he"], a["mask"], a["vec"], a["coef"], a["ex"])
        return rc, lib.phys_last_error().decode()

    assert run() == (E, "null world")  # every field passes: the world is looked at next
    assert run(ex=None) == (E, "null world")
    assert run(count=1025) == (E, "phys_set_force_fields: more than PHYS_MAX_FORCE_FIELDS force fields")
    for missing in ("kind", "shape", "pos", "he", "vec", "coef"):
        assert run(**{missing: None}) == (E, "force fields need kind, shape_type, pos, half_extent, vec and coef")
    kind[1] = 7
    assert run() == (E, "force field 1: kind is neither ACCEL nor DRAG nor RADIAL")
    kind[1] = 2
    shape[0] = 0
    assert run() == (E, "force field 0: shape is neither SPHERE nor BOX nor CAPSULE")
    shape[0] = 2
    vec[4] = float("nan")
    assert run() == (E, "force field 1: non-finite number")
    vec[4] = 0.0
    he[1] = -1.0
    assert run() == (E, "force field 0: negative half extent")
    he[1] = 1.0
    coef[1] = -0.5
    assert run() == (E, "force field 0: negative drag coefficient")
    coef[1] = 0.5
    coef[3] = 0.0
    assert run() == (E, "force field 1: r0 (coef[1]) must be above 0")
    coef[3] = 1.0
    ex[1] = 3
    assert run() == (E, "force field 1: exponent above 2")
    for name in NAMES[1:]:
        args = {"phys_set_force_field_poses": (None, 0, None, None), "phys_set_force_field_params": (None, 0, None, None),
                "phys_apply_force_fields": (None,)}[name]
        assert getattr(lib, name)(*args) == E and lib.phys_last_error().decode() == "null world"


# ---- the reference on its own, and the committed scene ----------------------------------------------------------------------
def test_reference_signed_distances():
    s = np.sqrt(0.5)
    rz = [0, 0, s, s]  # a quarter turn about z: local x -> world y, local y -> world -x
    assert fr.signed_distance(fr.SPHERE, [1, 2, 3], None, [2, 0, 0], [1, 2, 4]) == pytest.approx(-1.0)
    assert fr.signed_distance(fr.SPHERE, [1, 2, 3], rz, [2, 0, 0], [4, 2, 3]) == pytest.approx(1.0)
    assert fr.signed_distance(fr.BOX, [0, 0, 0], None, [1, 2, 3], [0.5, 0, 0]) == pytest.approx(-0.5)
    assert fr.signed_distance(fr.BOX, [0, 0, 0], None, [1, 2, 3], [2, 3, 3]) == pytest.approx(np.sqrt(2.0))
    assert fr.signed_distance(fr.BOX, [0, 0, 0], rz, [1, 2, 3], [1.5, 0, 0]) == pytest.approx(-0.5)   # world x is local y: 2 - 1.5
    assert fr.signed_distance(fr.BOX, [0, 0, 0], rz, [1, 2, 3], [0, 1.5, 0]) == pytest.approx(0.5)    # world y is local x: 1.5 - 1
    assert fr.signed_distance(fr.CAPSULE, [0, 0, 0], None, [0.5, 2, 0], [0, 2.25, 0]) == pytest.approx(-0.25)
    assert fr.signed_distance(fr.CAPSULE, [0, 0, 0], None, [0.5, 2, 0], [1, 0, 0]) == pytest.approx(0.5)
    assert fr.signed_distance(fr.CAPSULE, [0, 0, 0], rz, [0.5, 2, 0], [-2.25, 0, 0]) == pytest.approx(-0.25)  # the core lies along world x


@pytest.mark.parametrize("n_bodies,n_fields,pairs,most,untouched,closest", [(65, 33, 62, 4, 23, 7.6e-3), (257, 70, 357, 5, 61, 2.7e-3)])
def test_committed_scene_figures(n_bodies, n_fields, pairs, most, untouched, closest):
    """No (field, body) pair of the committed scene lies within 1e-3 of a boundary, so the comparisons on it need no exclusions."""
    bodies, fields = fr.scene(n_bodies, n_fields)
    res = fr.evaluate(fields, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"])
    print(f"scene ({n_bodies}, {n_fields}): closest {res['margin']:.3e}, {len(res['pairs'])} pairs, most {res['K'].max()}, "
          f"untouched {(res['K'] == 0).sum()}, kinds {np.bincount(fields['kind'], minlength=3)}, shapes {np.bincount(fields['shape'])[1:]}")
    assert res["margin"] > 1e-3 and res["margin"] == pytest.approx(closest, rel=0.02)
    assert (len(res["pairs"]), int(res["K"].max()), int((res["K"] == 0).sum())) == (pairs, most, untouched)
    assert (np.bincount(fields["kind"], minlength=3) > 0).all() and (np.bincount(fields["shape"], minlength=4)[1:] > 0).all()
    assert np.abs(fields["pos"]).max() <= 7.0 and fields["half_extent"].min() >= 0.8 and fields["half_extent"].max() <= 3.5


@pytest.mark.parametrize("n_bodies", [63, 64, 65, 257])
@pytest.mark.parametrize("n_fields", [1, 32, 33, 70])
def test_every_size_of_the_gpu_comparison_keeps_clear_of_the_boundaries(n_bodies, n_fields):
    bodies, fields = fr.scene(n_bodies, n_fields)
    assert fr.evaluate(fields, bodies["pos"])["margin"] > 1e-3


# ---- known answers by hand ----------------------------------------------------------------------------------------------
S2 = float(np.sqrt(0.5))
RZ = [0.0, 0.0, S2, S2]
# (label, field, body position, velocity, spin, mass, force, torque) - every expected value from the closed form, by hand
HAND = [
    ("accel box", dict(kind=fr.ACCEL, shape=fr.BOX, pos=[1, 1, 1], rot=None, he=[1, 2, 3], vec=[0, 9.81, 0.5], coef=[0, 0], ex=0),
     [1.5, 2.5, -1.0], [3, 0, 0], [0, 1, 0], 2.0, [0, 19.62, 1.0], [0, 0, 0]),
    ("accel rotated box: inside only because it is turned", dict(kind=fr.ACCEL, shape=fr.BOX, pos=[0, 0, 0], rot=RZ, he=[1, 2, 3], vec=[1, 2, 3], coef=[0, 0], ex=0),
     [1.5, 0, 0], [0, 0, 0], [0, 0, 0], 0.5, [0.5, 1.0, 1.5], [0, 0, 0]),
    ("accel rotated box: outside only because it is turned", dict(kind=fr.ACCEL, shape=fr.BOX, pos=[0, 0, 0], rot=RZ, he=[1, 2, 3], vec=[1, 2, 3], coef=[0, 0], ex=0),
     [0, 1.5, 0], [0, 0, 0], [0, 0, 0], 0.5, None, None),
    ("accel sphere", dict(kind=fr.ACCEL, shape=fr.SPHERE, pos=[0, 0, 0], rot=None, he=[2, 0, 0], vec=[0, 0, -4], coef=[0, 0], ex=0),
     [1, 1, 1], [0, 0, 0], [0, 0, 0], 3.0, [0, 0, -12.0], [0, 0, 0]),
    ("accel capsule: beside the core's end cap", dict(kind=fr.ACCEL, shape=fr.CAPSULE, pos=[0, 0, 0], rot=None, he=[0.5, 2, 0], vec=[2, 0, 0], coef=[0, 0], ex=0),
     [0.25, 2.25, 0], [0, 0, 0], [0, 0, 0], 1.5, [3.0, 0, 0], [0, 0, 0]),
    ("drag box with wind", dict(kind=fr.DRAG, shape=fr.BOX, pos=[0, 0, 0], rot=None, he=[4, 4, 4], vec=[1, 0, -2], coef=[0.5, 0.25], ex=0),
     [1, 2, 3], [3, -2, 0], [4, 0, -8], 7.0, [-1.0, 1.0, -1.0], [-1.0, 0, 2.0]),
    ("drag sphere, the closed boundary counts", dict(kind=fr.DRAG, shape=fr.SPHERE, pos=[0, 0, 0], rot=None, he=[2, 0, 0], vec=[0, 0, 0], coef=[2, 0], ex=0),
     [2, 0, 0], [1, 2, 4], [1, 1, 1], 1.0, [-2.0, -4.0, -8.0], [0, 0, 0]),
    ("drag capsule along world x", dict(kind=fr.DRAG, shape=fr.CAPSULE, pos=[0, 0, 0], rot=RZ, he=[0.5, 2, 0], vec=[0, 0, 0], coef=[0, 4], ex=0),
     [-2.25, 0, 0], [1, 1, 1], [0.5, 0, -1], 1.0, [0, 0, 0], [-2.0, 0, 4.0]),
    ("drag capsule along world x: not along y", dict(kind=fr.DRAG, shape=fr.CAPSULE, pos=[0, 0, 0], rot=RZ, he=[0.5, 2, 0], vec=[0, 0, 0], coef=[0, 4], ex=0),
     [0, 2.25, 0], [1, 1, 1], [0.5, 0, -1], 1.0, None, None),
    ("radial exponent 0, r > r0", dict(kind=fr.RADIAL, shape=fr.SPHERE, pos=[1, 0, 0], rot=None, he=[8, 0, 0], vec=[0, 0, 0], coef=[6, 1], ex=0),
     [1, 3, 4], [0, 0, 0], [0, 0, 0], 1.0, [0, 3.6, 4.8], [0, 0, 0]),
    ("radial exponent 1, r > r0", dict(kind=fr.RADIAL, shape=fr.SPHERE, pos=[1, 0, 0], rot=None, he=[8, 0, 0], vec=[0, 0, 0], coef=[6, 2.5], ex=1),
     [1, 3, 4], [0, 0, 0], [0, 0, 0], 1.0, [0, 1.8, 2.4], [0, 0, 0]),
    ("radial exponent 2, r > r0, attracting", dict(kind=fr.RADIAL, shape=fr.BOX, pos=[1, 0, 0], rot=None, he=[8, 8, 8], vec=[0, 0, 0], coef=[-8, 2.5], ex=2),
     [1, 3, 4], [0, 0, 0], [0, 0, 0], 1.0, [0, -1.2, -1.6], [0, 0, 0]),
    ("radial exponent 2, r < r0: the full strength", dict(kind=fr.RADIAL, shape=fr.SPHERE, pos=[0, 0, 0], rot=None, he=[8, 0, 0], vec=[0, 0, 0], coef=[5, 10], ex=2),
     [0, 0, -0.5], [0, 0, 0], [0, 0, 0], 1.0, [0, 0, -5.0], [0, 0, 0]),
    ("radial exponent 1, r < r0", dict(kind=fr.RADIAL, shape=fr.CAPSULE, pos=[0, 0, 0], rot=None, he=[1, 1, 0], vec=[0, 0, 0], coef=[5, 10], ex=1),
     [0.5, 0, 0], [0, 0, 0], [0, 0, 0], 1.0, [5.0, 0, 0], [0, 0, 0]),
    ("radial at the centre: nothing", dict(kind=fr.RADIAL, shape=fr.SPHERE, pos=[1, 2, 3], rot=None, he=[8, 0, 0], vec=[0, 0, 0], coef=[5, 1], ex=2),
     [1, 2, 3], [0, 0, 0], [0, 0, 0], 1.0, None, None),
]


def _hand_fields(f):
    return dict(kind=np.array([f["kind"]], np.uint32), shape=np.array([f["shape"]], np.uint32), pos=np.array([f["pos"]], np.float32),
                rot=None if f["rot"] is None else np.array([f["rot"]], np.float32), half_extent=np.array([f["he"]], np.float32), mask=None,
                vec=np.array([f["vec"]], np.float32), coef=np.array([f["coef"]], np.float32), exponent=np.array([f["ex"]], np.uint32))


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_known_answers_by_hand(case, probe, tmp_path):
    """One body at a stated point in one field; the starting accumulators are (1, 2, 3) and (-1, -2, -3), and a field that does
    not act leaves them as they are."""
    _, f, x, v, w, mass, F, T = case
    fields = _hand_fields(f)
    acc_f, acc_t = np.array([[1, 2, 3]], np.float32), np.array([[-1, -2, -3]], np.float32)
    want_f = acc_f[0] + (0 if F is None else np.array(F)), acc_t[0] + (0 if T is None else np.array(T))
    res = fr.evaluate(fields, [x], vel=[v], ang=[w], mass=[mass], force=acc_f, torque=acc_t)
    assert res["K"][0] == (F is not None)
    # (the reference reads the float32 inputs the library gets: 9.81 is not one)
    assert np.allclose(res["F"][0], want_f[0], rtol=0, atol=1e-6) and np.allclose(res["T"][0], want_f[1], rtol=0, atol=1e-6)
    scene = str(tmp_path / "scene.txt")
    fp.write_scene(scene, fields, [x], vel=[v], ang=[w], mass=np.array([mass], np.float32), force=acc_f, torque=acc_t)
    acted, got_f, got_t = fp.run(probe, scene)
    assert acted[0] == (F is not None)
    tol = fr.bound(res)[0]
    assert (np.abs(got_f[0] - want_f[0]) <= tol).all() and (np.abs(got_t[0] - want_f[1]) <= tol).all(), (got_f, got_t, want_f)
    if F is None:
        assert got_f.tobytes() == acc_f.tobytes() and got_t.tobytes() == acc_t.tobytes()


def test_masks_pick_the_reference_pairs():
    bodies, fields = fr.scene(65, 33)
    rng = np.random.default_rng(5)
    cat = (1 << rng.integers(0, 4, 65)).astype(np.uint16)
    fields["mask"] = rng.integers(0, 16, 33).astype(np.uint16)
    res = fr.evaluate(fields, bodies["pos"], category=cat)
    every = fr.evaluate(dict(fields, mask=None), bodies["pos"])
    assert res["pairs"] == {(k, i) for k, i in every["pairs"] if cat[i] & fields["mask"][k]} and 0 < len(res["pairs"]) < len(every["pairs"])


# ---- the library's arithmetic against float64, under the sanitizers ----------------------------------------------------------
def test_spec_against_float64_on_the_committed_scene(probe, probe_sanitized, tmp_path):
    """The probe on the committed scene (257 bodies, 70 fields), zero and nonzero starting accumulators, plain and masked:
    within (16 + K) * 2^-23 * S of the float64 reference per body and component, untouched bodies keep their bits, and the
    build under -fsanitize=address,undefined prints the same bits and reports nothing."""
    bodies, fields = fr.scene(257, 70)
    rng = np.random.default_rng(11)
    acc = rng.normal(size=(2, 257, 3)).astype(np.float32) * 5
    cat = (1 << rng.integers(0, 4, 257)).astype(np.uint16)
    masks = rng.integers(1, 16, 70).astype(np.uint16)
    worst = 0.0
    for label, f, t, masked in (("zero", None, None, False), ("nonzero", acc[0], acc[1], False), ("masked", acc[0], acc[1], True)):
        fl = dict(fields, mask=masks if masked else None)
        scene = str(tmp_path / f"scene_{label}.txt")
        fp.write_scene(scene, fl, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"], category=cat, force=f, torque=t)
        acted, got_f, got_t = fp.run(probe, scene)
        res = fr.evaluate(fl, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"], category=cat, force=f, torque=t)
        assert (acted == (res["K"] > 0)).all()
        tol = fr.bound(res)
        err = np.maximum(np.abs(got_f - res["F"]), np.abs(got_t - res["T"]))
        worst = max(worst, float((err[acted] / tol[acted]).max()))
        assert (err <= tol).all(), label
        start_f, start_t = (np.zeros((257, 3), np.float32) if f is None else f), (np.zeros((257, 3), np.float32) if t is None else t)
        assert got_f[~acted].tobytes() == start_f[~acted].tobytes() and got_t[~acted].tobytes() == start_t[~acted].tobytes()
        if label == "masked":
            san = fp.run(probe_sanitized, scene)
            assert san[0].tobytes() == acted.tobytes() and san[1].tobytes() == got_f.tobytes() and san[2].tobytes() == got_t.tobytes()
    print(f"worst error / bound: {worst:.3f}")
    r = subprocess.run([probe_sanitized, "--messages"], capture_output=True, text=True)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
