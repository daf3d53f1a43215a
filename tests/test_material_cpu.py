"""CPU: materials (include/physics_hip.h) without a GPU: the new symbols are declared, exported and
bound; argument errors of a NULL world; the Python layer's checks before the library is reached; the normative functions
of include/spec/contact_solve.h, compiled on the host, against exact identities and a hand-written table; the float64
statement of tests/material_ref.py against the same table and against tests/contact_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contact_ref as cr
import material_ref as mr
from physics_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["phys_set_body_materials", "phys_get_body_materials", "phys_set_static_materials", "phys_set_ground_material",
       "phys_set_restitution_threshold"]
DT = 1.0 / 60.0


def test_symbols_declared_exported_bound_and_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "physics_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    mirror = open(os.path.join(ROOT, "include", "physics_state.hpp")).read()
    lib = _abi.load_library()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert len(re.findall(rf"pub fn {n}\s*\(", rust)) == 1, n
        assert hasattr(lib, n) and n in _abi.PROTOTYPES, n
    for n in ("phys_set_body_materials", "phys_set_ground_material", "phys_set_restitution_threshold"):
        assert n in mirror, n
    assert lib.phys_abi_version() == 2 == _abi.PHYS_ABI_VERSION


def test_null_world_is_an_argument_error():
    lib = _abi.load_library()
    E = _abi.PHYS_ERR_INVALID_ARG
    f = (C.c_float * 4)()
    assert lib.phys_set_body_materials(None, 0, None, None) == E
    assert lib.phys_set_body_materials(None, 4, f, f) == E
    assert lib.phys_get_body_materials(None, f, f) == E
    assert lib.phys_set_static_materials(None, 0, None, None) == E
    assert lib.phys_set_ground_material(None, 0.5, 0.0) == E
    assert lib.phys_set_restitution_threshold(None, 1.0) == E
    assert b"null world" in lib.phys_last_error()


class _NoLib:
    """Stands in for the library: any call reaching it is a failure of the Python checks."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def _world(n=4, n_static=2):
    from physics_amd.world import World
    w = World.__new__(World)
    w.lib, w.h, w.n, w.n_static = _NoLib(), C.c_void_p(), n, n_static
    return w


@pytest.mark.parametrize("kw", [dict(friction=[0.1, 0.2, 0.3]), dict(restitution=np.zeros((4, 1))), dict(friction=[0.1, 0.2, 0.3, -0.1]),
                                dict(friction=[0.1, 0.2, 0.3, np.inf]), dict(friction=[0.1, np.nan, 0.3, 0.1]),
                                dict(restitution=[0, 0, 0, 1.5]), dict(restitution=[0, 0, 0, -0.1]), dict(restitution=[0, 0, np.nan, 0]),
                                dict(friction=["a", "b", "c", "d"])])
def test_python_rejects_bad_materials_before_the_library(kw):
    w = _world()
    with pytest.raises(ValueError):
        w.set_body_materials(**kw)
    with pytest.raises(ValueError):
        w.set_static_materials(**kw)  # two statics: every case is mis-shaped or out of range for them too


@pytest.mark.parametrize("args", [(-0.5, 0.0), (0.5, 1.5), (0.5, -0.1), (np.nan, 0.0), (np.inf, 0.0), (None, 0.0), (0.5, None), ([0.5, 0.5], 0.0)])
def test_python_rejects_bad_ground_material(args):
    with pytest.raises(ValueError):
        _world().set_ground_material(*args)


@pytest.mark.parametrize("v", [-1.0, np.nan, np.inf, None, [1.0, 2.0]])
def test_python_rejects_bad_threshold(v):
    with pytest.raises(ValueError):
        _world().set_restitution_threshold(v)


# ---- the normative functions of contact_solve.h, compiled on the host -------------------------------------------------------
SHIM = r"""
#include <stdint.h>
#include "spec/contact_solve.h"
extern "C" {
void combine_many(uint64_t n, const float* fa, const float* fb, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = material_friction(fa[i], fb[i]); }
float combine_e(float ea, float eb) { return material_restitution(ea, eb); }
float plain_bias(float depth, float dt, float baumgarte, float slop, float max_bias) {
    solve_params_t sp; sp.dt = dt; sp.baumgarte = baumgarte; sp.slop = slop; sp.friction = 0.5f; sp.max_bias = max_bias;
    return contact_bias(depth, &sp);
}
float bounce_bias(float depth, float vn, float e, float threshold, float dt, float baumgarte, float slop, float max_bias) {
    solve_params_t sp; sp.dt = dt; sp.baumgarte = baumgarte; sp.slop = slop; sp.friction = 0.5f; sp.max_bias = max_bias;
    return contact_bias_restitution(depth, vn, e, threshold, &sp);
}
float normal_velocity(const float* n, const float* vA, const float* wA, const float* rA, const float* vB, const float* wB, const float* rB) {
    return contact_normal_velocity(v3_make(n[0], n[1], n[2]), v3_make(vA[0], vA[1], vA[2]), v3_make(wA[0], wA[1], wA[2]),
                                   v3_make(rA[0], rA[1], rA[2]), v3_make(vB[0], vB[1], vB[2]), v3_make(wB[0], wB[1], wB[2]),
                                   v3_make(rB[0], rB[1], rB[2]));
}
}
"""


@pytest.fixture(scope="module")
def spec(tmp_path_factory):
    d = tmp_path_factory.mktemp("material_spec")
    src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libshim.so")
    open(src, "w").write(SHIM)
    # the oracle's flags (oracle/Makefile): fused multiply-add only where the header asks for it
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I",
                    os.path.join(ROOT, "include"), "-o", so, src, "-lm"], check=True)
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    lib.combine_many.argtypes = [C.c_uint64, fp, fp, fp]
    lib.combine_e.restype = C.c_float
    lib.combine_e.argtypes = [C.c_float] * 2
    lib.plain_bias.restype = C.c_float
    lib.plain_bias.argtypes = [C.c_float] * 5
    lib.bounce_bias.restype = C.c_float
    lib.bounce_bias.argtypes = [C.c_float] * 8
    lib.normal_velocity.restype = C.c_float
    lib.normal_velocity.argtypes = [fp] * 7
    return lib


def _combine(lib, fa, fb):
    fa = np.ascontiguousarray(fa, np.float32)
    fb = np.ascontiguousarray(fb, np.float32)
    out = np.empty_like(fa)
    fp = C.POINTER(C.c_float)
    lib.combine_many(len(fa), fa.ctypes.data_as(fp), fb.ctypes.data_as(fp), out.ctypes.data_as(fp))
    return out


def test_combining_a_friction_with_itself_is_exact(spec):
    """combine(f, f) == f bit for bit: 1e5 random finite floats of every exponent (denormals and values near FLT_MAX
    included), and the edge values themselves."""
    rng = np.random.default_rng(14)
    bits = rng.integers(0, 0x7F800000, 100000, dtype=np.uint32)  # every non-negative finite float is equally likely
    f = bits.view(np.float32)
    edge = np.array([0.0, 1e-45, 1.1754942e-38, 1.1754944e-38, 0.5, 1.0, 3.4028235e38], np.float32)
    f = np.concatenate([f, edge])
    assert (f.view(np.uint32) < 0x00800000).sum() > 100 and (f > 1e30).sum() > 100  # denormals and large values took part
    got = _combine(spec, f, f)
    assert np.array_equal(got.view(np.uint32), f.view(np.uint32))


def test_combined_friction_is_the_geometric_mean(spec):
    rng = np.random.default_rng(15)
    fa = rng.uniform(0.0, 2.0, 10000).astype(np.float32)
    fb = rng.uniform(0.0, 2.0, 10000).astype(np.float32)
    got = _combine(spec, fa, fb)
    want = mr.combine_friction(fa, fb)
    assert np.array_equal(got, want.astype(np.float32))  # the product is exact in double, the root correctly rounded
    assert np.array_equal(got, _combine(spec, fb, fa))
    assert _combine(spec, [0.0], [0.9])[0] == 0.0  # ice against anything is ice


P = dict(dt=DT, baumgarte=0.2, slop=0.01, max_bias=3.0)
# depth, vn, e, threshold -> bounces?, and the bias. contact_bias: 0 inside the slop, 12 (depth - 0.01) capped at 3 beyond
# it, depth * 60 for a speculative point.
TABLE = [
    (0.005, -0.5, 0.5, 1.0, False, 0.0),                  # below the threshold: resting contact
    (0.005, -1.0, 0.5, 1.0, False, 0.0),                  # at the threshold: not faster than it
    (0.005, -2.0, 0.5, 1.0, True, 1.0),                   # above: rebound e |vn|
    (0.005, -2.0, 0.5, 3.0, False, 0.0),                  # ... unless the threshold is raised
    (0.005, -0.5, 0.5, 0.0, True, 0.25),                  # threshold 0: every approach bounces
    (0.005, +2.0, 0.5, 1.0, False, 0.0),                  # separating
    (-0.01, -3.0, 0.5, 1.0, True, 1.5),                   # speculative, gap 0.01 < 3 / 60: closes, bounces
    (-0.06, -3.0, 0.5, 1.0, False, -0.06 * 60.0),         # speculative, gap 0.06 > 0.05: does not touch in this update
    (-0.05, -3.0, 0.5, 1.0, True, 1.5),                   # ... gap closed exactly
    (0.005, -2.0, 0.0, 1.0, False, 0.0),                  # e = 0
    (-0.01, -3.0, 0.0, 1.0, False, -0.01 * 60.0),         # e = 0, speculative
    (0.11, -1.5, 0.5, 1.0, True, 12.0 * 0.10),            # push-out 1.2 larger than the bounce 0.75
    (0.11, -4.0, 0.5, 1.0, True, 2.0),                    # bounce 2.0 larger than the push-out 1.2
    (0.50, -4.0, 0.5, 1.0, True, 3.0),                    # push-out at its cap 3 larger than the bounce 2
    (0.005, -2.0, 1.0, 1.0, True, 2.0),                   # fully elastic
]


def test_bias_rule_matches_the_hand_table(spec):
    p = cr.Params(DT)
    for depth, vn, e, thr, bounces, want in TABLE:
        got = spec.bounce_bias(depth, vn, e, thr, P["dt"], P["baumgarte"], P["slop"], P["max_bias"])
        assert got == pytest.approx(want, rel=1e-6, abs=1e-7), (depth, vn, e, thr, got, want)
        plain = spec.plain_bias(depth, P["dt"], P["baumgarte"], P["slop"], P["max_bias"])
        if not bounces or e == 0.0:
            assert np.float32(got).tobytes() == np.float32(plain).tobytes()  # the plain function's bits
        # the float64 statement says the same
        push, rebound = mr.pushout_and_rebound(depth, vn, e, thr, p)
        assert bool(np.isfinite(rebound)) == bounces, (depth, vn, e, thr)
        assert float(mr.restitution_bias(depth, vn, e, thr, p)) == pytest.approx(want, rel=1e-9, abs=1e-12)
        assert float(push) == pytest.approx(plain, rel=1e-6, abs=1e-7)


def test_restitution_is_the_larger_one_and_zero_restitution_never_moves_the_bias(spec):
    assert spec.combine_e(0.25, 0.75) == 0.75 and spec.combine_e(0.75, 0.25) == 0.75 and spec.combine_e(0.0, 0.0) == 0.0
    assert mr.combine_restitution(0.2, 0.8) == 0.8
    rng = np.random.default_rng(16)
    for depth, vn in zip(rng.uniform(-0.1, 0.3, 2000), rng.uniform(-10, 10, 2000)):
        a = spec.bounce_bias(depth, vn, 0.0, 1.0, P["dt"], P["baumgarte"], P["slop"], P["max_bias"])
        b = spec.plain_bias(depth, P["dt"], P["baumgarte"], P["slop"], P["max_bias"])
        assert np.float32(a).tobytes() == np.float32(b).tobytes()


def test_normal_velocity_matches_float64(spec):
    rng = np.random.default_rng(17)
    fp = C.POINTER(C.c_float)
    for _ in range(500):
        v = rng.normal(size=(7, 3)).astype(np.float32)
        v[0] /= np.linalg.norm(v[0])
        got = spec.normal_velocity(*[np.ascontiguousarray(x).ctypes.data_as(fp) for x in v])
        want = mr.normal_velocity(*v.astype(np.float64))
        assert got == pytest.approx(float(want), abs=2e-5)
    z = np.zeros(3, np.float32)
    n = np.array([0, -1, 0], np.float32)
    vA = np.array([0.3, -3, 0.1], np.float32)
    assert spec.normal_velocity(*[x.ctypes.data_as(fp) for x in (n, vA, z, z, z, z, z)]) == -3.0  # falling onto a resting B


# ---- the float64 reference --------------------------------------------------------------------------------------------------
def test_manifold_materials_pick_the_right_side():
    m = mr.Materials([0.4, 0.9, 0.1], [0.0, 0.5, 0.2], static_friction=[1.6, 0.0], static_restitution=[0.9, 0.0], ground=(0.25, 0.3))
    a = np.array([0, 0, 1, 2, 2])
    b = np.array([1, cr.GROUND, mr.STATIC_ID_BIT | 0, mr.STATIC_ID_BIT | 1, cr.GROUND])
    mu, e = m.of_manifolds(a, b)
    assert mu == pytest.approx([0.6, np.sqrt(0.1), 1.2, 0.0, np.sqrt(0.025)])
    assert e.tolist() == [0.5, 0.3, 0.9, 0.2, 0.3]


def test_reference_with_default_materials_is_the_contact_reference():
    """material_ref.solve with one friction everywhere and no restitution reproduces tests/contact_ref.py exactly, over
    warm-started updates of the friction pairs (positions advanced by the reference's own velocities)."""
    bodies = cr.friction_pairs(3, 6)
    n = len(bodies["pos"])
    inv_m, inv_I = cr.body_inverses(n, bodies["mass"], bodies["inertia"])
    p = cr.Params(DT, friction=0.35)
    plain, mat = cr.SolverRef(n, p, 8), mr.MaterialSolverRef(n, p, 8)
    mats = mr.Materials(np.full(n, 0.35), np.zeros(n), ground=(0.35, 0.0))
    # hand-made manifolds: every upper body of a group against its lower one, one point, and every fifth against the ground
    ids, counts, normals, points = [], [], [], []
    for g in range(6):
        for a, b in ((5 * g, 5 * g + 1), (5 * g + 2, 5 * g + 3), (5 * g + 4, cr.GROUND)):
            ids.append((a, b))
            counts.append(2)
            normals.append((0.0, 1.0 if b != cr.GROUND else -1.0, 0.0))
            base = bodies["pos"][a].astype(np.float64) + (0, 0.6 if b != cr.GROUND else -0.6, 0)
            points.append([list(base + (0.3, 0, 0.1)) + [0.03], list(base + (-0.3, 0, -0.2)) + [-0.004], [0] * 4, [0] * 4])
    man = (np.array(ids, np.uint32), np.array(counts, np.uint32), np.array(normals, np.float32), np.array(points, np.float32))
    lin, ang = bodies["lin_vel"].astype(np.float64), bodies["ang_vel"].astype(np.float64)
    for _ in range(3):
        o1 = plain.update(man, bodies["pos"], lin, ang, inv_m, inv_I, np.array([0.0, -9.81, 0.0]))
        o2 = mat.update(man, bodies["pos"], lin, ang, inv_m, inv_I, np.array([0.0, -9.81, 0.0]), materials=mats)
        assert np.array_equal(o1["lin"], o2["lin"]) and np.array_equal(o1["ang"], o2["ang"]) and np.array_equal(o1["impulses"], o2["impulses"])
        lin, ang = o1["lin"], o1["ang"]
    assert np.abs(o1["impulses"]).max() > 0.1
