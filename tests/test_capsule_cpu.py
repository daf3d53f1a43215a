"""CPU: the capsule shape on every surface (C header, Python, Rust shim, C++ host mirror), static capsules accepted and
invalid ones refused before any device is touched, and the spec's capsule contacts (through the oracle) against the
float64 reference of capsule_ref on random pairs.

What this file leaves out - pairs without a contact, cores inside the box, near-parallel capsules, the swapped index
order, static partners, the second point on a face - is covered by tests/shape_pair_ref.py: tests/test_shape_pairs_cpu.py
runs its checks through the oracle, tests/test_gpu_shape_pairs.py on the GPU's own manifolds."""
import os
import re

import numpy as np

import capsule_ref as cref
import physics_amd
from physics_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 0.02


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_constant_is_on_every_surface():
    assert re.search(r"#define PHYS_SHAPE_CAPSULE 3u", _read("include", "physics_hip.h"))
    assert re.search(r"#define PHYS_SPEC_SHAPE_CAPSULE 3u", _read("include", "spec", "collide.h"))
    assert _abi.SHAPE_CAPSULE == 3 and physics_amd.SHAPE_CAPSULE == 3 and "SHAPE_CAPSULE" in physics_amd.__all__
    assert re.search(r"pub const PHYS_SHAPE_CAPSULE: u32 = 3;", _read("rust", "physics_hip_sys", "src", "lib.rs"))
    assert "PHYS_SHAPE_CAPSULE" in _read("include", "physics_state.hpp")
    # the ABI version stays: the change is additive
    assert re.search(r"#define PHYS_ABI_VERSION 2u", _read("include", "physics_hip.h"))


def test_capsule_inertia_of_the_limits():
    # h = 0: a solid sphere; r -> 0: a thin rod of length 2h about its middle
    assert np.allclose(physics_amd.capsule_inertia(2.0, 0.5, 0.0), np.eye(3) * 0.4 * 2.0 * 0.25)
    rod = physics_amd.capsule_inertia(3.0, 1e-6, 2.0)
    assert np.allclose(np.diag(rod), [3.0 * 16 / 12, 0.0, 3.0 * 16 / 12], atol=1e-5)


def _static_call(shape, he):
    """phys_set_static_bodies on a NULL world: the arguments are checked before the world is looked at"""
    lib = _abi.load_library()
    pos = np.zeros((1, 3), np.float32)
    st = np.uint32([shape])
    h = np.ascontiguousarray(np.float32(he).reshape(1, 3))
    rc = lib.phys_set_static_bodies(None, 1, pos.ctypes.data_as(_abi.f32p), None, st.ctypes.data_as(_abi.u32p),
                                    h.ctypes.data_as(_abi.f32p))
    return rc, lib.phys_last_error().decode()


def test_static_capsules_are_accepted_and_invalid_ones_refused_without_a_device():
    rc, msg = _static_call(_abi.SHAPE_CAPSULE, [0.3, 2.0, 0.0])
    assert rc == _abi.PHYS_ERR_INVALID_ARG and msg == "null world"  # accepted: only the missing world is left
    rc, msg = _static_call(_abi.SHAPE_CAPSULE, [0.3, 0.0, 0.0])    # h = 0
    assert msg == "null world"
    for he, want in (([-0.3, 2.0, 0.0], "negative half extent"), ([0.3, -1.0, 0.0], "negative half extent"),
                     ([np.nan, 1.0, 0.0], "non-finite"), ([0.3, np.inf, 0.0], "non-finite")):
        rc, msg = _static_call(_abi.SHAPE_CAPSULE, he)
        assert rc == _abi.PHYS_ERR_INVALID_ARG and want in msg, (he, msg)
    rc, msg = _static_call(4, [0.3, 2.0, 0.0])
    assert rc == _abi.PHYS_ERR_INVALID_ARG and "neither SPHERE nor BOX nor CAPSULE" in msg


# ---- the spec against the float64 reference -----------------------------------------------------------------------
def _rand_quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(np.float32)


def _oracle_manifold(A, B, ground=False):
    """(normal, [(point, depth)]) of the pair A, B (or of A on the ground) from the oracle, or None"""
    from oracle import binding as ob
    flags = physics_amd.FLAG_COLLISIONS | (physics_amd.FLAG_GROUND_PLANE if ground else 0)
    w = ob.OracleWorld(physics_amd.default_config(flags=flags, gravity_offset=(0, 0, 0), contact_margin=MARGIN), trig=ob.TRIG_DET)
    bodies = [A] if ground else [A, B]
    w.set_bodies(np.float32([b[0] for b in bodies]), rot=np.float32([b[1] for b in bodies]),
                 shape_type=np.uint32([b[3] for b in bodies]), half_extent=np.float32([b[2] for b in bodies]))
    w.collide_now()
    ids, counts, normals, points = w.get_manifolds()
    w.close()
    if len(ids) == 0:
        return None
    assert len(ids) == 1
    return normals[0].astype(np.float64), [(points[0, k, :3].astype(np.float64), float(points[0, k, 3])) for k in range(counts[0])]


def _capsule(rng):
    return (rng.uniform(-1, 1, 3).astype(np.float32), _rand_quat(rng),
            np.float32([rng.uniform(0.2, 0.8), rng.uniform(0.0, 1.2), 0.0]), physics_amd.SHAPE_CAPSULE)


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if got is None:
        return
    assert np.allclose(got[0], want[0], atol=1e-4), (what, got[0], want[0])
    assert len(got[1]) == len(want[1]), what
    for (pg, dg), (pw, dw) in zip(sorted(got[1], key=lambda x: tuple(x[0])), sorted(want[1], key=lambda x: tuple(x[0]))):
        assert abs(dg - dw) < 1e-4 and np.allclose(pg, pw, atol=1e-4), (what, pg, pw, dg, dw)


def test_ground_sphere_and_capsule_contacts_match_float64():
    rng = np.random.default_rng(1)
    checked = 0
    for k in range(300):
        A = _capsule(rng)
        kind = k % 3
        if kind == 0:  # ground: skip ends within 1e-3 of the margin
            A = (A[0] + np.float32([0, rng.uniform(0.0, 1.5), 0]), A[1], A[2], A[3])
            c, u, hl, r = cref.segment(A[0], A[1], A[2])
            if min(abs(-(p[1] - r) + MARGIN) for p in (c - hl * u, c + hl * u)) < 1e-3:
                continue
            want = cref.ground(A[0], A[1], A[2], 0.0, MARGIN)
            want = (np.array([0.0, -1.0, 0.0]), want) if want else None
            _same(_oracle_manifold(A, None, ground=True), want, ("ground", k))
        elif kind == 1:  # sphere
            B = (rng.uniform(-1, 1, 3).astype(np.float32) * 1.5, np.float32([0, 0, 0, 1]),
                 np.float32([rng.uniform(0.2, 0.8)] * 3), physics_amd.SHAPE_SPHERE)
            want = cref.capsule_sphere(A[:3], B[:3], MARGIN)
            if want is not None and abs(want[1][0][1] + MARGIN) < 1e-3:
                continue
            _same(_oracle_manifold(A, B), want, ("sphere", k))
        else:  # capsule: clear of the parallel threshold and of the margin
            B = _capsule(rng)
            B = (B[0] * 1.5, B[1], B[2], B[3])
            ua, ub = cref.segment(*A[:3])[1], cref.segment(*B[:3])[1]
            if abs(1.0 - (ua @ ub) ** 2 - 1e-4) < 1e-5:
                continue
            want = cref.capsule_capsule(A[:3], B[:3], MARGIN)
            if want is not None and min(abs(d + MARGIN) for _, d in want[1]) < 1e-3:
                continue
            _same(_oracle_manifold(A, B), want, ("capsule", k))
        checked += 1
    assert checked > 250


def test_capsule_box_depth_matches_the_exact_distance():
    """Capsule-box pairs whose core is outside the box, within the margin or touching: the deepest point of the spec's
    manifold has the depth of the exact segment-box distance (float64, by minimisation), and the manifold's normal is
    the direction of that distance."""
    rng = np.random.default_rng(2)
    checked = 0
    for k in range(600):
        A = _capsule(rng)
        B = (rng.uniform(-1, 1, 3).astype(np.float32) * 2.0, _rand_quat(rng), rng.uniform(0.3, 1.0, 3).astype(np.float32),
             physics_amd.SHAPE_BOX)
        want = cref.capsule_box(A[:3], B[:3], MARGIN)
        if want is None or want[1] < -MARGIN + 1e-3:
            continue  # no contact, or within rounding of the margin
        got = _oracle_manifold(A, B)
        assert got is not None, k
        deepest = max(d for _, d in got[1])
        assert abs(deepest - want[1]) < 1e-4, (k, deepest, want[1])
        assert np.allclose(got[0], want[0], atol=1e-3), (k, got[0], want[0])
        checked += 1
    assert checked > 80
