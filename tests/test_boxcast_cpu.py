"""CPU: the box cast without a device. The float64 brute force (tests/boxcast_ref.py) checks itself; the seeded inputs of the
GPU tests (tests/boxcast_cases.py) stay within half the cap of near ties, and their stored answers answer the inputs of today;
the host probe (tests/cpp/boxcast_probe.cpp over include/spec/box_cast.h: what the kernel runs) is held to the reference on the
hand scene, a soup and the degenerate sets, once under the address and undefined-behaviour sanitizers; the argument checks of
the four entry points."""
import subprocess

import numpy as np
import pytest

import boxcast_accept as acc
import boxcast_cases as cases
import boxcast_probe as probe
import boxcast_ref as ref
import query_ref
from query_accept import cast_cap
from raycast_ref import rotation_matrices


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("boxcast") / "boxcast_probe"))


# ---- the reference's own distance of two boxes ---------------------------------------------------------------------------------
def _golden(f, lo, hi, iters=34):
    g = (np.sqrt(5.0) - 1.0) / 2.0
    a, b = lo.copy(), hi.copy()
    for _ in range(iters):
        m1, m2 = b - g * (b - a), a + g * (b - a)
        left = f(m1) <= f(m2)
        b = np.where(left, m2, b)
        a = np.where(left, a, m1)
    return f(0.5 * (a + b))


def test_box_box_distance_against_nested_golden_sections():
    """200 pairs, aligned, edge-parallel and containing ones among them: the least distance of a point of box a to box b (exact:
    a clamp in b's frame, convex over a's solid) found by three nested golden sections over a's coordinates"""
    rng = np.random.default_rng(41)
    n = 200
    qa, qb = cases.quats(rng, n).astype(np.float64), cases.quats(rng, n).astype(np.float64)
    ha, hb = rng.uniform(0.1, 1.5, (n, 3)), rng.uniform(0.1, 1.5, (n, 3))
    ca, cb = rng.uniform(-2.5, 2.5, (n, 3)), rng.uniform(-2.5, 2.5, (n, 3))
    qb[:30] = qa[:30]                                                  # aligned: every cross axis vanishes
    for k in range(30, 60):                                            # one shared axis: edge-parallel
        qb[k] = cases._qmul(qa[k], cases._turn([[1, 0, 0], [0, 1, 0], [0, 0, 1]][k % 3], rng.uniform(0.2, 1.3)))
    cb[60:80] = ca[60:80] + rng.uniform(-0.05, 0.05, (20, 3))          # containing: a small box inside a large one
    ha[60:70], hb[60:70] = rng.uniform(1.0, 1.5, (10, 3)), rng.uniform(0.05, 0.2, (10, 3))
    ha[70:80], hb[70:80] = rng.uniform(0.05, 0.2, (10, 3)), rng.uniform(1.0, 1.5, (10, 3))
    ha[80:90, 0] = 0.0                                                 # plates and rods
    hb[90:100, 1:] = 0.0
    Ra, Rb = rotation_matrices(qa), rotation_matrices(qb)
    q, p, d = ref.box_box_closest(ca, Ra, ha, cb, Rb, hb)

    def dist(x, y, z):
        pt = ca + np.einsum("pjk,pk->pj", Ra, np.column_stack([x, y, z]))
        l = np.einsum("pj,pjk->pk", pt - cb, Rb)
        return np.linalg.norm(l - np.clip(l, -hb, hb), axis=1)

    lo, hi = -ha, ha
    want = _golden(lambda x: _golden(lambda y: _golden(lambda z: dist(x, y, z), lo[:, 2], hi[:, 2]), lo[:, 1], hi[:, 1]), lo[:, 0], hi[:, 0])
    assert (d[60:80] == 0).all() and (d > 0).sum() > 100
    assert np.abs(d - want).max() <= 1e-5, np.abs(d - want).max()
    # the pair it returns lies on the two boxes and is that far apart
    la, lb = np.einsum("pj,pjk->pk", q - ca, Ra), np.einsum("pj,pjk->pk", p - cb, Rb)
    assert (np.abs(la) <= ha + 1e-9).all() and (np.abs(lb) <= hb + 1e-9).all()
    assert np.abs(np.linalg.norm(q - p, axis=1) - d).max() <= 1e-9


# ---- the seeded inputs ---------------------------------------------------------------------------------------------------------
def test_near_ties_of_every_seeded_input_stay_within_half_the_cap():
    for c in cases.all_cases():
        h = c["h"]
        n = len(h["t"])
        ties = acc.near_ties(h)
        print(c["label"], n, "casts", int((h["body"] != 0xFFFFFFFE).sum()), "hits", int((h["t"] == 0).sum()), "start touching,", ties, "near ties")
        assert 2 * ties <= cast_cap(n), (c["label"], ties)


def test_stored_answers_answer_todays_inputs_and_one_is_recomputed():
    stored = list(cases.stored_cases())
    assert len(stored) >= 13 and all(c["stored"] for c in stored), [c["label"] for c in stored if not c["stored"]]
    c = cases.filter_case()[3][1][1]  # the casts of mask 1
    h = ref.boxcast(c["o"], c["d"], c["rot"], c["he"], c["tg"], ground=c["ground"])
    assert np.array_equal(h["body"], c["h"]["body"]) and np.array_equal(h["which"], c["h"]["which"])
    # (1e-12: the same float64 arithmetic, but another numpy or libm may round a sine or a reduction differently)
    for k in ("t", "t2", "normal", "point"):
        assert np.array_equal(np.isfinite(h[k]), np.isfinite(c["h"][k])), k
        fin = np.isfinite(h[k])
        assert np.abs(h[k][fin] - c["h"][k][fin]).max() <= 1e-12, k


# ---- the host probe: what the kernel runs, against the reference ----------------------------------------------------------------
def test_probe_hand_scene(exe, tmp_path):
    bodies, casts = cases.hand_scene()
    tg = query_ref.targets({k: np.asarray(v, np.float32) for k, v in bodies.items()})
    f = np.float32
    case = dict(tg=tg, o=np.array([c["o"] for c in casts], f), d=np.array([c["d"] for c in casts], f), rot=np.array([c["rot"] for c in casts], f),
                he=np.array([c["he"] for c in casts], f), ground=0.0, max_t=None, ignore=None)
    body, t, nrm, pnt = probe.evaluate(exe, tmp_path, case)
    for i, c in enumerate(casts):
        assert body[i] == c["body"], (c["name"], body[i])
        assert abs(t[i] - c["t"]) <= 1e-5, (c["name"], t[i])
        assert np.abs(nrm[i] - c["normal"]).max() <= 1e-5, (c["name"], nrm[i])
        for a in range(3):
            if c["point"][a] is not None:
                assert abs(pnt[i][a] - c["point"][a]) <= 1e-5, (c["name"], pnt[i])
        for a, lo, hi in cases.FREE_RANGE.get(c["name"], []):
            assert lo - 1e-5 <= pnt[i][a] <= hi + 1e-5, (c["name"], pnt[i])


def test_probe_soup(exe, tmp_path):
    c = cases.soup(1)
    acc.compare_boxcasts(c["h"], probe.evaluate(exe, tmp_path, c), label=c["label"])


@pytest.mark.parametrize("name", cases.DEGENERATE)
def test_probe_degenerate_sets(name, exe, tmp_path):
    c = cases.degenerate(name)
    body = probe.evaluate(exe, tmp_path, c)
    acc.compare_boxcasts(c["h"], body, label=name)
    assert (body[0] < len(c["bodies"]["pos"])).sum() > 30


def test_probe_under_sanitizers(exe, tmp_path):
    """the stand-alone probe built with -fsanitize=address,undefined runs a soup clean and prints what the plain build prints"""
    san = probe.build(str(tmp_path / "boxcast_probe_san"), sanitize=True)
    c = cases.soup(2)
    a, b = probe.evaluate(exe, tmp_path, c), probe.evaluate(san, tmp_path, c)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    acc.compare_boxcasts(c["h"], b, label="soup 2 under sanitizers")


# ---- the entry points' argument checks -----------------------------------------------------------------------------------------
def test_argument_checks_of_the_entry_points(exe):
    r = subprocess.run([exe, "--args"], capture_output=True, text=True)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr


def test_entry_points_are_declared_everywhere():
    """The box cast's declarations stand in files of their own (include/physics_hip.h says why, beside the call's description): this test holds them to
    one another as tests/test_abi.py holds those of include/physics_hip.h - the header's symbols are the library's exports, the
    ctypes prototypes and the Rust declarations, each with the header's argument count and types."""
    import ctypes as C
    import os
    import re
    from physics_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "physics_hip.h")).read()
    assert '#include "physics_hip_boxcast.h"' in main  # every caller of physics_hip.h has them
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "physics_hip_boxcast.h")).read(), flags=re.S)
    rust = open(os.path.join(root, "rust", "physics_hip_sys", "src", "boxcast.rs")).read()
    assert "mod boxcast;" in open(os.path.join(root, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    names = ["phys_boxcast", "phys_boxcast_device", "phys_boxcast_device_filtered", "phys_boxcast_filtered"]
    assert sorted(set(re.findall(r"\b(phys_[a-z0-9_]+)\s*\(", header))) == names
    assert sorted(re.findall(r"pub fn (phys_[a-z0-9_]+)\s*\(", rust)) == names
    assert sorted(_abi.BOXCAST_PROTOTYPES) == names and not set(names) & set(_abi.PROTOTYPES)
    lib = _abi.load_library()
    c_types = {"phys_world*": C.c_void_p, "uint64_t": C.c_uint64, "const float*": _abi.f32p, "float*": _abi.f32p,
               "const uint32_t*": _abi.u32p, "uint32_t*": _abi.u32p, "const uint16_t*": _abi.u16p}
    rust_types = {"*mut phys_world": C.c_void_p, "u64": C.c_uint64, "*const f32": _abi.f32p, "*mut f32": _abi.f32p,
                  "*const u32": _abi.u32p, "*mut u32": _abi.u32p, "*const u16": _abi.u16p}
    for name in names:
        assert hasattr(lib, name), f"{name} declared but not exported"
        res, args = _abi.BOXCAST_PROTOTYPES[name]
        assert res is C.c_int32 and len(args) == (13 if "filtered" in name else 12)
        c_args = re.search(rf"int32_t {name}\((.*?)\);", header, flags=re.S).group(1).split(",")
        r_args = re.search(rf"pub fn {name}\s*\((.*?)\) -> i32;", rust, flags=re.S).group(1).split(",")
        assert len(c_args) == len(r_args) == len(args), name
        for k, (c, r, a) in enumerate(zip(c_args, r_args, args)):
            ct = c_types[" ".join(c.split()[:-1])]
            rt = rust_types[r.split(":", 1)[1].strip()]
            assert ct is rt and c.split()[-1] == r.split(":")[0].strip(), (name, k, c, r)
            assert a is (C.c_void_p if "device" in name and k >= 2 else ct), (name, k)  # device arrays travel as void pointers
    import physics_amd
    assert all(hasattr(physics_amd.World, k) for k in ("boxcast", "boxcast_device"))
    from physics_amd.state import PhysicsState
    assert hasattr(PhysicsState, "boxcast")
