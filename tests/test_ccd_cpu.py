"""CPU: continuous collision's rule (include/spec/ccd.h) as the host probe runs it (tests/cpp/ccd_probe.cpp, the functions the
kernel calls) against the float64 reference (tests/ccd_ref.py) over the committed cases (tests/ccd_cases.py), the staging of the
list (setup.hpp stage_ccd), and the mirrors of the new calls.

Acceptance of t and the normal: the box cast's own (tests/boxcast_accept.py), since it is the box cast's arithmetic:
  t       within tol = 1e-5 (1 + |x|_inf + |he| + t), he the mover's core half extents each grown by its radius
  normal  within 1e-4 of the reference's; grazing contacts (|n . u| < 0.1) are counted, not failed
  target  another target (or a hit against a miss) only where the float64 reference itself says the decision lies within tol:
          a second hit within 4 tol of the first, a hit within tol of L, a start within tol of touching, a pass within tol of
          the target. These are counted with the grazing normals and capped at 2 % of a case (CAP): no committed case of
          situations may have one, a soup of 96 bodies at most one.
The ground with a radius and the exchanged roles (a round mover at a box static) need no bound of their own: MEASURED below is
the largest |t - t_ref| / tol measured over the committed cases, every kind of pair included;
test_the_probe_meets_the_reference prints the current figure and holds it to four times that and to 1."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boxcast_accept as accept
import ccd_cases
import ccd_probe
import ccd_ref as ref
from raycast_ref import GROUND, MISS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.02  # of a case's bodies: decisions the float64 reference itself puts within tol
MEASURED = 0.0074  # largest |t - t_ref| / tol over the committed cases (see the docstring); the rule's bound is 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return ccd_probe.build(str(tmp_path_factory.mktemp("ccd") / "ccd_probe"))


def _tol_view(case, h):
    """the reference's answer under the names boxcast_accept.tol_of reads"""
    bd = case["bodies"]
    he = np.zeros((len(bd["pos"]), 3))
    for i in range(len(he)):
        hc, rho = ref.mover(int(bd["shape"][i]), bd["half_extent"][i]) if int(bd["shape"][i]) != ref.SHAPE_NONE else (np.zeros(3), 0.0)
        he[i] = hc + rho
    return dict(t=h["t"], o=np.asarray(bd["pos"], np.float64), he=he, valid=h["swept"] & np.isfinite(np.asarray(bd["pos"], np.float64)).all(1))


def compare(case, out):
    """out: (frac, target, normal, pos, rot) of the probe. Returns (odd cases, largest |t - t_ref| / tol)."""
    h = case["h"]
    frac, target, nrm = out[0], out[1], out[2]
    view = _tol_view(case, h)
    n = len(frac)
    bad, odd, worst = [], [], 0.0
    for i in range(n):
        rt, rid, gid = float(h["t"][i]), int(h["target"][i]), int(target[i])
        L = float(h["L"][i])
        gt = float(frac[i]) * L if gid != MISS else np.inf
        tol = accept.tol_of(view, i, gt)
        if gid == MISS and not (frac[i] == np.float32(1.0) and not nrm[i].any()):
            bad.append((i, "miss with frac / normal", float(frac[i]), nrm[i]))
            continue
        if gid == rid:
            if rid == MISS:
                continue
            worst = max(worst, abs(gt - rt) / tol)
            if abs(gt - rt) > tol:
                bad.append((i, "t", gid, gt, rt, tol))
            elif np.abs(nrm[i] - h["normal"][i]).max() > 1e-4:
                if abs(float(h["normal"][i] @ h["u"][i])) < 0.1:
                    odd.append((i, "grazing normal"))
                else:
                    bad.append((i, "normal", nrm[i], h["normal"][i]))
            continue
        # another answer: only where the reference itself cannot tell
        if rid != MISS and gid != MISS and h["t2"][i] - rt <= 4 * tol and abs(gt - rt) <= 4 * tol:
            odd.append((i, "tie", gid, rid))
        elif rid != MISS and gid == MISS and L - rt <= tol:
            odd.append((i, "hit at L", rt, L))
        elif rid == MISS and gid != MISS and (h["sep_min"][i] <= tol or abs(gt - L) <= tol):
            odd.append((i, "graze", gid, gt))
        elif 0 < abs(h["sep0"][i]) <= tol:  # (exactly 0: two boxes that overlap, however deep)
            odd.append((i, "touching start", h["sep0"][i]))
        else:
            bad.append((i, "target", hex(gid), gt, hex(rid), rt, L))
    assert not bad, f"{case['label']}: {len(bad)} of {n}: {bad[:6]}"
    assert len(odd) <= int(CAP * n), f"{case['label']}: {len(odd)} decisions too close to call of {n}: {odd[:8]}"
    return odd, worst


def test_the_probe_meets_the_reference(probe, tmp_path):
    worst, odd_total, hits = 0.0, 0, 0
    for case in ccd_cases.cases():
        out = ccd_probe.evaluate(probe, tmp_path, case)
        odd, w = compare(case, out)
        worst, odd_total = max(worst, w), odd_total + len(odd)
        hits += int((case["h"]["target"] != MISS).sum())
    print(f"largest |t - t_ref| / tol over {len(ccd_cases.cases())} cases, {hits} hits: {worst:.4f} (written down: {MEASURED}); "
          f"too close to call: {odd_total}")
    assert worst <= 1.0
    assert worst <= 4 * MEASURED, "the figure in this file's head is out of date"


def test_every_situation_comes_to_what_it_is_there_for():
    """by the float64 reference alone: the committed situations are what their names say"""
    seen = set()
    for case in ccd_cases.cases():
        if case["expect"] is None:
            continue
        h = case["h"]
        for i, want in enumerate(case["expect"]):
            got = int(h["target"][i])
            if want == "miss":
                assert got == MISS and h["frac"][i] == 1.0, (case["label"], ccd_cases.SITUATIONS[i], hex(got))
            elif want in ("solid", "front"):
                assert got == case["ids"][want], (case["label"], ccd_cases.SITUATIONS[i], hex(got))
                assert 0 < h["t"][i] < h["L"][i]
            seen.add(want)
        if case["ground"] is None:
            # the twin at the same pose gives the same t: the lower id won; the start inside the margin is inside it; the
            # penetrating start really penetrates; the front static really lies in front
            assert h["t2"][0] == h["t"][0]
            assert 0 < h["t"][4] < ccd_cases.MARGIN and h["sep0"][5] <= 0  # (two boxes that overlap are 0 apart, not less)
            assert h["t"][6] < h["t"][0]
        else:
            assert 0 < h["t"][4] < 2 * ccd_cases.MARGIN and h["sep0"][5] < -1e-3  # (along its slanted path: 0.01 / |u.y|)
    assert seen == {"miss", "solid", "front", "any"} or seen == {"miss", "solid", "front"}


def test_the_reference_keeps_clear_of_its_own_close_calls():
    """the cap of 2 % holds by the reference alone: its near ties (other than the exact twins), hits near L and starts near
    touching, counted with the acceptance's own tol"""
    for case in ccd_cases.cases():
        h = case["h"]
        view = _tol_view(case, h)
        close = 0
        for i in range(len(h["t"])):
            if not h["swept"][i]:
                continue
            tol = accept.tol_of(view, i, float(h["L"][i]))
            tie = np.isfinite(h["t2"][i]) and 0 < h["t2"][i] - h["t"][i] <= 4 * tol
            close += bool(tie or abs(h["L"][i] - h["t"][i]) <= tol or 0 < abs(h["sep0"][i]) <= tol or abs(h["sep_min"][i]) <= tol)
        assert close <= int(CAP * len(h["t"])), (case["label"], close)


def test_unswept_bodies_move_by_the_plain_step(probe, tmp_path):
    """frac is 1.0f exactly for a body that hits nothing, and dt * 1.0f == dt: the pose the probe prints is the plain step's"""
    case = ccd_cases.cases()[0]
    far = dict(case, statics={k: v[:0] for k, v in case["statics"].items()})
    a = ccd_probe.evaluate(probe, tmp_path, far)
    assert (a[0] == np.float32(1.0)).all() and (a[1] == MISS).all() and not a[2].any()
    bd = case["bodies"]
    dt = np.float32(case["dt"])
    want = (bd["pos"] + bd["lin"] * dt).astype(np.float32)
    fin = np.isfinite(want).all(1)
    assert np.array_equal(a[3][fin], want[fin])


def test_the_probe_under_the_sanitizers(tmp_path):
    """a stand-alone -fsanitize=address,undefined build of the probe over every committed case and the staging"""
    exe = ccd_probe.build(str(tmp_path / "ccd_probe_san"), sanitize=True)
    for case in ccd_cases.cases():
        ccd_probe.evaluate(exe, tmp_path, case)
    assert ccd_probe.staging(exe, 8, [5, 0, 7])[0] == 0
    assert ccd_probe.staging(exe, 8, [5, 5])[0] != 0


def test_staging(probe):
    from physics_amd import _abi
    code, ids, msg, null_code, big_code = ccd_probe.staging(probe, 10, [7, 2, 9, 0])
    assert (code, ids) == (0, [7, 2, 9, 0])                      # the order is kept
    assert (null_code, big_code) == (_abi.PHYS_ERR_INVALID_ARG, _abi.PHYS_ERR_INVALID_ARG)
    code, ids, msg, _, _ = ccd_probe.staging(probe, 10, [])      # n = 0: an empty list
    assert (code, ids) == (0, [])
    code, ids, msg, _, _ = ccd_probe.staging(probe, 10, [3, 4, 3])
    assert code == _abi.PHYS_ERR_INVALID_ARG and ids == [] and "body 3 is listed twice" in msg
    code, ids, msg, _, _ = ccd_probe.staging(probe, 10, [3, 10])
    assert code == _abi.PHYS_ERR_OUT_OF_RANGE and ids == [] and "entry 1 names body 10" in msg
    code, ids, msg, _, _ = ccd_probe.staging(probe, 10, [9])
    assert (code, ids) == (0, [9])
    code, _, _, _, _ = ccd_probe.staging(probe, 0, [0])
    assert code == _abi.PHYS_ERR_OUT_OF_RANGE
    # out of range is said before a duplicate, as the body edits say it before their other checks
    assert ccd_probe.staging(probe, 4, [1, 1, 4])[0] == _abi.PHYS_ERR_OUT_OF_RANGE


def test_symbols_exported_bound_and_declared():
    from physics_amd import _abi
    import physics_amd
    lib = _abi.load_library()
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    header = open(os.path.join(ROOT, "include", "physics_hip.h")).read()
    mirror = open(os.path.join(ROOT, "include", "physics_state.hpp")).read()
    for name in ("phys_set_ccd_bodies", "phys_get_ccd_hits", "phys_get_ccd_hits_device"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
        assert len(re.findall(r"pub fn %s\s*\(" % name, rust)) == 1
        assert re.search(r"int32_t %s\s*\(" % name, header)
    assert "phys_set_ccd_bodies" in mirror and "phys_get_ccd_hits" in mirror
    assert hasattr(physics_amd.World, "set_ccd_bodies") and hasattr(physics_amd.World, "ccd_hits")


def test_the_kernel_obeys_the_build_rules():
    """k_ccd_sweep, both instances, and the position half's CCD instances: no scratch, no spills (tests/test_build_rules.py
    holds the whole library to it; this names the new kernels, so that their absence is noticed)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    table = code_objects.kernels(os.path.join(ROOT, "physics_amd", "csrc", "libphysics_hip.so"))
    sweeps = [k for k in table if "k_ccd_sweep" in k["name"]]
    position = [k for k in table if "k_step_position" in k["name"]]
    assert len(sweeps) == 2 and len(position) == 4, ([k["name"] for k in sweeps], [k["name"] for k in position])
    for k in sweeps + position:
        assert not k["scratch"] and not k["spills"], k
