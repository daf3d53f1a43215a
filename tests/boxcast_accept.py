"""The acceptance of box casts against their float64 reference (tests/boxcast_ref.py), shared by tests/test_gpu_boxcast.py
and tests/test_boxcast_cpu.py. capsulecast_accept's rule, with the magnitudes that enter the arithmetic of a box cast:

  t       within tol = 1e-5 (1 + |o|_inf + |he| + t): the box's corners lie |he| from the centre
  normal  within 1e-4 of the reference's; where the contact turns fast along t it is judged at the answer's t; grazing
          contacts (|n . u| < 0.1) are counted, not failed
  point   within tol of the target's surface and of the cast box's surface at the answer's t. The point is a world coordinate
          stored in float32: the spacing of float32 at that coordinate is added
  id      another id only at a near tie (the reference's second-best t within 4 tol) or a grazing touch; these are counted
          with the other odd cases and capped at cast_cap(n) = max(3, n // 200). near_ties() is the reference's own count of the
          first kind: tests/test_boxcast_cpu.py holds it to half the cap for every seeded input of the GPU tests."""
import math

import numpy as np

import boxcast_ref as ref
from capsulecast_accept import _surface_gap
from query_accept import cast_cap
from raycast_ref import GROUND, MISS


def tol_of(h, i, gt=math.inf):
    rt = float(h["t"][i])
    oinf = float(np.abs(h["o"][i]).max()) if h["valid"][i] else 0.0
    return 1e-5 * (1.0 + oinf + float(np.linalg.norm(h["he"][i])) + (rt if math.isfinite(rt) else (gt if math.isfinite(gt) else 0.0)))


def near_ties(h):
    """how many queries have a second target within 4 tol of the first: where float32 may rightly report the other id"""
    return sum(1 for i in range(len(h["t"])) if math.isfinite(h["t2"][i]) and h["t2"][i] - h["t"][i] <= 4 * tol_of(h, i))


def _box_gap(h, i, t, p):
    """|distance| of the point p from the surface of query i's box with its centre at t"""
    l = h["R"][i].T @ (p - (h["o"][i] + t * h["u"][i]))
    g = np.abs(l) - h["he"][i]
    return float(np.linalg.norm(np.maximum(g, 0.0))) if (g > 0).any() else float(abs(g.max()))


def _point_ok(h, i, k, gt, pt, tol, centre):
    """pt: the answer's point relative to the centre (float64)"""
    world = pt + (0.0 if centre is None else np.asarray(centre, np.float64))
    tol = tol + float(np.spacing(np.float32(np.abs(world).max())))
    gap = abs(pt[1] - h["ground"]) if k < 0 else _surface_gap(pt, h["tg"], k)
    own = _box_gap(h, i, gt, pt)
    return gap <= tol and own <= tol, (gap, own, tol)


def compare_boxcasts(h, out, label="", centre=None):
    """h: the reference's answer; out: (body, t, normal, point) of the kernel or of the host probe. Returns the count of odd
    cases (near ties, grazing contacts, touching starts)."""
    body, t, nrm, pnt = out
    tg = h["tg"]
    n = len(body)
    c64 = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    odd, bad, odd_cases = 0, [], []
    for i in range(n):
        rb, rt, gb, gt = int(h["body"][i]), float(h["t"][i]), int(body[i]), float(t[i])
        tol = tol_of(h, i, gt)
        if gb == rb:
            if rb == MISS:
                if not (gt == math.inf and not nrm[i].any() and not pnt[i].any()):
                    bad.append((i, "miss with t / normal / point"))
                continue
            if abs(gt - rt) > tol:
                bad.append((i, "t", gb, gt, rt, tol))
                continue
            if gt == 0 or rt == 0:
                if gt != rt:
                    odd_cases.append((i, "touching start", gt, rt))
                elif np.abs(nrm[i] - h["normal"][i]).max() > 1e-6 or pnt[i].any():
                    bad.append((i, "t = 0: normal / point", nrm[i], pnt[i]))
                continue
            k = int(h["which"][i])
            if np.abs(nrm[i] - h["normal"][i]).max() > 1e-4:
                alt, _ = ref.contact(h, i, gt)
                if abs(float(h["normal"][i] @ h["u"][i])) < 0.1:
                    odd += 1  # a grazing contact: the normal turns fast with t there
                elif np.abs(nrm[i] - alt).max() > 1e-3:
                    bad.append((i, "normal", gb, nrm[i], h["normal"][i], alt))
                    continue
            ok, figures = _point_ok(h, i, k, gt, pnt[i].astype(np.float64) - c64, tol, centre)
            if not ok:
                bad.append((i, "point", gb, pnt[i], h["point"][i] + c64, figures))
            continue
        if math.isfinite(rt) and abs(float(h["t2"][i]) - rt) <= 4 * tol and abs(gt - rt) <= 4 * tol:
            odd_cases.append((i, "tie", gb, gt, rb, rt))
            continue
        if gb == MISS and not math.isfinite(float(h["t2"][i])) and rt > 0:
            odd_cases.append((i, "gpu miss", rb, rt))  # the float64 contact is the only one: a grazing touch float32 missed
            continue
        if gb != MISS and gb != GROUND and math.isfinite(gt):
            k = int(np.nonzero(tg["id"] == gb)[0][0])
            if ref.separation_at(h, i, gt, k) <= tol and gt <= rt + tol:
                odd_cases.append((i, "graze", gb, gt, rb, rt))
                continue
        bad.append((i, "id", gb, gt, rb, rt))
    odd = len(odd_cases) + odd
    print(f"{label}: {n} box casts, {int((h['body'] != MISS).sum())} hits, near ties / grazing contacts {odd}")
    assert not bad, f"{label}: {len(bad)} of {n}: {bad[:6]}"
    assert odd <= cast_cap(n), f"{label}: {odd} near ties / grazing contacts of {n}: {odd_cases[:8]}"
    return odd
