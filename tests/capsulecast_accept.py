"""The acceptance of capsule casts against their float64 reference (tests/capsulecast_ref.py), shared by
tests/test_gpu_capsulecast.py and tests/test_capsulecast_cpu.py. The rule of query_accept.compare_casts, with the
magnitudes that enter the arithmetic of a capsule cast:

  t       within tol = 1e-5 (1 + |o|_inf + h + t): the core's ends lie h from the centre
  normal  within 1e-4 of the reference's; where the contact turns fast along t it is judged at the GPU's t
  point   within tol of the target's surface and within R + tol of the capsule's core at the GPU's t. The point is a world
          coordinate stored in float32: the spacing of float32 at that coordinate is added (1/64 at 2e5 from the origin)
  id      another id only at a near tie (the reference's second-best t within 4 tol) or a grazing contact; these are
          counted and capped at cast_cap(n) = max(3, n // 200). near_ties() is the reference's own count of the first kind:
          tests/test_capsulecast_cpu.py holds it to half the cap for every seeded input of the GPU tests."""
import math

import numpy as np

import capsulecast_ref as ref
import query_ref
from query_accept import cast_cap
from raycast_ref import GROUND, MISS


def tol_of(h, i, gt=math.inf):
    rt = float(h["t"][i])
    oinf = float(np.abs(h["o"][i]).max()) if h["valid"][i] else 0.0
    return 1e-5 * (1.0 + oinf + float(h["hq"][i]) + (rt if math.isfinite(rt) else (gt if math.isfinite(gt) else 0.0)))


def near_ties(h):
    """how many queries have a second target within 4 tol of the first: where float32 may rightly report the other id"""
    return sum(1 for i in range(len(h["t"])) if math.isfinite(h["t2"][i]) and h["t2"][i] - h["t"][i] <= 4 * tol_of(h, i))


def _surface_gap(p, tg, k):
    """|distance| of the point p from the surface of target row k"""
    d = p - tg["pos"][k]
    he, shape = tg["half_extent"][k], tg["shape"][k]
    R = query_ref._frames(tg)[k]
    if shape == query_ref.SHAPE_SPHERE:
        return abs(np.linalg.norm(d) - he[0])
    if shape == query_ref.SHAPE_CAPSULE:
        w = R[:, 1]
        return abs(np.linalg.norm(d - np.clip(d @ w, -he[1], he[1]) * w) - he[0])
    l = R.T @ d
    g = np.abs(l) - he
    return np.linalg.norm(np.maximum(g, 0.0)) if (g > 0).any() else abs(g.max())


def _core_dist(h, i, t, p):
    c = h["o"][i] + t * h["u"][i]
    a = h["a"][i]
    return np.linalg.norm(p - c - np.clip((p - c) @ a, -h["hq"][i], h["hq"][i]) * a)


def _point_ok(h, i, k, gt, pt, tol, centre):
    """pt: the GPU's point relative to the centre (float64)"""
    world = pt + (0.0 if centre is None else np.asarray(centre, np.float64))
    tol = tol + float(np.spacing(np.float32(np.abs(world).max())))
    if k < 0:
        gap = abs(pt[1] - h["ground"])
    else:
        gap = _surface_gap(pt, h["tg"], k)
    return gap <= tol and _core_dist(h, i, gt, pt) <= h["rad"][i] + tol, (gap, _core_dist(h, i, gt, pt) - h["rad"][i], tol)


def compare_capsulecasts(w, tg, o, d, rot, rad, hq, ground=0.0, ignore=None, out=None, label="", centre=None, max_t=None, h=None):
    """Returns the GPU's (body, t, normal, point). h: the reference's answer where the caller has it already; out: the
    GPU's where the caller made the call (a filtered or device call)."""
    body, t, nrm, pnt = out if out is not None else w.capsulecast(o, d, rad, hq, rot=rot, max_t=max_t, ignore=ignore)
    if h is None:
        h = ref.capsulecast(o, d, rot, rad, hq, tg, max_t=max_t, ignore=ignore, ground=ground, centre=centre)
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
                    # a cast that starts within rounding of touching: one side says t = 0, the other a t below tol
                    odd_cases.append((i, "touching start", gt, rt))
                elif np.abs(nrm[i] - h["normal"][i]).max() > 1e-6 or pnt[i].any():
                    bad.append((i, "t = 0: normal / point", nrm[i], pnt[i]))
                continue
            k = int(h["which"][i])
            if np.abs(nrm[i] - h["normal"][i]).max() > 1e-4:
                # a contact at an edge: the normal turns fast along t; judge at the GPU's t
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
        # another id: a near tie (the second-best float64 t is within tolerance) or a grazing contact
        if math.isfinite(rt) and abs(float(h["t2"][i]) - rt) <= 4 * tol and abs(gt - rt) <= 4 * tol:
            odd_cases.append((i, "tie", gb, gt, rb, rt))
            continue
        if gb == MISS and not math.isfinite(float(h["t2"][i])) and rt > 0:
            odd_cases.append((i, "gpu miss", rb, rt))  # the float64 contact is the only one: a grazing touch float32 missed
            continue
        if gb != MISS and gb != GROUND and math.isfinite(gt):
            # a grazing touch of the GPU's target that float64 calls a miss or a later contact
            k = int(np.nonzero(tg["id"] == gb)[0][0])
            if ref.separation_at(h, i, gt, k) <= tol and gt <= rt + tol:
                odd_cases.append((i, "graze", gb, gt, rb, rt))
                continue
        bad.append((i, "id", gb, gt, rb, rt))
    assert not bad, f"{label}: {len(bad)} of {n}: {bad[:6]}"
    odd = len(odd_cases) + odd
    print(f"{label}: {n} capsule casts, {int((h['body'] != MISS).sum())} hits, near ties / grazing contacts {odd}")
    assert odd <= cast_cap(n), f"{label}: {odd} near ties / grazing contacts of {n}: {odd_cases[:8]}"
    return body, t, nrm, pnt
