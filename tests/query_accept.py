"""The acceptance of the read-only queries against their float64 references (tests/raycast_ref.py, tests/query_ref.py),
shared by tests/test_gpu_raycast.py, tests/test_gpu_query.py, tests/test_gpu_filter.py and tests/test_gpu_query_grid.py.

Tolerances: t within 1e-5 (1 + |o|_inf + t), normals and overlap distances within 1e-4; another answer than the
reference's only where the reference itself is ambiguous (a near tie, a grazing ray, a pair within 1e-4 of touching), and
those counted and capped at max(2, n // 1000) rays, max(3, n // 200) casts, max(2, n // 200) overlap queries.
`centre`: the scene's centre, subtracted in float64 by the references; |o| is then measured from it (the kernels test
every candidate in body-relative coordinates, so the distance of a scene from the origin costs them nothing)."""
import math

import numpy as np

import query_ref
import raycast_ref


def ray_cap(n):
    return max(2, n // 1000)


def cast_cap(n):
    return max(3, n // 200)


def overlap_cap(n):
    return max(2, n // 200)


def ray_tol(h, i, gt=math.inf):
    """1e-5 (1 + |o|_inf + t) of ray i: t the reference's, or the GPU's where the reference missed"""
    rt = float(h["t"][i])
    oinf = float(np.abs(h["o"][i]).max()) if h["valid"][i] else 0.0
    return 1e-5 * (1.0 + oinf + (rt if math.isfinite(rt) else (gt if math.isfinite(gt) else 0.0)))


def _normal_ok(h, i, gb, gt, nrm):
    ref = raycast_ref
    u = h["u"][i]
    if gt == 0:
        opts = [-u]
    elif gb == ref.GROUND:
        opts = [np.array([0.0, 1.0, 0.0])]
    else:
        k = ref.row_of(h, gb)
        opts = ref.normal_of(h["o"][i], u, gt, h["pos"][k], h["R"][k], h["he"][k], h["shape"][k])
        if h["t"][i] != gt:  # judged at the float64 t as well
            opts += ref.normal_of(h["o"][i], u, h["t"][i], h["pos"][k], h["R"][k], h["he"][k], h["shape"][k])
    return any(np.abs(nrm - o).max() <= 1e-4 for o in opts)


def compare(w, bodies, o, d, max_t=None, ignore=None, ground=0.0, label="", out=None, statics=None, centre=None, h=None):
    """Ray casts: same id -> |dt| <= 1e-5 (1 + |o|_inf + t), normal to 1e-4 (either face at an edge); another id only for
    a near tie or a grazing ray; hit against miss only for grazing rays (counted, asserted tiny). h: the reference's
    answer where the caller has it already."""
    ref = raycast_ref
    body, t, nrm = out if out is not None else w.raycast(o, d, max_t, ignore)
    if h is None:
        h = ref.cast(o, d, bodies, max_t, ignore, ground, statics=statics, centre=centre)
    ground = h["ground"]
    n = len(body)
    grazing, bad = 0, []
    for i in range(n):
        rb, rt = int(h["body"][i]), float(h["t"][i])
        gb, gt = int(body[i]), float(t[i])
        tol = ray_tol(h, i, gt)
        if gb == rb:
            if rb == ref.MISS:
                if not (gt == math.inf and not nrm[i].any()):
                    bad.append((i, "miss with t / normal", gt, nrm[i]))
            elif abs(gt - rt) > tol:
                bad.append((i, "t", gb, gt, rt))
            elif not _normal_ok(h, i, gb, gt, nrm[i]):
                bad.append((i, "normal", gb, nrm[i], h["normal"][i]))
            continue
        if gb != ref.MISS and rb != ref.MISS:
            if gb == ref.GROUND:
                u = h["u"][i]
                tg64 = 0.0 if h["o"][i][1] <= ground else ((ground - h["o"][i][1]) / u[1] if u[1] < 0 else math.inf)
            else:
                tg64 = ref.t_of(h, i, gb)
            if abs(tg64 - rt) <= tol and abs(gt - rt) <= tol:
                continue  # near tie
            if h["span"][i] <= tol or (gb != ref.GROUND and not math.isfinite(tg64) and ref.near_body(h, i, gb, gt, tol)):
                grazing += 1
                continue
            bad.append((i, "id", gb, gt, rb, rt, tg64))
        elif gb == ref.MISS:
            if h["span"][i] <= tol:
                grazing += 1
            else:
                bad.append((i, "gpu miss", rb, rt, h["span"][i]))
        else:
            if gb != ref.GROUND and ref.near_body(h, i, gb, gt, tol):
                grazing += 1
            else:
                bad.append((i, "ref miss", gb, gt))
    print(f"{label}: {n} rays, {int((h['body'] != ref.MISS).sum())} hits, grazing disagreements {grazing}")
    assert not bad, f"{label}: {len(bad)} mismatches, first {bad[:8]}"
    assert grazing <= ray_cap(n), f"{label}: {grazing} grazing disagreements"
    return body, t, nrm


def compare_casts(w, tg, o, d, rad, ground=0.0, ignore=None, out=None, label="", centre=None, max_t=None, h=None):
    """Sphere casts: same id -> |dt| <= 1e-5 (1 + |o|_inf + t), normal within 1e-4; another id only at a near tie (both
    ids' float64 t within tolerance) or a grazing contact (the second target's float64 t near the GPU's); counted and
    asserted rare"""
    ref = query_ref
    body, t, nrm = out if out is not None else w.spherecast(o, d, rad, max_t=max_t, ignore=ignore)
    if h is None:
        h = ref.spherecast(o, d, rad, tg, max_t=max_t, ignore=ignore, ground=ground, centre=centre)
    tg = h["tg"]
    n = len(body)
    odd, bad, odd_cases = 0, [], []
    for i in range(n):
        rb, rt, gb, gt = int(h["body"][i]), float(h["t"][i]), int(body[i]), float(t[i])
        oinf = float(np.abs(h["o"][i]).max()) if h["valid"][i] else 0.0
        tol = 1e-5 * (1.0 + oinf + (rt if math.isfinite(rt) else (gt if math.isfinite(gt) else 0.0)))
        if gb == rb:
            if rb == ref.MISS:
                if not (gt == math.inf and not nrm[i].any()):
                    bad.append((i, "miss with t / normal"))
            elif abs(gt - rt) > tol:
                bad.append((i, "t", gb, gt, rt))
            elif np.abs(nrm[i] - h["normal"][i]).max() > 1e-4 and rt > 0:
                # a contact at an edge: the normal turns fast along t; judge at the GPU's t
                k = h["which"][i]
                if gb == ref.GROUND or k < 0:
                    bad.append((i, "normal", nrm[i], h["normal"][i]))
                else:
                    alt = ref.closest_normal(h["o"][i] + gt * h["u"][i], tg["pos"][k], ref._frames(tg)[k],
                                             tg["half_extent"][k], tg["shape"][k])
                    if abs(float(h["normal"][i] @ h["u"][i])) < 0.1:
                        odd += 1  # a grazing contact: the normal turns fast with t there
                    elif np.abs(nrm[i] - alt).max() > 1e-3:
                        bad.append((i, "normal", nrm[i], h["normal"][i]))
            continue
        # another id: a near tie (the second-best float64 t is within tolerance) or a grazing contact
        if math.isfinite(rt) and abs(float(h["t2"][i]) - rt) <= 4 * tol and abs(gt - rt) <= 4 * tol:
            odd_cases.append((i, "tie", gb, gt, rb, rt))
            continue
        if gb == ref.MISS and not math.isfinite(float(h["t2"][i])) and rt > 0:
            odd_cases.append((i, "gpu miss", rb, rt))  # the float64 contact is the only one: a grazing touch float32 missed
            continue
        if gb != ref.MISS and gb != ref.GROUND and math.isfinite(gt):
            # a grazing touch of the GPU's target that float64 calls a miss or a later contact
            k = int(np.nonzero(tg["id"] == gb)[0][0])
            c = (h["o"][i] + gt * h["u"][i])[None]
            r_i = float(np.broadcast_to(np.asarray(rad, np.float64), (n,))[i])
            dist = ref.point_dist(c, tg["pos"][k:k + 1], ref._frames(tg)[k:k + 1], tg["half_extent"][k:k + 1],
                                  tg["shape"][k:k + 1])[0]
            if dist <= r_i + tol and gt <= rt + tol:
                odd_cases.append((i, "graze", gb, gt, rb, rt))
                continue
        bad.append((i, "id", gb, gt, rb, rt))
    assert not bad, f"{label}: {len(bad)} of {n}: {bad[:8]}"
    odd = len(odd_cases) + odd
    print(f"{label}: {n} casts, {int((h['body'] != ref.MISS).sum())} hits, near ties / grazing contacts {odd}")
    assert odd <= cast_cap(n), f"{label}: {odd} near ties / grazing contacts of {n}: {odd_cases[:8]}"
    return body, t, nrm


def compare_overlaps(w, tg, st, pos, rot, he, ground=0.0, ignore=None, label="", centre=None, want=None, out=None):
    """Overlap queries: ascending unique ids per query, the reference's set but for pairs within 1e-4 of touching
    (counted and capped). want: the reference's answer where the caller has it already."""
    ref = query_ref
    off, ids = out if out is not None else w.overlap(st, pos, rot, he, ignore=ignore)
    if want is None:
        want = ref.overlap(st, pos, rot, he, tg, ignore=ignore, ground=ground, centre=centre)
    n = len(pos)
    assert len(off) == n + 1 and off[0] == 0 and off[n] == len(ids)
    near = 0
    for i in range(n):
        got = [int(x) for x in ids[off[i]:off[i + 1]]]
        assert got == sorted(set(got)), (label, i, got[:16])
        exp, close = want[i]
        diff = set(got) ^ set(exp)
        for k in diff:
            assert k in close and abs(close[k]) <= 1e-4, (label, i, k, got[:16], exp[:16], close.get(k))
            near += 1
    print(f"{label}: {n} queries, {int(off[n])} ids, pairs within 1e-4 of touching that differ {near}")
    assert near <= overlap_cap(n), f"{label}: {near} pairs within 1e-4 of touching of {n} queries"
    return off, ids
