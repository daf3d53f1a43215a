"""Float64 reference of continuous collision (include/physics_hip.h, phys_set_ccd_bodies), written for the tests: every body
against every static and the ground, numpy only. It shares nothing with the kernel's arithmetic: the kernel casts rays at
Minkowski sums and sweeps separating axes (include/spec/box_cast.h); this reference walks the exact distance between the
mover's TRUE shape at x + t u and the target, with the closest-distance functions of tests/boxcast_ref.py.

The time of impact is the first t at which that distance reaches zero. The mover is its core box (a box, a point, a rod) plus its
radius rho, so distance(t) = boxcast_ref.closest(core at x + t u, target).d - r_target - rho, convex in t: a golden section over
[0, L] finds its minimum, a bisection the first t with distance <= 0.

    h = sweep(case)     case: the dict tests/ccd_probe.py writes as a scene (dt, ground, statics, bodies, filters)

Per body: target, t (inf without a hit), t2 (the second-best hit), frac, L, u, normal, which (the winner's static, -1 the ground),
and what tells how close each decision was: sep0 (the least distance at the start over the targets it may hit), sep_min (the least
distance over [0, L] of every target that was NOT hit, inf without one)."""
import numpy as np

import boxcast_ref as bref
import query_ref
from raycast_ref import GROUND, MISS, rotation_matrices

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, query_ref.SHAPE_SPHERE, query_ref.SHAPE_BOX, query_ref.SHAPE_CAPSULE
STATIC_ID_BIT = query_ref.STATIC_ID_BIT
FILTER_DEFAULT = (0xFFFF0001, 0)


def filter_pass(a, b):
    """the narrow phase's rule on two filters (word, group word)"""
    if a[1] == b[1] and a[1] != 0:
        return (a[1] & 0xFFFFFFFF) < 0x80000000
    return (a[0] & (b[0] >> 16)) != 0 and (b[0] & (a[0] >> 16)) != 0


def mover(shape, he):
    """(core half extents, rho) of a body shape"""
    he = np.asarray(he, np.float64)
    if shape == SHAPE_BOX:
        return he.copy(), 0.0
    if shape == SHAPE_CAPSULE:
        return np.array([0.0, he[1], 0.0]), float(he[0])
    return np.zeros(3), float(he[0])


def _filters(d, n):
    return np.asarray(d["filt"], np.uint64).reshape(n, 2) if "filt" in d else np.tile(np.array(FILTER_DEFAULT, np.uint64), (n, 1))


def sweep(case, iters=60):
    st, bd = case["statics"], case["bodies"]
    m, n = len(st["pos"]), len(bd["pos"])
    dt = float(np.float32(case["dt"]))
    ground = case.get("ground")
    gfilt = (int(case.get("ground_filt", FILTER_DEFAULT[0])), 0)
    sf, bf = _filters(st, m), _filters(bd, n)
    spos = np.asarray(st["pos"], np.float64).reshape(m, 3)
    she = np.asarray(st["half_extent"], np.float64).reshape(m, 3)
    sshape = np.asarray(st["shape"], np.int64).reshape(m)
    sR = rotation_matrices(np.asarray(st["rot"], np.float64).reshape(m, 4)) if m else np.zeros((0, 3, 3))
    sbound = query_ref._bound(she, sshape) if m else np.zeros(0)
    out = dict(target=np.full(n, MISS, np.int64), t=np.full(n, np.inf), t2=np.full(n, np.inf), frac=np.ones(n), L=np.zeros(n),
               u=np.zeros((n, 3)), normal=np.zeros((n, 3)), which=np.full(n, -2, np.int64), sep0=np.full(n, np.inf),
               sep_min=np.full(n, np.inf), swept=np.zeros(n, bool))
    X = np.asarray(bd["pos"], np.float64).reshape(n, 3)
    Q = np.asarray(bd["rot"], np.float64).reshape(n, 4)
    shape = np.asarray(bd["shape"], np.int64).reshape(n)
    with np.errstate(all="ignore"):
        M = np.asarray(bd["lin"], np.float64).reshape(n, 3) * dt
        L = np.sqrt((M * M).sum(1))
        swept = np.isfinite(L) & (L > 0) & (shape != SHAPE_NONE) & np.isfinite(X).all(1) & np.isfinite(Q).all(1)
    L = np.where(swept, L, 0.0)
    U = np.where(swept[:, None], M / np.where(swept, L, 1.0)[:, None], 0.0)
    X = np.where(swept[:, None], X, 0.0)
    R = rotation_matrices(np.where(swept[:, None], Q, [0.0, 0.0, 0.0, 1.0])) if n else np.zeros((0, 3, 3))
    HC, RHO = np.zeros((n, 3)), np.zeros(n)
    for i in np.nonzero(swept)[0]:
        HC[i], RHO[i] = mover(int(shape[i]), bd["half_extent"][i])
    out["swept"], out["L"], out["u"] = swept, L, U
    hits = [[] for _ in range(n)]  # (t, id, which)
    if ground is not None:
        for i in np.nonzero(swept)[0]:
            if not filter_pass((int(bf[i, 0]), int(bf[i, 1])), gfilt):
                continue
            gap = X[i, 1] - (HC[i] * np.abs(R[i][1, :])).sum() - RHO[i] - ground
            out["sep0"][i] = min(out["sep0"][i], gap)
            if gap > 0 and U[i, 1] < 0 and gap / -U[i, 1] < L[i]:
                hits[i].append((gap / -U[i, 1], GROUND, -1))
            elif gap > 0:
                out["sep_min"][i] = min(out["sep_min"][i], gap + min(U[i, 1], 0.0) * L[i])
    # the pairs that pass the filters and whose bounding spheres come near each other along the motion
    passes = np.array([[swept[i] and filter_pass((int(bf[i, 0]), int(bf[i, 1])), (int(sf[k, 0]), int(sf[k, 1]))) for k in range(m)]
                       for i in range(n)], bool).reshape(n, m)
    ri, ki = np.nonzero(passes)
    if len(ri):
        rel = spos[ki] - X[ri]
        along = np.clip((rel * U[ri]).sum(1), 0.0, L[ri])
        gap = np.linalg.norm(rel - along[:, None] * U[ri], axis=1) - (sbound[ki] + np.linalg.norm(HC[ri], axis=1) + RHO[ri])
        for i in np.unique(ri[gap > 0.5]):
            out["sep_min"][i] = min(out["sep_min"][i], float(gap[(ri == i) & (gap > 0.5)].min()))
        ri, ki = ri[gap <= 0.5], ki[gap <= 0.5]
    if len(ri):
        Lr = L[ri]

        def f(t, sel=slice(None)):
            r_, k_ = ri[sel], ki[sel]
            _, _, d, r = bref.closest(X[r_] + t[:, None] * U[r_], R[r_], HC[r_], spos[k_], sR[k_], she[k_], sshape[k_])
            return d - r - RHO[r_]

        f0 = f(np.zeros(len(ri)))
        np.minimum.at(out["sep0"], ri, f0)
        g = (np.sqrt(5.0) - 1.0) / 2.0
        lo, hi = np.zeros(len(ri)), Lr.copy()
        for _ in range(iters):
            m1, m2 = hi - g * (hi - lo), lo + g * (hi - lo)
            left = f(m1) <= f(m2)
            hi = np.where(left, m2, hi)
            lo = np.where(left, lo, m1)
        tmin = 0.5 * (lo + hi)
        fmin = np.minimum(f(tmin), f(Lr))
        touches = (f0 > 0) & (fmin <= 1e-9)
        sel = np.nonzero(touches)[0]
        lo, hi = np.zeros(len(sel)), tmin[sel].copy()
        for _ in range(iters):
            mid = 0.5 * (lo + hi)
            inside = f(mid, sel) <= 0
            hi = np.where(inside, mid, hi)
            lo = np.where(inside, lo, mid)
        t_hit = np.full(len(ri), np.inf)
        t_hit[sel] = hi
        for j in range(len(ri)):
            i, k = int(ri[j]), int(ki[j])
            if t_hit[j] < L[i]:
                hits[i].append((float(t_hit[j]), STATIC_ID_BIT | k, k))
            elif f0[j] > 0:
                out["sep_min"][i] = min(out["sep_min"][i], float(fmin[j]))
    for i in range(n):
        if not hits[i]:
            continue
        hits[i].sort()
        t, tid, which = hits[i][0]
        out["target"][i], out["t"][i], out["which"][i], out["frac"][i] = tid, t, which, min(t / L[i], 1.0)
        if len(hits[i]) > 1:
            out["t2"][i] = hits[i][1][0]
        out["normal"][i] = normal_at(X[i], U[i], R[i], HC[i], t, which, spos, sR, she, sshape)
    return out


def normal_at(x, u, R, hc, t, which, spos, sR, she, sshape):
    """the direction of the shortest vector from the target to the mover's core with the mover at t (a little before it where
    the two would coincide), +y for the ground"""
    if which < 0:
        return np.array([0.0, 1.0, 0.0])
    k = which
    for back in (0.0, 1e-6, 1e-4):
        c = (x + max(t - back, 0.0) * u)[None]
        qc, p, d, _ = bref.closest(c, R[None], hc[None], spos[k:k + 1], sR[k:k + 1], she[k:k + 1], sshape[k:k + 1])
        if d[0] > 1e-9:
            return (qc[0] - p[0]) / d[0]
    return -u
