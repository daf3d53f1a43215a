"""Float64 statement of depenetration (include/physics_hip.h, phys_penetration and phys_depenetrate), written for the tests
from the rule's text on top of the closest points of tests/capsulecast_ref.py: numpy only, one query at a time. An
independent restatement: it shares no code with include/spec/depenetrate.h, include/spec/collide.h or the kernels.

    valid(pos, rot, R, h)                                            the query's own values are usable
    depths(p, a, R, h, tg, ground)  -> (ids, depth, normal, inside)  every target's depth at p (ascending ids, the ground last)
    deepest(p, a, R, h, tg, ground, gap, ignore=None) -> (id, depth, normal, second depth, inside)
    depenetrate(pos, a, R, h, tg, ground, skin, max_iters) -> (p, status, [(id, normal, depth, inside)])

tg: the target dict of query_ref.targets. a: the capsule's axis (unit). Where the core lies outside a target, depth =
R + r_T - dist (boxes: R - dist) and the normal runs along the closest points, target to capsule. Where the core enters a
box (`inside`), the depth is R + the least overlap over the six separating axes of a segment and a box (the three face normals,
exit e_f + h |a_f| - |p_f|, and the three axes core x box edge): the least translation that frees the core. The spec prefers a
face within a band, so there the tests check properties only; deepest and the slots of depenetrate flag a probe as `inside` when ANY target within the gap holds the core, since
the winner then depends on that convention. Cores that meet (distance 0 between round shapes) leave along (0,-1,0), the narrow phase's
fallback seen from the target."""
import numpy as np

import capsulecast_ref as ref

STUCK, INVALID = 0x100, 0x400
MISS, GROUND = ref.MISS, ref.GROUND
MAX_HALF_LENGTH = 3.4e38
_SHAPED = (ref.SHAPE_SPHERE, ref.SHAPE_BOX, ref.SHAPE_CAPSULE)


def valid(pos, rot, R, h):
    vals = [np.asarray(pos, np.float64), np.float64(R), np.float64(h)]
    if rot is not None:
        vals.append(np.asarray(rot, np.float64))
    if not all(np.isfinite(v).all() for v in vals):
        return False
    return bool(R >= 0 and 0 <= h <= MAX_HALF_LENGTH)


def axis(rot):
    """the y axis turned by rot, float64"""
    if rot is None:
        return np.array([0.0, 1.0, 0.0])
    return ref.rotation_matrices(np.asarray(rot, np.float64).reshape(1, 4))[0][:, 1]


def frames(tg):
    return ref.query_ref._frames(tg)


def depths(p, a, R, h, tg, ground, frames_=None):
    p, a = np.asarray(p, np.float64), np.asarray(a, np.float64)
    keep = np.nonzero(np.isin(tg["shape"], _SHAPED) & np.isfinite(tg["pos"]).all(1))[0] if len(tg["pos"]) else np.zeros(0, np.int64)
    m = len(keep)
    ids, depth, normal, inside = tg["id"][keep].astype(np.int64), np.zeros(m), np.zeros((m, 3)), np.zeros(m, bool)
    if m:
        Rt = (frames(tg) if frames_ is None else frames_)[keep]
        he, shape, tp = tg["half_extent"][keep], tg["shape"][keep], tg["pos"][keep]
        q, pt, d, r = ref.closest(np.tile(p, (m, 1)), np.tile(a, (m, 1)), np.full(m, float(h)), tp, Rt, he, shape)
        out = d > 0
        with np.errstate(all="ignore"):
            normal[out] = (q[out] - pt[out]) / d[out, None]
        depth[out] = R + r[out] - d[out]
        for k in np.nonzero(~out)[0]:
            if shape[k] == ref.SHAPE_BOX:
                l, al = Rt[k].T @ (p - tp[k]), Rt[k].T @ a
                exit_ = he[k] + h * np.abs(al) - np.abs(l)
                f = int(np.argmin(exit_))
                nl = np.zeros(3)
                nl[f] = -1.0 if l[f] < 0 else 1.0
                best = exit_[f]
                for e in range(3):  # the axes core x box edge
                    x = np.cross(al, np.eye(3)[e])
                    ln = np.linalg.norm(x)
                    if ln < 1e-9:
                        continue
                    pen = (he[k] @ np.abs(x) - abs(l @ x)) / ln
                    if pen < best:
                        best, nl = pen, (x / ln) * (-1.0 if l @ x < 0 else 1.0)
                depth[k], normal[k], inside[k] = R + best, Rt[k] @ nl, True
            else:
                depth[k], normal[k] = R + r[k], (0.0, -1.0, 0.0)
    if ground is not None:
        ids = np.append(ids, GROUND)
        depth = np.append(depth, ground - (p[1] - h * abs(a[1]) - R))
        normal = np.vstack([normal, [0.0, 1.0, 0.0]])
        inside = np.append(inside, False)
    return ids, depth, normal, inside


def deepest(p, a, R, h, tg, ground, gap, ignore=None, frames_=None):
    ids, depth, normal, inside = depths(p, a, R, h, tg, ground, frames_)
    ok = depth >= -gap
    if ignore is not None:
        ok &= ids != ignore
    if not ok.any():
        return MISS, -np.inf, np.zeros(3), -np.inf, False
    ids, depth, normal, inside = ids[ok], depth[ok], normal[ok], inside[ok]
    order = np.lexsort((ids, -depth))
    k = order[0]
    return int(ids[k]), float(depth[k]), normal[k], float(depth[order[1]]) if len(order) > 1 else -np.inf, bool(inside.any())


def depenetrate(pos, a, R, h, tg, ground, skin, max_iters, ignore=None, frames_=None):
    """(p, status, slots): the loop of the rule's text"""
    p, status, slots = np.asarray(pos, np.float64).copy(), 0, []
    for k in range(max_iters + 1):
        i, d, n, _, inside = deepest(p, a, R, h, tg, ground, skin, ignore, frames_)
        if i == MISS or not d > -0.5 * skin:
            break
        if k == max_iters:
            status |= STUCK
            break
        slots.append((i, n, d, inside))
        status += 1
        p = p + n * (d + skin)
    return p, status, slots


def face_exit(p, a, R, h, pos, Rt, he):
    """R + the least exit of the core through a face of the box (pos, Rt, he): the most a probe may report for a core inside it"""
    l, al = Rt.T @ (np.asarray(p, np.float64) - pos), Rt.T @ np.asarray(a, np.float64)
    return R + float((he + h * np.abs(al) - np.abs(l)).min())


def separation(p, a, R, h, tg, ground, frames_=None):
    """the least float64 separation of the capsule at p from every target (-depth of the deepest); +inf with none"""
    _, depth, _, _ = depths(p, a, R, h, tg, ground, frames_)
    return -depth.max() if len(depth) else np.inf
