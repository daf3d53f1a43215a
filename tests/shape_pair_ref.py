"""Float64 geometry of two convex shapes out of {sphere, box, capsule} (and of each against the plane y = 0), the
generators of isolated pairs, and the checks that hold a narrow phase's manifolds to that geometry. numpy only; shares no
code with the project's collision header or with the CPU oracle: tests/test_gpu_shape_pairs.py calls the checks on the
GPU's manifolds, tests/test_shape_pairs_cpu.py on the oracle's (which validates this reference and its tolerances where
there is no GPU).

    sc = scene(kind, n_pairs, seed)            kind in KINDS ("SS", "SB", "SC", "BC", "CC", "BB")
    arr = arrange(sc, order)                   order in ("ab", "ba"): bodies 2k, 2k + 1 = first, second shape (or swapped)
    rep = check(kind, A, B, keys, manifolds)   A, B: lists of Shape in MANIFOLD order; keys: the id pair of each
    rep.assert_ok()

Geometry. Sphere and capsule are a core segment (of length 0 for the sphere) and a radius, so every pair without two
boxes is `distance of the core to the other core / box, minus the radii`, in CLOSED FORM: segment - segment from the
interior stationary point and the four end projections, segment - box from the twelve box edges, the two core ends and
a slab test. Where the core enters the box the gap is -(radius + the deepest core point's distance to its nearest face):
exact in sign, a lower bound in size. Two boxes: the 15-axis SAT separation (test_gpu_independent.sat_separation), exact
in sign, which is also the quantity the contact margin is defined on.

TOLERANCES (all absolute, on coordinates below ~100 where float32 resolves 8e-6):
  BAND = 1e-3       around the contact margin: existence and point counts are not judged inside it (the project's band).
  TOL = 1e-4        depths and normals against closed forms (the project's float32-vs-float64 tolerance). Every reference
                    here is a closed form; query_ref.separation's golden-section value differs from it by <= 2e-9 on the
                    committed seeds (test_shape_pairs_cpu.py measures that), which adds nothing at this scale.
  TOL_PUSH[kind]    what may remain of an overlap after B is moved out along the manifold normal by the deepest depth:
                    TWICE the worst residual the spec leaves on the committed seeds (N_PAIRS pairs per kind, both index
                    orders), measured through the CPU oracle against the float64 gap (test_shape_pairs_cpu.py prints the
                    figures), and never below TOL. Measured worst residuals:
                      SS 2.1e-7, SB 2.1e-7, SC 4.3e-6, CC 7.3e-6, BB 8.2e-6: float32 rounding -> TOL each;
                      BC 4.12e-3 (at depth 0.70: a core inside the box leaves through a face with the depth of the part
                         of the core over that face's rectangle; the part beyond the rectangle can still graze the
                         face's edge) -> 8.3e-3. A wrong or flipped axis leaves residuals of the size of the depth.
EXCEPTIONS (where the spec differs from the exact geometry on purpose), stated in float64 and counted with the skipped:
  * near-parallel capsules: the spec treats two cores with sin^2 <= 1e-4 of their angle as parallel (normal = the offset
    of the axes, points = the ends of the overlap). For pairs with sin^2 <= PAR_SIN2 + PAR_BAND the normal may differ from
    the closest direction by 2 sin, the depth by 2 sin^2 x the pair's reach, and points of the two index orders by
    2 sin x reach (measured: normal 9.6e-3, depth 4.3e-5, points 5.5e-3).
  * a capsule core near-parallel to a box edge (sin^2 <= PAR_SIN2 + PAR_BAND to an axis of the box): the spec's segment -
    segment routine starts near-parallel segments from the MIDDLE of the core and does not move along it, so the core
    point of a one-point contact may sit up to hl from the closest one and hl x sin farther from the edge: depth and
    push-out get hl x sin more, the normal hl x sin / distance (measured: depth 6.9e-4, normal 1.6e-2; the bound allows
    up to 1.2e-2 of depth at hl = 1.2 - a candidate for a later change of the spec).
  * a capsule over a box face whose core leans past the face's edge by a hair: the spec keeps the face normal unless the
    edge is nearer than the clipped core by more than 1e-6; face_readings() accepts the normal of a face from which the
    clipped core is no farther than the true distance + 2e-6 (1 pair of 3000; its depth still holds to TOL).
  * two boxes: the sliver rule and the face preference, exactly as test_gpu_independent states them (its helpers). Two
    boxes have no order symmetry (the faces of A are preferred) and no closest-direction check (the normal is a SAT axis,
    checked in test_gpu_independent).
SHARES per kind, asserted by Report.assert_ok: at most 10 % skipped or under an exception, at least 25 % contacts, at
least 25 % clear misses (measured: skipped + excepted 0.1 % SS ... 6.1 % BB; contacts 48-67 %; misses 32-46 %)."""
import itertools
from collections import namedtuple

import numpy as np

import capsule_ref as cref
import query_ref as qref
from test_gpu_independent import (GROUND, MARGIN, SLIVER_DEPTH, SLIVER_REL, _box_pairs, pair_base, quat_to_matrix, random_quats,
                                  sat_separation, sliver_readings)

SPHERE, BOX, CAPSULE = qref.SHAPE_SPHERE, qref.SHAPE_BOX, qref.SHAPE_CAPSULE
STATIC_ID_BIT = qref.STATIC_ID_BIT
KINDS = {"SS": (SPHERE, SPHERE), "SB": (SPHERE, BOX), "SC": (SPHERE, CAPSULE), "BC": (BOX, CAPSULE),
         "CC": (CAPSULE, CAPSULE), "BB": (BOX, BOX)}
GROUND_KINDS = {"S": SPHERE, "B": BOX, "C": CAPSULE}
BAND = 1e-3
TOL = 1e-4
TOL_PUSH = {"SS": TOL, "SB": TOL, "SC": TOL, "CC": TOL, "BB": TOL, "BC": 8.3e-3}
PAR_SIN2, PAR_BAND = 1e-4, 1e-5
MAX_SKIPPED, MIN_CONTACTS, MIN_MISSES = 0.10, 0.25, 0.25
N_PAIRS = 3000           # per kind, in one world and one update
SEEDS = {"SS": 101, "SB": 102, "SC": 103, "BC": 104, "CC": 105, "BB": 106, "S": 111, "B": 112, "C": 113}

Shape = namedtuple("Shape", "type c R h")  # float64: centre, rotation matrix, half extents


def shapes(types, pos, rot, he):
    """Shape list of the float32 arrays a world is given (the values the device sees, as float64)."""
    types = np.broadcast_to(np.asarray(types), (len(pos),))
    return [Shape(int(t), p.astype(np.float64), quat_to_matrix(q.astype(np.float64)), h.astype(np.float64))
            for t, p, q, h in zip(types, pos, rot, he)]


def moved(s, d):
    return Shape(s.type, s.c + d, s.R, s.h)


# ------------------------------------------------------------------------------------------------ closed-form distances
def core(s):
    """(centre, unit axis, half-length, radius) of a sphere's or a capsule's core segment"""
    if s.type == CAPSULE:
        return s.c, s.R[:, 1], float(s.h[1]), float(s.h[0])
    return s.c, np.array([0.0, 1.0, 0.0]), 0.0, float(s.h[0])


def seg_segs(ca, ua, ha, cb, ub, hb):
    """One segment ca + s ua (|s| <= ha) against m segments cb + t ub (|t| <= hb), unit axes: (distance, point on the
    one, point on the other) per segment. The minimum is at the interior stationary point or has a parameter at a bound,
    where the other parameter is the projection of that end: five candidates, the least wins."""
    cb, ub, hb = np.atleast_2d(cb), np.atleast_2d(ub), np.atleast_1d(hb).astype(np.float64)
    r = ca - cb
    b, c, f = ub @ ua, r @ ua, (r * ub).sum(1)
    den = 1.0 - b * b
    ok = den > 1e-12
    s0 = np.clip(np.where(ok, (b * f - c) / np.where(ok, den, 1.0), 0.0), -ha, ha)
    t0 = np.clip(b * s0 + f, -hb, hb)
    s0 = np.clip(b * t0 - c, -ha, ha)
    t0 = np.clip(b * s0 + f, -hb, hb)
    ss, tt = [s0], [t0]
    for s_end in (-ha, ha):
        ss.append(np.full_like(b, s_end))
        tt.append(np.clip(b * s_end + f, -hb, hb))
    for sign in (-1.0, 1.0):
        t_end = sign * hb
        ss.append(np.clip(b * t_end - c, -ha, ha))
        tt.append(t_end)
    ss, tt = np.array(ss), np.array(tt)                                   # (5, m)
    pa = ca + ss[:, :, None] * ua                                           # (5, m, 3)
    pb = cb[None] + tt[:, :, None] * ub[None]
    d = np.linalg.norm(pa - pb, axis=2)
    k = np.argmin(d, axis=0)
    i = np.arange(len(b))
    return d[k, i], pa[k, i], pb[k, i]


_EDGES = [(k, sj, sl) for k in range(3) for sj in (-1.0, 1.0) for sl in (-1.0, 1.0)]


def seg_box(c, u, hl, box):
    """Core segment against a box: (distance, point on the core, point on the box), world coordinates. Distance 0: the
    core touches or enters the box, and the first point then carries no meaning."""
    pc, dl, e = box.R.T @ (c - box.c), box.R.T @ u, box.h
    # slab test: the part of the segment inside the box
    lo, hi = -hl, hl
    for j in range(3):
        if abs(dl[j]) < 1e-300:
            if abs(pc[j]) > e[j]:
                lo, hi = 1.0, -1.0
        else:
            t0, t1 = (-e[j] - pc[j]) / dl[j], (e[j] - pc[j]) / dl[j]
            lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
    if lo <= hi:
        p = box.c + box.R @ (pc + 0.5 * (lo + hi) * dl)
        return 0.0, p, p
    cb, ub, hb = np.zeros((12, 3)), np.zeros((12, 3)), np.zeros(12)
    for n, (k, sj, sl) in enumerate(_EDGES):
        j, l = (k + 1) % 3, (k + 2) % 3
        cb[n, j], cb[n, l], ub[n, k], hb[n] = sj * e[j], sl * e[l], 1.0, e[k]
    d, pa, pb = seg_segs(pc, dl, hl, cb, ub, hb)
    k = int(np.argmin(d))
    best = (float(d[k]), pa[k], pb[k])
    for s_end in ((-hl, hl) if hl > 0 else (0.0,)):
        p = pc + s_end * dl
        q = np.clip(p, -e, e)
        dist = float(np.linalg.norm(p - q))
        if dist < best[0]:
            best = (dist, p, q)
    return best[0], box.c + box.R @ best[1], box.c + box.R @ best[2]


def core_depth_in_box(c, u, hl, box):
    """The deepest core point's distance to its nearest face: max over the core of min_i (h_i - |p_i(s)|), a concave
    piecewise-linear function of s: its maximum is at an end of the core or where two of the six linear pieces meet."""
    pc, dl, e = box.R.T @ (c - box.c), box.R.T @ u, box.h
    off = np.concatenate([e - pc, e + pc])        # piece m: off[m] + slope[m] * s
    slope = np.concatenate([-dl, dl])
    cand = [-hl, hl]
    for m, n in itertools.combinations(range(6), 2):
        ds = slope[m] - slope[n]
        if abs(ds) > 1e-300:
            s = (off[n] - off[m]) / ds
            if -hl < s < hl:
                cand.append(s)
    return max(float(np.min(off + slope * s)) for s in cand)


def pair_gap(a, b):
    """(signed gap, unit direction from a's closest point to b's - None unless the cores / the core and the box are apart,
    core distance). Two boxes: the SAT separation over all 15 axes, no direction."""
    if a.type == BOX and b.type == BOX:
        return sat_separation(a.c, a.R, a.h, b.c, b.R, b.h, min_cross=1e-6)[0], None, None
    if a.type == BOX:
        g, n, d = pair_gap(b, a)
        return g, (None if n is None else -n), d
    ca, ua, ha, ra = core(a)
    if b.type == BOX:
        dist, p, q = seg_box(ca, ua, ha, b)
        if dist == 0.0:
            return -(ra + core_depth_in_box(ca, ua, ha, b)), None, 0.0
        return dist - ra, (q - p) / dist, dist
    cb, ub, hb, rb = core(b)
    dist, p, q = seg_segs(ca, ua, ha, cb, ub, hb)
    dist, p, q = float(dist[0]), p[0], q[0]
    return dist - ra - rb, ((q - p) / dist if dist > 1e-9 else None), dist


def plane_gap(s):
    """height of the lowest point of the shape above the plane y = 0"""
    if s.type == SPHERE:
        return float(s.c[1] - s.h[0])
    if s.type == CAPSULE:
        return float(s.c[1] - abs(s.R[1, 1]) * s.h[1] - s.h[0])
    return float(s.c[1] - np.abs(s.R[1]) @ s.h)


def surface_dist(p, s):
    """distance of point p to the closed shape (0 inside), by query_ref.point_dist"""
    return float(qref.point_dist(p[None], s.c[None], s.R[None], s.h[None], np.array([s.type]))[0])


def cores_sin2(a, b):
    """sin^2 of the angle of two capsules' cores (1 where one of them has no length)"""
    if a.type != CAPSULE or b.type != CAPSULE or a.h[1] == 0 or b.h[1] == 0:
        return 1.0
    ua, ub = a.R[:, 1], b.R[:, 1]
    return float(1.0 - (ua @ ub) ** 2 / ((ua @ ua) * (ub @ ub)))


def edge_parallel_slack(a, b):
    """hl x sin of a capsule core within sin^2 <= PAR_SIN2 + PAR_BAND of an axis of the box, else 0 (see EXCEPTIONS)"""
    cap, box = (a, b) if a.type == CAPSULE else (b, a)
    dl = box.R.T @ cap.R[:, 1]
    sin2 = float(np.min(1.0 - dl * dl / (dl @ dl)))
    slack = float(cap.h[1] * np.sqrt(max(sin2, 0.0))) if sin2 <= PAR_SIN2 + PAR_BAND else 0.0
    return slack if slack > 0.1 * TOL else 0.0   # (parallel within float32 rounding: no slack needed, no exception counted)


def face_readings(a, b, dist):
    """Capsule - box pairs that are apart: the unit normals A -> B of the box faces whose reading the spec may keep. The
    spec clips the core to a face's rectangle and takes the face normal; an edge of the face overrides that only where it
    is nearer than the clipped core by more than 1e-6. In float64: a face from which the clipped core is no farther than
    the true distance + 2e-6."""
    cap, box = (a, b) if a.type == CAPSULE else (b, a)
    c, u, hl, r = core(cap)
    pc, dl, e = box.R.T @ (c - box.c), box.R.T @ u, box.h
    out = []
    for f in range(3):
        lo, hi = -hl, hl
        for j in range(3):
            if j == f:
                continue
            if abs(dl[j]) < 1e-300:
                if abs(pc[j]) > e[j]:
                    lo, hi = 1.0, -1.0
            else:
                t0, t1 = (-e[j] - pc[j]) / dl[j], (e[j] - pc[j]) / dl[j]
                lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
        if lo > hi:
            continue
        for sg in (-1.0, 1.0):
            h = min(sg * (pc[f] + s * dl[f]) - e[f] for s in (lo, hi))
            if h > 0 and h - dist <= 2e-6:
                n = box.R[:, f] * sg                     # box -> capsule
                out.append(n if a.type == BOX else -n)
    return out


def reach(s):
    return float(s.h[0] if s.type == SPHERE else (s.h[0] + s.h[1] if s.type == CAPSULE else np.linalg.norm(s.h)))


# ------------------------------------------------------------------------------------------------ generators
def quat_y_to(v, rng=None):
    """quaternion [i, j, k, w] turning the y axis onto unit vector v (times a random spin about y first)"""
    y = np.array([0.0, 1.0, 0.0])
    c = float(y @ v)
    if c < -1.0 + 1e-12:
        q = np.array([1.0, 0.0, 0.0, 0.0])
    else:
        ax = np.cross(y, v)
        q = np.array([ax[0], ax[1], ax[2], 1.0 + c])
        q /= np.linalg.norm(q)
    if rng is not None:
        a = rng.uniform(0, 2 * np.pi)
        i, j, k, w = q
        sj, sw = np.sin(a / 2), np.cos(a / 2)   # q * (0, sj, 0, sw)
        q = np.array([i * sw - k * sj, j * sw + w * sj, k * sw + i * sj, w * sw - j * sj])
    return q


def _unit(v):
    return v / np.linalg.norm(v)


def _rand_dir(rng):
    return _unit(rng.normal(size=3))


def _perp(rng, v):
    return _unit(np.cross(v, _rand_dir(rng)))


def _sizes(rng, t):
    if t == SPHERE:
        r = rng.uniform(0.3, 1.0)
        return np.array([r, r, r])
    if t == BOX:
        return rng.uniform(0.4, 1.2, size=3)
    return np.array([rng.uniform(0.2, 0.7), rng.uniform(0.05, 1.2), 0.0])


def _support(t, R, h, d):
    if t == SPHERE:
        return h[0]
    if t == BOX:
        return float(h @ np.abs(R.T @ d))
    return float(h[0] + h[1] * abs(R[:, 1] @ d))


def _touch(rng, a, b, d):
    """b moved along d to where the float64 gap is the margin, scattered +-0.03 (bisection on the distance)"""
    target = MARGIN + rng.uniform(-0.03, 0.03)
    lo, hi = 0.0, reach(a) + reach(b) + 0.2
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if pair_gap(a, Shape(b.type, a.c + d * mid, b.R, b.h))[0] < target:
            lo = mid
        else:
            hi = mid
    return a.c + d * hi


def _special(kind, rng, cls, a, hb):
    """An awkward pose of the second shape (half extents hb, may be changed) for the first shape a: (centre, quaternion,
    half extents), or None for the generic pose. cls in 0..11 picks the pose."""
    t1, t2 = KINDS[kind]
    sg = rng.choice([-1.0, 1.0])
    if kind == "BC":
        e, R = a.h, a.R
        f = int(rng.integers(3))
        j, l = (f + 1) % 3, (f + 2) % 3
        nf = np.zeros(3); nf[f] = sg
        r, hl = hb[0], hb[1]
        ang = rng.uniform(0, np.pi)
        inplane = np.zeros(3); inplane[j], inplane[l] = np.cos(ang), np.sin(ang)
        off = np.zeros(3); off[j], off[l] = rng.uniform(-1.3, 1.3) * e[j], rng.uniform(-1.3, 1.3) * e[l]
        height = e[f] + r + rng.uniform(-0.3 * r, 0.05)
        if cls in (0, 1, 2):      # lying on a face: parallel to it (0, 1), 1 along an edge direction; nearly parallel (2)
            if cls == 1:
                inplane = np.zeros(3); inplane[j] = 1.0
            if cls == 2:
                inplane = _unit(inplane + nf * rng.uniform(-0.03, 0.03))
            if rng.random() < 0.6:  # wholly over the face rectangle
                lim_j, lim_l = e[j] - hl * abs(inplane[j]) - 0.01, e[l] - hl * abs(inplane[l]) - 0.01
                if lim_j > 0 and lim_l > 0:
                    off[j], off[l] = rng.uniform(-lim_j, lim_j), rng.uniform(-lim_l, lim_l)
            return nf * height + off, inplane, hb
        if cls == 3:              # parallel to a box edge and next to it, diagonally off the edge
            ax = np.zeros(3); ax[f] = 1.0
            out = np.zeros(3); a_ = rng.uniform(0, np.pi / 2); out[j], out[l] = np.cos(a_), np.sin(a_)
            s2 = rng.choice([-1.0, 1.0], size=2)
            out[j] *= s2[0]; out[l] *= s2[1]
            corner = np.zeros(3); corner[j], corner[l] = s2[0] * e[j], s2[1] * e[l]
            tilt = _rand_dir(rng) * (rng.uniform(0, 0.02) if rng.random() < 0.5 else 0.0)
            return corner + out * (r + rng.uniform(-0.3 * r, 0.05)) + ax * rng.uniform(-1, 1) * e[f], _unit(ax + tilt), hb
        if cls == 4:              # zero-length capsule, generic pose
            hb[1] = 0.0
            return None
        if cls == 5:              # standing on an end on a face
            return nf * (e[f] + hl + r + rng.uniform(-0.3 * r, 0.05)) + off * 0.6, nf, hb
        if cls in (6, 7, 8):      # core through the box centre, leaving through a face (6), an edge (7), a corner (8)
            if cls == 6:
                v = nf
            elif cls == 7:
                v = np.zeros(3); v[j], v[l] = e[j] * sg, e[l] * rng.choice([-1.0, 1.0])
            else:
                v = e * rng.choice([-1.0, 1.0], size=3)
            v = _unit(v)
            hb[1] = rng.uniform(0.4, 1.2)
            return v * rng.uniform(0.0, 1.0) * np.linalg.norm(e) + rng.normal(size=3) * 0.02, v, hb
        return None
    if kind == "CC":
        ca, ua, ha, ra = core(a)
        r, hl = hb[0], hb[1]
        if cls in (0, 1, 2, 3):   # side by side: parallel (0, 1), nearly parallel on both sides of sin^2 = 1e-4 (2, 3)
            v = ua * sg
            if cls >= 2:
                v = _unit(v + _perp(rng, ua) * 10 ** rng.uniform(-3.0, -1.5))
            side = _perp(rng, ua)
            return ua * rng.uniform(-1.2, 1.2) * (ha + hl) + side * (ra + r + rng.uniform(-0.3 * min(ra, r), 0.05)), v, hb
        if cls == 4:              # a zero-length capsule
            hb[1] = 0.0
            return None
        if cls == 5:              # collinear, end to end or overlapping
            return ua * sg * (ha + hl + (ra + r) * rng.uniform(0.5, 1.2)), ua, hb
        if cls == 6:              # crossing at right angles, close
            v = _perp(rng, ua)
            w = np.cross(ua, v)
            return ua * rng.uniform(-1, 1) * ha + w * (ra + r + rng.uniform(-0.3 * min(ra, r), 0.05)), v, hb
        return None
    if kind == "SC":
        r, hl = hb[0], hb[1]
        ra = a.h[0]
        v = _rand_dir(rng)
        if cls in (0, 1):         # the sphere beside the cylinder part
            return _perp(rng, v) * (ra + r + rng.uniform(-0.3 * min(ra, r), 0.05)) + v * rng.uniform(-1, 1) * hl, v, hb
        if cls == 2:              # at an end cap, on the axis
            return v * (hl + ra + r + rng.uniform(-0.3 * min(ra, r), 0.05)), v, hb
        if cls == 3:
            hb[1] = 0.0
            return None
        return None
    if kind == "SB":
        e = hb
        if cls in (0, 1):         # the sphere's centre inside the box
            return rng.uniform(-1, 1, size=3) * e * 0.95, None, hb
        if cls in (2, 3, 4):      # near a face (2), an edge (3), a corner (4), expressed in the box frame
            v = np.zeros(3)
            axes = rng.permutation(3)[: cls - 1]
            v[axes] = rng.choice([-1.0, 1.0], size=len(axes))
            p = v * e + rng.uniform(-0.5, 0.5, size=3) * e * (v == 0)
            return p + _unit(v) * (a.h[0] + rng.uniform(-0.3 * a.h[0], 0.05)), None, hb
        return None
    return None


Scene = namedtuple("Scene", "kind n types pos rot he")  # pos (n, 2, 3), rot (n, 2, 4), he (n, 2, 3): float32


def scene(kind, n_pairs, seed):
    """n_pairs isolated pairs of the kind on pair_base's lattice: the first shape at the lattice point, the second from
    deep overlap to clear separation along a random direction; every 20 pairs hold the 12 awkward poses of the kind and one
    pair touching at the margin +-0.03."""
    rng = np.random.default_rng(seed)
    t1, t2 = KINDS[kind]
    if kind == "BB":
        pos, rot, _, he = _box_pairs(rng, n_pairs)
        return Scene(kind, n_pairs, (t1, t2), pos.reshape(n_pairs, 2, 3), rot.reshape(n_pairs, 2, 4), he.reshape(n_pairs, 2, 3))
    pos = np.zeros((n_pairs, 2, 3))
    rot = np.zeros((n_pairs, 2, 4))
    he = np.zeros((n_pairs, 2, 3))
    for k in range(n_pairs):
        base = pair_base(k, n_pairs)
        ha, hb = _sizes(rng, t1), _sizes(rng, t2)
        qa = random_quats(rng, 1)[0].astype(np.float64)
        if rng.random() < 0.2:
            qa = np.array([0.0, 0.0, 0.0, 1.0])
        qb = random_quats(rng, 1)[0].astype(np.float64)
        a = Shape(t1, base, quat_to_matrix(qa), ha)
        cls = k % 20
        sp = _special(kind, rng, cls, a, hb) if cls < 12 else None
        if sp is not None:
            p, v, hb = sp
            if kind == "SB":   # p: the sphere's centre in the frame of the box (the second shape)
                cb = base - quat_to_matrix(qb) @ p
            else:              # p, v: the second shape's centre and axis in the frame of the first
                cb = base + a.R @ p
                qb = quat_y_to(a.R @ v, rng)
        else:
            d = _rand_dir(rng)
            b0 = Shape(t2, base, quat_to_matrix(qb), hb)
            if cls == 19:
                cb = _touch(rng, a, b0, d)
            else:
                cb = base + d * (_support(t1, a.R, ha, d) + _support(t2, b0.R, hb, d)) * rng.uniform(0.5, 1.25)
        pos[k], rot[k], he[k] = (base, cb), (qa, qb), (ha, hb)
    return Scene(kind, n_pairs, (t1, t2), pos.astype(np.float32), rot.astype(np.float32), he.astype(np.float32))


def arrange(sc, order):
    """World arrays of the scene's pairs as bodies 2k, 2k + 1 - "ab": first, second shape; "ba": second, first - with the
    Shape lists in manifold order (A = the lower index) and the manifold key of each pair."""
    i, j = (0, 1) if order == "ab" else (1, 0)
    n = sc.n
    pos = np.empty((2 * n, 3), np.float32); pos[0::2], pos[1::2] = sc.pos[:, i], sc.pos[:, j]
    rot = np.empty((2 * n, 4), np.float32); rot[0::2], rot[1::2] = sc.rot[:, i], sc.rot[:, j]
    he = np.empty((2 * n, 3), np.float32); he[0::2], he[1::2] = sc.he[:, i], sc.he[:, j]
    st = np.empty(2 * n, np.uint32); st[0::2], st[1::2] = sc.types[i], sc.types[j]
    A = shapes(sc.types[i], sc.pos[:, i], sc.rot[:, i], sc.he[:, i])
    B = shapes(sc.types[j], sc.pos[:, j], sc.rot[:, j], sc.he[:, j])
    return dict(pos=pos, rot=rot, shape=st, he=he, A=A, B=B, keys=[(2 * k, 2 * k + 1) for k in range(n)])


def arrange_static(sc, order):
    """The same pairs with the manifold's B as static collider k and its A as body k ("ab": the second shape is static)."""
    i, j = (0, 1) if order == "ab" else (1, 0)
    body = dict(pos=sc.pos[:, i].copy(), rot=sc.rot[:, i].copy(), shape=np.full(sc.n, sc.types[i], np.uint32), he=sc.he[:, i].copy())
    static = dict(pos=sc.pos[:, j].copy(), rot=sc.rot[:, j].copy(), shape=np.full(sc.n, sc.types[j], np.uint32), he=sc.he[:, j].copy())
    A = shapes(sc.types[i], sc.pos[:, i], sc.rot[:, i], sc.he[:, i])
    B = shapes(sc.types[j], sc.pos[:, j], sc.rot[:, j], sc.he[:, j])
    return dict(body=body, static=static, A=A, B=B, keys=[(k, STATIC_ID_BIT | k) for k in range(sc.n)])


def ground_scene(gkind, n, seed):
    """n bodies of one shape over the plane y = 0 on a grid 8 apart, the lowest point from 0.25 below to 0.2 above it.
    Capsules: every 10 hold a lying one, a standing one, a nearly lying one, a zero-length one; boxes: two flat ones; one
    of every 10 of any shape touches at the margin +-0.03."""
    rng = np.random.default_rng(seed)
    t = GROUND_KINDS[gkind]
    pos = np.zeros((n, 3)); rot = np.zeros((n, 4)); he = np.zeros((n, 3))
    side = int(np.ceil(np.sqrt(n)))
    for k in range(n):
        h = _sizes(rng, t)
        q = random_quats(rng, 1)[0].astype(np.float64)
        cls = k % 10
        if t == CAPSULE:
            flat = np.array([np.cos(cls + k), 0.0, np.sin(cls + k)])
            if cls == 0:
                q = quat_y_to(flat, rng)
            elif cls == 1:
                q = np.array([0.0, 0.0, 0.0, 1.0])
            elif cls == 2:
                q = quat_y_to(_unit(flat + np.array([0.0, rng.uniform(-0.03, 0.03), 0.0])), rng)
            elif cls == 3:
                h[1] = 0.0
        elif t == BOX and cls in (0, 1):
            q = np.array([0.0, 0.0, 0.0, 1.0])
        s0 = Shape(t, np.zeros(3), quat_to_matrix(q.astype(np.float32).astype(np.float64)), h)
        lift = MARGIN + rng.uniform(-0.03, 0.03) if cls == 9 else rng.uniform(-0.25, 0.2)
        pos[k] = ((k % side - 0.5 * side) * 8.0, lift - plane_gap(s0), (k // side - 0.5 * side) * 8.0)
        rot[k], he[k] = q, h
    pos, rot, he = pos.astype(np.float32), rot.astype(np.float32), he.astype(np.float32)
    return dict(pos=pos, rot=rot, shape=np.full(n, t, np.uint32), he=he, A=shapes(t, pos, rot, he),
                keys=[(k, GROUND) for k in range(n)])


# ------------------------------------------------------------------------------------------------ the checks
class Report:
    def __init__(self, what):
        self.what, self.failures = what, []
        self.n = self.hits = self.misses = self.skipped = self.excepted = 0
        self.worst = {}   # figure -> worst value seen (printed by the tests before they assert)
        self.counts = {}  # regime -> pairs that reached it

    def fail(self, k, msg):
        self.failures.append(f"{self.what} pair {k}: {msg}")

    def see(self, name, value):
        self.worst[name] = max(self.worst.get(name, 0.0), float(value))

    def count(self, name):
        self.counts[name] = self.counts.get(name, 0) + 1

    def summary(self):
        w = ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items()))
        c = ", ".join(f"{k} {v}" for k, v in sorted(self.counts.items()))
        return (f"{self.what}: {self.n} pairs, {self.hits} contacts, {self.misses} misses, {self.skipped} skipped, "
                f"{self.excepted} under an exception; "
                f"worst: {w}; regimes: {c}; {len(self.failures)} failures")

    def assert_ok(self, shares=True):
        print(self.summary())
        assert not self.failures, f"{len(self.failures)} failures, the first: " + " | ".join(self.failures[:5])
        if shares:
            assert self.skipped + self.excepted <= MAX_SKIPPED * self.n, self.summary()
            assert self.hits >= MIN_CONTACTS * self.n and self.misses >= MIN_MISSES * self.n, self.summary()


def manifolds_of(world):
    """{(a, b): (count, normal, points[count, 4])} in float64 from get_manifolds() of a world or an oracle world"""
    ids, counts, normals, points = world.get_manifolds()
    return {(int(a), int(b)): (int(c), n.astype(np.float64), p[:int(c)].astype(np.float64))
            for (a, b), c, n, p in zip(ids, counts, normals, points)}


def _box_existence(a, b, got, rep, k):
    """Existence for two boxes, as test_box_box_manifolds_against_brute_force_sat states it. Returns "miss", "skip",
    "hit" (a manifold to check further)."""
    s_star, seps = sat_separation(a.c, a.R, a.h, b.c, b.R, b.h)
    if s_star > MARGIN + BAND:
        if got is not None:
            rep.fail(k, f"separated by {s_star:.5f} along a SAT axis, yet a manifold")
        return "miss"
    band = s_star > MARGIN - BAND
    if got is None:
        if band:
            return "skip"
        s_all, _ = sat_separation(a.c, a.R, a.h, b.c, b.R, b.h, min_cross=1e-6)
        if s_all > MARGIN - BAND:
            return "skip"
        slivers = [lab for lab, fp in sliver_readings(a.c, a.R, a.h, b.c, b.R, b.h, seps, s_star)
                   if fp is None or (fp[0] < SLIVER_REL * fp[1] + 1e-3 and fp[2] <= SLIVER_DEPTH + 1e-4)]
        if not slivers:
            rep.fail(k, f"no separating axis (max separation {s_all:.5f}), no sliver reading, yet no manifold")
        rep.count("sliver")
        return "skip"
    return "skip+" if band else "hit"


def check(kind, A, B, keys, man, what=None):
    """Every check of the module docstring on the manifolds `man` of the pairs (A[k], B[k]) with id pairs keys[k]."""
    rep = Report(what or kind)
    rep.n = len(A)
    wanted = set(keys)
    for key in man:
        if key not in wanted:
            rep.fail(-1, f"a manifold {key} that joins no pair of the scene (or has its ids out of order)")
    tol_push = TOL_PUSH[kind]
    for k, (a, b) in enumerate(zip(A, B)):
        got = man.get(keys[k])
        if kind == "BB":
            state = _box_existence(a, b, got, rep, k)
            gap, n_ref, cdist = pair_gap(a, b)
            if state == "miss":
                rep.misses += 1
                continue
            if state.startswith("skip"):
                rep.skipped += 1
                if got is None:
                    continue
            else:
                rep.hits += 1
        else:
            gap, n_ref, cdist = pair_gap(a, b)
            if gap > MARGIN + BAND:
                rep.misses += 1
                if got is not None:
                    rep.fail(k, f"gap {gap:.5f} beyond the margin, yet a manifold")
                continue
            if gap > MARGIN - BAND:
                rep.skipped += 1
                if got is None:
                    continue
            else:
                rep.hits += 1
                if got is None:
                    rep.fail(k, f"gap {gap:.5f} inside the margin, no manifold")
                    continue
        count, normal, pts = got
        max_pts = 1 if SPHERE in (a.type, b.type) else (2 if CAPSULE in (a.type, b.type) else 4)
        if not 1 <= count <= max_pts:
            rep.fail(k, f"{count} points (at most {max_pts})")
            continue
        depth = pts[:, 3]
        deepest = float(depth.max())
        # the normal is a unit vector
        rep.see("|normal| - 1", abs(np.linalg.norm(normal) - 1.0))
        if abs(np.linalg.norm(normal) - 1.0) > TOL:
            rep.fail(k, f"normal {normal} is not a unit vector")
        sin2 = cores_sin2(a, b)
        par = sin2 <= PAR_SIN2 + PAR_BAND
        sin = np.sqrt(max(sin2, 0.0)) if par else 0.0
        span = reach(a) + reach(b)
        tol_n = TOL + 2 * sin
        tol_d = TOL + 2 * sin * sin * span
        if kind == "BC":
            # near-parallel exception of a core and a box edge: the core point may sit hl x sin from the closest one
            slack = edge_parallel_slack(a, b)
            par = slack > 0
            tol_d, tol_n, tol_push = TOL + slack, TOL + slack / max(cdist, 1e-9), TOL_PUSH[kind] + slack
        if par:
            rep.excepted += 1
        if kind != "BB":
            if gap > 0:
                # apart, inside the margin: the closest direction and the distance
                rep.count("apart")
                err_n, err_d = np.abs(normal - n_ref).max(), abs(deepest + gap)
                if kind == "BC" and err_n > tol_n:
                    faces = face_readings(a, b, cdist)
                    if faces:
                        rep.count("apart: face reading within 2e-6 of the distance")
                        err_n = min(np.abs(normal - n).max() for n in faces)
                rep.see("apart: normal" + (" (near-parallel)" if par else ""), err_n)
                rep.see("apart: depth" + (" (near-parallel)" if par else ""), err_d)
                rep.see("apart: depth + gap, signed low" + (" (near-parallel)" if par else ""), -(deepest + gap))
                if err_n > tol_n:
                    rep.fail(k, f"apart by {gap:.5f}: normal {normal} vs the closest direction {n_ref}")
                if err_d > tol_d:
                    rep.fail(k, f"apart by {gap:.5f}: deepest depth {deepest:.6f}")
            elif kind != "BC" and cdist > 1e-6:
                # overlapping, closed form: penetration = radii - core distance (sphere in a box: radius + nearest face)
                rep.count("overlap, closed form")
                err_d = abs(deepest + gap)
                rep.see("overlap: depth" + (" (near-parallel)" if par else ""), err_d)
                if err_d > tol_d:
                    rep.fail(k, f"penetration {-gap:.6f}, deepest depth {deepest:.6f}")
            elif kind == "SB" and cdist == 0.0:
                rep.count("overlap, centre inside")
                rep.see("overlap: depth", abs(deepest + gap))
                if abs(deepest + gap) > TOL:
                    rep.fail(k, f"centre inside the box: penetration {-gap:.6f}, deepest depth {deepest:.6f}")
        if gap < 0:
            # push-out: B moved along the normal by the deepest depth leaves no overlap (a flipped normal deepens it)
            rep.count("overlap")
            left = pair_gap(a, moved(b, normal * deepest))[0]
            rep.see("push-out residual" + (" (near-parallel)" if par else ""), -left)
            if left < -tol_push:
                rep.fail(k, f"gap {gap:.5f}: after moving B by normal x {deepest:.5f} the gap is {left:.5f}")
        # point counts
        if SPHERE in (a.type, b.type):
            pass  # one point: max_pts above
        elif kind == "BC":
            cap, box = (a, b) if a.type == CAPSULE else (b, a)
            want2 = _lies_on_a_face(cap, box)
            if want2:
                rep.count("two points on a face")
                if count != 2:
                    rep.fail(k, f"both core ends over a face within the margin, {count} point(s)")
        elif kind == "CC" and (sin2 < PAR_SIN2 - PAR_BAND or sin2 > PAR_SIN2 + PAR_BAND):
            want = _cc_rule(a, b)
            if want is not None:
                rep.count("capsule rule: %d point(s)" % want)
                if count != want:
                    rep.fail(k, f"the capsule-capsule rule gives {want} point(s), the manifold has {count}")
        # every point near both surfaces
        for p, dep in zip(pts[:, :3], depth):
            far = max(surface_dist(p, a), surface_dist(p, b)) - (abs(dep) + MARGIN)
            rep.see("point off the surfaces", max(far, 0.0))
            if far > TOL:
                rep.fail(k, f"point {p} (depth {dep:.5f}) lies {far + abs(dep) + MARGIN:.5f} from a shape")
    return rep


def _lies_on_a_face(cap, box):
    """Both core ends outside one face of the box, over its rectangle and within the margin of it, each by more than the
    band; the core has a length."""
    c, u, hl, r = core(cap)
    if hl <= 0:
        return False
    ends = [box.R.T @ (c + s * u - box.c) for s in (-hl, hl)]
    for f in range(3):
        for sg in (-1.0, 1.0):
            ok = True
            for p in ends:
                hgt = sg * p[f] - box.h[f]
                over = all(abs(p[j]) < box.h[j] - BAND for j in range(3) if j != f)
                ok = ok and over and BAND < hgt < r + MARGIN - BAND
            if ok:
                return True
    return False


def _cc_rule(a, b):
    """Point count of two capsules by the spec's documented rule, restated in float64 (capsule_ref.capsule_capsule): two
    where the cores are parallel (sin^2 <= 1e-4) and their projections overlap by more than the band, with both ends of
    the overlap inside the margin; None where a depth or the overlap sits inside the band."""
    ca, ua, ha, ra = core(a)
    cb, ub, hb, rb = core(b)
    if ha == 0 or hb == 0 or cores_sin2(a, b) > PAR_SIN2:
        return 1
    d = cb - ca
    sb, pb = d @ ua, hb * abs(ua @ ub)
    lo, hi = max(-ha, sb - pb), min(ha, sb + pb)
    if abs(hi - lo) < BAND:
        return None
    if lo > hi:
        return 1
    perp = d - ua * sb
    if np.linalg.norm(perp) < 1e-6:
        return None
    n = perp / np.linalg.norm(perp)
    inside = 0
    for s in (lo, hi):
        pa = ca + s * ua
        qb = cb + cref.closest_param(cb, ub, hb, pa) * ub
        dep = ra + rb - (qb - pa) @ n
        if abs(dep + MARGIN) < BAND:
            return None
        inside += dep > -MARGIN
    return inside if inside else None


def check_ground(gkind, A, keys, man, what=None):
    """Bodies over the plane y = 0: existence, ids (body, GROUND), normal (0, -1, 0), deepest depth = -(lowest point),
    point counts (sphere 1; capsule one per core end inside the margin; box one per vertex, at most 4), points between the
    body's lowest point and the plane."""
    rep = Report(what or "ground " + gkind)
    rep.n = len(A)
    wanted = set(keys)
    for key in man:
        if key not in wanted:
            rep.fail(-1, f"a manifold {key} that is no (body, ground) pair of the scene")
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    for k, a in enumerate(A):
        got = man.get(keys[k])
        gap = plane_gap(a)
        if gap > MARGIN + BAND:
            rep.misses += 1
            if got is not None:
                rep.fail(k, f"lowest point {gap:.5f} above the plane, yet a manifold")
            continue
        if gap > MARGIN - BAND:
            rep.skipped += 1
            if got is None:
                continue
        else:
            rep.hits += 1
            if got is None:
                rep.fail(k, f"lowest point {gap:.5f} above the plane, no manifold")
                continue
        count, normal, pts = got
        if np.abs(normal - (0.0, -1.0, 0.0)).max() > 1e-6:
            rep.fail(k, f"normal {normal}: A = body, B = ground gives (0, -1, 0)")
        deepest = float(pts[:, 3].max()) if count else -np.inf
        rep.see("depth", abs(deepest + gap))
        if abs(deepest + gap) > TOL:
            rep.fail(k, f"lowest point {gap:.6f}, deepest depth {deepest:.6f}")
        if a.type == SPHERE:
            lows = np.array([gap])
        elif a.type == CAPSULE:
            c, u, hl, r = core(a)
            lows = np.array([c[1] - hl * u[1] - r, c[1] + hl * u[1] - r]) if hl > 0 else np.array([gap])
        else:
            lows = (a.c + (corners * a.h) @ a.R.T)[:, 1]
        sure, maybe = int((lows < MARGIN - BAND).sum()), int((lows < MARGIN + BAND).sum())
        if a.type == CAPSULE and len(lows) == 2 and sure == 2:
            rep.count("two points")
        if not min(4, sure) <= count <= min(4, maybe):
            rep.fail(k, f"{count} point(s), {sure}..{maybe} lowest points inside the margin")
        for p in pts:
            off = max(surface_dist(p[:3], a), abs(p[1])) - (abs(p[3]) + MARGIN)
            rep.see("point off the surfaces", max(off, 0.0))
            if off > TOL:
                rep.fail(k, f"point {p[:3]} (depth {p[3]:.5f}) away from the body or the plane")
    return rep


def _match_points(p1, p2):
    """worst coordinate / depth difference of two point sets under the best assignment (<= 2 points each)"""
    best = np.inf
    for perm in itertools.permutations(range(len(p2))):
        best = min(best, float(np.abs(p1 - p2[list(perm)]).max()))
    return best


def check_symmetry(kind, ab, man_ab, ba, man_ba, what=None):
    """The same geometry with the two bodies' indices exchanged: the same points and depths, the normal negated. Pairs
    whose swap goes through the dispatcher (the capsule, or the sphere against a box, is always tested as A) run the same
    arithmetic: equal to 1e-6. Two spheres or two capsules run it from the other side: TOL, plus for two capsules the
    conditioning of the closest points, 1e-6 / sin^2 (their parameters are a quotient by sin^2 of sums of ~4 products of
    size <= 4, each rounded to 6e-8), and the near-parallel exception of the module docstring. Two boxes are not
    symmetric by definition (the faces of A are preferred as reference) and are left out: each order is checked on its own."""
    rep = Report(what or kind + " order symmetry")
    rep.n = len(ab["A"])
    if kind == "BB":
        return rep
    same_code = kind in ("SB", "SC", "BC")
    for k in range(rep.n):
        m1, m2 = man_ab.get(ab["keys"][k]), man_ba.get(ba["keys"][k])
        if (m1 is None) != (m2 is None):
            if same_code or abs(pair_gap(ab["A"][k], ab["B"][k])[0] - MARGIN) > BAND:
                rep.fail(k, "a manifold in one index order only")
            rep.skipped += 1
            continue
        if m1 is None:
            rep.misses += 1
            continue
        rep.hits += 1
        tol_n = tol_p = tol_d = 1e-6
        if not same_code:
            a, b = ab["A"][k], ab["B"][k]
            sin2 = cores_sin2(a, b)
            span = reach(a) + reach(b)
            tol_n = tol_d = TOL
            tol_p = TOL + 1e-6 / max(sin2, PAR_SIN2)
            if sin2 <= PAR_SIN2 + PAR_BAND:
                sin = np.sqrt(max(sin2, 0.0))
                tol_n, tol_d, tol_p = TOL + 2 * sin, TOL + 2 * sin * sin * span, TOL + 2 * sin * span
        if m1[0] != m2[0]:
            rep.fail(k, f"{m1[0]} point(s) in one order, {m2[0]} in the other")
            continue
        err_n = np.abs(m1[1] + m2[1]).max()
        err_p = _match_points(m1[2][:, :3], m2[2][:, :3])
        err_d = _match_points(np.sort(m1[2][:, 3:], axis=0), np.sort(m2[2][:, 3:], axis=0))
        rep.see("normal", err_n); rep.see("points", err_p); rep.see("depths", err_d)
        if err_n > tol_n or err_p > tol_p or err_d > tol_d:
            rep.fail(k, f"orders differ: normal by {err_n:.2e}, points by {err_p:.2e}, depths by {err_d:.2e}")
    return rep


def check_same(man1, keys1, man2, keys2, what):
    """Two runs of the same collide call (B as a static collider / as a body): identical manifolds, bit for bit."""
    rep = Report(what)
    rep.n = len(keys1)
    for k, (k1, k2) in enumerate(zip(keys1, keys2)):
        m1, m2 = man1.get(k1), man2.get(k2)
        if (m1 is None) != (m2 is None):
            rep.fail(k, "a manifold on one path only")
        elif m1 is None:
            rep.misses += 1
        else:
            rep.hits += 1
            if m1[0] != m2[0] or not np.array_equal(m1[1], m2[1]) or not np.array_equal(m1[2], m2[2]):
                rep.fail(k, f"the two paths differ: {m1} vs {m2}")
    return rep
