"""The seeded scenes and capsules of the depenetration tests, with the float64 reference of every capsule (tests/depen_ref.py):
its probe where it starts and its whole push-out loop, computed once per process and shared, unchanged, by
tests/test_depen_cpu.py (which counts the reference's own near ties) and tests/test_gpu_depen.py. numpy and the references only.

The scenes are slide_cases' (the soup of 300 bodies of all shapes and NONE with four statics and the ground; the same without
bodies; an empty world). Four in five capsules are placed ON a target: the centre at a point of its surface, moved along a random
direction by up to the capsule's radius, so that most overlap something; the rest lie anywhere in the scene's volume and mostly
start clear. A tenth are balls (h = 0), a tenth segments (R = 0).

A case: dict(label, bodies, statics, ground, tg, frames, pos, rot, a, rad, hq, skin, max_iters, near (per query: the rows of tg a
push-out can reach), first (id, depth, normal, second depth, inside at pos), out (p, status, slots))."""
import functools

import numpy as np

import capsulecast_cases as cc
import depen_ref as ref
import slide_cases
from capsulecast_ref import query_ref, rotation_matrices

SKIN = 0.02
MAX_ITERS = 8
SCENES = slide_cases.SCENES
N = 600
EXTENT = slide_cases.EXTENT
REACH = 6.0  # no loop of 8 pushes out of these targets (extents <= 1.2, statics apart) carries a capsule further


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def tol_of(pos, hq):
    """capsulecast_accept.tol_of for a query that does not move: 1e-5 (1 + |pos|_inf + h)"""
    return 1e-5 * (1.0 + float(np.abs(pos).max()) + float(hq))


def _surface_points(rng, tg, ground, n):
    """n points on the surfaces of randomly chosen targets (a fifth of them on the ground, where there is one)"""
    shaped = np.nonzero(np.isin(tg["shape"], (1, 2, 3)))[0] if len(tg["pos"]) else np.zeros(0, np.int64)
    out = np.zeros((n, 3))
    R = query_ref._frames(tg) if len(tg["pos"]) else None
    for i in range(n):
        if len(shaped) == 0 or (ground is not None and rng.random() < 0.2):
            out[i] = (rng.uniform(-EXTENT, EXTENT), 0.0 if ground is None else ground, rng.uniform(-EXTENT, EXTENT))
            continue
        k = shaped[rng.integers(len(shaped))]
        he, s = tg["half_extent"][k], tg["shape"][k]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if s == 1:
            out[i] = tg["pos"][k] + he[0] * u
        elif s == 3:
            out[i] = tg["pos"][k] + R[k][:, 1] * rng.uniform(-he[1], he[1]) + he[0] * u
        else:
            l = rng.uniform(-1.0, 1.0, 3) * he
            f = rng.integers(3)
            l[f] = he[f] * (1.0 if rng.random() < 0.5 else -1.0)
            out[i] = tg["pos"][k] + R[k] @ l
    return out


def capsules(rng, n, tg, ground):
    f = np.float32
    rot = cc.quats(rng, n)
    rad = rng.uniform(0.1, 0.5, n).astype(f)
    hq = rng.uniform(0.2, 1.0, n).astype(f)
    kind = rng.random(n)
    hq[kind < 0.1] = 0.0
    rad[kind > 0.9] = 0.0
    on = rng.random(n) < 0.8
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = _surface_points(rng, tg, ground, n) + u * (rng.uniform(-1.0, 1.0, n) * rad)[:, None]
    free = rng.uniform([-EXTENT, 0.5, -EXTENT], [EXTENT, EXTENT, EXTENT], (n, 3))
    pos = np.where(on[:, None], pos, free).astype(f)
    return pos, rot, rad, hq


def reference(pos, rot, rad, hq, tg, ground, skin, max_iters):
    """per query: its near rows of tg, the probe at pos, the whole loop"""
    n = len(pos)
    frames = query_ref._frames(tg)
    a = np.tile([0.0, 1.0, 0.0], (n, 1)) if rot is None else rotation_matrices(np.asarray(rot, np.float64))[:, :, 1]
    bound = query_ref._bound(tg["half_extent"], tg["shape"]) if len(tg["pos"]) else np.zeros(0)
    near, first, out = [], [], []
    for i in range(n):
        p = pos[i].astype(np.float64)
        rows = np.nonzero(np.linalg.norm(tg["pos"] - p, axis=1) - bound - (rad[i] + hq[i]) < REACH)[0] if len(bound) else np.zeros(0, np.int64)
        sub = {k: v[rows] for k, v in tg.items()}
        near.append(rows)
        first.append(ref.deepest(p, a[i], float(rad[i]), float(hq[i]), sub, ground, skin, frames_=frames[rows]))
        out.append(ref.depenetrate(p, a[i], float(rad[i]), float(hq[i]), sub, ground, skin, max_iters, frames_=frames[rows]))
    return a, frames, near, first, out


@functools.lru_cache(maxsize=None)
def case(name, n=N):
    bodies, statics, ground = slide_cases.scene(name)
    tg = query_ref.targets(bodies, statics)
    rng = np.random.default_rng(5200 + SCENES.index(name))
    pos, rot, rad, hq = capsules(rng, n, tg, ground)
    a, frames, near, first, out = reference(pos, rot, rad, hq, tg, ground, SKIN, MAX_ITERS)
    return _frozen(dict(label=f"depen {name}", bodies=bodies, statics=statics, ground=ground, tg=tg, frames=frames, pos=pos, rot=rot, a=a,
                        rad=rad, hq=hq, skin=SKIN, max_iters=MAX_ITERS, near=near, first=first, out=out))


def all_cases():
    yield from (case(s) for s in SCENES)


def near_ties(c):
    """how many queries have a second target within the tolerance of the deepest: where float32 may rightly report the other id"""
    return sum(1 for i, (_, d, _, d2, _) in enumerate(c["first"]) if np.isfinite(d2) and d - d2 < tol_of(c["pos"][i], c["hq"][i]))


def probe_targets(tg):
    """tg (query_ref.targets) as the explicit list tests/depen_probe.py takes: float32, ascending ids"""
    return dict(id=tg["id"].astype(np.uint32), shape=tg["shape"].astype(np.uint32), pos=tg["pos"].astype(np.float32),
                rot=tg["rot"].astype(np.float32), half_extent=tg["half_extent"].astype(np.float32))
