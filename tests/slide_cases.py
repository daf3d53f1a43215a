"""The seeded scenes and characters of the move-and-slide tests, with the float64 capsule cast of every character along the
motion it asks for (tests/capsulecast_ref.py), computed once per process and shared, unchanged, by tests/test_slide_cpu.py
(which counts the reference's own near ties) and tests/test_gpu_slide.py. numpy and the references only.

A case: dict(label, bodies, statics, ground, tg, pos, motion, rot, rad, hq, skin, h): h the reference's cast from pos along
motion with no max_t."""
import functools

import numpy as np

import capsulecast_cases as cc
import capsulecast_ref as ref
import query_ref
from raycast_ref import rotation_matrices

SKIN = 0.02
SCENES = ("soup", "statics", "empty")
N = 600
EXTENT = 15.0


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def separation(pos, rot, rad, hq, tg, ground):
    """float64: the least separation of each capsule (rows) from every target and the ground (exact where it is below 1, a
    lower bound beyond); +inf with neither"""
    n = len(pos)
    pos = np.asarray(pos, np.float64)
    a = rotation_matrices(np.asarray(rot, np.float64))[:, :, 1]
    rad, hq = np.asarray(rad, np.float64), np.asarray(hq, np.float64)
    out = np.full(n, np.inf)
    if ground is not None:
        out = pos[:, 1] - hq * np.abs(a[:, 1]) - rad - ground
    m = len(tg["pos"])
    if m:
        shaped = np.isin(tg["shape"], (query_ref.SHAPE_SPHERE, query_ref.SHAPE_BOX, query_ref.SHAPE_CAPSULE))
        b = query_ref._bound(tg["half_extent"], tg["shape"])
        gap = np.linalg.norm(pos[:, None, :] - tg["pos"][None, :, :], axis=2) - b[None, :] - (rad + hq)[:, None]
        # far pairs need no exact distance: their gap of bounding balls (>= 1) is a lower bound of the separation
        near = (gap < 1.0) & shaped[None, :]
        qi, ti = np.nonzero(near)
        out = np.minimum(out, np.where(shaped[None, :] & ~near, gap, np.inf).min(1))
        if len(qi):
            R = query_ref._frames(tg)
            _, _, d, r = ref.closest(pos[qi], a[qi], hq[qi], tg["pos"][ti], R[ti], tg["half_extent"][ti], tg["shape"][ti])
            np.minimum.at(out, qi, d - r - rad[qi])
    return out


def characters(rng, n, tg, ground, clear):
    """n characters that start at least `clear` away from everything (rejection in float64), a tenth of them balls (h = 0)
    and a tenth segments (R = 0), with motions aimed into the scene"""
    f = np.float32
    got = {k: [] for k in ("pos", "rot", "rad", "hq")}
    have = 0
    while have < n:
        m = 4 * n
        pos = rng.uniform([-EXTENT, 0.0, -EXTENT], [EXTENT, EXTENT, EXTENT], (m, 3)).astype(f)
        rot = cc.quats(rng, m)
        rad = rng.uniform(0.1, 0.5, m).astype(f)
        hq = rng.uniform(0.2, 1.0, m).astype(f)
        kind = rng.random(m)
        hq[kind < 0.1] = 0.0
        rad[kind > 0.9] = 0.0
        keep = separation(pos, rot, rad, hq, tg, ground) >= clear
        for k, v in (("pos", pos), ("rot", rot), ("rad", rad), ("hq", hq)):
            got[k].append(v[keep])
        have += int(keep.sum())
    pos, rot, rad, hq = (np.concatenate(got[k])[:n] for k in ("pos", "rot", "rad", "hq"))
    aim = rng.uniform([-EXTENT, -1.0, -EXTENT], [EXTENT, EXTENT, EXTENT], (n, 3))
    aim[: n // 3, 1] = -1.0  # a third at the ground and the platform on it
    d = aim - pos
    motion = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 10.0, (n, 1))).astype(f)
    return pos, motion, rot, rad, hq


@functools.lru_cache(maxsize=None)
def scene(name):
    """(bodies or None, statics or None, ground height or None)"""
    rng = np.random.default_rng(4100)
    bodies = cc.soup_bodies(rng, 300, EXTENT)
    statics = cc.soup_statics(rng)
    if name == "soup":
        return bodies, statics, 0.0
    if name == "statics":
        return None, statics, 0.0
    return None, None, None


@functools.lru_cache(maxsize=None)
def case(name, n=N):
    bodies, statics, ground = scene(name)
    tg = query_ref.targets(bodies, statics)
    rng = np.random.default_rng(4200 + SCENES.index(name))
    pos, motion, rot, rad, hq = characters(rng, n, tg, ground, SKIN + 0.01)
    h = ref.capsulecast(pos, motion, rot, rad, hq, tg, ground=ground)
    return _frozen(dict(label=f"slide {name}", bodies=bodies, statics=statics, ground=ground, tg=tg, pos=pos, motion=motion, rot=rot,
                        rad=rad, hq=hq, skin=SKIN, h=h))


def all_cases():
    yield from (case(s) for s in SCENES)


# ---- filters and ignore over the soup ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filters():
    """(body categories, static categories, ground category, per-query masks, per-query ignore ids) for case('soup')"""
    rng = np.random.default_rng(4300)
    cat = rng.choice([1, 2, 4], 300).astype(np.uint16)
    scat = np.array([1, 2, 4, 2], np.uint16)
    masks = rng.choice([1, 2, 3, 5, 6, 7], N).astype(np.uint16)
    first = case("soup")["h"]["body"]
    ignore = np.where((first < 300) & (rng.random(N) < 0.7), first, 0xFFFFFFFF).astype(np.uint32)
    return cat, scat, 4, masks, ignore
