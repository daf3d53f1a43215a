"""GPU: continuous collision (phys_set_ccd_bodies, phys_get_ccd_hits) against the library's own statement
of its arithmetic (tests/cpp/ccd_probe.cpp: include/spec/ccd.h compiled by the host compiler) bit for bit, and against what it is
for: a fast body stops at the wall and at the ground it would pass through, and a world that lists nobody - or somebody who hits
nothing - computes the bits it computed before.

List sizes either side of a wave and past several workgroups (1, 63, 64, 65, 257 entries), static counts either side of the
kernel's LDS tile and a tail beyond two tiles (1, 63, 64, 65, 150); with and without filters, the ground, exact rotation. Every
scene has at most a few hundred bodies."""
import functools
import os
import re

import numpy as np
import pytest

import ccd_cases
import ccd_probe
from boxcast_accept import tol_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 16_666_667
DT_S = np.float32(0.0) + np.float32(DT) / np.float32(1.0e9)  # Duration::as_secs_f32, as the library forms it
TILE = 64  # physics_amd/csrc/ccd.hip kCcdTile (test_the_tile_is_what_the_sizes_assume)
MISS, GROUND, STATIC = 0xFFFFFFFE, 0xFFFFFFFF, 0x80000000
SPHERE, BOX, CAPSULE = ccd_cases.SPHERE, ccd_cases.BOX, ccd_cases.CAPSULE


def _pa():
    import physics_amd
    return physics_amd


def _abi():
    from physics_amd import _abi
    return _abi


@functools.lru_cache(maxsize=None)
def _probe():
    import tempfile
    return ccd_probe.build(tempfile.mkdtemp(prefix="ccd_probe_") + "/ccd_probe")


def test_the_tile_is_what_the_sizes_assume():
    src = open(os.path.join(ROOT, "physics_amd", "csrc", "ccd.hip")).read()
    assert int(re.search(r"kCcdTile = (\d+);", src).group(1)) == TILE


def _world(bodies, statics=None, flags=0, **cfg):
    pa = _pa()
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | flags, **cfg))
    w.set_bodies(bodies["pos"], rot=bodies.get("rot"), lin_vel=bodies.get("lin"), ang_vel=bodies.get("ang"), shape_type=bodies["shape"],
                 half_extent=bodies["half_extent"])
    if statics is not None and len(statics["pos"]):
        w.set_static_bodies(statics["pos"], rot=statics.get("rot"), shape_type=statics["shape"], half_extent=statics["half_extent"])
    return w


def _filters(words):
    w = np.asarray(words, np.uint64)
    return (w[:, 0] & 0xFFFF).astype(np.uint16), (w[:, 0] >> 16).astype(np.uint16), w[:, 1].astype(np.int64).astype(np.int16)


# ---- 1. bit for bit against the probe ------------------------------------------------------------------------------------------

def _lattice_scene(n_bodies, n_statics, seed, filtered):
    """ccd_cases.soup with the bodies on a jittered lattice of 1 m (no two touch: the largest reaches 0.45 m from its centre with
    its margin), so the update has no body-body contact"""
    sc = ccd_cases.soup(seed, n_bodies, n_statics, filtered=filtered)
    rng = np.random.default_rng(seed + 1000)
    side = int(np.ceil(n_bodies ** (1 / 3)))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n_bodies]
    sc["bodies"]["pos"] = (cells - [side / 2, 0, side / 2] + [0.0, 1.0, 0.0] + rng.uniform(-0.04, 0.04, (n_bodies, 3))).astype(np.float32)
    return sc


SIZES = [(1, TILE + 1), (63, TILE + 1), (64, TILE + 1), (65, TILE + 1), (257, TILE + 1), (65, 1), (65, TILE - 1), (65, TILE), (65, 2 * TILE + 22)]
VARIANTS = [(f, g, e) for f in (False, True) for g in (False, True) for e in (False, True)]
CASES = [(nl, ns, *VARIANTS[k % 8]) for k, (nl, ns) in enumerate(SIZES)] + [(65, TILE + 1, *v) for v in VARIANTS]


@pytest.mark.parametrize("n_list,n_statics,filtered,ground,exact", sorted(set(CASES)))
def test_bit_for_bit_against_the_probe(n_list, n_statics, filtered, ground, exact, tmp_path):
    pa = _pa()
    n_bodies = n_list + 5  # some bodies stay unlisted
    sc = _lattice_scene(n_bodies, n_statics, 7 * n_list + n_statics, filtered)
    bd, st = sc["bodies"], sc["statics"]
    flags = (pa.FLAG_GROUND_PLANE if ground else 0) | (pa.FLAG_EXACT_ROTATION if exact else 0)
    w = _world(bd, st, flags=flags, ground_height=0.25)
    if filtered:
        w.set_body_filters(*_filters(bd["filt"]))
        w.set_static_filters(*_filters(st["filt"]))
    ids = np.random.default_rng(n_list).permutation(n_bodies)[:n_list].astype(np.uint32)
    w.set_ccd_bodies(ids)
    pos0, rot0 = w.get_transforms()
    w.update(DT)
    w.sync()
    lin, ang = w.get_velocities()
    pos1, rot1 = w.get_transforms()
    frac, target, normal, count = w.ccd_hits()
    w.close()
    listed = dict(shape=bd["shape"][ids], pos=pos0[ids], rot=rot0[ids], half_extent=bd["half_extent"][ids], lin=lin[ids], ang=ang[ids])
    case = dict(dt=DT_S, margin=0.02, ground=0.25 if ground else None, exact_rot=exact, statics=dict(st), bodies=listed)
    if filtered:
        listed["filt"] = bd["filt"][ids]
    else:
        case["statics"].pop("filt", None)
    p_frac, p_target, p_normal, p_pos, p_rot = ccd_probe.evaluate(_probe(), tmp_path, case)
    hits = int((p_target != MISS).sum())
    print(f"{n_list} listed, {n_statics} statics: {hits} stopped, {int((p_target == GROUND).sum())} of them by the ground")
    assert np.array_equal(frac.view(np.uint32), p_frac.view(np.uint32))
    assert np.array_equal(target, p_target)
    assert np.array_equal(normal.view(np.uint32), p_normal.view(np.uint32))
    assert np.array_equal(pos1[ids].view(np.uint32), p_pos.view(np.uint32))
    assert np.array_equal(rot1[ids].view(np.uint32), p_rot.view(np.uint32))
    assert np.array_equal(count, (p_target != MISS).astype(np.uint32))
    if n_list >= 63 and n_statics >= TILE - 1:
        assert hits > 0, "the scene is meant to stop somebody"
    # the unlisted bodies took the whole step
    rest = np.setdiff1d(np.arange(n_bodies), ids)
    assert np.array_equal(pos1[rest], (pos0[rest] + lin[rest] * DT_S).astype(np.float32))


# ---- 2. it stops what tunnels ----------------------------------------------------------------------------------------------------

TURN_Z45 = (0.0, 0.0, float(np.sin(np.pi / 8)), float(np.cos(np.pi / 8)))
PROJECTILES = {  # shape, half extent, rotation, how far its front lies ahead of its centre along +x
    "ball": (SPHERE, (0.1, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 0.1),
    "capsule": (CAPSULE, (0.1, 0.15, 0.0), (0.0, 0.0, 0.0, 1.0), 0.1),
    "turned box": (BOX, (0.1, 0.1, 0.1), TURN_Z45, 0.1 * np.sqrt(2.0)),  # edge first, the edge in line with the centre
}
WALL = dict(pos=np.array([[1.15, 0.0, 0.0]], np.float32), rot=np.array([[0, 0, 0, 1]], np.float32), shape=np.array([BOX], np.uint32),
            half_extent=np.array([[0.05, 2.0, 2.0]], np.float32))  # 0.1 m thick, its near face at x = 1.1


def _projectile(name, speed=120.0):
    shape, he, rot, front = PROJECTILES[name]
    # its front 1 m from the wall's near face
    return dict(pos=np.array([[1.1 - 1.0 - front, 0.0, 0.0]], np.float32), rot=np.array([rot], np.float32), lin=np.array([[speed, 0, 0]], np.float32),
                ang=np.zeros((1, 3), np.float32), shape=np.array([shape], np.uint32), half_extent=np.array([he], np.float32)), front


def _touch_bound(x, he, t):
    """the bound the CPU comparison holds t to (tests/test_ccd_cpu.py: boxcast_accept.tol_of), for a position along the path"""
    return tol_of(dict(t=np.array([t]), o=np.array([x], np.float64), he=np.array([he], np.float64), valid=np.array([True])), 0)


@pytest.mark.parametrize("name", list(PROJECTILES))
def test_a_listed_projectile_stops_at_the_wall(name):
    bd, front = _projectile(name)
    w = _world(bd, WALL, gravity_force=(0.0, 0.0, 0.0))
    w.set_ccd_bodies([0])
    w.update(DT)
    pos, _ = w.get_transforms()
    frac, target, normal, count = w.ccd_hits()
    gap = 1.1 - (float(pos[0, 0]) + front)
    bound = _touch_bound(bd["pos"][0], np.full(3, front), 1.0) + float(np.spacing(np.float32(1.1)))
    print(f"{name}: front {gap:+.3e} m from the wall after the first update (bound {bound:.3e}), frac {frac[0]:.6f}")
    assert target[0] == STATIC | 0 and count[0] == 1 and 0 < frac[0] < 1
    assert np.allclose(normal[0], (-1.0, 0.0, 0.0), atol=1e-4)
    assert abs(gap) <= bound, "on the near side, touching"
    w.update_n(DT, 10)
    pos, _ = w.get_transforms()
    lin, _ = w.get_velocities()
    w.close()
    print(f"{name}: after ten more updates x = {pos[0, 0]:.5f}, v.x = {lin[0, 0]:.3e}")
    assert float(pos[0, 0]) + front <= 1.1 + 0.02, "still on the near side (within the contact margin of the face)"
    assert lin[0, 0] <= 1e-3 * 120.0, "restitution 0: the velocity into the wall is gone"


@pytest.mark.parametrize("name", list(PROJECTILES))
def test_the_same_projectile_unlisted_tunnels(name):
    """what the feature is for (this half passes without it)"""
    bd, front = _projectile(name)
    w = _world(bd, WALL, gravity_force=(0.0, 0.0, 0.0))
    w.update(DT)
    pos, _ = w.get_transforms()
    w.close()
    assert float(pos[0, 0]) - front > 1.2, "beyond the wall after one update"


@pytest.mark.parametrize("name", list(PROJECTILES))
def test_a_listed_body_never_ends_an_update_under_the_ground(name):
    pa = _pa()
    shape, he, rot, _ = PROJECTILES[name]
    bd = dict(pos=np.array([[0.0, 5.0, 0.0]], np.float32), rot=np.array([rot], np.float32), lin=np.array([[0.0, -600.0, 0.0]], np.float32),
              ang=np.zeros((1, 3), np.float32), shape=np.array([shape], np.uint32), half_extent=np.array([he], np.float32))
    low = {"ball": 0.1, "capsule": 0.25, "turned box": 0.1 * np.sqrt(2.0)}[name]  # its lowest point below its centre
    w = _world(bd, flags=pa.FLAG_GROUND_PLANE)
    w.set_ccd_bodies([0])
    lows = []
    for _ in range(12):
        w.update(DT)
        pos, _ = w.get_transforms()
        lows.append(float(pos[0, 1]) - low)
    frac, target, _, count = w.ccd_hits()
    w.close()
    print(f"{name}: lowest point after each update: {['%.4f' % y for y in lows]}")
    assert min(lows) >= 0.0 - 0.02, "never below ground_y - contact_margin"
    # (a body that lands a float32 spacing above the ground is stopped again, by that hair, in the updates that follow: count >= 1)
    assert count[0] >= 1 and abs(lows[0]) <= 1e-4, "stopped at the ground in the first update"


# ---- 3. untouched where it should be -----------------------------------------------------------------------------------------------

def _cloud(n=200):
    rng = np.random.default_rng(5)
    shape = rng.choice([SPHERE, BOX, CAPSULE], size=n).astype(np.uint32)
    he = rng.uniform(0.15, 0.3, (n, 3)).astype(np.float32)
    pos = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4))
    return dict(pos=pos, rot=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32), lin=(-pos * 2 + rng.normal(size=(n, 3))).astype(np.float32),
                ang=rng.normal(size=(n, 3)).astype(np.float32), shape=shape, half_extent=he)


FAR_STATIC = dict(pos=np.array([[1000.0, 0.0, 0.0]], np.float32), rot=np.array([[0, 0, 0, 1]], np.float32), shape=np.array([BOX], np.uint32),
                  half_extent=np.array([[1.0, 1.0, 1.0]], np.float32))


def _run_cloud(listed, batch, profile=False):
    pa = _pa()
    bd = _cloud()
    w = _world(bd, FAR_STATIC, flags=pa.FLAG_GROUND_PLANE, ground_height=-1000.0)
    if listed:
        w.set_ccd_bodies(np.arange(len(bd["pos"])))
    if profile:
        w.profile_enable()
    if batch:
        w.update_n(DT, 30)
    else:
        for _ in range(30):
            w.update(DT)
    w.sync()
    out = (*w.get_transforms(), *w.get_velocities(), w.get_stats().n_manifolds, w.ccd_hits(), w.profile_get() if profile else None)
    w.close()
    return out


@pytest.mark.parametrize("batch", [False, True])
def test_a_world_whose_listed_bodies_hit_nothing_computes_the_same_bits(batch):
    a, b = _run_cloud(False, batch), _run_cloud(True, batch)
    assert a[4] > 20, "the cloud is meant to collide"
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    frac, target, normal, count = b[5]
    assert len(frac) == 200 and (frac == np.float32(1.0)).all() and (target == MISS).all() and not count.any() and not normal.any()
    assert len(a[5][0]) == 0


def test_a_world_without_a_list_launches_what_it_launched():
    """the sweep is the one launch per update a list adds (stage misc), and every other stage has the same launches in both
    worlds"""
    (_, _, _, _, _, _, (pa_, steps_a)), (_, _, _, _, _, _, (pb_, steps_b)) = _run_cloud(False, False, True), _run_cloud(True, False, True)
    assert steps_a == steps_b == 30
    assert pb_["misc"][1] == pa_.get("misc", (0.0, 0))[1] + 30  # (the stage also holds the memset that restarts the extent bound)
    assert pa_["position"][1] == pb_["position"][1] == 30
    assert {k: v[1] for k, v in pa_.items() if k != "misc"} == {k: v[1] for k, v in pb_.items() if k != "misc"}


# ---- 4. filters --------------------------------------------------------------------------------------------------------------------

def test_a_filtered_wall_is_flown_through_and_the_next_one_stops():
    bd, front = _projectile("ball")
    walls = dict(pos=np.array([[1.15, 0, 0], [3.65, 0, 0]], np.float32), rot=np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1)),
                 shape=np.array([BOX, BOX], np.uint32), half_extent=np.tile(np.array([0.05, 2.0, 2.0], np.float32), (2, 1)))
    w = _world(bd, walls, gravity_force=(0.0, 0.0, 0.0))
    w.set_body_filters(category=1, mask=0xFFFD)        # sees everything but category 2
    w.set_static_filters(category=np.array([2, 1]))    # the first wall is category 2
    w.set_ccd_bodies([0])
    w.update(DT)
    pos, _ = w.get_transforms()
    frac, target, _, count = w.ccd_hits()
    assert frac[0] == np.float32(1.0) and target[0] == MISS and count[0] == 0
    assert float(pos[0, 0]) - 0.1 > 1.2, "through the wall its filter leaves out"
    w.update(DT)
    pos, _ = w.get_transforms()
    frac, target, _, count = w.ccd_hits()
    w.close()
    assert target[0] == STATIC | 1 and count[0] == 1 and 0 < frac[0] < 1
    assert abs(3.6 - (float(pos[0, 0]) + 0.1)) <= _touch_bound(pos[0], np.full(3, 0.1), 2.0) + float(np.spacing(np.float32(3.6)))


# ---- 5. life cycle and errors ----------------------------------------------------------------------------------------------------

def test_life_cycle():
    pa = _pa()
    bd, _ = _projectile("ball")
    bd = {k: np.concatenate([v, v]) for k, v in bd.items()}
    bd["pos"][1] = (0.0, 50.0, 0.0)
    bd["lin"][1] = (0.0, 0.0, 0.0)
    w = _world(bd, WALL, gravity_force=(0.0, 0.0, 0.0))
    assert w.n_ccd == 0 and len(w.ccd_hits()[0]) == 0
    w.set_ccd_bodies([1, 0])                            # the order is kept: entry 1 is body 0
    frac, target, normal, count = w.ccd_hits()
    assert (frac == 1).all() and (target == MISS).all() and not count.any() and not normal.any()
    w.update(DT)
    frac, target, _, count = w.ccd_hits()
    assert list(target) == [MISS, STATIC | 0] and list(count) == [0, 1] and frac[0] == 1 and frac[1] < 1
    # duplicates and bad ids are refused and leave the old list in force
    for bad, code in (([0, 0], _abi().PHYS_ERR_INVALID_ARG), ([0, 2], _abi().PHYS_ERR_OUT_OF_RANGE)):
        with pytest.raises(pa.PhysError) as e:
            w.set_ccd_bodies(bad)
        assert e.value.code == code
    assert w.n_ccd == 2 and list(w.ccd_hits()[3]) == [0, 1]
    # replacing the statics keeps the list (and its counts)
    w.set_static_bodies(WALL["pos"] + np.float32(10.0), rot=WALL["rot"], shape_type=WALL["shape"], half_extent=WALL["half_extent"])
    assert w.n_ccd == 2 and list(w.ccd_hits()[3]) == [0, 1]
    # a new list resets the counts
    w.set_ccd_bodies([0])
    frac, target, _, count = w.ccd_hits()
    assert len(frac) == 1 and frac[0] == 1 and target[0] == MISS and count[0] == 0
    # n = 0 clears the list, in the library: its read-out writes nothing, and the ball, put back, flies through the wall
    w.set_ccd_bodies([])
    assert w.n_ccd == 0 and len(w.ccd_hits()[0]) == 0
    _assert_the_library_holds_no_list(w, bd)
    # set_bodies clears the list, in the library (the ids would be stale)
    w.set_ccd_bodies([0, 1])
    w.set_bodies(bd["pos"], rot=bd["rot"], lin_vel=bd["lin"], shape_type=bd["shape"], half_extent=bd["half_extent"])
    assert w.n_ccd == 0 and len(w.ccd_hits()[0]) == 0
    _assert_the_library_holds_no_list(w, bd)
    # ... and a list given again works as before
    w.set_body_poses([0], pos=bd["pos"][:1])
    w.set_body_velocities([0], lin=bd["lin"][:1])
    w.set_ccd_bodies([0])
    w.update(DT)
    assert list(w.ccd_hits()[1]) == [STATIC | 0]
    w.close()


@functools.lru_cache(maxsize=None)
def _misc_launches_of_an_update(listed):
    """launches of the profiler's stage misc in the second update of the life-cycle test's world, with or without a list"""
    bd, _ = _projectile("ball")
    w = _world(bd, WALL, gravity_force=(0.0, 0.0, 0.0))
    if listed:
        w.set_ccd_bodies([0])
    w.update(DT)
    w.sync()
    w.profile_enable(True)
    w.update(DT)
    w.sync()
    n = w.profile_get()[0].get("misc", (0.0, 0))[1]
    w.close()
    return n


def _assert_the_library_holds_no_list(w, bd):
    """asked of the library itself, not of the Python object's own count: phys_get_ccd_hits leaves sentinel-filled arrays as they
    are, and body 0, put back 1 m in front of the wall at 120 m/s, ends the update beyond it with one launch fewer than a listed
    world's update has"""
    import ctypes as C
    frac, normal = np.full(4, -7.0, np.float32), np.full(12, -7.0, np.float32)
    target, count = np.full(4, 0xDEADBEEF, np.uint32), np.full(4, 0xDEADBEEF, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = w.lib.phys_get_ccd_hits(w.h, frac.ctypes.data_as(fp), target.ctypes.data_as(up), normal.ctypes.data_as(fp), count.ctypes.data_as(up))
    assert rc == 0
    assert (frac == -7.0).all() and (normal == -7.0).all() and (target == 0xDEADBEEF).all() and (count == 0xDEADBEEF).all()
    w.set_static_bodies(WALL["pos"], rot=WALL["rot"], shape_type=WALL["shape"], half_extent=WALL["half_extent"])
    w.set_body_poses([0], pos=bd["pos"][:1])
    w.set_body_velocities([0], lin=bd["lin"][:1])
    w.sync()
    w.profile_enable(True)
    before = w.profile_get()[0].get("misc", (0.0, 0))[1]
    w.update(DT)
    w.sync()
    after = w.profile_get()[0].get("misc", (0.0, 0))[1]
    w.profile_enable(False)
    pos, _ = w.get_transforms()
    assert float(pos[0, 0]) - 0.1 > 1.2, "unlisted again: through the wall"
    # (the stage's other launch is the memset that restarts the extent bound; a world that never had a list says how often)
    assert after - before == _misc_launches_of_an_update(False) == _misc_launches_of_an_update(True) - 1, "no sweep was launched"


def test_unsupported_worlds_refuse_the_call():
    pa = _pa()
    bd, _ = _projectile("ball")
    w = pa.World(pa.default_config(flags=0))
    w.set_bodies(bd["pos"], shape_type=bd["shape"], half_extent=bd["half_extent"])
    with pytest.raises(pa.PhysError) as e:
        w.set_ccd_bodies([0])
    assert e.value.code == _abi().PHYS_ERR_UNSUPPORTED
    w.close()
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS, max_ghosts=4))
    w.set_bodies(bd["pos"], shape_type=bd["shape"], half_extent=bd["half_extent"])
    with pytest.raises(pa.PhysError) as e:
        w.set_ccd_bodies([0])
    assert e.value.code == _abi().PHYS_ERR_UNSUPPORTED
    w.close()


def test_the_device_read_out_equals_the_host_read_out():
    import torch
    sc = _lattice_scene(70, TILE + 1, 99, False)
    w = _world(sc["bodies"], sc["statics"])
    w.set_ccd_bodies(np.arange(0, 70, 2))
    w.update(DT)
    host = w.ccd_hits()
    n = w.n_ccd
    dev = (torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
           torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    w.ccd_hits_device(*dev)
    w.sync()
    w.ccd_hits_device(frac_out=dev[0])  # any of them may be left out
    w.sync()
    w.close()
    assert (host[1] != MISS).any()
    assert np.array_equal(host[0], dev[0].cpu().numpy())
    assert np.array_equal(host[1], dev[1].cpu().numpy().view(np.uint32))
    assert np.array_equal(host[2], dev[2].cpu().numpy())
    assert np.array_equal(host[3], dev[3].cpu().numpy().view(np.uint32))


def _bouncing_world():
    """a ball between two walls 2.5 m apart, everything with restitution 1: it is stopped at one wall, thrown back by the contact,
    and stopped at the other within five updates"""
    bd, _ = _projectile("ball")
    walls = dict(pos=np.array([[1.15, 0, 0], [-1.55, 0, 0]], np.float32), rot=np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1)),
                 shape=np.array([BOX, BOX], np.uint32), half_extent=np.tile(np.array([0.05, 2.0, 2.0], np.float32), (2, 1)))
    w = _world(bd, walls, gravity_force=(0.0, 0.0, 0.0))
    w.set_body_materials(restitution=1.0)
    w.set_static_materials(restitution=1.0)
    w.set_ccd_bodies([0])
    return w


def test_counts_accumulate_across_a_batch():
    w = _bouncing_world()
    stops, targets = 0, []
    for _ in range(5):
        w.update(DT)
        _, target, _, count = w.ccd_hits()
        stops += int(target[0] != MISS)
        targets.append(int(target[0]))
        assert count[0] == stops
    w.close()
    print("targets per update:", [hex(t) for t in targets])
    assert stops >= 2 and {STATIC | 0, STATIC | 1} <= set(targets), "stopped in two different updates, at both walls"
    w = _bouncing_world()
    w.update_n(DT, 5)
    _, target, _, count = w.ccd_hits()
    w.close()
    assert count[0] == stops and int(target[0]) == targets[-1], "the batch hides no hit; the record is the last update's"
