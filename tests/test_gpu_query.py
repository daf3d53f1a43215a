"""GPU: sphere casts (phys_spherecast / phys_spherecast_device) and overlap queries (phys_overlap) against the float64
brute force of tests/query_ref.py.

Hand scenes with known answers; random soups of spheres, boxes, capsules and NONE bodies with statics and the ground;
radius 0 against phys_raycast; ignore_body; ascending unique ids (a body whose two cells share a bucket included);
capacity and the Python retry; a scene-covering query (the direct path); invalid queries; no side effects on the updates;
determinism; current poses; ghost slots never reported."""
import math

import numpy as np
import pytest

import query_ref as ref
from query_accept import compare_casts, compare_overlaps  # noqa: F401 (tests/test_gpu_filter.py reads them here too)

pytestmark = pytest.mark.gpu


def _pa():
    import physics_amd
    return physics_amd


def _world(pos, shape, he, rot=None, flags=None, ground=0.0, **cfg):
    pa = _pa()
    if flags is None:
        flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE
    kw = dict(flags=flags, gravity_offset=(0.0, 0.0, 0.0), ground_height=ground)
    kw.update(cfg)
    w = pa.World(pa.default_config(**kw))
    w.set_bodies(np.asarray(pos, np.float32), rot=None if rot is None else np.asarray(rot, np.float32),
                 shape_type=np.asarray(shape, np.uint32), half_extent=np.asarray(he, np.float32))
    return w


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _soup(rng, n, extent):
    pos = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.0, extent, n)
    shape = rng.choice([1, 2, 3, 0], n, p=[0.3, 0.35, 0.3, 0.05]).astype(np.uint32)
    he = rng.uniform(0.2, 1.2, (n, 3)).astype(np.float32)
    return pos, _quats(rng, n), shape, he


def _statics(rng):
    # a raised platform (its top 0.3 above the ground: no exact ties with the ground plane), a ball, a capsule, a box
    pos = np.array([[0, -0.2, 0], [6, 2, -4], [-5, 1, 5], [3, 4, 8]], np.float32)
    shape = np.array([2, 1, 3, 2], np.uint32)
    he = np.array([[10, 0.5, 10], [1.5, 0, 0], [0.7, 2, 0], [1, 2, 0.5]], np.float32)
    rot = np.concatenate([np.array([[0, 0, 0, 1]], np.float32), _quats(rng, 3)])
    return pos, rot, shape, he


def _targets(w, shape, he, statics=None):
    pos, rot = w.get_transforms()
    b = dict(pos=pos, rot=rot, half_extent=np.asarray(he, np.float32), shape=np.asarray(shape))
    s = None if statics is None else dict(pos=statics[0], rot=statics[1], shape=statics[2], half_extent=statics[3])
    return ref.targets(b, s)


def _casts(rng, n, extent):
    o = rng.uniform(-extent - 3, extent + 3, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(0.0, extent + 3, n)
    aim = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    d = (aim - o).astype(np.float32)
    d[: n // 4] = rng.normal(size=(n // 4, 3))
    return o, d


# ---- 1. hand scenes --------------------------------------------------------------------------------------------------
def test_hand_spherecasts():
    pa = _pa()
    w = _world([[0, 5, 0], [10, 5, 0], [20, 5, 0]], [pa.SHAPE_BOX, pa.SHAPE_CAPSULE, pa.SHAPE_SPHERE],
               [[1, 1, 1], [0.5, 1, 0], [1, 0, 0]], rot=[[0, 0, 0, 1]] * 3)
    o = np.array([[-5, 5.2, 0.3], [-5, 6.3, 0], [-5, 6.3, 1.2], [10, 10, 0.3], [5, 5.5, 0], [20, 10, 0], [30, 3, 0], [0, 5, 0]],
                 np.float32)
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, -1, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    body, t, n = w.spherecast(o, d, 0.5)
    assert list(body[:3]) == [0, 0, 0]
    assert abs(t[0] - 3.5) < 1e-5 and np.allclose(n[0], [-1, 0, 0], atol=1e-5)   # face
    assert abs(t[1] - 3.6) < 1e-5 and np.allclose(n[1], [-0.8, 0.6, 0], atol=1e-5)  # edge
    r = math.sqrt(0.25 - 0.13)
    assert abs(t[2] - (4 - r)) < 1e-5 and np.allclose(n[2], np.array([-r, 0.3, 0.2]) / 0.5, atol=1e-5)  # corner
    hh = math.sqrt(1.0 - 0.09)
    assert body[3] == 1 and abs(t[3] - (10 - 6 - hh)) < 1e-5  # capsule end ball
    assert body[4] == 1 and abs(t[4] - (5 - 1.0)) < 1e-5 and np.allclose(n[4], [-1, 0, 0], atol=1e-5)  # capsule side
    assert body[5] == 2 and abs(t[5] - 3.5) < 1e-5
    assert body[6] == pa.RAY_GROUND and abs(t[6] - 2.5) < 1e-5 and np.allclose(n[6], [0, 1, 0])
    assert body[7] == 0 and t[7] == 0 and np.allclose(n[7], [0, 0, -1])  # starts inside: t = 0, -dir
    # invalid radius and rays miss
    body, t, n = w.spherecast(o[:4], d[:4], np.array([-1, np.nan, np.inf, 0.5], np.float32), max_t=[9, 9, 9, -1])
    assert list(body) == [pa.RAY_MISS] * 4 and np.isinf(t).all() and not n.any()
    w.close()


def test_hand_overlaps_and_sat_edge_case():
    pa = _pa()
    qz = [0, 0, math.sin(math.pi / 8), math.cos(math.pi / 8)]
    qx = [math.sin(math.pi / 8), 0, 0, math.cos(math.pi / 8)]
    w = _world([[0, 5, 0], [4, 5, 0]], [pa.SHAPE_BOX, pa.SHAPE_SPHERE], [[1, 1, 1], [1, 0, 0]], rot=[qz, [0, 0, 0, 1]])
    c = 5 + 2 * math.sqrt(2)
    off, ids = w.overlap(pa.SHAPE_BOX, [[0, c - 1e-3, 0], [0, c + 1e-3, 0]], rot=[qx, qx], half_extent=[1, 1, 1])
    assert list(off) == [0, 1, 1] and list(ids) == [0]
    # a capsule along z by the box edge (1, 6) of body 1 turned back to axis-aligned: just inside / just outside
    w.set_bodies(np.array([[0, 5, 0]], np.float32), shape_type=np.array([pa.SHAPE_BOX], np.uint32),
                 half_extent=np.ones((1, 3), np.float32))
    along_z = [math.sin(math.pi / 4), 0, 0, math.cos(math.pi / 4)]
    q = [[1 + d / math.sqrt(2), 6 + d / math.sqrt(2), 0] for d in (0.5 - 1e-3, 0.5 + 1e-3)]
    off, ids = w.overlap(pa.SHAPE_CAPSULE, q, rot=[along_z] * 2, half_extent=[0.5, 2, 0])
    assert list(off) == [0, 1, 1] and list(ids) == [0]
    # ground and invalid queries
    off, ids = w.overlap([pa.SHAPE_SPHERE, pa.SHAPE_SPHERE, 9, pa.SHAPE_BOX, pa.SHAPE_SPHERE],
                         [[0, 0.5, 20], [0, 0.5, 0], [0, 5, 0], [0, 5, 0], [np.nan, 5, 0]],
                         half_extent=[[0.5, 0, 0], [0.4, 0, 0], [1, 1, 1], [1, -1, 1], [1, 0, 0]])
    assert list(off) == [0, 1, 1, 1, 1, 1] and list(ids) == [pa.RAY_GROUND]
    w.close()


# ---- 2. random soups against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_random_soup_spherecasts(seed):
    pa = _pa()
    rng = np.random.default_rng(seed)
    pos, rot, shape, he = _soup(rng, 400, 15.0)
    w = _world(pos, shape, he, rot=rot)
    sp = _statics(rng)
    w.set_static_bodies(sp[0], sp[1], sp[2], sp[3])
    tg = _targets(w, shape, he, sp)
    o, d = _casts(rng, 1500, 15.0)
    for rad in (0.25, 1.0):
        compare_casts(w, tg, o, d, rad, label=f"seed {seed} radius {rad}")
    radv = rng.uniform(0, 1.5, len(o)).astype(np.float32)
    body, _, _ = compare_casts(w, tg, o, d, radv, label=f"seed {seed} mixed radii")
    assert (body < len(pos)).sum() > len(o) // 5 and (body & pa.STATIC_ID_BIT != 0).sum() > 0
    w.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_random_soup_overlaps(seed):
    pa = _pa()
    rng = np.random.default_rng(10 + seed)
    pos, rot, shape, he = _soup(rng, 400, 15.0)
    w = _world(pos, shape, he, rot=rot)
    sp = _statics(rng)
    w.set_static_bodies(sp[0], sp[1], sp[2], sp[3])
    tg = _targets(w, shape, he, sp)
    m = 1500
    qp = rng.uniform(-16, 16, (m, 3)).astype(np.float32)
    qp[:, 1] = rng.uniform(-0.5, 16, m)
    qs = rng.choice([pa.SHAPE_SPHERE, pa.SHAPE_BOX, pa.SHAPE_CAPSULE], m).astype(np.uint32)
    qh = rng.uniform(0.1, 2.0, (m, 3)).astype(np.float32)
    off, ids = compare_overlaps(w, tg, qs, qp, _quats(rng, m), qh, label=f"seed {seed}")
    per = np.diff(off)
    assert (per > 0).sum() > m // 3 and (ids < len(pos)).sum() > m // 4
    w.close()


# ---- 3. radius 0 is the ray cast ---------------------------------------------------------------------------------------
def test_radius_zero_agrees_with_raycast():
    rng = np.random.default_rng(21)
    pos, rot, shape, he = _soup(rng, 2000, 25.0)
    w = _world(pos, shape, he, rot=rot)
    sp = _statics(rng)
    w.set_static_bodies(sp[0], sp[1], sp[2], sp[3])
    o, d = _casts(rng, 20_000, 25.0)
    rb, rt, _ = w.raycast(o, d)
    sb, st, _ = w.spherecast(o, d, 0.0)
    same = rb == sb
    fin = np.isfinite(rt) & same
    oinf = np.abs(o).max(1)
    assert (np.abs(st[fin] - rt[fin]) <= 1e-5 * (1 + oinf[fin] + rt[fin])).all()
    assert (~same).sum() <= len(o) // 1000, int((~same).sum())
    w.close()


# ---- 4. rules ----------------------------------------------------------------------------------------------------------
def test_ignore_capacity_retry_and_direct_path():
    pa = _pa()
    rng = np.random.default_rng(4)
    pos, rot, shape, he = _soup(rng, 300, 10.0)
    w = _world(pos, shape, he, rot=rot)
    # ignore_body
    body, t, _ = w.spherecast([[-30, 5, 0]], [[1, 0, 0]], 0.5)
    if body[0] < len(pos):
        b2, t2, _ = w.spherecast([[-30, 5, 0]], [[1, 0, 0]], 0.5, ignore=[body[0]])
        assert b2[0] != body[0] and t2[0] >= t[0]
    i0 = int(np.nonzero(shape != pa.SHAPE_NONE)[0][0])
    off, ids = w.overlap(pa.SHAPE_SPHERE, [pos[i0]], half_extent=[0.1, 0, 0])
    assert i0 in ids
    off, ids = w.overlap(pa.SHAPE_SPHERE, [pos[i0]], half_extent=[0.1, 0, 0], ignore=[i0])
    assert i0 not in ids
    # capacity: a too small cap reports the total, the Python retry gets it all
    q = rng.uniform(-10, 10, (200, 3)).astype(np.float32)
    off_full, ids_full = w.overlap(pa.SHAPE_BOX, q, half_extent=[3, 3, 3], cap=1 << 20)
    assert off_full[-1] > 20
    from physics_amd import _abi
    offs = np.zeros(201, np.uint64)
    small = np.zeros(4, np.uint32)
    st = np.full(200, pa.SHAPE_BOX, np.uint32)
    hq = np.full((200, 3), 3, np.float32)
    rc = w.lib.phys_overlap(w.h, 200, st.ctypes.data_as(_abi.u32p), q.ctypes.data_as(_abi.f32p), None,
                            hq.ctypes.data_as(_abi.f32p), None, 4, offs.ctypes.data_as(_abi.u64p), small.ctypes.data_as(_abi.u32p))
    assert rc == _abi.PHYS_ERR_CAPACITY and np.array_equal(offs, off_full)
    off2, ids2 = w.overlap(pa.SHAPE_BOX, q, half_extent=[3, 3, 3], cap=4)  # the retry
    assert np.array_equal(off2, off_full) and np.array_equal(ids2, ids_full)
    # a scene-covering query: every shaped body, in order (the direct path), then the ground
    off, ids = w.overlap(pa.SHAPE_SPHERE, [[0, 0, 0]], half_extent=[1000, 0, 0])
    want = [i for i in range(len(pos)) if shape[i] != pa.SHAPE_NONE] + [pa.RAY_GROUND]
    assert list(ids) == want
    w.close()


def test_ids_unique_when_two_cells_share_a_bucket():
    """Brute force: find a body whose cells hash to one bucket under the grid the scene gives, then query around it."""
    pa = _pa()

    def bucket(x, y, z, bits):
        h = ((x * 73856093) ^ (y * 19349663) ^ (z * 83492791)) & 0xFFFFFFFF
        return ((h * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)

    # unit cubes on a lattice of pitch 1.5: cell edge about 2, so every cube spans two cells per axis; 1024 bodies -> a
    # table of 4096 buckets (bits 12). Search cell pairs (x, x + 1) along x that collide.
    hits = [(x, y, z) for x in range(40) for y in range(40) for z in range(6)
            if bucket(x, y, z, 12) in (bucket(x + 1, y, z, 12), bucket(x, y + 1, z, 12), bucket(x, y, z + 1, 12))]
    assert hits
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(4), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    pos = (g * 1.5 + 2.0).astype(np.float32)
    n = len(pos)
    w = _world(pos, np.full(n, pa.SHAPE_BOX), np.full((n, 3), 0.5, np.float32))
    tg = _targets(w, np.full(n, pa.SHAPE_BOX), np.full((n, 3), 0.5, np.float32))
    # many queries over the whole lattice: every list must be ascending and unique, and equal to the reference
    m = 3000
    qp = rng.uniform(0, 26, (m, 3)).astype(np.float32)
    qp[:, 1] = rng.uniform(1, 8, m)
    compare_overlaps(w, tg, np.full(m, pa.SHAPE_BOX, np.uint32), qp, _quats(rng, m),
                     rng.uniform(0.3, 2.5, (m, 3)).astype(np.float32), ground=0.0, label="lattice")
    w.close()


# ---- 5. no side effects --------------------------------------------------------------------------------------------------
def _snapshot(w):
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    st = w.get_stats()
    return [pos, rot, lin, ang], {k: getattr(st, k) for k, _ in type(st)._fields_}, w.get_manifolds()


@pytest.mark.parametrize("name", ["c2", "cluster_tower"])
def test_queries_leave_updates_bit_identical(name):
    import torch
    pa = _pa()
    from physics_amd import scenes
    if name == "c2":
        sc = scenes.c2()
    else:
        sc = scenes.c5(16, 130, 16)
        sc.flags |= pa.FLAG_SOLVER_CLUSTER
    worlds = []
    for _ in range(2):
        w = pa.World(sc.config())
        sc.populate(w)
        worlds.append(w)
    quiet, probed = worlds
    rng = np.random.default_rng(3)
    lo, hi = sc.pos.min(0) - 3, sc.pos.max(0) + 3
    o = rng.uniform(lo, hi, (2000, 3)).astype(np.float32)
    d = rng.normal(size=(2000, 3)).astype(np.float32)
    qp = rng.uniform(lo, hi, (500, 3)).astype(np.float32)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tr = torch.full((len(o),), 0.5, dtype=torch.float32, device="cuda")
    tb = torch.empty(len(o), dtype=torch.int32, device="cuda")
    tt = torch.empty(len(o), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    found = 0
    for k in range(12):
        for w in worlds:
            w.update_n(scenes.DT_NANOS, 2)
        probed.spherecast(o, d, 0.5)
        probed.spherecast_device(to, td, tr, tb, tt)
        off, _ = probed.overlap(pa.SHAPE_BOX, qp, half_extent=[1, 1, 1])
        found += int(off[-1])
    for w in worlds:
        w.sync()
    a, b = _snapshot(quiet), _snapshot(probed)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    assert found > 0
    for w in worlds:
        w.close()


# ---- 6. determinism, current poses, device variant, ghosts ----------------------------------------------------------------
def test_determinism_device_variant_and_current_poses():
    import torch
    pa = _pa()
    rng = np.random.default_rng(11)
    pos, rot, shape, he = _soup(rng, 5000, 30.0)
    w = _world(pos, shape, he, rot=rot)
    o, d = _casts(rng, 20_000, 30.0)
    rad = rng.uniform(0, 1, len(o)).astype(np.float32)
    a = w.spherecast(o, d, rad)
    b = w.spherecast(o, d, rad)
    perm = rng.permutation(len(o))
    c = w.spherecast(o[perm], d[perm], rad[perm])
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.array_equal(x[perm].view(np.uint32), z.view(np.uint32))
    to, td, tr = (torch.from_numpy(x).cuda() for x in (o, d, rad))
    tb = torch.empty(len(o), dtype=torch.int32, device="cuda")
    tt = torch.empty(len(o), dtype=torch.float32, device="cuda")
    tn = torch.empty((len(o), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w.spherecast_device(to, td, tr, tb, tt, tn)
    w.sync()
    assert np.array_equal(tb.cpu().numpy().view(np.uint32), a[0])
    assert np.array_equal(tt.cpu().numpy().view(np.uint32), a[1].view(np.uint32))
    assert np.array_equal(tn.cpu().numpy().view(np.uint32), a[2].view(np.uint32))
    # overlaps: the same per query across calls, orders and batch sizes
    m = 4000
    qp = rng.uniform(-30, 30, (m, 3)).astype(np.float32)
    qs = rng.choice([1, 2, 3], m).astype(np.uint32)
    qr = _quats(rng, m)
    qh = rng.uniform(0.2, 3, (m, 3)).astype(np.float32)
    off, ids = w.overlap(qs, qp, qr, qh)
    lists = [ids[off[i]:off[i + 1]] for i in range(m)]
    off2, ids2 = w.overlap(qs[perm[:m] % m], qp[perm[:m] % m], qr[perm[:m] % m], qh[perm[:m] % m])
    for j, i in enumerate(perm[:m] % m):
        assert np.array_equal(ids2[off2[j]:off2[j + 1]], lists[i])
    for s in range(0, m, 997):
        o3, i3 = w.overlap(qs[s:s + 1], qp[s:s + 1], qr[s:s + 1], qh[s:s + 1])
        assert np.array_equal(i3, lists[s])
    # current poses: move body 0 far away through set_bodies; the queries follow at once
    pos2 = pos.copy()
    pos2[0] = [500, 500, 500]
    w.set_bodies(pos2, rot=rot, shape_type=shape, half_extent=he)
    if shape[0] != pa.SHAPE_NONE:
        body, t, _ = w.spherecast([[500, 500, 490]], [[0, 0, 1]], 0.5)
        assert body[0] == 0
        _, ids = w.overlap(pa.SHAPE_SPHERE, [[500, 500, 500]], half_extent=[0.1, 0, 0])
        assert list(ids) == [0]
    # and after updates: the queries see the poses the last update left
    w.update_n(1_000_000_000 // 60, 3)
    w.sync()
    p3, r3 = w.get_transforms()
    tg = ref.targets(dict(pos=p3, rot=r3, half_extent=he, shape=shape))
    compare_casts(w, tg, o[:800], d[:800], 0.5, label="after updates")
    w.close()


def test_ghost_slots_are_never_reported():
    import torch
    pa = _pa()
    zs = [-6.0, -2.0, 2.0, 6.0]
    cap = 64

    def make(xs, x_lo, x_hi, gid0):
        pos = np.array([[x, 5.0, z] for x in xs for z in zs], np.float32)
        cfg = pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0, 0, 0), max_ghosts=2 * cap)
        w = pa.World(cfg)
        n = len(pos)
        w.set_bodies(pos, shape_type=np.full(n, pa.SHAPE_BOX, np.uint32), half_extent=np.ones((n, 3), np.float32))
        w.set_global_ids(np.arange(gid0, gid0 + n, dtype=np.uint32))
        w.set_slab(x_lo, x_hi, 4.0)
        return w, pos

    left, lpos = make([-1.5, -20.0], -1.0e6, 0.0, 0)
    right, rpos = make([1.5, 20.0], 0.0, 1.0e6, 100)
    buf = torch.full((cap * 96,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    left.halo_pack_bodies(buf.data_ptr(), cap)
    left.sync()
    right.halo_unpack_ghosts(buf.data_ptr(), cap, 0, 0)
    right.sync()
    assert right.get_stats().n_ghosts == len(zs)
    n = right.n
    ghost_pos = lpos[:len(zs)]
    body, _, _ = right.spherecast(ghost_pos + [0, 10, 0], np.tile([0.0, -1.0, 0.0], (len(zs), 1)), 0.25)
    assert list(body) == [pa.RAY_GROUND] * len(zs), body
    off, ids = right.overlap(pa.SHAPE_SPHERE, ghost_pos, half_extent=[0.5, 0, 0])
    assert ((ids < n) | (ids == pa.RAY_GROUND)).all() and not (ids < n).any()
    off, ids = right.overlap(pa.SHAPE_SPHERE, [[0, 0, 0]], half_extent=[100, 0, 0])
    assert list(ids) == list(range(n)) + [pa.RAY_GROUND]
    left.close()
    right.close()
