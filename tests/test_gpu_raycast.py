"""GPU: batched ray casts (phys_raycast / phys_raycast_device) against the float64 brute force of tests/raycast_ref.py.

Hand cases with known answers; random scenes with rays inside, far outside and along the ground; the CURRENT poses
(not the pose the last broad phase saw, not the start-of-update copy); no side effects on the updates (bit-identical
worlds with and without ray casts in between, the cluster solver's bucket-order deal included); determinism; ghost
slots never hit; the 1M-body scene."""
import ctypes as C
import math

import numpy as np
import pytest

import raycast_ref as ref
from query_accept import compare

pytestmark = pytest.mark.gpu


def _pa():
    import physics_amd
    return physics_amd


def _world(pos, shape, he, rot=None, flags=None, lin_vel=None, **cfg):
    pa = _pa()
    if flags is None:
        flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE
    kw = dict(flags=flags, gravity_offset=(0.0, 0.0, 0.0))
    kw.update(cfg)
    w = pa.World(pa.default_config(**kw))
    w.set_bodies(np.asarray(pos, np.float32), rot=None if rot is None else np.asarray(rot, np.float32), lin_vel=lin_vel,
                 shape_type=np.asarray(shape, np.uint32), half_extent=np.asarray(he, np.float32))
    return w


def _bodies(w, shape, he):
    pos, rot = w.get_transforms()
    return dict(pos=pos, rot=rot, half_extent=np.asarray(he, np.float32).reshape(-1, 3), shape=np.asarray(shape).reshape(-1))


# ---- 1. hand scene ---------------------------------------------------------------------------------------------------
S45 = math.sin(math.pi / 8)


def _hand_world(flags=None):
    pa = _pa()
    B, S, N = pa.SHAPE_BOX, pa.SHAPE_SPHERE, pa.SHAPE_NONE
    pos = [[0, 5, 0], [10, 5, 0], [20, 5, 0], [30, 5, 0], [40, 5, 0], [45, 5, 0], [60, -1, 0]]
    shape = [B, B, S, N, B, B, B]
    he = [[1, 2, 3], [1, 1, 1], [2, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    rot = np.tile([0, 0, 0, 1.0], (7, 1))
    rot[1] = [0, S45, 0, math.cos(math.pi / 8)]
    return _world(pos, shape, he, rot=rot, flags=flags), shape, he


@pytest.mark.parametrize("mode", ["collisions", "broadphase_only", "no_collisions"])
def test_hand_scene(mode):
    pa = _pa()
    flags = {"collisions": pa.FLAG_COLLISIONS, "broadphase_only": pa.FLAG_COLLISIONS | pa.FLAG_BROADPHASE_ONLY,
             "no_collisions": 0}[mode] | pa.FLAG_GROUND_PLANE
    w, shape, he = _hand_world(flags)
    M, G = pa.RAY_MISS, pa.RAY_GROUND
    s = math.sqrt(0.5)
    cases = [  # origin, dir, max_t, ignore, body, t, normal
        ([-10, 5.5, 0.5], [3, 0, 0], None, None, 0, 9.0, [-1, 0, 0]),              # axis-aligned box
        ([5, 5, 0.3], [1, 0, 0], None, None, 1, 5.3 - math.sqrt(2), [-s, 0, s]),   # box turned 45 degrees about y
        ([20, 5, -10], [0, 0, 1], None, None, 2, 8.0, [0, 0, -1]),                  # sphere
        ([0.5, 5, 0], [0, 1, 0], None, None, 0, 0.0, [0, -1, 0]),                   # origin inside
        ([-10, 7.5, 0], [1, 0, 0], None, None, M, math.inf, [0, 0, 0]),             # parallel miss
        ([-10, 5.5, 0.5], [1, 0, 0], 8.9, None, M, math.inf, [0, 0, 0]),            # max_t cut
        ([-10, 5.5, 0.5], [1, 0, 0], 9.0, None, 0, 9.0, [-1, 0, 0]),
        ([30, 10, 0], [0, -1, 0], None, None, G, 10.0, [0, 1, 0]),                  # NONE body: never hit
        ([37, 5, 0], [1, 0, 0], None, None, 4, 2.0, [-1, 0, 0]),
        ([37, 5, 0], [1, 0, 0], None, 4, 5, 7.0, [-1, 0, 0]),                       # ignore_body
        ([37, 5, 0], [1, 0, 0], None, 7, 4, 2.0, [-1, 0, 0]),                       # >= n_bodies: ignores nothing
        ([37, 5, 0], [1, 0, 0], None, 0xFFFFFFFF, 4, 2.0, [-1, 0, 0]),
        ([60, 5, 0], [0, -2, 0], None, None, 6, 5.0, [0, 1, 0]),                    # box top = ground: the body wins
        ([70, 5, 0], [0, -1, 0], None, None, G, 5.0, [0, 1, 0]),                    # the ground
        ([70, -1, 0], [1, 0, 0], None, None, G, 0.0, [-1, 0, 0]),                   # origin inside the ground
        ([70, 5, 0], [0, 0, 0], None, None, M, math.inf, [0, 0, 0]),                # zero direction
        ([70, 5, 0], [math.nan, -1, 0], None, None, M, math.inf, [0, 0, 0]),        # NaN direction
        ([math.inf, 5, 0], [0, -1, 0], None, None, M, math.inf, [0, 0, 0]),         # infinite origin
    ]
    o = np.array([c[0] for c in cases], np.float32)
    d = np.array([c[1] for c in cases], np.float32)
    mt = np.array([math.inf if c[2] is None else c[2] for c in cases], np.float32)
    ig = np.array([0xFFFFFFFF if c[3] is None else c[3] for c in cases], np.uint32)
    body, t, nrm = w.raycast(o, d, mt, ig)
    for k, c in enumerate(cases):
        assert body[k] == c[4], (k, c, body[k], t[k])
        if math.isinf(c[5]):
            assert t[k] == math.inf, (k, t[k])
        else:
            assert abs(t[k] - c[5]) <= 1e-5, (k, t[k], c[5])
        assert np.abs(nrm[k] - np.array(c[6])).max() <= 1e-5, (k, nrm[k], c[6])
    # without max_t / ignore / normal arrays
    b2, t2, _ = w.raycast(o[:5], d[:5])
    assert list(b2) == [c[4] for c in cases[:5]]
    # no bodies: the ground or nothing
    w.set_bodies(np.zeros((0, 3), np.float32))
    b0, t0, _ = w.raycast([[0, 5, 0], [0, 5, 0]], [[0, -1, 0], [0, 1, 0]])
    assert list(b0) == [G, M] and t0[0] == 5.0 and t0[1] == math.inf
    assert w.raycast(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0,)
    w.close()


def test_invalid_arguments():
    pa = _pa()
    w, _, _ = _hand_world()
    one = np.zeros(3, np.float32)
    out_b, out_t = np.zeros(1, np.uint32), np.zeros(1, np.float32)
    f32p, u32p = pa._abi.f32p, pa._abi.u32p
    p = lambda a, t=f32p: a.ctypes.data_as(t)  # noqa: E731
    assert w.lib.phys_raycast(w.h, 1, None, p(one), None, None, p(out_b, u32p), p(out_t), None) == pa._abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_raycast(w.h, 1, p(one), p(one), None, None, None, p(out_t), None) == pa._abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_raycast(w.h, 1 << 31, p(one), p(one), None, None, p(out_b, u32p), p(out_t), None) == pa._abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_raycast_device(w.h, 1, None, None, None, None, None, None, None) == pa._abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_raycast(w.h, 0, None, None, None, None, None, None, None) == 0
    w.close()


def _lattice_planes():
    """Unit cubes at (2i, 2j + 1, 2k): the grid of the documented rule (include/physics_hip.h) in float32."""
    f = np.float32
    idx = np.arange(5)
    pos = np.stack(np.meshgrid(2.0 * idx, 2.0 * idx + 1.0, 2.0 * idx, indexing="ij"), -1).reshape(-1, 3).astype(f)
    lo, hi = pos.min(0) - f(0.5), pos.max(0) + f(0.5)
    e = f(1.0)
    m = f(max(np.abs(lo).max(), np.abs(hi).max()))
    pad = f(2.0 ** -16) * (m + e)
    cell = (e + f(2) * pad) * f(1 + 2.0 ** -10)
    glo = lo - pad
    return pos, glo, cell


def test_rays_in_grid_planes_and_through_grid_corners():
    pa = _pa()
    pos, glo, cell = _lattice_planes()
    n = len(pos)
    shape, he = np.full(n, pa.SHAPE_BOX), np.full((n, 3), 0.5, np.float32)
    w = _world(pos, shape, he)
    bodies = _bodies(w, shape, he)
    o, d = [], []
    ks = range(0, 11)
    for a in ks:
        for b in ks:
            py, pz = glo[1] + np.float32(a) * cell, glo[2] + np.float32(b) * cell
            o.append([-5.0, py, pz]); d.append([1.0, 0.0, 0.0])             # along x through grid corners (two planes)
            o.append([glo[0] + np.float32(a) * cell, 20.0, pz]); d.append([0.0, -1.0, 0.3])  # inside one plane
            px = glo[0] + np.float32(a) * cell
            o.append([px, py, pz]); d.append([1.0, 1.0, 1.0])               # from a grid corner, diagonal
            o.append([px, py, pz]); d.append([-1.0, 0.5, 0.0])
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    compare(w, bodies, o, d, label="grid planes")
    w.close()


# ---- 2. random scenes against the brute force ------------------------------------------------------------------------
def _random_scene(rng, n, extent):
    pa = _pa()
    pos = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.0, 2 * extent, n)
    q = rng.normal(size=(n, 4))
    rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    shape = np.where(rng.random(n) < 0.5, pa.SHAPE_SPHERE, pa.SHAPE_BOX).astype(np.uint32)
    he = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    return pos, rot, shape, he


def _rays(rng, n, lo, hi):
    """a third inside the bounds, a third from far outside aimed into them, a third along the ground; random lengths"""
    k = n // 3
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, size = (lo + hi) / 2, float((hi - lo).max())
    o1 = rng.uniform(lo, hi, (k, 3))
    d1 = rng.normal(size=(k, 3))
    v = rng.normal(size=(k, 3))
    o2 = c + 2.0 * size * v / np.linalg.norm(v, axis=1, keepdims=True)
    d2 = rng.uniform(lo, hi, (k, 3)) - o2
    m = n - 2 * k
    o3 = np.column_stack([rng.uniform(lo[0], hi[0], m), rng.uniform(0.001, 0.5, m), rng.uniform(lo[2], hi[2], m)])
    d3 = np.column_stack([rng.normal(size=m), rng.uniform(-0.2, 0.2, m), rng.normal(size=m)])
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    d *= rng.uniform(0.1, 10.0, (n, 1))
    return o.astype(np.float32), d.astype(np.float32)


def _scene(name, rng):
    pa = _pa()
    from physics_amd import scenes
    if name == "64":
        pos, rot, shape, he = _random_scene(rng, 64, 8.0)
        return pos, rot, shape, he, pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE
    if name == "10k":
        pos, rot, shape, he = _random_scene(rng, 10_000, 40.0)
        return pos, rot, shape, he, pa.FLAG_GROUND_PLANE
    if name == "40k":
        sc = scenes.c3(nx=40, ny=25, nz=40)
        return sc.pos, None, sc.shape_type, sc.half_extent, sc.flags
    if name == "big_box":
        sc = scenes.falling_cubes(20, 20, 20, "lattice")
        pos = np.concatenate([sc.pos, [[10.0, 30.0, 5.0]]]).astype(np.float32)
        he = np.concatenate([sc.half_extent, [[20.0, 20.0, 20.0]]]).astype(np.float32)
        shape = np.concatenate([sc.shape_type, [pa.SHAPE_BOX]]).astype(np.uint32)
        return pos, None, shape, he, pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE
    raise ValueError(name)


@pytest.mark.parametrize("name", ["64", "10k", "40k", "big_box"])
def test_random_scene_against_brute_force(name):
    rng = np.random.default_rng({"64": 1, "10k": 2, "40k": 3, "big_box": 4}[name])
    pos, rot, shape, he, flags = _scene(name, rng)
    w = _world(pos, shape, he, rot=rot, flags=flags)
    bodies = _bodies(w, shape, he)
    lo = bodies["pos"].min(0) - 2.0
    hi = bodies["pos"].max(0) + 2.0
    n = 10_000
    o, d = _rays(rng, n, lo, hi)
    mt = np.where(rng.random(n) < 0.3, rng.uniform(0, 50, n), np.inf).astype(np.float32)
    ig = np.where(rng.random(n) < 0.1, rng.integers(0, len(pos), n), 0xFFFFFFFF).astype(np.uint32)
    compare(w, bodies, o, d, label=f"{name} plain")
    compare(w, bodies, o, d, mt, ig, label=f"{name} max_t + ignore")
    w.close()


# ---- 3. the current poses --------------------------------------------------------------------------------------------
def _hip_memcpy_h2d(dst, src):
    from physics_amd import _abi
    paths = _abi.rocm_runtime_mapped()
    assert paths, "no HIP runtime mapped"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(dst), src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0
    assert hip.hipDeviceSynchronize() == 0


def test_current_poses_not_the_last_broad_phase():
    pa = _pa()
    from physics_amd import scenes
    n = 6
    pos = np.array([[4.0 * i, 5.0, 0.0] for i in range(n)], np.float32)
    vel = np.tile([50.0, 0.0, 0.0], (n, 1)).astype(np.float32)
    shape, he = np.full(n, pa.SHAPE_BOX), np.full((n, 3), 0.25, np.float32)
    w = _world(pos, shape, he, lin_vel=vel, gravity_force=(0.0, 0.0, 0.0))
    w.update(scenes.DT_NANOS)
    w.sync()
    now, _ = w.get_transforms()
    assert np.all(now[:, 0] - pos[:, 0] > 0.8)
    down = np.tile([0.0, -1.0, 0.0], (n, 1)).astype(np.float32)
    body, t, _ = w.raycast(now + [0, 10, 0], down)
    assert list(body) == list(range(n)) and np.allclose(t, 10 - 0.25, atol=1e-5)
    body, _, _ = w.raycast(pos + [0, 10, 0], down)  # where the broad phase of that update saw them
    assert list(body) == [pa.RAY_GROUND] * n
    # poses written through the device view are what the next ray cast sees
    v = w.device_view()
    moved = now.copy()
    moved[:, 2] += 7.0
    _hip_memcpy_h2d(v.pos, np.ascontiguousarray(moved, np.float32))
    body, t, _ = w.raycast(moved + [0, 10, 0], down)
    assert list(body) == list(range(n))
    body, _, _ = w.raycast(now + [0, 10, 0], down)
    assert list(body) == [pa.RAY_GROUND] * n
    w.close()


# ---- 4. no side effects ----------------------------------------------------------------------------------------------
def _snapshot(w):
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    st = w.get_stats()
    stats = {k: getattr(st, k) for k, _ in type(st)._fields_}
    return [pos, rot, lin, ang], stats, w.get_manifolds()


def _side_effect_scenes():
    pa = _pa()
    from physics_amd import scenes
    c2 = scenes.c2()
    tower = scenes.c5(16, 130, 16)  # 33 280 boxes in resting contact: the cluster solver and its bucket-order deal
    tower.flags |= pa.FLAG_SOLVER_CLUSTER
    cg = scenes.reference_cg(216)
    cg.shape_type, cg.half_extent = np.full(cg.n, pa.SHAPE_BOX, np.uint32), np.full((cg.n, 3), 0.5, np.float32)
    return {"c2": c2, "cluster_tower": tower, "constraints": cg}


@pytest.mark.parametrize("name", ["c2", "cluster_tower", "constraints"])
def test_ray_casts_leave_updates_bit_identical(name):
    import torch
    pa = _pa()
    from physics_amd import scenes
    sc = _side_effect_scenes()[name]
    worlds = []
    for _ in range(2):
        w = pa.World(sc.config())
        sc.populate(w)
        worlds.append(w)
    quiet, probed = worlds
    rng = np.random.default_rng(3)
    lo, hi = sc.pos.min(0) - 3, sc.pos.max(0) + 3
    o, d = _rays(rng, 3000, lo, hi)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tb = torch.empty(len(o), dtype=torch.int32, device="cuda")
    tt = torch.empty(len(o), dtype=torch.float32, device="cuda")
    tn = torch.empty((len(o), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def probe(w):
        w.raycast(o, d)
        w.raycast_device(to, td, tb, tt, tn)

    hits = 0
    for k in range(20):  # single updates with ray casts in between
        for w in worlds:
            w.update(scenes.DT_NANOS)
        probe(probed)
    for k in range(5):  # batches
        for w in worlds:
            w.update_n(scenes.DT_NANOS, 4)
        probe(probed)
        hits += int((probed.raycast(o, d)[0] < probed.n).sum())
    for w in worlds:
        w.sync()
    a, b = _snapshot(quiet), _snapshot(probed)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    st = probed.get_stats()
    print(f"{name}: {st.n_bodies} bodies, {st.n_manifolds} manifolds, {hits} body hits in the batches")
    assert hits > 0
    for w in worlds:
        w.close()


# ---- 5. determinism --------------------------------------------------------------------------------------------------
def test_determinism_order_and_device_variant():
    import torch
    rng = np.random.default_rng(11)
    pos, rot, shape, he = _random_scene(rng, 10_000, 40.0)
    pa = _pa()
    w = _world(pos, shape, he, rot=rot, flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE)
    o, d = _rays(rng, 30_000, pos.min(0) - 2, pos.max(0) + 2)
    mt = rng.uniform(0, 80, len(o)).astype(np.float32)
    a = w.raycast(o, d, mt)
    b = w.raycast(o, d, mt)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    perm = rng.permutation(len(o))
    c = w.raycast(o[perm], d[perm], mt[perm])
    for x, y in zip(a, c):
        assert np.array_equal(x[perm].view(np.uint32), y.view(np.uint32))
    to, td, tm = (torch.from_numpy(x).cuda() for x in (o, d, mt))
    tb = torch.empty(len(o), dtype=torch.int32, device="cuda")
    tt = torch.empty(len(o), dtype=torch.float32, device="cuda")
    tn = torch.empty((len(o), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w.raycast_device(to, td, tb, tt, tn, max_t=tm)
    w.sync()
    assert np.array_equal(tb.cpu().numpy().view(np.uint32), a[0])
    assert np.array_equal(tt.cpu().numpy().view(np.uint32), a[1].view(np.uint32))
    assert np.array_equal(tn.cpu().numpy().view(np.uint32), a[2].view(np.uint32))
    assert (a[0] < len(pos)).sum() > len(o) // 10
    w.close()


# ---- 6. ghosts -------------------------------------------------------------------------------------------------------
def test_ghost_slots_are_never_hit():
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
    assert right.get_stats().n_ghosts == len(zs)  # the four boundary bodies of the left rank
    n = right.n
    ghost_pos = lpos[:len(zs)]
    down = np.tile([0.0, -1.0, 0.0], (len(zs), 1)).astype(np.float32)
    body, t, _ = right.raycast(ghost_pos + [0, 10, 0], down)
    assert list(body) == [pa.RAY_GROUND] * len(zs), body
    across = np.tile([1.0, 0.0, 0.0], (len(zs), 1)).astype(np.float32)
    body, t, _ = right.raycast(ghost_pos - [10, 0, 0], across)  # through the ghost to the owned body behind it
    assert list(body) == list(range(len(zs))) and np.allclose(t, 10 + 3.0 - 1.0, atol=1e-5)
    rng = np.random.default_rng(5)
    o, d = _rays(rng, 3000, [-25, 0, -10], [25, 10, 10])
    body, _, _ = right.raycast(o, d)
    assert ((body < n) | (body == pa.RAY_MISS) | (body == pa.RAY_GROUND)).all()
    left.close()
    right.close()


# ---- 7. scale --------------------------------------------------------------------------------------------------------
def test_target_1m_million_rays():
    pa = _pa()
    from physics_amd import scenes
    sc = scenes.target_1m()
    w = pa.World(sc.config())
    sc.populate(w)
    w.update_n(scenes.DT_NANOS, 5)
    w.sync()
    rng = np.random.default_rng(1)
    lo, hi = sc.pos.min(0) - 2, sc.pos.max(0) + 2
    o, d = _rays(rng, 1_000_000, lo, hi)
    body, t, nrm = w.raycast(o, d)
    assert body.shape == (1_000_000,) and (body < sc.n).sum() > 300_000
    bodies = _bodies(w, sc.shape_type, sc.half_extent)
    pick = rng.choice(len(o), 256, replace=False)
    compare(w, bodies, o[pick], d[pick], label="target_1m sample", out=(body[pick], t[pick], nrm[pick]))
    w.close()
