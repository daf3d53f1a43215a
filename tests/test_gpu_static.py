"""GPU: static colliders (phys_set_static_bodies). Worlds without statics are unchanged bit for bit; statics take no
colour (a slab under 10,000 cubes); a slab and the ground plane hold cubes at the same height; the manifolds against
statics match closed forms and the body-body path; every solver path gives the same bits; friction on a static ramp
follows Coulomb; containers hold; ray casts match a float64 brute force; runs repeat bit for bit; one update matches
the float64 solver of contact_ref; ghosts of a sharded pair meet a static; a tiled floor's first update has room."""
import math

import numpy as np
import pytest

import contact_ref as cr
import physics_amd
import raycast_ref as ref
from physics_amd import scenes
from test_gpu_independent import quat_to_matrix, sat_separation

pytestmark = pytest.mark.gpu

DT = scenes.DT_NANOS
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
BIT = physics_amd.STATIC_ID_BIT
BOX, SPHERE = physics_amd.SHAPE_BOX, physics_amd.SHAPE_SPHERE
COLL, GROUND = physics_amd.FLAG_COLLISIONS, physics_amd.FLAG_GROUND_PLANE
MARGIN = 0.02


def _quat_z(angle):
    return np.array([0.0, 0.0, math.sin(angle / 2), math.cos(angle / 2)], np.float32)


def _statics(boxes=(), spheres=()):
    """boxes: (centre, half extent[, quaternion]); spheres: (centre, radius) -> arrays for set_static_bodies"""
    pos, rot, shape, he = [], [], [], []
    for b in boxes:
        pos.append(b[0]); he.append(b[1]); rot.append(b[2] if len(b) > 2 else [0, 0, 0, 1]); shape.append(BOX)
    for c, r in spheres:
        pos.append(c); he.append([r, r, r]); rot.append([0, 0, 0, 1]); shape.append(SPHERE)
    return (np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(rot, np.float32).reshape(-1, 4),
            np.asarray(shape, np.uint32), np.asarray(he, np.float32).reshape(-1, 3))


def _set(w, st):
    pos, rot, shape, he = st
    w.set_static_bodies(pos, rot=rot, shape_type=shape, half_extent=he)


def _container(x0, x1, z0, z1, floor_top, height, wall=1.0):
    """floor slab + four walls around [x0, x1] x [z0, z1]"""
    cx, cz, hx, hz = (x0 + x1) / 2, (z0 + z1) / 2, (x1 - x0) / 2, (z1 - z0) / 2
    yb = floor_top + height / 2
    return [([cx, floor_top - wall, cz], [hx + 2 * wall, wall, hz + 2 * wall]),
            ([x0 - wall, yb, cz], [wall, height / 2, hz + 2 * wall]), ([x1 + wall, yb, cz], [wall, height / 2, hz + 2 * wall]),
            ([cx, yb, z0 - wall], [hx, height / 2, wall]), ([cx, yb, z1 + wall], [hx, height / 2, wall])]


def _world(sc, flags=None, **cfg):
    w = physics_amd.World(sc.config(**({"flags": flags} if flags is not None else {}), **cfg))
    sc.populate(w)
    return w


def _state(w):
    p, q = w.get_transforms()
    v, a = w.get_velocities()
    return [x.copy() for x in (p, q, v, a)]


def test_far_statics_change_no_bit():
    """C2-sized scene: a static set far from every body gives the poses and velocities of the same scene without one."""
    sc = scenes.c2()
    far = _statics(boxes=[([5000, 0, 5000], [3, 3, 3]), ([-4000, 100, 0], [50, 1, 50])], spheres=[([0, 9000, 0], 5.0)])
    runs = []
    for with_statics in (False, True):
        w = _world(sc)
        if with_statics:
            _set(w, far)
        for _ in range(5):
            w.update_n(DT, 10)
            w.sync()
        runs.append(_state(w))
        if with_statics:
            assert w.get_static_stats() == (3, 0, 0)
        w.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _layer_on_slab(nx, nz, top, spacing=2.5, drop=0.3):
    xs, zs = np.meshgrid(np.arange(nx) * spacing, np.arange(nz) * spacing, indexing="ij")
    n = nx * nz
    pos = np.column_stack([xs.ravel(), np.full(n, top + 0.5 + drop), zs.ravel()]).astype(np.float32)
    return pos


def test_ten_thousand_cubes_rest_on_one_static_slab():
    """Beyond the 64-manifold cap: a body holding 10,000 manifolds is PHYS_ERR_CAPACITY; a static slab takes no colour."""
    top = 1.0
    pos = _layer_on_slab(100, 100, top)
    n = len(pos)
    cfg = physics_amd.default_config(flags=COLL, gravity_offset=(0, 0, 0))
    w = physics_amd.World(cfg)
    w.set_bodies(pos, shape_type=np.full(n, BOX, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))
    span = 100 * 2.5
    _set(w, _statics(boxes=[([span / 2, top - 0.5, span / 2], [span / 2 + 5, 0.5, span / 2 + 5])]))
    for _ in range(4):
        w.update_n(DT, 50)
        w.sync()  # raises PhysError on PHYS_ERR_CAPACITY
    p, _ = w.get_transforms()
    v, a = w.get_velocities()
    slop = cfg.slop
    assert np.abs(p[:, 1] - (top + 0.5)).max() <= slop + 1e-3, np.abs(p[:, 1] - (top + 0.5)).max()
    assert np.abs(v).max() < 0.02 and np.abs(a).max() < 0.02
    n_st, n_pairs, n_man = w.get_static_stats()
    assert (n_st, n_pairs, n_man) == (1, n, n)
    st = w.get_stats()
    assert st.n_ground_manifolds == 0 and st.n_manifolds == n and st.overflow == 0
    w.close()


def test_static_slab_holds_cubes_at_the_height_of_the_plane():
    h = 1.5
    pos = _layer_on_slab(8, 8, h, spacing=1.7)
    n = len(pos)
    ys = []
    for use_slab in (False, True):
        cfg = physics_amd.default_config(flags=COLL | (0 if use_slab else GROUND), ground_height=h, gravity_offset=(0, 0, 0))
        w = physics_amd.World(cfg)
        w.set_bodies(pos, shape_type=np.full(n, BOX, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))
        if use_slab:
            _set(w, _statics(boxes=[([6, h - 2.0, 6], [40, 2.0, 40])]))
        w.update_n(DT, 150)
        w.sync()
        ys.append(w.get_transforms()[0][:, 1].copy())
        w.close()
    assert np.abs(ys[0] - ys[1]).max() <= cfg.slop, np.abs(ys[0] - ys[1]).max()


def test_manifolds_against_statics_match_closed_forms_and_the_body_path():
    """Spheres against static spheres / boxes: closed forms in float64. Boxes against static boxes: the manifold of the
    body-body path for the same two shapes (B a body placed where the static is)."""
    rng = np.random.default_rng(11)
    n = 600
    base = np.column_stack([np.arange(n) % 25 * 14.0, np.zeros(n), np.arange(n) // 25 * 14.0])
    kind = rng.integers(0, 4, n)  # 0 sphere-static sphere, 1 sphere-static box, 2 box-static box, 3 box-static sphere
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rotA = q.astype(np.float32)
    q2 = rng.normal(size=(n, 4))
    q2 /= np.linalg.norm(q2, axis=1, keepdims=True)
    rotS = q2.astype(np.float32)
    heA = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    heS = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    shapeA = np.where(kind >= 2, BOX, SPHERE).astype(np.uint32)
    shapeS = np.where((kind == 0) | (kind == 3), SPHERE, BOX).astype(np.uint32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    reach = np.where(shapeA == SPHERE, heA[:, 0], np.linalg.norm(heA, axis=1)) + np.where(shapeS == SPHERE, heS[:, 0], np.linalg.norm(heS, axis=1))
    posS = base.astype(np.float32)
    posA = (base + d * reach[:, None] * rng.uniform(0.45, 0.9, (n, 1))).astype(np.float32)
    kw = dict(flags=COLL, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0))
    w = physics_amd.World(physics_amd.default_config(**kw))
    w.set_bodies(posA, rot=rotA, shape_type=shapeA, half_extent=heA)
    w.set_static_bodies(posS, rot=rotS, shape_type=shapeS, half_extent=heS)
    w.update(DT)
    w.sync()
    ids, counts, normals, points = w.get_manifolds()
    got = {(int(a), int(b)): (int(c), nn.astype(np.float64), p.astype(np.float64)) for (a, b), c, nn, p in zip(ids, counts, normals, points)}
    assert all(b & BIT for _, b in got) and len(got) == w.get_static_stats()[2]
    # the body path: body 2k = A, body 2k + 1 = the static's shape as a body
    pb = np.empty((2 * n, 3), np.float32); pb[0::2] = posA; pb[1::2] = posS
    rb = np.empty((2 * n, 4), np.float32); rb[0::2] = rotA; rb[1::2] = rotS
    hb = np.empty((2 * n, 3), np.float32); hb[0::2] = heA; hb[1::2] = heS
    sb = np.empty(2 * n, np.uint32); sb[0::2] = shapeA; sb[1::2] = shapeS
    w2 = physics_amd.World(physics_amd.default_config(**kw))
    w2.set_bodies(pb, rot=rb, shape_type=sb, half_extent=hb)
    w2.update(DT)
    w2.sync()
    ids2, counts2, normals2, points2 = w2.get_manifolds()
    body = {(int(a), int(b)): (int(c), nn.astype(np.float64), p.astype(np.float64)) for (a, b), c, nn, p in zip(ids2, counts2, normals2, points2)}
    checked = checked_box_sphere = checked_box_box = 0
    for k in range(n):
        s = got.get((k, BIT | k))
        b2 = body.get((2 * k, 2 * k + 1))
        assert (s is None) == (b2 is None), k
        if s is None:
            continue
        assert s[0] == b2[0] and np.array_equal(s[1], b2[1]) and np.array_equal(s[2], b2[2]), k
        if kind[k] == 0:
            cA, cS = posA[k].astype(np.float64), posS[k].astype(np.float64)
            dist = np.linalg.norm(cS - cA)
            nexp = (cS - cA) / dist
            dep = float(heA[k, 0]) + float(heS[k, 0]) - dist
            assert s[0] == 1 and np.abs(s[1] - nexp).max() < 1e-4 and abs(s[2][0, 3] - dep) < 1e-4
            assert np.abs(s[2][0, :3] - (cA + nexp * (float(heA[k, 0]) - 0.5 * dep))).max() < 1e-4
            checked += 1
        elif kind[k] == 1:
            # sphere A against box S: the closest point of the box to the sphere's centre
            qq = rotS[k].astype(np.float64)
            i, j, kk, ww = qq / np.linalg.norm(qq)
            R = np.array([[1 - 2 * (j * j + kk * kk), 2 * (i * j - kk * ww), 2 * (i * kk + j * ww)],
                          [2 * (i * j + kk * ww), 1 - 2 * (i * i + kk * kk), 2 * (j * kk - i * ww)],
                          [2 * (i * kk - j * ww), 2 * (j * kk + i * ww), 1 - 2 * (i * i + j * j)]])
            cA, cS = posA[k].astype(np.float64), posS[k].astype(np.float64)
            local = (cA - cS) @ R
            ql = np.clip(local, -heS[k].astype(np.float64), heS[k].astype(np.float64))
            if np.array_equal(ql, local):
                continue
            qw = cS + R @ ql
            dist = np.linalg.norm(qw - cA)
            assert s[0] == 1 and np.abs(s[1] - (qw - cA) / dist).max() < 1e-4
            assert abs(s[2][0, 3] - (float(heA[k, 0]) - dist)) < 1e-4 and np.abs(s[2][0, :3] - qw).max() < 1e-4
            checked += 1
        elif kind[k] == 3:
            # box A against sphere S: the closest point q of the box to the sphere's centre; normal A -> B = (s - q) / |s - q|
            cA, cS = posA[k].astype(np.float64), posS[k].astype(np.float64)
            RA, hA, r = quat_to_matrix(rotA[k].astype(np.float64)), heA[k].astype(np.float64), float(heS[k, 0])
            local = (cS - cA) @ RA
            ql = np.clip(local, -hA, hA)
            if np.array_equal(ql, local):
                continue  # the sphere's centre inside the box: no closed form (the body path above checks it)
            qw = cA + RA @ ql
            dist = np.linalg.norm(cS - qw)
            assert s[0] == 1 and np.abs(s[1] - (cS - qw) / dist).max() < 1e-4
            assert abs(s[2][0, 3] - (r - dist)) < 1e-4 and np.abs(s[2][0, :3] - qw).max() < 1e-4
            checked_box_sphere += 1
        else:
            # box A against box S, float64 SAT (tests/test_gpu_independent.py): the normal is a unit vector from A
            # towards S along one of the 15 axes and a near-minimum-penetration one, and no point is deeper than the
            # overlap along it
            cA, cS = posA[k].astype(np.float64), posS[k].astype(np.float64)
            RA, RS = quat_to_matrix(rotA[k].astype(np.float64)), quat_to_matrix(rotS[k].astype(np.float64))
            hA, hS = heA[k].astype(np.float64), heS[k].astype(np.float64)
            s_star, _ = sat_separation(cA, RA, hA, cS, RS, hS)
            count, normal, pts = s
            assert s_star <= MARGIN + 1e-3, f"pair {k}: separated by {s_star} along a SAT axis, yet a manifold"
            assert 1 <= count <= 4 and abs(np.linalg.norm(normal) - 1.0) < 1e-4 and normal @ (cS - cA) > -1e-4
            _, seps_all = sat_separation(cA, RA, hA, cS, RS, hS, min_cross=0.0099)
            along = [sv for sv, L, _, _ in seps_all if abs(abs(L @ normal) - 1.0) < 2e-4]
            assert along, f"pair {k}: normal {normal} is none of the 15 SAT axes"
            assert max(along) >= s_star - (0.03 + 0.11 * abs(s_star)) - 1e-4
            assert pts[:count, 3].max() <= -min(along) + 1e-4, (k, pts[:count, 3], along)
            checked_box_box += 1
    assert checked > 100 and checked_box_sphere > 40 and checked_box_box > 60, (checked, checked_box_sphere, checked_box_box)
    w.close(); w2.close()


def _around(sc, room, height):
    """a static container around the scene's bodies, `room` from the outermost centres to the inner wall faces"""
    lo, hi = sc.pos.min(axis=0), sc.pos.max(axis=0)
    return _container(float(lo[0]) - room, float(hi[0]) + room, float(lo[2]) - room, float(hi[2]) + room, 0.0, height)


def _tower(nx, ny, nz):
    sc = scenes.falling_cubes(nx, ny, nz, "static_tower")
    return sc, _statics(boxes=_around(sc, 1.5, ny * 2.5 + 10))


def _hash(w):
    return tuple(hash(x.tobytes()) for x in _state(w))


def test_every_solver_path_gives_the_same_bits_in_a_static_container():
    sc, st = _tower(16, 130, 16)
    flags = sc.flags & ~GROUND
    hashes = []
    for extra in (0, physics_amd.FLAG_SOLVER_PER_COLOR, physics_amd.FLAG_SOLVER_CLUSTER):
        w = _world(sc, flags=flags | extra)
        _set(w, st)
        for _ in range(7):
            w.update_n(DT, 10)
            w.sync()
        assert w.get_static_stats()[2] >= 16 * 16 and w.get_transforms()[0][:, 1].min() > 0.0
        hashes.append(_hash(w))
        w.close()
    assert hashes[0] == hashes[1] == hashes[2]


@pytest.mark.parametrize("mu,theta_deg", [(0.5, 15.0), (0.1, 20.0), (0.2, 25.0)])
def test_box_on_a_static_ramp_follows_coulomb(mu, theta_deg):
    th = math.radians(theta_deg)
    q = _quat_z(-th)
    up = np.array([math.sin(th), math.cos(th), 0.0])
    down = np.array([math.cos(th), -math.sin(th), 0.0])
    cfg = physics_amd.default_config(flags=COLL, friction=mu, gravity_offset=(0, 0, 0))
    w = physics_amd.World(cfg)
    w.set_bodies((up * 1.505).astype(np.float32)[None], rot=q[None], shape_type=np.array([BOX], np.uint32),
                 half_extent=np.full((1, 3), 0.5, np.float32))
    _set(w, _statics(boxes=[([0, 0, 0], [60, 1, 5], q)]))
    w.update_n(DT, 20)
    w.sync()
    s0 = float(w.get_transforms()[0][0] @ down)
    v0 = float(w.get_velocities()[0][0] @ down)
    w.update_n(DT, 60)
    w.sync()
    s1 = float(w.get_transforms()[0][0] @ down)
    v1 = float(w.get_velocities()[0][0] @ down)
    g = 9.81
    want = g * (math.sin(th) - mu * math.cos(th))
    if want <= 0:
        assert abs(s1 - s0) < 0.02 and abs(v1) < 0.01, (s1 - s0, v1)
    else:
        acc = (v1 - v0) / (60 * DT_S)
        assert abs(acc - want) <= 0.05 * want, (acc, want)
    assert w.get_static_stats()[2] == 1
    w.close()


def test_cubes_never_leave_a_static_container():
    sc = scenes.falling_cubes(6, 8, 6, "static_box", spacing=1.6, y0=2.0)
    walls = _around(sc, 3.0, 40.0)
    lo = np.array([walls[1][0][0] + 1.0, 0.0, walls[3][0][2] + 1.0])  # inner faces of the walls, top of the floor
    hi = np.array([walls[2][0][0] - 1.0, 40.0, walls[4][0][2] - 1.0])
    w = _world(sc, flags=sc.flags & ~GROUND)
    _set(w, _statics(boxes=walls))
    for _ in range(10):
        w.update_n(DT, 50)
        w.sync()
        p = w.get_transforms()[0]
        assert (p > lo).all() and (p < hi).all(), (p.min(axis=0), p.max(axis=0))
    assert w.get_static_stats()[2] >= 36  # the bottom layer at least rests on the floor
    w.close()


def test_ray_casts_hit_statics_like_a_float64_brute_force():
    from test_gpu_raycast import compare
    rng = np.random.default_rng(5)
    n, ns = 300, 120
    pos = rng.uniform(-30, 30, (n, 3)).astype(np.float32); pos[:, 1] = np.abs(pos[:, 1]) + 1
    shape = rng.choice([BOX, SPHERE], n).astype(np.uint32)
    he = rng.uniform(0.3, 2.0, (n, 3)).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32); rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    spos = rng.uniform(-30, 30, (ns, 3)).astype(np.float32); spos[:, 1] = np.abs(spos[:, 1]) + 1
    sshape = rng.choice([BOX, SPHERE], ns).astype(np.uint32)
    she = rng.uniform(0.3, 3.0, (ns, 3)).astype(np.float32)
    srot = rng.normal(size=(ns, 4)).astype(np.float32); srot /= np.linalg.norm(srot, axis=1, keepdims=True)
    w = physics_amd.World(physics_amd.default_config(flags=GROUND, ground_height=0.0))
    w.set_bodies(pos, rot=rot, shape_type=shape, half_extent=he)
    w.set_static_bodies(spos, rot=srot, shape_type=sshape, half_extent=she)
    o = rng.uniform(-40, 40, (20000, 3)).astype(np.float32); o[:, 1] = rng.uniform(0.5, 40, 20000)
    d = rng.normal(size=(20000, 3)).astype(np.float32)
    body, t, nrm = w.raycast(o, d)
    st = ((body & BIT) != 0) & (body != ref.GROUND) & (body != ref.MISS)
    assert st.sum() > 500 and (body < n).sum() > 500 and (body == ref.GROUND).sum() > 500
    mapped = body.astype(np.int64).copy()
    mapped[st] = n + (body[st] & ~np.uint32(BIT))
    both = dict(pos=np.concatenate([pos, spos]).astype(np.float64), rot=np.concatenate([rot, srot]).astype(np.float64),
                half_extent=np.concatenate([he, she]).astype(np.float64), shape=np.concatenate([shape, sshape]))
    compare(w, both, o, d, ground=0.0, out=(mapped.astype(np.uint32), t, nrm))
    w.close()


def test_exact_ties_go_to_bodies_then_statics_then_ground():
    # top faces at y = 0: body 0 and static 0 under the first ray, static 1 and the ground under the second, the ground
    # alone under the third
    w = physics_amd.World(physics_amd.default_config(flags=GROUND, ground_height=0.0))
    w.set_bodies(np.array([[0, -1, 0]], np.float32), shape_type=np.array([BOX], np.uint32), half_extent=np.ones((1, 3), np.float32))
    w.set_static_bodies(np.array([[0, -1, 0], [10, -1, 0]], np.float32), shape_type=np.array([BOX, BOX], np.uint32),
                        half_extent=np.ones((2, 3), np.float32))
    o = np.array([[0, 5, 0], [10, 5, 0], [20, 5, 0]], np.float32)
    d = np.array([[0, -1, 0]] * 3, np.float32)
    body, t, _ = w.raycast(o, d)
    assert body.tolist() == [0, BIT | 1, physics_amd.RAY_GROUND] and t.tolist() == [5.0, 5.0, 5.0]
    w.close()


def test_ray_casts_between_updates_leave_them_bit_identical():
    sc, st = _tower(6, 10, 6)
    runs = []
    for rays in (False, True):
        w = _world(sc, flags=sc.flags & ~GROUND)
        _set(w, st)
        rng = np.random.default_rng(3)
        for _ in range(6):
            w.update_n(DT, 10)
            if rays:
                w.raycast(rng.uniform(-5, 20, (4096, 3)).astype(np.float32), rng.normal(size=(4096, 3)).astype(np.float32))
            w.sync()
        runs.append(_hash(w))
        w.close()
    assert runs[0] == runs[1]


def test_runs_repeat_and_a_replaced_set_forgets_the_warm_start():
    sc, st = _tower(8, 20, 8)
    hashes = []
    for _ in range(2):
        w = _world(sc, flags=sc.flags & ~GROUND)
        _set(w, st)
        w.update_n(DT, 60)
        w.sync()
        hashes.append(_hash(w))
        w.close()
    assert hashes[0] == hashes[1]
    # replacing the set with the same set: the next update colours afresh and starts cold, like a new world from here
    w = _world(sc, flags=sc.flags & ~GROUND)
    _set(w, st)
    w.update_n(DT, 40)
    w.sync()
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    _set(w, st)
    w.update(DT)
    w.sync()
    st1 = w.get_stats()
    m1 = w.get_manifolds()
    assert st1.n_new_manifolds == st1.n_manifolds  # nothing kept: no colour, no warm start
    w2 = physics_amd.World(sc.config(flags=sc.flags & ~GROUND))
    w2.set_bodies(pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=sc.shape_type, half_extent=sc.half_extent)
    _set(w2, st)
    w2.update(DT)
    w2.sync()
    m2 = w2.get_manifolds()
    for a, b in zip(m1, m2):
        assert np.array_equal(a, b)
    assert _hash(w) == _hash(w2)
    w.close(); w2.close()


def _ref_update_with_statics(ref_obj, n, st_pos, man, pos, lin, ang, inv_m, inv_I, force):
    """contact_ref.SolverRef through a thin wrapper: static k becomes extra body n + k with zero inverse mass and inertia
    and zero velocity (so its rows are one-sided: rB x impulse x 0), and the colour priority keeps hashing the full pair
    (a, PHYS_STATIC_ID_BIT | k). The reference colours the extra body like any other; with ONE manifold per static (the
    caller checks) that changes no colour: its `top` is that manifold's own priority and its `used` mask is empty."""
    ids, counts, normals, points = man
    ids = np.asarray(ids, np.int64).copy()
    st = ((ids[:, 1] & BIT) != 0) & (ids[:, 1] != ref.GROUND)
    ids[st, 1] = n + (ids[st, 1] - BIT)
    k = len(st_pos)
    z3 = np.zeros((k, 3))
    orig = cr.color_priority

    def full_pair_priority(a, b):
        b = np.asarray(b, np.int64)
        return orig(a, np.where((b >= n) & (b != cr.GROUND), BIT | (b - n), b))

    cr.color_priority = full_pair_priority
    try:
        return ref_obj.update((ids, counts, normals, points), np.concatenate([pos, st_pos]), np.concatenate([lin, z3]),
                              np.concatenate([ang, z3]), np.concatenate([inv_m, np.zeros(k)]),
                              np.concatenate([inv_I, np.zeros((k, 3, 3))]), np.concatenate([force, z3]))
    finally:
        cr.color_priority = orig


@pytest.mark.parametrize("solver", ["default", "per_color"])
def test_one_update_on_static_boxes_against_the_float64_solver(solver):
    """Sliding and spinning boxes and spheres on static boxes (some with a second box on top): one update of the
    device's solver against contact_ref.SolverRef, tolerance of the coupled piles of test_gpu_solver_independent."""
    bodies, statics = cr.static_boxes(21, 120)  # (the scene moved there as it was: tests/test_contact_ref_cpu.py runs it too)
    pos, rot, lin, ang, shape, he = (bodies[k] for k in ("pos", "rot", "lin_vel", "ang_vel", "shape_type", "half_extent"))
    st_pos, st_he, n_st, n = statics["pos"].astype(np.float64), statics["half_extent"], len(statics["pos"]), len(pos)
    flags = COLL | (physics_amd.FLAG_SOLVER_PER_COLOR if solver == "per_color" else 0)
    w = physics_amd.World(physics_amd.default_config(flags=flags, gravity_offset=(0, 0, 0)))
    w.set_bodies(pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=shape, half_extent=he)
    w.set_static_bodies(st_pos.astype(np.float32), shape_type=np.full(n_st, BOX, np.uint32), half_extent=st_he.astype(np.float32))
    p0, _ = w.get_transforms()
    v0, w0 = w.get_velocities()
    w.update(DT)
    w.sync()
    man = w.get_manifolds()
    lin1, ang1 = w.get_velocities()
    b = man[0][:, 1].astype(np.int64)
    st_b = b[(b & BIT) != 0]
    assert len(st_b) >= 100 and len(np.unique(st_b)) == len(st_b), "one manifold per static (the wrapper's condition)"
    assert ((b & BIT) == 0).sum() >= 20, "body-body manifolds on top of the static ones"
    inv_m, inv_I = cr.body_inverses(n)
    ref_obj = cr.SolverRef(n + n_st, cr.Params(DT_S), 8)
    force = np.tile([0.0, -9.81, 0.0], (n, 1))
    out = _ref_update_with_statics(ref_obj, n, st_pos.astype(np.float32).astype(np.float64), man, p0, v0, w0, inv_m, inv_I, force)
    assert out["n_colors"] == w.get_stats().n_colors
    assert np.array_equal(np.bincount(out["colors"], minlength=64)[:64], w.get_color_counts())
    err, amb = cr.velocity_error(out, np.concatenate([lin1, np.zeros((n_st, 3))]), np.concatenate([ang1, np.zeros((n_st, 3))]))
    assert amb <= 2
    assert err < 2e-5, err  # TOL_COUPLED of test_gpu_solver_independent
    w.close()


def test_sharded_ghosts_meet_a_static_floor_and_runs_repeat():
    """Two ranks in the style of test_gpu_ghosts (no ground plane): each sets the same static floor; ghosts of the
    boundary bodies rest on it in the receiving world. No error over the run, and the run repeats bit for bit."""
    from test_gpu_ghosts import TwoRanks, _two_piles
    pos, vel = _two_piles()
    floor = _statics(boxes=[([0.0, -1.0, 0.0], [200.0, 1.0, 200.0])])
    runs = []
    for _ in range(2):
        t = TwoRanks(pos, vel, ground=False)
        for w in t.worlds:
            _set(w, floor)
        ghost_static = 0
        for _chunk in range(16):
            t.step(10)
            for w in t.worlds:
                s = w.get_stats()
                assert s.overflow == 0
                ids = w.get_manifolds()[0].astype(np.int64)
                ghost_static += int(((ids[:, 0] >= s.n_bodies) & ((ids[:, 1] & BIT) != 0) & (ids[:, 1] != ref.GROUND)).sum())
        assert ghost_static > 0, "no ghost met the static floor"
        assert t.positions()[:, 1].min() > 0.8  # unit half extents resting on the floor's top at y = 0
        runs.append(t.state())
        t.close()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b), "the sharded run with statics is not reproducible"


def test_first_update_sizes_the_pairs_of_a_tiled_floor():
    """Each cube over a floor of tiles smaller than itself meets 4 to 9 of them: more than the starting budget of four
    pairs per body. The first update measures the count and sizes the buffer: no capacity error, no skipped solve."""
    t = 84
    ti, tj = np.meshgrid(np.arange(t), np.arange(t), indexing="ij")
    tiles = [([0.6 * i, -0.25, 0.6 * j], [0.3, 0.25, 0.3]) for i, j in zip(ti.ravel(), tj.ravel())]
    cx, cz = np.meshgrid(np.arange(20) * 2.5 + 1.0, np.arange(20) * 2.5 + 1.0, indexing="ij")
    n = cx.size
    pos = np.column_stack([cx.ravel(), np.full(n, 0.49), cz.ravel()]).astype(np.float32)
    w = physics_amd.World(physics_amd.default_config(flags=COLL, gravity_offset=(0, 0, 0)))
    w.set_bodies(pos, shape_type=np.full(n, BOX, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))
    _set(w, _statics(boxes=tiles))
    w.update(DT)
    w.sync()  # raises PhysError on PHYS_ERR_CAPACITY
    n_st, n_pairs, n_man = w.get_static_stats()
    assert n_st == t * t and n_pairs > 4 * n and n_man >= n
    w.update_n(DT, 60)
    w.sync()
    p = w.get_transforms()[0]
    assert np.abs(p[:, 1] - 0.5).max() < 0.02
    w.close()


def test_pair_offsets_carry_past_1024_workgroups():
    """k_static_scan scans the per-workgroup pair counts 1024 at a time with a carry: the second trip starts at workgroup
    1024 = body 1024 * 256. One body more than that, on a sparse lattice, with one static box through five of them - the
    last body (the second trip: its offset is the carry) and four spread over the first trip. The pair count and the
    pair set (every pair here penetrates, so each is a manifold against the static) must equal a numpy AABB-overlap
    count over the same arrays."""
    n = 1024 * 256 + 1
    k = np.arange(64 * 64 * 65)[:n]
    pos = (3.0 * np.column_stack([k % 64, (k // 64) % 64, k // 4096]) + [0.0, 0.0, 30.0]).astype(np.float32)
    touched = np.array([5, 70_000, 200_000, n - 2, n - 1])
    pos[touched] = [[3.0 * j, 0.0, 0.0] for j in range(5)]  # a row of their own, clear of the lattice
    box_c, box_h = np.array([6.0, 0.0, 0.0]), np.array([6.2, 0.3, 0.3])
    w = physics_amd.World(physics_amd.default_config(flags=COLL, gravity_offset=(0, 0, 0)))  # (contact margin: MARGIN)
    w.set_bodies(pos, shape_type=np.full(n, BOX, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))
    _set(w, _statics(boxes=[(box_c, box_h)]))
    w.update(DT)
    w.sync()
    aabb = w.get_aabbs()
    lo, hi = aabb[:, :3], aabb[:, 3:]
    hit = np.all((lo <= box_c + box_h + MARGIN) & (hi >= box_c - box_h - MARGIN), axis=1)
    assert sorted(np.flatnonzero(hit)) == sorted(touched), "the scene is not the one the test describes"
    n_st, n_pairs, n_man = w.get_static_stats()
    assert (n_st, n_pairs, n_man) == (1, int(hit.sum()), int(hit.sum()))
    ids = w.get_manifolds()[0]
    got = sorted((int(a), int(b)) for a, b in ids if b & BIT)
    assert got == [(int(i), BIT | 0) for i in sorted(touched)]
    w.close()
