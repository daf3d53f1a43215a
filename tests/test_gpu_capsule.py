"""GPU: capsule bodies and static capsules (PHYS_SHAPE_CAPSULE). A soup of every shape has the oracle's AABBs, pairs and
manifolds bit for bit; a capsule pile steps bit for bit with the oracle on every solver path; capsules settle at their
resting heights; static capsules hold bodies; ray casts hit capsules as the float64 reference does; ray casts change
nothing of a run; a capsule that is a ghost of another rank collides."""
import numpy as np
import pytest

import capsule_ref as cref
import physics_amd
from physics_amd import scenes

pytestmark = pytest.mark.gpu

DT = scenes.DT_NANOS
CAP, BOX, SPHERE = physics_amd.SHAPE_CAPSULE, physics_amd.SHAPE_BOX, physics_amd.SHAPE_SPHERE
COLL, GROUND = physics_amd.FLAG_COLLISIONS, physics_amd.FLAG_GROUND_PLANE
S = float(np.sqrt(0.5))
Q_X = [0.0, 0.0, S, S]  # the capsule's axis along x


def _oracle(cfg):
    from oracle import binding as ob
    return ob.OracleWorld(cfg, trig=ob.TRIG_DET)


def _compare_state(w, o, what=""):
    for name, a, b in zip(("pos", "rot", "lin", "ang"), w.get_transforms() + w.get_velocities(), o.get_transforms() + o.get_velocities()):
        assert np.array_equal(a, b), f"{what} {name}: max abs diff {np.abs(a - b).max()}"


def _compare_manifolds(w, o):
    for a, b, name in zip(w.get_manifolds(), o.get_manifolds(), ("ids", "counts", "normals", "points")):
        assert a.shape == b.shape and np.array_equal(a, b), name


def _soup(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-6, 6, size=(n, 3)).astype(np.float32)
    pos[:, 1] += 6.5
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    st = rng.integers(0, 4, n).astype(np.uint32)
    he = rng.uniform(0.3, 1.0, size=(n, 3)).astype(np.float32)
    return pos, q, st, he


def test_soup_of_every_shape_matches_the_oracle_bit_for_bit():
    pos, q, st, he = _soup(1500, 11)
    cfg = physics_amd.default_config(flags=COLL | GROUND, gravity_offset=(0, 0, 0))
    w, o = physics_amd.World(cfg), _oracle(physics_amd.default_config(flags=COLL | GROUND, gravity_offset=(0, 0, 0)))
    for x in (w, o):
        x.set_bodies(pos, rot=q, shape_type=st, half_extent=he)
    assert np.array_equal(w.broadphase(), o.broadphase())
    assert np.array_equal(w.get_aabbs(), o.get_aabbs())
    for x in (w, o):
        x.update_n(DT, 3)
    w.sync()
    _compare_manifolds(w, o)
    _compare_state(w, o, "soup")
    ids, counts, _, _ = w.get_manifolds()
    b = ids[:, 1]
    isb = b < len(st)
    cap_b = np.zeros(len(b), bool)
    cap_b[isb] = st[b[isb]] == CAP
    with_cap = (st[ids[:, 0]] == CAP) | cap_b
    assert with_cap.sum() > 50, "the soup has few capsule contacts"
    assert (counts[with_cap] == 2).any()
    w.close()
    o.close()


def _run_pile(sc, flags_extra, steps, chunk, threads=1, profile_stage=None):
    w = physics_amd.World(sc.config(flags=sc.flags | flags_extra))
    o = _oracle(sc.config())
    if threads > 1:
        o.set_threads(threads)
    for x in (w, o):
        sc.populate(x)
    done = 0
    prof = None
    while done < steps:
        k = min(chunk, steps - done)
        if profile_stage and done + k >= steps:
            w.profile_enable(True)
        w.update_n(DT, k)
        o.update_n(DT, k)
        done += k
        w.sync()
        _compare_state(w, o, f"{sc.name} update {done}")
    if profile_stage:
        prof, _ = w.profile_get()
    st = w.get_stats()
    w.close()
    o.close()
    return st, prof


@pytest.mark.parametrize("flag", [0, physics_amd.FLAG_SOLVER_PER_COLOR])
def test_capsule_pile_steps_bit_for_bit_with_the_oracle(flag):
    sc = scenes.capsule_pile(8, 6, 8)
    st, _ = _run_pile(sc, flag, 90, 30)
    assert st.n_manifolds > 100


def test_capsule_tower_on_the_cluster_solver_is_bit_exact():
    """Lying capsules in resting contact (16 x 160 x 16, touching along y and z): enough manifolds that the cluster
    solver runs when PHYS_FLAG_SOLVER_CLUSTER asks for it."""
    nx, ny, nz = 16, 160, 16
    pos = scenes.lattice(nx, ny, nz, 1.0, 0.5, 0.0)
    pos[:, 0] *= 2.05  # the capsules lie along x, 2 long: a small gap between them along x
    n = len(pos)
    sc = scenes.Scene("capsule_tower", pos, np.full(n, CAP, np.uint32), np.tile(np.float32([0.5, 0.5, 0.0]), (n, 1)),
                      COLL | GROUND, rot=np.tile(np.float32(Q_X), (n, 1)))
    st, prof = _run_pile(sc, physics_amd.FLAG_SOLVER_CLUSTER, 12, 8, threads=16, profile_stage=True)
    assert "solve_cluster" in prof, f"the cluster solver did not run: {sorted(prof)}"
    assert st.n_manifolds > 50_000


def _settle(pos, rot, he, steps=240):
    w = physics_amd.World(physics_amd.default_config(flags=COLL | GROUND, gravity_offset=(0, 0, 0)))
    n = len(pos)
    w.set_bodies(np.float32(pos), rot=np.float32(rot), shape_type=np.full(n, CAP, np.uint32), half_extent=np.float32(he),
                 inertia=np.tile(physics_amd.capsule_inertia(1.0, he[0][0], he[0][1]).reshape(-1), (n, 1)))
    w.update_n(DT, steps)
    w.sync()
    p, q = w.get_transforms()
    v, _ = w.get_velocities()
    w.close()
    return p, q, v


def test_dropped_capsules_settle_lying_and_standing():
    p, _, v = _settle([[0, 1.5, 0]], [Q_X], [[0.5, 1.0, 0.0]])
    assert abs(p[0, 1] - 0.5) < 0.03 and np.abs(v).max() < 0.05
    p, _, v = _settle([[0, 2.0, 0]], [[0, 0, 0, 1]], [[0.5, 1.0, 0.0]], steps=60)
    assert abs(p[0, 1] - 1.5) < 0.03


def test_static_capsules_hold_bodies():
    """A pillar (standing static capsule) holds a sphere on its top; two railings (static capsules lying along x) hold
    a box across them."""
    w = physics_amd.World(physics_amd.default_config(flags=COLL, gravity_offset=(0, 0, 0)))
    w.set_bodies(np.float32([[0, 5.0, 0], [10, 2.0, 0]]), shape_type=np.uint32([SPHERE, BOX]),
                 half_extent=np.float32([[0.5, 0.5, 0.5], [1, 0.5, 1]]))
    w.set_static_bodies(np.float32([[0, 1.5, 0], [10, 0, -0.8], [10, 0, 0.8]]), rot=np.float32([[0, 0, 0, 1], Q_X, Q_X]),
                        shape_type=np.uint32([CAP, CAP, CAP]), half_extent=np.float32([[0.5, 1.5, 0], [0.3, 5, 0], [0.3, 5, 0]]))
    w.update_n(DT, 150)
    w.sync()
    p = w.get_transforms()[0]
    n_st, n_pairs, n_man = w.get_static_stats()
    assert n_st == 3 and n_man == 3
    assert abs(p[0, 1] - 4.0) < 0.03 and abs(p[0, 0]) < 1e-3  # on the pillar's top: 1.5 + 1.5 + 0.5 + 0.5
    assert abs(p[1, 1] - 0.8) < 0.03                        # on the railings: 0.3 + 0.5
    ids, counts, _, _ = w.get_manifolds()
    assert sorted(ids[:, 1].tolist()) == [physics_amd.STATIC_ID_BIT | k for k in range(3)]
    assert sorted(counts.tolist()) == [1, 2, 2]
    w.close()


def _ray_scene(rng, n):
    pos = rng.uniform(-8, 8, size=(n, 3)).astype(np.float32)
    pos[:, 1] += 10
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    he = np.column_stack([rng.uniform(0.2, 0.6, n), rng.uniform(0.0, 1.5, n), np.zeros(n)]).astype(np.float32)
    return pos, q, he


def test_raycasts_hit_capsule_bodies_and_statics_like_the_float64_reference():
    rng = np.random.default_rng(3)
    pos, q, he = _ray_scene(rng, 120)
    spos, sq, she = _ray_scene(rng, 30)
    w = physics_amd.World(physics_amd.default_config(flags=COLL, gravity_offset=(0, 0, 0)))
    w.set_bodies(pos, rot=q, shape_type=np.full(len(pos), CAP, np.uint32), half_extent=he)
    w.set_static_bodies(spos, rot=sq, shape_type=np.full(len(spos), CAP, np.uint32), half_extent=she)
    caps = [(pos[k], q[k], he[k]) for k in range(len(pos))] + [(spos[k], sq[k], she[k]) for k in range(len(spos))]
    ids = list(range(len(pos))) + [physics_amd.STATIC_ID_BIT | k for k in range(len(spos))]
    targets = np.concatenate([pos, spos])[rng.integers(0, len(caps), 1000)] + rng.normal(scale=0.6, size=(1000, 3))
    origins = rng.uniform(-20, 20, size=(1000, 3))
    origins[:, 1] += 10
    origins[:20] = np.concatenate([pos, spos])[:20]  # inside a capsule: t = 0
    dirs = (targets - origins).astype(np.float32)
    dirs[:20] = rng.normal(size=(20, 3))
    origins = origins.astype(np.float32)
    body, t, normal = w.raycast(origins, dirs)
    w.close()
    want = cref.raycast(origins, dirs, caps, ids)
    # rays that graze a capsule: hit or miss could go either way in float32
    fat = cref.raycast(origins, dirs, [(c, qq, h + np.float32([1e-4, 0, 0])) for c, qq, h in caps], ids)
    thin = cref.raycast(origins, dirs, [(c, qq, h - np.float32([1e-4, 0, 0])) for c, qq, h in caps], ids)
    hits = checked = 0
    for k, (kid, kt, kn, gap) in enumerate(want):
        if gap < 1e-3 or fat[k][0] != kid or thin[k][0] != kid:
            continue  # two candidates within rounding of each other, or a grazing ray
        checked += 1
        if kid is None:
            assert body[k] == physics_amd.RAY_MISS, k
            continue
        hits += 1
        assert body[k] == kid, (k, body[k], kid)
        assert abs(t[k] - kt) <= 1e-4 * (1 + kt), (k, t[k], kt)
        assert np.allclose(normal[k], kn, atol=2e-3), (k, normal[k], kn)
    assert checked > 900 and hits > 400
    assert (t[:20] == 0).all()


def test_raycasts_between_updates_change_nothing():
    sc = scenes.capsule_pile(6, 4, 6)
    runs = []
    for cast in (False, True):
        w = physics_amd.World(sc.config())
        sc.populate(w)
        rng = np.random.default_rng(0)
        for _ in range(20):
            w.update_n(DT, 3)
            if cast:
                w.raycast(rng.uniform(-10, 10, size=(500, 3)), rng.normal(size=(500, 3)))
        w.sync()
        runs.append(w.get_transforms() + w.get_velocities())
        w.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_capsule_ghosts_collide_across_the_cut():
    """Two ranks in the style of test_gpu_ghosts, with capsules: two capsules lying along z slide into each other across
    the plane x = 0. The ghosts carry the capsule shape, so each rank sees the other's capsule and they stop."""
    from test_gpu_ghosts import TwoRanks
    pos = np.array([[-2.0, 5.0, 0.0], [2.0, 5.0, 0.0]], np.float32)
    vel = np.array([[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0]], np.float32)
    t = TwoRanks(pos, vel, ground=False, gravity=(0.0, 0.0, 0.0))
    for k, w in enumerate(t.worlds):  # the same bodies again, as capsules (radius 0.5, core half-length 1 along z)
        w.set_bodies(pos[k:k + 1], rot=np.float32([[S, 0, 0, S]]), lin_vel=vel[k:k + 1], shape_type=np.uint32([CAP]),
                     half_extent=np.float32([[0.5, 1.0, 0.0]]))
        w.set_global_ids(np.uint32([k]))
        w.set_slab(-1.0e6 if k == 0 else 0.0, 0.0 if k == 0 else 1.0e6, 4.0)
    ghost_manifolds = 0
    for _ in range(60):
        t.step(1)
        for w in t.worlds:
            s = w.get_stats()
            assert s.overflow == 0
            ids = w.get_manifolds()[0]
            ghost_manifolds += int((ids[:, 1] == 1).sum()) if len(ids) else 0
    p = t.positions()
    t.close()
    assert ghost_manifolds > 0
    assert p[1, 0] - p[0, 0] > 0.95  # two radii apart (not passed through each other)
