"""GPU: box casts (phys_boxcast and its device / filtered variants) against the float64 brute force of tests/boxcast_ref.py,
on the seeded inputs of tests/boxcast_cases.py (the answers of the larger ones are stored under tests/golden/boxcast and
recomputed by tests/test_boxcast_cpu.py).

A hand scene with closed-form answers and invalid queries; random soups of spheres, boxes, capsules and NONE bodies with
statics and the ground; degenerate orientations and sizes; the grid's edges; ignore, max_t and the filtered instance; host
and device variants, batching, NULL outputs, current poses, ghost slots; no side effects on the updates."""
import numpy as np
import pytest

import boxcast_cases as cases
import boxcast_ref as ref
import query_ref
from boxcast_accept import compare_boxcasts, tol_of
from query_accept import cast_cap

pytestmark = pytest.mark.gpu


def _pa():
    import physics_amd
    return physics_amd


def _world(bodies, statics=None, ground=0.0, **cfg):
    pa = _pa()
    flags = pa.FLAG_COLLISIONS | (pa.FLAG_GROUND_PLANE if ground is not None else 0)
    kw = dict(flags=flags, gravity_offset=(0.0, 0.0, 0.0), ground_height=0.0 if ground is None else ground)
    kw.update(cfg)
    w = pa.World(pa.default_config(**kw))
    f = np.float32
    w.set_bodies(np.asarray(bodies["pos"], f), rot=np.asarray(bodies["rot"], f), shape_type=np.asarray(bodies["shape"], np.uint32),
                 half_extent=np.asarray(bodies["half_extent"], f))
    if statics is not None:
        w.set_static_bodies(statics["pos"], rot=statics["rot"], shape_type=statics["shape"], half_extent=statics["half_extent"])
    return w


def _run(c, w=None, out=None):
    """the case through World.boxcast, held to its reference"""
    own = w is None
    if own:
        w = _world(c["bodies"], c["statics"], c["ground"])
    if out is None:
        out = w.boxcast(c["o"], c["d"], c["he"], rot=c["rot"], max_t=c["max_t"], ignore=c["ignore"])
    compare_boxcasts(c["h"], out, label=c["label"], centre=c["centre"])
    if own:
        w.close()
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1. the hand scene ----------------------------------------------------------------------------------------------------------
def test_hand_scene_and_invalid_queries():
    pa = _pa()
    bodies, casts = cases.hand_scene()
    w = _world(bodies)
    o, d = np.array([c["o"] for c in casts], np.float32), np.array([c["d"] for c in casts], np.float32)
    rot = np.array([c["rot"] for c in casts], np.float32)
    he = np.array([c["he"] for c in casts], np.float32)
    body, t, nrm, pnt = w.boxcast(o, d, he, rot=rot)
    for i, c in enumerate(casts):
        print(c["name"], body[i], t[i], nrm[i], pnt[i])
    for i, c in enumerate(casts):
        assert body[i] == c["body"], (c["name"], body[i])
        assert abs(t[i] - c["t"]) <= 1e-5, (c["name"], t[i])
        assert np.abs(nrm[i] - c["normal"]).max() <= 1e-5, (c["name"], nrm[i])
        for a in range(3):
            if c["point"][a] is not None:
                assert abs(pnt[i][a] - c["point"][a]) <= 1e-5, (c["name"], pnt[i])
        for a, lo, hi in cases.FREE_RANGE.get(c["name"], []):
            assert lo - 1e-5 <= pnt[i][a] <= hi + 1e-5, (c["name"], pnt[i])
    # rot = None is the identity, half_extent (3,) is every query's
    plain = [i for i, c in enumerate(casts) if c["rot"] == cases.IDENT and c["he"] == [0.5, 0.5, 0.5]]
    assert len(plain) >= 4
    again = w.boxcast(o[plain], d[plain], [0.5, 0.5, 0.5])
    for x, y in zip(again, (body, t, nrm, pnt)):
        assert np.array_equal(_bits(x), _bits(y[plain]))
    # invalid half extents, rot, dir and max_t all miss; zero components are valid
    n = 12
    o2, d2 = np.tile(o[0], (n, 1)), np.tile(d[0], (n, 1))
    rot2 = np.tile(np.array(cases.IDENT, np.float32), (n, 1))
    he2, mt2 = np.full((n, 3), 0.5, np.float32), np.full(n, 9.0, np.float32)
    he2[0, 0], he2[1, 1], he2[2, 2], he2[3, 1], he2[4, 0] = -1, np.nan, np.inf, -np.inf, -1e-30
    rot2[5, 2] = np.nan
    rot2[6, 0] = np.inf
    d2[7] = 0
    d2[8, 1] = np.inf
    d2[9, 0] = np.nan
    mt2[10] = -1
    he2[11] = 0  # a point: valid
    body, t, nrm, pnt = w.boxcast(o2, d2, he2, rot=rot2, max_t=mt2)
    assert list(body[:11]) == [pa.RAY_MISS] * 11 and np.isinf(t[:11]).all() and not nrm[:11].any() and not pnt[:11].any()
    assert body[11] == 0 and abs(t[11] - 5.0) <= 1e-5
    with pytest.raises(ValueError):
        w.boxcast(o2, d2, he2[:5])
    with pytest.raises(ValueError):
        w.boxcast(o2, d2[:5], he2)
    w.close()


# ---- 2. random soups against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.SOUP_SEEDS)
def test_random_soups(seed):
    pa = _pa()
    c = cases.soup(seed)
    body = _run(c)[0]
    nb = len(c["bodies"]["pos"])
    assert (body < nb).sum() > 100 and ((body & pa.STATIC_ID_BIT != 0) & (body < pa.RAY_MISS)).sum() > 0
    assert (body == pa.RAY_GROUND).sum() > 0


# ---- 3. degenerate orientations and sizes, one call each ------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.DEGENERATE)
def test_degenerate_sets(name):
    c = cases.degenerate(name)
    w = _world(c["bodies"], c["statics"], c["ground"])
    body, t, _, _ = _run(c, w)
    assert (body < len(c["bodies"]["pos"])).sum() > 30
    if name == "point":
        # a box of no extent is a ray: phys_raycast's t within the tolerance
        rb, rt, _ = w.raycast(c["o"], c["d"])
        both = np.isfinite(t) & np.isfinite(rt)
        # (a ray that grazes a target may be a hit to one and a miss to the other: within the cap of odd cases)
        assert both.sum() > 30 and (np.isfinite(t) != np.isfinite(rt)).sum() <= cast_cap(len(t))
        for i in np.nonzero(both)[0]:
            assert abs(float(t[i]) - float(rt[i])) <= tol_of(c["h"], i), (i, t[i], rt[i])
    w.close()


# ---- 4. the grid's edges ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_world():
    import query_scenes as qs
    made = {}

    def get(name):
        if name not in made:
            sc = qs.scene(name)
            made[name] = _world(sc["bodies"], sc["statics"], sc["ground"])
        return made[name]

    yield get
    for w in made.values():
        w.close()


@pytest.mark.parametrize("kind", ["mixed", "huge"])
@pytest.mark.parametrize("name", cases.GRID_SCENES)
def test_grid_edges(name, kind, grid_world):
    c = cases.grid_case(name, kind)
    body = _run(c, grid_world(name))[0]
    assert (body < len(c["bodies"]["pos"])).sum() > len(body) // 2
    bad = ~c["h"]["valid"]
    assert bad.sum() >= 6 and (body[bad] == _pa().RAY_MISS).all()


# ---- 5. ignore and max_t ------------------------------------------------------------------------------------------------------------
def test_ignore_and_max_t():
    c = cases.rules_case()
    body, t, _, _ = _run(c)
    ig = c["ignore"]
    given = ig != 0xFFFFFFFF
    assert given.sum() > 50 and (body[given] != ig[given]).all()
    assert (t[np.isfinite(t)] <= c["max_t"][np.isfinite(t)]).all() and (np.isfinite(c["max_t"]) & ~np.isfinite(t)).sum() > 10


# ---- 6. the filtered instance -------------------------------------------------------------------------------------------------------
def test_filtered_casts_match_the_filtered_reference():
    import torch
    pa = _pa()
    base = cases.soup(2)
    cat, scat, masks, per = cases.filter_case()
    w = _world(base["bodies"], base["statics"], base["ground"])
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(cases.GROUND_CATEGORY, 0xFFFF)
    n = len(masks)
    o, d, rot, he = (np.ascontiguousarray(base[k][:n]) for k in ("o", "d", "rot", "he"))
    got = w.boxcast(o, d, he, rot=rot, mask=masks)
    nb = len(cat)
    for mask, (k, c) in per.items():
        body = _run(c, w, out=tuple(x[k] for x in got))[0]
        # what a mask rejects is never reported
        assert ((cat[body[body < nb]] & mask) != 0).all()
        st = body[(body >= pa.STATIC_ID_BIT) & (body < pa.RAY_MISS)] - pa.STATIC_ID_BIT
        assert ((scat[st] & mask) != 0).all()
        assert mask & cases.GROUND_CATEGORY or not (body == pa.RAY_GROUND).any()
    # a mask of all ones is the plain call; mask 0 sees nothing; the device variant of the filtered call equals the host's
    plain = w.boxcast(o, d, he, rot=rot)
    for x, y in zip(plain, w.boxcast(o, d, he, rot=rot, mask=0xFFFF)):
        assert np.array_equal(_bits(x), _bits(y))
    assert (w.boxcast(o, d, he, rot=rot, mask=0)[0] == pa.RAY_MISS).all()
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()  # (a copy: the cases' arrays are read-only)
    tb = torch.empty(n, dtype=torch.int32, device="cuda")
    tt = torch.empty(n, dtype=torch.float32, device="cuda")
    tn, tp = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    w.boxcast_device(dev(o), dev(d), dev(he), tb, tt, tn, tp, rot=dev(rot), mask=dev(masks.view(np.int16)))
    w.sync()
    for x, y in zip(got, (tb, tt, tn, tp)):
        assert np.array_equal(_bits(x), _bits(y.cpu().numpy()))
    w.close()


# ---- 7. host and device variants, batching, NULL outputs, current poses, ghosts ---------------------------------------------------
def test_device_variant_batching_and_null_outputs():
    import torch
    from physics_amd import _abi
    c = cases.soup(1)
    w = _world(c["bodies"], c["statics"], c["ground"])
    n = 240
    o, d, rot, he = (np.ascontiguousarray(c[k][:n]) for k in ("o", "d", "rot", "he"))
    a = w.boxcast(o, d, he, rot=rot)
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()
    tb = torch.empty(n, dtype=torch.int32, device="cuda")
    tt = torch.empty(n, dtype=torch.float32, device="cuda")
    tn, tp = (torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    w.boxcast_device(dev(o), dev(d), dev(he), tb, tt, tn, tp, rot=dev(rot))
    w.sync()
    for x, y in zip(a, (tb, tt, tn, tp)):
        assert np.array_equal(_bits(x), _bits(y.cpu().numpy()))
    # normal_out and point_out NULL: the others as before
    tb2, tt2 = torch.empty_like(tb), torch.empty_like(tt)
    w.boxcast_device(dev(o), dev(d), dev(he), tb2, tt2, rot=dev(rot))
    w.sync()
    assert torch.equal(tb, tb2) and torch.equal(tt, tt2)
    p = lambda x, t=_abi.f32p: x.ctypes.data_as(t)
    hb, ht = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    assert w.lib.phys_boxcast(w.h, n, p(o), p(d), p(rot), p(he), None, None, p(hb, _abi.u32p), p(ht), None, None) == 0
    assert np.array_equal(hb, a[0]) and np.array_equal(_bits(ht), _bits(a[1]))
    # the argument checks of the entry points, and n == 0
    assert w.lib.phys_boxcast(w.h, n, p(o), p(d), p(rot), None, None, None, p(hb, _abi.u32p), p(ht), None, None) != 0
    assert "phys_boxcast: null origin, dir, half_extent, body_out or t_out" in w.lib.phys_last_error().decode()
    assert w.lib.phys_boxcast_device(w.h, 1 << 31, None, None, None, None, None, None, None, None, None, None) != 0
    assert "phys_boxcast: n must be below 2^31" in w.lib.phys_last_error().decode()
    assert w.lib.phys_boxcast(w.h, 0, None, None, None, None, None, None, None, None, None, None) == 0
    # the same answers in reverse order and one at a time
    r = w.boxcast(o[::-1], d[::-1], he[::-1], rot=rot[::-1])
    for x, y in zip(a, r):
        assert np.array_equal(_bits(x), _bits(y[::-1]))
    for i in range(0, n, 10):
        one = w.boxcast(o[i:i + 1], d[i:i + 1], he[i:i + 1], rot=rot[i:i + 1])
        for x, y in zip(a, one):
            assert np.array_equal(_bits(x[i:i + 1]), _bits(y))
    w.close()


def test_current_poses_after_an_update():
    pa = _pa()
    c = cases.soup(2)
    w = _world(c["bodies"], None, 0.0)
    w.update_n(1_000_000_000 // 60, 3)
    w.sync()
    pos, rot = w.get_transforms()
    assert not np.array_equal(pos, c["bodies"]["pos"])
    tg = query_ref.targets(dict(pos=pos, rot=rot, half_extent=c["bodies"]["half_extent"], shape=c["bodies"]["shape"]))
    k = slice(0, 40)
    h = ref.boxcast(c["o"][k], c["d"][k], c["rot"][k], c["he"][k], tg, ground=0.0)
    compare_boxcasts(h, w.boxcast(c["o"][k], c["d"][k], c["he"][k], rot=c["rot"][k]), label="after updates")
    # and at once after set_bodies
    b = {x: np.array(v) for x, v in c["bodies"].items()}
    b["pos"][0] = [500, 500, 500]
    b["shape"][0] = pa.SHAPE_BOX
    w.set_bodies(b["pos"], rot=b["rot"], shape_type=b["shape"], half_extent=b["half_extent"])
    body, t, _, _ = w.boxcast([[500, 500, 480]], [[0, 0, 1]], [0.5, 0.5, 0.5])
    assert body[0] == 0 and 15 < t[0] < 20
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
    right, _ = make([1.5, 20.0], 0.0, 1.0e6, 100)
    buf = torch.full((cap * 96,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    left.halo_pack_bodies(buf.data_ptr(), cap)
    left.sync()
    right.halo_unpack_ghosts(buf.data_ptr(), cap, 0, 0)
    right.sync()
    assert right.get_stats().n_ghosts == len(zs)
    ghost_pos = lpos[:len(zs)]
    body, t, _, pnt = right.boxcast(ghost_pos + [0, 10, 0], np.tile([0.0, -1.0, 0.0], (len(zs), 1)), [0.25, 0.5, 0.25])
    assert list(body) == [pa.RAY_GROUND] * len(zs), body
    assert np.allclose(t, 15 - 0.5) and np.allclose(pnt, ghost_pos * [1, 0, 1])
    left.close()
    right.close()


# ---- 8. no side effects ---------------------------------------------------------------------------------------------------------------
def _snapshot(w):
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    st = w.get_stats()
    return [pos, rot, lin, ang], {k: getattr(st, k) for k, _ in type(st)._fields_}, w.get_manifolds()


@pytest.mark.parametrize("name", ["c2", "cluster_tower"])
def test_box_casts_leave_updates_bit_identical(name):
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
    n = 2000
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rot = cases.quats(rng, n)
    he = rng.uniform(0.1, 0.8, (n, 3)).astype(np.float32)
    to, td, tq, th = (torch.from_numpy(x).cuda() for x in (o, d, rot, he))
    tb = torch.empty(n, dtype=torch.int32, device="cuda")
    tt = torch.empty(n, dtype=torch.float32, device="cuda")
    tp = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    found = 0
    for k in range(12):
        for w in worlds:
            w.update_n(scenes.DT_NANOS, 2)
        body = probed.boxcast(o, d, he, rot=rot)[0]
        probed.boxcast_device(to, td, th, tb, tt, point_out=tp, rot=tq)
        found += int((body < probed.n).sum())
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
