"""GPU: collision filters (category, mask, group; include/physics_hip.h) on bodies, statics, the
ground, ghosts and the three query kinds.

The oracle has no filters. What stands in for it: the bits of unfiltered runs (default filters change no bit; a
filtered update's manifolds are exactly the unfiltered ones minus the pairs the numpy rule of physics_amd.filters
rejects), tests/contact_ref.py (the float64 solver fed the filtered manifolds) and tests/query_ref.py (float64 queries
over the target list filtered in numpy)."""
import ctypes as C

import numpy as np
import pytest

import contact_ref as cr
import query_ref as ref
import test_gpu_query as gq

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
ALL = 0xFFFF


def _pa():
    import physics_amd
    return physics_amd


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _soup(seed, n=400):
    """Spheres, boxes, capsules and a few NONE bodies packed closely above the ground, beside three statics."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-5.0, 5.0, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.3, 6.0, n)
    shape = rng.choice([1, 2, 3, 0], n, p=[0.3, 0.35, 0.3, 0.05]).astype(np.uint32)
    he = rng.uniform(0.3, 0.7, (n, 3)).astype(np.float32)
    bodies = dict(pos=pos, rot=_quats(rng, n), shape_type=shape, half_extent=he)
    statics = (np.array([[2.0, 1.0, 2.0], [-3.0, 1.5, -2.0], [0.0, 2.0, -4.0]], np.float32),
               np.concatenate([np.array([[0, 0, 0, 1]], np.float32), _quats(rng, 2)]),
               np.array([2, 1, 3], np.uint32), np.array([[1.5, 0.5, 1.5], [1.0, 0, 0], [0.5, 1.5, 0]], np.float32))
    return bodies, statics


def _world(bodies, statics=None, flags=0, ground=True, **cfg):
    pa = _pa()
    f = pa.FLAG_COLLISIONS | (pa.FLAG_GROUND_PLANE if ground else 0) | flags
    w = pa.World(pa.default_config(flags=f, gravity_offset=(0.0, 0.0, 0.0), **cfg))
    w.set_bodies(**bodies)
    if statics is not None:
        w.set_static_bodies(statics[0], rot=statics[1], shape_type=statics[2], half_extent=statics[3])
    return w


def _random_filters(rng, n, cats=(1, 2, 4, 8), groups=(0, 0, 0, 0, 1, -1, 2, -2)):
    cat = rng.choice(cats, n).astype(np.uint16)
    mask = (rng.integers(0, 16, n) | rng.choice([0, 0xFFF0], n)).astype(np.uint16)
    grp = rng.choice(groups, n).astype(np.int16)
    return cat, mask, grp


def _state(w):
    return list(w.get_transforms()) + list(w.get_velocities())


def _same_manifolds(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---- 1. default filters change no bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["default", "per_color", "cluster"])
def test_default_filters_set_explicitly_change_no_bit(solver):
    """Setting the default filters on bodies, statics and ground makes the world run the filtered narrow phase; its
    transforms, velocities and manifolds must equal those of a world that never set a filter, over 200 updates."""
    pa = _pa()
    if solver == "cluster":
        from physics_amd import scenes
        sc = scenes.c5(16, 130, 16)  # enough resting contacts for the cluster solver
        n = len(sc.pos)
        shape = sc.shape_type.copy()
        shape[::7] = pa.SHAPE_CAPSULE
        he = sc.half_extent.copy()
        he[::7] = [0.9, 0.1, 0.0]  # as tall as the cubes
        bodies = dict(pos=sc.pos, shape_type=shape, half_extent=he)
        statics = (np.array([[30.0, 1.0, 8.0], [-4.0, 0.5, 8.0]], np.float32), None, np.array([2, 3], np.uint32),
                   np.array([[1.0, 1.0, 1.0], [0.5, 1.0, 0.0]], np.float32))
        flags, chunk = pa.FLAG_SOLVER_CLUSTER, 50
    else:
        bodies, statics = _soup(11)
        n = len(bodies["pos"])
        flags, chunk = (0 if solver == "default" else pa.FLAG_SOLVER_PER_COLOR), 25
    plain = _world(bodies, statics, flags, gravity_force=(0.0, -9.81, 0.0))
    filt = _world(bodies, statics, flags, gravity_force=(0.0, -9.81, 0.0))
    filt.set_body_filters(np.full(n, 1), np.full(n, ALL), np.zeros(n, np.int16))
    filt.set_static_filters()
    filt.set_ground_filter(pa.FILTER_DEFAULT_CATEGORY, pa.FILTER_DEFAULT_MASK)
    if solver == "cluster":
        for w in (plain, filt):
            w.profile_enable(True)
    manifolds = 0
    for done in range(chunk, 201, chunk):
        for w in (plain, filt):
            w.update_n(DT, chunk)
            w.sync()
        for a, b in zip(_state(plain), _state(filt)):
            assert np.array_equal(a, b), f"{solver}: update {done} differs"
        ma, mb = plain.get_manifolds(), filt.get_manifolds()
        assert _same_manifolds(ma, mb), f"{solver}: manifolds of update {done} differ"
        manifolds = max(manifolds, len(ma[0]))
    assert manifolds > 100
    if solver == "cluster":
        assert "solve_cluster" in filt.profile_get()[0]
    plain.close()
    filt.close()


# ---- 2. exactly the rejected manifolds vanish --------------------------------------------------------------------------
def _expected_keep(ids, bc, bm, bg, sc, sm, sg, ground):
    pa = _pa()
    fl = pa.filters
    a, b = ids[:, 0].astype(np.int64), ids[:, 1].astype(np.int64)
    keep = np.zeros(len(ids), bool)
    gnd = b == pa.GROUND_ID
    st = ~gnd & (b >= pa.STATIC_ID_BIT)
    bb = ~gnd & ~st
    keep[bb] = fl.collide(bc[a[bb]], bm[a[bb]], bg[a[bb]], bc[b[bb]], bm[b[bb]], bg[b[bb]])
    k = b[st] - pa.STATIC_ID_BIT
    keep[st] = fl.collide(bc[a[st]], bm[a[st]], bg[a[st]], sc[k], sm[k], sg[k])
    keep[gnd] = fl.collide(bc[a[gnd]], bm[a[gnd]], bg[a[gnd]], ground[0], ground[1], 0)
    return keep


@pytest.mark.parametrize("seed", [3, 4])
def test_filtered_update_drops_exactly_the_rejected_manifolds(seed):
    rng = np.random.default_rng(seed)
    bodies, statics = _soup(seed)
    n, ns = len(bodies["pos"]), len(statics[0])
    bc, bm, bg = _random_filters(rng, n)
    # the big platform (static 0) collides with the bodies whose mask has bit 0, the ball with nobody but group 1
    sc, sm, sg = np.array([1, 2, 4], np.uint16), np.array([ALL, 0, ALL], np.uint16), np.array([0, 1, 0], np.int16)
    ground = (1, 0xFFFB)  # category 4 bodies miss the ground
    plain = _world(bodies, statics)
    filt = _world(bodies, statics)
    filt.set_body_filters(bc, bm, bg)
    filt.set_static_filters(sc, sm, sg)
    filt.set_ground_filter(*ground)
    assert all(np.array_equal(x, y) for x, y in zip(filt.get_body_filters(), (bc, bm, bg)))
    for w in (plain, filt):
        w.update(DT)
        w.sync()
    ids, counts, normals, points = plain.get_manifolds()
    keep = _expected_keep(ids, bc, bm, bg, sc, sm, sg, ground)
    kinds = [ids[:, 1] < _pa().STATIC_ID_BIT, (ids[:, 1] >= _pa().STATIC_ID_BIT) & (ids[:, 1] != _pa().GROUND_ID),
             ids[:, 1] == _pa().GROUND_ID]
    for kind in kinds:  # every kind of work item has manifolds kept and manifolds dropped
        assert (kind & keep).any() and (kind & ~keep).any()
    want = (ids[keep], counts[keep], normals[keep], points[keep])
    got = filt.get_manifolds()
    assert _same_manifolds(want, got), f"{len(got[0])} manifolds, {int(keep.sum())} expected of {len(ids)}"
    assert filt.get_stats().n_pairs == plain.get_stats().n_pairs  # the pair search does not look at filters
    assert filt.get_static_stats()[1] == plain.get_static_stats()[1]
    plain.close()
    filt.close()


# ---- 3. the solve on the filtered list matches float64 -----------------------------------------------------------------
def test_filtered_heap_solve_matches_the_float64_reference():
    pa = _pa()
    bodies = cr.random_heap(5)
    n = len(bodies["pos"])
    # half the heap is debris that ignores itself, one column group never collides within itself
    cat = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint16)
    mask = np.where(cat == 2, 0xFFFD, 0xFFFF).astype(np.uint16)
    grp = np.where(np.arange(n) % 10 == 3, -5, 0).astype(np.int16)
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_force=(0, -9.81, 0),
                                   gravity_offset=(0, 0, 0)))
    w.set_bodies(**bodies)
    w.set_body_filters(cat, mask, grp)
    sref = cr.SolverRef(n, cr.Params(DT_S), 8)
    inv_m, inv_I = cr.body_inverses(n, bodies.get("mass"), bodies.get("inertia"))
    worst = 0.0
    for _ in range(4):
        pos, _ = w.get_transforms()
        lin, ang = w.get_velocities()
        w.update(DT)
        w.sync()
        man = w.get_manifolds()
        ids = man[0].astype(np.int64)
        bb = ids[:, 1] < n
        assert pa.filters.collide(cat[ids[bb, 0]], mask[ids[bb, 0]], grp[ids[bb, 0]],
                                  cat[ids[bb, 1]], mask[ids[bb, 1]], grp[ids[bb, 1]]).all()
        out = sref.update(man, pos, lin, ang, inv_m, inv_I, np.array([0.0, -9.81, 0.0]))
        lin1, ang1 = w.get_velocities()
        err, amb = cr.velocity_error(out, lin1, ang1)
        assert amb <= 0.01 * len(out["a"])
        worst = max(worst, err)
    assert len(man[0]) > 200
    assert worst < 2e-5, worst  # TOL_COUPLED of tests/test_gpu_solver_independent.py
    w.close()


# ---- 4. behaviour ------------------------------------------------------------------------------------------------------
def _cubes(pos):
    n = len(pos)
    return dict(pos=np.asarray(pos, np.float32), shape_type=np.full(n, 2, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))


def _columns(y0, cols=3, height=3):
    return [[3.0 * i, y0 + 1.05 * k, 3.0 * j] for i in range(cols) for j in range(cols) for k in range(height)]


def test_interleaved_lattices_pass_through_each_other():
    A, B = _columns(0.6), _columns(1.1)  # B's cubes half inside A's
    nA = len(A)
    g = dict(gravity_force=(0.0, -9.81, 0.0))
    w = _world(_cubes(A + B), **g)
    # A in layer 2, B in layer 4, each blind to the other; both still see the ground's layer 1
    w.set_body_filters(category=[2] * nA + [4] * nA, mask=[0xFFFB] * nA + [0xFFFD] * nA)
    for _ in range(300):
        w.update(DT)
        ids = w.get_manifolds()[0]
        assert not ((ids[:, 0] < nA) & (ids[:, 1] >= nA) & (ids[:, 1] < 2 * nA)).any(), "an A-B manifold"
    y = w.get_transforms()[0][:, 1]
    for part, start in ((A, 0), (B, nA)):
        alone = _world(_cubes(part), **g)
        alone.update_n(DT, 300)
        alone.sync()
        ya = alone.get_transforms()[0][:, 1]
        assert np.abs(y[start:start + nA] - ya).max() < 0.01, (y[start:start + nA], ya)
        assert np.abs(ya - np.tile(0.5 + np.arange(3), 9)).max() < 0.05  # stacks of three resting on the ground
        alone.close()
    w.close()


def test_negative_group_chain_of_capsules():
    pa = _pa()
    n = 8
    q = [0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4)]  # local y along x
    bodies = dict(pos=np.array([[1.5 * i, 0.6, 0.0] for i in range(n)], np.float32), rot=np.tile(np.float32(q), (n, 1)),
                  shape_type=np.full(n, pa.SHAPE_CAPSULE, np.uint32), half_extent=np.tile(np.float32([0.5, 0.5, 0.0]), (n, 1)))
    for grouped in (False, True):
        w = _world(bodies, gravity_force=(0.0, -9.81, 0.0))
        if grouped:
            w.set_body_filters(group=np.full(n, -1))
        chain = ground = 0
        for _ in range(60):
            w.update(DT)
            ids = w.get_manifolds()[0]
            chain += int((ids[:, 1] < n).sum())
            ground += int((ids[:, 1] == pa.GROUND_ID).sum())
        assert ground > 0
        assert (chain == 0) == grouped, (grouped, chain)
        w.close()


def test_same_positive_group_overrides_masks():
    pa = _pa()
    for group in (0, 3):
        w = _world(_cubes([[0.0, 0.5, 0.0], [0.0, 1.6, 0.0]]), gravity_force=(0.0, -9.81, 0.0))
        w.set_body_filters(category=[2, 4], mask=[1, 1], group=[group, group])  # both see only the ground's layer
        w.update_n(DT, 120)
        w.sync()
        y = w.get_transforms()[0][:, 1]
        if group:
            assert abs(y[1] - 1.5) < 0.05 and abs(y[0] - 0.5) < 0.05, y
        else:
            assert abs(y[1] - 0.5) < 0.05, y  # fell through the lower cube onto the ground
        w.close()


def test_ground_mask_lets_one_category_fall_through():
    w = _world(_cubes([[0.0, 1.0, 0.0], [3.0, 1.0, 0.0]]), gravity_force=(0.0, -9.81, 0.0))
    w.set_body_filters(category=[1, 2])
    w.set_ground_filter(1, 0xFFFD)
    w.update_n(DT, 120)
    w.sync()
    y = w.get_transforms()[0][:, 1]
    assert abs(y[0] - 0.5) < 0.05 and y[1] < -5.0, y
    w.close()


def test_static_floor_mask_lets_one_category_drop_to_the_ground():
    floor = (np.array([[0.0, 3.0, 0.0]], np.float32), None, np.array([2], np.uint32), np.array([[10.0, 0.25, 10.0]], np.float32))
    w = _world(_cubes([[0.0, 4.5, 0.0], [3.0, 4.5, 0.0]]), floor, gravity_force=(0.0, -9.81, 0.0))
    w.set_body_filters(category=[1, 2])
    w.set_static_filters(mask=[0xFFFD])
    w.update_n(DT, 150)
    w.sync()
    y = w.get_transforms()[0][:, 1]
    assert abs(y[0] - 3.75) < 0.05 and abs(y[1] - 0.5) < 0.05, y
    w.close()


# ---- 5. changes, resets, determinism -----------------------------------------------------------------------------------
def _pair_ids(w):
    return {tuple(int(x) for x in r) for r in w.get_manifolds()[0]}


def test_filter_changes_take_effect_at_the_next_update_and_resets():
    pa = _pa()
    w = _world(_cubes([[0.0, 0.5, 0.0], [1.0, 0.5, 0.0]]))  # side by side on the ground, touching
    w.update(DT)
    assert (0, 1) in _pair_ids(w) and (1, pa.GROUND_ID) in _pair_ids(w)
    w.set_body_filters(category=[2, 4], mask=[0xFFFB, 0xFFFD])
    w.update(DT)
    assert (0, 1) not in _pair_ids(w) and (1, pa.GROUND_ID) in _pair_ids(w)
    w.set_body_filters()  # all defaults again: the pair comes back
    w.update(DT)
    assert (0, 1) in _pair_ids(w)
    w.set_ground_filter(1, 0xFFFD)
    w.set_body_filters(category=[1, 2])
    w.update(DT)
    assert (1, pa.GROUND_ID) not in _pair_ids(w) and (0, pa.GROUND_ID) in _pair_ids(w)
    # phys_set_bodies resets the body filters (the ground's stays)
    w.set_body_filters(category=[1, 2], mask=[0xFFFD, 0xFFFE], group=[-1, 7])
    w.set_bodies(**_cubes([[0.0, 0.5, 0.0], [1.0, 0.5, 0.0]]))
    c, m, g = w.get_body_filters()
    assert list(c) == [1, 1] and list(m) == [ALL, ALL] and list(g) == [0, 0]
    w.update(DT)
    assert {(0, 1), (0, pa.GROUND_ID), (1, pa.GROUND_ID)} <= _pair_ids(w)
    w.close()
    # phys_set_static_bodies resets the static filters
    floor = (np.array([[0.0, 0.0, 0.0]], np.float32), None, np.array([2], np.uint32), np.array([[5.0, 0.25, 5.0]], np.float32))
    w = _world(_cubes([[0.0, 0.75, 0.0]]), floor, ground=False)
    w.set_static_filters(mask=[0])
    w.update(DT)
    assert not _pair_ids(w)
    w.set_static_bodies(floor[0], shape_type=floor[2], half_extent=floor[3])
    w.update(DT)
    assert _pair_ids(w) == {(0, pa.STATIC_ID_BIT)}
    w.close()


def test_filtered_runs_repeat_bit_for_bit():
    rng = np.random.default_rng(8)
    bodies, statics = _soup(8)
    n = len(bodies["pos"])
    f = _random_filters(rng, n)
    runs = []
    for _ in range(2):
        w = _world(bodies, statics, gravity_force=(0.0, -9.81, 0.0))
        w.set_body_filters(*f)
        w.set_static_filters(category=[1, 2, 4], mask=[ALL, 0xFFFE, 0xFFF0])
        w.update_n(DT, 100)
        w.sync()
        runs.append(_state(w) + list(w.get_manifolds()))
        w.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 6. sharded worlds -------------------------------------------------------------------------------------------------
REC = 96


def _two_ranks(filters=None):
    pa = _pa()
    import torch
    ws = []
    for r, x in enumerate((-0.45, 0.45)):
        w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS, gravity_force=(0.0, 0.0, 0.0), gravity_offset=(0, 0, 0),
                                       max_ghosts=16))
        w.set_bodies(**_cubes([[x, 5.0, 0.0]]))
        w.set_global_ids(np.array([r], np.uint32))
        w.set_slab(-1.0e6 if r == 0 else 0.0, 0.0 if r == 0 else 1.0e6, 4.0)
        if filters is not None:
            w.set_body_filters(*filters[r])
        ws.append(w)
    bufs = [torch.empty(8 * REC, dtype=torch.uint8, device="cuda") for _ in ws]
    for w, b in zip(ws, bufs):
        w.halo_pack_bodies(b.data_ptr(), 8)
    for w in ws:
        w.sync()
    gathered = torch.cat(bufs)
    torch.cuda.synchronize()
    for r, w in enumerate(ws):
        w.halo_unpack_ghosts(gathered.data_ptr(), 16, r * 8, 8)
        w.update(DT)
    for w in ws:
        w.sync()
    words = [b.cpu().numpy().view(np.uint32).reshape(8, 24) for b in bufs]
    return ws, words


def test_ghost_filters_cross_the_cut():
    ws, _ = _two_ranks()
    assert all((0, 1) in _pair_ids(w) for w in ws), "control: the overlapping cubes touch across the cut"
    for w in ws:
        w.close()
    filt = [([1], [0xFFFD], [0]), ([2], [0xFFFE], [0])]
    ws, words = _two_ranks(filt)
    for w in ws:
        assert w.get_stats().n_ghosts == 1
        assert not _pair_ids(w), "a manifold between bodies whose masks exclude each other"
    rec = words[0][0]  # rank 0's record carries its filter
    c, m, g, full = _pa().filters.halo_decode(rec[19], rec[23])
    assert (int(c), int(m), int(g), bool(full)) == (1, 0xFFFD, 0, False)
    for w in ws:
        w.close()


def test_default_filter_records_keep_their_bits():
    ws, words = _two_ranks()
    for blk in words:
        valid = blk[:, 17] != 0xFFFFFFFF
        assert valid.sum() == 1
        assert (blk[valid, 23] == 0).all() and np.isin(blk[valid, 19], [0, 1]).all()
    for w in ws:
        w.close()


# ---- 7. queries --------------------------------------------------------------------------------------------------------
def _query_world(seed):
    pa = _pa()
    rng = np.random.default_rng(seed)
    pos, rot, shape, he = gq._soup(rng, 300, 12.0)
    statics = gq._statics(rng)
    w = gq._world(pos, shape, he, rot=rot)
    w.set_static_bodies(statics[0], rot=statics[1], shape_type=statics[2], half_extent=statics[3])
    cat = rng.choice([1, 2, 4], len(pos)).astype(np.uint16)
    scat = np.array([1, 2, 4, 2], np.uint16)
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(2, ALL)
    tg = gq._targets(w, shape, he, statics)
    return w, rng, tg, cat, scat


def _category_of(ids, cat, scat):
    """Category of each reported id (the ground's is 2; a miss gets 0)."""
    pa = _pa()
    ids = np.asarray(ids, np.int64)
    out = np.zeros(len(ids), np.int64)
    body = ids < len(cat)
    st = (ids >= pa.STATIC_ID_BIT) & (ids < pa.RAY_MISS)
    out[body] = cat[ids[body]]
    out[st] = scat[ids[st] - pa.STATIC_ID_BIT]
    out[ids == pa.RAY_GROUND] = 2
    return out


def _only(tg, cat, scat, mask):
    keep = (_category_of(tg["id"], cat, scat) & mask) != 0
    return {k: v[keep] for k, v in tg.items()}


def _check_casts(w, tg, cat, scat, o, d, rad, mask, ignore=None, label=""):
    """Filtering only removes targets: where the unfiltered cast's answer passes the mask, the filtered cast gives the same
    bits; everywhere else the filtered answer is checked against the float64 reference over the filtered targets."""
    ray = rad is None
    plain = w.raycast(o, d, ignore=ignore) if ray else w.spherecast(o, d, rad, ignore=ignore)
    got = w.raycast(o, d, ignore=ignore, mask=mask) if ray else w.spherecast(o, d, rad, ignore=ignore, mask=mask)
    same = (_category_of(plain[0], cat, scat) & mask) != 0
    for a, b in zip(plain, got):
        assert np.array_equal(a[same].view(np.uint32), b[same].view(np.uint32)), label
    other = ~same
    assert other.sum() > 50, label
    sub = _only(tg, cat, scat, mask)
    gnd = 0.0 if mask & 2 else None
    r = 0.0 if ray else np.broadcast_to(np.asarray(rad, np.float32), (len(o),))[other]
    ig = None if ignore is None else ignore[other]
    if ray:
        # rays against the float64 ball of radius 0: the same target and t within 1e-4 relative (that reference is not the
        # ray casts' own, whose exact arithmetic tests/test_gpu_raycast.py checks), another target only at a near tie
        h = ref.spherecast(o[other], d[other], 0.0, sub, ignore=ig, ground=gnd)
        gb, gt = got[0][other].astype(np.int64), got[1][other].astype(np.float64)
        fin = np.isfinite(h["t"])
        same_id = gb == h["body"]
        close = np.where(fin, np.abs(gt - h["t"]) <= 1e-4 * (1.0 + np.abs(h["o"]).max(1) + np.where(fin, h["t"], 0.0)), np.isinf(gt))
        tie = np.isfinite(h["t2"]) & (np.abs(h["t2"] - h["t"]) <= 1e-3 * (1.0 + h["t"]))
        odd = ~(same_id & close) & ~tie
        assert odd.sum() <= max(3, len(gb) // 200), (label, np.nonzero(odd)[0][:8], gb[odd][:8], h["body"][odd][:8])
        return
    gq.compare_casts(w, sub, o[other], d[other], r, ground=gnd, ignore=ig, out=(got[0][other], got[1][other], got[2][other]),
                     label=label)


@pytest.mark.parametrize("mask", [1, 2, 5, 6])
def test_filtered_casts_match_the_float64_reference(mask):
    w, rng, tg, cat, scat = _query_world(24)
    o, d = gq._casts(rng, 2000, 12.0)
    _check_casts(w, tg, cat, scat, o, d, None, mask, label=f"rays {mask}")
    rad = rng.uniform(0.0, 1.0, len(o)).astype(np.float32)
    _check_casts(w, tg, cat, scat, o, d, rad, mask, label=f"balls {mask}")
    ign = rng.integers(0, 300, len(o)).astype(np.uint32)  # ignore_body composes with the mask
    _check_casts(w, tg, cat, scat, o, d, rad, mask, ignore=ign, label=f"balls {mask} ignore")
    w.close()


@pytest.mark.parametrize("mask", [1, 6])
def test_filtered_overlaps_match_the_float64_reference(mask):
    w, rng, tg, cat, scat = _query_world(22)
    n = 400
    st = rng.choice([1, 2, 3], n).astype(np.uint32)
    pos = rng.uniform(-12.0, 12.0, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.0, 10.0, n)
    rot = _quats(rng, n)
    he = rng.uniform(0.3, 2.0, (n, 3)).astype(np.float32)
    ign = rng.integers(0, 300, n).astype(np.uint32)
    off, ids = w.overlap(st, pos, rot, he, ignore=ign, mask=mask)
    want = ref.overlap(st, pos, rot, he, _only(tg, cat, scat, mask), ignore=ign, ground=0.0 if mask & 2 else None)
    near, total = 0, 0
    for i in range(n):
        got = [int(x) for x in ids[off[i]:off[i + 1]]]
        assert got == sorted(set(got)), (i, got)
        exp, close = want[i]
        total += len(exp)
        for k in set(got) ^ set(exp):
            assert k in close and abs(close[k]) <= 1e-4, (i, k, got, exp)
            near += 1
    assert total > 200 and near <= max(2, n // 200)
    w.close()


def test_null_and_zero_masks_and_device_variants():
    import torch
    pa = _pa()
    w, rng, tg, cat, scat = _query_world(23)
    o, d = gq._casts(rng, 1000, 12.0)
    rad = rng.uniform(0.0, 1.0, len(o)).astype(np.float32)
    lib, n = w.lib, len(o)
    # query_mask NULL: the plain call's bits
    b0, t0, n0 = w.raycast(o, d)
    b1, t1, n1 = np.empty(n, np.uint32), np.empty(n, np.float32), np.empty((n, 3), np.float32)
    p = lambda a, t=C.c_float: a.ctypes.data_as(C.POINTER(t))
    assert lib.phys_raycast_filtered(w.h, n, p(o), p(d), None, None, None, p(b1, C.c_uint32), p(t1), p(n1)) == 0
    assert np.array_equal(b0, b1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(n0, n1)
    s0 = w.spherecast(o, d, rad)
    assert lib.phys_spherecast_filtered(w.h, n, p(o), p(d), p(rad), None, None, None, p(b1, C.c_uint32), p(t1), p(n1)) == 0
    assert np.array_equal(s0[0], b1) and np.array_equal(s0[1], t1) and np.array_equal(s0[2], n1)
    qs = np.full(64, pa.SHAPE_SPHERE, np.uint32)
    qp = o[:64].copy()
    qh = np.tile(np.float32([3.0, 0, 0]), (64, 1))
    off0, ids0 = w.overlap(qs, qp, half_extent=qh)
    off1, ids1 = np.zeros(65, np.uint64), np.empty(len(ids0) + 1, np.uint32)
    assert lib.phys_overlap_filtered(w.h, 64, p(qs, C.c_uint32), p(qp), None, p(qh), None, None, len(ids0) + 1,
                                     p(off1, C.c_uint64), p(ids1, C.c_uint32)) == 0
    assert np.array_equal(off0, off1) and np.array_equal(ids0, ids1[:len(ids0)])
    # mask 0 reports nothing
    b, t, _ = w.raycast(o, d, mask=0)
    assert (b == pa.RAY_MISS).all() and np.isinf(t).all()
    assert (w.spherecast(o, d, rad, mask=0)[0] == pa.RAY_MISS).all()
    off, ids = w.overlap(qs, qp, half_extent=qh, mask=0)
    assert len(ids) == 0 and not off.any() and len(ids0) > 0
    # device variants: the host variants' bits
    masks = rng.choice([0, 1, 2, 3, 4, 7, ALL], n).astype(np.uint16)
    hb, ht, hn = w.raycast(o, d, mask=masks)
    sb, stt, sn = w.spherecast(o, d, rad, mask=masks)
    assert (hb != b0).any()  # the masks changed some answers
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ob, ot, on = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, device="cuda"), torch.empty((n, 3), device="cuda")
    dm = dev(masks.view(np.int16))
    w.raycast_device(dev(o), dev(d), ob, ot, on, mask=dm)
    w.sync()
    torch.cuda.synchronize()
    assert np.array_equal(ob.cpu().numpy().view(np.uint32), hb) and np.array_equal(ot.cpu().numpy(), ht)
    assert np.array_equal(on.cpu().numpy(), hn)
    w.spherecast_device(dev(o), dev(d), dev(rad), ob, ot, on, mask=dm)
    w.sync()
    torch.cuda.synchronize()
    assert np.array_equal(ob.cpu().numpy().view(np.uint32), sb) and np.array_equal(ot.cpu().numpy(), stt)
    assert np.array_equal(on.cpu().numpy(), sn)
    w.close()


def test_filtered_queries_between_updates_change_nothing():
    bodies, statics = _soup(9)
    n = len(bodies["pos"])
    rng = np.random.default_rng(9)
    f = _random_filters(rng, n)
    a = _world(bodies, statics, gravity_force=(0.0, -9.81, 0.0))
    b = _world(bodies, statics, gravity_force=(0.0, -9.81, 0.0))
    for w in (a, b):
        w.set_body_filters(*f)
    o, d = gq._casts(rng, 500, 6.0)
    for _ in range(20):
        a.update(DT)
        b.update(DT)
        b.raycast(o, d, mask=3)
        b.spherecast(o, d, 0.4, mask=5)
        b.overlap(2, o[:50], half_extent=[1, 1, 1], mask=ALL)
    a.sync()
    b.sync()
    for x, y in zip(_state(a) + list(a.get_manifolds()), _state(b) + list(b.get_manifolds())):
        assert np.array_equal(x, y)
    a.close()
    b.close()
