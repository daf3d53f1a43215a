"""GPU: trigger volumes (phys_set_triggers, phys_get_trigger_events, phys_get_trigger_overlaps) against the float64
reference of tests/trigger_ref.py, against phys_overlap, and against themselves.

Hand scenes; the random soup per update; occupancy-word and tail boundaries (33 and 70 triggers, 193 bodies, a list longer
than a wave); batches and a full event buffer; updates bit-identical with and without triggers; masks and filters; the
history rules of phys_set_triggers / phys_set_bodies / phys_set_trigger_poses, kept rotations; ghost slots; argument errors
and the capacity protocol of both getters."""
import ctypes as C

import numpy as np
import pytest

import trigger_ref as tr

pytestmark = pytest.mark.gpu
DT = tr.DT_NANOS


def _pa():
    import physics_amd
    return physics_amd


def _set_triggers(w, trig, mask=None):
    w.set_triggers(trig["shape"], trig["pos"], rot=trig.get("rot"), half_extent=trig["half_extent"], mask=mask)


def _gpu_pairs(w):
    return tr.csr_pairs(*w.get_trigger_overlaps())


def _event_list(ev):
    return [(int(e["kind"]), int(e["trigger"]), int(e["body"])) for e in ev]


def _soup_world(sc, events=1 << 16, mask=None):
    pa = _pa()
    cfg = pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0), ground_height=-sc["cage"])
    w = pa.World(cfg)
    w.set_bodies(sc["pos"], rot=sc["rot"], lin_vel=sc["vel"], shape_type=sc["shape"], half_extent=sc["half_extent"])
    _set_triggers(w, sc["triggers"], mask=mask)
    if events:
        w.enable_trigger_events(events)
    return w


def _follow(w, trig, shape, he, updates, label, check_overlap=False, category=None, mask=None):
    """`updates` single updates. After each one: the occupancy against the reference at the poses read back (band and cap of
    trigger_ref), optionally against World.overlap of the trigger shapes, and the drained events EXACTLY the difference of
    the GPU's own consecutive occupancies. Returns (all GPU events as (step, kind, trigger, body), reference event count)."""
    before_gpu, before_ref = _gpu_pairs(w), set()  # (every caller starts from a reset: nothing inside yet)
    assert before_gpu == set()
    n_near, n_ref_events, log = 0, 0, []
    step0 = int(w.get_stats().steps)
    for u in range(updates):
        w.update(DT)
        pos, rot = w.get_transforms()
        got = _gpu_pairs(w)
        want, near = tr.occupancy(trig, pos, rot, shape, he, category=category, mask=mask)
        n_near += tr.disagreements(got, want, near, f"{label} update {u}")
        if check_overlap:
            off, ids = w.overlap(trig["shape"], trig["pos"], trig.get("rot"), trig["half_extent"],
                                 mask=None if mask is None else np.asarray(mask, np.uint16))
            bodies = {(k, int(i)) for k in range(len(off) - 1) for i in ids[int(off[k]):int(off[k + 1])] if i < len(pos)}
            for pair in got ^ bodies:
                assert pair in near and abs(near[pair]) <= tr.NEAR, (label, u, "overlap", pair)
        ev, dropped = w.get_trigger_events()
        assert dropped == 0 and (ev["step"] == step0 + u + 1).all()
        assert _event_list(ev) == tr.events(before_gpu, got), (label, u)
        log += [(step0 + u + 1,) + e for e in _event_list(ev)]
        n_ref_events += len(tr.events(before_ref, want))
        before_gpu, before_ref = got, want
    assert n_near <= tr.near_cap(n_ref_events), f"{label}: {n_near} near-touch disagreements, {n_ref_events} reference events"
    w.sync()
    return log, n_ref_events


# ---- 1. hand scene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collide", [False, True])
def test_hand_scene_bodies_fly_through_a_box(collide):
    """A sphere, a box and a capsule, each carried through one box trigger by its velocity: one ENTER and one EXIT each, at
    the updates the reference derives from the poses read back. Without a collision stage (flags 0), then with collisions
    and a ground plane."""
    pa = _pa()
    flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE if collide else 0
    w = pa.World(pa.default_config(flags=flags, gravity_force=(0.0, 0.0, 0.0), gravity_offset=(0.0, 0.0, 0.0)))
    pos = np.array([[-4.03, 5.6, 0.2], [0.3, 5.0, -5.07], [4.55, 4.2, 0.1]], np.float32)  # (three heights: they never meet)
    vel = np.array([[9.1, 0, 0], [0, 0, 8.3], [-11.7, 0, 0.4]], np.float32)
    shape = np.array([pa.SHAPE_SPHERE, pa.SHAPE_BOX, pa.SHAPE_CAPSULE], np.uint32)
    he = np.array([[0.4, 0, 0], [0.3, 0.5, 0.2], [0.25, 0.6, 0]], np.float32)
    w.set_bodies(pos, lin_vel=vel, shape_type=shape, half_extent=he)
    trig = dict(shape=np.array([pa.SHAPE_BOX], np.uint32), pos=np.array([[0.13, 5.0, 0.07]], np.float32),
                rot=np.array([[0, 0.19866933, 0, 0.98006658]], np.float32), half_extent=np.array([[1.5, 1.0, 1.2]], np.float32))
    _set_triggers(w, trig)
    w.enable_trigger_events(64)
    log, n_ref = _follow(w, trig, shape, he, 60, f"hand collide={collide}", check_overlap=True)
    for body in range(3):
        kinds = [k for _, k, t, b in log if b == body]
        assert kinds == [pa.TRIGGER_ENTER, pa.TRIGGER_EXIT], (body, log)
    assert n_ref == 6 and _gpu_pairs(w) == set()
    w.close()


# ---- 2. random soup ------------------------------------------------------------------------------------------------------------
def test_random_soup_against_reference_overlap_and_itself():
    sc = tr.soup()
    w = _soup_world(sc)
    log, n_ref = _follow(w, sc["triggers"], sc["shape"], sc["half_extent"], 48, "soup", check_overlap=True)
    assert n_ref >= 100 and {k for _, k, _, _ in log} == {tr.ENTER, tr.EXIT}
    w.close()


# ---- 3. word and tail boundaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_trig", [33, 70])
def test_word_and_tail_boundaries(n_trig):
    """193 bodies (a partial last workgroup) and 33 / 70 triggers (a word boundary and a partial last word). Trigger 0 encloses
    every body (a list longer than a wave), trigger 1 none, triggers 31, 32 and 33 (the last bit of a word and the first of
    the next) have different occupants."""
    pa = _pa()
    rng = np.random.default_rng(n_trig)
    n = 193
    pos = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    shape = rng.choice([1, 2, 3], n).astype(np.uint32)
    he = rng.uniform(0.1, 0.3, (n, 3)).astype(np.float32)
    w = pa.World(pa.default_config(flags=0, gravity_force=(0.0, 0.0, 0.0)))
    w.set_bodies(pos, rot=tr._quats(rng, n), lin_vel=rng.normal(size=(n, 3)).astype(np.float32), shape_type=shape, half_extent=he)
    tp = rng.uniform(-6, 6, (n_trig, 3)).astype(np.float32)
    ts = rng.choice([1, 2, 3], n_trig).astype(np.uint32)
    th = rng.uniform(0.5, 2.5, (n_trig, 3)).astype(np.float32)
    tq = tr._quats(rng, n_trig)
    tp[0], ts[0], th[0] = (0, 0, 0), pa.SHAPE_BOX, (20, 20, 20)
    tp[1], ts[1], th[1] = (100, 100, 100), pa.SHAPE_SPHERE, (1, 0, 0)
    for k, x in ((31, -4.0), (32, 0.0)) + (((33, 4.0),) if n_trig > 33 else ()):
        tp[k], ts[k], th[k], tq[k] = (x, 0, 0), pa.SHAPE_BOX, (2, 7, 7), (0, 0, 0, 1)
    trig = dict(shape=ts, pos=tp, rot=tq, half_extent=th)
    _set_triggers(w, trig)
    w.enable_trigger_events(1 << 14)
    _follow(w, trig, shape, he, 3, f"boundaries {n_trig}")
    off, ids = w.get_trigger_overlaps()
    assert len(off) == n_trig + 1
    assert list(ids[int(off[0]):int(off[1])]) == list(range(n)) and off[2] == off[1]
    lists = [set(ids[int(off[k]):int(off[k + 1])].tolist()) for k in range(n_trig)]
    assert lists[31] and lists[32] and lists[31] != lists[32]
    if n_trig > 33:
        assert lists[33] and lists[33] != lists[32] and lists[33] != lists[31]
    w.close()


# ---- 4. batches and drops ------------------------------------------------------------------------------------------------------
def test_batch_equals_single_updates_and_a_full_buffer_drops():
    sc = tr.soup()
    single, batch, small = _soup_world(sc), _soup_world(sc), _soup_world(sc, events=50)
    for _ in range(48):
        single.update(DT)
    batch.update_n(DT, 48)
    small.update_n(DT, 48)
    a, da = single.get_trigger_events()
    b, db = batch.get_trigger_events()
    assert da == 0 and db == 0 and len(a) > 100 and a.tobytes() == b.tobytes()
    c, dc = small.get_trigger_events()
    assert len(c) == 50 and len(c) + dc == len(a)
    small.sync()  # no sticky error
    assert _gpu_pairs(small) == _gpu_pairs(single) == _gpu_pairs(batch)
    # the lists are the history folded up: ENTER minus EXIT
    occ = set()
    for e in a:
        (occ.add if e["kind"] == tr.ENTER else occ.discard)((int(e["trigger"]), int(e["body"])))
    assert occ == _gpu_pairs(single)
    for w in (single, batch, small):
        w.close()


# ---- 5. leaves updates alone ---------------------------------------------------------------------------------------------------
def _snapshot(w):
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    st = w.get_stats()
    return [pos, rot, lin, ang], {k: getattr(st, k) for k, _ in type(st)._fields_}, w.get_manifolds()


@pytest.mark.parametrize("name", ["c2", "cluster_tower"])
def test_triggers_leave_updates_bit_identical(name):
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
        w.profile_enable(True)
        worlds.append(w)
    quiet, watched = worlds
    rng = np.random.default_rng(5)
    lo, hi = sc.pos.min(0), sc.pos.max(0)
    watched.set_triggers(pa.SHAPE_BOX, rng.uniform(lo, hi, (16, 3)).astype(np.float32), rot=tr._quats(rng, 16),
                         half_extent=rng.uniform(1, 4, (16, 3)).astype(np.float32))
    watched.enable_trigger_events(1 << 16)
    for w in worlds:
        w.update_n(scenes.DT_NANOS, 24)
        w.sync()
    ev, _ = watched.get_trigger_events()
    assert len(ev) > 0
    a, b = _snapshot(quiet), _snapshot(watched)
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert x.tobytes() == y.tobytes()
    (pq, sq), (pw, sw) = quiet.profile_get(), watched.profile_get()
    assert sq == sw == 24
    for stage in set(pq) | set(pw):
        if stage != "misc":
            assert pq.get(stage, (0, 0))[1] == pw.get(stage, (0, 0))[1], stage
    assert pw["misc"][1] == pq.get("misc", (0, 0))[1] + 24  # one launch per update
    for w in worlds:
        w.close()


# ---- 6. masks and filters ------------------------------------------------------------------------------------------------------
def test_masks_and_body_filters():
    pa = _pa()
    sc = tr.soup()
    n = len(sc["pos"])
    rng = np.random.default_rng(2)
    category = rng.choice([1, 2, 4], n).astype(np.uint16)
    mask = np.array([1, 2, 4, 0xFFFF, 3, 0], np.uint16)
    w = _soup_world(sc, mask=mask)
    w.set_body_filters(category=category)
    _follow(w, sc["triggers"], sc["shape"], sc["half_extent"], 6, "masks", check_overlap=True, category=category, mask=mask)
    off, ids = w.get_trigger_overlaps()
    for k in range(6):
        assert all(category[i] & mask[k] for i in ids[int(off[k]):int(off[k + 1])])
    assert off[6] == off[5] and off[4] > off[3]  # mask 0 sees nothing; 0xFFFF sees something
    # a resident of trigger 3 moved out of every mask: EXIT at the next update from every trigger that held it, no ENTER
    body = int(ids[int(off[3])])
    held = sorted(k for k, i in _gpu_pairs(w) if i == body)
    assert 3 in held
    category[body] = 0
    w.set_body_filters(category=category)
    w.update(DT)
    ev, _ = w.get_trigger_events()
    assert sorted(int(e["trigger"]) for e in ev if e["body"] == body) == held
    assert all(e["kind"] == pa.TRIGGER_EXIT for e in ev if e["body"] == body)
    assert not any(i == body for _, i in _gpu_pairs(w))
    w.close()


# ---- 7. history ----------------------------------------------------------------------------------------------------------------
def test_history_moves_resets_and_clearing():
    pa = _pa()
    n = 40
    pos = np.array([[(i % 8) * 1.0, 5.0, (i // 8) * 1.0] for i in range(n)], np.float32)
    shape = np.full(n, pa.SHAPE_SPHERE, np.uint32)
    he = np.full((n, 3), 0.2, np.float32)
    w = pa.World(pa.default_config(flags=0, gravity_force=(0.0, 0.0, 0.0)))
    w.profile_enable(True)
    w.set_bodies(pos, shape_type=shape, half_extent=he)
    w.update_n(DT, 4)
    base, steps = w.profile_get()
    assert steps == 4 and "misc" not in base
    tpos = np.array([[1.0, 5.0, 0.5], [5.5, 5.0, 3.5]], np.float32)
    w.set_triggers(pa.SHAPE_BOX, tpos, half_extent=[[1.3, 1, 0.8], [1.8, 1, 0.8]])
    w.enable_trigger_events(1024)
    assert _gpu_pairs(w) == set()  # before the first update since a reset every list is empty
    w.update(DT)
    first = _gpu_pairs(w)
    in0, in1 = {i for k, i in first if k == 0}, {i for k, i in first if k == 1}
    assert in0 and in1 and not in0 & in1
    ev, _ = w.get_trigger_events()
    assert _event_list(ev) == tr.events(set(), first)
    # moving trigger 0 off its occupants: EXIT for each of them, nothing for trigger 1's
    tpos2 = tpos.copy()
    tpos2[0] = [50, 50, 50]
    w.set_trigger_poses(tpos2)
    w.update(DT)
    ev, _ = w.get_trigger_events()
    assert _event_list(ev) == [(pa.TRIGGER_EXIT, 0, i) for i in sorted(in0)]
    # ... and a rotation alone (positions as they are): trigger 1 turned by 90 degrees about y sheds the far bodies
    w.set_trigger_poses(tpos2, rot=[[0, 0, 0, 1], [0, 0.70710678, 0, 0.70710678]])
    w.update(DT)
    ev, _ = w.get_trigger_events()
    turned = {i for k, i in _gpu_pairs(w) if k == 1}
    assert turned != in1 and _event_list(ev) == tr.events({(1, i) for i in in1}, {(1, i) for i in turned})
    w.set_trigger_poses(tpos2, rot=None)  # keeps the rotation
    w.update(DT)
    assert len(w.get_trigger_events()[0]) == 0
    # set_triggers discards the pending events; then ENTER for every occupant and no EXIT
    w.set_trigger_poses(tpos)
    w.update(DT)  # pending events now
    w.set_triggers(pa.SHAPE_BOX, tpos, half_extent=[[1.3, 1, 0.8], [1.8, 1, 0.8]])
    ev, dropped = w.get_trigger_events()
    assert len(ev) == 0 and dropped == 0 and _gpu_pairs(w) == set()
    w.update(DT)
    ev, _ = w.get_trigger_events()
    assert _event_list(ev) == tr.events(set(), first)
    # set_bodies likewise (the same bodies, shifted along z)
    w.set_trigger_poses(tpos2)
    w.update(DT)  # pending EXITs
    w.set_bodies(pos + np.array([0.0, 0.0, 1.0], np.float32), shape_type=shape, half_extent=he)
    ev, _ = w.get_trigger_events()
    assert len(ev) == 0 and _gpu_pairs(w) == set()
    w.update(DT)
    ev, _ = w.get_trigger_events()
    now = _gpu_pairs(w)
    assert now and all(e["kind"] == pa.TRIGGER_ENTER for e in ev) and _event_list(ev) == tr.events(set(), now)
    # clearing the set: nothing is launched any more, in misc either
    w.sync()
    w.profile_enable(True)  # resets the sums
    w.set_triggers(pa.SHAPE_BOX, np.zeros((0, 3), np.float32), half_extent=np.zeros((0, 3), np.float32))
    w.update_n(DT, 4)
    after, steps = w.profile_get()
    assert steps == 4 and after == {k: (after[k][0], v[1]) for k, v in base.items()}
    off, ids = w.get_trigger_overlaps()
    assert list(off) == [0] and len(ids) == 0 and len(w.get_trigger_events()[0]) == 0
    w.close()


def test_poses_without_rotations_keep_the_rotations_of_set_triggers():
    """The quaternions phys_set_triggers was given live on the host; phys_set_trigger_poses(rot = NULL) builds the records from
    them again. Two volumes that are not rotation-symmetric - a box (2, 0.5, 0.5) turned 45 degrees about z, a capsule (r 0.3,
    hl 1.5) turned 90 degrees about z, its axis along x then - and four small spheres at rest: one in each volume's turned tip,
    0.5 and 1.1 clear of the volume as the identity rotation would leave it, and one at each centre."""
    pa = _pa()
    w = pa.World(pa.default_config(flags=0, gravity_force=(0.0, 0.0, 0.0)))
    d = 1.6 * np.sqrt(0.5)
    pos = np.array([[d, d, 0], [0, 0, 0], [11.5, 0, 0], [10, 0, 0]], np.float32)
    w.set_bodies(pos, shape_type=np.full(4, pa.SHAPE_SPHERE, np.uint32), half_extent=np.full((4, 3), 0.1, np.float32))
    tpos = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    rot = np.array([[0, 0, 0.38268343, 0.92387953], [0, 0, 0.70710678, 0.70710678]], np.float32)
    w.set_triggers(np.array([pa.SHAPE_BOX, pa.SHAPE_CAPSULE], np.uint32), tpos, rot=rot,
                   half_extent=np.array([[2, 0.5, 0.5], [0.3, 1.5, 0]], np.float32))
    w.enable_trigger_events(64)
    w.update(DT)
    everybody = {(0, 0), (0, 1), (1, 2), (1, 3)}
    assert _gpu_pairs(w) == everybody
    assert _event_list(w.get_trigger_events()[0]) == tr.events(set(), everybody)
    w.set_trigger_poses(tpos, rot=None)
    w.update(DT)
    assert _gpu_pairs(w) == everybody and len(w.get_trigger_events()[0]) == 0
    w.set_trigger_poses(tpos, rot=[[0, 0, 0, 1], [0, 0, 0, 1]])
    w.update(DT)
    assert _gpu_pairs(w) == {(0, 1), (1, 3)}
    assert sorted(_event_list(w.get_trigger_events()[0])) == [(pa.TRIGGER_EXIT, 0, 0), (pa.TRIGGER_EXIT, 1, 2)]
    w.close()


# ---- 8. ghost world ------------------------------------------------------------------------------------------------------------
def test_ghost_slots_are_never_occupants():
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
    # one volume around the ghosts alone, one around everything
    right.set_triggers([pa.SHAPE_BOX, pa.SHAPE_SPHERE], [[-1.5, 5.0, 0.0], [0, 0, 0]], half_extent=[[0.4, 3, 9], [500, 0, 0]])
    right.enable_trigger_events(256)
    right.update(DT)
    right.sync()
    off, ids = right.get_trigger_overlaps()
    assert off[1] == 0 and list(ids) == list(range(n))
    ev, _ = right.get_trigger_events()
    assert _event_list(ev) == [(pa.TRIGGER_ENTER, 1, i) for i in range(n)]
    left.close()
    right.close()


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_capacity_protocols():
    pa = _pa()
    from physics_amd import _abi
    f32p, u32p, u64p = _abi.f32p, _abi.u32p, _abi.u64p
    w = pa.World(pa.default_config(flags=0, gravity_force=(0.0, 0.0, 0.0)))
    pos = np.array([[0, 0, 0], [0.5, 0, 0], [9, 0, 0]], np.float32)
    w.set_bodies(pos, shape_type=np.full(3, pa.SHAPE_SPHERE, np.uint32), half_extent=np.full((3, 3), 0.25, np.float32))

    def raw_set(n, shape, p, he, rot=None):
        shape, p, he = np.ascontiguousarray(shape, np.uint32), np.ascontiguousarray(p, np.float32), np.ascontiguousarray(he, np.float32)
        return w.lib.phys_set_triggers(w.h, n, shape.ctypes.data_as(u32p), p.ctypes.data_as(f32p),
                                       None if rot is None else np.ascontiguousarray(rot, np.float32).ctypes.data_as(f32p),
                                       he.ctypes.data_as(f32p), None)

    one = np.ones((1025, 3), np.float32)
    assert raw_set(1025, np.full(1025, 2), one, one) == _abi.PHYS_ERR_INVALID_ARG
    assert raw_set(1024, np.full(1024, 2), one[:1024], one[:1024]) == 0
    assert raw_set(1, [0], one[:1], one[:1]) == _abi.PHYS_ERR_INVALID_ARG        # PHYS_SHAPE_NONE
    assert raw_set(1, [7], one[:1], one[:1]) == _abi.PHYS_ERR_INVALID_ARG
    assert raw_set(1, [2], [[np.nan, 0, 0]], one[:1]) == _abi.PHYS_ERR_INVALID_ARG
    assert raw_set(1, [2], one[:1], one[:1], rot=[[0, np.inf, 0, 1]]) == _abi.PHYS_ERR_INVALID_ARG
    assert raw_set(1, [2], one[:1], [[1, -0.5, 1]]) == _abi.PHYS_ERR_INVALID_ARG
    assert raw_set(1, [2], one[:1], [[1, np.inf, 1]]) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_set_triggers(w.h, 1, None, one.ctypes.data_as(f32p), None, one.ctypes.data_as(f32p), None) == _abi.PHYS_ERR_INVALID_ARG
    # (a refused call leaves the set that was there: 1024 volumes)
    assert w.lib.phys_set_trigger_poses(w.h, 3, one.ctypes.data_as(f32p), None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_set_trigger_poses(w.h, 1024, None, None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_set_trigger_poses(w.h, 1024, one.ctypes.data_as(f32p), None) == 0
    # events off: the getter is unsupported, the occupancy is still tracked
    w.set_triggers(pa.SHAPE_SPHERE, [[0.2, 0, 0], [9, 0, 0], [50, 0, 0]], half_extent=[1, 0, 0])
    n, dropped = C.c_uint64(), C.c_uint64()
    assert w.lib.phys_get_trigger_events(w.h, None, 0, C.byref(n), C.byref(dropped)) == _abi.PHYS_ERR_UNSUPPORTED
    with pytest.raises(pa.PhysError) as e:
        w.get_trigger_events()
    assert e.value.code == _abi.PHYS_ERR_UNSUPPORTED
    w.update(DT)
    assert _gpu_pairs(w) == {(0, 0), (0, 1), (1, 2)}
    assert w.lib.phys_trigger_events_enable(w.h, 1 << 31) == _abi.PHYS_ERR_INVALID_ARG
    # enabling resets nothing: no events for what is inside already
    w.enable_trigger_events(8)
    w.update(DT)
    assert len(w.get_trigger_events()[0]) == 0
    w.set_trigger_poses([[0.2, 0, 0], [50, 0, 0], [9, 0, 0]])
    w.update(DT)
    # capacity protocol of the event getter
    assert w.lib.phys_get_trigger_events(w.h, None, 0, None, None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_trigger_events(w.h, None, 4, C.byref(n), None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_trigger_events(w.h, None, 0, C.byref(n), C.byref(dropped)) == 0 and (n.value, dropped.value) == (2, 0)
    out = np.zeros(4, pa.TRIGGER_EVENT_DTYPE)
    ptr = out.ctypes.data_as(C.POINTER(_abi.PhysTriggerEvent))
    assert w.lib.phys_get_trigger_events(w.h, ptr, 1, C.byref(n), None) == _abi.PHYS_ERR_CAPACITY and n.value == 2  # kept
    assert w.lib.phys_get_trigger_events(w.h, ptr, 4, C.byref(n), C.byref(dropped)) == 0 and n.value == 2
    step = int(w.get_stats().steps)
    assert [tuple(int(x) for x in e) for e in out[:2]] == [(2, 2, pa.TRIGGER_ENTER, step), (1, 2, pa.TRIGGER_EXIT, step)]
    assert w.lib.phys_get_trigger_events(w.h, ptr, 4, C.byref(n), None) == 0 and n.value == 0  # drained
    # ... and of the overlaps: offsets always written
    off = np.full(4, 99, np.uint64)
    ids = np.zeros(8, np.uint32)
    assert w.lib.phys_get_trigger_overlaps(w.h, 0, None, None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_trigger_overlaps(w.h, 4, off.ctypes.data_as(u64p), None) == _abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_trigger_overlaps(w.h, 2, off.ctypes.data_as(u64p), ids.ctypes.data_as(u32p)) == _abi.PHYS_ERR_CAPACITY
    assert list(off) == [0, 2, 2, 3]
    assert w.lib.phys_get_trigger_overlaps(w.h, 3, off.ctypes.data_as(u64p), ids.ctypes.data_as(u32p)) == 0
    assert list(off) == [0, 2, 2, 3] and list(ids[:3]) == [0, 1, 2]
    o2, i2 = w.get_trigger_overlaps(cap=1)  # the wrapper retries once
    assert list(o2) == [0, 2, 2, 3] and list(i2) == [0, 1, 2]
    # a new capacity drops the pending events; 0 turns them off
    w.set_trigger_poses([[50, 0, 0], [50, 0, 0], [50, 0, 0]])
    w.update(DT)
    w.enable_trigger_events(16)
    assert len(w.get_trigger_events()[0]) == 0
    w.enable_trigger_events(0)
    with pytest.raises(pa.PhysError):
        w.get_trigger_events()
    w.sync()
    w.close()
