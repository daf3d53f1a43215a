"""GPU: contact events and per-manifold impulses (include/physics_hip.h), all through the C ABI.

What the events are compared with: tests/events_ref.py (numpy only: set differences of the per-update manifold id sets
that phys_get_manifolds reports), the rows of phys_get_manifolds / phys_get_contact_impulses (payload, bitwise), worlds
with events off (no bit of the step changes) and momentum balances computed in float64 from downloaded velocities."""
import ctypes as C

import numpy as np
import pytest

import events_ref as er

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
G = (0.0, -9.81, 0.0)


def _pa():
    import physics_amd
    return physics_amd


def _world(bodies, statics=None, flags=0, ground=True, events=None, **cfg):
    pa = _pa()
    f = pa.FLAG_COLLISIONS | (pa.FLAG_GROUND_PLANE if ground else 0) | flags
    cfg.setdefault("gravity_force", G)
    w = pa.World(pa.default_config(flags=f, gravity_offset=(0.0, 0.0, 0.0), **cfg))
    w.set_bodies(**bodies)
    if statics is not None:
        w.set_static_bodies(statics[0], rot=statics[1], shape_type=statics[2], half_extent=statics[3])
    if events:
        w.enable_contact_events(events)
    return w


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _heap(n=2000, seed=5):
    """A heap of mixed spheres, boxes and capsules falling onto the ground and four static boxes."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-11.0, 11.0, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.4, 14.0, n)
    shape = rng.choice([1, 2, 3], n, p=[0.35, 0.35, 0.3]).astype(np.uint32)
    he = rng.uniform(0.3, 0.7, (n, 3)).astype(np.float32)
    bodies = dict(pos=pos, rot=_quats(rng, n), shape_type=shape, half_extent=he)
    statics = (np.array([[4.0, 1.0, 4.0], [-5.0, 0.5, -3.0], [0.0, 1.5, -7.0], [-6.0, 1.0, 6.0]], np.float32), None,
               np.full(4, 2, np.uint32), np.array([[2.0, 1.0, 2.0], [1.5, 0.5, 1.5], [3.0, 1.5, 1.0], [1.0, 1.0, 1.0]], np.float32))
    return bodies, statics, 0


def _tower():
    """The 33 280-box tower of DESIGN section 2, for the cluster solver."""
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    return dict(pos=sc.pos, shape_type=sc.shape_type, half_extent=sc.half_extent), None, _pa().FLAG_SOLVER_CLUSTER


def _grid(n_side=20):
    """n_side^2 unit spheres lying on the ground, far enough apart never to touch each other: every one of them begins
    its ground contact in the first update."""
    xs = np.arange(n_side, dtype=np.float32) * 1.5
    pos = np.stack([np.repeat(xs, n_side), np.full(n_side * n_side, 0.499, np.float32), np.tile(xs, n_side)], axis=1)
    n = len(pos)
    return dict(pos=pos, shape_type=np.full(n, 1, np.uint32), half_extent=np.full((n, 3), 0.5, np.float32))


def _bytes(ev):
    return np.ascontiguousarray(ev).tobytes()


# ---- 1. events equal the manifold diff, exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["heap", "tower_cluster"])
def test_events_equal_the_manifold_diff(scene):
    """One update at a time over 132 updates (the colour table is rebuilt at updates 64 and 128): the drained events equal
    the set differences of consecutive phys_get_manifolds id sets - ids, kinds, steps, nothing left out - and every update
    raises as many BEGIN events as phys_stats.n_new_manifolds counts."""
    bodies, statics, flags = _heap() if scene == "heap" else _tower()
    w = _world(bodies, statics, flags, events=1 << 21)
    if scene == "tower_cluster":
        w.profile_enable(True)
    sets, drained, total = [], [], 0
    for u in range(132):
        w.update(DT)
        ids = w.get_manifolds()[0]
        ev, dropped = w.get_contact_events()
        st = w.get_stats()
        assert dropped == 0 and st.overflow == 0, (u, dropped, st.overflow)
        assert len(ids) == st.n_manifolds
        assert int((ev["kind"] == er.BEGIN).sum()) == st.n_new_manifolds, f"update {u + 1}"
        assert np.all(ev["step"] == u + 1)
        sets.append(ids)
        drained.append(ev)
        total = max(total, len(ids))
    w.sync()
    if scene == "tower_cluster":
        assert "solve_cluster" in w.profile_get()[0]
    w.close()
    got = er.keys_of(np.concatenate(drained))
    want = er.expected_events(sets)
    print(f"\n{scene}: {len(want)} events over 132 updates, up to {total} manifolds; "
          f"{int((want['kind'] == er.END).sum())} END")
    assert total > 1000 and int((want["kind"] == er.END).sum()) > 0
    assert len(got) == len(want) and np.array_equal(got, want)


# ---- 2. batches --------------------------------------------------------------------------------------------------------------
def test_a_batch_of_updates_gives_the_concatenation_of_the_single_drains():
    bodies, statics, flags = _heap()
    w = _world(bodies, statics, flags, events=1 << 20)
    single = []
    for _ in range(50):
        w.update(DT)
        ev, dropped = w.get_contact_events()
        assert dropped == 0
        single.append(ev)
    w.sync()
    w.close()
    single = np.concatenate(single)
    runs = []
    for _ in range(2):
        w = _world(bodies, statics, flags, events=1 << 20)
        w.update_n(DT, 50)
        ev, dropped = w.get_contact_events()
        assert dropped == 0
        assert len(w.get_contact_events()[0]) == 0  # the drain emptied the buffer
        w.sync()
        w.close()
        runs.append(ev)
    assert len(single) > 500 and set(np.unique(single["step"])) <= set(range(1, 51))
    assert _bytes(runs[0]) == _bytes(single)
    assert _bytes(runs[0]) == _bytes(runs[1])


# ---- 3. no bit of the step changes ------------------------------------------------------------------------------------------
def _everything(w):
    s = w.get_stats()
    counters = (s.n_pairs, s.n_manifolds, s.n_contacts, s.n_colors, s.color_rounds, s.n_new_manifolds, s.n_ground_manifolds,
                s.overflow, s.steps)
    return list(w.get_transforms()) + list(w.get_velocities()) + list(w.get_manifolds()) + [w.get_color_counts()], counters


@pytest.mark.parametrize("solver", ["default", "per_color", "cluster"])
def test_events_change_no_bit_of_the_step(solver):
    pa = _pa()
    if solver == "cluster":
        bodies, statics, flags = _tower()
        chunk = 50
    else:
        bodies, statics, flags = _heap(n=600, seed=8)
        flags |= pa.FLAG_SOLVER_PER_COLOR if solver == "per_color" else 0
        chunk = 25
    off = _world(bodies, statics, flags)
    on = _world(bodies, statics, flags, events=1 << 20)
    if solver == "cluster":
        off.profile_enable(True)
        on.profile_enable(True)
    events = 0
    for done in range(chunk, 201, chunk):
        for w in (off, on):
            w.update_n(DT, chunk)
            w.sync()
        (a, ca), (b, cb) = _everything(off), _everything(on)
        assert ca == cb, f"{solver}: counters of update {done} differ: {ca} {cb}"
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{solver}: update {done}, array {k} differs"
        events += len(on.get_contact_events()[0])
    assert events > 100
    if solver == "cluster":
        assert "solve_cluster" in on.profile_get()[0] and "solve_cluster" in off.profile_get()[0]
        assert on.profile_get()[0]["misc"][1] >= off.profile_get()[0].get("misc", (0, 0))[1] + 2 * 200  # two launches per update
    off.close()
    on.close()


# ---- 4. payload ----------------------------------------------------------------------------------------------------------------
def test_begin_payload_is_the_manifold_row_and_its_impulses_bitwise():
    bodies, statics, flags = _heap(n=800, seed=9)
    w = _world(bodies, statics, flags, events=1 << 20)
    checked = multi = nonzero = 0
    for u in range(70):
        w.update(DT)
        ids, counts, normals, points = w.get_manifolds()
        imp = w.get_contact_impulses()
        ev, dropped = w.get_contact_events()
        assert dropped == 0 and imp.shape == (len(ids), 4, 3)
        beyond = np.arange(4)[None, :] >= counts[:, None]
        assert not np.any(imp[beyond]), "impulses beyond a manifold's point count must be zero"
        assert np.all(imp[..., 0] >= 0.0), "a normal impulse never pulls"
        b = ev[ev["kind"] == er.BEGIN]
        e = ev[ev["kind"] == er.END]
        assert not np.any(e["point"]) and not np.any(e["normal"]) and not np.any(e["impulse"]) and not np.any(ev["reserved"])
        if not len(b):
            continue
        keys = (ids[:, 0].astype(np.uint64) << np.uint64(32)) | ids[:, 1]
        want = (b["body_a"].astype(np.uint64) << np.uint64(32)) | b["body_b"]
        row = np.searchsorted(keys, want)
        assert np.array_equal(keys[row], want)
        depth = np.where(np.arange(4)[None, :] < counts[row][:, None], points[row][:, :, 3], -np.inf)
        deepest = np.argmax(depth, axis=1)  # the first of equal maxima: the lowest index
        pt = points[row, deepest, :3]
        assert np.array_equal(b["point"].view(np.uint32), np.ascontiguousarray(pt).view(np.uint32)), f"update {u + 1}: point"
        assert np.array_equal(b["normal"].view(np.uint32), np.ascontiguousarray(normals[row]).view(np.uint32)), f"update {u + 1}: normal"
        pn = imp[row][:, :, 0]
        total = ((pn[:, 0] + pn[:, 1]) + pn[:, 2]) + pn[:, 3]
        assert total.dtype == np.float32
        assert np.array_equal(b["impulse"].view(np.uint32), total.view(np.uint32)), f"update {u + 1}: impulse"
        checked += len(b)
        multi += int((counts[row] > 1).sum())
        nonzero += int((total > 0).sum())
    w.sync()
    w.close()
    print(f"\npayload: {checked} BEGIN events checked, {multi} with more than one point, {nonzero} with an impulse")
    assert checked > 500 and multi > 50 and nonzero > 100


# ---- 5. impulses mean something ------------------------------------------------------------------------------------------------
def test_dropped_sphere_impulse_is_its_change_of_momentum():
    """A sphere of mass 2 dropped onto the ground (restitution 0, gravity applied at the centre): in the update of first
    touch, and again at rest, the impulse the manifold gave the sphere equals m (v_after - v_presolve) with v_presolve =
    v_before + F / m dt in float64, to 1e-4 relative; at rest no events are raised. The sphere is body A of its manifold
    and a manifold's normal points from A to B (include/spec/collide.h), so the impulse on it is -sum(pn) n."""
    pa = _pa()
    m = 2.0
    bodies = dict(pos=np.array([[0.0, 1.0, 0.0]], np.float32), mass=np.array([m], np.float32),
                  shape_type=np.array([pa.SHAPE_SPHERE], np.uint32), half_extent=np.full((1, 3), 0.5, np.float32))
    w = _world(bodies, events=64)
    F = np.array(G, np.float64)

    def balance(before, after):
        ids, counts, normals, _ = w.get_manifolds()
        imp = w.get_contact_impulses()
        assert len(ids) == 1 and ids[0, 1] == pa.GROUND_ID
        lhs = -imp[0, :, 0].astype(np.float64).sum() * normals[0].astype(np.float64)  # on body A: against the normal
        rhs = m * (after.astype(np.float64) - (before.astype(np.float64) + F / m * DT_S))
        return lhs, rhs

    touched = None
    for u in range(200):
        before = w.get_velocities()[0][0]
        w.update(DT)
        after = w.get_velocities()[0][0]
        ev, _ = w.get_contact_events()
        if touched is None and len(ev):
            assert len(ev) == 1 and ev[0]["kind"] == er.BEGIN and (ev[0]["body_a"], ev[0]["body_b"]) == (0, pa.GROUND_ID)
            assert ev[0]["step"] == u + 1
            lhs, rhs = balance(before, after)
            rel = np.abs(lhs - rhs).max() / np.abs(rhs).max()
            print(f"\nfirst touch in update {u + 1}: -sum(pn) n = {lhs}, m dv = {rhs}, relative difference {rel:.3e}")
            assert np.abs(rhs).max() > 0.5 and rel < 1e-4
            assert float(ev[0]["impulse"]) == pytest.approx(float(np.linalg.norm(rhs)), rel=1e-4)
            touched = u
        elif touched is not None and u > touched + 100:
            assert len(ev) == 0, f"update {u + 1}: an event at rest"
    assert touched is not None
    lhs, rhs = balance(before, after)
    rel = np.abs(lhs - rhs).max() / np.abs(rhs).max()
    print(f"at rest: -sum(pn) n = {lhs}, m dv = {rhs}, relative difference {rel:.3e}")
    assert rel < 1e-4 and rhs[1] == pytest.approx(9.81 * DT_S, rel=1e-3)
    w.sync()
    w.close()


def test_two_spheres_head_on_one_begin_one_end_and_twice_the_momentum():
    """Unit masses, touching 0.005 deep (inside the slop: no push-out), approaching at 2 and -2 with restitution 1: one BEGIN
    whose impulse is 2 m v within 1e-4, and one END once they have parted."""
    pa = _pa()
    v = 2.0
    bodies = dict(pos=np.array([[-0.4975, 5.0, 0.0], [0.4975, 5.0, 0.0]], np.float32),
                  lin_vel=np.array([[v, 0.0, 0.0], [-v, 0.0, 0.0]], np.float32),
                  shape_type=np.full(2, pa.SHAPE_SPHERE, np.uint32), half_extent=np.full((2, 3), 0.5, np.float32))
    w = _world(bodies, ground=False, gravity_force=(0.0, 0.0, 0.0), events=16)
    w.set_body_materials(restitution=[1.0, 0.0])
    w.update_n(DT, 10)
    ev, dropped = w.get_contact_events()
    lin = w.get_velocities()[0]
    w.sync()
    w.close()
    assert dropped == 0 and len(ev) == 2, ev
    assert (ev[0]["kind"], ev[0]["body_a"], ev[0]["body_b"], ev[0]["step"]) == (er.BEGIN, 0, 1, 1)
    assert (ev[1]["kind"], ev[1]["body_a"], ev[1]["body_b"]) == (er.END, 0, 1) and ev[1]["step"] > 1
    print(f"\nhead-on: impulse {ev[0]['impulse']:.7f} against 2 m v = {2 * v}; END in update {ev[1]['step']}")
    assert float(ev[0]["impulse"]) == pytest.approx(2.0 * 1.0 * v, rel=1e-4)
    assert np.abs(lin[:, 0] - np.array([-v, v])).max() < 1e-4 * v


# ---- 6. filters and statics ----------------------------------------------------------------------------------------------------
def test_filters_and_static_ids():
    """Body 0 (a box) rests on static collider 1; bodies 1 and 2 are overlapping spheres on the ground that share a negative
    group: their pair never appears. Masking body 0 out raises END for (0, static 1) in the next update, and BEGIN when the
    mask returns."""
    pa = _pa()
    bodies = dict(pos=np.array([[0.0, 2.499, 0.0], [10.0, 0.499, 0.0], [10.9, 0.499, 0.0]], np.float32),
                  shape_type=np.array([pa.SHAPE_BOX, pa.SHAPE_SPHERE, pa.SHAPE_SPHERE], np.uint32),
                  half_extent=np.full((3, 3), 0.5, np.float32))
    statics = (np.array([[30.0, 1.0, 0.0], [0.0, 1.0, 0.0]], np.float32), None, np.full(2, pa.SHAPE_BOX, np.uint32),
               np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 2.0]], np.float32))
    w = _world(bodies, statics, events=256)
    group = np.array([0, -3, -3], np.int16)
    w.set_body_filters(group=group)
    on_static = (0, pa.STATIC_ID_BIT | 1)
    w.update_n(DT, 40)
    ev, _ = w.get_contact_events()
    pairs = {(int(r["body_a"]), int(r["body_b"])) for r in ev}
    assert on_static in pairs and (1, pa.GROUND_ID) in pairs and (2, pa.GROUND_ID) in pairs
    assert (1, 2) not in pairs and (2, 1) not in pairs
    assert any((int(a), int(b)) == on_static for a, b in w.get_manifolds()[0])  # resting there now
    w.set_body_filters(mask=np.array([0, 0xFFFF, 0xFFFF], np.uint16), group=group)
    w.update(DT)
    ev, _ = w.get_contact_events()
    step = w.get_stats().steps
    assert [(int(r["kind"]), int(r["body_a"]), int(r["body_b"]), int(r["step"])) for r in ev] == [(er.END, *on_static, step)]
    w.set_body_filters(group=group)
    w.update(DT)
    ev, _ = w.get_contact_events()
    assert [(int(r["kind"]), int(r["body_a"]), int(r["body_b"]), int(r["step"])) for r in ev] == [(er.BEGIN, *on_static, step + 1)]
    w.update_n(DT, 20)
    ev, _ = w.get_contact_events()
    assert all((int(r["body_a"]), int(r["body_b"])) not in ((1, 2), (2, 1)) for r in ev)
    w.sync()
    w.close()


# ---- 7. capacity ------------------------------------------------------------------------------------------------------------------
def test_a_full_buffer_counts_what_it_drops_and_disturbs_nothing():
    pa = _pa()
    bodies = _grid()
    small = _world(bodies, events=4)
    off = _world(bodies)
    for w in (small, off):
        w.update(DT)
        w.sync()  # PHYS_OK: a full event buffer is no sticky error
    total = small.get_stats().n_new_manifolds
    assert total == 400
    for a, b in zip(list(small.get_transforms()) + list(small.get_velocities()), list(off.get_transforms()) + list(off.get_velocities())):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lib, n, dropped = small.lib, C.c_uint64(), C.c_uint64()
    ev_t = pa._abi.PhysContactEvent
    assert lib.phys_get_contact_events(small.h, None, 0, C.byref(n), C.byref(dropped)) == 0  # the count query
    assert (n.value, dropped.value) == (4, total - 4)
    two = (ev_t * 2)()
    assert lib.phys_get_contact_events(small.h, two, 2, C.byref(n), C.byref(dropped)) == pa._abi.PHYS_ERR_CAPACITY
    assert (n.value, dropped.value) == (4, total - 4)
    ev, d = small.get_contact_events()  # ... and the events were kept
    assert len(ev) == 4 and d == total - 4
    assert np.all(ev["kind"] == er.BEGIN) and np.all(ev["body_b"] == pa.GROUND_ID) and len(set(ev["body_a"])) == 4
    ev, d = small.get_contact_events()
    assert len(ev) == 0 and d == 0  # drained: the dropped count starts again
    small.update_n(DT, 3)
    small.sync()
    off.update_n(DT, 3)
    assert np.array_equal(small.get_transforms()[0], off.get_transforms()[0])
    small.close()
    off.close()


# ---- 8. life cycle ----------------------------------------------------------------------------------------------------------------
def test_new_body_and_static_sets_discard_events_and_start_all_begin():
    pa = _pa()
    bodies = _grid(8)
    statics = (np.array([[100.0, 1.0, 0.0]], np.float32), None, np.full(1, pa.SHAPE_BOX, np.uint32), np.ones((1, 3), np.float32))
    w = _world(bodies, statics, events=4096)
    for reset in ("bodies", "statics"):
        w.update_n(DT, 2)
        w.sync()
        if reset == "bodies":
            pos, rot = w.get_transforms()
            lin, ang = w.get_velocities()
            w.set_bodies(pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=bodies["shape_type"], half_extent=bodies["half_extent"])
        else:
            w.set_static_bodies(statics[0], shape_type=statics[2], half_extent=statics[3])
        ev, dropped = w.get_contact_events()
        assert len(ev) == 0 and dropped == 0, f"{reset}: pending events survived"
        w.update(DT)
        ev, _ = w.get_contact_events()
        st = w.get_stats()
        assert st.n_manifolds == 64 and len(ev) == 64 and np.all(ev["kind"] == er.BEGIN) and np.all(ev["step"] == st.steps), reset
        w.update(DT)
        assert len(w.get_contact_events()[0]) == 0
    w.close()


def test_enabling_mid_run_reports_against_the_update_before():
    bodies, statics, flags = _heap(n=600, seed=8)
    w = _world(bodies, statics, flags)
    w.update_n(DT, 30)
    previous = w.get_manifolds()[0]
    w.enable_contact_events(1 << 18)
    sets, drained = [], []
    for _ in range(10):
        w.update(DT)
        sets.append(w.get_manifolds()[0])
        drained.append(w.get_contact_events()[0])
    w.sync()
    want = er.expected_events(sets, first_step=31, previous=previous)
    got = er.keys_of(np.concatenate(drained))
    assert len(previous) > 100 and 0 < len(want) < len(previous) + len(sets[0])
    assert int((want["kind"] == er.END).sum()) > 0
    assert np.array_equal(got, want)
    # a new capacity drops what is pending and keeps the history; capacity 0 turns events off
    w.update(DT)
    w.enable_contact_events(1 << 10)
    assert len(w.get_contact_events()[0]) == 0
    last = w.get_manifolds()[0]
    w.update(DT)
    assert np.array_equal(er.keys_of(w.get_contact_events()[0]), er.expected_events([w.get_manifolds()[0]], first_step=42, previous=last))
    w.enable_contact_events(0)
    with pytest.raises(_pa().PhysError) as e:
        w.get_contact_events()
    assert e.value.code == _pa()._abi.PHYS_ERR_UNSUPPORTED
    w.update_n(DT, 2)
    assert w.get_contact_impulses().shape == (len(w.get_manifolds()[0]), 4, 3)  # impulses need no events
    w.sync()
    w.close()


def test_unsupported_worlds_and_argument_errors():
    pa = _pa()
    abi = pa._abi
    bodies = _grid(4)
    for flags, collisions in ((pa.FLAG_NO_WARM_START, True), (pa.FLAG_BROADPHASE_ONLY, True), (0, False)):
        f = (pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE if collisions else 0) | flags
        w = pa.World(pa.default_config(flags=f))
        w.set_bodies(**bodies)
        for call in (lambda: w.enable_contact_events(64), w.get_contact_events, w.get_contact_impulses):
            with pytest.raises(pa.PhysError) as e:
                call()
            assert e.value.code == abi.PHYS_ERR_UNSUPPORTED, (flags, collisions)
        w.update(DT)
        w.sync()
        w.close()
    w = _world(bodies)
    with pytest.raises(pa.PhysError) as e:
        w.get_contact_events()  # events off
    assert e.value.code == abi.PHYS_ERR_UNSUPPORTED
    with pytest.raises(pa.PhysError) as e:
        w.enable_contact_events(1 << 31)
    assert e.value.code == abi.PHYS_ERR_INVALID_ARG
    w.enable_contact_events(8)
    n = C.c_uint64()
    assert w.lib.phys_get_contact_events(w.h, None, 3, C.byref(n), None) == abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_contact_events(w.h, None, 0, None, None) == abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_contact_impulses(w.h, None, 0, None) == abi.PHYS_ERR_INVALID_ARG
    assert w.lib.phys_get_contact_events(w.h, None, 0, C.byref(n), None) == 0 and n.value == 0  # n_dropped may be NULL
    w.close()


def test_queries_between_updates_change_no_event():
    bodies, statics, flags = _heap(n=600, seed=8)
    rng = np.random.default_rng(3)
    origins = rng.uniform(-10, 10, (64, 3)).astype(np.float32)
    origins[:, 1] = 20.0
    dirs = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (64, 1))
    out = []
    for queries in (False, True):
        w = _world(bodies, statics, flags, events=1 << 18)
        for _ in range(40):
            w.update(DT)
            if queries:
                w.raycast(origins, dirs)
                w.overlap(np.full(4, 1, np.uint32), origins[:4] * np.array([1, 0.05, 1], np.float32), half_extent=np.full((4, 3), 2.0, np.float32))
        ev, dropped = w.get_contact_events()
        assert dropped == 0
        w.sync()
        w.close()
        out.append(ev)
    assert len(out[0]) > 100 and _bytes(out[0]) == _bytes(out[1])
