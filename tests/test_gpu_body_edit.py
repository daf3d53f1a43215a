"""GPU: in-place body edits (phys_set_body_poses, phys_set_body_velocities, phys_apply_impulses, phys_apply_forces,
phys_get_body_states and their _device twins) against numpy's "one entry after another", against the library's own statement of
the arithmetic (tests/cpp/body_edit_probe.cpp: include/spec/body_edit.h compiled by the host compiler) bit for bit, against the
float64 reference of tests/body_edit_ref.py within its derived bound, against the existing single-body force calls, and against
worlds built afresh from the edited state.

Body counts 1, 63, 64, 65, 257 (either side of a wave, past a workgroup); entry counts 1, 64, 65, 300 with shuffled ids that
contain repeats. The collision scenes are one 4 x 4 x 4 pile of cubes on the ground."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import body_edit_probe as bp
import body_edit_ref as br

pytestmark = pytest.mark.gpu
DT = 16_666_667
SIZES = [(nb, ne) for nb in (1, 63, 64, 65, 257) for ne in (1, 64, 65, 300)]
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (point, third array) given


def _pa():
    import physics_amd
    return physics_amd


@functools.lru_cache(maxsize=None)
def _probe():
    import tempfile
    return bp.build(tempfile.mkdtemp(prefix="body_edit_probe_") + "/body_edit_probe")


def _bodies(n, seed, layout="shared"):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    return dict(pos=rng.uniform(-5, 5, (n, 3)).astype(np.float32), rot=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                vel=rng.normal(size=(n, 3)).astype(np.float32), ang=rng.normal(size=(n, 3)).astype(np.float32),
                mass=rng.uniform(0.5, 3.0, n).astype(np.float32), inertia=br.inertia_tensors(layout, n, rng))


def _world(b, flags=0, **cfg):
    pa = _pa()
    w = pa.World(pa.default_config(flags=flags, **cfg))
    w.set_bodies(b["pos"], rot=b.get("rot"), lin_vel=b.get("vel"), ang_vel=b.get("ang"), mass=b.get("mass"),
                 inertia=None if b.get("inertia") is None else b["inertia"].reshape(-1, 9), shape_type=b.get("shape"),
                 half_extent=b.get("half_extent"))
    return w


def _entries(n, m, seed):
    """m entries on n bodies: shuffled ids with repeats (a run of up to seven on one body), three (m, 3) arrays and rotations."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n, m)
    ids[: min(m, 7)] = ids[0]
    rng.shuffle(ids)
    return dict(ids=ids.astype(np.uint32), a=(rng.normal(size=(m, 3)) * 3).astype(np.float32), b=rng.uniform(-6, 6, (m, 3)).astype(np.float32),
                c=rng.normal(size=(m, 3)).astype(np.float32), rot=rng.normal(size=(m, 4)).astype(np.float32))


def _one_after_another(start, ids, values):
    out = np.array(start)
    for k, i in enumerate(ids):
        out[i] = values[k]
    return out


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _state(w):
    return (*w.get_transforms(), *w.get_velocities())


# ---- 1. set and get -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,ne", SIZES)
def test_set_and_get(nb, ne):
    b = _bodies(nb, 100 + nb, "diag")
    e = _entries(nb, ne, 7 * nb + ne)
    w = _world(b)
    pos, rot, lin, ang = b["pos"], b["rot"], b["vel"], b["ang"]
    query = np.random.default_rng(ne).integers(0, nb, 2 * nb + 3).astype(np.uint32)  # any order, with repeats
    steps = [("pose", dict(pos=e["a"], rot=e["rot"])), ("pose", dict(pos=e["b"])), ("pose", dict(rot=e["rot"][::-1].copy())),
             ("vel", dict(lin=e["c"], ang=e["a"])), ("vel", dict(lin=e["b"])), ("vel", dict(ang=e["c"]))]
    for kind, kw in steps:
        if kind == "pose":
            w.set_body_poses(e["ids"], **kw)
            pos = _one_after_another(pos, e["ids"], kw["pos"]) if "pos" in kw else pos
            rot = _one_after_another(rot, e["ids"], kw["rot"]) if "rot" in kw else rot  # stored as given: not normalised
        else:
            w.set_body_velocities(e["ids"], **kw)
            lin = _one_after_another(lin, e["ids"], kw["lin"]) if "lin" in kw else lin
            ang = _one_after_another(ang, e["ids"], kw["ang"]) if "ang" in kw else ang
        got = _state(w)
        for g, want in zip(got, (pos, rot, lin, ang)):
            assert _same(g, want), (kind, list(kw))  # untouched bodies included: the whole arrays
        for g, want in zip(w.get_body_states(query), (pos, rot, lin, ang)):
            assert _same(g, want[query]), (kind, list(kw))
    # the velocity sets left the masses alone: an impulse at the centre gives J * inv_mass
    some = np.unique(e["ids"])
    J = np.random.default_rng(5).normal(size=(len(some), 3)).astype(np.float32)
    w.apply_impulses(some, J)
    inv_mass = (np.float32(1.0) / b["mass"]).astype(np.float32)
    want = lin.copy()
    want[some] = lin[some] + J * inv_mass[some, None]
    got_lin, got_ang = w.get_velocities()
    assert _same(got_lin, want) and _same(got_ang, ang)
    w.sync()
    w.close()


# ---- 2. impulses ----------------------------------------------------------------------------------------------------------------
def _impulse_case(nb, ne, layout, has_point, has_third, ids=None):
    b = _bodies(nb, 200 + nb, layout)
    e = _entries(nb, ne, 11 * nb + ne)
    ids = e["ids"] if ids is None else ids
    point, third = (e["b"] if has_point else None), (e["c"] if has_third else None)
    w = _world(b)
    w.apply_impulses(ids, e["a"], point=point, ang_impulse=third)
    gv, gw = w.get_velocities()
    pos_after, rot_after = w.get_transforms()
    w.sync()
    w.close()
    assert _same(pos_after, b["pos"]) and _same(rot_after, b["rot"])
    scene = os.path.join(os.path.dirname(_probe()), f"imp_{nb}_{ne}_{layout}_{int(has_point)}{int(has_third)}.txt")
    bp.write_scene(scene, "impulses", layout, b["pos"], ids, e["a"], point, third, vel=b["vel"], ang=b["ang"], mass=b["mass"], inertia=b["inertia"])
    pv, pw, inv = bp.run(_probe(), scene)
    assert _same(gv, pv) and _same(gw, pw), np.argwhere((gv != pv) | (gw != pw))[:8]
    if layout == "shared":
        inv = np.broadcast_to(inv[0], inv.shape)
    inv_mass = (np.float32(1.0) / b["mass"]).astype(np.float32)
    ref = br.apply_impulses(b["pos"], b["vel"], b["ang"], inv_mass, inv, ids, e["a"], point, third)
    assert (np.abs(gv - ref["v"]) <= br.bound(ref["K"], ref["Sv"])).all()
    assert (np.abs(gw - ref["w"]) <= br.bound(ref["K"], ref["Sw"])).all()
    return gv, gw, b


@pytest.mark.parametrize("layout", ["shared", "diag", "full"])
@pytest.mark.parametrize("nb,ne", SIZES)
def test_impulses_equal_the_spec_and_the_reference(nb, ne, layout):
    _impulse_case(nb, ne, layout, True, True)


@pytest.mark.parametrize("layout", ["shared", "diag", "full"])
@pytest.mark.parametrize("has_point,has_third", VARIANTS[:3])
def test_impulses_without_point_or_angular_part(layout, has_point, has_third):
    _impulse_case(65, 300, layout, has_point, has_third)


@pytest.mark.parametrize("layout", ["shared", "full"])
def test_a_run_of_300_entries_on_one_body(layout):
    gv, gw, b = _impulse_case(65, 300, layout, True, True, ids=np.full(300, 5, np.uint32))
    others = np.arange(65) != 5
    assert _same(gv[others], b["vel"][others]) and _same(gw[others], b["ang"][others]) and (gv[5] != b["vel"][5]).any()


# ---- 3. forces: a batch equals the same single calls ----------------------------------------------------------------------------
def _force_case(nb, ne, has_point, has_torque):
    b = _bodies(nb, 300 + nb, "diag")
    e = _entries(nb, ne, 13 * nb + ne)
    point, torque = (e["b"] if has_point else None), (e["c"] if has_torque else None)
    wa, wb = _world(b), _world(b)
    wa.apply_forces(e["ids"], e["a"], point=point, torque=torque)
    for k, i in enumerate(e["ids"]):
        if has_point:
            wb.apply_force_at_position(int(i), e["a"][k], point[k])
        else:
            wb.apply_force_centre_of_gravity(int(i), e["a"][k])
        if has_torque:  # no single call adds a bare torque: the accumulator sum itself, in float32
            F, T = wb.get_forces()
            T[i] = T[i] + torque[k]
            wb.set_forces(F, T)
    fa, fb = wa.get_forces(), wb.get_forces()
    assert _same(fa[0], fb[0]) and _same(fa[1], fb[1])
    assert np.abs(fa[0]).max() > 0 and (has_point or has_torque) == bool(np.abs(fa[1]).max() > 0)
    for w in (wa, wb):
        w.update(DT)
    for x, y in zip(_state(wa), _state(wb)):
        assert _same(x, y)
    fa = wa.get_forces()
    assert not fa[0].any() and not fa[1].any()  # consumed by the update, as ever
    for w in (wa, wb):
        w.sync()
        w.close()


@pytest.mark.parametrize("nb,ne", SIZES)
def test_force_batch_equals_single_calls(nb, ne):
    has_point, has_torque = VARIANTS[SIZES.index((nb, ne)) % 4]
    _force_case(nb, ne, has_point, has_torque and ne <= 65)  # (the torque twin costs a read-back per entry)


@pytest.mark.parametrize("has_point,has_torque", VARIANTS)
def test_force_batch_variants(has_point, has_torque):
    _force_case(65, 65, has_point, has_torque)


# ---- 4. device variants ---------------------------------------------------------------------------------------------------------
def _sorted_device(e):
    import torch
    ids = torch.from_numpy(e["ids"].astype(np.int32)).cuda()
    ids, order = torch.sort(ids, stable=True)
    dev = {k: torch.from_numpy(e[k]).cuda()[order].contiguous() for k in ("a", "b", "c", "rot")}
    torch.cuda.synchronize()
    return ids, dev


@pytest.mark.parametrize("nb,ne", [(1, 1), (64, 65), (65, 300), (257, 64)])
@pytest.mark.parametrize("layout", ["shared", "full"])
def test_device_variants_equal_host_variants(nb, ne, layout):
    import torch
    b = _bodies(nb, 400 + nb, layout)
    e = _entries(nb, ne, 17 * nb + ne)
    ids, d = _sorted_device(e)
    wh, wd = _world(b), _world(b)
    wh.set_body_poses(e["ids"], pos=e["b"], rot=e["rot"])
    wd.set_body_poses_device(ids, pos=d["b"], rot=d["rot"])
    wh.set_body_velocities(e["ids"], lin=e["c"], ang=e["a"])
    wd.set_body_velocities_device(ids, lin=d["c"], ang=d["a"])
    wh.apply_impulses(e["ids"], e["a"], point=e["b"], ang_impulse=e["c"])
    wd.apply_impulses_device(ids, d["a"], point=d["b"], ang_impulse=d["c"])
    wh.apply_impulses(e["ids"], e["c"])
    wd.apply_impulses_device(ids, d["c"])
    wh.apply_forces(e["ids"], e["a"], point=e["b"], torque=e["c"])
    wd.apply_forces_device(ids, d["a"], point=d["b"], torque=d["c"])
    wd.sync()
    for x, y in zip(_state(wh) + wh.get_forces(), _state(wd) + wd.get_forces()):
        assert _same(x, y)
    # the read-back on device arrays, ids in any order
    q = np.random.default_rng(3).integers(0, nb, nb + 5).astype(np.int32)
    tq = torch.from_numpy(q).cuda()
    outs = [torch.zeros((len(q), c), dtype=torch.float32, device="cuda") for c in (3, 4, 3, 3)]
    torch.cuda.synchronize()
    wd.get_body_states_device(tq, *outs)
    wd.sync()
    for t, want in zip(outs, wh.get_body_states(q.astype(np.uint32))):
        assert _same(t.cpu().numpy(), want)
    for w in (wh, wd):
        w.sync()
        w.close()


def test_device_ids_out_of_order_are_reported_once():
    import torch
    pa = _pa()
    b = _bodies(65, 5, "diag")
    w = _world(b)
    ids = torch.tensor([5, 2, 5], dtype=torch.int32, device="cuda")
    J = torch.ones((3, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w.apply_impulses_device(ids, J)
    with pytest.raises(pa.PhysError) as err:
        w.sync()
    assert err.value.code == -1 and "body edit" in str(err.value)
    w.sync()  # once: the next one is clean
    lin, _ = w.get_velocities()
    untouched = np.ones(65, bool)
    untouched[[2, 5]] = False
    assert _same(lin[untouched], b["vel"][untouched])
    inv_mass = (np.float32(1.0) / b["mass"]).astype(np.float32)
    assert _same(lin[2], b["vel"][2] + np.float32(1.0) * inv_mass[2])  # the entry in order was applied
    w.update(DT)  # and the world goes on
    w.sync()
    w.close()


@pytest.mark.parametrize("bad", [65, 0x7FFFFFFF, -1])
def test_device_id_out_of_range_is_skipped_and_reported(bad):
    import torch
    pa = _pa()
    b = _bodies(65, 6, "full")
    for kind in ("poses", "velocities", "impulses", "forces", "states"):
        w = _world(b)
        ids = torch.tensor([1, 3, 3, bad], dtype=torch.int32, device="cuda")  # -1 is 0xFFFFFFFF: the largest id, so the order holds
        v = torch.full((4, 3), 2.0, dtype=torch.float32, device="cuda")
        out = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        before = _state(w) + w.get_forces()
        if kind == "poses":
            w.set_body_poses_device(ids, pos=v)
        elif kind == "velocities":
            w.set_body_velocities_device(ids, lin=v)
        elif kind == "impulses":
            w.apply_impulses_device(ids, v)
        elif kind == "forces":
            w.apply_forces_device(ids, v)
        else:
            w.get_body_states_device(ids, pos_out=out)
        with pytest.raises(pa.PhysError) as err:
            w.sync()
        assert err.value.code == -1
        w.sync()
        after = _state(w) + w.get_forces()
        changed = {"poses": 0, "velocities": 2, "impulses": 2, "forces": 4}.get(kind)
        for k, (x, y) in enumerate(zip(before, after)):
            rest = np.ones(65, bool)
            rest[[1, 3]] = False
            assert _same(x[rest], y[rest])  # nothing outside the entries in range
            assert (k == changed) == bool((x[[1, 3]] != y[[1, 3]]).any()), (kind, k)
        if kind == "poses":
            assert _same(after[0][[1, 3]], np.full((2, 3), 2.0, np.float32))
        if kind == "states":
            got = out.cpu().numpy()
            assert _same(got[:3], b["pos"][[1, 3, 3]]) and not got[3].any()
        w.close()


def test_host_id_out_of_range_writes_nothing():
    pa = _pa()
    b = _bodies(65, 7, "diag")
    w = _world(b)
    before = _state(w) + w.get_forces()
    v = np.ones((3, 3), np.float32)
    calls = [lambda ids: w.set_body_poses(ids, pos=v), lambda ids: w.set_body_velocities(ids, ang=v), lambda ids: w.apply_impulses(ids, v),
             lambda ids: w.apply_forces(ids, v, point=v), lambda ids: w.get_body_states(ids)]
    for call in calls:
        with pytest.raises(pa.PhysError) as err:
            call([1, 65, 2])
        assert err.value.code == -6
    for call in calls[:4]:
        with pytest.raises(pa.PhysError) as err:
            v[1, 1] = np.nan
            call([1, 2, 3])
        assert err.value.code == -1
        v[1, 1] = np.inf
        with pytest.raises(pa.PhysError) as err:
            call([1, 2, 3])
        assert err.value.code == -1
        v[1, 1] = 1.0
    for x, y in zip(before, _state(w) + w.get_forces()):
        assert _same(x, y)
    w.sync()
    w.close()


# ---- 5. free flight: the edited world goes on as a world built afresh from its state ---------------------------------------------
@pytest.mark.parametrize("layout", ["shared", "diag", "full"])
def test_free_flight_equals_a_fresh_world(layout):
    nb = 65
    b = _bodies(nb, 500, layout)
    e = _entries(nb, 64, 501)
    w = _world(b)
    for _ in range(3):
        w.update(DT)
    w.set_body_poses(e["ids"][:20], pos=e["b"][:20], rot=b["rot"][e["ids"][:20]])
    w.set_body_velocities(e["ids"][20:40], lin=e["c"][20:40], ang=e["a"][20:40])
    w.apply_impulses(e["ids"], e["a"], point=e["b"], ang_impulse=e["c"])
    pos, rot, lin, ang = _state(w)
    fresh = _world(dict(b, pos=pos, rot=rot, vel=lin, ang=ang))
    for x in (w, fresh):
        x.apply_forces(e["ids"], e["c"], point=e["b"], torque=e["a"])
        for _ in range(3):
            x.update(DT)
    for x, y in zip(_state(w), _state(fresh)):
        assert _same(x, y)
    assert not _same(pos, w.get_transforms()[0])
    for x in (w, fresh):
        x.sync()
        x.close()


# ---- 6 - 8. the pile: history is kept, teleports, batches -----------------------------------------------------------------------
def _pile():
    from physics_amd import scenes
    return scenes.falling_cubes(4, 4, 4, "pile_4x4x4", spacing=2.0, y0=1.0, jitter=0.0)


def _pile_world(events=True, state=None, **cfg):
    pa = _pa()
    sc = _pile()
    w = pa.World(sc.config(**cfg))
    sc.populate(w, state)
    if events:
        w.enable_contact_events(1 << 14)
    return w


def test_history_is_kept_when_the_state_is_written_back():
    wa, wb = _pile_world(), _pile_world()
    for w in (wa, wb):
        w.update_n(DT, 10)
    sa, sb = _state(wa), _state(wb)
    assert all(_same(x, y) for x, y in zip(sa, sb))
    ids = np.random.default_rng(1).permutation(64).astype(np.uint32)
    wa.set_body_poses(ids, pos=sa[0][ids], rot=sa[1][ids])
    wa.set_body_velocities(ids, lin=sa[2][ids], ang=sa[3][ids])
    for w in (wa, wb):
        w.update_n(DT, 10)
    for x, y in zip(_state(wa), _state(wb)):
        assert _same(x, y)
    (ea, da), (eb, db) = wa.get_contact_events(), wb.get_contact_events()
    assert da == db == 0 and len(ea) > 0 and ea.tobytes() == eb.tobytes()
    ma, mb = wa.get_manifolds(), wb.get_manifolds()
    assert len(ma[0]) > 32 and _same(ma[0], mb[0])
    assert _same(wa.get_contact_impulses(), wb.get_contact_impulses())  # warm starting went on from the same records
    for w in (wa, wb):
        w.sync()
        w.close()


INNER = 1 + 4 * 1 + 16 * 1  # the cube at lattice (1, 1, 1)


def _manifolds_by_pair(w):
    ids, counts, normals, points = w.get_manifolds()
    valid = np.arange(4)[None, :, None] < counts[:, None, None]
    return ids, counts, normals, np.where(valid, points, 0)


def test_teleport_ends_old_contacts_and_enters_a_trigger():
    pa = _pa()
    w = _pile_world()
    w.update_n(DT, 10)
    pos, rot, lin, ang = _state(w)
    target = pos[INNER] + np.array([100.0, 0.0, 0.0], np.float32)
    w.set_triggers(pa.SHAPE_BOX, target[None], half_extent=[1.5, 1.5, 1.5])
    w.enable_trigger_events(256)
    w.update(DT)  # the occupancy before the teleport: nobody is out there
    assert len(w.get_trigger_events()[0]) == 0
    w.get_contact_events()  # drained: what follows is the teleport's
    ids_before = w.get_manifolds()[0]
    old = {tuple(p) for p in ids_before if INNER in p}
    assert len(old) >= 2
    pos = w.get_transforms()[0]
    target = pos[INNER] + np.array([100.0, 0.0, 0.0], np.float32)
    w.set_body_poses([INNER], pos=target[None])
    state = _state(w)
    assert _same(state[0][INNER], target)
    w.update(DT)
    ids, counts, normals, points = _manifolds_by_pair(w)
    mine = [tuple(p) for p in ids if INNER in p]
    assert all(p == (INNER, pa.GROUND_ID) for p in mine)  # nothing, or the ground where it landed
    fresh = _pile_world(events=False, state=state)
    fresh.update(DT)
    for x, y in zip((ids, counts, normals, points), _manifolds_by_pair(fresh)):
        assert _same(x, y)
    ev, dropped = w.get_contact_events()
    ended = {(int(r["body_a"]), int(r["body_b"])) for r in ev if r["kind"] == pa.CONTACT_END}
    assert dropped == 0 and old <= ended
    tev, _ = w.get_trigger_events()
    assert [(int(r["trigger"]), int(r["body"]), int(r["kind"])) for r in tev] == [(0, INNER, pa.TRIGGER_ENTER)]
    for x in (w, fresh):
        x.sync()
        x.close()


def test_broadphase_aabbs_and_ray_casts_see_the_new_pose_at_once():
    pa = _pa()
    w = _pile_world(events=False)
    w.update_n(DT, 10)
    pos = w.get_transforms()[0]
    assert any(INNER in p for p in w.broadphase())
    target = pos[INNER] + np.array([100.0, 0.0, 0.0], np.float32)
    w.set_body_poses([INNER], pos=target[None])
    pairs = w.broadphase()
    assert len(pairs) > 0 and not any(INNER in p for p in pairs)
    box = w.get_aabbs()[INNER]
    assert (box[:3] < target).all() and (target < box[3:]).all()
    above = np.array([target + [0, 50, 0], pos[INNER] + [0, 50, 0]], np.float32)
    body, t, _ = w.raycast(above, np.array([[0, -1, 0], [0, -1, 0]], np.float32))
    assert body[0] == INNER and abs(t[0] - 49.0) < 1e-2
    assert body[1] != INNER and body[1] != pa.RAY_MISS
    w.update(DT)  # and the update after the read-outs is sound
    w.sync()
    w.close()


def test_update_n_after_edits_equals_single_updates():
    wa, wb = _pile_world(), _pile_world()
    e = _entries(64, 65, 9)
    for w in (wa, wb):
        w.update_n(DT, 6)
        w.apply_impulses(e["ids"], e["a"], point=None, ang_impulse=e["c"])
        w.set_body_velocities([INNER], lin=[[0, 6, 0]])
        w.apply_forces(e["ids"], e["c"] * np.float32(20))
    wa.update_n(DT, 4)
    for _ in range(4):
        wb.update(DT)
    for x, y in zip(_state(wa), _state(wb)):
        assert _same(x, y)
    assert wa.get_contact_events()[0].tobytes() == wb.get_contact_events()[0].tobytes()
    for w in (wa, wb):
        w.sync()
        w.close()


def test_refusals_and_no_ops():
    pa = _pa()
    b = _bodies(8, 9, "diag")
    w = _world(b)
    before = _state(w) + w.get_forces()
    none3 = np.zeros((0, 3), np.float32)
    w.set_body_poses([], pos=none3)
    w.set_body_velocities([], lin=none3)
    w.apply_impulses([], none3)
    w.apply_forces([], none3)
    assert all(x.shape[0] == 0 for x in w.get_body_states([]))
    lib, v = w.lib, np.ones((3, 3), np.float32)
    fp = v.ctypes.data_as(C.POINTER(C.c_float))
    ids = np.arange(3, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.phys_apply_impulses(w.h, 0, None, None, None, None) == 0      # n = 0: a no-op whatever the pointers
    assert lib.phys_apply_impulses_device(w.h, 0, None, None, None, None) == 0
    assert lib.phys_set_body_poses(w.h, 3, None, fp, None) == -1             # null ids
    assert lib.phys_set_body_velocities(w.h, 3, None, fp, None) == -1
    assert lib.phys_apply_impulses(w.h, 3, None, fp, None, None) == -1
    assert lib.phys_apply_forces(w.h, 3, None, fp, None, None) == -1
    assert lib.phys_get_body_states(w.h, 3, None, fp, None, None, None) == -1
    assert lib.phys_apply_impulses(w.h, 3, ids, None, fp, None) == -1        # null impulse
    assert lib.phys_apply_forces(w.h, 3, ids, None, None, fp) == -1          # null force
    for name, extra in (("phys_set_body_poses_device", 2), ("phys_set_body_velocities_device", 2), ("phys_apply_impulses_device", 3),
                        ("phys_apply_forces_device", 3), ("phys_get_body_states_device", 4)):
        assert getattr(lib, name)(w.h, 3, None, *([None] * extra)) == -1
    for x, y in zip(before, _state(w) + w.get_forces()):
        assert _same(x, y)
    w.sync()
    w.close()
    # a sharded world refuses all ten
    g = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS, max_ghosts=8))
    g.set_bodies(b["pos"], shape_type=np.full(8, pa.SHAPE_BOX, np.uint32), half_extent=np.ones((8, 3), np.float32))
    for call in (lambda: g.set_body_poses([0], pos=v[:1]), lambda: g.set_body_velocities([0], lin=v[:1]), lambda: g.apply_impulses([0], v[:1]),
                 lambda: g.apply_forces([0], v[:1]), lambda: g.get_body_states([0])):
        with pytest.raises(pa.PhysError) as err:
            call()
        assert err.value.code == -7
    for name, extra in (("phys_set_body_poses_device", 2), ("phys_set_body_velocities_device", 2), ("phys_apply_impulses_device", 3),
                        ("phys_apply_forces_device", 3), ("phys_get_body_states_device", 4)):
        assert getattr(g.lib, name)(g.h, 1, None, *([None] * extra)) == -7
    g.close()
