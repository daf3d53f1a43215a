"""GPU: force fields (phys_set_force_fields, phys_apply_force_fields ...) against the library's own statement of their
arithmetic (tests/cpp/field_probe.cpp: include/spec/force_field.h compiled by the host compiler) bit for bit, against the float64
reference of tests/field_ref.py within a derived bound, and against themselves.

Either side of a wave and past a workgroup (1, 63, 64, 65, 257 bodies), a full LDS tile, one over and a tail (1, 32, 33, 70
fields); the update uses exactly the evaluation apply_force_fields gives; batches; a world without fields is untouched; masks;
poses, params and clearing; damping does what it is for; argument errors. Every scene has at most a few hundred bodies, but for
one collision scene of 10 000 cubes (scenes.c2), stepped five times."""
import ctypes as C
import functools

import numpy as np
import pytest

import field_probe as fp
import field_ref as fr

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(DT * 1e-9))


def _pa():
    import physics_amd
    return physics_amd


@functools.lru_cache(maxsize=None)
def _probe():
    import tempfile
    return fp.build(tempfile.mkdtemp(prefix="field_probe_") + "/field_probe")


def _set_fields(w, f, mask="own"):
    w.set_force_fields(f["kind"], f["shape"], f["pos"], rot=f.get("rot"), half_extent=f["half_extent"],
                       mask=f.get("mask") if isinstance(mask, str) else mask, vec=f["vec"], coef=f["coef"], exponent=f.get("exponent"))


def _world(bodies, flags=0, **cfg):
    pa = _pa()
    w = pa.World(pa.default_config(flags=flags, **cfg))
    w.set_bodies(bodies["pos"], rot=bodies.get("rot"), lin_vel=bodies.get("vel"), ang_vel=bodies.get("ang"), mass=bodies.get("mass"),
                 shape_type=bodies.get("shape"), half_extent=bodies.get("half_extent"))
    return w


def _hand_scene():
    """One body inside one rotated RADIAL box field (the hand scene of body count 1)."""
    bodies = dict(pos=np.array([[0.4, 1.1, -0.3]], np.float32), vel=np.array([[1, 2, 3]], np.float32), ang=np.array([[0.5, 0, -1]], np.float32),
                  mass=np.array([2.0], np.float32))
    fields = dict(kind=np.array([fr.RADIAL], np.uint32), shape=np.array([fr.BOX], np.uint32), pos=np.array([[0.1, 1.0, 0.2]], np.float32),
                  rot=np.array([[0, 0.19866933, 0, 0.98006658]], np.float32), half_extent=np.array([[1.5, 1.0, 1.2]], np.float32), mask=None,
                  vec=np.zeros((1, 3), np.float32), coef=np.array([[7.0, 0.25]], np.float32), exponent=np.array([2], np.uint32))
    return bodies, fields


@functools.lru_cache(maxsize=None)
def _evaluated(n_bodies, n_fields, start):
    """(gpu F, gpu T, probe acted, probe F, probe T, reference result) of the committed scene (n_bodies == 1: the hand scene)
    from zero (`start` False) or nonzero starting accumulators. Computed once per case and shared; nobody changes it."""
    import os
    bodies, fields = _hand_scene() if n_bodies == 1 else fr.scene(n_bodies, n_fields)
    n = len(bodies["pos"])
    acc = (np.random.default_rng(n_bodies * 1000 + n_fields).normal(size=(2, n, 3)) * 5).astype(np.float32) if start else (None, None)
    w = _world(bodies)
    _set_fields(w, fields)
    if start:
        w.set_forces(acc[0], acc[1])
    w.apply_force_fields()
    gf, gt = w.get_forces()
    w.sync()
    w.close()
    scene = os.path.join(os.path.dirname(_probe()), f"scene_{n_bodies}_{n_fields}_{int(start)}.txt")
    fp.write_scene(scene, fields, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"], force=acc[0], torque=acc[1])
    acted, pf, pt = fp.run(_probe(), scene)
    res = fr.evaluate(fields, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"], force=acc[0], torque=acc[1])
    return gf, gt, acted, pf, pt, res, acc


CASES = [(1, 1)] + [(nb, nf) for nb in (63, 64, 65, 257) for nf in (1, 32, 33, 70)]


# ---- 1. the kernel against the spec, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [False, True], ids=["zero", "nonzero"])
@pytest.mark.parametrize("n_bodies,n_fields", CASES)
def test_kernel_equals_the_spec_bit_for_bit(n_bodies, n_fields, start):
    gf, gt, acted, pf, pt, res, _ = _evaluated(n_bodies, n_fields, start)
    assert gf.tobytes() == pf.tobytes() and gt.tobytes() == pt.tobytes(), np.argwhere((gf != pf) | (gt != pt))[:8]
    if n_bodies == 1:
        assert acted[0] and np.abs(gf).max() > 0


# ---- 2. the maths against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [False, True], ids=["zero", "nonzero"])
@pytest.mark.parametrize("n_bodies,n_fields", CASES)
def test_forces_match_float64_within_the_derived_bound(n_bodies, n_fields, start):
    """Per body and component |gpu - float64| <= (16 + K) * 2^-23 * S, K the fields acting on the body and S the sum of the
    magnitudes of their contributions and of the starting accumulators; no exclusions. Bodies on which no field acts keep
    their accumulator bits."""
    gf, gt, _, _, _, res, acc = _evaluated(n_bodies, n_fields, start)
    assert res["margin"] > 1e-3
    tol = fr.bound(res)
    err = np.maximum(np.abs(gf - res["F"]), np.abs(gt - res["T"]))
    acting = res["K"] > 0
    if acting.any():
        print(f"({n_bodies}, {n_fields}, start={start}): {int(acting.sum())} bodies acted on, worst error / bound "
              f"{float((err[acting] / tol[acting]).max()):.3f}")
    assert (err <= tol).all(), np.argwhere(err > tol)[:8]
    n = len(gf)
    f0, t0 = (acc[0], acc[1]) if start else (np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32))
    assert gf[~acting].tobytes() == f0[~acting].tobytes() and gt[~acting].tobytes() == t0[~acting].tobytes()
    if n_fields >= 32:
        assert acting.any() and (~acting).any()


# ---- 3. the update uses exactly that evaluation -----------------------------------------------------------------------------------
def _state(w):
    return [a.tobytes() for a in (*w.get_transforms(), *w.get_velocities())]


def _scene_wide_fields(lo, hi):
    """A DRAG box over the whole scene with wind, an ACCEL sphere and a RADIAL attractor inside it."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    return dict(kind=np.array([fr.DRAG, fr.ACCEL, fr.RADIAL], np.uint32), shape=np.array([fr.BOX, fr.SPHERE, fr.CAPSULE], np.uint32),
                pos=np.array([c, c + h * [0.3, -0.2, 0.1], c - h * [0.2, 0.1, 0.3]], np.float32), rot=None,
                half_extent=np.array([h * 1.5 + 1, [h.max() * 0.7, 0, 0], [h.max() * 0.5, h.max() * 0.4, 0]], np.float32), mask=None,
                vec=np.array([[1.5, 0, -0.5], [0.7, 3.0, -0.4], [0, 0, 0]], np.float32),
                coef=np.array([[0.4, 0.2], [0, 0], [-6.0, 2.0]], np.float32), exponent=np.array([0, 0, 1], np.uint32))


def _follow_twins(a, b, updates, extra=lambda w: []):
    """World a has fields. World b has none: before each update it gets a's apply_force_fields result through set_forces.
    Bit-identical transforms and velocities (and `extra`) after every update."""
    n = a.n
    zero = np.zeros((n, 3), np.float32)
    acted = 0
    for u in range(updates):
        a.apply_force_fields()
        f, t = a.get_forces()
        acted += int((f != 0).any(1).sum())
        a.set_forces(zero, zero)  # the update makes the same evaluation again, from the same zeros
        b.set_forces(f, t)
        a.update(DT)
        b.update(DT)
        assert _state(a) == _state(b), f"update {u}"
        assert [x.tobytes() for x in extra(a)] == [x.tobytes() for x in extra(b)], f"update {u}"
    a.sync()
    b.sync()
    return acted


def test_update_equals_explicit_forces_without_collisions():
    bodies, _ = fr.scene(257, 1)
    fields = _scene_wide_fields([-8, -8, -8], [8, 8, 8])
    a, b = _world(bodies), _world(bodies)
    _set_fields(a, fields)
    assert _follow_twins(a, b, 5) >= 5 * 257
    a.close(), b.close()


def test_update_equals_explicit_forces_in_the_c2_collision_scene():
    pa = _pa()
    from physics_amd import scenes
    sc = scenes.c2()
    w0 = pa.World(sc.config())
    sc.populate(w0)
    w0.update_n(DT, 30)  # the lowest layer has landed: the five updates below solve contacts
    state = (*w0.get_transforms(), *w0.get_velocities())
    w0.sync()
    w0.close()
    a, b = pa.World(sc.config()), pa.World(sc.config())
    for w in (a, b):
        sc.populate(w, state=state)
    _set_fields(a, _scene_wide_fields(sc.pos.min(0), sc.pos.max(0)))
    assert _follow_twins(a, b, 5) >= 5 * sc.n
    assert a.get_stats().n_manifolds > 0 and a.get_stats().n_manifolds == b.get_stats().n_manifolds
    a.close(), b.close()


def test_update_equals_explicit_forces_with_a_pinned_body():
    """Body 0 pinned by a fix-point constraint: its right-hand side reads the accumulators, so the pinned body feels the wind,
    and the constraint's lambda is the same bits too."""
    bodies, _ = fr.scene(65, 1)
    fields = _scene_wide_fields([-8, -8, -8], [8, 8, 8])
    a, b = _world(bodies), _world(bodies)
    for w in (a, b):
        w.add_constraint_fix_point(0, bodies["pos"][0])
    _set_fields(a, fields)
    _follow_twins(a, b, 5, extra=lambda w: [w.get_lambda()])
    assert len(a.get_lambda()) == 3 and np.abs(a.get_lambda()).max() > 0
    # ... and it is the fields that lambda answers to: without them it differs
    c = _world(bodies)
    c.add_constraint_fix_point(0, bodies["pos"][0])
    c.update_n(DT, 5)
    assert c.get_lambda().tobytes() != a.get_lambda().tobytes()
    a.close(), b.close(), c.close()


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collide", [False, True])
def test_batches_equal_single_updates_and_runs_repeat(collide):
    pa = _pa()
    bodies, fields = fr.scene(257, 70)
    assert (fields["kind"] == fr.DRAG).any()  # velocities change between the steps of a batch
    flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE if collide else 0
    out = []
    for mode in ("batch", "single", "batch"):
        w = _world(bodies, flags=flags, ground_height=-9.0)
        _set_fields(w, fields)
        if mode == "batch":
            w.update_n(DT, 3)
        else:
            for _ in range(3):
                w.update(DT)
        out.append(_state(w))
        w.sync()
        w.close()
    assert out[0] == out[1] and out[0] == out[2]
    w = _world(bodies, flags=flags, ground_height=-9.0)  # and the fields did something
    w.update_n(DT, 3)
    assert _state(w) != out[0]
    w.close()


# ---- 5. a world without fields is untouched -----------------------------------------------------------------------------------
@pytest.mark.parametrize("collide", [False, True])
def test_world_without_fields_launches_and_computes_what_it_did(collide):
    pa = _pa()
    bodies, fields = fr.scene(257, 33)
    flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE if collide else 0

    def run(prepare):
        w = _world(bodies, flags=flags, ground_height=-9.0)
        prepare(w)
        w.profile_enable(True)
        w.update_n(DT, 2)
        for _ in range(3):
            w.update(DT)
        prof, steps = w.profile_get()
        st = _state(w)
        w.sync()
        w.close()
        return {k: v[1] for k, v in prof.items()}, steps, st

    def cleared(w):
        _set_fields(w, fields)
        w.apply_force_fields()  # the fields act once ...
        w.set_force_fields(fr.ACCEL, fr.BOX, np.zeros((0, 3), np.float32))  # ... n = 0 clears the set
        w.set_bodies(bodies["pos"], rot=bodies["rot"], lin_vel=bodies["vel"], ang_vel=bodies["ang"], mass=bodies["mass"],
                     shape_type=bodies["shape"], half_extent=bodies["half_extent"])

    def nobody(w):
        w.set_body_filters(category=1)
        _set_fields(w, fields, mask=0xFFFE)

    never = run(lambda w: None)
    assert never[1] == 5
    if not collide:
        assert never[0] == {"step_full": 5}, never[0]  # what a world launched before fields existed: one per update
    after_clear = run(cleared)
    assert after_clear[0] == never[0] and after_clear[2] == never[2]
    with_fields = run(lambda w: _set_fields(w, fields))
    if not collide:  # (with contacts the fields change what collides, and with it the colouring's launches)
        assert with_fields[0] == {"step_full": 5, "misc": 5}, with_fields[0]  # one launch per update, counted under MISC
    assert with_fields[2] != never[2]
    masked_out = run(nobody)
    assert masked_out[2] == never[2]  # a set whose masks match no body leaves every bit unchanged


# ---- 6. masks and filters -----------------------------------------------------------------------------------------------------
def test_masks_pick_exactly_the_reference_pairs():
    """Body categories and field masks: the (field, body) set, read one field at a time as unit ACCEL fields on unit masses, is
    the reference's; and the whole masked set equals the spec bit for bit."""
    import os
    bodies, fields = fr.scene(257, 33)
    rng = np.random.default_rng(5)
    cat = (1 << rng.integers(0, 4, 257)).astype(np.uint16)
    fields["mask"] = rng.integers(0, 16, 33).astype(np.uint16)
    want = fr.evaluate(fields, bodies["pos"], category=cat)["pairs"]
    unmasked = fr.evaluate(dict(fields, mask=None), bodies["pos"])["pairs"]
    assert 0 < len(want) < len(unmasked)
    w = _world(dict(bodies, mass=None))
    w.set_body_filters(category=cat)
    got = set()
    for k in range(33):
        w.set_force_fields(fr.ACCEL, fields["shape"][k:k + 1], fields["pos"][k:k + 1], rot=fields["rot"][k:k + 1],
                           half_extent=fields["half_extent"][k:k + 1], mask=fields["mask"][k:k + 1], vec=[1.0, 0, 0], coef=[0, 0])
        w.set_forces(np.zeros((257, 3), np.float32), np.zeros((257, 3), np.float32))
        w.apply_force_fields()
        f, _ = w.get_forces()
        assert np.isin(f[:, 0], (0.0, 1.0)).all()
        got |= {(k, int(i)) for i in np.nonzero(f[:, 0])[0]}
    assert got == want
    w.close()
    w = _world(bodies)
    w.set_body_filters(category=cat)
    _set_fields(w, fields)
    w.apply_force_fields()
    gf, gt = w.get_forces()
    w.close()
    scene = os.path.join(os.path.dirname(_probe()), "scene_masked.txt")
    fp.write_scene(scene, fields, bodies["pos"], bodies["vel"], bodies["ang"], bodies["mass"], category=cat)
    _, pf, pt = fp.run(_probe(), scene)
    assert gf.tobytes() == pf.tobytes() and gt.tobytes() == pt.tobytes()


# ---- 7. poses, params, clearing -------------------------------------------------------------------------------------------------
def test_poses_params_and_set_bodies():
    pa = _pa()
    pos = np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]], np.float32)
    mass = np.array([2.0, 1.0], np.float32)
    cfg = dict(gravity_force=(0.0, 0.0, 0.0), gravity_offset=(0.0, 0.0, 0.0))
    w = _world(dict(pos=pos, mass=mass), **cfg)
    vec = np.array([[3.0, 0.0, -6.0]], np.float32)
    w.set_force_fields(fr.ACCEL, fr.SPHERE, [[10.0, 0.0, 0.0]], half_extent=[1.0, 0, 0], vec=vec, coef=[0, 0])
    w.update(DT)
    assert not np.any(w.get_velocities()[0])  # nobody inside
    w.set_force_field_poses([[0.2, 0.0, 0.0]])
    w.update(DT)
    v = w.get_velocities()[0]
    dt = np.float32(DT * 1e-9)
    assert v[0].tobytes() == (np.float32(2.0) * vec[0] / np.float32(2.0) * dt).tobytes() and not np.any(v[1])  # F = m * vec; v = 0 + F / m * dt
    w.set_force_field_poses([[20.5, 0.0, 0.0]], rot=[[0, 0, 0, 1]])  # ... and the body it left keeps its velocity
    w.update(DT)
    v2 = w.get_velocities()[0]
    assert v2[0].tobytes() == v[0].tobytes() and v2[1].tobytes() == (vec[0] * dt).tobytes()
    # set_bodies keeps the set
    w.set_bodies(pos, mass=mass)
    w.apply_force_fields()
    f, _ = w.get_forces()
    assert not np.any(f[0]) and f[1].tobytes() == vec[0].tobytes()
    w.close()
    # strength 0 through set_force_field_params: the bits of a world without fields
    bodies, fields = fr.scene(65, 33)
    a, b = _world(bodies), _world(bodies)
    _set_fields(a, fields)
    coef0 = fields["coef"].copy()
    coef0[:, 0] = 0
    coef0[fields["kind"] == fr.DRAG, 1] = 0
    a.set_force_field_params(np.zeros((33, 3), np.float32), coef0)
    a.apply_force_fields()
    assert not np.any(a.get_forces()[0]) and not np.any(a.get_forces()[1])
    a.update_n(DT, 5), b.update_n(DT, 5)
    assert _state(a) == _state(b)
    a.set_force_field_params(fields["vec"], fields["coef"])  # ... and switched on again they act
    a.update(DT), b.update(DT)
    assert _state(a) != _state(b)
    a.close(), b.close()


# ---- 8. damping does what it is for -------------------------------------------------------------------------------------------
def test_a_rolling_sphere_comes_to_rest_only_with_a_drag_field():
    pa = _pa()
    r, v0 = 0.5, 2.0
    body = dict(pos=np.array([[0.0, r, 0.0]], np.float32), vel=np.array([[v0, 0, 0]], np.float32), ang=np.array([[0, 0, -v0 / r]], np.float32),
                shape=np.array([pa.SHAPE_SPHERE], np.uint32), half_extent=np.array([[r, 0, 0]], np.float32))
    runs = {}
    for drag in (True, False):
        w = _world(body, flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0))
        if drag:  # unit mass and unit inertia: both decay at the same rate, the sphere keeps rolling
            w.set_force_fields(fr.DRAG, fr.BOX, [[0.0, 0.0, 0.0]], half_extent=[1000.0, 1000.0, 1000.0], coef=[0.5, 0.5])
        speed, spin = [v0], [v0 / r]
        for _ in range(120):
            w.update(DT)
            lin, ang = w.get_velocities()
            speed.append(float(np.linalg.norm(lin[0, [0, 2]])))
            spin.append(float(np.linalg.norm(ang[0])))
        w.sync()
        w.close()
        runs[drag] = (np.array(speed), np.array(spin))
    print(f"drag: speed {runs[True][0][-1]:.4f} spin {runs[True][1][-1]:.4f}; none: speed {runs[False][0][-1]:.4f} spin {runs[False][1][-1]:.4f}")
    assert (np.diff(runs[True][0]) < 0).all() and (np.diff(runs[True][1]) < 0).all()
    assert runs[True][0][-1] < 0.5 * v0 and runs[True][1][-1] < 0.5 * v0 / r  # exp(-0.5 * 2 s) = 0.37
    # without the field nothing takes energy out of a sphere that rolls without slipping: both are kept. (10 % is left to the
    # contact solver, which is not what this test is about; the drag's closed form is 37 %.)
    assert abs(runs[False][0][-1] - v0) < 0.1 * v0 and abs(runs[False][1][-1] - v0 / r) < 0.1 * v0 / r


def test_free_flight_in_a_wind_approaches_the_wind_velocity():
    """v after each update against the closed form v + (-c (v - w) / m) * dt from the velocity before it, within the bound of
    test 2 with one contribution: 17 * 2^-23 * (|v| + |c (v - w) / m * dt|)."""
    c, m = 1.5, 2.0
    wind = np.array([4.0, -1.0, 2.5])
    body = dict(pos=np.array([[0.0, 0.0, 0.0]], np.float32), vel=np.array([[-3.0, 6.0, 0.5]], np.float32), mass=np.array([m], np.float32))
    w = _world(body, gravity_force=(0.0, 0.0, 0.0), gravity_offset=(0.0, 0.0, 0.0))
    w.set_force_fields(fr.DRAG, fr.SPHERE, [[0.0, 0.0, 0.0]], half_extent=[1000.0, 0, 0], vec=wind, coef=[c, 0.0])
    v = body["vel"][0].astype(np.float64)
    gap = [np.linalg.norm(v - wind)]
    for u in range(240):
        w.update(DT)
        got = w.get_velocities()[0][0].astype(np.float64)
        step = -c * (v - wind) / m * DT_S
        tol = 17 * 2.0 ** -23 * (np.linalg.norm(v) + np.linalg.norm(step))
        assert (np.abs(got - (v + step)) <= tol).all(), (u, got, v + step, tol)
        v = got
        gap.append(np.linalg.norm(v - wind))
    w.close()
    assert (np.diff(gap) < 0).all() and gap[-1] < 0.06 * gap[0]  # exp(-0.75 * 4 s) = 0.05


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    pa = _pa()
    from physics_amd import _abi
    E, U = _abi.PHYS_ERR_INVALID_ARG, _abi.PHYS_ERR_UNSUPPORTED
    w = _world(dict(pos=np.zeros((4, 3), np.float32)))
    lib = w.lib
    f32, u32 = C.c_float, C.c_uint32

    def arrays(n):
        return dict(kind=(u32 * n)(*([2] * n)), shape=(u32 * n)(*([1] * n)), pos=(f32 * (3 * n))(), rot=(f32 * (4 * n))(*([0, 0, 0, 1] * n)),
                    he=(f32 * (3 * n))(*([1.0] * (3 * n))), mask=None, vec=(f32 * (3 * n))(), coef=(f32 * (2 * n))(*([1.0, 1.0] * n)),
                    ex=(u32 * n)())

    def call(a, n, handle=None):
        rc = lib.phys_set_force_fields(handle or w.h, n, a["kind"], a["shape"], a["pos"], a["rot"], a["he"], a["mask"], a["vec"], a["coef"], a["ex"])
        return rc, lib.phys_last_error().decode()

    assert call(arrays(3), 3)[0] == 0
    cases = [("kind", 1, 5, "force field 1: kind is neither ACCEL nor DRAG nor RADIAL"), ("shape", 2, 0, "force field 2: shape is neither SPHERE nor BOX nor CAPSULE"),
             ("pos", 4, float("nan"), "force field 1: non-finite number"), ("rot", 0, float("inf"), "force field 0: non-finite number"),
             ("vec", 8, float("nan"), "force field 2: non-finite number"), ("coef", 0, float("-inf"), "force field 0: non-finite number"),
             ("he", 3, -0.5, "force field 1: negative half extent"), ("coef", 5, 0.0, "force field 2: r0 (coef[1]) must be above 0"),
             ("coef", 5, -1.0, "force field 2: r0 (coef[1]) must be above 0"), ("ex", 1, 3, "force field 1: exponent above 2")]
    for name, index, value, message in cases:
        a = arrays(3)
        a[name][index] = value
        assert call(a, 3) == (E, message)
    a = arrays(3)
    a["kind"][1] = 1
    a["coef"][2] = -0.25
    assert call(a, 3) == (E, "force field 1: negative drag coefficient")
    a["coef"][2], a["coef"][3] = 0.25, -0.25
    assert call(a, 3) == (E, "force field 1: negative drag coefficient")
    for name in ("kind", "shape", "pos", "he", "vec", "coef"):
        a = arrays(3)
        a[name] = None
        assert call(a, 3) == (E, "force fields need kind, shape_type, pos, half_extent, vec and coef")
    assert call(arrays(1025), 1025) == (E, "phys_set_force_fields: more than PHYS_MAX_FORCE_FIELDS force fields")
    assert call(arrays(1024), 1024)[0] == 0  # the most a world keeps
    w.apply_force_fields()
    assert call(arrays(3), 3)[0] == 0  # (a refused call left the set as it was; this one replaces it)
    # count mismatches and bad values in the poses / params calls
    p2, p3 = (f32 * 6)(), (f32 * 9)()
    c3 = (f32 * 6)(*([1.0, 1.0] * 3))
    assert lib.phys_set_force_field_poses(w.h, 2, p2, None) == E and "n must equal the force field count" in lib.phys_last_error().decode()
    assert lib.phys_set_force_field_params(w.h, 4, p3, c3) == E and "n must equal the force field count" in lib.phys_last_error().decode()
    assert lib.phys_set_force_field_poses(w.h, 3, None, None) == E
    assert lib.phys_set_force_field_params(w.h, 3, p3, None) == E and lib.phys_set_force_field_params(w.h, 3, None, c3) == E
    p3[4] = float("nan")
    assert lib.phys_set_force_field_poses(w.h, 3, p3, None) == E and "non-finite" in lib.phys_last_error().decode()
    assert lib.phys_set_force_field_params(w.h, 3, p3, c3) == E and lib.phys_last_error().decode() == "force field 1: non-finite number"
    p3[4] = 0.0
    c3[3] = 0.0
    assert lib.phys_set_force_field_params(w.h, 3, p3, c3) == E and lib.phys_last_error().decode() == "force field 1: r0 (coef[1]) must be above 0"
    c3[3] = 1.0
    assert lib.phys_set_force_field_poses(w.h, 3, p3, None) == 0 and lib.phys_set_force_field_params(w.h, 3, p3, c3) == 0
    w.sync()
    w.close()
    # sharded worlds: all four calls
    g = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0, 0, 0), max_ghosts=8))
    g.set_bodies(np.zeros((2, 3), np.float32) + [[0, 5, 0], [3, 5, 0]], shape_type=np.full(2, pa.SHAPE_BOX, np.uint32), half_extent=np.ones((2, 3), np.float32))
    assert call(arrays(3), 3, handle=g.h)[0] == U and "max_ghosts" in lib.phys_last_error().decode()
    assert lib.phys_set_force_field_poses(g.h, 0, None, None) == U and lib.phys_set_force_field_params(g.h, 0, None, None) == U
    assert lib.phys_apply_force_fields(g.h) == U
    with pytest.raises(pa.PhysError) as e:
        g.apply_force_fields()
    assert e.value.code == U
    g.close()
