"""GPU: liquids (phys_set_liquids, phys_apply_liquids, phys_get_submersion ...) against the library's own statement of their
arithmetic (tests/cpp/liquid_probe.cpp: include/spec/liquid.h compiled by the host compiler) bit for bit, against the float64
reference of tests/liquid_ref.py within the bounds tests/test_liquid_cpu.py measured, and against themselves.

Either side of a wave and past a workgroup (1, 63, 64, 65, 257 bodies), a full LDS tile, one over and a tail (1, 32, 33, 40
liquids); fields first, then liquids; the read-out; the update uses exactly the evaluation apply_liquids gives; batches; a world
without liquids is untouched; poses, params and set_bodies; bodies float at the water line their weight implies and lie flat,
or sink to the floor; argument errors. Every scene has at most a few hundred bodies, but for one collision scene of 10 000 cubes
(scenes.c2), stepped five times."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import field_probe as fp
import field_ref as fr
import liquid_probe as lp
import liquid_ref as lr
from test_liquid_cpu import C_CAPSULE, C_SPHERE_BOX, EPS, bound

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(DT * 1e-9))


def _pa():
    import physics_amd
    return physics_amd


@functools.lru_cache(maxsize=None)
def _probe():
    import tempfile
    return lp.build(tempfile.mkdtemp(prefix="liquid_probe_") + "/liquid_probe")


@functools.lru_cache(maxsize=None)
def _field_probe():
    import tempfile
    return fp.build(tempfile.mkdtemp(prefix="field_probe_") + "/field_probe")


def _set_liquids(w, lq, mask="own", drag="own"):
    w.set_liquids(lq["pos"], rot=lq.get("rot"), half_extent=lq["half_extent"], mask=lq.get("mask") if isinstance(mask, str) else mask,
                  density=lq["density"], gravity=lq["gravity"], flow=lq["flow"], drag=lq["drag"] if isinstance(drag, str) else drag)


def _world(bodies, flags=0, **cfg):
    pa = _pa()
    w = pa.World(pa.default_config(flags=flags, **cfg))
    w.set_bodies(bodies["pos"], rot=bodies.get("rot"), lin_vel=bodies.get("vel"), ang_vel=bodies.get("ang"), mass=bodies.get("mass"),
                 shape_type=bodies.get("shape"), half_extent=bodies.get("half_extent"))
    return w


def _scene(n_bodies, n_liquids):
    """The committed scene; n_bodies == 1: one turned box whose centre is on liquid 0's surface, over the middle of its pool."""
    bodies, liquids = lr.scene(max(n_bodies, 2), n_liquids)
    if n_bodies == 1:
        n = lr.rot_matrix(liquids["rot"][0])[:, 1]
        x = (liquids["pos"][0].astype(np.float64) + float(liquids["half_extent"][0][1]) * n).astype(np.float32)
        bodies = dict(pos=x[None], rot=np.array([[0.18, -0.37, 0.09, 0.9063]], np.float32), vel=np.array([[1, -2, 3]], np.float32),
                      ang=np.array([[0.5, 0, -1]], np.float32), shape=np.array([lr.BOX], np.uint32), half_extent=np.array([[0.4, 0.2, 0.3]], np.float32))
    return bodies, liquids


@functools.lru_cache(maxsize=None)
def _evaluated(n_bodies, n_liquids, start, masked=False, drag=True):
    """(gpu F, T, frac, liquid, device frac, device liquid, forces after the read-out; probe acted, F, T, frac, liquid; acc) of the
    committed scene from zero (`start` False) or nonzero accumulators. Computed once per case and shared; nobody changes it."""
    import torch
    bodies, liquids = _scene(n_bodies, n_liquids)
    n = len(bodies["pos"])
    rng = np.random.default_rng(n_bodies * 1000 + n_liquids)
    acc = (rng.normal(size=(2, n, 3)) * 5).astype(np.float32) if start else (None, None)
    cat = (1 << rng.integers(0, 4, n)).astype(np.uint16) if masked else None
    lq = dict(liquids, mask=rng.integers(1, 16, n_liquids).astype(np.uint16) if masked else None,
              drag=liquids["drag"] if drag else np.zeros_like(liquids["drag"]))
    w = _world(bodies)
    if masked:
        w.set_body_filters(category=cat)
    _set_liquids(w, lq)
    if start:
        w.set_forces(acc[0], acc[1])
    before = w.get_forces()
    frac, liquid = w.get_submersion()
    d_frac = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    d_liquid = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    w.get_submersion_device(d_frac, d_liquid)
    w.sync()
    after = w.get_forces()
    w.apply_liquids()
    gf, gt = w.get_forces()
    w.sync()
    w.close()
    untouched = all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    probe = lp.evaluate(_probe(), os.path.dirname(_probe()), lq, bodies, category=cat, force=acc[0], torque=acc[1])
    return (gf, gt, frac, liquid, d_frac.cpu().numpy(), d_liquid.cpu().numpy().view(np.uint32), untouched), probe, (lq, bodies, cat, acc)


CASES = [(nb, nl) for nb in (1, 63, 64, 65, 257) for nl in (1, 32, 33, 40)]


# ---- 1. the kernels against the spec, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("start", [False, True], ids=["zero", "nonzero"])
@pytest.mark.parametrize("n_bodies,n_liquids", CASES)
def test_kernel_equals_the_spec_bit_for_bit(n_bodies, n_liquids, start):
    (gf, gt, *_), (acted, pf, pt, _, _), _ = _evaluated(n_bodies, n_liquids, start)
    assert gf.tobytes() == pf.tobytes() and gt.tobytes() == pt.tobytes(), np.argwhere((gf != pf) | (gt != pt))[:8]
    if n_bodies == 1:
        assert acted[0] and np.abs(gf).max() > 0 and np.abs(gt).max() > 0
    if n_bodies == 257 and n_liquids >= 32:
        assert acted.any() and (~acted).any()


@pytest.mark.parametrize("masked,drag", [(True, True), (False, False), (True, False)], ids=["masked", "no drag", "masked, no drag"])
@pytest.mark.parametrize("n_bodies,n_liquids", [(65, 33), (257, 40)])
def test_every_instance_equals_the_spec_bit_for_bit(n_bodies, n_liquids, masked, drag):
    (gf, gt, frac, liquid, *_), (acted, pf, pt, pfrac, pliquid), _ = _evaluated(n_bodies, n_liquids, True, masked, drag)
    assert gf.tobytes() == pf.tobytes() and gt.tobytes() == pt.tobytes()
    assert frac.tobytes() == pfrac.tobytes() and liquid.tobytes() == pliquid.tobytes()
    plain = _evaluated(n_bodies, n_liquids, True)[1]
    assert acted.sum() < plain[0].sum() if masked else pf.tobytes() != plain[1].tobytes()


@pytest.mark.parametrize("n_bodies,n_liquids", CASES)
def test_submersion_read_out_equals_the_spec_and_leaves_the_accumulators(n_bodies, n_liquids):
    (_, _, frac, liquid, d_frac, d_liquid, untouched), (acted, _, _, pfrac, pliquid), _ = _evaluated(n_bodies, n_liquids, True)
    assert frac.tobytes() == pfrac.tobytes() and liquid.tobytes() == pliquid.tobytes()
    assert d_frac.tobytes() == pfrac.tobytes() and d_liquid.tobytes() == pliquid.tobytes()
    assert untouched
    assert ((liquid == lr.NO_LIQUID) == ~acted).all() and (frac[~acted] == 0).all() and (frac[acted] > 0).all() and frac.max() <= 1.0


def test_forces_match_float64_within_the_measured_bound():
    """The GPU's bits are the probe's, and the probe is held to float64 on the CPU; here the GPU's own numbers once more, on the
    largest case: C * 2^-23 * S (S * b for torques), no exclusions."""
    (gf, gt, frac, liquid, *_), _, (lq, bodies, cat, acc) = _evaluated(257, 40, True)
    res = lr.evaluate(lq, bodies, category=cat, force=acc[0], torque=acc[1])
    assert res["margin"] > 1e-3
    tol_f, tol_t = bound(res, bodies["shape"], acc[0], acc[1])
    assert (np.abs(gf - res["F"]) <= tol_f).all() and (np.abs(gt - res["T"]) <= tol_t).all()
    assert (liquid == res["liquid"]).all() and np.abs(frac - res["frac"]).max() <= 64 * EPS


def test_fields_first_then_liquids():
    """A world with a field set and a liquid set: apply_force_fields then apply_liquids, and one update's own order, give the
    bits of the two probes chained - the fields' result is the liquids' starting accumulator."""
    bodies, liquids = lr.scene(257, 33)
    _, fields = fr.scene(257, 33)
    mass = np.random.default_rng(7007).uniform(0.5, 3.0, 257).astype(np.float32)
    w = _world(dict(bodies, mass=mass))
    w.set_force_fields(fields["kind"], fields["shape"], fields["pos"], rot=fields["rot"], half_extent=fields["half_extent"], vec=fields["vec"],
                       coef=fields["coef"], exponent=fields["exponent"])
    _set_liquids(w, liquids)
    w.apply_force_fields()
    w.apply_liquids()
    gf, gt = w.get_forces()
    w.close()
    scene = os.path.join(os.path.dirname(_field_probe()), "scene_chain.txt")
    fp.write_scene(scene, fields, bodies["pos"], bodies["vel"], bodies["ang"], mass)
    facted, ff, ft = fp.run(_field_probe(), scene)
    lacted, pf, pt, _, _ = lp.evaluate(_probe(), os.path.dirname(_probe()), liquids, bodies, force=ff, torque=ft)
    assert (facted & lacted).sum() > 10
    assert gf.tobytes() == pf.tobytes() and gt.tobytes() == pt.tobytes()


# ---- 2. the update uses exactly that evaluation ------------------------------------------------------------------------------
def _state(w):
    return [a.tobytes() for a in (*w.get_transforms(), *w.get_velocities())]


def _ocean(lo, hi, level):
    """One scene-wide liquid with flow and drag whose surface is the plane y = level, and a denser tilted pool inside it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2 + 2.0
    bottom = lo[1] - 2.0
    return dict(pos=np.array([[c[0], (level + bottom) / 2, c[2]], [c[0] + 0.3, level - 1.0, c[2] - 0.2]], np.float32),
                rot=np.array([[0, 0, 0, 1], [0.06, 0, -0.08, 0.995]], np.float32),
                half_extent=np.array([[h[0], (level - bottom) / 2, h[2]], [h[0] * 0.5, 2.0, h[2] * 0.5]], np.float32), mask=None,
                density=np.array([1.4, 3.0], np.float32), gravity=np.array([[0, -9.81, 0], [0.3, -9.0, 0.2]], np.float32),
                flow=np.array([[0.5, 0, -0.25], [0, 0, 0]], np.float32), drag=np.array([[0.3, 0.2], [0.6, 0.1]], np.float32))


def _follow_twins(a, b, updates, extra=lambda w: []):
    """World a has liquids. World b has none: before each update it gets a's apply_liquids result through set_forces.
    Bit-identical transforms and velocities (and `extra`) after every update."""
    zero = np.zeros((a.n, 3), np.float32)
    acted = 0
    for u in range(updates):
        a.apply_liquids()
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
    bodies, _ = lr.scene(257, 1)
    a, b = _world(bodies), _world(bodies)
    _set_liquids(a, _ocean([-8, -8, -8], [8, 8, 8], 1.0))
    assert _follow_twins(a, b, 5) >= 5 * 100
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
    lo, hi = state[0].min(0), state[0].max(0)
    _set_liquids(a, _ocean(lo, hi, float((lo[1] + hi[1]) / 2)))
    assert _follow_twins(a, b, 5) >= 5 * sc.n // 3
    assert a.get_stats().n_manifolds > 0 and a.get_stats().n_manifolds == b.get_stats().n_manifolds
    a.close(), b.close()


def test_update_equals_explicit_forces_with_a_pinned_body():
    """Body 0 pinned by a fix-point constraint under water: its right-hand side reads the accumulators, so the pinned body feels
    the buoyancy, and the constraint's lambda is the same bits too."""
    bodies, _ = lr.scene(65, 1)
    bodies = dict(bodies, shape=bodies["shape"].copy())
    bodies["shape"][0] = lr.BOX
    a, b = _world(bodies), _world(bodies)
    for w in (a, b):
        w.add_constraint_fix_point(0, bodies["pos"][0])
    _set_liquids(a, _ocean([-8, -8, -8], [8, 8, 8], 7.5))
    _follow_twins(a, b, 5, extra=lambda w: [w.get_lambda()])
    assert len(a.get_lambda()) == 3 and np.abs(a.get_lambda()).max() > 0
    c = _world(bodies)  # ... and it is the liquids that lambda answers to: without them it differs
    c.add_constraint_fix_point(0, bodies["pos"][0])
    c.update_n(DT, 5)
    assert c.get_lambda().tobytes() != a.get_lambda().tobytes()
    a.close(), b.close(), c.close()


# ---- 3. batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collide", [False, True])
def test_batches_equal_single_updates_and_runs_repeat(collide):
    pa = _pa()
    bodies, liquids = lr.scene(257, 40)
    assert (liquids["drag"] > 0).any()  # velocities change between the steps of a batch
    flags = pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE if collide else 0
    out = []
    for mode in ("batch", "single", "batch"):
        w = _world(bodies, flags=flags, ground_height=-9.0)
        _set_liquids(w, liquids)
        if mode == "batch":
            w.update_n(DT, 3)
        else:
            for _ in range(3):
                w.update(DT)
        out.append(_state(w))
        w.sync()
        w.close()
    assert out[0] == out[1] and out[0] == out[2]
    w = _world(bodies, flags=flags, ground_height=-9.0)  # and the liquids did something
    w.update_n(DT, 3)
    assert _state(w) != out[0]
    w.close()


# ---- 4. a world without liquids is untouched ---------------------------------------------------------------------------------
@pytest.mark.parametrize("collide", [False, True])
def test_world_without_liquids_launches_and_computes_what_it_did(collide):
    """The suite keeps no recorded state of an earlier build, so the three worlds are held to each other: one that never set
    liquids, one that set and cleared them, one whose masks match no body; and to the launch counts of a plain world."""
    pa = _pa()
    bodies, liquids = lr.scene(257, 33)
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
        _set_liquids(w, liquids)
        w.apply_liquids()  # the liquids act once ...
        w.set_liquids(np.zeros((0, 3), np.float32))  # ... n = 0 clears the set
        w.set_bodies(bodies["pos"], rot=bodies["rot"], lin_vel=bodies["vel"], ang_vel=bodies["ang"], shape_type=bodies["shape"],
                     half_extent=bodies["half_extent"])

    def nobody(w):
        w.set_body_filters(category=1)
        _set_liquids(w, liquids, mask=0xFFFE)

    never = run(lambda w: None)
    assert never[1] == 5
    if not collide:
        assert never[0] == {"step_full": 5}, never[0]  # what a world launched before liquids existed: one per update
    after_clear = run(cleared)
    assert after_clear[0] == never[0] and after_clear[2] == never[2]
    with_liquids = run(lambda w: _set_liquids(w, liquids))
    if not collide:  # (with contacts the liquids change what collides, and with it the colouring's launches)
        assert with_liquids[0] == {"step_full": 5, "misc": 5}, with_liquids[0]  # one launch per update, counted under MISC
    assert with_liquids[2] != never[2]
    assert run(nobody)[2] == never[2]  # a set whose masks match no body leaves every bit unchanged


# ---- 5. poses, params, set_bodies ---------------------------------------------------------------------------------------------
def test_poses_params_and_set_bodies():
    pa = _pa()
    r = 0.5
    V = 4.0 / 3.0 * np.pi * r ** 3
    body = dict(pos=np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]], np.float32), shape=np.full(2, pa.SHAPE_SPHERE, np.uint32),
                half_extent=np.array([[r, 0, 0]] * 2, np.float32))
    w = _world(body, gravity_force=(0.0, 0.0, 0.0), gravity_offset=(0.0, 0.0, 0.0))
    w.set_liquids([[10.0, -3.0, 0.0]], half_extent=[2.0, 3.0, 2.0], density=2.0, gravity=[0, -10.0, 0])
    w.apply_liquids()
    assert not np.any(w.get_forces()[0])  # nobody over the pool
    w.set_liquid_poses([[0.5, -3.0, 0.0]])  # under body 0, the surface through its centre
    w.apply_liquids()
    f = w.get_forces()[0]
    assert f[0][1] == pytest.approx(2.0 * V / 2 * 10.0, rel=1e-5) and f[0][0] == 0 and not np.any(f[1])
    assert w.get_submersion()[0][0] == pytest.approx(0.5, abs=1e-6) and list(w.get_submersion()[1]) == [0, lr.NO_LIQUID]
    w.set_forces(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32))
    w.set_liquid_poses([[0.5, -3.0 + r, 0.0]], rot=[[0, 0, 0, 1]])  # a tide: the surface rises over the sphere
    w.set_liquid_params(3.0, [0, -10.0, 0], flow=[1.0, 0, 0], drag=[4.0, 0.0])  # ... denser, and flowing
    w.apply_liquids()
    f = w.get_forces()[0]
    assert f[0][1] == pytest.approx(3.0 * V * 10.0, rel=1e-5) and f[0][0] == pytest.approx(4.0, rel=1e-6)
    # set_bodies keeps the set, with another body count
    w.set_bodies(np.array([[0.0, -1.0, 0.0], [20.0, 0.0, 0.0], [0.5, -2.0, 0.5]], np.float32), shape_type=np.full(3, pa.SHAPE_SPHERE, np.uint32),
                 half_extent=np.array([[r, 0, 0]] * 3, np.float32))
    frac, liquid = w.get_submersion()
    assert list(frac) == [1.0, 0.0, 1.0] and list(liquid) == [0, lr.NO_LIQUID, 0]
    w.set_liquid_params(0.0, [0, -10.0, 0])  # density 0 and no drag: the liquid is there and pushes nothing
    w.apply_liquids()
    assert not np.any(w.get_forces()[0]) and list(w.get_submersion()[0]) == [1.0, 0.0, 1.0]
    w.close()


# ---- 6. behaviour -------------------------------------------------------------------------------------------------------------
W_FORCE = 9.81  # the world's gravity is a force, the same on every body
UPDATES = 600


def _float64_settle(shape, he, q, density, drag0, y0, updates):
    """The flat body of unit mass dropped from y0 into a pool whose surface is y = 0, translation only, stepped as an update
    steps it (v += F dt, then y += v dt), in float64: frac after each update."""
    R, n = lr.rot_matrix(q), np.array([0.0, 1.0, 0.0])
    Vs = lr.shape_volume(shape, he)
    y, v, out = y0, 0.0, []
    for _ in range(updates):
        V, _ = lr.wet(shape, R, he, y, n)
        f = min(V / Vs, 1.0)
        v += (-W_FORCE + density * V * 9.81 - drag0 * f * v) * DT_S
        y += v * DT_S
        out.append(min(lr.wet(shape, R, he, y, n)[0] / Vs, 1.0))
    return np.array(out)


@pytest.mark.parametrize("shape,he,flat", [(lr.SPHERE, [0.4, 0, 0], 0.0), (lr.BOX, [0.5, 0.2, 0.35], 0.0), (lr.CAPSULE, [0.2, 0.45, 0], np.pi / 2)],
                         ids=["sphere", "box", "capsule"])
def test_lighter_bodies_float_at_their_water_line_and_lie_flat(shape, he, flat):
    """Two bodies of one shape, half as heavy as the liquid they displace, dropped into a pool with drag: body 0 in the attitude
    it floats in, body 1 turned 0.25 rad out of it. After 600 updates both are at rest (speed and spin below 1e-3), frac of
    body 0 is the 0.5 its weight implies - within what the float64 reference stepped the same way is away from it, plus twice
    that reference's last step-to-step change, plus 2 C 2^-23 for the float32 balance of forces - and body 1 lies flat too."""
    Vs = lr.shape_volume(shape, he)
    density = W_FORCE / (0.5 * Vs * 9.81)  # floats half wet
    q = [[0, 0, float(np.sin(a / 2)), float(np.cos(a / 2))] for a in (flat, flat + 0.25)]
    y0 = 0.8
    body = dict(pos=np.array([[0, y0, 0], [3, y0, 0]], np.float32), rot=np.array(q, np.float32), shape=np.full(2, shape, np.uint32),
                half_extent=np.array([he, he], np.float32))
    w = _world(body, gravity_offset=(0.0, 0.0, 0.0))
    w.set_liquids([[0, -3, 0]], half_extent=[8, 3, 8], density=density, gravity=[0, -9.81, 0], drag=[30.0, 6.0])
    w.update_n(DT, UPDATES)
    frac, liquid = w.get_submersion()
    lin, ang = w.get_velocities()
    rot = w.get_transforms()[1]
    w.sync()
    w.close()
    ref = _float64_settle(shape, he, q[0], density, 30.0, y0, UPDATES)
    c = C_CAPSULE if shape == lr.CAPSULE else C_SPHERE_BOX
    tol = abs(ref[-1] - 0.5) + 2 * abs(ref[-1] - ref[-2]) + 2 * c * EPS
    up = [abs(lr.rot_matrix(rot[i])[1, 1]) for i in range(2)]  # |cos| of the angle between the body's y axis and the world's
    print(f"frac {frac}, reference {ref[-1]:.9f} (last change {abs(ref[-1] - ref[-2]):.2e}), tolerance {tol:.2e}; speed "
          f"{np.linalg.norm(lin, axis=1)}, spin {np.linalg.norm(ang, axis=1)}; |y axis . up| {up}")
    assert list(liquid) == [0, 0]
    assert np.linalg.norm(lin, axis=1).max() < 1e-3 and np.linalg.norm(ang, axis=1).max() < 1e-3
    assert abs(frac[0] - 0.5) <= tol
    assert abs(frac[1] - 0.5) <= tol + 1e-3  # (its water line is that of the attitude it has come to, to second order in the tilt left)
    if shape == lr.BOX:
        assert min(up) > np.cos(0.02)
    if shape == lr.CAPSULE:
        assert max(up) < np.sin(0.02)


def test_a_heavier_body_sinks_to_the_floor():
    pa = _pa()
    r = 0.4
    V = 4.0 / 3.0 * np.pi * r ** 3
    body = dict(pos=np.array([[0, 0.2, 0]], np.float32), shape=np.array([pa.SHAPE_SPHERE], np.uint32), half_extent=np.array([[r, 0, 0]], np.float32))
    w = _world(body, flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, ground_height=-2.0, gravity_offset=(0.0, 0.0, 0.0))
    w.set_liquids([[0, -1.5, 0]], half_extent=[8, 1.5, 8], density=0.5 * W_FORCE / (V * 9.81), gravity=[0, -9.81, 0], drag=[4.0, 1.0])
    w.update_n(DT, UPDATES)
    y = float(w.get_transforms()[0][0][1])
    speed = float(np.linalg.norm(w.get_velocities()[0][0]))
    frac = w.get_submersion()[0]
    w.sync()
    w.close()
    print(f"y {y:.5f} (floor {-2.0 + r}), speed {speed:.2e}")
    assert abs(y - (-2.0 + r)) < 0.02 and speed < 1e-2 and frac[0] == 1.0


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    pa = _pa()
    from physics_amd import _abi
    E, U = _abi.PHYS_ERR_INVALID_ARG, _abi.PHYS_ERR_UNSUPPORTED
    w = _world(dict(pos=np.zeros((4, 3), np.float32)))
    lib = w.lib
    f32 = C.c_float

    def arrays(n):
        return dict(pos=(f32 * (3 * n))(), rot=(f32 * (4 * n))(*([0, 0, 0, 1] * n)), he=(f32 * (3 * n))(*([1.0] * (3 * n))), mask=None,
                    density=(f32 * n)(*([1.0] * n)), gravity=(f32 * (3 * n))(*([0, -9.81, 0] * n)), flow=(f32 * (3 * n))(),
                    drag=(f32 * (2 * n))(*([1.0, 1.0] * n)))

    def call(a, n, handle=None):
        rc = lib.phys_set_liquids(handle or w.h, n, a["pos"], a["rot"], a["he"], a["mask"], a["density"], a["gravity"], a["flow"], a["drag"])
        return rc, lib.phys_last_error().decode()

    assert call(arrays(3), 3)[0] == 0
    cases = [("pos", 4, float("nan"), "liquid 1: non-finite number"), ("rot", 0, float("inf"), "liquid 0: non-finite number"),
             ("he", 8, float("inf"), "liquid 2: non-finite number"), ("density", 1, float("nan"), "liquid 1: non-finite number"),
             ("gravity", 8, float("nan"), "liquid 2: non-finite number"), ("flow", 0, float("-inf"), "liquid 0: non-finite number"),
             ("drag", 5, float("nan"), "liquid 2: non-finite number"), ("he", 3, -0.5, "liquid 1: negative half extent"),
             ("density", 2, -1.0, "liquid 2: negative density"), ("drag", 2, -0.25, "liquid 1: negative drag coefficient"),
             ("drag", 3, -0.25, "liquid 1: negative drag coefficient")]
    for name, index, value, message in cases:
        a = arrays(3)
        a[name][index] = value
        assert call(a, 3) == (E, message)
    a = arrays(3)  # the stated order within one liquid, and the first offending liquid
    a["drag"][2], a["density"][1], a["he"][3] = -1.0, -1.0, -1.0
    assert call(a, 3) == (E, "liquid 1: negative half extent")
    a["he"][3] = 1.0
    assert call(a, 3) == (E, "liquid 1: negative density")
    a["flow"][5] = float("nan")
    assert call(a, 3) == (E, "liquid 1: non-finite number")
    a["drag"][0] = -1.0
    assert call(a, 3) == (E, "liquid 0: negative drag coefficient")
    for name in ("pos", "he", "density", "gravity", "flow", "drag"):
        a = arrays(3)
        a[name] = None
        assert call(a, 3) == (E, "liquids need pos, half_extent, density, gravity, flow and drag")
    assert call(arrays(1025), 1025) == (E, "phys_set_liquids: more than PHYS_MAX_LIQUIDS liquids")
    assert call(arrays(1024), 1024)[0] == 0  # the most a world keeps
    w.apply_liquids()
    assert call(arrays(3), 3)[0] == 0  # (a refused call left the set as it was; this one replaces it)
    # count mismatches and bad values in the poses / params calls
    p2, p3, d3 = (f32 * 6)(), (f32 * 9)(), (f32 * 3)(1.0, 1.0, 1.0)
    c3 = (f32 * 6)(*([1.0, 1.0] * 3))
    assert lib.phys_set_liquid_poses(w.h, 2, p2, None) == E and "n must equal the liquid count" in lib.phys_last_error().decode()
    assert lib.phys_set_liquid_params(w.h, 4, d3, p3, p3, c3) == E and "n must equal the liquid count" in lib.phys_last_error().decode()
    assert lib.phys_set_liquid_poses(w.h, 3, None, None) == E and lib.phys_last_error().decode() == "phys_set_liquid_poses: null pos"
    for args in ((None, p3, p3, c3), (d3, None, p3, c3), (d3, p3, None, c3), (d3, p3, p3, None)):
        assert lib.phys_set_liquid_params(w.h, 3, *args) == E
        assert lib.phys_last_error().decode() == "phys_set_liquid_params: null density, gravity, flow or drag"
    p3[4] = float("nan")
    assert lib.phys_set_liquid_poses(w.h, 3, p3, None) == E and lib.phys_last_error().decode() == "phys_set_liquid_poses: non-finite pose"
    assert lib.phys_set_liquid_params(w.h, 3, d3, p3, (f32 * 9)(), c3) == E and lib.phys_last_error().decode() == "liquid 1: non-finite number"
    p3[4] = 0.0
    d3[2] = -2.0
    assert lib.phys_set_liquid_params(w.h, 3, d3, p3, p3, c3) == E and lib.phys_last_error().decode() == "liquid 2: negative density"
    d3[2] = 2.0
    c3[1] = -1.0
    assert lib.phys_set_liquid_params(w.h, 3, d3, p3, p3, c3) == E and lib.phys_last_error().decode() == "liquid 0: negative drag coefficient"
    c3[1] = 1.0
    assert lib.phys_set_liquid_poses(w.h, 3, p3, None) == 0 and lib.phys_set_liquid_params(w.h, 3, d3, p3, p3, c3) == 0
    w.sync()
    w.close()
    # sharded worlds: every call
    g = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0, 0, 0), max_ghosts=8))
    g.set_bodies(np.zeros((2, 3), np.float32) + [[0, 5, 0], [3, 5, 0]], shape_type=np.full(2, pa.SHAPE_BOX, np.uint32), half_extent=np.ones((2, 3), np.float32))
    assert call(arrays(3), 3, handle=g.h)[0] == U and "max_ghosts" in lib.phys_last_error().decode()
    assert lib.phys_set_liquid_poses(g.h, 0, None, None) == U and lib.phys_set_liquid_params(g.h, 0, None, None, None, None) == U
    assert lib.phys_apply_liquids(g.h) == U and lib.phys_get_submersion(g.h, None, None) == U and lib.phys_get_submersion_device(g.h, None, None) == U
    with pytest.raises(pa.PhysError) as e:
        g.apply_liquids()
    assert e.value.code == U and e.value.args and "liquids are not supported in a world with max_ghosts > 0" in str(e.value)
    g.close()
