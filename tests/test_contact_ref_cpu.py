"""CPU: tests/contact_ref.py, the float64 reference of the contact solver and its colouring, proved here before the GPU
tests rely on it. Hand cases against closed forms; the colouring against the CPU oracle's, exactly; velocities against
the oracle's float32 solve (which equals the device's bit for bit on every solver path: tests/test_gpu_collision.py).
The largest float32-against-float64 spread of each case is printed: the GPU tolerances of
tests/test_gpu_solver_independent.py are taken from these numbers."""
import numpy as np
import pytest

import contact_ref as cr
from physics_amd import scenes
from physics_amd._abi import (FLAG_COLLISIONS, FLAG_GROUND_PLANE, FLAG_NO_WARM_START, SHAPE_BOX, SHAPE_SPHERE,
                              default_config)

DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
GRAVITY = np.array([0.0, -9.81, 0.0])


@pytest.fixture(scope="module")
def ob(oracle_lib):
    from oracle import binding
    return binding


def oracle_world(ob, bodies, flags=FLAG_COLLISIONS | FLAG_GROUND_PLANE, gravity=(0, 0, 0), **cfg):
    w = ob.OracleWorld(default_config(flags=flags, gravity_force=gravity, gravity_offset=(0, 0, 0), **cfg), trig=ob.TRIG_DET)
    w.set_threads(16)
    w.set_bodies(**bodies)
    return w


def run(world, ref, n_updates, inv_m, inv_I, force=None):
    """Per update: the reference started from the world's poses and velocities, and the world's velocities after."""
    for _ in range(n_updates):
        pos, _ = world.get_transforms()
        lin, ang = world.get_velocities()
        world.update(DT)
        out = ref.update(world.get_manifolds(), pos, lin, ang, inv_m, inv_I, force)
        lin1, ang1 = world.get_velocities()
        yield out, lin1, ang1, world.get_stats()


def one_update(ob, bodies, iterations=8, **cfg):
    n = len(bodies["pos"])
    w = oracle_world(ob, bodies, solver_iterations=iterations, **cfg)
    ref = cr.SolverRef(n, cr.Params(DT_S, **cfg), iterations)
    out, lin1, ang1, _ = next(run(w, ref, 1, *cr.body_inverses(n, bodies.get("mass"), bodies.get("inertia"))))
    return out, lin1, ang1


def body(pos, lin=(0, 0, 0), shape=SHAPE_BOX, he=(0.5, 0.5, 0.5), mass=1.0):
    return dict(pos=pos, lin=lin, shape=shape, he=he, mass=mass)


def bodies_of(*bs):
    return dict(pos=np.array([b["pos"] for b in bs], np.float32), lin_vel=np.array([b["lin"] for b in bs], np.float32),
                shape_type=np.array([b["shape"] for b in bs], np.uint32), half_extent=np.array([b["he"] for b in bs], np.float32),
                mass=np.array([b["mass"] for b in bs], np.float32))


# ---------------------------------------------------------------- hand cases with closed forms
def test_box_sliding_on_the_ground_slips_with_dvt_equal_mu_dvn(ob):
    """A flat box lands at 1 unit/s while sliding at 5 along x: every friction row of the four corners ends at the box
    clamp (n = -y: tangent 1 is z, tangent 2 is -x), so the tangential change is mu times the normal change, against the
    sliding direction."""
    out, lin1, ang1 = one_update(ob, bodies_of(body((0, 0.5, 0), lin=(5.0, -1.0, 0))))
    dv = out["lin"][0] - np.array([5.0, -1.0, 0])
    assert out["count"][0] == 4 and dv[1] > 0.9
    # (the normal row of a point runs after its friction rows and still moves pn by the Gauss-Seidel residual: 1e-3)
    assert dv[0] == pytest.approx(-0.5 * dv[1], rel=1e-3)
    P = out["impulses"][0]
    assert (np.abs(P[:, 1]) >= 0.99 * 0.5 * P[:, 2]).all() and (P[:, 1] < 0).all()  # every x row at the clamp
    assert abs(dv[2]) < 1e-3  # (unequal corner impulses turn the box a little about y: tangent 1 picks up a residue)
    assert np.abs(lin1 - out["lin"]).max() < 1e-5 and np.abs(ang1 - out["ang"]).max() < 1e-5


def test_box_sliding_slowly_on_the_ground_sticks(ob):
    """The same box sliding at 0.2 along x: friction holds (0.2 < mu x 1), and after the solve the contact points no
    longer slide (the Gauss-Seidel residual of 8 iterations on four coupled points)."""
    out, lin1, ang1 = one_update(ob, bodies_of(body((0, 0.5, 0), lin=(0.2, -1.0, 0))))
    v, w = out["lin"][0], out["ang"][0]
    corners = np.array([[sx, -0.5, sz] for sx in (-0.5, 0.5) for sz in (-0.5, 0.5)])
    slide = v[None, :] + np.cross(w, corners)
    assert np.abs(slide[:, [0, 2]]).max() < 1e-3, slide
    assert np.abs(lin1 - out["lin"]).max() < 1e-5


def test_head_on_pair_with_unequal_masses_ends_with_the_common_velocity(ob):
    """Spheres of masses 1 and 3 touching (depth within the slop: no bias) close at 4 units/s along x: the normal row
    leaves them with the velocity of their centre of mass, 0.5 units/s (perfectly inelastic contact)."""
    bs = bodies_of(body((0, 5, 0), lin=(3.0, 0, 0), shape=SHAPE_SPHERE, mass=1.0),
                   body((0.995, 5, 0), lin=(-1.0, 0, 0), shape=SHAPE_SPHERE, mass=3.0))
    out, lin1, _ = one_update(ob, bs)
    want = (1.0 * 3.0 + 3.0 * -1.0) / 4.0
    assert np.abs(out["lin"][:, 0] - want).max() < 1e-9 and np.abs(out["lin"][:, 1:]).max() < 1e-12
    assert np.abs(lin1 - out["lin"]).max() < 1e-6


def test_deep_overlap_is_pushed_apart_at_max_bias(ob):
    """Equal spheres 0.5 deep at rest: baumgarte / dt x (depth - slop) = 5.9 units/s is capped at max_bias = 3, so they
    separate at exactly 3 units/s, 1.5 each."""
    bs = bodies_of(body((0, 5, 0), shape=SHAPE_SPHERE), body((0.5, 5, 0), shape=SHAPE_SPHERE))
    out, lin1, _ = one_update(ob, bs)
    assert out["lin"][0, 0] == pytest.approx(-1.5, abs=1e-9) and out["lin"][1, 0] == pytest.approx(1.5, abs=1e-9)
    assert np.abs(lin1 - out["lin"]).max() < 1e-6
    out, lin1, _ = one_update(ob, bs, max_bias=1.25)
    assert out["lin"][1, 0] - out["lin"][0, 0] == pytest.approx(1.25, abs=1e-9)
    assert np.abs(lin1 - out["lin"]).max() < 1e-6


def test_speculative_point_closes_only_its_gap(ob):
    """Spheres 0.01 apart (a speculative point, depth < 0) closing at 2 units/s: the normal row lets them close at
    gap / dt = 0.6 units/s and no faster; closing at 0.3 they are left alone."""
    for speed, want in ((2.0, 0.01 / DT_S), (0.3, 0.3)):
        bs = bodies_of(body((0, 5, 0), lin=(speed, 0, 0), shape=SHAPE_SPHERE), body((1.01, 5, 0), shape=SHAPE_SPHERE))
        out, lin1, _ = one_update(ob, bs)
        assert out["lin"][0, 0] - out["lin"][1, 0] == pytest.approx(want, rel=1e-4)
        assert np.abs(lin1 - out["lin"]).max() < 1e-6


# ---------------------------------------------------------------- colouring: exactly the oracle's
def _check_colors(o, out):
    st = o.get_stats()
    assert np.array_equal(o.get_colors(), out["colors"])
    assert (st.n_colors, st.color_rounds, st.n_new_manifolds) == (out["n_colors"], out["color_rounds"], out["n_new_manifolds"])


def test_colouring_of_a_small_pile_matches_the_oracle(ob):
    sc = scenes.c1()
    o = ob.OracleWorld(sc.config(), trig=ob.TRIG_DET)
    sc.populate(o)
    o.update_n(DT, 150)
    pos, rot = o.get_transforms()
    lin, ang = o.get_velocities()
    o2 = oracle_world(ob, dict(pos=pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=sc.shape_type, half_extent=sc.half_extent),
                      gravity=(0, -9.81, 0))
    ref = cr.SolverRef(sc.n, cr.Params(DT_S), 8)
    seen = 0
    for out, *_ in run(o2, ref, 3, *cr.body_inverses(sc.n), GRAVITY):
        _check_colors(o2, out)
        seen = max(seen, out["n_colors"])
    assert seen >= 3


def test_persistent_colouring_of_a_churning_scene_matches_the_oracle_on_every_update(ob):
    """130 updates of a falling 1440-body mixed scene (two PHYS_COLOR_CACHE_PERIODs): manifolds appear and vanish every
    update; colours, n_colors, color_rounds and n_new_manifolds equal the oracle's on every one. The velocities of this
    warm-started coupled pile are compared too (the reference carries its own impulses all the way)."""
    sc = scenes.c3(12, 10, 12)
    o = ob.OracleWorld(sc.config(), trig=ob.TRIG_DET)
    o.set_threads(16)
    sc.populate(o)
    ref = cr.SolverRef(sc.n, cr.Params(DT_S), 8)
    worst, churn, rounds, n_amb = 0.0, 0, 0, 0
    for out, lin1, ang1, st in run(o, ref, 130, *cr.body_inverses(sc.n), GRAVITY):
        _check_colors(o, out)
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst, n_amb = max(worst, err), n_amb + amb
        churn += out["n_new_manifolds"] > 0 and out["n_new_manifolds"] < st.n_manifolds
        rounds = max(rounds, out["color_rounds"])
    print(f"\nC3(12,10,12) x 130 warm-started updates: largest velocity error {worst:.3g} ({n_amb} ambiguous manifolds)")
    assert churn > 50 and rounds >= 2 and out["n_colors"] >= 6
    assert worst < 2e-5


# ---------------------------------------------------------------- velocities against the oracle
@pytest.mark.parametrize("inertia", ["identity", "diag", "full"])
def test_friction_pairs_against_the_oracle(ob, inertia):
    """Isolated manifolds with friction engaged, 2 and 8 iterations, default and non-default parameters. GPU test (a)
    uses 1e-5: float32 rows against float64 measured at most 2.6e-6 here."""
    bodies = cr.friction_pairs(3, 150, inertia)
    for iterations in (2, 8):
        for params in ({}, dict(baumgarte=0.35, slop=0.003, friction=0.9, max_bias=1.25)):
            out, lin1, ang1 = one_update(ob, bodies, iterations=iterations, **params)
            err, amb = cr.velocity_error(out, lin1, ang1)
            clamped, inside = cr.friction_row_states(out, params.get("friction", 0.5))
            print(f"\nfriction pairs {inertia} it={iterations} {params or 'defaults'}: error {err:.3g}, clamped {clamped} inside {inside}, {amb} ambiguous")
            assert len(out["a"]) == 450 and amb <= 2
            assert clamped >= 0.2 * (clamped + inside) and inside >= 0.2 * (clamped + inside)
            assert err < 1e-5


def _warm_updates(ob, bodies, flags, n_updates, spin=None):
    n = len(bodies["pos"])
    warm = not flags & FLAG_NO_WARM_START
    o = oracle_world(ob, bodies, flags=FLAG_COLLISIONS | FLAG_GROUND_PLANE | flags)
    ref = cr.SolverRef(n, cr.Params(DT_S), 8, warm=warm)
    inv = cr.body_inverses(n, bodies.get("mass"), bodies.get("inertia"))
    return [(out, *cr.velocity_error(out, lin1, ang1)) for out, lin1, ang1, _ in run(o, ref, n_updates, *inv)]


@pytest.mark.parametrize("flags", [0, FLAG_NO_WARM_START])
def test_consecutive_warm_started_updates_against_the_oracle(ob, flags):
    """Six updates of the friction pairs: from the second on, the carried impulses matter (sweep 0)."""
    res = _warm_updates(ob, cr.friction_pairs(4, 150, "full"), flags, 6)
    worst = max(e for _, e, _ in res)
    carried = sum(int((np.abs(out["P0"]) > 0).any(axis=(1, 2)).sum()) for out, _, _ in res) if not flags else 0
    print(f"\nfriction pairs, 6 updates, flags {flags}: largest error {worst:.3g}, manifolds carrying impulses {carried}")
    assert worst < 1e-5
    if not flags:
        assert carried > 300


@pytest.mark.parametrize("scene", ["heap", "c1_settled"])
def test_coupled_piles_against_the_oracle(ob, scene):
    """Manifolds that share bodies, solved colour after colour, six warm-started updates from a fresh world."""
    if scene == "heap":
        bodies = cr.random_heap(5)
    else:
        sc = scenes.c1()
        o = ob.OracleWorld(sc.config(), trig=ob.TRIG_DET)
        sc.populate(o)
        o.update_n(DT, 300)
        pos, rot = o.get_transforms()
        lin, ang = o.get_velocities()
        bodies = dict(pos=pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=sc.shape_type, half_extent=sc.half_extent)
    n = len(bodies["pos"])
    o = oracle_world(ob, bodies, gravity=(0, -9.81, 0))
    ref = cr.SolverRef(n, cr.Params(DT_S), 8)
    worst, colors = 0.0, 0
    for out, lin1, ang1, _ in run(o, ref, 6, *cr.body_inverses(n, bodies.get("mass"), bodies.get("inertia")), GRAVITY):
        _check_colors(o, out)
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst, colors = max(worst, err), max(colors, out["n_colors"])
        assert amb <= 0.01 * len(out["a"])
    print(f"\n{scene}: {len(out['a'])} manifolds, {colors} colours, largest velocity error {worst:.3g}")
    assert colors >= 3
    assert worst < 2e-5


def test_cluster_tower_against_the_oracle(ob):
    """The 33k-body tower C5(16, 130, 16): six warm-started updates from a fresh world, about 100k coupled manifolds.
    GPU test (c) runs the cluster kernels on it with the tolerance measured here (x 10)."""
    sc = scenes.c5(16, 130, 16)
    o = ob.OracleWorld(sc.config(), trig=ob.TRIG_DET)
    o.set_threads(16)
    sc.populate(o)
    ref = cr.SolverRef(sc.n, cr.Params(DT_S), 8)
    worst = 0.0
    for out, lin1, ang1, _ in run(o, ref, 6, *cr.body_inverses(sc.n), GRAVITY):
        _check_colors(o, out)
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst = max(worst, err)
        assert amb == 0
    print(f"\nC5(16,130,16) tower: {len(out['a'])} manifolds, largest velocity error {worst:.3g}")
    assert len(out["a"]) > 90_000
    assert worst < 2e-5
