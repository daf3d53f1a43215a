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


# ---------------------------------------------------------------- the varied tower: unequal bodies, cold and short solves
def test_varied_tower_gives_every_body_constants_of_its_own():
    """The lattice is C5(16, 130, 16)'s; masses are log-uniform in [0.25, 4] and differ between neighbours; `uniform` is
    one diagonal tensor that is not the identity, `diag` three distinct entries per body, `full` has off-diagonals."""
    sc = scenes.c5(16, 130, 16)
    for kind in ("uniform", "diag", "full"):
        b = cr.varied_tower(cr.VARIED_SEED, kind)
        assert np.array_equal(b["pos"], sc.pos) and len(b["pos"]) == 33_280
        m = b["mass"].astype(np.float64)
        assert 0.25 <= m.min() < 0.26 and 3.9 < m.max() <= 4.0
        hist = np.histogram(np.log(m), bins=8, range=(np.log(0.25), np.log(4.0)))[0]
        assert hist.min() > 0.8 * len(m) / 8 and hist.max() < 1.2 * len(m) / 8
        assert (m[1:] != m[:-1]).all() and (m[256:] != m[:-256]).all() and (m[16:] != m[:-16]).all()
        I = b["inertia"].reshape(-1, 3, 3)
        d = np.stack([I[:, 0, 0], I[:, 1, 1], I[:, 2, 2]], 1)
        off = I - d[:, :, None] * np.eye(3, dtype=np.float32)
        if kind == "uniform":
            assert (I == I[0]).all() and not off.any() and (d[0] != 1).all()
        elif kind == "diag":
            assert not off.any() and (d[:, 0] != d[:, 1]).all() and (d[:, 1] != d[:, 2]).all() and (d[:, 0] != d[:, 2]).all()
            assert (d[1:] != d[:-1]).all()
        else:
            assert (np.abs(off).max(axis=(1, 2)) > 1e-3).all() and np.array_equal(I, I.transpose(0, 2, 1))
            assert (np.linalg.eigvalsh(I.astype(np.float64)) > 1.0).all()
        assert {int(s) for s in np.unique(b["shape_type"])} == {cr.SHAPE_SPHERE, cr.SHAPE_BOX, cr.SHAPE_CAPSULE}


@pytest.mark.parametrize("case", list(cr.VARIED_CASES))
def test_varied_tower_against_the_oracle(ob, case):
    """VARIED_UPDATES updates of the varied tower per case of contact_ref.VARIED_CASES, the oracle's float32 solve against
    the reference. Pins, for the reference alone, what the GPU tests rely on: more than 40 960 manifolds in every update
    (the cluster plan's floor), at least 6 colours, manifolds of 1, 2 and 4 points at least 2 % each, ambiguous manifolds
    within 1 %, and friction rows at the +-mu pn box and inside it, at least 10 % each, in every update of the warm
    eight-iteration solves and in update 1 of the cold one (the sliding the builder sets dies down: with nothing carried, a
    cold solve of update 3 leaves 9.8 % of the rows at the clamp; one or two iterations from rest leave hardly any).
    The error printed here, at its worst over the cases, is contact_ref.MEASURED_VARIED; TOL_VARIED is four times that."""
    inertia, warm, iterations = cr.VARIED_CASES[case]
    bodies = cr.varied_tower(cr.VARIED_SEED, inertia)
    n = len(bodies["pos"])
    o = oracle_world(ob, bodies, flags=FLAG_COLLISIONS | FLAG_GROUND_PLANE | (0 if warm else FLAG_NO_WARM_START),
                     gravity=(0, -9.81, 0), solver_iterations=iterations)
    ref = cr.SolverRef(n, cr.Params(DT_S), iterations, warm=warm)
    worst = 0.0
    for u, (out, lin1, ang1, _) in enumerate(run(o, ref, cr.VARIED_UPDATES, *cr.body_inverses(n, bodies["mass"], bodies["inertia"]), GRAVITY)):
        _check_colors(o, out)
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst = max(worst, err)
        m = len(out["a"])
        shares = cr.point_count_shares(out["count"])
        clamped, inside = cr.friction_row_states(out, cr.TOWER_MU)
        carried = int((np.abs(out["P0"]) > 0).any(axis=(1, 2)).sum()) if warm else 0
        print(f"\nvaried tower {case} update {u + 1}: {m} manifolds, {out['n_colors']} colours, 1/2/4 points "
              f"{shares[0]:.3f}/{shares[1]:.3f}/{shares[2]:.3f}, friction rows clamped {clamped} inside {inside}, "
              f"carrying impulses {carried}, {amb} ambiguous, error {err:.3g}")
        assert m > 40_960 and out["n_colors"] >= 6
        assert min(shares) >= 0.02
        assert amb <= 0.01 * m
        if iterations == 8 and (warm or u == 0):
            assert clamped >= 0.1 * (clamped + inside) and inside >= 0.1 * (clamped + inside)
        if warm and u:
            assert carried > 0.5 * m
    print(f"varied tower {case}: largest velocity error {worst:.3g} (MEASURED_VARIED {cr.MEASURED_VARIED:.3g}, TOL_VARIED {cr.TOL_VARIED:.3g})")
    assert worst <= cr.TOL_VARIED / 4


# ---------------------------------------------------------------- static colliders as partners
def _relabelled(man, n):
    """The manifolds of a world that holds the statics as bodies n + k: those of a body with a body or a static, the
    static's id written as STATIC_ID_BIT | k (the order by pair stays: n + k and BIT | k sort alike behind every body)."""
    ids, counts, normals, points = man
    ids = np.asarray(ids, np.int64)
    keep = ids[:, 0] < n
    ids = ids[keep].copy()
    st = ids[:, 1] >= n
    ids[st, 1] = cr.STATIC_ID_BIT | (ids[st, 1] - n)
    return ids, np.asarray(counts)[keep], np.asarray(normals)[keep], np.asarray(points)[keep]


def test_static_partners_native_equal_the_extra_body_wrapper(ob):
    """contact_ref with a static as what it is (a partner id with STATIC_ID_BIT: no body, like the ground) against the
    wrapper of tests/test_gpu_static.py that models static k as extra body n + k of infinite mass - right under ITS
    condition of one manifold per static, which this scene meets. Manifolds from the oracle's body path, relabelled:
    identical colours and velocities."""
    from test_gpu_static import _ref_update_with_statics
    bodies, statics = cr.static_boxes(21, 120)
    n, k = len(bodies["pos"]), len(statics["pos"])
    both = {key: np.concatenate([bodies[key], statics[key]]) for key in ("pos", "shape_type", "half_extent")}
    both["rot"] = np.concatenate([bodies["rot"], np.tile(np.float32([0, 0, 0, 1]), (k, 1))])
    o = oracle_world(ob, both, flags=FLAG_COLLISIONS)
    o.collide_now()
    man = _relabelled(o.get_manifolds(), n)
    b = man[0][:, 1]
    st_b = b[(b & cr.STATIC_ID_BIT) != 0]
    assert len(st_b) >= 100 and len(np.unique(st_b)) == len(st_b), "one manifold per static (the wrapper's condition)"
    assert ((b & cr.STATIC_ID_BIT) == 0).sum() >= 20, "body-body manifolds on top of the static ones"
    inv_m, inv_I = cr.body_inverses(n)
    force = np.tile(GRAVITY, (n, 1))
    pos, lin, ang = (bodies[key].astype(np.float64) for key in ("pos", "lin_vel", "ang_vel"))
    native = cr.SolverRef(n, cr.Params(DT_S), 8).update(man, pos, lin, ang, inv_m, inv_I, force)
    wrapped = _ref_update_with_statics(cr.SolverRef(n + k, cr.Params(DT_S), 8), n, statics["pos"].astype(np.float64), man, pos, lin, ang,
                                       inv_m, inv_I, force)
    assert np.array_equal(native["colors"], wrapped["colors"]) and native["n_colors"] == wrapped["n_colors"] >= 2
    assert (native["color_rounds"], native["n_new_manifolds"]) == (wrapped["color_rounds"], wrapped["n_new_manifolds"])
    assert np.array_equal(native["lin"], wrapped["lin"][:n]) and np.array_equal(native["ang"], wrapped["ang"][:n])
    assert not wrapped["lin"][n:].any() and np.abs(native["lin"] - lin).max() > 0.1
    assert np.array_equal(native["impulses"], wrapped["impulses"])


def test_statics_shared_by_several_bodies_take_no_colour_of_their_own():
    """Where the wrapper's condition fails - a slab under many bodies - the two differ, and the native handling is the
    documented one: bodies on one static share no body, so all their manifolds take colour 0 in one round."""
    m = 40
    a = np.arange(m)
    b = np.full(m, cr.STATIC_ID_BIT | 7)
    colors, n_colors, rounds, n_new = cr.color_manifolds(a, b, m)
    assert (colors == 0).all() and (n_colors, rounds, n_new) == (1, 1, m)
    # a body on the slab and against a wall, with a neighbour: three manifolds at body 0, three colours
    a = np.array([0, 0, 0, 1])
    b = np.array([1, cr.STATIC_ID_BIT | 0, cr.STATIC_ID_BIT | 3, cr.STATIC_ID_BIT | 0])
    colors, n_colors, _, _ = cr.color_manifolds(a, b, 2)
    assert sorted(colors[:3]) == [0, 1, 2] and colors[3] != colors[0] and n_colors == 3
    # the priority hashes the full pair: the id of the static matters
    assert cr.color_priority(0, cr.STATIC_ID_BIT | 0) != cr.color_priority(0, cr.STATIC_ID_BIT | 3) != cr.color_priority(0, cr.GROUND)


def test_heap_container_and_its_twin_on_the_ground_plane(ob):
    """The scene of test_gpu_solver_independent.py::test_heap_in_a_static_container_against_the_float64_solver: no body
    starts in overlap with a wall segment, every segment has a body within the margin, and the oracle's float32 spread on
    the twin - the same heap on the ground plane at the slab's height, where a static row has the form of a ground row -
    is what TOL_COUPLED was taken from."""
    bodies = cr.random_heap(5)
    n = len(bodies["pos"])
    st = cr.heap_container(bodies)
    box = cr.body_boxes(bodies)
    he, c = st["half_extent"].astype(np.float64), st["pos"].astype(np.float64)
    slo, shi = c - he, c + he
    assert len(c) == 1 + 4 * 12 and shi[0, 1] == 0.0
    near = 0
    for k in range(1, len(c)):
        gap = np.maximum(box[:, :3] - shi[k], slo[k] - box[:, 3:]).max(1)  # boxes against an axis-aligned wall: exact
        assert gap.min() > 0.5 * cr.CONTAINER_GAP, "no body starts in overlap with a wall"
        near += int((gap < 0.02 - 1e-3).sum())
        assert gap.min() < 2 * cr.CONTAINER_GAP
    low = box[:, 1] < 0.0
    print(f"\nheap container: {near} bodies within the margin of a wall segment, {int(low.sum())} bodies reach into the slab")
    assert near >= 48 and low.sum() >= 50
    o = oracle_world(ob, bodies, gravity=(0, -9.81, 0))
    ref = cr.SolverRef(n, cr.Params(DT_S), 8)
    worst = 0.0
    for out, lin1, ang1, _ in run(o, ref, 6, *cr.body_inverses(n, bodies.get("mass"), bodies.get("inertia")), GRAVITY):
        worst = max(worst, cr.velocity_error(out, lin1, ang1)[0])
    print(f"twin of the heap container (ground plane at the slab's height): oracle's spread {worst:.3g}; TOL_COUPLED is 2e-5")
    assert worst < 2e-5


# ---------------------------------------------------------------- the oracle's bits, pinned
def _contact_bits(ob):
    """SHA-256 of what the oracle holds after 20 updates of four small scenes: poses, velocities and manifolds. (The
    oracle reads no impulses out; in the warm-started scenes every update starts from the impulses of the one before, so
    they are in the velocities.) The oracle has neither materials nor static colliders: the scene with restitution is
    stood in for by the friction pairs (slop, max_bias cap, speculative points, clamped and sticking friction rows), the
    static partners by static_boxes' bodies on a ground plane at the statics' top (a static row has a ground row's form)."""
    import hashlib
    rng = np.random.default_rng(9)
    heap = cr.random_heap(5, n=128)
    heap["inertia"] = cr._inertia(rng, 128, "full")
    on_statics, _ = cr.static_boxes(21, 24)
    scenes_ = {
        "heap_full_inertia_warm": (heap, dict(gravity=(0, -9.81, 0))),
        "heap_full_inertia_cold": (heap, dict(gravity=(0, -9.81, 0), flags=FLAG_COLLISIONS | FLAG_GROUND_PLANE | FLAG_NO_WARM_START)),
        "friction_pairs_full_inertia": (cr.friction_pairs(3, 20, "full"), dict(gravity=(0, -9.81, 0))),
        "bodies_on_a_plane_at_the_statics_top": (on_statics, dict(gravity=(0, -9.81, 0), ground_height=0.5)),
    }
    out = {}
    for name, (bodies, kw) in scenes_.items():
        w = oracle_world(ob, bodies, **kw)
        w.set_threads(1)
        w.update_n(DT, 20)
        h = hashlib.sha256()
        for arr in (*w.get_transforms(), *w.get_velocities(), *w.get_manifolds()):
            h.update(np.ascontiguousarray(arr).tobytes())
        assert w.get_stats().n_manifolds > 20, name
        out[name] = h.hexdigest()
    return out


def test_oracle_bits_of_four_small_scenes_are_the_recorded_ones(ob):
    """Oracle and kernels compile the same include/spec/contact_solve.h, so GPU-equals-oracle cannot see a slip made in
    that header: tests/golden/contact_bits.json holds the hashes recorded before its row arithmetic was last restated."""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "contact_bits.json")) as f:
        want = json.load(f)
    assert _contact_bits(ob) == want
