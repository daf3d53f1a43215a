"""GPU: the contact solver's friction rows, warm starting, colour order and non-default parameters against the float64
reference of tests/contact_ref.py, which shares no code with include/spec, the oracle or the kernels (tests/test_abi.py
checks that). Every update is checked from the device's own read-back poses and velocities; the reference carries its
own float64 impulses from update to update. Each test asserts from profile_get() which solver stage ran.

Tolerances come from tests/test_contact_ref_cpu.py, which measures the same float32-against-float64 spread on the CPU
oracle (bit-equal to the device on every solver path): at most 2.3e-6 on isolated manifolds, 3.9e-6 on coupled piles,
5.1e-7 on the C5(16, 130, 16) tower (3.9e-6 again on the heap's twin of the static container test), 3.33e-6 on the
varied tower (every body with its own mass and inertia, cold and
short solves: section (d); the tolerance there is contact_ref.TOL_VARIED = 4 x that spread)."""
import numpy as np
import pytest

import contact_ref as cr

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
GRAVITY = np.array([0.0, -9.81, 0.0])
TOL_ISOLATED = 1e-5  # measured at most 2.3e-6 (test_contact_ref_cpu: friction pairs, six warm-started updates)
TOL_COUPLED = 2e-5   # measured at most 3.9e-6 (random heap; C3 over 130 updates 3.4e-6)
TOL_TOWER = 5e-6     # measured 5.1e-7 (test_cluster_tower_against_the_oracle), x 10
SOLVER_STAGES = {"solve", "solve_tail", "solve_flow", "solve_cluster"}
PER_COLOR = {"solve", "solve_tail"}


def flags_of(solver):
    import physics_amd
    return {"default": 0, "per_color": physics_amd.FLAG_SOLVER_PER_COLOR}[solver]


def check_stages(stages, solver):
    """The device picks its kernels itself; default flags on these scenes take the dataflow kernels from the first
    update on, PHYS_FLAG_SOLVER_PER_COLOR a launch per colour (colours of more than 512 manifolds: `solve`)."""
    if solver == "per_color":
        assert "solve" in stages and stages <= PER_COLOR, stages
    else:
        assert stages == {"solve_flow"}, stages
ALT = dict(baumgarte=0.35, slop=0.003, friction=0.9, max_bias=1.25)


def make_world(bodies, flags=0, gravity=(0, 0, 0), ground=True, **cfg):
    """A world of `bodies` (set_bodies arguments) with collisions and the ground (ground=False: without it); cfg:
    solver_iterations and the solver's parameters, as default_config takes them."""
    import physics_amd
    w = physics_amd.World(physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS | (physics_amd.FLAG_GROUND_PLANE if ground else 0) | flags,
                                                     gravity_force=gravity, gravity_offset=(0, 0, 0), **cfg))
    w.set_bodies(**bodies)
    return w


def checked_updates(w, ref, n_updates, inv_m, inv_I, force=None, cold=None, **ref_args):
    """Per update: (reference output, device velocities, solver stages that ran[, cold reference output]). Both
    references start from the device's poses and velocities of that update. ref_args: further arguments of ref.update
    (material_ref's `materials`)."""
    for _ in range(n_updates):
        pos, _ = w.get_transforms()
        lin, ang = w.get_velocities()
        w.profile_enable(True)
        w.update(DT)
        w.sync()
        stages = set(w.profile_get()[0]) & SOLVER_STAGES
        man = w.get_manifolds()
        lin1, ang1 = w.get_velocities()
        out = ref.update(man, pos, lin, ang, inv_m, inv_I, force, **ref_args)
        extra = (cold.update(man, pos, lin, ang, inv_m, inv_I, force),) if cold is not None else ()
        yield (out, lin1, ang1, stages) + extra


# ---------------------------------------------------------------- (a) friction engaged, isolated manifolds
@pytest.mark.parametrize("solver", ["default", "per_color"])
@pytest.mark.parametrize("params", [{}, ALT], ids=["defaults", "baumgarte.35_slop.003_mu.9_cap1.25"])
@pytest.mark.parametrize("iterations", [2, 8])
@pytest.mark.parametrize("inertia", ["identity", "diag", "full"])
def test_friction_rows_of_isolated_manifolds(inertia, iterations, params, solver):
    """Box on box, sphere on box and box on the ground, sliding at 0 to 6 units/s: friction ends at the +-mu pn box for
    some rows and inside it for others. One update from set_bodies, through the dataflow and the per-colour kernels."""
    bodies = cr.friction_pairs(3, 150, inertia)
    n = len(bodies["pos"])
    w = make_world(bodies, flags=flags_of(solver), solver_iterations=iterations, **params)
    ref = cr.SolverRef(n, cr.Params(DT_S, **params), iterations)
    out, lin1, ang1, stages = next(checked_updates(w, ref, 1, *cr.body_inverses(n, bodies["mass"], bodies["inertia"])))
    check_stages(stages, solver)
    assert len(out["a"]) == 450
    clamped, inside = cr.friction_row_states(out, params.get("friction", 0.5))
    assert clamped >= 0.2 * (clamped + inside) and inside >= 0.2 * (clamped + inside), (clamped, inside)
    # depths from -0.015 to 0.09: speculative points and points within the slop always occur; the cap binds for the
    # non-default set (at depth > 0.0625; the default cap of 3 would need 0.26)
    depth = np.asarray(w.get_manifolds()[3])[:, :, 3]
    p = cr.Params(DT_S, **params)
    act = np.arange(4)[None, :] < out["count"][:, None]
    assert (act & (depth > 0) & (depth <= p.slop)).sum() > 20 and (act & (depth < 0)).sum() > 20
    if params:
        assert (act & (cr.contact_bias(depth, p) == p.max_bias)).sum() > 20
    err, amb = cr.velocity_error(out, lin1, ang1)
    print(f"\n{inertia} it={iterations} {params or 'defaults'} {solver} [{sorted(stages)}]: error {err:.3g} (tolerance {TOL_ISOLATED}), {amb} ambiguous")
    assert amb <= 2
    assert err < TOL_ISOLATED


# ---------------------------------------------------------------- (b) warm starting
@pytest.mark.parametrize("mode", ["default", "per_color", "no_warm_start"])
def test_warm_started_updates_of_isolated_manifolds(mode):
    """Six consecutive updates of 900 isolated manifolds, two iterations each. Default flags: the dataflow kernels; per
    colour: colour 0 holds 900 > 512 manifolds and gets launches of its own; no warm start: against a cold reference.
    Negative control: with warm starting the device does NOT match the cold reference where the carried impulses are
    large (the warm path is live)."""
    import physics_amd
    flags = {"default": 0, "per_color": physics_amd.FLAG_SOLVER_PER_COLOR, "no_warm_start": physics_amd.FLAG_NO_WARM_START}[mode]
    bodies = cr.friction_pairs(4, 300, "full")
    n = len(bodies["pos"])
    # two iterations: eight all but converge on an isolated manifold, from any start, and warm and cold would agree
    w = make_world(bodies, flags=flags, solver_iterations=2)
    warm = mode != "no_warm_start"
    ref = cr.SolverRef(n, cr.Params(DT_S), 2, warm=warm)
    cold = cr.SolverRef(n, cr.Params(DT_S), 2, warm=False) if warm else None
    worst, n_amb, live, carried, off = 0.0, 0, 0, 0, 0.0
    for u, res in enumerate(checked_updates(w, ref, 6, *cr.body_inverses(n, bodies["mass"], bodies["inertia"]), cold=cold)):
        out, lin1, ang1, stages = res[:4]
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst, n_amb = max(worst, err), n_amb + amb
        check_stages(stages, "per_color" if mode == "per_color" else "default")
        if warm and u > 0:
            big = np.flatnonzero((np.abs(out["P0"][:, :, 2]) > 0.05).any(1) & ~out["ambiguous"])
            carried += len(big)
            c = res[4]
            for m in big:
                a, b = out["a"][m], out["b"][m]
                bodies_m = [a] if b == cr.GROUND else [a, b]
                d = max(np.abs(lin1[bodies_m] - c["lin"][bodies_m]).max(), np.abs(ang1[bodies_m] - c["ang"][bodies_m]).max())
                live += d > 10 * TOL_ISOLATED
                off = max(off, d)
    print(f"\nwarm start {mode}: error {worst:.3g} (tolerance {TOL_ISOLATED}), {n_amb} ambiguous; "
          f"{live} of {carried} manifolds with large carried impulses differ from the cold solve (up to {off:.3g})")
    assert n_amb <= 0.01 * 900 * 6
    assert worst < TOL_ISOLATED
    if warm:
        assert carried > 500 and live >= 0.3 * carried and off > 1000 * TOL_ISOLATED


@pytest.mark.parametrize("case", ["turn3", "turn1", "cross"])
def test_warm_start_follows_turning_normals(case):
    """Sphere on a heavy spinning box: the normal turns 3 degrees per update (beyond the 2.56 degrees of 0.999: nothing
    carried), 1 degree (carried), or 1 degree across |n.x| = 0.57735 (the normal impulse carried, friction not: the
    tangent basis switches branch)."""
    start, turn = {"turn3": ((0.0, 20.0), 3.0), "turn1": ((0.0, 20.0), 1.0), "cross": ((33.0, 34.8), 1.0)}[case]
    import physics_amd
    bodies = cr.spinning_pairs(8, 400, turn, start, DT_S)
    n = len(bodies["pos"])
    w = make_world(bodies, flags=physics_amd.FLAG_EXACT_ROTATION)  # (quirk Q1 would turn the box by sin(w dt / 2) only)
    ref = cr.SolverRef(n, cr.Params(DT_S), 8)
    worst, n_amb, with_pn, with_pt, switched = 0.0, 0, 0, 0, 0
    for u, (out, lin1, ang1, stages) in enumerate(checked_updates(w, ref, 6, *cr.body_inverses(n, bodies["mass"], bodies["inertia"]))):
        err, amb = cr.velocity_error(out, lin1, ang1)
        worst, n_amb = max(worst, err), n_amb + amb
        check_stages(stages, "default")
        if u:
            assert len(out["a"]) == 400
            ok = ~out["ambiguous"]
            with_pn += int(((out["P0"][:, 0, 2] > 0) & ok).sum())
            with_pt += int(((out["P0"][:, 0, :2] != 0).any(1) & ok).sum())
            nx = np.abs(np.asarray(w.get_manifolds()[2])[:, 0])
            switched += int(((nx >= cr.BASIS_SWITCH) & (out["P0"][:, 0, 2] > 0) & ok).sum())
    print(f"\n{case}: error {worst:.3g} (tolerance {TOL_ISOLATED}), {n_amb} ambiguous; carried pn {with_pn}, friction {with_pt}")
    assert n_amb <= 20
    assert worst < TOL_ISOLATED
    if case == "turn3":
        assert with_pn == 0 and with_pt == 0
    elif case == "turn1":
        assert with_pn > 1500 and with_pt > 1500
    else:
        assert with_pn > 1500 and switched > 300 and with_pt < with_pn - 300


# ---------------------------------------------------------------- (c) coupled manifolds
def test_persistent_colouring_of_a_churning_scene():
    """130 updates of C3(12, 10, 12): colour counts, n_colors, color_rounds and n_new_manifolds of every update equal
    the persistent colouring restated from the device's own manifolds."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c3(12, 10, 12)
    w = physics_amd.World(sc.config())
    sc.populate(w)
    prev_keys = prev_colors = None
    churn, stages_seen = 0, set()
    for u in range(130):
        w.profile_enable(True)
        w.update(DT)
        w.sync()
        stages_seen |= set(w.profile_get()[0]) & SOLVER_STAGES
        m = cr.unpack_manifolds(w.get_manifolds())
        colors, n_colors, rounds, n_new = cr.color_manifolds(m["a"], m["b"], sc.n, prev_keys, prev_colors)
        prev_keys, prev_colors = m["keys"], colors
        st = w.get_stats()
        assert np.array_equal(w.get_color_counts(), cr.color_counts(colors)), u
        assert (st.n_colors, st.color_rounds, st.n_new_manifolds) == (n_colors, rounds, n_new), u
        churn += 0 < n_new < st.n_manifolds
    assert churn > 50 and n_colors >= 6
    assert stages_seen and stages_seen <= SOLVER_STAGES - {"solve_cluster"}, stages_seen


def _coupled(bodies, n_updates=6, flags=0, expect=("solve_flow",), iterations=8, ref=None, prepare=None, each=None, ground=True,
             **ref_args):
    """n_updates of a world of `bodies` under gravity with `flags` and `iterations`, each against `ref` (default: a warm
    SolverRef of as many iterations): colour counts, n_colors, color_rounds, n_new_manifolds, the stages that ran and the
    share of ambiguous manifolds are asserted here; returns (largest velocity error, most colours, manifolds of the last
    update). prepare(world) runs once behind set_bodies; each(u, world, out, lin1, ang1) once per update. `expect`: the
    stages of every update, or a function of the set that says whether they are right."""
    n = len(bodies["pos"])
    w = make_world(bodies, flags=flags, gravity=(0, -9.81, 0), ground=ground, solver_iterations=iterations)
    if prepare is not None:
        prepare(w)
    if ref is None:
        ref = cr.SolverRef(n, cr.Params(DT_S), iterations)
    worst, colors = 0.0, 0
    for u, (out, lin1, ang1, stages) in enumerate(checked_updates(w, ref, n_updates, *cr.body_inverses(n, bodies.get("mass"),
                                                                                                       bodies.get("inertia")), GRAVITY, **ref_args)):
        st = w.get_stats()
        assert st.overflow == 0, (u, st.overflow)
        assert np.array_equal(w.get_color_counts(), cr.color_counts(out["colors"]))
        assert (st.n_colors, st.color_rounds, st.n_new_manifolds) == (out["n_colors"], out["color_rounds"], out["n_new_manifolds"])
        # (update 1 may take another family: the cluster plan needs the counts of an update before)
        right = expect(stages) if callable(expect) else stages == set(expect)
        assert right or (u == 0 and len(stages) >= 1 and stages <= SOLVER_STAGES), (u, stages)
        err, amb = cr.velocity_error(out, lin1, ang1)
        assert amb <= 0.01 * len(out["a"])
        worst, colors = max(worst, err), max(colors, out["n_colors"])
        if each is not None:
            each(u, w, out, lin1, ang1)
    w.close()
    return worst, colors, len(out["a"])


@pytest.mark.parametrize("scene", ["c1_settled", "heap"])
def test_coupled_piles_in_colour_order(scene):
    """Six warm-started updates from a fresh world, through the dataflow kernels."""
    import physics_amd
    from physics_amd import scenes
    if scene == "heap":
        bodies = cr.random_heap(5)
    else:
        sc = scenes.c1()
        w0 = physics_amd.World(sc.config())
        sc.populate(w0)
        w0.update_n(DT, 300)
        w0.sync()
        pos, rot = w0.get_transforms()
        lin, ang = w0.get_velocities()
        w0.close()
        bodies = dict(pos=pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=sc.shape_type, half_extent=sc.half_extent)
    worst, colors, m = _coupled(bodies)
    print(f"\n{scene}: {m} manifolds, {colors} colours, error {worst:.3g} (tolerance {TOL_COUPLED})")
    assert colors >= 3
    assert worst < TOL_COUPLED


@pytest.mark.parametrize("solver", ["default", "per_color"])
def test_heap_in_a_static_container_against_the_float64_solver(solver):
    """Statics that several bodies share: contact_ref.random_heap inside contact_ref.heap_container - a floor slab under
    the whole heap and walls whose segments the outermost bodies touch - and no ground plane. contact_ref takes a partner
    with STATIC_ID_BIT for what it is: no body, like the ground (one-sided rows, no entry in `used` or `top`, the priority
    hashed from the full pair). Six warm-started updates; colour counts, n_colors, color_rounds and n_new_manifolds equal
    the reference's (asserted by _coupled), velocities within TOL_COUPLED as it stands: a static row has the form of a
    ground row, and that figure was measured on this heap resting on the ground plane (the twin scene; the oracle's spread
    there is 3.89e-6, tests/test_contact_ref_cpu.py::test_heap_container_and_its_twin_on_the_ground_plane).
    Measured on the GPU: 4.24e-6 through either solver.
    The 33k tower on the cluster solver is not repeated with shared statics:
    test_gpu_static.py::test_every_solver_path_gives_the_same_bits_in_a_static_container ties it to these two paths."""
    bodies = cr.random_heap(5)
    st = cr.heap_container(bodies)
    seen = dict(slab=0, both=0, walls=0)

    def each(u, w, out, lin1, ang1):
        b = out["b"]
        static = ((b & cr.STATIC_ID_BIT) != 0) & (b != cr.GROUND)
        assert not (b == cr.GROUND).any(), "no ground plane in this world"
        assert w.get_static_stats()[2] == static.sum()
        per_body = np.bincount(out["a"][static], minlength=len(bodies["pos"]))
        on_slab = np.bincount(out["a"][b == (cr.STATIC_ID_BIT | 0)], minlength=len(bodies["pos"])) > 0
        on_wall = np.bincount(out["a"][static & (b != (cr.STATIC_ID_BIT | 0))], minlength=len(bodies["pos"])) > 0
        seen["slab"] = max(seen["slab"], int(on_slab.sum()))
        seen["both"] = max(seen["both"], int((on_slab & on_wall).sum()))
        seen["walls"] = max(seen["walls"], int((per_body >= 2).sum()))

    expect = ("solve_flow",) if solver == "default" else (lambda stages: len(stages) >= 1 and stages <= PER_COLOR)
    worst, colors, m = _coupled(bodies, flags=flags_of(solver), expect=expect, ground=False, each=each,
                                prepare=lambda w: w.set_static_bodies(st["pos"], shape_type=st["shape_type"], half_extent=st["half_extent"]))
    print(f"\nheap in a static container, {solver}: {m} manifolds, {colors} colours, {seen['slab']} bodies on the slab, {seen['both']} on "
          f"the slab and a wall, {seen['walls']} with two static manifolds or more; error {worst:.3g} (tolerance {TOL_COUPLED})")
    assert seen["slab"] >= 50, "static manifolds on the floor slab alone"
    assert seen["both"] >= 5 and seen["walls"] >= 5, "bodies with two or more static manifolds (floor and wall)"
    assert colors >= 3
    assert worst < TOL_COUPLED


def test_cluster_kernels_on_the_tower():
    """C5(16, 130, 16) with PHYS_FLAG_SOLVER_CLUSTER: updates 2 to 6 through the cluster kernels, against the reference."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    bodies = dict(pos=sc.pos, shape_type=sc.shape_type, half_extent=sc.half_extent)
    worst, colors, m = _coupled(bodies, flags=physics_amd.FLAG_SOLVER_CLUSTER, expect=("solve_cluster",))
    print(f"\nC5 tower (cluster): {m} manifolds, {colors} colours, error {worst:.3g} (tolerance {TOL_TOWER})")
    assert m > 90_000
    assert worst < TOL_TOWER


# ---------------------------------------------------------------- (d) the cluster kernel with unequal bodies, cold and short
def varied_flags(warm, exclusive=False):
    import physics_amd
    return (physics_amd.FLAG_SOLVER_CLUSTER | (0 if warm else physics_amd.FLAG_NO_WARM_START) |
            (physics_amd.FLAG_EXCLUSIVE_GPU if exclusive else 0))


def varied_materials(n):
    """Seeded friction in [0.1, 1] and restitution 0 per body (the ground keeps the default 0.5)."""
    return np.random.default_rng(cr.VARIED_SEED + 1).uniform(0.1, 1.0, n).astype(np.float32)


def _warm_run_leaves_the_cold_solve(bodies, iterations, cold_front, cold_out):
    """Negative control of a cold case: the same bodies WITH warm starting. Update 1 carries nothing, so update 2 starts
    with the cold world's bits; what the warm world makes of them must lie far from the cold reference."""
    w = make_world(bodies, flags=varied_flags(True), gravity=(0, -9.81, 0), solver_iterations=iterations)
    w.update(DT)
    w.sync()
    front = (w.get_transforms()[0],) + tuple(w.get_velocities())
    assert all(np.array_equal(a, b) for a, b in zip(front, cold_front)), "update 1 of a warm world carries no impulses"
    w.update(DT)
    w.sync()
    lin1, ang1 = w.get_velocities()
    w.close()
    return max(np.abs(lin1 - cold_out["lin"]).max(), np.abs(ang1 - cold_out["ang"]).max())


VARIED_GPU_CASES = [(case, False) for case in cr.VARIED_CASES] + [("full", True)]


@pytest.mark.parametrize("case,exclusive", VARIED_GPU_CASES, ids=[c + ("_exclusive" if x else "") for c, x in VARIED_GPU_CASES])
def test_cluster_kernel_on_the_varied_tower(case, exclusive):
    """contact_ref.varied_tower with PHYS_FLAG_SOLVER_CLUSTER: every body has its own mass and inertia (one shared
    diagonal, a diagonal per body, full tensors: k_solve_cluster<true, ...> with stride 0 and 1, <false, ...>), guarded
    and unguarded starts, warm and cold solves of 8, 2 and 1 iterations. Updates 2 to 4 run the cluster kernel alone;
    every update is held to the float64 reference under TOL_VARIED (4 x the oracle's spread, test_contact_ref_cpu).
    Cold cases: a warm world on the same bodies does NOT match the cold reference (the flag is live)."""
    inertia, warm, iterations = cr.VARIED_CASES[case]
    bodies = cr.varied_tower(cr.VARIED_SEED, inertia)
    n = len(bodies["pos"])
    seen = {}

    def each(u, w, out, lin1, ang1):
        assert len(out["a"]) > 40_960
        if u == 1:
            seen["out"] = out
        if u == 0:
            seen["front"] = (w.get_transforms()[0], lin1, ang1)

    worst, colors, m = _coupled(bodies, n_updates=cr.VARIED_UPDATES, flags=varied_flags(warm, exclusive), expect=("solve_cluster",),
                                iterations=iterations, ref=cr.SolverRef(n, cr.Params(DT_S), iterations, warm=warm), each=each)
    print(f"\nvaried tower {case}{' exclusive' if exclusive else ''}: {m} manifolds, {colors} colours, error {worst:.3g} (tolerance {cr.TOL_VARIED:.3g})")
    assert colors >= 6
    assert worst < cr.TOL_VARIED
    if not warm:
        off = _warm_run_leaves_the_cold_solve(bodies, iterations, seen["front"], seen["out"])
        print(f"  a warm world differs from the cold reference by up to {off:.3g}")
        assert off > 10 * cr.TOL_VARIED


def test_cluster_kernel_with_materials_on_the_varied_tower():
    """k_solve_cluster<false, *, true>: full tensors and a friction coefficient per body (restitution 0), against
    tests/material_ref.py's solver - the contact reference with a friction per manifold."""
    import material_ref as mr
    bodies = cr.varied_tower(cr.VARIED_SEED, "full")
    n = len(bodies["pos"])
    fr = varied_materials(n)
    mats = mr.Materials(fr, np.zeros(n))
    mus = []
    worst, colors, m = _coupled(bodies, n_updates=cr.VARIED_UPDATES, flags=varied_flags(True), expect=("solve_cluster",),
                                ref=mr.MaterialSolverRef(n, cr.Params(DT_S), 8), prepare=lambda w: w.set_body_materials(friction=fr, restitution=0.0),
                                each=lambda u, w, out, lin1, ang1: mus.append(out["mu"]), materials=mats)
    print(f"\nvaried tower with materials: {m} manifolds, {colors} colours, mu {min(x.min() for x in mus):.3f} to "
          f"{max(x.max() for x in mus):.3f}, error {worst:.3g} (tolerance {cr.TOL_VARIED:.3g})")
    assert m > 40_960 and colors >= 6
    assert min(x.min() for x in mus) < 0.2 and max(x.max() for x in mus) > 0.9
    assert worst < cr.TOL_VARIED
