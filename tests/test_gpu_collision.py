"""GPU parity of the collision stages through the C ABI against the CPU oracle.
These stages have no reference counterpart ("parity unpinned" by the reference); the bar is bit-exact
agreement with the oracle's sequential evaluation of the same specification (include/spec), plus the
analytic known answers of tests/test_collide_kat.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 16_666_667


def _worlds(cfg_fn):
    import physics_amd
    from oracle import binding as ob
    return physics_amd.World(cfg_fn()), ob.OracleWorld(cfg_fn(), trig=ob.TRIG_DET)


def _random_soup(n, seed, extent):
    import physics_amd
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-extent, extent, size=(n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    st = rng.integers(0, 3, size=n).astype(np.uint32)  # NONE / SPHERE / BOX
    he = rng.uniform(0.3, 1.2, size=(n, 3)).astype(np.float32)
    return pos, q, st, he


@pytest.mark.parametrize("n,extent", [(2, 1.0), (300, 6.0), (5000, 20.0), (20000, 30.0)])
def test_broadphase_pairs_and_aabbs(n, extent):
    import physics_amd
    pos, q, st, he = _random_soup(n, 100 + n, extent)
    cfg = lambda: physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS, max_pairs=64 * n + 4096)
    w, o = _worlds(cfg)
    for x in (w, o):
        x.set_bodies(pos, rot=q, shape_type=st, half_extent=he)
    assert np.array_equal(w.get_aabbs(), o.get_aabbs())
    pw, po = w.broadphase(), o.broadphase()
    assert pw.shape == po.shape and np.array_equal(pw, po)
    if n >= 300:
        assert len(pw) > n // 4  # the soup really overlaps


@pytest.mark.parametrize("name,n,box,he_hi", [
    ("cube", 60000, (45.0, 45.0, 45.0), 1.2),      # isotropic soup: the table's bits split evenly
    ("tower", 50000, (6.0, 300.0, 6.0), 1.2),      # 12 x 600 x 12: most of the bits go to y (grid_plan)
    ("slab", 50000, (150.0, 3.0, 150.0), 1.2),     # flat: hardly any bits for y - an axis of 4 cells wraps constantly
    ("dense", 40000, (10.0, 10.0, 10.0), 1.0),     # ~70 overlaps per body: regions beyond the LDS stage (global walk)
])
def test_broadphase_brick_kernel_against_the_oracle(name, n, box, he_hi):
    """Above 32768 bodies the pair search is one workgroup per brick of 4 x 4 x 4 cells with the brick's half-shell region
    staged in LDS (k_find_pairs_brick): the pair SET must equal the oracle's sort-and-sweep for every shape of scene -
    whatever the split of the bucket table over the axes, with cells that wrap, and where a region holds more records
    than the stage (those bricks walk global memory)."""
    import physics_amd
    rng = np.random.default_rng(len(name) + n)
    pos = (rng.uniform(-1.0, 1.0, size=(n, 3)) * np.array(box)).astype(np.float32)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    st = rng.integers(0, 3, size=n).astype(np.uint32)
    he = rng.uniform(0.3, he_hi, size=(n, 3)).astype(np.float32)
    cfg = lambda: physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS, max_pairs=96 * n)
    w, o = _worlds(cfg)
    for x in (w, o):
        x.set_bodies(pos, rot=q, shape_type=st, half_extent=he)
    pw, po = w.broadphase(), o.broadphase_grid()
    assert pw.shape == po.shape and np.array_equal(pw, po), (name, pw.shape, po.shape)
    assert len(pw) > n // 2


def test_broadphase_empty_and_none_shapes():
    import physics_amd
    cfg = physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS)
    w = physics_amd.World(cfg)
    w.set_bodies(np.zeros((5, 3), np.float32))  # all PHYS_SHAPE_NONE
    assert len(w.broadphase()) == 0


def test_pair_capacity_overflow_is_reported():
    import physics_amd
    n = 2000
    pos = np.zeros((n, 3), np.float32)  # everything overlaps everything
    st = np.full(n, physics_amd.SHAPE_SPHERE, np.uint32)
    he = np.ones((n, 3), np.float32)
    w = physics_amd.World(physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS, max_pairs=10000))
    w.set_bodies(pos, shape_type=st, half_extent=he)
    with pytest.raises(physics_amd.PhysError) as e:
        w.broadphase()
    assert e.value.code == -5


def _compare_state(w, o, what=""):
    for name, a, b in zip(("pos", "rot"), w.get_transforms(), o.get_transforms()):
        assert np.array_equal(a, b), f"{what} {name}: max abs diff {np.abs(a - b).max()}"
    for name, a, b in zip(("lin", "ang"), w.get_velocities(), o.get_velocities()):
        assert np.array_equal(a, b), f"{what} {name}: max abs diff {np.abs(a - b).max()}"


def _compare_manifolds(w, o):
    mw, mo = w.get_manifolds(), o.get_manifolds()
    for a, b, name in zip(mw, mo, ("ids", "counts", "normals", "points")):
        assert a.shape == b.shape, name
        assert np.array_equal(a, b), name
    sw, so = w.get_stats(), o.get_stats()
    for f in ("n_pairs", "n_manifolds", "n_contacts", "n_colors", "color_rounds"):
        assert getattr(sw, f) == getattr(so, f), f


def _run_scene(sc, steps, check_every):
    import physics_amd
    w, o = _worlds(sc.config)
    for x in (w, o):
        sc.populate(x)
    done = 0
    while done < steps:
        k = min(check_every, steps - done)
        w.update_n(DT, k)
        o.update_n(DT, k)
        done += k
        w.sync()
        _compare_state(w, o, f"{sc.name} step {done}")
        _compare_manifolds(w, o)
    return w, o


def test_c1_64_cubes_1000_steps_bit_exact():
    from physics_amd import scenes
    w, o = _run_scene(scenes.c1(), 1000, 100)
    assert w.get_stats().n_manifolds >= 64  # the pile is in contact


def test_mixed_spheres_boxes_bit_exact():
    from physics_amd import scenes
    _run_scene(scenes.c3(8, 6, 8), 400, 50)


def test_tower_resting_contact_bit_exact():
    from physics_amd import scenes
    _run_scene(scenes.c5(4, 40, 4), 300, 50)


def test_c2_10k_cubes_bit_exact():
    from physics_amd import scenes
    _run_scene(scenes.c2(), 150, 50)


def test_new_manifolds_stat_counts_the_pairs_without_a_manifold_in_the_update_before():
    """phys_stats.n_new_manifolds = manifolds of the last update whose pair had none in the update before (what the narrow
    phase could keep no colour and no starting impulses for): checked against the manifold ids of consecutive updates, on
    a pile that is still landing (hundreds of new contacts per update) and on a column at rest (none)."""
    import physics_amd
    from physics_amd import scenes
    for sc, pre, lo in ((scenes.c3(10, 8, 10), 40, 10), (scenes.c5(2, 12, 2), 400, 0)):
        w = physics_amd.World(sc.config())
        sc.populate(w)
        w.update_n(DT, pre)
        prev = {tuple(p) for p in w.get_manifolds()[0].tolist()}
        seen_new = 0
        for _ in range(6):
            w.update(DT)
            ids = {tuple(p) for p in w.get_manifolds()[0].tolist()}
            st = w.get_stats()
            assert st.n_new_manifolds == len(ids - prev), (st.n_new_manifolds, len(ids - prev), len(ids))
            seen_new += st.n_new_manifolds
            prev = ids
        assert seen_new >= lo
        w.close()


def test_tumbling_boxes_edge_contacts():
    """Rotated boxes with angular velocity dropped on each other: exercises the SAT edge axes,
    clipping and the reduction to 4 points."""
    import physics_amd
    rng = np.random.default_rng(3)
    n = 200
    pos = np.stack([rng.uniform(-4, 4, n), rng.uniform(1.5, 30, n), rng.uniform(-4, 4, n)], 1).astype(np.float32)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    ang = rng.normal(scale=1.5, size=(n, 3)).astype(np.float32)
    st = np.full(n, physics_amd.SHAPE_BOX, np.uint32)
    he = rng.uniform(0.4, 1.0, size=(n, 3)).astype(np.float32)
    cfg = lambda: physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_GROUND_PLANE,
                                             gravity_offset=(0, 0, 0), max_pairs=64 * n)
    w, o = _worlds(cfg)
    for x in (w, o):
        x.set_bodies(pos, rot=q, ang_vel=ang, shape_type=st, half_extent=he)
    for k in range(6):
        w.update_n(DT, 50)
        o.update_n(DT, 50)
        w.sync()
        _compare_state(w, o, f"tumble {50 * (k + 1)}")
        _compare_manifolds(w, o)
    assert w.get_stats().n_contacts > 50


def test_double_run_determinism():
    """Two GPU runs of the same scene give identical bits (race detector for the parallel stages)."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c3(10, 8, 10)
    out = []
    for _ in range(2):
        w = physics_amd.World(sc.config())
        sc.populate(w)
        w.update_n(DT, 200)
        w.sync()
        out.append(w.get_transforms())
        w.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_dataflow_and_per_colour_solver_are_bit_identical():
    """The single-launch dataflow solver (default) and one launch per colour class (PHYS_FLAG_SOLVER_PER_COLOR)
    apply the same updates to every body in the same order: identical bits, and both equal the oracle."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c3(20, 16, 20)
    worlds = [physics_amd.World(sc.config()),
              physics_amd.World(sc.config(flags=sc.flags | physics_amd.FLAG_SOLVER_PER_COLOR))]
    for w in worlds:
        sc.populate(w)
    for k in range(4):
        for w in worlds:
            w.update_n(DT, 60)
            w.sync()
        for a, b in zip(worlds[0].get_transforms() + worlds[0].get_velocities(),
                        worlds[1].get_transforms() + worlds[1].get_velocities()):
            assert np.array_equal(a, b), f"solver modes differ after {60 * (k + 1)} steps"
    assert worlds[0].get_stats().n_manifolds > sc.n  # a contact-rich state was reached
    prof = []
    for w in worlds:
        w.profile_enable(True)
        w.update_n(DT, 4)
        prof.append(w.profile_get()[0])
    assert "solve_flow" in prof[0] and "solve" not in prof[0]
    assert "solve_flow" not in prof[1] and ("solve" in prof[1] or "solve_tail" in prof[1])


def test_full_inertia_tensors_and_unequal_masses_bit_exact():
    """Non-diagonal inertia tensors and per-body masses: the general (non-DIAG) solver kernels, both modes."""
    import physics_amd
    rng = np.random.default_rng(11)
    n = 300
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(1.5, 25, n), rng.uniform(-5, 5, n)], 1).astype(np.float32)
    st = rng.integers(1, 3, size=n).astype(np.uint32)
    he = rng.uniform(0.5, 1.0, size=(n, 3)).astype(np.float32)
    mass = rng.uniform(0.5, 3.0, size=n).astype(np.float32)
    a = rng.normal(scale=0.2, size=(n, 3, 3))
    inertia = (np.eye(3)[None] * rng.uniform(0.5, 2.0, size=(n, 1, 1)) + a @ a.transpose(0, 2, 1)).astype(np.float32)
    for extra in (0, physics_amd.FLAG_SOLVER_PER_COLOR):
        cfg = lambda: physics_amd.default_config(
            flags=physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_GROUND_PLANE | extra, gravity_offset=(0, 0, 0),
            max_pairs=64 * n)
        w, o = _worlds(cfg)
        for x in (w, o):
            x.set_bodies(pos, mass=mass, inertia=inertia.reshape(n, 9), shape_type=st, half_extent=he)
        for k in range(4):
            w.update_n(DT, 50)
            o.update_n(DT, 50)
            w.sync()
            _compare_state(w, o, f"full inertia, flags +{extra}, step {50 * (k + 1)}")
        assert w.get_stats().n_contacts > 50


def test_dataflow_solver_under_concurrent_load():
    """The inter-workgroup hand-off of k_solve_flow (data-tagged 16-byte granules, sc1 stores / loads) must not
    depend on timing: step a contact-rich scene while another stream keeps the memory system and the CUs busy
    with unrelated copies and GEMMs (uneven load is where a missing fence or a stale L1 line shows up), and
    compare every bit with the per-colour path run on a quiet GPU."""
    import torch
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c2()
    quiet = physics_amd.World(sc.config(flags=sc.flags | physics_amd.FLAG_SOLVER_PER_COLOR))
    sc.populate(quiet)
    quiet.update_n(DT, 260)
    quiet.sync()
    ref = quiet.get_transforms() + quiet.get_velocities()
    quiet.close()

    busy = physics_amd.World(sc.config())
    sc.populate(busy)
    side = torch.cuda.Stream()
    a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    m = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    for k in range(26):
        with torch.cuda.stream(side):
            for _ in range(3):
                b.copy_(a, non_blocking=True)
                m2 = m @ m
        busy.update_n(DT, 10)
        if k % 5 == 0:
            busy.sync()
    busy.sync()
    torch.cuda.synchronize()
    del m2
    prof_on = busy.get_stats()
    assert prof_on.overflow == 0
    for x, y in zip(busy.get_transforms() + busy.get_velocities(), ref):
        assert np.array_equal(x, y)


def test_small_scene_kernels_outgrown_between_two_hints():
    """The one-workgroup kernels of small scenes (k_color_small) are chosen from a LAGGED manifold count. A layer
    of 143 x 143 touching cubes (40 612 face-neighbour manifolds: just "small"; the edge-touching diagonals are slivers,
    collide.h) lands on the plane in one step (+20 449 ground manifolds): for a few steps the kernels meet more manifolds
    than they were sized for and must still produce the exact colouring, order and solve."""
    from physics_amd import scenes
    nx = 143
    pos = scenes.lattice(nx, 1, nx, 2.0, 1.2, 0.0)
    st, he = scenes._cubes(pos.shape[0])
    sc = scenes.Scene("one_layer", pos, st, he, scenes.FLAG_COLLISIONS | scenes.FLAG_GROUND_PLANE)
    w, o = _worlds(sc.config)
    for x in (w, o):
        sc.populate(x)
    seen = []
    for k in range(8):
        w.update_n(DT, 3)
        o.update_n(DT, 3)
        w.sync()
        seen.append(w.get_stats().n_manifolds)
        _compare_state(w, o, f"one layer, step {3 * (k + 1)}")
        _compare_manifolds(w, o)
    assert min(seen) <= 40960 < max(seen), seen  # the limit of the one-workgroup kernels (kSmallTrips * 1024)


def test_c2_10k_cubes_1000_steps_north_star_tolerance():
    """BASELINE.json north_star: "body transforms within 1e-4 relative of the CPU reference over 1000 steps", on the
    benchmark scene itself (C2, 10 000 cubes). The tolerance written out: max |x_gpu - x_cpu| <= 1e-4 * max(1, |x_cpu|)
    on positions and quaternions after 1000 steps. The implementation does better - the bits are equal - and that is
    asserted as well (every 250 steps), so a regression shows up as 'no longer exact' long before it reaches 1e-4."""
    from physics_amd import scenes
    sc = scenes.c2()
    w, o = _worlds(sc.config)
    for x in (w, o):
        sc.populate(x)
    for k in range(4):
        w.update_n(DT, 250)
        o.update_n(DT, 250)
        w.sync()
        for name, a, b in zip(("pos", "rot"), w.get_transforms(), o.get_transforms()):
            tol = 1.0e-4 * np.maximum(1.0, np.abs(b))
            assert (np.abs(a.astype(np.float64) - b) <= tol).all(), f"{name} beyond 1e-4 relative after {250 * (k + 1)} steps"
        _compare_state(w, o, f"C2 step {250 * (k + 1)}")
    assert w.get_stats().n_manifolds > 10000


@pytest.mark.parametrize("scene", ["c1", "tower", "mixed"])
def test_cold_solver_flag_equals_the_oracle_too(scene):
    """PHYS_FLAG_NO_WARM_START (the solver of rounds 1-2: every update from zero impulses, no sweep 0) stays a supported
    path: bit for bit against the oracle run with the same flag - and different from the warm-started run."""
    import physics_amd
    from physics_amd import scenes
    sc = {"c1": scenes.c1, "tower": lambda: scenes.c5(4, 40, 4), "mixed": lambda: scenes.c3(8, 6, 8)}[scene]()
    sc.flags |= physics_amd.FLAG_NO_WARM_START
    w, o = _run_scene(sc, 200, 50)
    warm = physics_amd.World(sc.config(flags=sc.flags & ~physics_amd.FLAG_NO_WARM_START))
    sc.populate(warm)
    warm.update_n(DT, 200)
    warm.sync()
    assert not np.array_equal(warm.get_transforms()[0], w.get_transforms()[0]), "the flag changed nothing"


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_solver_iteration_counts(iterations):
    """Tickets of the dataflow solver are iteration * degree + rank: the first and the last iteration are special
    (plain velocity record in, plain record out), so 1, 2 and 5 iterations exercise what 8 does not."""
    from physics_amd import scenes
    sc = scenes.c3(6, 5, 6)
    sc.solver_iterations = iterations
    w, o = _run_scene(sc, 200, 50)
    assert w.get_stats().n_manifolds > 100


def test_one_lane_dataflow_kernel_with_full_inertia_tensors():
    """More than 64k manifolds (below: four lanes per manifold) AND non-diagonal inertia tensors: k_solve_flow<false>
    (the general instance of the one-lane-per-manifold dataflow kernel), which no benchmark scene reaches."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5(16, 100, 16)
    rng = np.random.default_rng(21)
    n = sc.n
    a = rng.normal(scale=0.15, size=(n, 3, 3))
    inertia = (np.eye(3)[None] * rng.uniform(0.6, 1.5, size=(n, 1, 1)) + a @ a.transpose(0, 2, 1)).astype(np.float32)
    mass = rng.uniform(0.7, 1.4, size=n).astype(np.float32)
    w, o = _worlds(sc.config)
    for x in (w, o):
        x.set_bodies(sc.pos, mass=mass, inertia=inertia.reshape(n, 9), shape_type=sc.shape_type, half_extent=sc.half_extent)
    for k in range(3):
        w.update_n(DT, 8)
        o.update_n(DT, 8)
        w.sync()
        _compare_state(w, o, f"tower with full inertia, step {8 * (k + 1)}")
    assert w.get_stats().n_manifolds > 64000
    w.profile_enable(True)
    w.update_n(DT, 2)
    assert "solve_flow" in w.profile_get()[0]


def test_every_step_under_a_concurrent_gemm():
    """A bf16 GEMM (hipBLASLt, MFMA) is launched on another stream right before every step of one world; a second
    world steps quietly. Both are synchronised after every step (the way a frame loop uses the library) and must stay
    bit-identical. This failed in most runs while the kernels contained packed fp32 instructions (v_pk_mul_f32 /
    v_pk_add_f32): next to MFMA waves those returned slightly wrong values for 16 lanes at a time (DESIGN.md section 8;
    tools/frozen_probe.py and tools/race_probe.py are the diagnostic forms of this test). The library is built
    without them - tests/test_build_rules.py holds that on the CPU."""
    import torch
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c2()
    busy, quiet = physics_amd.World(sc.config()), physics_amd.World(sc.config())
    for w in (busy, quiet):
        sc.populate(w)
    side = torch.cuda.Stream()
    m = torch.randn(2048, 2048, device="cuda", dtype=torch.bfloat16)
    for step in range(1, 301):
        with torch.cuda.stream(side):
            m2 = m @ m
            m3 = m2 @ m
        busy.update(DT)
        busy.sync()
        torch.cuda.synchronize()
        quiet.update(DT)
        quiet.sync()
        if step % 10 == 0 or step > 30:
            sa, sb = busy.get_stats(), quiet.get_stats()
            assert (sa.n_pairs, sa.n_manifolds, sa.n_contacts) == (sb.n_pairs, sb.n_manifolds, sb.n_contacts), f"step {step}"
    for x, y in zip(busy.get_transforms() + busy.get_velocities(), quiet.get_transforms() + quiet.get_velocities()):
        assert np.array_equal(x, y)


def test_frozen_scene_gives_the_same_manifolds_every_step_under_a_concurrent_gemm():
    """The collision stages with time taken out (tools/frozen_probe.py as a test): a settled C2 stack in a world with
    zero gravity, zero velocities and zero solver iterations never moves, so every step must produce the manifolds of
    the first step, bit for bit - here with a bf16 GEMM on a second stream before every step. With packed fp32
    instructions in the narrow phase 1-6 steps in 400 did not (16 manifolds each, clip planes off by 1e-4):
    DESIGN.md section 8."""
    import torch
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c2()
    rolled = physics_amd.World(sc.config())
    sc.populate(rolled)
    rolled.update_n(DT, 120)
    rolled.sync()
    pos, rot = rolled.get_transforms()
    frozen = physics_amd.World(sc.config(gravity_force=(0.0, 0.0, 0.0), solver_iterations=0))
    frozen.set_bodies(pos, rot=rot, shape_type=sc.shape_type, half_extent=sc.half_extent)

    def snapshot():
        ids, cnt, nrm, pts = frozen.get_manifolds()
        order = np.argsort(ids[:, 0].astype(np.uint64) << np.uint64(32) | ids[:, 1])
        live = np.arange(4)[None, :] < cnt[order][:, None]
        return ids[order], cnt[order], nrm[order], np.where(live[..., None], pts[order], 0)

    frozen.update(DT)
    frozen.sync()
    first = snapshot()
    assert len(first[0]) > 5000
    side = torch.cuda.Stream()
    m = torch.randn(2048, 2048, device="cuda", dtype=torch.bfloat16)
    for step in range(2, 401):
        with torch.cuda.stream(side):
            m2 = m @ m
            m3 = m2 @ m
        frozen.update(DT)
        frozen.sync()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(), first):
            assert got.shape == want.shape and np.array_equal(got, want), f"step {step}"
    p1, r1 = frozen.get_transforms()
    assert np.array_equal(p1, pos) and np.array_equal(r1, rot)


def test_cluster_solver_bit_exact_against_the_oracle_on_a_33k_tower():
    """The cluster solver (cluster.hip: body velocities resident in LDS per spatial cluster, one launch for all
    iterations and colours, tagged granules only for bodies updated by another cluster's rows) takes over where contacts
    are dense and plentiful (from 170k manifolds; asked for here with PHYS_FLAG_SOLVER_CLUSTER): a 16 x 130 x 16 tower of
    boxes in resting contact (33 280 bodies, ~100k manifolds). Same arithmetic, same order of updates per body as every
    other solver path: poses, velocities and counters equal the sequential CPU oracle's bit for bit."""
    import physics_amd
    from oracle import binding as ob
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    w = physics_amd.World(sc.config(flags=sc.flags | physics_amd.FLAG_SOLVER_CLUSTER))
    o = ob.OracleWorld(sc.config(), trig=ob.TRIG_DET)
    o.set_threads(16)
    for x in (w, o):
        sc.populate(x)
    w.update_n(DT, 8)
    o.update_n(DT, 8)
    w.profile_enable(True)
    w.update_n(DT, 4)
    o.update_n(DT, 4)
    w.sync()
    prof, _ = w.profile_get()
    assert "solve_cluster" in prof, f"the cluster solver did not run: {sorted(prof)}"
    for a, b in zip(w.get_transforms() + w.get_velocities(), o.get_transforms() + o.get_velocities()):
        assert np.array_equal(a, b)
    sw, so = w.get_stats(), o.get_stats()
    assert (sw.n_pairs, sw.n_manifolds, sw.n_contacts, sw.n_colors) == (so.n_pairs, so.n_manifolds, so.n_contacts, so.n_colors)
    assert sw.n_manifolds > 90_000


def test_guarded_start_of_the_cluster_solver_changes_nothing():
    """The default start of the cluster solver (also implied by a second world on the device): every workgroup of the launch
    is counted in before anything is written, and a launch that cannot be resident as a whole is called off and tried again
    (other streams' kernels beside the start of a launch leave register holes that cost it workgroups: DESIGN.md).
    PHYS_FLAG_EXCLUSIVE_GPU skips the count. Same bits with and without, and the cluster solver runs in both."""
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    states = []
    for extra in (physics_amd.FLAG_EXCLUSIVE_GPU, 0):
        w = physics_amd.World(sc.config(flags=sc.flags | extra | physics_amd.FLAG_SOLVER_CLUSTER))
        sc.populate(w)
        w.update_n(DT, 8)
        w.profile_enable(True)
        w.update_n(DT, 6)
        w.sync()
        prof, _ = w.profile_get()
        assert "solve_cluster" in prof
        states.append(w.get_transforms() + w.get_velocities())
        w.close()
    for a, b in zip(states[0], states[1]):
        assert np.array_equal(a, b)


def test_cluster_solver_under_a_stream_of_foreign_kernels():
    """The case the guarded start (the default) is for: bf16 GEMMs and small element-wise kernels are launched on another stream
    right before every update of a 33k tower on the cluster solver, so that some of them run beside the START of its
    launch. No hand-off time-out, and the same bits as a world stepping on a quiet GPU."""
    import torch
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    busy = physics_amd.World(sc.config(flags=sc.flags | physics_amd.FLAG_SOLVER_CLUSTER))
    sc.populate(busy)
    side = torch.cuda.Stream()
    m = torch.randn(1024, 1024, device="cuda", dtype=torch.bfloat16)
    v = torch.zeros(1 << 20, device="cuda")
    for step in range(40):
        with torch.cuda.stream(side):
            for _ in range(6):
                m2 = m @ m
                v.add_(1.0)
        busy.update(DT)
        if step % 8 == 7:
            busy.sync()  # raises on a time-out
    busy.sync()
    torch.cuda.synchronize()
    busy_state = busy.get_transforms() + busy.get_velocities()
    busy.close()
    quiet = physics_amd.World(sc.config())  # (the dataflow kernel at this size: one more path with the same bits)
    sc.populate(quiet)
    quiet.update_n(DT, 40)
    quiet.sync()
    for a, b in zip(busy_state, quiet.get_transforms() + quiet.get_velocities()):
        assert np.array_equal(a, b)
    quiet.close()


@pytest.mark.parametrize("cap", ["", "9000"])
def test_dynamic_clusters_equal_the_per_colour_kernels(cap):
    """Scenes whose bodies outnumber the chip's LDS (the 1M-cube drop) get DYNAMIC clusters: homes are dealt out every
    update to the bodies that have a manifold in it, in the broad phase's bucket order; a row belongs to the home of its
    body A, else of B; a body without a home (more active bodies than homes) is served as "another cluster's body" on
    whichever side it stands. Forced here on a 33k tower in a fresh process (the library reads the switches once), with
    homes for everybody and with PHYS_DEBUG_CLUSTER_CAP=9000: the same bits as the per-colour kernels. (A cluster has 64
    slots at least, so on 256 CUs the cap still leaves 672 x 64 homes with these diagonal tensors - nobody is homeless;
    tests/test_gpu_cluster_variants.py has the combinations of switches that leave bodies without a home.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PHYS_DEBUG_CLUSTER_DYNAMIC="1")
    if cap:
        env["PHYS_DEBUG_CLUSTER_CAP"] = cap
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "dynamic_cluster_probe.py")], cwd=root, env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "identical cluster_ran True per_colour_ran_cluster False" in out.stdout, out.stdout + out.stderr


def _probe(args, env_extra, timeout=900):
    """tools/solver_probe.py in a fresh process (the library reads its PHYS_DEBUG_* switches once per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "solver_probe.py")] + args, cwd=root,
                         env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("a,b,env", [
    ("percolour", "default", {"PHYS_DEBUG_COLOR_KERNEL": "quad"}),  # k_solve_color_quad for every colour above the tail
    ("percolour", "default", {"PHYS_DEBUG_COLOR_KERNEL": "lane"}),  # k_solve_color
    ("default", "percolour", {}),                                   # k_solve_flow_quad
    ("default", "percolour", {"PHYS_DEBUG_FLOW_QUAD_MAX": "1"}),    # k_solve_flow
], ids=["color_quad", "color_lane", "flow_quad", "flow_lane"])
def test_each_row_solver_kernel_equals_the_oracle(a, b, env):
    """The profile names both per-colour kernels "solve" and both dataflow kernels "solve_flow", so a scene that picks
    one of them says nothing about the other. Each kernel is forced here on a 33k tower whose colours exceed the tail's
    512 rows (cluster solver off), against the other solver path and the oracle."""
    out = _probe(["c5:16:130:16", "--pre", "4", "--steps", "8", "--a", a, "--b", b, "--oracle"],
                 dict(env, PHYS_DEBUG_NO_CLUSTER="1"))
    fields = dict(f.split("=", 1) for f in out.split()[1:])
    ran = {p: set(fields[k].split("+")) for p, k in ((a, "a_ran"), (b, "b_ran"))}
    assert out.startswith("identical") and fields["oracle"] == "identical", out
    assert ran["default"] == {"solve_flow"}, out
    assert "solve" in ran["percolour"] and ran["percolour"] <= {"solve", "solve_tail"}, out


@pytest.mark.parametrize("per_cu,rows", [("3", "fewer than 256"), ("1", "257 to 512")])
def test_cluster_rows_read_back_by_the_lane_that_stored_them(per_cu, rows):
    """Regression for round 2's d106316 (`s_waitcnt vmcnt(0)` before a lane re-reads the impulses and masses of the row
    it has just stored): a lane of the cluster kernel solves rows l, l + 256, ... of its cluster and reads its own stores
    of the previous iteration back. With FEWER rows than lanes the next row IS the one just stored (a few instructions
    earlier); with 257-512 rows a lane's two rows alternate. A 33k tower forced onto the cluster solver has ~143 rows per
    cluster at three workgroups per CU and ~430 at one: eight iterations, against the per-colour kernels AND the oracle."""
    out = _probe(["c5:16:130:16", "--pre", "4", "--steps", "8", "--a", "cluster", "--b", "percolour", "--oracle"],
                 {"PHYS_DEBUG_CLUSTERS_PER_CU": per_cu})
    assert out.startswith("identical a_ran=solve_cluster b_ran=solve") and "oracle=identical" in out, out


def test_tag_epoch_wrap_on_a_cluster_step():
    """the 16-bit tag epoch wraps every 65535 solves; the reset zeroes row_acc = planes 12-15 of the row
    allocation, where k_rows_build has just put the constants of foreign bodies on a cluster step - the reset now runs
    ahead of that kernel. Started two solves before the wrap (PHYS_DEBUG_FLOW_EPOCH), the cluster solver must still equal
    the per-colour kernels (which carry no tags) over the steps around it."""
    out = _probe(["c5:16:130:16", "--pre", "0", "--steps", "8", "--a", "cluster", "--b", "percolour"],
                 {"PHYS_DEBUG_FLOW_EPOCH": str(0xFFFC)})
    assert out.startswith("identical a_ran=solve_cluster"), out


def test_crowded_colour_table_still_equals_the_oracle_and_a_full_one_is_reported():
    """The persistent colour table is open addressing with BOUNDED walks (a full chain must end a look-up, not hang a
    wave). Shrunk by PHYS_DEBUG_CTAB_SLOTS to barely more slots than the scene has manifolds (load ~0.9: long chains of
    live and dead entries) the run still equals the oracle bit for bit; shrunk below the manifold count an insert gives
    up - and says so (overflow bit 6 -> PHYS_ERR_CAPACITY, solve of that step skipped): never a silent divergence from
    the oracle's map, which keeps every colour."""
    # c3 12 x 10 x 12 settles at ~2.3k manifolds, churning every step: load 0.56 of 4096 slots - plus the dead entries of
    # up to 64 updates (the table is rebuilt every 64th)
    out = _probe(["c3:12:10:12", "--pre", "100", "--steps", "100", "--a", "default", "--b", "percolour", "--oracle"],
                 {"PHYS_DEBUG_CTAB_SLOTS": "4096"})
    assert out.startswith("identical") and "oracle=identical" in out, out
    assert 1800 < int(out.split("manifolds=")[1].split()[0]) < 4096, out
    # c3 15 x 10 x 15: ~3.9k manifolds (load 0.95): live and dead entries may well fill every slot between two rebuilds,
    # and a look-up of an absent key then walks the whole table - either outcome is fine, a wrong colouring is not
    out = _probe(["c3:15:10:15", "--pre", "100", "--steps", "60", "--a", "default", "--b", "percolour", "--oracle"],
                 {"PHYS_DEBUG_CTAB_SLOTS": "4096"})
    assert (out.startswith("identical") and "oracle=identical" in out) or out.startswith("error -5 overflow=64"), out
    out = _probe(["c3:12:10:12", "--pre", "100", "--steps", "50", "--a", "default", "--expect-error"],
                 {"PHYS_DEBUG_CTAB_SLOTS": "1024"})
    assert out.startswith("error -5") and int(out.split("overflow=")[1]) & 64, out
