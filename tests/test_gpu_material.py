"""GPU: per-body materials - friction and restitution (include/physics_hip.h) on bodies, static
colliders and the ground.

The oracle has no materials. What stands in for it: the bits of worlds without materials (default materials change no bit;
one friction set through materials equals a world configured with that friction), tests/material_ref.py (the float64
statement of the combine and bias rules, written from the definitions) feeding tests/contact_ref.py (the float64
sequential-impulse reference), and closed forms (a one-point normal row is solved exactly by the first relaxation)."""
import numpy as np
import pytest

import contact_ref as cr
import material_ref as mr

pytestmark = pytest.mark.gpu
DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
G = (0.0, -9.81, 0.0)


def _pa():
    import physics_amd
    return physics_amd


def _world(bodies, statics=None, flags=0, ground=True, **cfg):
    pa = _pa()
    f = pa.FLAG_COLLISIONS | (pa.FLAG_GROUND_PLANE if ground else 0) | flags
    cfg.setdefault("gravity_force", G)
    w = pa.World(pa.default_config(flags=f, gravity_offset=(0.0, 0.0, 0.0), **cfg))
    w.set_bodies(**bodies)
    if statics is not None:
        w.set_static_bodies(statics[0], rot=statics[1], shape_type=statics[2], half_extent=statics[3])
    return w


def _state(w):
    return list(w.get_transforms()) + list(w.get_velocities())


def _same_manifolds(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _counters(w):
    s = w.get_stats()
    return (s.n_pairs, s.n_manifolds, s.n_contacts, s.n_colors)


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _heap(solver, seed=11, n=400):
    """(bodies, statics, flags, updates per comparison): a mixed heap of spheres, boxes and capsules beside three statics;
    for the cluster solver a 33k-box tower with capsules and two statics (enough resting contacts for that kernel)."""
    pa = _pa()
    if solver == "cluster":
        from physics_amd import scenes
        sc = scenes.c5(16, 130, 16)
        shape = sc.shape_type.copy()
        shape[::7] = pa.SHAPE_CAPSULE
        he = sc.half_extent.copy()
        he[::7] = [0.9, 0.1, 0.0]
        bodies = dict(pos=sc.pos, shape_type=shape, half_extent=he)
        statics = (np.array([[30.0, 1.0, 8.0], [-4.0, 0.5, 8.0]], np.float32), None, np.array([2, 3], np.uint32),
                   np.array([[1.0, 1.0, 1.0], [0.5, 1.0, 0.0]], np.float32))
        return bodies, statics, pa.FLAG_SOLVER_CLUSTER, 50
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-5.0, 5.0, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0.3, 6.0, n)
    shape = rng.choice([1, 2, 3, 0], n, p=[0.3, 0.35, 0.3, 0.05]).astype(np.uint32)
    he = rng.uniform(0.3, 0.7, (n, 3)).astype(np.float32)
    bodies = dict(pos=pos, rot=_quats(rng, n), shape_type=shape, half_extent=he)
    statics = (np.array([[2.0, 1.0, 2.0], [-3.0, 1.5, -2.0], [0.0, 2.0, -4.0]], np.float32),
               np.concatenate([np.array([[0, 0, 0, 1]], np.float32), _quats(rng, 2)]),
               np.array([2, 1, 3], np.uint32), np.array([[1.5, 0.5, 1.5], [1.0, 0, 0], [0.5, 1.5, 0]], np.float32))
    return bodies, statics, (0 if solver == "default" else pa.FLAG_SOLVER_PER_COLOR), 25


def _run_side_by_side(plain, mat, updates, chunk, label, want_cluster):
    if want_cluster:
        for w in (plain, mat):
            w.profile_enable(True)
    manifolds = 0
    for done in range(chunk, updates + 1, chunk):
        for w in (plain, mat):
            w.update_n(DT, chunk)
            w.sync()
        for a, b in zip(_state(plain), _state(mat)):
            assert np.array_equal(a, b), f"{label}: update {done} differs"
        ma, mb = plain.get_manifolds(), mat.get_manifolds()
        assert _same_manifolds(ma, mb), f"{label}: manifolds of update {done} differ"
        assert _counters(plain) == _counters(mat), f"{label}: counters of update {done} differ"
        manifolds = max(manifolds, len(ma[0]))
    assert manifolds > 100
    if want_cluster:
        assert "solve_cluster" in mat.profile_get()[0] and "solve_cluster" in plain.profile_get()[0]


# ---- 1. default materials change no bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["default", "per_color", "cluster"])
def test_default_materials_set_explicitly_change_no_bit(solver):
    """Materials (cfg.friction, 0) on bodies, statics and ground select the material kernels; transforms, velocities,
    manifolds and counters must equal those of a world that never made a material call, over 200 updates."""
    bodies, statics, flags, chunk = _heap(solver)
    n = len(bodies["pos"])
    plain = _world(bodies, statics, flags)
    mat = _world(bodies, statics, flags)
    f = mat.cfg.friction
    mat.set_body_materials(np.full(n, f, np.float32), np.zeros(n, np.float32))
    mat.set_static_materials(f, 0.0)
    mat.set_ground_material(f, 0.0)
    _run_side_by_side(plain, mat, 200, chunk, solver, solver == "cluster")
    plain.close()
    mat.close()


# ---- 2. one friction through the rows is the configured friction --------------------------------------------------------
@pytest.mark.parametrize("solver", ["default", "per_color", "cluster"])
@pytest.mark.parametrize("fr", [0.0, 0.2, 0.9])
def test_uniform_material_friction_equals_the_configured_friction(solver, fr):
    """A world created with cfg.friction = f' and no materials against a world with the default cfg.friction and the
    material f' everywhere: the per-row friction must produce the global friction's bits (the path the oracle verifies)."""
    bodies, statics, flags, chunk = _heap(solver, seed=12)
    plain = _world(bodies, statics, flags, friction=fr)
    mat = _world(bodies, statics, flags)
    assert mat.cfg.friction != fr
    mat.set_body_materials(friction=fr)
    mat.set_static_materials(friction=fr)
    mat.set_ground_material(fr, 0.0)
    _run_side_by_side(plain, mat, 2 * chunk, chunk, f"{solver} f'={fr}", solver == "cluster")
    plain.close()
    mat.close()


# ---- 3. bounce -----------------------------------------------------------------------------------------------------------
def _drop(speed, e_body, e_floor, on_static, updates=1):
    """A unit-mass sphere of radius 0.5 moving down at `speed`, 0.015 above the ground or above a static box (inside the
    contact margin: the first update holds the contact). No gravity. Returns what the update of impact saw and made."""
    pa = _pa()
    top = 2.0 if on_static else 0.0
    bodies = dict(pos=np.array([[0.0, top + 0.5 + 0.015, 0.0]], np.float32), lin_vel=np.array([[0.0, -speed, 0.0]], np.float32),
                  shape_type=np.array([pa.SHAPE_SPHERE], np.uint32), half_extent=np.array([[0.5, 0.5, 0.5]], np.float32))
    statics = (np.array([[0.0, 1.0, 0.0]], np.float32), None, np.array([pa.SHAPE_BOX], np.uint32), np.array([[2.0, 1.0, 2.0]], np.float32)) if on_static else None
    w = _world(bodies, statics, gravity_force=(0.0, 0.0, 0.0))
    if e_body is not None:
        w.set_body_materials(restitution=e_body)
    if e_floor is not None:
        (w.set_static_materials(restitution=e_floor) if on_static else w.set_ground_material(w.cfg.friction, e_floor))
    states = []
    for _ in range(updates):
        w.update(DT)
        w.sync()
        states.append(_state(w))
    man = w.get_manifolds()
    w.close()
    return man, states


@pytest.mark.parametrize("on_static", [False, True])
@pytest.mark.parametrize("e", [0.0, 0.3, 0.8])
def test_dropped_sphere_leaves_with_its_restitution_bias(e, on_static):
    """In the update of impact the outgoing normal velocity of a one-point manifold is that point's bias (the first
    relaxation solves the row exactly, later ones find nothing to do): relative 1e-5. Impact speed 3 > threshold 1; the
    point is speculative (gap 0.015 < 3 dt), so its push-out term is negative and the rebound e |vn| exceeds it."""
    speed = 3.0
    p = cr.Params(DT_S)
    for where in ("body", "floor"):  # the material on the sphere, then on the ground / static instead: max(e, 0) either way
        man, states = _drop(speed, e if where == "body" else 0.0, e if where == "floor" else 0.0, on_static)
        ids, counts, normals, points = man
        assert len(ids) == 1 and counts[0] == 1
        assert ids[0, 1] == (_pa().STATIC_ID_BIT if on_static else _pa().GROUND_ID)
        n = normals[0].astype(np.float64)
        depth = float(points[0, 0, 3])
        vn = float(n @ (0.0 - np.array([0.0, -np.float32(speed), 0.0])))
        push, rebound = mr.pushout_and_rebound(depth, vn, e, 1.0, p)
        want = float(mr.restitution_bias(depth, vn, e, 1.0, p))
        if e > 0.0:
            assert rebound > push and want == pytest.approx(e * speed, rel=1e-6)
        lin = states[0][2][0].astype(np.float64)
        got = float(n @ (0.0 - lin))
        print(f"\ne={e} on {where} static={on_static}: depth {depth:.6f} push-out {float(push):.6f} rebound {float(rebound):.6f} outgoing {got:.7f}")
        assert got == pytest.approx(want, rel=1e-5)


@pytest.mark.parametrize("on_static", [False, True])
def test_impact_below_the_threshold_equals_no_restitution(on_static):
    _, bouncy = _drop(0.8, 0.8, 0.5, on_static, updates=6)
    _, dead = _drop(0.8, 0.0, 0.0, on_static, updates=6)
    _, never = _drop(0.8, None, None, on_static, updates=6)
    for a, b, c in zip(bouncy, dead, never):
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    # ... and above it the same materials do bounce
    _, fast = _drop(3.0, 0.8, 0.5, on_static, updates=1)
    assert fast[0][2][0, 1] > 2.0


# ---- 4. two spheres head-on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [1.0, 0.0])
def test_two_spheres_head_on(e):
    """Equal masses, touching 0.005 deep (inside the slop: no push-out), approaching along x at 3 and -1. e = 1 exchanges
    the normal velocities, e = 0 leaves both with the common one; momentum is conserved to 1e-5 relative."""
    pa = _pa()
    bodies = dict(pos=np.array([[-0.4975, 5.0, 0.0], [0.4975, 5.0, 0.0]], np.float32),
                  lin_vel=np.array([[3.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], np.float32),
                  shape_type=np.full(2, pa.SHAPE_SPHERE, np.uint32), half_extent=np.full((2, 3), 0.5, np.float32))
    w = _world(bodies, ground=False, gravity_force=(0.0, 0.0, 0.0))
    w.set_body_materials(restitution=[e, 0.0])  # on one of them: max
    w.update(DT)
    w.sync()
    assert len(w.get_manifolds()[0]) == 1
    lin = w.get_velocities()[0].astype(np.float64)
    w.close()
    want = [[-1.0, 0, 0], [3.0, 0, 0]] if e == 1.0 else [[1.0, 0, 0], [1.0, 0, 0]]
    assert np.abs(lin - np.array(want)).max() < 1e-5 * 3.0, lin
    assert abs(lin[:, 0].sum() - 2.0) < 1e-5 * 4.0 and np.abs(lin[:, 1:]).max() < 1e-6


# ---- 5. sliding ----------------------------------------------------------------------------------------------------------
def test_sliding_box_stops_where_the_float64_reference_stops():
    """A unit cube sliding along x on the ground, friction 0.8 on the cube and 0.2 on the ground (mu = 0.4). Every update
    the float64 reference is given the device's manifolds and the device's state before the update; its velocities,
    summed, are the reference's path. 150 updates x 1e-4 (the velocity tolerance of tests/test_gpu_independent.py) x dt
    = 2.5e-4; the bound is 1e-3. The path also lies within 5 % of v0^2 / (2 mu g)."""
    pa = _pa()
    v0, fb, fg = 3.0, 0.8, 0.2
    bodies = dict(pos=np.array([[0.0, 0.495, 0.0]], np.float32), lin_vel=np.array([[v0, 0.0, 0.0]], np.float32),
                  shape_type=np.array([pa.SHAPE_BOX], np.uint32), half_extent=np.full((1, 3), 0.5, np.float32))
    w = _world(bodies)
    w.set_body_materials(friction=fb)
    w.set_ground_material(fg, 0.0)
    mats = mr.Materials([fb], [0.0], ground=(fg, 0.0))
    sref = mr.MaterialSolverRef(1, cr.Params(DT_S), 8)
    ref_path, worst = 0.0, 0.0
    for _ in range(150):
        pos, _ = w.get_transforms()
        lin, ang = w.get_velocities()
        w.update(DT)
        w.sync()
        out = sref.update(w.get_manifolds(), pos, lin, ang, np.ones(1), np.eye(3)[None], np.array(G), materials=mats)
        assert out["mu"][0] == pytest.approx(0.4)
        ref_path += out["lin"][0, 0] * DT_S
        worst = max(worst, np.abs(w.get_velocities()[0][0] - out["lin"][0]).max())
    x = float(w.get_transforms()[0][0, 0])
    v_end = w.get_velocities()[0][0]
    w.close()
    print(f"\nsliding: device {x:.6f} reference {ref_path:.6f} closed form {v0 * v0 / (2 * 0.4 * 9.81):.6f}; worst velocity error {worst:.3g}")
    assert worst < 1e-4  # every update's velocities against the reference's, before anything is summed
    assert abs(v_end[0]) < 1e-3, "the cube has stopped"
    assert abs(x - ref_path) < 1e-3
    assert abs(x - v0 * v0 / (2 * 0.4 * 9.81)) < 0.05 * v0 * v0 / (2 * 0.4 * 9.81)


@pytest.mark.parametrize("factor", [0.7, 1.3])
def test_box_on_a_static_ramp_sticks_below_and_slides_above_the_friction_angle(factor):
    """A cube resting on a static ramp tilted about z by atan(factor mu), mu = sqrt(0.9 x 0.4) = 0.6: well below the friction
    angle it creeps less than the slop (0.01) over 120 updates, well above it slides (closed form 0.5 a t^2 = 2.7)."""
    pa = _pa()
    f_box, f_ramp = 0.9, 0.4
    mu = float(np.sqrt(f_box * f_ramp))
    th = float(np.arctan(factor * mu))
    q = np.array([[0.0, 0.0, np.sin(th / 2), np.cos(th / 2)]], np.float32)
    up = np.array([-np.sin(th), np.cos(th), 0.0])
    centre = np.array([0.0, 10.0, 0.0])
    bodies = dict(pos=(centre + up * (0.5 + 0.5 - 0.005))[None].astype(np.float32), rot=q,
                  shape_type=np.array([pa.SHAPE_BOX], np.uint32), half_extent=np.full((1, 3), 0.5, np.float32))
    statics = (centre[None].astype(np.float32), q, np.array([pa.SHAPE_BOX], np.uint32), np.array([[8.0, 0.5, 2.0]], np.float32))
    w = _world(bodies, statics, ground=False)
    w.set_body_materials(friction=f_box)
    w.set_static_materials(friction=f_ramp)
    p0 = w.get_transforms()[0][0].astype(np.float64)
    w.update_n(DT, 120)
    w.sync()
    moved = float(np.linalg.norm(w.get_transforms()[0][0].astype(np.float64) - p0))
    assert len(w.get_manifolds()[0]) == 1
    w.close()
    print(f"\nramp at {np.degrees(th):.1f} deg (mu {mu:.2f} x {factor}): moved {moved:.5f}")
    if factor < 1.0:
        assert moved < 0.01
    else:
        a = 9.81 * (np.sin(th) - mu * np.cos(th))
        assert moved > 0.5 * (0.5 * a * 4.0) and moved < 1.1 * (0.5 * a * 4.0)


# ---- 6. a mixed heap of isolated manifolds against float64 ---------------------------------------------------------------
@pytest.mark.parametrize("inertia", ["identity", "full"])
@pytest.mark.parametrize("iterations", [1, 8])
def test_random_materials_on_isolated_manifolds_match_float64(iterations, inertia):
    """800 groups of (box on box, sphere on box, box on the ground), 4000 bodies, every body and the ground with a random
    material; upper bodies approach at up to 2 (some above the threshold 1, some below) and slide at up to 6. One update,
    no input left out. Velocities within 1e-4 absolute + 1e-4 relative of material_ref + contact_ref (the tolerance of
    tests/test_gpu_independent.py); the contact impulses conserve each pair's momentum."""
    bodies = cr.friction_pairs(21, 800, inertia=inertia)  # full: non-diagonal tensors, the kernels' general instances
    n = len(bodies["pos"])
    rng = np.random.default_rng(22)
    fr = rng.uniform(0.0, 1.2, n).astype(np.float32)
    re = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 1.0, n), 0.0).astype(np.float32)
    ground = (0.7, 0.4)
    w = _world(bodies, solver_iterations=iterations)
    w.set_body_materials(fr, re)
    w.set_ground_material(*ground)
    f2, e2 = w.get_body_materials()
    assert np.array_equal(f2, fr) and np.array_equal(e2, re)
    pos, _ = w.get_transforms()
    lin, ang = w.get_velocities()
    w.update(DT)
    w.sync()
    man = w.get_manifolds()
    lin1, ang1 = w.get_velocities()
    w.close()
    inv_m, inv_I = cr.body_inverses(n, bodies["mass"], bodies["inertia"])
    sref = mr.MaterialSolverRef(n, cr.Params(DT_S), iterations)
    out = sref.update(man, pos, lin, ang, inv_m, inv_I, np.array(G), materials=mr.Materials(fr, re, ground=ground))
    assert len(out["a"]) > 2000 and out["bounces"].any(1).sum() > 200 and (~out["bounces"].any(1)).sum() > 200
    assert not out["ambiguous"].any()  # one cold update: no warm-start decision; no normal at the basis switch
    err_v = np.abs(lin1 - out["lin"]) - 1e-4 * np.abs(out["lin"])
    err_w = np.abs(ang1 - out["ang"]) - 1e-4 * np.abs(out["ang"])
    print(f"\nit={iterations} {inertia}: {len(out['a'])} manifolds, {int(out['bounces'].any(1).sum())} bounce; worst |dv| {np.abs(lin1 - out['lin']).max():.3g} |dw| {np.abs(ang1 - out['ang']).max():.3g}")
    assert err_v.max() < 1e-4 and err_w.max() < 1e-4
    # momentum: each body-body pair is isolated, so what one gained the other lost (gravity's share taken out)
    mass = bodies["mass"].astype(np.float64)
    dp = mass[:, None] * (lin1.astype(np.float64) - lin.astype(np.float64)) - DT_S * np.array(G)  # (gravity is a force here: dv = dt F / m)
    bb = out["b"] != cr.GROUND
    a, b = out["a"][bb], out["b"][bb]
    scale = 1.0 + np.abs(dp[a]).max(1)
    assert (np.abs(dp[a] + dp[b]).max(1) < 1e-4 * scale).all()


# ---- 6b. every row-solver kernel's material instance, forced in a fresh process -----------------------------------------
def _probe(args, env_extra, timeout=900):
    """tools/material_probe.py in a fresh process (the library reads its PHYS_DEBUG_* switches once per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "material_probe.py")] + args, cwd=root,
                         env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("path,env,inertia", [
    ("percolour", {"PHYS_DEBUG_COLOR_KERNEL": "quad", "PHYS_DEBUG_NO_CLUSTER": "1"}, "identity"),  # k_solve_color_quad
    ("percolour", {"PHYS_DEBUG_COLOR_KERNEL": "lane", "PHYS_DEBUG_NO_CLUSTER": "1"}, "identity"),  # k_solve_color
    ("default", {"PHYS_DEBUG_NO_CLUSTER": "1"}, "identity"),                                       # k_solve_flow_quad
    ("default", {"PHYS_DEBUG_FLOW_QUAD_MAX": "1", "PHYS_DEBUG_NO_CLUSTER": "1"}, "identity"),      # k_solve_flow
    ("cluster", {}, "identity"),                                                                   # k_solve_cluster
    ("percolour", {"PHYS_DEBUG_COLOR_KERNEL": "quad", "PHYS_DEBUG_NO_CLUSTER": "1"}, "full"),      # the general-tensor instances
    ("percolour", {"PHYS_DEBUG_COLOR_KERNEL": "lane", "PHYS_DEBUG_NO_CLUSTER": "1"}, "full"),
    ("default", {"PHYS_DEBUG_FLOW_QUAD_MAX": "1", "PHYS_DEBUG_NO_CLUSTER": "1"}, "full"),
    ("cluster", {}, "full"),
], ids=["color_quad", "color_lane", "flow_quad", "flow_lane", "cluster", "color_quad_full", "color_lane_full", "flow_lane_full",
        "cluster_full"])
def test_each_row_solver_kernel_with_materials(path, env, inertia):
    """The small heaps above end in the tail kernel and the four-lane dataflow kernel, so they say nothing about
    k_solve_color, k_solve_color_quad and k_solve_flow. Each row kernel is forced here as
    tests/test_gpu_collision.py::test_each_row_solver_kernel_equals_the_oracle forces it, on the 33k tower whose colours
    exceed the tail's 512 rows, and its material instance must give (1) with default materials the bits of the plain
    instance, (2) with a uniform friction of 0, 0.2, 0.9 the bits of the world configured with it, (3) with random
    materials and a threshold low enough for settling contacts to bounce, three warm-started updates within 1e-4 of
    material_ref + contact_ref (the velocity tolerance of case 6), at most 1 % of the manifolds left out as ambiguous
    (a warm-start or tangent-basis decision within rounding of its threshold; the share is printed)."""
    out = _probe(["c5:16:130:16", "--path", path, "--pre", "4", "--steps", "8", "--ref", "3", "--inertia", inertia], env)
    print("\n" + out.strip())
    fields = dict(f.split("=", 1) for f in out.split())
    assert fields["defaults"] == "identical" and fields["uniform"] == "identical", out
    for key in ("plain_ran", "mat_ran", "ref_ran"):
        ran = set(fields[key].split("+"))
        if path == "percolour":
            assert "solve" in ran and ran <= {"solve", "solve_tail"}, out
        else:
            assert ran == {"solve_flow" if path == "default" else "solve_cluster"}, out
    assert int(fields["manifolds"]) > 90_000
    assert int(fields["ref_bounces"]) > 1000
    assert float(fields["ref_ambiguous"]) <= 0.01
    assert float(fields["ref_err"]) < 1e-4, out


# ---- 7. a pile at rest stays at rest ------------------------------------------------------------------------------------
def test_warm_started_column_with_restitution_stands_like_the_one_without():
    """The 12-cube column of tests/test_collide_kat.py with e = 0.5 on every cube and the ground, 240 updates: the bounds
    of that test (bottom cube at y = 1 to 2e-4, every cube within 0.03 of its lattice height, speeds below 0.1) - no
    resting contact approaches faster than the threshold."""
    from physics_amd import scenes
    pa = _pa()
    pos = scenes.lattice(1, 12, 1, 2.0, 1.0, 0.0)
    bodies = dict(pos=pos, shape_type=np.full(12, pa.SHAPE_BOX, np.uint32), half_extent=np.ones((12, 3), np.float32))
    out = {}
    for label in ("plain", "bouncy"):
        w = _world(bodies)
        if label == "bouncy":
            w.set_body_materials(restitution=0.5)
            w.set_ground_material(w.cfg.friction, 0.5)
        w.update_n(DT, 240)
        w.sync()
        out[label] = _state(w)
        w.close()
    y, v = out["bouncy"][0][:, 1], out["bouncy"][2]
    assert abs(y[0] - 1.0) < 2e-4 and np.abs(y - (1.0 + 2.0 * np.arange(12))).max() < 0.03, y
    assert np.abs(v).max() < 0.1
    # nothing ever exceeded the threshold, so the bits are the plain column's too
    assert all(np.array_equal(a, b) for a, b in zip(out["plain"], out["bouncy"]))


# ---- 8. housekeeping -------------------------------------------------------------------------------------------------------
def test_getters_resets_and_argument_errors():
    pa = _pa()
    bodies, statics, _, _ = _heap("default", seed=13, n=50)
    w = _world(bodies, statics)
    f0, e0 = w.get_body_materials()
    assert np.array_equal(f0, np.full(50, w.cfg.friction, np.float32)) and not e0.any()
    rng = np.random.default_rng(1)
    fr, re = rng.uniform(0, 2, 50).astype(np.float32), rng.uniform(0, 1, 50).astype(np.float32)
    w.set_body_materials(fr, re)
    assert all(np.array_equal(a, b) for a, b in zip(w.get_body_materials(), (fr, re)))
    w.set_body_materials(restitution=re)  # a missing array: that field's default
    assert np.array_equal(w.get_body_materials()[0], f0)
    w.set_static_materials([0.1, 0.2, 0.3], [0.0, 0.5, 1.0])
    lib, E = w.lib, pa._abi.PHYS_ERR_INVALID_ARG
    f32 = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(pa._abi.f32p)  # noqa: E731
    assert lib.phys_set_body_materials(w.h, 49, f32(fr), f32(re)) == E
    assert lib.phys_set_static_materials(w.h, 2, None, None) == E
    bad = fr.copy(); bad[7] = -0.1
    assert lib.phys_set_body_materials(w.h, 50, f32(bad), None) == E
    bad[7] = np.inf
    assert lib.phys_set_body_materials(w.h, 50, f32(bad), None) == E
    bad = re.copy(); bad[3] = 1.01
    assert lib.phys_set_body_materials(w.h, 50, None, f32(bad)) == E
    assert lib.phys_set_ground_material(w.h, -1.0, 0.0) == E and lib.phys_set_ground_material(w.h, 0.5, 2.0) == E
    assert lib.phys_set_restitution_threshold(w.h, -1.0) == E and lib.phys_set_restitution_threshold(w.h, float("nan")) == E
    assert lib.phys_get_body_materials(w.h, None, None) == 0
    # the failed calls changed nothing; phys_set_bodies resets the body materials
    assert np.array_equal(w.get_body_materials()[1], re)
    w.set_bodies(**bodies)
    f1, e1 = w.get_body_materials()
    assert np.array_equal(f1, f0) and not e1.any()
    w.close()


def test_resets_restore_the_plain_behaviour():
    """After phys_set_bodies / phys_set_static_bodies a world that had bouncy, slippery materials runs like a fresh one."""
    bodies, statics, _, _ = _heap("default", seed=14, n=200)
    fresh = _world(bodies, statics)
    used = _world(bodies, statics)
    used.set_body_materials(0.05, 0.9)
    used.set_static_materials(0.05, 0.9)
    used.update_n(DT, 20)
    used.sync()
    used.set_bodies(**bodies)
    used.set_static_bodies(statics[0], rot=statics[1], shape_type=statics[2], half_extent=statics[3])
    for w in (fresh, used):
        w.update_n(DT, 40)
        w.sync()
    assert all(np.array_equal(a, b) for a, b in zip(_state(fresh), _state(used)))
    fresh.close()
    used.close()


def test_a_change_between_updates_takes_effect_at_the_next_one_and_keeps_warm_starts():
    """Ten updates without materials, then e = 0.8 on the ground: the eleventh update equals, bit for bit, that of a world
    that had the (then inert) material from the start - colours and warm-start impulses survive the call - and a sphere
    arriving later bounces."""
    pa = _pa()
    bodies = dict(pos=np.array([[0.0, 0.5, 0.0], [4.0, 1.3, 0.0]], np.float32), lin_vel=np.array([[0, 0, 0], [0, 0, 0]], np.float32),
                  shape_type=np.full(2, pa.SHAPE_SPHERE, np.uint32), half_extent=np.full((2, 3), 0.5, np.float32))
    late, early = _world(bodies), _world(bodies)
    early.set_ground_material(early.cfg.friction, 0.8)
    ups = []
    for k in range(40):
        if k == 10:
            late.set_ground_material(late.cfg.friction, 0.8)
        for w in (late, early):
            w.update(DT)
            w.sync()
        if k < 10:
            continue  # (the falling sphere is still in the air; the resting one never exceeds the threshold)
        assert all(np.array_equal(a, b) for a, b in zip(_state(late), _state(early))), k
        ups.append(float(late.get_velocities()[0][1, 1]))
    assert max(ups) > 0.8 * 3.0, ups  # fell 0.8 (3.96 at impact less a step), left at about 0.8 of that
    late.close()
    early.close()


def test_identical_runs_give_identical_bits_and_queries_do_not_disturb_updates():
    bodies, statics, _, _ = _heap("default", seed=15, n=300)
    n = len(bodies["pos"])
    rng = np.random.default_rng(2)
    fr, re = rng.uniform(0, 1.5, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    runs = []
    for probe in (False, False, True):
        w = _world(bodies, statics)
        w.set_body_materials(fr, re)
        w.set_static_materials([0.3, 0.6, 0.9], [0.9, 0.0, 0.5])
        w.set_ground_material(0.8, 0.6)
        w.set_restitution_threshold(0.5)
        for _ in range(30):
            w.update_n(DT, 2)
            if probe:
                o = rng.uniform(-5, 5, (64, 3)).astype(np.float32)
                w.raycast(o, np.tile(np.array([[0, -1, 0]], np.float32), (64, 1)))
                w.overlap(np.full(8, 1, np.uint32), o[:8], half_extent=np.full((8, 3), 1.0, np.float32))
        w.sync()
        runs.append(_state(w) + list(w.get_manifolds()))
        w.close()
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
    assert np.abs(runs[0][2]).max() > 0.5  # things are still moving: the comparison is not of a settled scene


def test_sharded_worlds_refuse_materials():
    pa = _pa()
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, max_ghosts=16))
    w.set_bodies(np.zeros((4, 3), np.float32) + [[0, 1, 0]], shape_type=np.full(4, 1, np.uint32), half_extent=np.full((4, 3), 0.5, np.float32))
    U = pa._abi.PHYS_ERR_UNSUPPORTED
    out = np.zeros(4, np.float32)
    p = out.ctypes.data_as(pa._abi.f32p)
    assert w.lib.phys_set_body_materials(w.h, 4, None, None) == U
    assert w.lib.phys_get_body_materials(w.h, p, p) == U
    assert w.lib.phys_set_static_materials(w.h, 0, None, None) == U
    assert w.lib.phys_set_ground_material(w.h, 0.5, 0.5) == U
    assert w.lib.phys_set_restitution_threshold(w.h, 1.0) == U
    with pytest.raises(pa.world.PhysError):
        w.set_body_materials(restitution=0.5)
    w.close()
