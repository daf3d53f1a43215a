"""The configurations that tests/test_dynamics_ref_cpu.py (oracle against float64) and
tests/test_gpu_dynamics_independent.py (kernels against float64 and the oracle) share: seeded inputs, one driver that
feeds any world (physics_amd.World or oracle.binding.OracleWorld - same method names), and the float64 trajectories of
tests/dynamics_ref.py, computed once per configuration and never modified."""
import functools

import numpy as np

import dynamics_ref as dr

DT = 16_666_667
UPDATES = 50
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)  # either side of one wave and of one 256-thread block; several blocks
FORCES = ("off", "both", "force", "torque")
INERTIA = ("shared", "diag", "full")
GRAVITY_FORCE = (0.0, float(np.float32(-9.81)), 0.0)   # physics.rs:90, the float32 the worlds hold
GRAVITY_OFFSET = (0.0, 0.0, 1.5)    # physics.rs:91
CG_MAX_ERROR, CG_MIN_ERROR = 1e-2, 1e-3  # sle_solver.rs:6-7
# force-only worlds start with torque in two accumulators, so that "set_forces(force) leaves the torques alone" is seen
SEED_FORCE = np.array([0.5, -1.0, 0.25], np.float32)
SEED_OFFSET = np.array([0.3, 0.0, -0.2], np.float32)
SPHERE_RADIUS = 1e-3  # collision worlds: every eighth body is a tiny sphere, the others have no shape
SPHERE_STRIDE = 8
QUANTITIES = ("pos", "rot", "lin", "ang", "inst")


def random_state(n, seed):
    """The draw of tests/test_gpu_integrate.py: every seventh angular velocity is zero."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(scale=5.0, size=(n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    lin = rng.normal(size=(n, 3)).astype(np.float32)
    ang = rng.normal(scale=2.0, size=(n, 3)).astype(np.float32)
    ang[::7] = 0.0
    mass = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
    return pos, q, lin, ang, mass


def inertia_for(layout, n, seed):
    """(tensor for dynamics_ref.State, (n, 9) float32 tensor for set_bodies)."""
    rng = np.random.default_rng(seed)
    if layout == "shared":  # one diagonal tensor, not the identity: inertia_stride 0 reads entry 0 for everybody
        d = np.tile(np.array([2.0, 3.0, 0.5], np.float32), (n, 1))
    elif layout == "diag":  # a diagonal per body: inertia_stride 1
        d = rng.uniform(0.5, 4.0, size=(n, 3)).astype(np.float32)
    else:
        full = np.tile(np.eye(3, dtype=np.float32) * 2.0, (n, 1, 1)) + rng.normal(scale=0.2, size=(n, 3, 3)).astype(np.float32)
        return full.reshape(n, 9), full.reshape(n, 9)
    full = np.zeros((n, 3, 3), np.float32)
    full[:, 0, 0], full[:, 1, 1], full[:, 2, 2] = d[:, 0], d[:, 1], d[:, 2]
    return d, full.reshape(n, 9)


def integrator_inputs(n, inertia):
    pos, q, lin, ang, mass = random_state(n, 4321 + n)
    ref_inertia, world_inertia = inertia_for(inertia, n, 77 + n)
    return dict(pos=pos, rot=q, lin=lin, ang=ang, mass=mass, ref_inertia=ref_inertia, inertia=world_inertia)


def force_schedule(n, forces, k):
    """(force, torque) handed to set_forces before update k; None = that side is not passed."""
    if forces == "off":
        return None, None
    rng = np.random.default_rng(100_000 * n + k)
    F = rng.normal(scale=5.0, size=(n, 3)).astype(np.float32)
    T = rng.normal(scale=2.0, size=(n, 3)).astype(np.float32)
    return (F if forces in ("both", "force") else None), (T if forces in ("both", "torque") else None)


def shapes_for(n):
    st = np.zeros(n, np.uint32)
    st[::SPHERE_STRIDE] = 1  # SHAPE_SPHERE
    he = np.zeros((n, 3), np.float32)
    he[::SPHERE_STRIDE] = SPHERE_RADIUS
    return st, he


def snapshot(world):
    pos, rot = world.get_transforms()
    lin, ang = world.get_velocities()
    f, t = world.get_forces()
    return dict(pos=pos, rot=rot, lin=lin, ang=ang, force=f, torque=t, inst=world.get_instance_matrices())


def drive_integrator(world, n, forces, mode, inertia, checkpoints=(1, UPDATES)):
    """Run UPDATES updates on `world`; mode "update" / "collisions": world.update, "gravity_step": apply_gravity + step.
    Returns ({k: snapshot after k updates}, notes) where notes["seed"] = accumulators (before, after) the first
    set_forces of a force-only world."""
    inp = integrator_inputs(n, inertia)
    kw = {}
    if mode == "collisions":
        kw["shape_type"], kw["half_extent"] = shapes_for(n)
    world.set_bodies(inp["pos"], rot=inp["rot"], lin_vel=inp["lin"], ang_vel=inp["ang"], mass=inp["mass"],
                     inertia=inp["inertia"], **kw)
    out, notes = {}, {}
    for k in range(max(checkpoints)):
        F, T = force_schedule(n, forces, k)
        if forces == "force" and k == 0:
            for b in sorted({0, n - 1}):
                world.apply_force_at_offset(b, SEED_FORCE, SEED_OFFSET)
            before = world.get_forces()
            world.set_forces(F, T)
            notes["seed"] = (before, world.get_forces())
        elif forces != "off":
            world.set_forces(F, T)
        if mode == "gravity_step":
            world.apply_gravity()
            world.step(DT)
        else:
            world.update(DT)
        if k + 1 in checkpoints:
            out[k + 1] = snapshot(world)
    return out, notes


@functools.lru_cache(maxsize=None)
def integrator_reference(forces, inertia, exact, gravity_offset=GRAVITY_OFFSET):
    """Float64 trajectory of every size at once (bodies do not interact): {n: {k: State}} for k = 1 and UPDATES, and
    {n: (UPDATES + 1, n, 3) positions} for the bodies-apart check."""
    parts = [integrator_inputs(n, inertia) for n in SIZES]
    cat = lambda key: np.concatenate([p[key] for p in parts])
    ref_inertia = np.concatenate([p["ref_inertia"].reshape(n, -1) for p, n in zip(parts, SIZES)])
    s = dr.State(cat("pos"), cat("rot"), cat("lin"), cat("ang"), cat("mass"), ref_inertia)
    N = sum(SIZES)
    starts = np.cumsum((0,) + SIZES)
    dt = dr.duration_as_secs_f32(DT)
    states, track = {}, [s.pos.copy()]
    for k in range(UPDATES):
        F, T = np.zeros((N, 3)), np.zeros((N, 3))
        for n, lo in zip(SIZES, starts):
            f, t = force_schedule(n, forces, k)
            if f is not None:
                F[lo:lo + n] = f
            if t is not None:
                T[lo:lo + n] = t
            if forces == "force" and k == 0:  # rigid_body.rs:60, then set_forces overwrites the force side only
                for b in {0, n - 1}:
                    T[lo + b] = np.cross(SEED_OFFSET.astype(np.float64), SEED_FORCE.astype(np.float64))
        s, _, _ = dr.step(s, dt, F, T, GRAVITY_FORCE, gravity_offset, exact)
        track.append(s.pos.copy())
        if k + 1 in (1, UPDATES):
            states[k + 1] = s
    track = np.stack(track)
    by_n = {n: {k: dr.State(st.pos[lo:lo + n], st.rot[lo:lo + n], st.lin[lo:lo + n], st.ang[lo:lo + n], st.mass[lo:lo + n])
                for k, st in states.items()} for n, lo in zip(SIZES, starts)}
    return by_n, {n: track[:, lo:lo + n] for n, lo in zip(SIZES, starts)}


# the `|u|^2 <= eps^2` edge of the quaternion exponential and the `angular_velocity != 0` branch, in a world whose gravity
# has no lever arm (no torque: omega stays what was set). Body 1 sits below the edge (dq = identity), body 2 above it.
EDGE_N = 65
EDGE_GRAVITY_OFFSET = (0.0, 0.0, 0.0)
EDGE_BELOW, EDGE_ABOVE = 1, 2


def edge_inputs():
    pos, q, lin, ang, mass = random_state(EDGE_N, 31)
    ang[EDGE_BELOW] = (1e-6, 0.0, 0.0)
    ang[EDGE_ABOVE] = (1e-4, 0.0, 0.0)
    return dict(pos=pos, rot=q, lin=lin, ang=ang, mass=mass)


def drive_edge(world, mode):
    inp = edge_inputs()
    kw = {}
    if mode == "collisions":
        kw["shape_type"], kw["half_extent"] = shapes_for(EDGE_N)
    world.set_bodies(inp["pos"], rot=inp["rot"], lin_vel=inp["lin"], ang_vel=inp["ang"], mass=inp["mass"], **kw)
    if mode == "gravity_step":
        world.apply_gravity()
        world.step(DT)
    else:
        world.update(DT)
    return snapshot(world)


@functools.lru_cache(maxsize=None)
def edge_reference(exact):
    inp = edge_inputs()
    s = dr.State(inp["pos"], inp["rot"], inp["lin"], inp["ang"], inp["mass"])
    return dr.step(s, dr.duration_as_secs_f32(DT), None, None, GRAVITY_FORCE, EDGE_GRAVITY_OFFSET, exact)[0]


def state_errors(snap, ref):
    """Worst float32-ulp deviation per quantity of a snapshot from a float64 State (dynamics_ref.ulp_error)."""
    e = {q: float(dr.ulp_error(snap[q], getattr(ref, q)).max()) for q in ("pos", "rot", "lin", "ang")}
    # the instance matrices are a function of the pose: judged on the pose the world itself holds
    e["inst"] = float(dr.ulp_error(snap["inst"], dr.instance_matrix(snap["pos"], snap["rot"])).max())
    return e


# ---------------------------------------------------------------------------------------------------------------------
# constraint solve: C constraints, 3C rows; what each size reaches in k_constraint_solve (1024 threads, dot products
# staged 8192 rows at a time, eight chains of 16 links per trip)
CONSTRAINT_COUNTS = (1, 3, 5, 11, 43, 341, 342, 2730, 2731, 2734, 5462, 8192)
CONSTRAINT_UPDATES = 3  # the second and third read the warm start
LIVE_COUNT = 342
LIVE_FORCE = np.array([3.0, -2.0, 1.5], np.float32)
LIVE_POINT = np.array([0.5, 1.0, -0.25], np.float32)


@functools.lru_cache(maxsize=None)
def constraint_case(C):
    """One (body, kind) per constraint (two of a kind on one body make J W J^T singular: SURVEY Q8), both kinds mixed in
    random order, masses in [0.5, 3], random targets; body 0 carries both kinds (C >= 2), being the one body that
    feels lambda (Q3)."""
    rng = np.random.default_rng(9000 + C)
    nb = (3 * C) // 4 + 2
    slots = np.arange(2 * nb)  # slot = 2 * body + kind
    if C >= 2:
        rest = rng.choice(slots[2:], C - 2, replace=False)
        chosen = np.concatenate([[0, 1], rest])
    else:
        chosen = np.array([0])
    chosen = rng.permutation(chosen)
    body, kind = chosen // 2, chosen % 2
    pos = rng.normal(scale=2.0, size=(nb, 3)).astype(np.float32)
    q = rng.normal(size=(nb, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    lin = rng.normal(scale=0.5, size=(nb, 3)).astype(np.float32)
    ang = rng.normal(scale=0.5, size=(nb, 3)).astype(np.float32)
    mass = rng.uniform(0.5, 3.0, nb).astype(np.float32)
    target = np.where((kind == 0)[:, None], rng.normal(size=(C, 3)), rng.uniform(-0.5, 0.5, size=(C, 3))).astype(np.float32)
    return dict(nb=nb, pos=pos, rot=q, lin=lin, ang=ang, mass=mass, body=body.astype(np.int64), kind=kind.astype(np.int64),
                target=target)


def live_forces(nb, k):
    rng = np.random.default_rng(555 + k)
    return rng.normal(scale=4.0, size=(nb, 3)).astype(np.float32), rng.normal(scale=2.0, size=(nb, 3)).astype(np.float32)


def drive_constraints(world, C, live=False, shapes=False):
    """CONSTRAINT_UPDATES updates of constraint_case(C). live: set_forces on every body and apply_force_at_position on
    body 0 before each update. Returns one record per update: the state before, the accumulators handed in (float64,
    from the inputs - not read back), lambda, the CG's verdict and the state after."""
    case = constraint_case(C)
    nb = case["nb"]
    kw = {}
    if shapes:
        kw["shape_type"], kw["half_extent"] = np.zeros(nb, np.uint32), np.zeros((nb, 3), np.float32)
    world.set_bodies(case["pos"], rot=case["rot"], lin_vel=case["lin"], ang_vel=case["ang"], mass=case["mass"], **kw)
    for kind, b, t in zip(case["kind"], case["body"], case["target"]):
        (world.add_constraint_fix_point if kind == 0 else world.add_constraint_fix_orientation)(int(b), t)
    records = []
    for k in range(CONSTRAINT_UPDATES):
        pre = snapshot(world)
        F, T = np.zeros((nb, 3)), np.zeros((nb, 3))
        if live:
            f, t = live_forces(nb, k)
            world.set_forces(f, t)
            world.apply_force_at_position(0, LIVE_FORCE, LIVE_POINT)
            F, T = f.astype(np.float64), t.astype(np.float64)
            # rigid_body.rs:52-53 on the position body 0 has now
            T[0] += np.cross(LIVE_POINT.astype(np.float64) - pre["pos"][0].astype(np.float64), LIVE_FORCE.astype(np.float64))
            F[0] += LIVE_FORCE
        world.update(DT)
        world.sync()
        st = world.get_stats()
        records.append(dict(pre=pre, F=F, T=T, lam=world.get_lambda(), converged=int(st.cg_converged),
                            iterations=int(st.cg_iterations), post=snapshot(world), n_manifolds=int(st.n_manifolds)))
    return records


def check_constraint_record(rec, C):
    """Float64 judgement of one update: (residual / bound of lambda, worst ulp deviation per quantity of the state after
    from `step` with entity 0 alone receiving J^T lambda)."""
    case = constraint_case(C)
    pre = rec["pre"]
    s = dr.State(pre["pos"], pre["rot"], pre["lin"], pre["ang"], case["mass"])
    cols = dr.constraint_columns(case["kind"], case["body"])
    rhs = dr.constraint_rhs(s, rec["F"], rec["T"], case["kind"], case["body"], case["target"], GRAVITY_FORCE, GRAVITY_OFFSET)
    W = np.repeat(1.0 / s.mass, 6)
    lam = rec["lam"].astype(np.float64)
    assert lam.shape == rhs.shape, "no lambda: the CG did not converge"
    ratio = dr.residual(lam, rhs, W, cols) / dr.bound(rhs, CG_MAX_ERROR, CG_MIN_ERROR)
    jl = dr.entity0_force(lam, cols)
    # physics.rs:42-54: gravity, then J^T lambda on entity 0, then step - every other body moves as if unconstrained
    g, o = np.asarray(GRAVITY_FORCE, np.float64), np.asarray(GRAVITY_OFFSET, np.float64)
    F, T = rec["F"] + g, rec["T"] + np.cross(o, g)
    F[0] += jl[:3]
    T[0] += jl[3:]
    after, _, _ = dr.step(s, dr.duration_as_secs_f32(DT), F, T, None, None, False)
    return ratio, state_errors(rec["post"], after), jl
