"""integrate.hip and constraints.hip against the float64 reference of tests/dynamics_ref.py - written from the Rust
sources, independent of the oracle - and, bit for bit, against the CPU oracle, at the sizes where their loops change
trips: either side of a wave and of a 256-thread block for the integrator; for k_constraint_solve (1024 threads, dot
products staged 8192 rows at a time, eight chains adding 16 links per trip) the row counts of dynamics_cases.
CONSTRAINT_COUNTS. Tolerances: the table at the top of dynamics_ref.py, measured from the oracle on these very
configurations by tests/test_dynamics_ref_cpu.py."""
import functools

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr

pytestmark = pytest.mark.gpu

MODES = ("update", "gravity_step", "collisions")
STATE = ("pos", "rot", "lin", "ang", "inst")


def _flags(exact=False, collisions=False):
    import physics_amd
    return (physics_amd.FLAG_EXACT_ROTATION if exact else 0) | (physics_amd.FLAG_COLLISIONS if collisions else 0)


def _world(**cfg):
    import physics_amd
    return physics_amd.World(physics_amd.default_config(**cfg))


def _oracle(**cfg):
    import physics_amd
    from oracle import binding as ob
    return ob.OracleWorld(physics_amd.default_config(**cfg), trig=ob.TRIG_DET)


def _assert_within(errors, tol, what):
    print(what, {q: round(v, 3) for q, v in errors.items()})
    for q in dc.QUANTITIES:
        assert errors[q] <= tol[q], f"{what}: {q} is {errors[q]:.2f} ulp from float64, tolerance {tol[q]:.2f}"


def _assert_same(snap, osnap, what):
    for q in STATE:
        assert np.array_equal(snap[q], osnap[q]), f"{what}: {q} differs from the oracle (max abs {np.abs(snap[q] - osnap[q]).max()})"


# ---- integrator -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_integrator(n, forces, inertia, exact):
    """The oracle's update (apply_gravity + step, physics.rs:41-55) - what all three GPU modes must reproduce."""
    return dc.drive_integrator(_oracle(flags=_flags(exact)), n, forces, "update", inertia)


@pytest.mark.parametrize("exact", (False, True), ids=("quirk_q1", "exact_rotation"))
@pytest.mark.parametrize("inertia", dc.INERTIA)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("forces", dc.FORCES)
def test_integrator_one_and_fifty_updates(forces, mode, inertia, exact):
    """Every size, after 1 and after 50 updates: within the table of float64, accumulators zero, bit-equal to the oracle.
    mode "gravity_step" reaches the GRAVITY = false kernels, "collisions" k_step_velocity_aabb + k_step_position (bodies
    apart: the same integration); forces != "off" the FORCES = true instances through set_forces."""
    ref, _ = dc.integrator_reference(forces, inertia, exact)
    for n in dc.SIZES:
        what = f"n={n}"
        with _world(flags=_flags(exact, mode == "collisions")) as w:
            snaps, notes = dc.drive_integrator(w, n, forces, mode, inertia)
            if mode == "collisions":
                w.sync()
                assert w.get_stats().n_manifolds == 0
        osnaps, onotes = _oracle_integrator(n, forces, inertia, exact)
        for k, tol in ((1, dr.TOL_ONE), (dc.UPDATES, dr.TOL_K50)):
            _assert_within(dc.state_errors(snaps[k], ref[n][k]), tol, f"{what} update {k}")
            assert not snaps[k]["force"].any() and not snaps[k]["torque"].any()  # rigid_body.rs:38-39
            _assert_same(snaps[k], osnaps[k], f"{what} update {k}")
        if forces == "force":  # set_forces(force, None): the force side is replaced, the torque side reads back as before
            (f0, t0), (f1, t1) = notes["seed"]
            assert t0[0].any() and t0[n - 1].any() and np.array_equal(f0[0], dc.SEED_FORCE)
            assert np.array_equal(t1, t0) and np.array_equal(f1, dc.force_schedule(n, forces, 0)[0])
            assert np.array_equal(t1, onotes["seed"][1][1])


@pytest.mark.parametrize("exact", (False, True), ids=("quirk_q1", "exact_rotation"))
@pytest.mark.parametrize("mode", MODES)
def test_zero_omega_and_the_exponential_edge(mode, exact):
    """Gravity without a lever arm: omega = 0 skips the rotation (rigid_body.rs:32), omega = 1e-6 lands on the
    `|u|^2 <= eps^2` side of the quaternion exponential (dq = identity), omega = 1e-4 on the other."""
    inp = dc.edge_inputs()
    ref = dc.edge_reference(exact)
    with _world(flags=_flags(exact, mode == "collisions"), gravity_offset=dc.EDGE_GRAVITY_OFFSET) as w:
        snap = dc.drive_edge(w, mode)
    osnap = dc.drive_edge(_oracle(flags=_flags(exact), gravity_offset=dc.EDGE_GRAVITY_OFFSET), "update")
    for b in list(np.flatnonzero(~inp["ang"].any(axis=1))) + [dc.EDGE_BELOW]:
        assert np.array_equal(snap["rot"][b], inp["rot"][b]), b
    assert not np.array_equal(snap["rot"][dc.EDGE_ABOVE], inp["rot"][dc.EDGE_ABOVE])
    _assert_within(dc.state_errors(snap, ref), dr.TOL_ONE, mode)
    _assert_same(snap, osnap, mode)


def test_instance_matrices_of_scaled_quaternions():
    """Quaternions that are not unit (never renormalised, Q6): the matrix is ww + ii - jj - kk on the diagonal, not
    1 - 2 (jj + kk). An entry is four float32 products and three sums, half an ulp of at most |q|^2 = 1.1 each."""
    pos, q, _, _, _ = dc.random_state(1000, 12)
    q[500:] *= np.float32(1.05)
    with _world() as w:
        w.set_bodies(pos, rot=q)
        got = w.get_instance_matrices()
    assert dr.ulp_error(got, dr.instance_matrix(pos, q)).max() <= 3.5
    assert (got.reshape(-1, 4, 4)[:, :, 3] == [0, 0, 0, 1]).all()


# ---- constraint solve -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_constraints(C, live):
    return dc.drive_constraints(_oracle(), C, live=live)


def _check_constraint_run(records, orecords, C):
    case = dc.constraint_case(C)
    other = next(int(b) for b in case["body"] if b != 0) if C > 1 else None
    for k, (rec, orec) in enumerate(zip(records, orecords)):
        what = f"C={C} update {k + 1}"
        # bit-equal to the oracle: lambda, the CG's verdict, the state after
        assert np.array_equal(rec["lam"], orec["lam"]), f"{what}: lambda differs from the oracle"
        assert (rec["converged"], rec["iterations"]) == (orec["converged"], orec["iterations"]) and rec["converged"] == 1
        _assert_same(rec["post"], orec["post"], what)
        assert rec["n_manifolds"] == 0
        # float64: the true residual of the GPU's lambda, and every body after the update - entity 0 with J^T lambda in
        # its accumulators, v + (F + g + J^T lambda) / m dt; everybody else as if unconstrained (Q3)
        ratio, errors, jl = dc.check_constraint_record(rec, C)
        print(what, "residual / bound", round(ratio, 4), "iterations", rec["iterations"])
        assert ratio <= dr.CG_MARGIN, f"{what}: float64 residual of lambda is {ratio:.3f} x bound, margin {dr.CG_MARGIN}"
        _assert_within(errors, dr.TOL_ONE, what)
        assert np.abs(jl[:3]).max() > 1.0  # the scatter is no rounding matter: left out, entity 0 misses by thousands of ulps
        if other is not None:  # a constrained body other than entity 0: its lambda goes nowhere
            g = np.asarray(dc.GRAVITY_FORCE)
            v = rec["pre"]["lin"][other].astype(np.float64) + (rec["F"][other] + g) / float(case["mass"][other]) * float(dr.duration_as_secs_f32(dc.DT))
            assert dr.ulp_error(rec["post"]["lin"][other], v).max() <= dr.TOL_ONE["lin"]
        if k > 0:
            assert np.abs(records[k - 1]["lam"]).max() > 0  # the warm start that this update read


@pytest.mark.parametrize("C", dc.CONSTRAINT_COUNTS)
def test_constraint_solve_at_loop_edges(C):
    with _world() as w:
        records = dc.drive_constraints(w, C)
    _check_constraint_run(records, _oracle_constraints(C, False), C)


@pytest.mark.parametrize("collisions", (False, True), ids=("plain", "collisions"))
def test_constraints_with_live_accumulators(collisions):
    """set_forces on every body and apply_force_at_position on body 0 before each update: Q is no longer gravity alone,
    and the FORCES instances that take J^T lambda run (k_step_full; with collisions k_step_velocity_aabb)."""
    C = dc.LIVE_COUNT
    with _world(flags=_flags(collisions=collisions)) as w:
        records = dc.drive_constraints(w, C, live=True, shapes=collisions)
    assert all(r["F"].any() and r["T"].any() for r in records)
    _check_constraint_run(records, _oracle_constraints(C, True), C)
