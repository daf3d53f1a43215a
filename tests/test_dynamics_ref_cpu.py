"""The float64 dynamics reference (tests/dynamics_ref.py) against the CPU oracle, deterministic trig and libm, on every
configuration tests/test_gpu_dynamics_independent.py uses (tests/dynamics_cases.py). This is what proves the reference
and what the tolerance table at the top of dynamics_ref.py is measured from: each test asserts that the oracle stays
within the MEASURED figures on 100 % of bodies and rows, and `test_table_*` that those figures are the worst ones seen,
not guesses (at most 25 % above the worst). The kernels are held to 4 x these figures; nothing here runs a kernel."""
import functools

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr

TRIGS = (1, 0)  # oracle.binding.TRIG_DET, TRIG_LIBM


def _oracle(trig, **cfg):
    import physics_amd
    from oracle import binding as ob
    return ob.OracleWorld(physics_amd.default_config(**cfg), trig=trig)


def _worse(into, e):
    for k, v in e.items():
        into[k] = max(into.get(k, 0.0), v)


# ---- pieces -----------------------------------------------------------------------------------------------------------
def _euler_bound(q):
    """Allowed |float32 - float64| of the three angles. The rotation-matrix entries are sums of four float32 products of
    magnitude <= |q|^2: absolute error <= 4 ulp(|q|^2) each. roll and yaw are atan2 of two entries of a vector of length
    c = cos(pitch) |q|^2 and pitch = asin(r20) has slope 1 / cos(pitch): all three amplify the entry error by 1 / c
    (the gimbal branches: by 1 / hypot(r01, r02)). asin / atan2 / cos / the division add a few ulp of the result (<= pi)."""
    R = dr.rotation_matrix(np.asarray(q, np.float64).reshape(-1, 4))
    n2 = np.einsum("ij,ij->i", q, q).astype(np.float64)
    reg = np.abs(R[:, 2, 0]) < 1.0
    c = np.where(reg, np.hypot(R[:, 2, 1], R[:, 2, 2]), np.hypot(R[:, 0, 1], R[:, 0, 2]))
    return dr.F32_EPS * (16.0 + 8.0 * n2 / c)


def _euler_inputs():
    rng = np.random.default_rng(3)
    q = rng.normal(size=(2000, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[1000:] *= rng.uniform(0.9, 1.1, size=(1000, 1))  # never renormalised (Q6): not unit in general
    gimbal = np.array([[0.0, 0.8, 0.0, 0.8],      # r20 = 2 (ik - wj) = -1.28 <= -1: pitch = +pi/2
                       [0.0, -0.8, 0.0, 0.8],     # r20 = +1.28 >= 1: pitch = -pi/2
                       [0.3, 0.75, -0.2, 0.75],   # both again, with roll to recover from r01, r02
                       [0.3, -0.75, -0.2, 0.75]])
    return np.concatenate([q, gimbal]).astype(np.float32)


@pytest.mark.parametrize("trig", TRIGS)
def test_euler_angles_vs_oracle(trig):
    from oracle import binding as ob
    q = _euler_inputs()
    ref = dr.euler_angles(q)
    assert (np.abs(ref[-4:, 1]) == np.pi / 2).all() and (ref[-4:, 2] == 0.0).all()  # the gimbal branches were taken
    assert ref[-4, 1] > 0 > ref[-3, 1]
    got = np.stack([ob.quat_euler_angles(qi, trig) for qi in q]).astype(np.float64)
    assert (np.abs(got - ref) <= _euler_bound(q)[:, None]).all(), np.abs(got - ref).max()


def test_instance_matrix_vs_oracle():
    pos, q, _, _, _ = dc.random_state(500, 12)
    q[250:] *= 1.05
    o = _oracle(1)
    o.set_bodies(pos, rot=q)
    got = o.get_instance_matrices()
    ref = dr.instance_matrix(pos, q)
    assert (got.reshape(-1, 4, 4)[:, :, 3] == [0, 0, 0, 1]).all()
    # an entry of R is four float32 products and three sums, each rounded once to half an ulp of at most |q|^2 = 1.1
    assert dr.ulp_error(got, ref).max() <= 3.5


# ---- integrator -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integrator_worst(forces, inertia, exact):
    """Worst oracle-against-float64 deviation after 1 and after UPDATES updates, over every size and both trig sets."""
    import physics_amd
    ref, _ = dc.integrator_reference(forces, inertia, exact)
    worst = {1: {}, dc.UPDATES: {}}
    for trig in TRIGS:
        for n in dc.SIZES:
            o = _oracle(trig, flags=physics_amd.FLAG_EXACT_ROTATION if exact else 0)
            snaps, _ = dc.drive_integrator(o, n, forces, "update", inertia)
            for k, snap in snaps.items():
                _worse(worst[k], dc.state_errors(snap, ref[n][k]))
                assert not snap["force"].any() and not snap["torque"].any()
    return worst


INTEGRATOR_KEYS = [(f, i, e) for f in dc.FORCES for i in dc.INERTIA for e in (False, True)]


@pytest.mark.parametrize("forces,inertia,exact", INTEGRATOR_KEYS)
def test_integrator_oracle_within_table(forces, inertia, exact):
    worst = _integrator_worst(forces, inertia, exact)
    for q in dc.QUANTITIES:
        assert worst[1][q] <= dr.MEASURED_ONE[q], (q, worst[1][q])
        assert worst[dc.UPDATES][q] <= dr.MEASURED_K50[q], (q, worst[dc.UPDATES][q])


@pytest.mark.parametrize("exact", (False, True))
def test_edge_bodies_oracle(exact):
    """omega = 0, and omega on either side of the `|u|^2 <= eps^2` edge: float32 and float64 take the same branch."""
    import physics_amd
    ref = dc.edge_reference(exact)
    inp = dc.edge_inputs()
    still = np.flatnonzero(~inp["ang"].any(axis=1))
    assert len(still) >= 9
    for trig in TRIGS:
        o = _oracle(trig, flags=physics_amd.FLAG_EXACT_ROTATION if exact else 0, gravity_offset=dc.EDGE_GRAVITY_OFFSET)
        snap = dc.drive_edge(o, "update")
        for b in list(still) + [dc.EDGE_BELOW]:
            assert np.array_equal(snap["rot"][b], inp["rot"][b]) and np.array_equal(ref.rot[b], inp["rot"][b].astype(np.float64))
        assert not np.array_equal(snap["rot"][dc.EDGE_ABOVE], inp["rot"][dc.EDGE_ABOVE])
        assert not np.array_equal(ref.rot[dc.EDGE_ABOVE], inp["rot"][dc.EDGE_ABOVE].astype(np.float64))
        e = dc.state_errors(snap, ref)
        for q in dc.QUANTITIES:
            assert e[q] <= dr.MEASURED_ONE[q], (q, e[q])


def test_collision_cases_keep_bodies_apart():
    """The collision-mode runs of the GPU file promise "the same integration": their tiny spheres must never meet. Two
    spheres of radius 1e-3 whose AABBs are fattened by the contact margin of 0.02 are not even a candidate pair beyond a
    centre distance of 2 * (1e-3 + 0.02) * sqrt(3) = 0.073."""
    for forces in dc.FORCES:
        _, track = dc.integrator_reference(forces, "shared", False)  # positions do not depend on inertia or rotation
        for n in dc.SIZES:
            p = track[n][:, ::dc.SPHERE_STRIDE]  # the spheres
            if p.shape[1] < 2:
                continue
            d = np.linalg.norm(p[:, :, None, :] - p[:, None, :, :], axis=3)
            d[:, np.arange(p.shape[1]), np.arange(p.shape[1])] = np.inf
            assert d.min() > 0.08, (forces, n, d.min())


# ---- constraints ------------------------------------------------------------------------------------------------------
CONSTRAINT_KEYS = [(C, False, False) for C in dc.CONSTRAINT_COUNTS] + [(dc.LIVE_COUNT, True, False), (dc.LIVE_COUNT, True, True)]


@functools.lru_cache(maxsize=None)
def _constraint_worst(C, live, collisions):
    """(worst residual / bound, worst one-update deviation) of the oracle over the updates and both trig sets."""
    import physics_amd
    ratio, worst = 0.0, {}
    for trig in TRIGS:
        o = _oracle(trig, flags=physics_amd.FLAG_COLLISIONS if collisions else 0)
        for rec in dc.drive_constraints(o, C, live=live, shapes=collisions):
            assert rec["converged"] == 1 and rec["iterations"] >= 1 and rec["n_manifolds"] == 0
            r, e, _ = dc.check_constraint_record(rec, C)
            ratio = max(ratio, r)
            _worse(worst, e)
    return ratio, worst


@pytest.mark.parametrize("C,live,collisions", CONSTRAINT_KEYS)
def test_constraints_oracle_within_table(C, live, collisions):
    ratio, worst = _constraint_worst(C, live, collisions)
    assert ratio <= dr.MEASURED_CG_RATIO, ratio
    for q in dc.QUANTITIES:
        assert worst[q] <= dr.MEASURED_ONE[q], (q, worst[q])


def test_constraint_case_shape():
    for C in dc.CONSTRAINT_COUNTS:
        case = dc.constraint_case(C)
        slots = 2 * case["body"] + case["kind"]
        assert len(slots) == C == len(set(slots.tolist()))  # Q8: one (body, kind) each
        if C >= 2:
            assert {0, 1} <= set(slots.tolist()) and 0 < case["kind"].sum() < C
        assert 0.5 <= case["mass"].min() and case["mass"].max() <= 3.0


def test_entity0_force_and_residual_by_hand():
    # two constraints on body 0 (point, orientation), one on body 1: rows 0-2 -> columns 0-2, 3-5 -> 3-5, 6-8 -> 6-8
    cols = dr.constraint_columns([0, 1, 0], [0, 0, 1])
    assert cols.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    lam = np.arange(1.0, 10.0)
    assert dr.entity0_force(lam, cols).tolist() == [1, 2, 3, 4, 5, 6]
    W = np.repeat([0.5, 0.25], 6)
    rhs = dr.apply_A(lam, W, cols)
    assert rhs.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 1.75, 2.0, 2.25]
    assert dr.residual(lam, rhs + np.array([0, 0, 0, 0, 0, 0, 0, 0, 0.125]), W, cols) == 0.125
    assert dr.bound(rhs, 1e-2, 1e-3) == 0.03 and dr.bound(rhs * 1e-3, 1e-2, 1e-3) == 1e-3


# ---- the table ----------------------------------------------------------------------------------------------------------
def measure():
    """Everything the table of dynamics_ref.py records, measured now."""
    one, k50, ratio = {}, {}, 0.0
    for key in INTEGRATOR_KEYS:
        w = _integrator_worst(*key)
        _worse(one, w[1])
        _worse(k50, w[dc.UPDATES])
    for key in CONSTRAINT_KEYS:
        r, w = _constraint_worst(*key)
        ratio = max(ratio, r)
        _worse(one, w)
    return one, k50, ratio


def test_table_holds_the_measured_worst():
    one, k50, ratio = measure()
    for q in dc.QUANTITIES:
        assert one[q] <= dr.MEASURED_ONE[q] <= 1.25 * one[q], (q, one[q])
        assert k50[q] <= dr.MEASURED_K50[q] <= 1.25 * k50[q], (q, k50[q])
        assert dr.TOL_ONE[q] == 4.0 * dr.MEASURED_ONE[q] and dr.TOL_K50[q] == 4.0 * dr.MEASURED_K50[q]
    assert ratio <= dr.MEASURED_CG_RATIO <= 1.25 * ratio, ratio
    assert dr.CG_MARGIN == max(1.0, 2.0 * dr.MEASURED_CG_RATIO)

