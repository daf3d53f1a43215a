"""GPU: the cluster solver's other shapes on the varied tower of tests/contact_ref.py - every body with a mass and an inertia
of its own - which only a FRESH process reaches, because the library reads its PHYS_DEBUG_* switches once: dynamic clusters
(PHYS_DEBUG_CLUSTER_DYNAMIC), dynamic clusters with fewer homes than bodies (PHYS_DEBUG_CLUSTER_CAP=9000: bodies A and B
without a home, whose constants ride with the row in planes 12-15 or, full tensors, are gathered by id), and one workgroup
per CU (PHYS_DEBUG_CLUSTERS_PER_CU=1: a lane's two rows alternate). A cluster has 64 slots at least, so on 256 CUs the cap
alone still leaves 672 x 64 homes with diagonal tensors - one for everybody - and 448 x 64 = 28 672 with full ones; with one
workgroup per CU as well it is 224 x 64 = 14 336 for the 33 280 bodies (tests/cpp/setup_probe.cpp pins the three), and
that is the case which reaches planes 14-15 with diagonal tensors. tools/cluster_probe.py runs each and only writes
files; this file judges: updates 2 to 4 ran the cluster kernel alone, every update holds to the float64 reference under
contact_ref.TOL_VARIED, colours and counters are the reference's, and every bit of poses and velocities equals the run of a
process with PHYS_DEBUG_NO_CLUSTER (the dataflow kernels), whose dump is also what the reference is computed from - once
per inertia kind.

And in this process: the cases of tests/test_gpu_solver_independent.py's varied tower against a CPU oracle world given the
same bodies, flags and iterations, bit for bit (that file keeps to the numpy reference: tests/test_abi.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import contact_ref as cr
import test_gpu_solver_independent as si

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {"no_cluster": {"PHYS_DEBUG_NO_CLUSTER": "1"},
        "dynamic": {"PHYS_DEBUG_CLUSTER_DYNAMIC": "1"},
        "dynamic_cap9000": {"PHYS_DEBUG_CLUSTER_DYNAMIC": "1", "PHYS_DEBUG_CLUSTER_CAP": "9000"},
        "dynamic_cap9000_one_per_cu": {"PHYS_DEBUG_CLUSTER_DYNAMIC": "1", "PHYS_DEBUG_CLUSTER_CAP": "9000", "PHYS_DEBUG_CLUSTERS_PER_CU": "1"},
        "one_per_cu": {"PHYS_DEBUG_CLUSTERS_PER_CU": "1"}}
VARIANTS = [("dynamic", "diag"), ("dynamic", "full"), ("dynamic_cap9000", "diag"), ("dynamic_cap9000", "full"),
            ("one_per_cu", "diag"), ("dynamic_cap9000_one_per_cu", "diag"), ("dynamic_cap9000_one_per_cu", "full")]
OVF_HANDOFF = 1 << 4
_dir = None


@pytest.fixture(autouse=True, scope="module")
def _files(tmp_path_factory):
    global _dir
    _dir = str(tmp_path_factory.mktemp("cluster_probe"))
    yield
    _probe.cache_clear()
    _reference.cache_clear()


@functools.lru_cache(maxsize=None)
def _probe(variant, inertia):
    """One run of tools/cluster_probe.py; (arrays, None) or (None, the failure) - kept: a failed run is not started again."""
    out = os.path.join(_dir, f"{variant}_{inertia}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PHYS_DEBUG_")}
    env.update(ENVS[variant])
    try:
        # set-up, four updates and their read-backs take a few seconds; a hand-off that times out ends after 3 s per update
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cluster_probe.py"), "--out", out, "--inertia", inertia],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return None, f"cluster_probe {variant} {inertia}: no end after {e.timeout} s"
    if r.returncode != 0:
        return None, f"cluster_probe {variant} {inertia}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    return dict(np.load(out)), None


def _run(variant, inertia):
    arrays, failure = _probe(variant, inertia)
    assert failure is None, failure
    for u in range(1, cr.VARIED_UPDATES + 1):
        assert not int(arrays[f"u{u}.stats"][4]) & OVF_HANDOFF, (variant, inertia, u, arrays[f"u{u}.stats"])
        assert int(arrays[f"u{u}.stats"][4]) == 0, (variant, inertia, u)
    return arrays


def _manifolds(arrays, u):
    return tuple(arrays[f"u{u}.{f}"] for f in ("ids", "counts", "normals", "points"))


@functools.lru_cache(maxsize=None)
def _reference(inertia):
    """The float64 reference's four updates, from what the process without cluster kernels dumped. Computed once per
    inertia kind: a variant whose bits equal that process's started every update from the same bits."""
    arrays = _run("no_cluster", inertia)
    bodies = cr.varied_tower(cr.VARIED_SEED, inertia)
    n = len(bodies["pos"])
    inv_m, inv_I = cr.body_inverses(n, bodies["mass"], bodies["inertia"])
    ref = cr.SolverRef(n, cr.Params(si.DT_S), 8)
    return [ref.update(_manifolds(arrays, u), arrays[f"u{u}.pos"], arrays[f"u{u}.lin"], arrays[f"u{u}.ang"], inv_m, inv_I, si.GRAVITY)
            for u in range(1, cr.VARIED_UPDATES + 1)]


def _check_against_reference(arrays, outs, what):
    worst = 0.0
    for u, out in enumerate(outs, 1):
        n_manifolds, n_colors, rounds, n_new = (int(x) for x in arrays[f"u{u}.stats"][:4])
        assert n_manifolds == len(out["a"]) > 40_960, (what, u)
        assert np.array_equal(arrays[f"u{u}.color_counts"], cr.color_counts(out["colors"])), (what, u)
        assert (n_colors, rounds, n_new) == (out["n_colors"], out["color_rounds"], out["n_new_manifolds"]), (what, u)
        err, amb = cr.velocity_error(out, arrays[f"u{u}.lin1"], arrays[f"u{u}.ang1"])
        assert amb <= 0.01 * len(out["a"]), (what, u, amb)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("inertia", ["diag", "full"])
def test_the_process_without_cluster_kernels_holds_to_float64(inertia):
    """The control the variants are compared with: PHYS_DEBUG_NO_CLUSTER leaves the dataflow kernels."""
    arrays = _run("no_cluster", inertia)
    for u in range(1, cr.VARIED_UPDATES + 1):
        stages = set(str(arrays[f"u{u}.stages"]).split("+"))
        assert stages and stages <= si.SOLVER_STAGES - {"solve_cluster"}, (u, stages)
    worst = _check_against_reference(arrays, _reference(inertia), f"no_cluster {inertia}")
    print(f"\nno cluster kernels, {inertia}: error {worst:.3g} (tolerance {cr.TOL_VARIED:.3g})")
    assert worst < cr.TOL_VARIED


@pytest.mark.parametrize("variant,inertia", VARIANTS)
def test_cluster_variant_on_the_varied_tower(variant, inertia):
    arrays, base = _run(variant, inertia), _run("no_cluster", inertia)
    for u in range(2, cr.VARIED_UPDATES + 1):
        assert str(arrays[f"u{u}.stages"]) == "solve_cluster", (u, arrays[f"u{u}.stages"])
    for u in range(1, cr.VARIED_UPDATES + 1):
        for f in ("pos", "lin", "ang", "ids", "counts", "normals", "points", "pos1", "rot1", "lin1", "ang1"):
            a, b = arrays[f"u{u}.{f}"], base[f"u{u}.{f}"]
            if a.shape != b.shape or a.tobytes() != b.tobytes():
                # (the bits differ: say how far the float64 reference is, from this run's own inputs, before failing)
                bodies = cr.varied_tower(cr.VARIED_SEED, inertia)
                n = len(bodies["pos"])
                ref = cr.SolverRef(n, cr.Params(si.DT_S), 8)
                err = None
                for k in range(1, u + 1):
                    out = ref.update(_manifolds(arrays, k), arrays[f"u{k}.pos"], arrays[f"u{k}.lin"], arrays[f"u{k}.ang"],
                                     *cr.body_inverses(n, bodies["mass"], bodies["inertia"]), si.GRAVITY)
                    err = cr.velocity_error(out, arrays[f"u{k}.lin1"], arrays[f"u{k}.ang1"])[0]
                assert False, (f"{variant} {inertia}: update {u} {f} differs from the process without cluster kernels; "
                               f"error against float64 {err:.3g} (tolerance {cr.TOL_VARIED:.3g})")
    worst = _check_against_reference(arrays, _reference(inertia), f"{variant} {inertia}")
    print(f"\n{variant} {inertia}: error {worst:.3g} (tolerance {cr.TOL_VARIED:.3g}), bit-equal to the process without cluster kernels")
    assert worst < cr.TOL_VARIED


# ---------------------------------------------------------------- in this process: bit for bit against the oracle
@pytest.mark.parametrize("case,exclusive", si.VARIED_GPU_CASES, ids=[c + ("_exclusive" if x else "") for c, x in si.VARIED_GPU_CASES])
def test_varied_tower_equals_the_oracle_bit_for_bit(case, exclusive, oracle_lib):
    import physics_amd
    from oracle import binding as ob
    inertia, warm, iterations = cr.VARIED_CASES[case]
    bodies = cr.varied_tower(cr.VARIED_SEED, inertia)
    flags = physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_GROUND_PLANE | si.varied_flags(warm, exclusive)
    cfg = dict(flags=flags, gravity_force=(0, -9.81, 0), gravity_offset=(0, 0, 0), solver_iterations=iterations)
    w = physics_amd.World(physics_amd.default_config(**cfg))
    o = ob.OracleWorld(physics_amd.default_config(**cfg), trig=ob.TRIG_DET)
    o.set_threads(16)
    for x in (w, o):
        x.set_bodies(**bodies)
    for u in range(cr.VARIED_UPDATES):
        w.profile_enable(True)
        w.update(si.DT)
        w.sync()
        o.update(si.DT)
        stages = set(w.profile_get()[0]) & si.SOLVER_STAGES
        assert u == 0 or stages == {"solve_cluster"}, (u, stages)
        assert w.get_stats().overflow == 0
        for name, a, b in zip(("pos", "rot", "lin", "ang"), w.get_transforms() + w.get_velocities(), o.get_transforms() + o.get_velocities()):
            assert np.array_equal(a, b), f"{case}: update {u + 1}, {name} differs from the oracle on {int((a != b).any(1).sum())} bodies"
    w.close()
