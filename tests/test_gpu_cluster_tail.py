"""GPU: what the tail of k_solve_cluster's row loop stores - the accumulated impulses and row masses a lane reads back one
sweep later, the per-manifold impulse record of the last sweep - on the 16 x 130 x 16 tower of tests/test_gpu_cluster_rows.py
(33 280 bodies, the smallest world that kernel accepts), six updates. Between those stores and the fetch of the lane's next
row the kernel has no memory wait but the one it asks for itself when the next row is the row just stored; the waits ahead of
the solve are the compiler's, steered by explicit ones on the rare paths and in front of the solve (cluster_loads_landed,
physics_amd/csrc/cluster.hip). A read-back that overtook its store, or a row solved before its planes
had landed, changes bits here.

Each case runs tools/cluster_tail_probe.py in a FRESH process (the library reads its PHYS_DEBUG_* switches once) and is
compared, bit for bit, with a process under PHYS_DEBUG_NO_CLUSTER (the dataflow kernels) on the same world: poses,
velocities, and the impulse records of phys_get_contact_impulses, which come sorted by body pair like phys_get_manifolds
(the emission order of manifolds is arbitrary). The cases, chosen for where the tail can go wrong:

  default           static clusters, three workgroups per CU
  one_per_cu        PHYS_DEBUG_CLUSTERS_PER_CU=1: a lane owns several rows of one sweep
  dynamic_cap9000   PHYS_DEBUG_CLUSTER_DYNAMIC=1, PHYS_DEBUG_CLUSTER_CAP=9000: homes dealt out per update, clusters with fewer
                    rows than lanes (the row just stored is the next one fetched)
  dynamic_cap9000_one_per_cu   ... and PHYS_DEBUG_CLUSTERS_PER_CU=1 as well: with diagonal tensors a cluster has 64 slots at
                    least, so the cap alone still leaves a home for every body of this tower on 256 CUs (DESIGN.md section 4,
                    tests/cpp/setup_probe.cpp); 224 x 64 = 14 336 homes do not: bodies A without a home (the foreign-A
                    planes and the first update's velocity gather, the loads the rare path waits for itself)
  cold              PHYS_FLAG_NO_WARM_START: no impulse record, the masses are written in sweep 0 of a solve that starts from
                    zero impulses
  spheres           the top layer is spheres: rows of one point, whose second and third plane stores are skipped"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATES = 6
# case -> (environment, arguments of the probe); the control of a case: the same arguments under PHYS_DEBUG_NO_CLUSTER
CASES = {"default": ({}, ()),
         "one_per_cu": ({"PHYS_DEBUG_CLUSTERS_PER_CU": "1"}, ()),
         "dynamic_cap9000": ({"PHYS_DEBUG_CLUSTER_DYNAMIC": "1", "PHYS_DEBUG_CLUSTER_CAP": "9000"}, ()),
         "dynamic_cap9000_one_per_cu": ({"PHYS_DEBUG_CLUSTER_DYNAMIC": "1", "PHYS_DEBUG_CLUSTER_CAP": "9000", "PHYS_DEBUG_CLUSTERS_PER_CU": "1"}, ()),
         "cold": ({}, ("--cold",)),
         "spheres": ({}, ("--spheres",))}
NO_CLUSTER = {"PHYS_DEBUG_NO_CLUSTER": "1"}
_dir = None


@pytest.fixture(autouse=True, scope="module")
def _files(tmp_path_factory):
    global _dir
    _dir = str(tmp_path_factory.mktemp("cluster_tail"))
    yield
    _probe.cache_clear()


@functools.lru_cache(maxsize=None)
def _probe(env_items, args):
    """One run of tools/cluster_tail_probe.py; (arrays, None) or (None, the failure) - kept: a failed run is not started again,
    and the control of several cases runs once."""
    name = "_".join([k[len("PHYS_DEBUG_"):].lower() + v for k, v in env_items] + [a.lstrip("-") for a in args]) or "default"
    out = os.path.join(_dir, name + ".npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PHYS_DEBUG_")}
    env.update(dict(env_items))
    try:
        # set-up, six updates and the read-backs take a few seconds; a hand-off that times out ends after 3 s per update
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cluster_tail_probe.py"), "--out", out, "--updates", str(UPDATES), *args],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return None, f"cluster_tail_probe {name}: no end after {e.timeout} s"
    if r.returncode != 0:
        return None, f"cluster_tail_probe {name}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    return dict(np.load(out)), None


def _run(env, args):
    arrays, failure = _probe(tuple(sorted(env.items())), tuple(args))
    assert failure is None, failure
    assert int(arrays["stats"][3]) == 0, ("overflow", env, args, arrays["stats"])
    return arrays


@pytest.mark.parametrize("case", list(CASES))
def test_cluster_tail_equals_the_process_without_cluster_kernels(case):
    env, args = CASES[case]
    got, want = _run(env, args), _run(NO_CLUSTER, args)
    stages, control = str(got["stages"]).split(","), str(want["stages"]).split(",")
    assert len(stages) == len(control) == UPDATES
    # the first update has no counters of an earlier one to plan with; every later one is the cluster kernel's alone
    assert stages[1:] == ["solve_cluster"] * (UPDATES - 1), stages
    assert all(s and "solve_cluster" not in s.split("+") for s in control), control
    n_manifolds, n_contacts = int(got["stats"][0]), int(got["stats"][1])
    assert n_manifolds > 90_000 and np.array_equal(got["stats"], want["stats"]), (got["stats"], want["stats"])
    if case == "spheres":  # rows of fewer than four points
        assert n_contacts < 4 * n_manifolds, (n_manifolds, n_contacts)
    for f in ("pos", "rot", "lin", "ang", "ids", "counts"):
        a, b = got[f], want[f]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
            f"{case}: {f} differs from the process without cluster kernels on {int((a != b).reshape(len(a), -1).any(1).sum())} rows"
    if case == "cold":
        assert "impulses" not in got and "impulses" not in want  # (no impulse record without warm starting)
        return
    a, b = got["impulses"], want["impulses"]
    assert a.shape == b.shape == (n_manifolds, 4, 3)
    assert np.any(a != 0.0), "no impulse was recorded"
    differ = (a.view(np.uint32) != b.view(np.uint32)).reshape(n_manifolds, -1).any(1)
    assert not differ.any(), (f"{case}: the impulse records of {int(differ.sum())} of {n_manifolds} manifolds differ from the process "
                              f"without cluster kernels; first: bodies {got['ids'][np.argmax(differ)]}")
