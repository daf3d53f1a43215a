"""GPU: both builds of the narrow-phase kernel (128 and 512 threads) and both orders of its colour-table probe, on the
scenes of tests/shape_pair_ref.py - every pair kind in both index orders, static partners, the ground - over TWO updates,
so that the second one runs the table look-up that a first update after phys_set_bodies never reaches. The library reads
PHYS_DEBUG_NP_THREADS and PHYS_DEBUG_NP_EARLY_PROBE once per process: tools/pair_probe.py runs the worlds in four fresh
processes, from arrays this file writes, and dumps the manifolds of either update. All four must agree bit for bit, with
each other and - first update - with the in-process worlds that tests/test_gpu_shape_pairs.py holds to float64 (left to
itself a world of this size takes the 128-thread kernel there); the float64 checks of that file run again on what a
512-thread process gave."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import shape_pair_ref as spr
import test_gpu_shape_pairs as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PAIRS, SEEDS = spr.N_PAIRS, spr.SEEDS
PROCESSES = [(threads, early) for threads in ("128", "512") for early in ("0", "1")]
BODY_WORLDS = [(kind, order) for kind in spr.KINDS for order in ("ab", "ba")]
_dir = None


@pytest.fixture(autouse=True, scope="module")
def _files(tmp_path_factory):
    global _dir
    _dir = str(tmp_path_factory.mktemp("narrow_probe"))
    yield
    _probe.cache_clear()
    _input.cache_clear()


@functools.lru_cache(maxsize=None)
def _ground(gkind):
    return spr.ground_scene(gkind, N_PAIRS, SEEDS[gkind])


@functools.lru_cache(maxsize=None)
def _input():
    """The worlds of tests/test_gpu_shape_pairs.py as arrays: b.<kind>.<order>, s.<kind>.<order> (B static), g.<shape>."""
    a, names = {}, []
    for kind, order in BODY_WORLDS:
        arr = spr.arrange(sp._scene(kind), order)
        name = f"b.{kind}.{order}"
        names.append(name)
        for f in ("pos", "rot", "shape", "he"):
            a[f"{name}.{f}"] = arr[f]
        arr = spr.arrange_static(sp._scene(kind), order)
        name = f"s.{kind}.{order}"
        names.append(name)
        for f in ("pos", "rot", "shape", "he"):
            a[f"{name}.{f}"] = arr["body"][f]
            a[f"{name}.s_{f}"] = arr["static"][f]
    for gkind in spr.GROUND_KINDS:
        arr = _ground(gkind)
        name = f"g.{gkind}"
        names.append(name)
        for f in ("pos", "rot", "shape", "he"):
            a[f"{name}.{f}"] = arr[f]
        a[f"{name}.ground"] = np.array(True)
    path = os.path.join(_dir, "worlds.npz")
    np.savez(path, names=np.array(names), **a)
    return path, names


@functools.lru_cache(maxsize=None)
def _probe(threads, early):
    """One run of tools/pair_probe.py narrow; (arrays, None) or (None, the failure) - kept: a failed run is not started again."""
    out = os.path.join(_dir, f"np{threads}_early{early}.npz")
    env = dict(os.environ, PHYS_DEBUG_NP_THREADS=threads, PHYS_DEBUG_NP_EARLY_PROBE=early)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pair_probe.py"), "narrow", "--input", _input()[0], "--out", out],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return None, f"pair_probe narrow {threads} {early}: no end after {e.timeout} s"
    if r.returncode != 0:
        return None, f"pair_probe narrow {threads} {early}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    return dict(np.load(out)), None


def _run(threads, early):
    arrays, failure = _probe(threads, early)
    assert failure is None, failure
    return arrays


def _manifolds(arrays, name, update):
    """spr.manifolds_of, from the arrays a process dumped"""
    ids, counts, normals, points = (arrays[f"{name}.{update}.{f}"] for f in ("ids", "counts", "normals", "points"))
    return {(int(a), int(b)): (int(c), n.astype(np.float64), p[:int(c)].astype(np.float64))
            for (a, b), c, n, p in zip(ids, counts, normals, points)}


def _same_bits(man, other, what):
    assert man.keys() == other.keys(), f"{what}: {len(man)} manifolds against {len(other)}"
    for key, (c, n, p) in man.items():
        c2, n2, p2 = other[key]
        assert c == c2 and n.tobytes() == n2.tobytes() and p.tobytes() == p2.tobytes(), f"{what}: manifold {key} differs"


@pytest.mark.parametrize("threads,early", PROCESSES[1:])
def test_every_variant_gives_the_same_bits_in_both_updates(threads, early):
    first, other = _run(*PROCESSES[0]), _run(threads, early)
    assert first.keys() == other.keys()
    for key in first:
        if not key.endswith(".stats"):
            assert first[key].dtype == other[key].dtype and first[key].tobytes() == other[key].tobytes(), key
        else:
            assert np.array_equal(first[key], other[key]), key


def test_second_update_keeps_manifolds_of_the_first():
    """phys_stats.n_new_manifolds counts the manifolds whose pair had none in the update before: fewer than all of them
    means the narrow phase found entries of the first update in the colour table - the probe ran."""
    for threads, early in PROCESSES:
        arrays = _run(threads, early)
        for name in _input()[1]:
            manifolds, new = (int(x) for x in arrays[f"{name}.stats"])
            assert manifolds == len(arrays[f"{name}.2.ids"]) > 0, name
            assert new < manifolds, (name, manifolds, new)


@pytest.mark.parametrize("kind,order", BODY_WORLDS)
def test_first_update_is_the_in_process_run_and_holds_to_float64(kind, order):
    """Bit for bit what tests/test_gpu_shape_pairs.py checks, bodies and static partners; and its checks, with its caps,
    on what the 512-thread kernel gave (early probe; the late-probe process is held to the same bits first)."""
    arrays = _run("512", "1")
    for threads, early in PROCESSES:
        other = _run(threads, early)
        for name in (f"b.{kind}.{order}", f"s.{kind}.{order}"):
            for f in ("ids", "counts", "normals", "points"):
                assert other[f"{name}.1.{f}"].tobytes() == arrays[f"{name}.1.{f}"].tobytes(), (name, threads, early)
    arr, man_here = sp._bodies(kind, order)
    man = _manifolds(arrays, f"b.{kind}.{order}", 1)
    _same_bits(man, man_here, f"{kind} {order}")
    rep = spr.check(kind, arr["A"], arr["B"], arr["keys"], man, what=f"{kind} {order} 512 threads")
    rep.assert_ok()
    assert rep.counts.get("overlap", 0) > 0.15 * N_PAIRS, rep.summary()
    if kind != "BB":
        assert rep.counts.get("apart", 0) > 10, rep.summary()
    if kind == "BC":
        assert rep.counts.get("two points on a face", 0) > 30, rep.summary()
    if kind == "CC":
        assert rep.counts.get("capsule rule: 2 point(s)", 0) > 30, rep.summary()
    sarr, sman_here = sp._statics(kind, order)
    sman = _manifolds(arrays, f"s.{kind}.{order}", 1)
    _same_bits(sman, sman_here, f"{kind} {order} static")
    assert all(b & spr.STATIC_ID_BIT for _, b in sman)
    rep = spr.check(kind, sarr["A"], sarr["B"], sarr["keys"], sman, what=f"{kind} {order} static 512 threads")
    rep.assert_ok()
    if kind == "BC":
        assert rep.counts.get("two points on a face", 0) > 30, rep.summary()
    same = spr.check_same(sman, sarr["keys"], man, arr["keys"], f"{kind} {order} static vs body 512 threads")
    same.assert_ok(shares=False)
    assert same.hits > 0.25 * N_PAIRS


@pytest.mark.parametrize("gkind", list(spr.GROUND_KINDS))
def test_ground_manifolds_of_the_512_thread_kernel_hold_to_float64(gkind):
    arrays = _run("512", "1")
    for f in ("ids", "counts", "normals", "points"):
        assert _run("512", "0")[f"g.{gkind}.1.{f}"].tobytes() == arrays[f"g.{gkind}.1.{f}"].tobytes()
    arr = _ground(gkind)
    rep = spr.check_ground(gkind, arr["A"], arr["keys"], _manifolds(arrays, f"g.{gkind}", 1))
    rep.assert_ok()
    if gkind == "C":
        assert rep.counts.get("two points", 0) > 50, rep.summary()
