"""GPU: every variant of the pair search (physics_amd/csrc/broadphase.hip: the slot grid, the brick kernel with either
stage, one and four lanes per body) held to the numpy reference of tests/pair_ref.py - float64 boxes written from the ABI
header's definitions, the pair set by sort-and-sweep - at 33 000 bodies, the smallest round size at which those kernels
run. The library reads its switches once per process, so tools/pair_probe.py runs each variant in a fresh process and
writes boxes and pairs to files; which kernel a set of switches gives, for any hint, is the table at the end of
tests/cpp/plan_probe.cpp. The scenes, and the case each one reaches (staged and unstaged bricks, the flush inside a brick,
a scene longer than the bucket table, either side of the brick stage rule), are checked on the CPU in
tests/test_pair_ref_cpu.py, where the tolerance of the boxes is measured as well.

Everything but the boxes is a set: compared exactly. A process that fails ends its tests; nothing is run twice."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_CAPACITY = -5
VARIANTS = {
    "lanes4": {"PHYS_DEBUG_PAIR_LANES": "4"},
    "lanes1": {"PHYS_DEBUG_PAIR_LANES": "1"},
    "brick128": {"PHYS_DEBUG_PAIR_KERNEL": "brick", "PHYS_DEBUG_BRICK_STAGE": "128"},
    "brick256": {"PHYS_DEBUG_PAIR_KERNEL": "brick", "PHYS_DEBUG_BRICK_STAGE": "256"},
    "unforced": {},
}
FORCED = [v for v in VARIANTS if v != "unforced"]
SWITCHES = ("PHYS_DEBUG_PAIR_LANES", "PHYS_DEBUG_PAIR_KERNEL", "PHYS_DEBUG_BRICK_STAGE")
SCENES = list(pr.SCENES)
_dir = None


@pytest.fixture(autouse=True, scope="module")
def _files(tmp_path_factory):
    global _dir
    _dir = str(tmp_path_factory.mktemp("pair_probe"))
    yield
    _probe.cache_clear()
    _reference.cache_clear()


@functools.lru_cache(maxsize=None)
def _probe(variant, *args):
    """One run of tools/pair_probe.py under the variant's switches; the directory of its files, or the failure - kept, so
    that every test of a failed run reports it and none starts it again."""
    out = os.path.join(_dir, variant + "_" + "_".join(a.strip("-").replace(",", "+") for a in args))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(VARIANTS[variant])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pair_probe.py"), "pairs", "--out", out, *args],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return None, f"pair_probe {variant} {args}: no end after {e.timeout} s"
    if r.returncode != 0:
        return None, f"pair_probe {variant} {args}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    return out, None


def _load(variant, name, updates, *args, n=pr.N):
    out, failure = _probe(variant, *args)
    assert failure is None, failure
    return np.load(os.path.join(out, f"{name}_n{n}_u{updates}.npz"))


def _all_scenes():
    return ("--scenes", ",".join(SCENES), "--updates", "0,3")


@functools.lru_cache(maxsize=None)
def _reference(box_bytes, n):
    """pair_ref.pairs of a box array, once per distinct array (every process must report the same boxes)."""
    return pr.pairs(np.frombuffer(box_bytes, np.float32).reshape(n, 6))


def _expected(box):
    return _reference(np.ascontiguousarray(box, np.float32).tobytes(), len(box))


def _check_set(got, box, what):
    want = _expected(box)
    assert got.dtype == np.uint32 and got.ndim == 2 and got.shape[1] == 2
    assert (got[:, 0] < got[:, 1]).all(), f"{what}: a pair with i >= j"
    key = got[:, 0].astype(np.uint64) << np.uint64(32) | got[:, 1].astype(np.uint64)
    assert (key[1:] > key[:-1]).all(), f"{what}: pairs not strictly sorted (a pair twice?)"
    ref = want[:, 0].astype(np.uint64) << np.uint64(32) | want[:, 1].astype(np.uint64)
    missing, extra = np.setdiff1d(ref, key), np.setdiff1d(key, ref)
    print(f"{what}: {len(got)} pairs, reference {len(want)}")
    assert len(missing) == 0 and len(extra) == 0, (
        f"{what}: {len(got)} pairs, reference {len(want)}; {len(missing)} missing (first {missing[:3] >> np.uint64(32)}, "
        f"{missing[:3] & np.uint64(0xFFFFFFFF)}), {len(extra)} not in the reference")
    assert len(want) >= len(box) // 2, "a scene with few pairs checks little"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_pair_set_is_the_reference_set(variant, name):
    """From phys_set_bodies (no hint) and after three updates (a hint: the brick kernel's stage is then sized from the
    largest region met, the unforced world picks by crowding and pair count)."""
    for updates in (0, 3):
        first = _load("lanes4", name, updates, *_all_scenes())["aabb"]
        d = _load(variant, name, updates, *_all_scenes())
        assert np.array_equal(d["aabb"].view(np.uint32), first.view(np.uint32)), "boxes differ between two processes"
        _check_set(d["pairs"], d["aabb"], f"{variant} {name} after {updates} updates")
        assert int(d["n_pairs"]) == len(d["pairs"])
        if updates:
            assert int(d["n_pairs_update"]) == len(_expected(d["aabb_before"])), "phys_stats.n_pairs of the third update"


@pytest.mark.parametrize("name", SCENES)
def test_boxes_hold_to_float64_and_contain_it(name):
    sc = pr.scene(name)
    got = _load("lanes4", name, 0, *_all_scenes())["aabb"]
    none = sc["shape"] == pr.SHAPE_NONE
    assert none.sum() > 1000 and (got[none, :3] > got[none, 3:]).all(), "a body without a shape has the inverted box"
    worst, short = pr.box_errors(got, pr.aabbs(sc["pos"], sc["rot"], sc["shape"], sc["he"]), sc["shape"])
    print(f"{name}: worst deviation {worst:.3f} ulps, worst shortfall {short:.3f} ulps (tolerance {pr.AABB_TOL_ULPS})")
    assert worst <= pr.AABB_TOL_ULPS
    assert short <= pr.AABB_TOL_ULPS, "a box smaller than the float64 one loses contacts"


@pytest.mark.parametrize("n", [32768, 32769])
def test_either_side_of_the_slot_grid(n):
    """32 768 bodies are the slot grid's last size, 32 769 the sorted grid's first (plan.hpp kSlotGridMaxBodies, held by
    tests/test_pair_ref_cpu.py): the same soup, one body more."""
    d = _load("unforced", "many_pairs", 0, "--scenes", "many_pairs", "--n", str(n), n=n)
    assert len(d["aabb"]) == n
    _check_set(d["pairs"], d["aabb"], f"unforced many_pairs n = {n}")


@pytest.mark.parametrize("variant", FORCED)
def test_pairs_beyond_their_capacity_are_reported_and_the_next_world_is_right(variant):
    """The dense scene with room for 10 000 pairs: the flushes of every kernel stay inside the buffer (the `dst <
    max_pairs` guards) and the call says PHYS_ERR_CAPACITY; a world with room, in the same process, gives the full set."""
    d = _load(variant, "dense", 0, "--scenes", "dense", "--capacity", "10000")
    assert int(d["capacity_code"]) == ERR_CAPACITY
    _check_set(d["pairs"], d["aabb"], f"{variant} dense behind an overflow")
    assert len(d["pairs"]) > 10000
