"""GPU: every shape pair of the narrow phase held to the float64 geometry of tests/shape_pair_ref.py - sphere, box and
capsule against each other in both index orders, against the same shape as a static collider, and against the ground
plane. A few thousand isolated pairs of one kind per world, one update, gravity and offset 0 so the poses are the ones
set; the checks (existence, ids, unit normal, closest direction, depth, push-out, point counts, point placement, order
symmetry, static path == body path) are those of shape_pair_ref, which tests/test_shape_pairs_cpu.py runs through the CPU
oracle. Neither this file nor shape_pair_ref shares code with the collision header or the oracle."""
import functools

import pytest

import shape_pair_ref as spr
from test_gpu_independent import DT, pair_world

pytestmark = pytest.mark.gpu
N_PAIRS, SEEDS = spr.N_PAIRS, spr.SEEDS


def _run(w):
    w.update(DT)
    w.sync()
    man = spr.manifolds_of(w)
    w.close()
    return man


@functools.lru_cache(maxsize=None)
def _scene(kind):
    return spr.scene(kind, N_PAIRS, SEEDS[kind])


@functools.lru_cache(maxsize=None)
def _bodies(kind, order):
    arr = spr.arrange(_scene(kind), order)
    return arr, _run(pair_world(arr["pos"], arr["rot"], arr["shape"], arr["he"]))


@functools.lru_cache(maxsize=None)
def _statics(kind, order):
    arr = spr.arrange_static(_scene(kind), order)
    b, s = arr["body"], arr["static"]
    w = pair_world(b["pos"], b["rot"], b["shape"], b["he"])
    w.set_static_bodies(s["pos"], rot=s["rot"], shape_type=s["shape"], half_extent=s["he"])
    return arr, _run(w)


@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("kind", list(spr.KINDS))
def test_body_pairs_hold_to_the_float64_geometry(kind, order):
    arr, man = _bodies(kind, order)
    rep = spr.check(kind, arr["A"], arr["B"], arr["keys"], man, what=f"{kind} {order}")
    rep.assert_ok()
    assert rep.counts.get("overlap", 0) > 0.15 * N_PAIRS, rep.summary()
    if kind != "BB":
        assert rep.counts.get("apart", 0) > 10, rep.summary()
    if kind == "BC":
        assert rep.counts.get("two points on a face", 0) > 30, rep.summary()
    if kind == "CC":
        assert rep.counts.get("capsule rule: 2 point(s)", 0) > 30, rep.summary()


@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("kind", list(spr.KINDS))
def test_static_partners_hold_to_the_float64_geometry_and_equal_the_body_path(kind, order):
    """B of every pair as static collider k (partner id STATIC_ID_BIT | k), A as body k: the float64 checks on those
    manifolds, and the manifold of the same two shapes as bodies (A the lower index), bit for bit."""
    arr, man = _statics(kind, order)
    assert all(b & spr.STATIC_ID_BIT for _, b in man)
    rep = spr.check(kind, arr["A"], arr["B"], arr["keys"], man, what=f"{kind} {order} static")
    rep.assert_ok()
    if kind == "BC":
        assert rep.counts.get("two points on a face", 0) > 30, rep.summary()
    body, man_body = _bodies(kind, order)
    same = spr.check_same(man, arr["keys"], man_body, body["keys"], f"{kind} {order} static vs body")
    same.assert_ok(shares=False)
    assert same.hits > 0.25 * N_PAIRS


@pytest.mark.parametrize("kind", [k for k in spr.KINDS if k != "BB"])
def test_both_index_orders_give_the_same_manifold(kind):
    (ab, man_ab), (ba, man_ba) = _bodies(kind, "ab"), _bodies(kind, "ba")
    rep = spr.check_symmetry(kind, ab, man_ab, ba, man_ba)
    rep.assert_ok(shares=False)
    assert rep.hits > 0.25 * N_PAIRS


@pytest.mark.parametrize("gkind", list(spr.GROUND_KINDS))
def test_ground_manifolds_hold_to_the_float64_geometry(gkind):
    arr = spr.ground_scene(gkind, N_PAIRS, SEEDS[gkind])
    man = _run(pair_world(arr["pos"], arr["rot"], arr["shape"], arr["he"], ground=True))
    rep = spr.check_ground(gkind, arr["A"], arr["keys"], man)
    rep.assert_ok()
    if gkind == "C":
        assert rep.counts.get("two points", 0) > 50, rep.summary()
