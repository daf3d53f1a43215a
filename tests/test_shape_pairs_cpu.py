"""CPU: the float64 shape-pair reference of tests/shape_pair_ref.py and its checks, driven through the CPU oracle
(OracleWorld.collide_now) over the generators and seeds that tests/test_gpu_shape_pairs.py runs on the GPU. The oracle
compiles the collision header the kernels compile, so this validates the reference, its tolerances and the shares of
contacts / misses / skipped pairs without a GPU, and measures the figures the tolerances are taken from (printed by every
test: run with -s). The oracle has no static colliders: those arrangements are GPU only."""
import numpy as np
import pytest

import physics_amd
import query_ref as qref
import shape_pair_ref as spr

N_PAIRS, SEEDS = spr.N_PAIRS, spr.SEEDS   # the scenes of the GPU suite


def oracle_manifolds(arr, ground=False):
    from oracle import binding as ob
    flags = physics_amd.FLAG_COLLISIONS | (physics_amd.FLAG_GROUND_PLANE if ground else 0)
    cfg = physics_amd.default_config(flags=flags, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0), contact_margin=spr.MARGIN)
    w = ob.OracleWorld(cfg, trig=ob.TRIG_DET)
    w.set_bodies(arr["pos"], rot=arr["rot"], shape_type=arr["shape"], half_extent=arr["he"])
    w.collide_now()
    man = spr.manifolds_of(w)
    w.close()
    return man


def test_closed_form_distances_match_the_golden_section_of_query_ref():
    """The reference's own error: its closed-form gaps against query_ref.separation (golden section over the core) on the
    committed capsule scenes, for every pair whose cores are apart."""
    worst = 0.0
    n = 0
    for kind in ("SC", "BC", "CC"):
        sc = spr.scene(kind, 400, SEEDS[kind])
        arr = spr.arrange(sc, "ab")
        for a, b in zip(arr["A"], arr["B"]):
            gap, _, cdist = spr.pair_gap(a, b)
            if cdist < 1e-6:
                continue
            other = qref.separation(a.type, a.c, a.R, a.h, b.type, b.c, b.R, b.h)
            worst = max(worst, abs(gap - other))
            n += 1
    print(f"closed form vs golden section: worst difference {worst:.3g} over {n} pairs")
    assert n > 900 and worst < 1e-7


def test_segment_distances_against_dense_sampling():
    """seg_segs and seg_box against a brute-force sampling of both segments / of the core (an upper bound that a
    closed form must not exceed, and must come within the sampling step of)."""
    rng = np.random.default_rng(0)
    t = np.linspace(-1.0, 1.0, 401)
    for _ in range(200):
        ca, cb = rng.normal(size=3), rng.normal(size=3)
        ua, ub = spr._unit(rng.normal(size=3)), spr._unit(rng.normal(size=3))
        ha, hb = rng.uniform(0, 1.5), rng.uniform(0, 1.5)
        d, pa, pb = spr.seg_segs(ca, ua, ha, cb, ub, hb)
        pts_a = ca + t[:, None] * ha * ua
        pts_b = cb + t[:, None] * hb * ub
        brute = np.linalg.norm(pts_a[:, None] - pts_b[None], axis=2).min()
        assert d[0] <= brute + 1e-12 and brute - d[0] < 0.01
        assert abs(np.linalg.norm(pa[0] - pb[0]) - d[0]) < 1e-12
        box = spr.Shape(spr.BOX, cb, spr.quat_to_matrix(spr._unit(rng.normal(size=4))), rng.uniform(0.3, 1.0, size=3))
        d2, p, q = spr.seg_box(ca, ua, ha, box)
        local = (pts_a - box.c) @ box.R
        brute = np.linalg.norm(np.maximum(np.abs(local) - box.h, 0.0), axis=1).min()
        assert d2 <= brute + 1e-12 and brute - d2 < 0.01


@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("kind", list(spr.KINDS))
def test_oracle_manifolds_hold_to_the_float64_geometry(kind, order):
    sc = spr.scene(kind, N_PAIRS, SEEDS[kind])
    arr = spr.arrange(sc, order)
    rep = spr.check(kind, arr["A"], arr["B"], arr["keys"], oracle_manifolds(arr), what=f"{kind} {order}")
    rep.assert_ok()
    regimes = rep.counts
    assert regimes.get("overlap", 0) > 0.15 * N_PAIRS, rep.summary()
    if kind != "BB":
        assert regimes.get("apart", 0) > 10, rep.summary()
    if kind == "BC":
        assert regimes.get("two points on a face", 0) > 30, rep.summary()
    if kind == "CC":
        assert regimes.get("capsule rule: 2 point(s)", 0) > 30, rep.summary()


@pytest.mark.parametrize("kind", [k for k in spr.KINDS if k != "BB"])
def test_oracle_manifolds_are_the_same_in_both_index_orders(kind):
    sc = spr.scene(kind, N_PAIRS, SEEDS[kind])
    ab, ba = spr.arrange(sc, "ab"), spr.arrange(sc, "ba")
    rep = spr.check_symmetry(kind, ab, oracle_manifolds(ab), ba, oracle_manifolds(ba))
    rep.assert_ok(shares=False)
    assert rep.hits > 0.25 * N_PAIRS


@pytest.mark.parametrize("gkind", list(spr.GROUND_KINDS))
def test_oracle_ground_manifolds_hold_to_the_float64_geometry(gkind):
    arr = spr.ground_scene(gkind, N_PAIRS, SEEDS[gkind])
    rep = spr.check_ground(gkind, arr["A"], arr["keys"], oracle_manifolds(arr, ground=True))
    rep.assert_ok()
    if gkind == "C":
        assert rep.counts.get("two points", 0) > 50, rep.summary()
