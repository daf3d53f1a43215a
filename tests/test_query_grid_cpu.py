"""CPU: the references and scenes behind tests/test_gpu_query_grid.py.

The float64 ray-capsule test on closed-form cases and against tests/capsule_ref.py; `centre` handling (a scene translated
and re-centred gives the same float64 answers); every row of the scene table (tests/query_scenes.py); the references' own
ambiguous population per scene and query set, within half of each acceptance cap (tests/query_accept.py); and the bound
on the grid's size: the float32 rule of rc_grid.hpp never exceeds 65 536 cells per axis and never coarsens."""
import math

import numpy as np
import pytest

import capsule_ref as cref
import query_accept as qa
import query_cases as qc
import query_ref
import query_scenes as qs
import raycast_ref as ref

S2 = math.sqrt(0.5)
Q_Z90 = [0.0, 0.0, S2, S2]  # local y (the capsule's axis) -> world -x


def _caps(pos, rot, he):
    n = len(pos)
    return dict(pos=np.array(pos, np.float64), rot=np.array(rot, np.float64), half_extent=np.array(he, np.float64), shape=np.full(n, 3))


# ---- 1. the capsule ray reference ----------------------------------------------------------------------------------------
def test_ray_capsule_closed_form_cases():
    # an upright capsule of radius 0.5 and core half-length 1 at (0, 5, 0), and one lying along x at (10, 5, 0)
    b = _caps([[0, 5, 0], [10, 5, 0]], [[0, 0, 0, 1], Q_Z90], [[0.5, 1, 0], [0.5, 1, 0]])
    cases = [  # origin, direction, body, t, normal
        ([-5, 5.5, 0], [1, 0, 0], 0, 4.5, [-1, 0, 0]),                    # the cylinder's side, square on
        ([-5, 5.5, 0.3], [1, 0, 0], 0, 5 - 0.4, [-0.8, 0, 0.6]),          # the side, off axis
        ([0, 10, 0], [0, -1, 0], 0, 3.5, [0, 1, 0]),                      # the top end ball, along the axis
        ([0.3, 10, 0], [0, -2, 0], 0, 4 - 0.4, [0.6, 0.8, 0]),            # the end ball, off axis (direction not unit)
        ([-5, 6.3, 0], [1, 0, 0], 0, 5 - 0.4, [-0.8, 0.6, 0]),            # the end ball from the side, above the seam
        ([-5, 6.0, 0], [1, 0, 0], 0, 4.5, [-1, 0, 0]),                    # exactly at the seam: side and ball agree
        ([0.2, 5.9, 0.1], [0, 0, 1], 0, 0.0, [0, 0, -1]),                 # from inside: t = 0, -u
        ([-5, 6.6, 0], [1, 0, 0], ref.MISS, math.inf, [0, 0, 0]),         # over the top
        ([0.6, 10, 0], [0, -1, 0], ref.MISS, math.inf, [0, 0, 0]),        # parallel to the axis, outside the radius
        ([5, 5, -5], [0, 0, 1], ref.MISS, math.inf, [0, 0, 0]),           # between the two
        ([10, 10, 0], [0, -1, 0], 1, 4.5, [0, 1, 0]),                     # the lying capsule's side from above
        ([5, 5.3, 0], [1, 0, 0], 1, 4 - 0.4, [-0.8, 0.6, 0]),             # the lying capsule's end ball, along its axis
        ([10.5, 5, 5], [0, 0, -3], 1, 4.5, [0, 0, 1]),
        ([11.3, 5, 5], [0, 0, -1], 1, 5 - 0.4, [0.6, 0, 0.8]),            # its end ball beyond the core's end
    ]
    h = ref.cast([c[0] for c in cases], [c[1] for c in cases], b)
    for k, c in enumerate(cases):
        assert h["body"][k] == c[2], (k, c, h["body"][k], h["t"][k])
        if math.isinf(c[3]):
            assert h["t"][k] == math.inf and not h["normal"][k].any(), (k, h["t"][k])
        else:
            assert abs(h["t"][k] - c[3]) <= 1e-12, (k, h["t"][k], c[3])
            assert np.abs(h["normal"][k] - np.array(c[4], np.float64)).max() <= 1e-12, (k, h["normal"][k], c[4])
    # chords: through the middle of the side 2 r; along the axis the whole length; a tangent line none
    assert abs(h["span"][0] - 1.0) <= 1e-12 and abs(h["span"][2] - 3.0) <= 1e-12
    graze = ref.cast([[-5, 5.5, 0.5], [-5, 5.5, 0.5 + 1e-9]], [[1, 0, 0], [1, 0, 0]], b)
    assert graze["body"][0] == 0 and graze["span"][0] <= 1e-6 and graze["body"][1] == ref.MISS


def test_ray_capsule_agrees_with_capsule_ref_on_its_cases():
    """the scene of tests/test_gpu_capsule.py (capsule bodies and static capsules, rays aimed at them, origins inside)"""
    rng = np.random.default_rng(3)

    def scene(n):
        pos = rng.uniform(-8, 8, size=(n, 3)).astype(np.float32)
        pos[:, 1] += 10
        q = rng.normal(size=(n, 4)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
        he = np.column_stack([rng.uniform(0.2, 0.6, n), rng.uniform(0.0, 1.5, n), np.zeros(n)]).astype(np.float32)
        return pos, q, he

    pos, q, he = scene(120)
    spos, sq, she = scene(30)
    caps = [(pos[k], q[k], he[k]) for k in range(120)] + [(spos[k], sq[k], she[k]) for k in range(30)]
    ids = list(range(120)) + [ref.STATIC_ID_BIT | k for k in range(30)]
    targets = np.concatenate([pos, spos])[rng.integers(0, len(caps), 1000)] + rng.normal(scale=0.6, size=(1000, 3))
    origins = rng.uniform(-20, 20, size=(1000, 3))
    origins[:, 1] += 10
    origins[:20] = np.concatenate([pos, spos])[:20]
    dirs = (targets - origins).astype(np.float32)
    dirs[:20] = rng.normal(size=(20, 3))
    origins = origins.astype(np.float32)
    want = cref.raycast(origins, dirs, caps, ids)
    h = ref.cast(origins, dirs, dict(pos=pos, rot=q, half_extent=he, shape=np.full(120, 3)),
                 statics=dict(pos=spos, rot=sq, half_extent=she, shape=np.full(30, 3)))
    hits = 0
    for k, (kid, kt, kn, gap) in enumerate(want):
        if kid is None:
            assert h["body"][k] == ref.MISS, k
            continue
        hits += 1
        # (capsule_ref keeps the quaternion as it is, this reference normalises it: float32 quaternions, 1e-7 apart)
        assert h["body"][k] == kid or gap <= 1e-5, (k, h["body"][k], kid, gap)
        if h["body"][k] == kid:
            assert abs(h["t"][k] - kt) <= 1e-5 * (1 + kt), (k, h["t"][k], kt)
            assert np.abs(h["normal"][k] - kn).max() <= 1e-4 or h["span"][k] <= 1e-3, (k, h["normal"][k], kn)
            assert not math.isfinite(gap) or abs(h["t2"][k] - h["t"][k] - gap) <= 1e-5 * (1 + kt), (k, h["t2"][k], gap)
    assert hits > 500 and (h["t"][:20] == 0).all()
    assert (h["body"] >= ref.STATIC_ID_BIT).sum() > 50  # static ids among them


def test_statics_are_targets_with_their_own_ids_and_ignore_names_bodies_only():
    b = dict(pos=[[0, 5, 0]], rot=[[0, 0, 0, 1]], half_extent=[[1, 1, 1]], shape=[2])
    s = dict(pos=[[4, 5, 0], [8, 5, 0]], rot=None, half_extent=[[1, 0, 0], [0.5, 1, 0]], shape=[1, 3])
    o, d = [[-5, 5, 0]] * 3 + [[6, 5, 0]], [[1, 0, 0]] * 4
    h = ref.cast(o, d, b, ignore=[-1, 0, ref.STATIC_ID_BIT, 0], statics=s, ground=0.0)
    assert list(h["body"]) == [0, ref.STATIC_ID_BIT, 0, ref.STATIC_ID_BIT | 1]
    assert np.allclose(h["t"], [4, 8, 4, 1.5]) and np.allclose(h["t2"][:2], [8, 12.5])
    assert ref.t_of(h, 0, ref.STATIC_ID_BIT | 1) == 12.5 and ref.near_body(h, 0, ref.STATIC_ID_BIT, 8.0, 1e-9)


# ---- 2. centre ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far", "farther"])
def test_a_translated_scene_re_centred_gives_the_same_float64_answers(name):
    near, moved = qs.scene("near"), qs.scene(name)
    c = moved["centre"].astype(np.float64)
    assert np.array_equal(moved["bodies"]["pos"].astype(np.float64) - c, near["bodies"]["pos"].astype(np.float64))
    for a, b in zip(qc.ray_sets("near"), qc.ray_sets(name)):
        assert np.array_equal(b["o"].astype(np.float64) - c, a["o"].astype(np.float64))  # the same rays, translated exactly
        for k in ("body", "t", "t2", "span", "normal", "o"):
            assert np.array_equal(a["h"][k], b["h"][k]), (a["label"], k)
    sl = slice(0, 120)
    a, b = qc.overlap_set("near"), qc.overlap_set(name)
    assert a["want"] == b["want"]
    if name in qc.CAST_SCENES:
        a, b = qc.cast_set("near", "mixed"), qc.cast_set(name, "mixed")
        for k in ("body", "t", "t2", "normal"):
            assert np.array_equal(a["h"][k], b["h"][k], equal_nan=True), k
    # without the centre the far scene's rays still find the same targets (the exact test takes differences first; only
    # the candidate search expands squares, with slack for it), and no centre is a centre at the origin
    s = qc.ray_sets(name)[0]
    raw = ref.cast(s["o"][sl], s["d"][sl], moved["bodies"], ground=0.0, statics=moved["statics"])
    fin = np.isfinite(raw["t"]) & np.isfinite(s["h"]["t"][sl])
    assert fin.sum() > 40 and np.abs(raw["t"][fin] - s["h"]["t"][sl][fin]).max() <= 1e-6
    n0 = qc.ray_sets("near")[0]
    same = ref.cast(n0["o"][sl], n0["d"][sl], near["bodies"], ground=0.0, statics=near["statics"], centre=None)
    assert np.array_equal(same["t"], n0["h"]["t"][sl])


def test_centre_is_subtracted_from_casts_and_overlaps_too():
    sc = qs.scene("one")
    tg = qc.targets(sc)
    c = np.array([4096.0, 0.0, -8192.0])
    moved = dict(tg, pos=tg["pos"] + c)
    o, d = np.array([[-5.0, 2.0, -1.0], [3.0, 9.0, -1.0]]), np.array([[1.0, 0, 0], [0, -1.0, 0]])
    a = query_ref.spherecast(o, d, 0.25, tg, ground=0.0)
    b = query_ref.spherecast(o + c, d, 0.25, moved, ground=0.0, centre=c)
    assert np.array_equal(a["body"], b["body"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["o"], b["o"])
    assert list(a["body"]) == [0, 0] and np.allclose(a["t"], [8 - 1.003 - 0.25, 7 - 0.503 - 0.25])
    qa_ = query_ref.overlap([2, 1], [[3, 2, -1], [3, 0.2, 6]], None, [[1, 1, 1], [0.5, 0, 0]], tg, ground=0.0)
    qb = query_ref.overlap([2, 1], np.array([[3, 2, -1], [3, 0.2, 6]]) + c, None, [[1, 1, 1], [0.5, 0, 0]], moved, ground=0.0, centre=c)
    assert qa_ == qb and qa_[0][0] == [0] and qa_[1][0] == [ref.GROUND]
    # a centre with a height moves the ground with it
    up = np.array([0.0, 3.0, 0.0])
    qc_ = query_ref.overlap([1], np.array([[3, 0.2, 6]]) + up, None, [[0.5, 0, 0]], dict(tg, pos=tg["pos"] + up), ground=3.0, centre=up)
    assert qc_[0][0] == [ref.GROUND]


# ---- 3. every row of the scene table -------------------------------------------------------------------------------------
def _grid(name, grow=0.0):
    return qs.grid_of(qs.scene(name)["bodies"], grow)


def test_scene_near_reaches_two_scan_tiles_and_near2048_one():
    sc = qs.scene("near")
    b = sc["bodies"]
    assert len(b["pos"]) == 2049 and set(np.unique(b["shape"])) == {0, 1, 2, 3}
    assert 0.03 < (b["shape"] == 0).mean() < 0.07
    assert len(sc["statics"]["pos"]) == 4 and set(sc["statics"]["shape"]) == {1, 2, 3}
    ext = np.where(b["shape"][:, None] == 1, b["half_extent"][:, :1], b["half_extent"])
    assert ext[b["shape"] != 0].min() >= 0.2 and ext.max() <= 1.5
    assert 1 << _grid("near")["bits"] == 8192 and 1 << _grid("near2048")["bits"] == 4096
    s2 = qs.scene("near2048")["bodies"]
    assert all(np.array_equal(s2[k], b[k][:2048]) for k in b)
    assert b["shape"][2048] != 0  # the body that tips the table over is one a ray can hit


@pytest.mark.parametrize("name,pad", [("far", 0.9), ("farther", 3.0)])
def test_scene_far_and_farther_reach_their_pads(name, pad):
    g, near = _grid(name), _grid("near")
    assert g["pad"] > pad and near["pad"] < 1e-3
    assert g["cell"] > near["cell"] + 2 * pad  # the pad, not the bodies, sets the cell there
    assert not g["coarse"] and (g["dims"] >= 4).all()


def test_scene_flung_reaches_60000_cells_along_x():
    g = _grid("flung")
    assert g["dims"][0] >= 60_000 and g["dims"][1] <= 4 and g["dims"][2] <= 4 and not g["coarse"]
    b = qs.scene("flung")["bodies"]
    x = b["pos"][:, 0]
    assert (x[:300] < -1.4e6).all() and (x[300:600] > 1.4e6).all() and (np.abs(x[600:]) < 1.45e6).all() and len(x) == 640
    cross = qc.ray_sets("flung")[4]
    assert cross["label"] == "flung crossing" and 16 <= len(cross["o"]) <= 64
    assert (np.abs(cross["h"]["normal"][:, 0]) == 1.0).all()  # square on a face of an unturned box


def test_scene_one_flat_tiny_and_statics_only_reach_their_grids():
    assert list(_grid("one")["dims"]) == [1, 1, 1]
    g = _grid("flat")
    assert g["dims"][1] in (1, 2) and g["dims"][0] >= 32 and g["dims"][2] >= 32 and len(qs.scene("flat")["bodies"]["pos"]) == 1024
    assert np.unique(qs.scene("flat")["bodies"]["pos"][:, 1]).size == 1
    g = _grid("tiny")
    assert g["cell"] < 5e-3 and g["valid"] and (g["dims"] >= 4).all() and len(qs.scene("tiny")["bodies"]["pos"]) == 500
    g = _grid("statics_only")
    assert not g["valid"] and list(g["dims"]) == [1, 1, 1] and qs.scene("statics_only")["statics"] is not None
    assert not qs.scene("statics_only")["bodies"]["shape"].any()


def test_scene_crowd_puts_its_records_into_eight_cells_and_one_bucket_above_2048():
    g = _grid("crowd")
    load, cells = qs.bucket_loads(g)
    assert len(cells) <= 8 and load.max() > 2048 and load.sum() >= g["shaped"].sum()
    b = qs.scene("crowd")["bodies"]
    small = b["half_extent"][:3000]
    assert len(b["pos"]) == 3001 and small[b["shape"][:3000] != 0].min() >= 0.05 and small.max() <= 0.2
    assert b["half_extent"][3000].min() > 30.0


@pytest.mark.parametrize("name", qc.CAST_SCENES)
def test_the_largest_radius_grows_the_grid_into_at_most_eight_cells(name):
    sc = qs.scene(name)
    rad = qc.cast_set(name, "huge")["rad"]
    valid = rad[np.isfinite(rad) & (rad >= 0)]
    lo, hi = qs.bounds(sc)
    assert valid.max() == np.float32(4.0 * float((hi - lo).max())) and (~(np.isfinite(rad) & (rad >= 0))).sum() >= 1
    g = qs.grid_of(sc["bodies"], grow=float(valid.max()))
    assert int(np.prod(g["dims"])) <= 8
    assert int(np.prod(_grid(name)["dims"])) > 1


def test_mixed_radii_hold_invalid_ones_and_reach_beyond_the_bodies():
    rad = qc.cast_set("near", "mixed")["rad"]
    bad = ~(np.isfinite(rad) & (rad >= 0))
    assert 0.005 * len(rad) < bad.sum() < 0.04 * len(rad)
    assert np.isnan(rad).any() and np.isinf(rad).any() and (rad < 0).any() and np.nanmax(rad[~bad]) > 1.4


# ---- 4. the references' own ambiguous cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qs.NAMES)
def test_ambiguous_rays_stay_within_half_the_cap(name):
    for s in qc.ray_sets(name):
        n = len(s["o"])
        if s["label"] == "flung crossing":
            # t is 3e6 there and the tolerance 45: above every chord a scene of 60 000 cells can hold (its bodies' edges stay
            # below 4.2), so every hit counts as ambiguous by that measure. These rays are held instead to what float32
            # resolves at that t (0.25): chords of CROSS_MIN_SPAN at least and no second target within CROSS_MIN_GAP, on
            # lines that float32 and float64 see alike (exact origins, directions along x)
            h = s["h"]
            assert (h["span"] >= qc.CROSS_MIN_SPAN).all() and (h["t2"] - h["t"] >= qc.CROSS_MIN_GAP).all() and (h["t"] > 2.9e6).all()
            continue
        count = int(qc.ambiguous_rays(s["h"]).sum())
        print(f"{s['label']}: {count} ambiguous of {n} (cap {qa.ray_cap(n)})")
        assert 2 * count <= qa.ray_cap(n), (s["label"], count)


@pytest.mark.parametrize("name", qs.NAMES)
def test_ambiguous_overlaps_stay_within_half_the_cap(name):
    s = qc.overlap_set(name)
    n = len(s["q"][1])
    count = qc.ambiguous_overlaps(s["want"])
    print(f"{s['label']}: {count} pairs within 1e-4 of touching of {n} queries (cap {qa.overlap_cap(n)})")
    assert n == qc.N_OVERLAPS and 2 * count <= qa.overlap_cap(n), (name, count)
    assert set(np.unique(s["q"][0])) == {1, 2, 3}


# ---- 5. the bound on the grid -------------------------------------------------------------------------------------------
def test_the_grid_never_exceeds_65536_cells_per_axis_and_never_coarsens():
    """cell >= 2 pad >= 2^-15 (M + e) and span <= 2 M + 2 pad, so span / cell stays below 65 474: the clamp to 2^20 cells of
    rc_grid.hpp never binds. Swept in the rule's own float32 arithmetic over bounds from 1e-30 to 1e37 and edges from 0 to
    the whole span, with the worst case (bounds symmetric about the origin, edge zero) among them."""
    rng = np.random.default_rng(5)
    worst, worst_in = 0, None
    cases = []
    for mag in np.logspace(-30, 37, 68):
        for e_rel in (0.0, 1e-12, 1e-7, 2.0 ** -16, 1e-3, 1.0):
            cases.append(((-mag, -mag, -mag), (mag, mag, mag), e_rel * mag))
            cases.append(((-mag, 0.0, 0.0), (mag, 0.0, 0.0), e_rel * mag))
            cases.append(((mag, mag, mag), (mag * (1 + 1e-6), mag, mag * 2), e_rel * mag))
    for _ in range(3000):
        mag = 10.0 ** rng.uniform(-30, 37)
        a, b = rng.uniform(-mag, mag, 3), rng.uniform(-mag, mag, 3)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        cases.append((lo, hi, float((hi - lo).max()) * 10.0 ** rng.uniform(-12, 0)))
    for lo, hi, e in cases:
        g = qs.grid_rule(np.float32(lo), np.float32(hi), np.float32(e))
        assert not g["coarse"], (lo, hi, e)
        assert np.isfinite(g["cell"]) and g["cell"] > 0
        if int(g["dims"].max()) > worst:
            worst, worst_in = int(g["dims"].max()), (lo, hi, e)
    print(f"most cells per axis: {worst} at {worst_in}")
    assert 65_000 < worst <= 65_536, (worst, worst_in)
