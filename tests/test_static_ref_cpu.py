"""CPU: the scenes of tests/static_ref.py checked against the cases they are named for, with the grid taken from
build_static_set itself (tests/cpp/static_set_cli.cpp) and the body boxes from the CPU oracle's get_aabbs() (bit-equal to
the device's, as tests/test_pair_ref_cpu.py takes them), so that tests/test_gpu_static_independent.py cannot pass by missing
its case. Also: the float32 static boxes held to the float64 definition, no pair of a committed scene within rounding of
the boxes' touching (other than the exact ones of `touching`), and - through the oracle with the statics appended as bodies
n + k - every pair a contact or a clear miss that shape_pair_ref.check accepts. Every test prints its figures (run with -s)."""
import functools

import numpy as np
import pytest

import pair_ref as pr
import shape_pair_ref as spr
import static_ref as sr
from test_gpu_static_independent import BODY_PATH_LEFT_OUT, build_cli, check_manifolds, cli_boxes

NAMES = list(sr.SCENES)


@pytest.fixture(scope="module")
def static_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("static_set")
    exe = build_cli(d)
    cache = {}

    def run(name):
        if name not in cache:
            cache[name] = cli_boxes(exe, d, name, sr.scene(name))
        return cache[name]
    return run


def _oracle(sc, with_statics):
    import physics_amd
    from oracle import binding as ob
    b, s = sc["body"], sc["static"]
    arr = {k: (np.concatenate([b[k], s[k]]) if with_statics else b[k]) for k in ("pos", "rot", "shape", "he")}
    n = len(arr["pos"])
    cfg = physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0),
                                     contact_margin=sc["margin"], max_pairs=64 * n, max_manifolds=64 * n)
    o = ob.OracleWorld(cfg, trig=ob.TRIG_DET)
    o.set_bodies(arr["pos"], rot=arr["rot"], shape_type=arr["shape"], half_extent=arr["he"])
    return o


@functools.lru_cache(maxsize=None)
def _body_boxes(name):
    sc = sr.scene(name)
    o = _oracle(sc, False)
    box = o.get_aabbs()
    o.close()
    return sc, box


def _per_body(pairs, n):
    return int(np.bincount(pairs[:, 0], minlength=n).max()) if len(pairs) else 0


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_static_pairs_by_hand():
    body = np.array([[0, 0, 0, 1, 1, 1], [np.nextafter(np.float32(1), np.float32(2)), 0, 0, 2, 1, 1], [1, 1, 1, 2, 2, 2],
                     [3e38, 3e38, 3e38, -3e38, -3e38, -3e38], [np.nan] * 6, [0, 0, 0, 1, np.nan, 1]], np.float32)
    static = np.array([[1, 1, 1, 3, 3, 3], [-1, -1, -1, 1, 0, 0], [-9, -9, -9, 9, 9, 9]], np.float32)
    assert sr.static_pairs(body, static).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 2]]  # (1, 1): one ulp apart
    assert sr.static_pairs(body[3:], static).shape == (0, 2)


# ---- the scenes reach their cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scene_reaches_its_case(name, static_set):
    sc, body_box = _body_boxes(name)
    box, f = static_set(name)
    pairs = sr.static_pairs(body_box, box)
    n, ns = len(body_box), len(box)
    assert n <= 1000 and ns <= 600
    per_body = _per_body(pairs, n)
    row = (len(pairs), f["n_large"], f["dim"], f["longest"], f["span"], f["first"], f["multi"], per_body)
    print(f"{name}: {n} bodies, {ns} statics, table row {row}, cell {f['cell']:.6g}, origin {f['org']}, one static in up to {f['cells']} cells")
    assert sr.SCENE_TABLE[name][:8] == row
    large = np.zeros(ns, bool)
    if f["n_large"]:
        # which statics are on the list: the ones the grid figures leave out cannot be told from the figures, so by extent
        edge = (box[:, 3:] - box[:, :3]).astype(np.float64)
        cell0 = np.sort(edge.max(axis=1).astype(np.float32))[ns // 2]
        large = np.prod(np.floor(edge / float(cell0)) + 2.0, axis=1) > 64
        assert large.sum() == f["n_large"]
    if name.startswith("tiles"):
        assert f["longest"] >= 6 and f["multi"] >= 500 and f["n_large"] == 0
        if n >= 63:
            assert per_body >= 10
        if n == 257:
            assert len(pairs) > 1028 + 1000, "the capacity test needs a count well past the floor of max(4 n, 1024)"
    if name.startswith("mixed"):
        assert f["n_large"] >= 6 and f["cells"] >= 27, "one small static in 27 cells or more"
        has = sc["body"]["shape"] != pr.SHAPE_NONE
        assert (~has).sum() >= n // 25 and not np.isin(pairs[:, 0], np.nonzero(~has)[0]).any()
        with_large = int(large[pairs[:, 1]].sum())
        # bodies with pairs whose box reaches outside the grid's bounds (their cells are clamped)
        lo = np.asarray(f["org"])
        hi = lo + np.asarray(f["dim"]) * f["cell"]
        out = ((body_box[:, :3] < lo) | (body_box[:, 3:] > hi)).any(axis=1)
        out_with_pairs = len(np.intersect1d(np.nonzero(out)[0], pairs[:, 0]))
        print(f"{name}: {with_large} pairs with LARGE statics, {out_with_pairs} bodies with pairs reach outside the grid")
        assert with_large >= 20 and len(pairs) - with_large >= 20, "the list and the grid answer together"
        assert out_with_pairs >= 10 and (per_body >= 30 or n < 1000), "a lane of k_static_fill with dozens of pairs"
    if name.startswith("line"):
        a = sr.AXES.index(name[-1])
        assert f["first"][a] >= 512 and f["dim"][a] > 512 and max(f["dim"][b] for b in range(3) if b != a) <= 8
        far = [0, 100, 200, 256]
        assert not np.isin(pairs[:, 0], far).any() and (np.abs(sc["body"]["pos"][far, a]) > 1550).all()
        assert len(pairs) >= 200
        where = sc["static"]["pos"][pairs[:, 1], a]
        assert (where > 100).sum() >= 30, "pairs with statics whose first cell is past 512"
        assert (np.abs(where) < 95).sum() >= 80, "pairs near the origin: contents checked in full"
    if name == "touching":
        m = sc["margin"]
        assert m == 2.0 ** -5 and f["cell"] == 1.0 and f["org"] == (9.0, 9.0, 9.0), "a dyadic cell on a dyadic origin"
        # every fattened box is exact: the float32 boxes equal the float64 ones
        assert np.array_equal(box.astype(np.float64), sr.static_boxes64(sc["static"], m))
        b = sc["body"]
        assert np.array_equal(body_box.astype(np.float64), pr.aabbs(b["pos"], b["rot"], b["shape"], b["he"], m))
        have = {(int(i), int(k)) for i, k in pairs}
        for i, k in sc["touch"]:
            assert (int(i), int(k)) in have
            assert ((body_box[i, :3] == box[k, 3:]) | (body_box[i, 3:] == box[k, :3])).sum() == 1, "touches in exactly one face"
        for i, k in sc["apart"]:
            assert (int(i), int(k)) not in have
            d = np.maximum(body_box[i, :3].astype(np.float64) - box[k, 3:], box[k, :3].astype(np.float64) - body_box[i, 3:]).max()
            assert d == 2.0 ** -20, "one float32 ulp of [8, 16) apart"
        for i, k in sc["inside"]:
            assert (int(i), int(k)) in have
            faces = np.concatenate([body_box[i, :3], body_box[i, 3:]]) - 9.0
            mid = 0.5 * (box[k, :3] + box[k, 3:])
            on = [(a, s) for a in range(3) for s in (0, 1) if body_box[i, 3 * s + a] == mid[a] and float(faces[3 * s + a]).is_integer()
                  and box[k, a] < mid[a] < box[k, 3 + a] and body_box[i, a] != box[k, a]]
            assert on, "a body face on a cell boundary in the middle of its static"
        assert len(pairs) == 12
    if name == "only_large":
        small = np.nonzero(~large)[0]
        assert f["n_large"] == 3 and len(small) == 4
        assert not np.isin(pairs[:, 1], small).any() and len(pairs) >= 100, "every pair comes from the LARGE list"
        assert (np.abs(body_box[:, :3]).max() < 20) and box[small, 0].min() > 190
        corner = np.bincount(pairs[:, 0], minlength=n)
        assert (corner >= 3).sum() >= 5, "bodies that meet the slab and both walls"
    if name == "one":
        assert ns == 1 and 1 <= len(pairs) < n


def test_static_boxes_hold_to_float64(static_set):
    worst = {}
    for name in NAMES:
        sc = sr.scene(name)
        box, _ = static_set(name)
        worst[name] = pr.box_errors(box, sr.static_boxes64(sc["static"], sc["margin"]), sc["static"]["shape"])
    print({k: (round(a, 3), round(b, 3)) for k, (a, b) in worst.items()})
    measured = max(a for a, _ in worst.values())
    print(f"static boxes: worst deviation {measured:.3f} ulps (the bodies' boxes: {pr.MEASURED_AABB_ULPS}; tolerance {pr.AABB_TOL_ULPS})")
    assert measured <= pr.AABB_TOL_ULPS and max(b for _, b in worst.values()) <= pr.AABB_TOL_ULPS
    assert 0.9 * sr.MEASURED_STATIC_BOX_ULPS < measured <= sr.MEASURED_STATIC_BOX_ULPS, measured


@pytest.mark.parametrize("name", NAMES)
def test_no_pair_is_within_rounding_of_touching(name, static_set):
    """A condition on the scenes: the float64 boxes of no (body, static) combination come within 2 x AABB_TOL_ULPS float32
    ulps of touching, so that the pair set is the same whichever way the boxes were rounded - other than the pairs of
    `touching`, whose boxes are exact."""
    sc, body_box = _body_boxes(name)
    b = sc["body"]
    b64 = pr.aabbs(b["pos"], b["rot"], b["shape"], b["he"], sc["margin"])
    s64 = sr.static_boxes64(sc["static"], sc["margin"])
    has = np.nonzero(b["shape"] != pr.SHAPE_NONE)[0]
    allp = np.stack(np.meshgrid(has, np.arange(len(s64)), indexing="ij"), axis=-1).reshape(-1, 2)
    gap, unit = sr.box_gaps64(b64, s64, allp)
    near = np.abs(gap) <= 2.0 * pr.AABB_TOL_ULPS * unit
    if name == "touching":
        exact = {(int(i), int(k)) for i, k in np.concatenate([sc["touch"], sc["apart"]])}
        assert {(int(i), int(k)) for i, k in allp[near]} == exact
        near[:] = False
    print(f"{name}: {int(near.sum())} ambiguous of {len(allp)} combinations; the nearest {np.abs(gap / unit).min():.1f} ulps")
    assert near.sum() == 0
    # and so the float64 pair set is the float32 one
    box, _ = static_set(name)
    assert np.array_equal(allp[gap <= 0], sr.static_pairs(body_box, box))


@pytest.mark.parametrize("name", NAMES)
def test_pairs_are_contacts_or_clear_misses(name, static_set):
    sc, body_box = _body_boxes(name)
    box, _ = static_set(name)
    pairs = sr.static_pairs(body_box, box)
    n = len(body_box)
    o = _oracle(sc, True)
    assert np.array_equal(o.get_aabbs()[:n], body_box)
    o.collide_now()
    every = spr.manifolds_of(o)
    man = {(a, sr.STATIC_ID_BIT | (b - n)): v for (a, b), v in every.items() if a < n <= b}
    at_body = np.bincount([i for key in every for i in key if i < n], minlength=n).max()
    assert at_body <= 64, "manifolds at one body, with statics and with bodies: the world's limit (its solve would be skipped)"
    # the body path of the GPU test holds the statics as bodies n + k: a scene is left out of it where one of those would pass
    # the same limit, and only there
    at_static = int(np.bincount([i - n for key in every for i in key if i >= n], minlength=len(box)).max())
    print(f"{name}: at most {at_static} manifolds at one static held as a body")
    assert (at_static > 64) == (name in BODY_PATH_LEFT_OUT)
    o.close()
    per_body = np.bincount([a for a, _ in man], minlength=n).max() if man else 0
    print(f"{name}: {len(man)} manifolds against statics, at most {per_body} at one body")
    assert per_body <= 64, "the limit of manifolds at one body"
    hits, misses, skipped = check_manifolds(name, sc, pairs, man)
    shares = hits >= spr.MIN_CONTACTS * len(pairs) and misses >= spr.MIN_MISSES * len(pairs)
    assert shares == sr.SCENE_TABLE[name][8], "the table says which scenes meet shape_pair_ref's floors"
