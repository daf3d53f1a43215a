"""GPU: ray casts, sphere casts and overlap queries at the edges of the query grid (physics_amd/csrc/rc_grid.hpp), against
the float64 brute forces of tests/raycast_ref.py and tests/query_ref.py over the scenes of tests/query_scenes.py.

What a compact soup near the origin never varies: the distance from the origin (pads of 0.9 and 3 at 6e4 and 2e5), 62 000
cells along one axis, one cell, a flat grid, no grid, lengths of 1e-3, a table of 8192 buckets against one of 4096, a
bucket of 2 900 records, overlap lists of 1 025..2 048 and of more than 2 048 ids (both sort paths of k_ov_order), the
overlap query's switch to its direct path from both sides, a grid grown into eight cells by one large radius, and the
filtered instances over two of these scenes; and, through PHYS_DEBUG_RAYCAST_STATS, that the device's grid is the one
tests/query_scenes.py grid_of restates. The acceptance is that of tests/query_accept.py, unchanged, with |o| measured
from the scene's centre; the query sets and their float64 answers are those of tests/query_cases.py, whose own ambiguous
cases tests/test_query_grid_cpu.py counts."""
import numpy as np
import pytest

import query_accept as qa
import query_cases as qc
import query_ref
import query_scenes as qs
import raycast_ref

pytestmark = pytest.mark.gpu


def _pa():
    import physics_amd
    return physics_amd


def _make(sc):
    pa = _pa()
    w = pa.World(pa.default_config(flags=pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0), ground_height=sc["ground"]))
    b = sc["bodies"]
    w.set_bodies(b["pos"], rot=b["rot"], shape_type=b["shape"], half_extent=b["half_extent"])
    s = sc["statics"]
    if s is not None:
        w.set_static_bodies(s["pos"], rot=s["rot"], shape_type=s["shape"], half_extent=s["half_extent"])
    pos, rot = w.get_transforms()
    assert np.array_equal(pos, b["pos"]) and np.array_equal(rot, b["rot"])  # the poses the references were given
    return w


@pytest.fixture(scope="module")
def world():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(qs.scene(name))
        return made[name]

    yield get
    for w in made.values():
        w.close()


# ---- 1. ray casts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qs.NAMES)
def test_rays_match_the_float64_reference(name, world):
    sc, w = qs.scene(name), world(name)
    for s in qc.ray_sets(name):
        body, t, _ = qa.compare(w, sc["bodies"], s["o"], s["d"], s["max_t"], s["ignore"], label=s["label"], h=s["h"])
        if s["label"] == "flung crossing":  # across 62 000 cells to a body of the other clump
            assert len(body) >= 16 and (body < 600).all() and (t > 2.9e6).all()
        if s["label"] == "flung short rays in the middle":
            assert (body == raycast_ref.MISS).sum() > len(body) // 2
    if name == "statics_only":
        assert (w.raycast(qc.ray_sets(name)[0]["o"], qc.ray_sets(name)[0]["d"])[0] < w.n).sum() == 0


def test_rays_that_miss_body_2048_give_the_same_bits_with_and_without_it(world):
    """2049 bodies take a table of 8192 buckets and two scan tiles, 2048 one of 4096 and one tile: other buckets, other
    record order, the same answers but for rays that meet the last body (or come within 1e-3 of it)."""
    near, less, sc = world("near"), world("near2048"), qs.scene("near")
    s = qc.ray_sets("near")[1]
    b = sc["bodies"]
    # the set's rays and 300 more aimed at and around the last body
    rng = np.random.default_rng(2048)
    aim = b["pos"][2048] + rng.normal(scale=0.5, size=(300, 3))
    o2 = (b["pos"][2048] + rng.normal(scale=12.0, size=(300, 3))).astype(np.float32)
    o = np.concatenate([s["o"], o2])
    d = np.concatenate([s["d"], (aim - o2).astype(np.float32)])
    mt = np.concatenate([s["max_t"], np.full(300, np.inf, np.float32)])
    ig = np.concatenate([np.where(s["ignore"] == 2048, 0xFFFFFFFF, s["ignore"]), np.full(300, 0xFFFFFFFF)]).astype(np.uint32)
    n = len(o)
    o64, u64, _ = raycast_ref._unit(o, d)
    fat = b["half_extent"][2048].astype(np.float64) * 1.001 + 1e-3
    t_last, _ = raycast_ref._intersect(o64, u64, np.tile(b["pos"][2048].astype(np.float64), (n, 1)),
                                       np.tile(raycast_ref.rotation_matrices(b["rot"][2048]), (n, 1, 1)), np.tile(fat, (n, 1)),
                                       np.full(n, b["shape"][2048]))
    clear = ~np.isfinite(t_last)
    assert 100 < (~clear).sum() < 350 and b["shape"][2048] != 0
    got, want = less.raycast(o, d, mt, ig), near.raycast(o, d, mt, ig)
    for x, y in zip(got, want):
        assert np.array_equal(x[clear].view(np.uint32), y[clear].view(np.uint32))
    assert (want[0][~clear] == 2048).sum() > 100 and (got[0] != 2048).all() and (want[0][clear] < 2048).sum() > 500


# ---- 2. sphere casts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["0", "0.25", "mixed", "huge"])
@pytest.mark.parametrize("name", qc.CAST_SCENES)
def test_spherecasts_match_the_float64_reference(name, kind, world):
    s, w = qc.cast_set(name, kind), world(name)
    body, t, nrm = qa.compare_casts(w, s["tg"], s["o"], s["d"], s["rad"], label=s["label"], h=s["h"])
    bad = ~(np.isfinite(s["rad"]) & (s["rad"] >= 0))
    if kind in ("mixed", "huge"):  # invalid radii miss, whatever the valid ones of the call grew the grid to
        assert bad.sum() >= 3 and (body[bad] == raycast_ref.MISS).all() and np.isinf(t[bad]).all() and not nrm[bad].any()
    if kind == "huge":
        g = qs.grid_of(qs.scene(name)["bodies"], grow=float(s["rad"][~bad].max()))
        assert int(np.prod(g["dims"])) <= 8
    assert ((body < w.n) & ~bad).sum() > (~bad).sum() // 4


# ---- 3. overlaps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qs.NAMES)
def test_overlaps_match_the_float64_reference(name, world):
    s, w = qc.overlap_set(name), world(name)
    off, ids = qa.compare_overlaps(w, s["tg"], *s["q"], label=s["label"], want=s["want"])
    if name != "statics_only":
        assert (ids < w.n).sum() > 50
    else:
        assert len(ids) > 50 and not (ids < w.n).any()


def _aabb_of_sphere(c, r):
    c = np.asarray(c, np.float32)
    return c - np.float32(r), c + np.float32(r)


@pytest.fixture(scope="module")
def long_lists():
    """`crowd`: ball queries around the cube of 3000 small bodies (against a ball the float64 reference is cheap for every
    target shape), with the ground, the platform and a static ball inside some of them; their float64 lists"""
    sc = qs.scene("crowd")
    S = qs.SPHERE
    q = [  # shape, centre, half extent: lists of 1025..2048 ids, then of more than 2048
        (S, [2.0, 1.5, 2.0], [2.5, 0, 0]), (S, [2.0, 3.0, 2.0], [2.05, 0, 0]), (S, [1.0, 3.5, 2.5], [1.9, 0, 0]),
        (S, [2.0, 3.0, 2.0], [9.0, 0, 0]), (S, [2.0, 6.0, 2.0], [5.5, 0, 0]), (S, [2.0, 1.0, 2.0], [4.0, 0, 0]),
    ]
    st = np.array([x[0] for x in q], np.uint32)
    pos = np.array([x[1] for x in q], np.float32)
    he = np.array([x[2] for x in q], np.float32)
    rot = qs._quats(np.random.default_rng(9), len(q))
    tg = qc.targets(sc)
    want = query_ref.overlap(st, pos, rot, he, tg, ground=sc["ground"])
    return dict(q=(st, pos, rot, he), want=want, tg=tg)


def test_long_overlap_lists_pass_through_both_sort_paths(long_lists, world):
    pa = _pa()
    w, sc = world("crowd"), qs.scene("crowd")
    st, pos, rot, he = long_lists["q"]
    want = long_lists["want"]
    lens = [len(e) for e, _ in want]
    print("list lengths", lens)
    assert all(1025 <= n <= 2048 for n in lens[:3]) and all(n > 2048 for n in lens[3:])
    g = qs.grid_of(sc["bodies"])
    for k in range(len(pos)):  # the grid path, not the direct one: few cells, thousands of records in one bucket
        reach = float(he[k, 0] + he[k, 1])
        assert qs.covered_cells(g, *_aabb_of_sphere(pos[k], reach)) <= g["n_bodies"]
    statics = {int(pa.STATIC_ID_BIT | k) for k in range(4)}
    for k in (0, 3, 5):  # the ground's and the statics' ids go through the sort with the bodies'
        assert pa.RAY_GROUND in want[k][0] and statics & set(want[k][0]), k
    assert pa.RAY_GROUND not in want[4][0]
    off, ids = qa.compare_overlaps(w, long_lists["tg"], st, pos, rot, he, label="crowd long lists", want=want)
    # one at a time (another block, the same list) and in the other order
    for k in (1, 4):
        o1, i1 = w.overlap(st[k:k + 1], pos[k:k + 1], rot[k:k + 1], he[k:k + 1])
        assert np.array_equal(i1, ids[off[k]:off[k + 1]])
    o2, i2 = w.overlap(st[::-1].copy(), pos[::-1].copy(), rot[::-1].copy(), he[::-1].copy())
    for k in range(len(pos)):
        j = len(pos) - 1 - k
        assert np.array_equal(i2[o2[j]:o2[j + 1]], ids[off[k]:off[k + 1]])


def test_capacity_and_retry_on_a_long_list(long_lists, world):
    from physics_amd import _abi
    w = world("crowd")
    st, pos, rot, he = (np.ascontiguousarray(x[3:5]) for x in long_lists["q"])
    off_full, ids_full = w.overlap(st, pos, rot, he, cap=1 << 20)
    assert off_full[-1] > 4096
    offs = np.zeros(3, np.uint64)
    small = np.full(2048, 0xDEADBEEF, np.uint32)
    rc = w.lib.phys_overlap(w.h, 2, st.ctypes.data_as(_abi.u32p), pos.ctypes.data_as(_abi.f32p), rot.ctypes.data_as(_abi.f32p),
                            he.ctypes.data_as(_abi.f32p), None, len(small), offs.ctypes.data_as(_abi.u64p),
                            small.ctypes.data_as(_abi.u32p))
    assert rc == _abi.PHYS_ERR_CAPACITY and np.array_equal(offs, off_full) and (small == 0xDEADBEEF).all()
    off2, ids2 = w.overlap(st, pos, rot, he, cap=2048)  # the retry with the reported total
    assert np.array_equal(off2, off_full) and np.array_equal(ids2, ids_full)


def test_overlap_boxes_on_both_sides_of_the_direct_path_switch(world):
    """k_ov_query walks the grid while the query covers at most n_bodies cells and tests every body directly above that:
    slabs over the whole of `near` in x and z, thick enough in y for 5 and for 6 of its 8 layers of cells (1805 and 2166
    cells against 2049 bodies), both around the last body."""
    sc, w = qs.scene("near"), world("near")
    b = sc["bodies"]
    g = qs.grid_of(b)
    n = g["n_bodies"]
    per_layer = int(g["dims"][0] * g["dims"][2])
    below, above = n // per_layer, n // per_layer + 1
    assert above <= g["dims"][1] and b["shape"][n - 1] != 0
    y_last = int(qs.coord(g, b["pos"][n - 1, 1], 1))
    lo, hi = qs.bounds(sc)
    boxes = []
    for layers in (below, above):
        first = min(max(y_last - layers // 2, 0), int(g["dims"][1]) - layers)
        y0 = float(g["lo"][1]) + (first + 0.25) * float(g["cell"])
        y1 = float(g["lo"][1]) + (first + layers - 0.25) * float(g["cell"])
        c = np.array([(lo[0] + hi[0]) / 2, (y0 + y1) / 2, (lo[2] + hi[2]) / 2], np.float32)
        h = np.array([(hi[0] - lo[0]) / 2 + 3.0, (y1 - y0) / 2, (hi[2] - lo[2]) / 2 + 3.0], np.float32)
        cells = qs.covered_cells(g, c - h, c + h)
        assert cells == layers * per_layer, (cells, layers, per_layer)
        boxes.append((c, h))
    assert below * per_layer <= n < above * per_layer
    pos = np.array([x[0] for x in boxes], np.float32)
    he = np.array([x[1] for x in boxes], np.float32)
    st = np.full(2, qs.BOX, np.uint32)
    tg = qc.targets(sc)
    want = query_ref.overlap(st, pos, None, he, tg, ground=sc["ground"])
    assert all(n - 1 in e for e, _ in want) and all(len(e) > 600 for e, _ in want)
    qa.compare_overlaps(w, tg, st, pos, None, he, label="near direct-path switch", want=want)


# ---- 4. the filtered instances -----------------------------------------------------------------------------------------------
GROUND_CATEGORY = 2
MASKS = (1, 2, 5, 6)


def _filtered(sc, cat, scat, mask):
    """the scene as a query of this mask sees it: targets of other categories lose their shape (and keep their ids)"""
    b = dict(sc["bodies"], shape=np.where((cat & mask) != 0, sc["bodies"]["shape"], 0).astype(np.uint32))
    s = dict(sc["statics"], shape=np.where((scat & mask) != 0, sc["statics"]["shape"], 0).astype(np.uint32))
    return b, s, (sc["ground"] if mask & GROUND_CATEGORY else None)


@pytest.mark.parametrize("name", ["farther", "crowd"])
def test_filtered_queries_match_the_filtered_reference(name):
    sc = qs.scene(name)
    w = _make(sc)
    rng = np.random.default_rng(41)
    nb = len(sc["bodies"]["pos"])
    cat = rng.choice([1, 2, 4], nb).astype(np.uint16)
    scat = np.array([1, 2, 4, 2], np.uint16)
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(GROUND_CATEGORY, 0xFFFF)
    rays = qc.ray_sets(name)[1]
    casts = qc.cast_set(name, "mixed")
    ov = qc.overlap_set(name)
    m_r = rng.choice(MASKS, len(rays["o"])).astype(np.uint16)
    m_c = rng.choice(MASKS, len(casts["o"])).astype(np.uint16)
    m_o = rng.choice(MASKS, 400).astype(np.uint16)
    oq = tuple(np.ascontiguousarray(x[:400]) for x in ov["q"])
    got_r = w.raycast(rays["o"], rays["d"], rays["max_t"], rays["ignore"], mask=m_r)
    got_c = w.spherecast(casts["o"], casts["d"], casts["rad"], mask=m_c)
    off, ids = w.overlap(*oq, mask=m_o)
    found = 0
    for mask in MASKS:
        b, s, ground = _filtered(sc, cat, scat, mask)
        tg = query_ref.targets(b, s)
        k = np.nonzero(m_r == mask)[0]
        qa.compare(w, b, rays["o"][k], rays["d"][k], rays["max_t"][k], rays["ignore"][k], ground=ground, statics=s,
                   centre=sc["centre"], out=tuple(x[k] for x in got_r), label=f"{name} rays mask {mask}")
        k = np.nonzero(m_c == mask)[0]
        qa.compare_casts(w, tg, casts["o"][k], casts["d"][k], casts["rad"][k], ground=ground, centre=casts["centre"],
                         out=tuple(x[k] for x in got_c), label=f"{name} casts mask {mask}")
        k = np.nonzero(m_o == mask)[0]
        sub_off = np.concatenate([[0], np.cumsum(off[k + 1] - off[k])]).astype(np.uint64)
        sub_ids = np.concatenate([ids[off[i]:off[i + 1]] for i in k] + [np.zeros(0, np.uint32)])
        qa.compare_overlaps(w, tg, *(x[k] for x in oq), ground=ground, centre=sc["centre"], out=(sub_off, sub_ids),
                            label=f"{name} overlaps mask {mask}")
        found += len(sub_ids)
        # what a mask rejects is never reported
        for body in (got_r[0][m_r == mask], got_c[0][m_c == mask], sub_ids):
            bodies = body[body < nb]
            assert ((cat[bodies] & mask) != 0).all()
            st = body[(body >= qa.raycast_ref.STATIC_ID_BIT) & (body < raycast_ref.MISS)] - raycast_ref.STATIC_ID_BIT
            assert ((scat[st] & mask) != 0).all()
            assert mask & GROUND_CATEGORY or not (body == raycast_ref.GROUND).any()
    assert found > 100
    w.close()


# ---- 5. the device's grid is grid_of's ---------------------------------------------------------------------------------------
_STATS_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import physics_amd as pa
import query_scenes as qs
for name in sys.argv[2:]:
    sc = qs.scene(name)
    b = sc["bodies"]
    w = pa.World(pa.default_config(flags=0, gravity_offset=(0.0, 0.0, 0.0)))
    w.set_bodies(b["pos"], rot=b["rot"], shape_type=b["shape"], half_extent=b["half_extent"])
    o, d = qs.sweep_rays(sc)
    body, t, _ = w.raycast(o, d)
    print("SWEEP", name, int((body != pa.RAY_MISS).sum()), flush=True)
    w.close()
"""


def test_rays_that_sweep_the_grid_visit_the_cells_grid_of_counts():
    """PHYS_DEBUG_RAYCAST_STATS (read once per process, so a child process) counts the cells the rays of a call visit. Rays
    along x above every body, from outside the grid, miss everything and visit each cell of their row once: nx per ray,
    with nx from grid_of. Another pad or cell edge on the device gives another count (`flung`: 62 379 cells; `farther`: 9,
    where the pad of 3 sets the cell)."""
    import os
    import subprocess
    import sys
    names = ["flung", "farther", "near", "tiny"]
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PHYS_DEBUG_RAYCAST_STATS="1")
    r = subprocess.run([sys.executable, "-c", _STATS_CHILD, here] + names, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    swept = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("SWEEP")]
    stats = [ln for ln in r.stderr.splitlines() if ln.startswith("PHYS_RAYCAST_STATS")]
    assert [s[1] for s in swept] == names and len(stats) == len(names), (r.stdout, r.stderr[-2000:])
    for name, s, ln in zip(names, swept, stats):
        sc = qs.scene(name)
        g = qs.grid_of(sc["bodies"])
        o, d = qs.sweep_rays(sc)
        h = raycast_ref.cast(o, d, sc["bodies"], centre=sc["centre"])
        assert (h["body"] == raycast_ref.MISS).all() and int(s[2]) == 0, (name, s)
        fields = dict(f.split("=") for f in ln.split()[1:])
        print(name, ln, "nx", int(g["dims"][0]))
        assert int(fields["rays"]) == len(o) and int(fields["cells"]) == len(o) * int(g["dims"][0]), (name, ln, g["dims"])
