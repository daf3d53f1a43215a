"""CPU: the checker of the colouring stage (tests/color_ref.py) on a colouring made sequentially here, with one planted
defect at a time; the conditions of the scene generators (tests/color_cases.py) that need no device, from float64
positions; the CPU oracle - which compiles the colouring rule from the headers the kernels use and shows per-manifold
colours - held to the same checker on the smaller scenes; and the probe library's host side (the plan of the case
table's hints, the counters' layout), which loads without a GPU."""
import numpy as np
import pytest

import color_cases as cc
import color_probe as cp
import color_ref as cf
import contact_ref as cr


# ---------------------------------------------------------------- a colouring made one manifold at a time
def sequential_coloring(a, b, n_bodies, kept=None):
    """Jones-Plassmann rounds with plain loops: in a round, a manifold colours if no uncoloured manifold at either of its
    bodies has a higher priority; it takes the lowest colour free at both bodies (as they stood before the round)."""
    M = len(a)
    prio = [int(p) for p in cr.color_priority(a, b)]
    color = [-1] * M if kept is None else [int(c) for c in kept]
    at = [[] for _ in range(n_bodies)]
    for m in range(M):
        at[a[m]].append(m)
        if cr.is_body(b[m]):
            at[b[m]].append(m)
    rounds, n_new = 0, sum(c < 0 for c in color)
    while any(c < 0 for c in color):
        wins = []
        for m in range(M):
            if color[m] >= 0:
                continue
            bodies = [a[m]] + ([b[m]] if cr.is_body(b[m]) else [])
            if all(prio[m] >= prio[o] for body in bodies for o in at[body] if color[o] < 0):
                taken = {color[o] for body in bodies for o in at[body] if color[o] >= 0}
                wins.append((m, min(c for c in range(64) if c not in taken)))
        for m, c in wins:
            color[m] = c
        rounds += 1
    return np.array(color, np.int64), rounds, n_new


def random_graph(seed=5, n_bodies=60, M=240):
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < M:
        i, j = sorted(rng.integers(0, n_bodies, 2).tolist())
        kind = rng.integers(0, 8)
        if kind == 0:
            pairs.add((i, cc.GROUND))
        elif kind == 1:
            pairs.add((i, cc.STATIC_ID_BIT | int(rng.integers(0, 3))))
        elif i != j:
            pairs.add((i, j))
    p = np.array(sorted(pairs), np.int64)
    p = p[rng.permutation(len(p))]
    return p[:, 0], p[:, 1], n_bodies


@pytest.fixture(scope="module")
def two_updates():
    """(first read-out, prev for the second, second read-out): the second update keeps two thirds of the first's manifolds."""
    a, b, n = random_graph()
    col, rounds, n_new = sequential_coloring(a, b, n)
    first = cf.readout(a, b, col, n, rounds, n_new)
    prev = cf.sort_by_key(a, b, col)
    keep = np.arange(len(a)) % 3 != 0
    a2, b2, _ = random_graph(seed=6, M=120)
    fresh = ~np.isin(cr.pair_keys(a2, b2), cr.pair_keys(a, b))
    a3, b3 = np.concatenate([a[keep], a2[fresh]]), np.concatenate([b[keep], b2[fresh]])
    kept = np.concatenate([col[keep], np.full(fresh.sum(), -1)])
    col3, rounds3, new3 = sequential_coloring(a3, b3, n, kept)
    return first, prev, cf.readout(a3, b3, col3, n, rounds3, new3)


def test_checker_accepts_the_sequential_colouring(two_updates):
    first, prev, second = two_updates
    assert first.color_rounds >= 3 and second.color_rounds >= 3 and 0 < second.n_new_manifolds < second.M
    got_prev, ref = cf.check_update(first)
    assert np.array_equal(got_prev[0], prev[0]) and np.array_equal(got_prev[1], prev[1])
    cf.check_update(second, prev)


def _copy(out):
    from types import SimpleNamespace
    return SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(out).items()})


def _same_colour_at_one_body(out, prev):
    # give a NEW manifold the colour of another one at its body A
    a, col = out.man_a, out.man_color
    for m in np.flatnonzero(~np.isin(cr.pair_keys(out.man_a, out.man_b), prev[0])):
        others = np.flatnonzero((a == a[m]) & (col != col[m]))
        if len(others):
            col[m] = col[others[0]]
            return "hold two manifolds"
    raise AssertionError("no body with two manifolds")


def _kept_colour_changed(out, prev):
    keys = cr.pair_keys(out.man_a, out.man_b)
    m = np.flatnonzero(np.isin(keys, prev[0]))[0]
    free = [c for c in range(64) if not (int(out.used[out.man_a[m]]) >> c) & 1 and
            not (cr.is_body(out.man_b[m]) and (int(out.used[out.man_b[m] if cr.is_body(out.man_b[m]) else 0]) >> c) & 1)]
    out.man_color[m] = free[0]  # a colour no neighbour has: independent, but not the colour it had
    return "changed colour"


def _row_repeated(out, prev):
    out.row_src[3] = out.row_src[4]
    return "no permutation"


def _row_in_wrong_segment(out, prev):
    r = int(out.color_start[1])  # the first row of colour 1 changes places with the first of colour 0
    out.row_src[0], out.row_src[r] = out.row_src[r], out.row_src[0]
    return "segment of another colour"


def _last_start_short(out, prev):
    out.color_start[64] += 1  # (thread 1023 adding a carry twice, say; the array still ascends)
    return r"color_start\[64\]"


def _valid_but_not_the_reference(out, prev):
    # a new manifold moved to a colour that is free at both bodies, rows and counters made consistent with it
    keys = cr.pair_keys(out.man_a, out.man_b)
    for m in np.flatnonzero(~np.isin(keys, prev[0])):
        b_body = cr.is_body(out.man_b[m])
        mask = int(out.used[out.man_a[m]]) | (int(out.used[out.man_b[m]]) if b_body else 0)
        free = [c for c in range(int(out.man_color[m]) + 1, 64) if not (mask >> c) & 1]
        if free:
            col = out.man_color.copy()
            col[m] = free[0]
            new = cf.readout(out.man_a, out.man_b, col, out.n_bodies, out.color_rounds, out.n_new_manifolds)
            vars(out).update(vars(new))
            cf.check_independent(out.man_a, out.man_b, out.man_color)  # the planted colouring IS a valid one
            cf.check_row_src(out)
            return "another colour than the reference"
    raise AssertionError("no new manifold to move")


def _losers_dropped_from_the_list(out, prev):
    # what a round list that loses ids leaves behind (k_color_small's re-listing without thread 0's manifolds, k_color_round's
    # overflow branch without its direct append): those manifolds never colour, the counting sort passes them over
    lost = np.flatnonzero(~np.isin(cr.pair_keys(out.man_a, out.man_b), prev[0]))[::7]
    col = out.man_color.copy()
    col[lost] = cf.UNCOLORED
    new = cf.readout(out.man_a, out.man_b, col, out.n_bodies, out.color_rounds, out.n_new_manifolds)
    new.row_src = new.row_src[:out.M - len(lost)]  # the rows the sort wrote
    new.n_uncolored = len(lost)
    new.used = out.used
    vars(out).update(vars(new))
    return "n_uncolored"


def _last_start_from_the_last_wave_alone(out, prev):
    # k_color_offsets with 16 workgroups: wave 15 scans the entries of colours 60 to 63; its total alone, without the carry
    out.color_start[64] = out.color_count[60:].sum()
    return "color_start"


DEFECTS = [_losers_dropped_from_the_list, _last_start_from_the_last_wave_alone, _same_colour_at_one_body, _kept_colour_changed, _row_repeated, _row_in_wrong_segment, _last_start_short,
           _valid_but_not_the_reference]


@pytest.mark.parametrize("plant", DEFECTS, ids=[f.__name__.strip("_") for f in DEFECTS])
def test_checker_rejects_a_planted_defect(two_updates, plant):
    first, prev, second = two_updates
    out = _copy(second)
    message = plant(out, prev)
    with pytest.raises(cf.CheckFailed, match=message):
        cf.check_update(out, prev)


def test_cluster_layout_checker():
    """check_cluster_rows on a hand-made (owner cluster, colour) layout, and with a row moved to another cluster's segment."""
    first = cf.readout(*random_graph()[:2], sequential_coloring(*random_graph())[0], 60, 0, 0)
    clusters, slots = 4, 16
    first.cluster_slot = np.arange(60, dtype=np.uint32)  # body i lives in cluster i // 16
    first.cluster_slot[50:] = cf.NO_HOME
    first.cluster_slots, first.cluster_count = slots, clusters
    owner = cf.row_owner(first.man_a, first.man_b, first.cluster_slot, slots, clusters)
    assert set(owner) == {0, 1, 2, 3} and np.all(owner[first.man_a < 48] == first.man_a[first.man_a < 48] // 16)
    cell = owner * 64 + first.man_color.astype(np.int64)
    first.row_src = np.argsort(cell, kind="stable").astype(np.uint32)
    first.seg_start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=clusters * 64))]).astype(np.uint32)
    cf.check_cluster_rows(first)
    bad = _copy(first)
    bad.row_src[0], bad.row_src[-1] = bad.row_src[-1], bad.row_src[0]
    with pytest.raises(cf.CheckFailed, match="outside the"):
        cf.check_cluster_rows(bad)


def test_round_sizes_agree_with_the_sequential_rounds(two_updates):
    first, prev, second = two_updates
    sizes = cf.round_sizes(second.man_a, second.man_b, second.n_bodies, prev)
    assert len(sizes) == second.color_rounds and sizes[0] == second.n_new_manifolds and all(x > y for x, y in zip(sizes, sizes[1:]))


# ---------------------------------------------------------------- the scenes' own conditions
def _new_per_update(sc, updates, statics=None):
    """{update: (manifolds, manifolds not there the update before)} from float64 positions."""
    out, prev = {}, None
    for u in range(max(updates) + 1):
        keys = cc.contacts(sc, u, statics)
        out[u] = (len(keys), len(keys) if prev is None else int((~np.isin(keys, prev)).sum()))
        prev = keys
    return out


@pytest.mark.parametrize("M", [1, 1023, 1024, 1025] + list(cc.SMALL_FULL_SIZES))
def test_exact_scenes_have_exactly_their_manifolds(M):
    sc = cc.small_full(M) if M in cc.SMALL_FULL_SIZES else cc.exact(M)
    assert len(cc.contacts(sc, 0)) == M == len(cc.contacts(sc, 3, "far" if M in cc.SMALL_FULL_SIZES else None))


@pytest.mark.parametrize("name", ["probe_20k", "small_incremental", "beyond_registers", "known_incremental", "known_full",
                                  "cluster_scene"])
def test_movers_arrive_when_they_should(name):
    """Manifolds of the first update, and the new ones of every update a group arrives in (none in the updates between)."""
    sc = getattr(cc, name)()
    arrivals = getattr(sc, "arrivals", {})
    seen = _new_per_update(sc, list(arrivals) + [1])
    assert seen[0][0] == sc.expect_M
    for u in range(1, max(seen) + 1):
        assert seen[u][1] == arrivals.get(u, 0), (u, seen[u])
    total = sc.expect_M + sum(arrivals.values())
    assert seen[max(seen)][0] == total
    if name in ("small_incremental",):
        assert total <= 40960
    if name == "beyond_registers":
        assert sc.expect_M <= 40960 and 50_000 <= total <= 60_000
    if name in ("known_incremental", "known_full", "cluster_scene"):
        assert sc.expect_M > 40960


def test_lattice_degrees_and_margin_band():
    sc = cc.Scene(ground=True)
    ids = sc.lattice(6, 4, 5)
    keys = cc.contacts(sc, 0)
    a, b = cc.split_keys(keys)
    deg = np.bincount(np.concatenate([a, b[b < sc.n]]), minlength=sc.n)
    assert deg[ids[2, 2, 2]] == 6 and deg[ids[0, 3, 0]] == 3 and deg[ids[0, 0, 0]] == 3 + 1  # (a corner on the ground: + 1)
    assert len(keys) == cc.lattice_edges(6, 4, 5, ground=True) and (b == cc.GROUND).sum() == 30


def test_static_slab_touches_one_face():
    sc = cc.known_full()
    keys = cc.contacts(sc, 0, "slab")
    a, b = cc.split_keys(keys)
    assert (b == cc.STATIC_ID_BIT).sum() == sc.slab_manifolds and len(keys) == sc.expect_M + sc.slab_manifolds
    assert len(cc.contacts(sc, 0, "far")) == sc.expect_M


@pytest.mark.parametrize("partners", [64, 65])
def test_hub_partner_count(partners):
    sc = cc.hub_scene(partners)
    a, b = cc.split_keys(cc.contacts(sc, 0))
    assert ((a == sc.hub_id[0]) | (b == sc.hub_id[0])).sum() == partners and len(a) == sc.expect_M
    colors, n_colors, _, _ = cr.color_manifolds(a, b, sc.n)
    assert n_colors == 64


def test_stage_overflow_scene_outnumbers_the_stages():
    """The implosion's edges all arrive in update 4; with round launches sized for the base, the losers of round 0 cannot fit
    the workgroups' stages (pigeonhole over round_blocks x 8192), with 10 % to spare for the device's own (a, b) order."""
    sc = cc.stage_overflow()
    seen = _new_per_update(sc, [4])
    assert [seen[u][1] for u in (1, 2, 3, 4)] == [0, 400, 0, sc.arrivals[4]] and sc.arrivals[4] >= 10 * seen[3][0]
    plan = cp.plan_of(n_owned=sc.n, max_manifolds=17 * sc.n, ctab_valid=True, color_epoch=4, hint_valid=True,
                      hint_n_manifolds=seen[3][0], hint_color_rounds=5)
    assert plan.path == "Known" and plan.round_blocks == (seen[3][0] * 5 // 4 + 1024) // 1024
    a, b = cc.split_keys(cc.contacts(sc, 4))
    prev = cf.sort_by_key(*cc.split_keys(cc.contacts(sc, 3)), np.zeros(seen[3][0], np.int64))
    sizes = cf.round_sizes(a, b, sc.n, prev)
    assert sizes[0] == sc.arrivals[4] and sizes[1] > 1.1 * plan.round_blocks * 8192


# ---------------------------------------------------------------- the oracle, held to the same checker
def _oracle_world(sc):
    import physics_amd
    from oracle import binding as ob
    flags = physics_amd.FLAG_COLLISIONS | (physics_amd.FLAG_GROUND_PLANE if sc.ground else 0)
    o = ob.OracleWorld(physics_amd.default_config(flags=flags, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0)), trig=ob.TRIG_DET)
    o.set_bodies(**sc.bodies())
    return o


@pytest.mark.parametrize("name", ["exact_1025", "hub_64", "small_incremental"])
def test_oracle_colours_pass_the_checker(oracle_lib, name):
    """Per update: the oracle's manifolds are the ones the generator predicts, and its colours, counts, n_colors,
    color_rounds and n_new_manifolds pass check_colors / check_counts (it has no row_src and no `used` to show)."""
    sc = {"exact_1025": lambda: cc.exact(1025), "hub_64": lambda: cc.hub_scene(64), "small_incremental": cc.small_incremental}[name]()
    o = _oracle_world(sc)
    prev = None
    for u in range(6 if name == "small_incremental" else 2):
        o.update(cc.DT_NANOS)
        ids = o.get_manifolds()[0]
        st = o.get_stats()
        out = cf.readout(ids[:, 0], ids[:, 1], o.get_colors(), sc.n, st.color_rounds, st.n_new_manifolds, row_src=False)
        out.overflow = st.overflow
        assert np.array_equal(cc.unordered_keys(ids[:, 0], ids[:, 1]), cc.contacts(sc, u)), u
        ref = cf.check_colors(out, prev)
        cf.check_counts(out, ref[0])
        assert st.n_colors == ref[1]
        prev = cf.sort_by_key(ids[:, 0], ids[:, 1], ref[0])
        if name == "small_incremental":
            assert st.n_new_manifolds == ({0: sc.expect_M} | sc.arrivals).get(u, 0), u


# ---------------------------------------------------------------- the probe library's host side
def test_probe_library_loads_without_a_gpu():
    lay = cp.layout()
    assert lay.size % 4 == 0 and lay.n_manifolds == 0 and lay.unc_count == 4
    assert lay.color_start == lay.color_count + 64 * 4 and lay.color_start + 65 * 4 <= lay.size


def test_plan_of_the_case_table():
    """What plan.hpp makes of the hints the cases steer to. sort_blocks 1 and 2 come with the Small path only, whose kernel
    sorts by itself: the hist / offsets / place kernels never run with fewer than 16 workgroups."""
    base = dict(n_owned=50_000, max_manifolds=850_000)
    p = cp.plan_of(**base)
    assert (p.path, p.sort_blocks, p.full, p.rebuild, p.round_blocks) == ("Probe", 512, True, True, 512)
    for hint, blocks in ((3000, 1), (6000, 2), (40960, 16)):
        p = cp.plan_of(**base, ctab_valid=True, color_epoch=3, hint_valid=True, hint_n_manifolds=hint, hint_color_rounds=4)
        assert (p.path, p.sort_blocks, p.full, p.rebuild) == ("Small", blocks, False, False)
    least = min(h for h in range(40961, 40961 + 8) if cp.plan_of(**base, ctab_valid=True, color_epoch=3, hint_valid=True,
                                                                 hint_n_manifolds=h).path != "Small")
    p = cp.plan_of(**base, ctab_valid=True, color_epoch=3, hint_valid=True, hint_n_manifolds=least, hint_color_rounds=4)
    assert (least, p.path, p.rounds, p.sort_blocks, p.round_blocks) == (40961, "Known", 4, 16, 51)
    # a full re-colouring with the hint intact: Small stays Small; Known takes hint.full_rounds, Probe without one
    p = cp.plan_of(**base, ctab_valid=False, color_epoch=3, hint_valid=True, hint_n_manifolds=30_000, hint_full_rounds=20)
    assert (p.path, p.full, p.rebuild) == ("Small", True, True)
    p = cp.plan_of(**base, ctab_valid=False, color_epoch=3, hint_valid=True, hint_n_manifolds=45_000, hint_color_rounds=4, hint_full_rounds=20)
    assert (p.path, p.full, p.rounds) == ("Known", True, 20)
    p = cp.plan_of(**base, ctab_valid=False, color_epoch=3, hint_valid=True, hint_n_manifolds=45_000, hint_color_rounds=4)
    assert (p.path, p.full) == ("Probe", True)
    # the table rebuild: every 64th update
    for epoch in (63, 64, 65, 128):
        p = cp.plan_of(**base, ctab_valid=True, color_epoch=epoch, hint_valid=True, hint_n_manifolds=45_000)
        assert p.rebuild == (epoch % 64 == 0) and not p.full and p.stamp == epoch + 1
    # sort_blocks of the updates the GPU cases run: 16 at 44k, 256 behind the stage overflow
    assert cp.plan_of(**base, ctab_valid=True, hint_valid=True, color_epoch=1, hint_n_manifolds=590_000).sort_blocks == 256
