"""CPU: tests/halo_ref.py checked against brute force, and the inputs of tests/test_gpu_halo_independent.py checked
against the conditions they must meet (enough cross pairs, pairs beyond an 8-cell sweep, a crowded bucket, the share of
bodies a pack selects), so that the GPU tests cannot pass by missing their case."""
import pathlib
import re

import numpy as np
import pytest

import halo_ref as hr


def _small_scene(kind):
    rng = np.random.default_rng({"uniform": 10, "mixed": 11, "giant": 12}[kind])
    sizes = (0.1, 0.6) if kind == "mixed" else (0.2, 0.3)
    ranks = []
    for r, (x0, x1) in enumerate(((-3.0, 0.0), (0.0, 3.0))):
        pos, shape, half = hr.small_bodies(rng, 600, x0, x1, none_every=17, side=6.0, sizes=sizes)
        if kind == "giant" and r == 1:
            pos[-1], shape[-1], half[-1] = (0.5, 3.0, 3.0), hr.SHAPE_BOX, 3.0
        ranks.append(hr.Rank(pos, shape, half, 2 * np.arange(600) + r, (-1.0e6, 0.0)[r], (0.0, 1.0e6)[r]))
    return ranks


@pytest.mark.parametrize("kind", ["uniform", "mixed", "giant"])
def test_local_and_cross_pairs_of_two_slabs_are_the_pairs_of_the_joined_scene(kind):
    ranks = _small_scene(kind)
    aabbs = [r.aabb for r in ranks]
    reach = hr.all_reduced_reach(*[(r.aabb, r.shape) for r in ranks])
    records, cross = hr.expected_exchange(ranks, aabbs, reach)
    got = set()
    for r, c in zip(ranks, cross):
        assert len(c) >= 20, "a rank that emits nothing checks nothing"
        for pairs in (r.gid[hr.brute_pairs(r.aabb, r.shape)], np.stack([r.gid[c[:, 0]], c[:, 1]], 1)):
            new = {(min(a, b), max(a, b)) for a, b in pairs.tolist()}
            assert len(new) == len(pairs) and not (new & got), "a pair twice"
            got |= new
    gid = np.concatenate([r.gid for r in ranks])
    joined = gid[hr.brute_pairs(np.concatenate(aabbs), np.concatenate([r.shape for r in ranks]))]
    assert got == {(min(a, b), max(a, b)) for a, b in joined.tolist()}
    if kind == "giant":  # the giant's record is wider than 8 of its neighbour's cells
        cell = hr.cell_size(ranks[0].aabb, ranks[0].shape)
        assert hr.cells_beyond_clamp(ranks[0].aabb, records[1], cross[0], cell).sum() >= 5


def test_touching_boxes_pair_and_a_gap_does_not():
    box = np.array([[-1, 0, 0, 0, 1, 1], [-3, 0, 0, -2, 1, 1]], np.float32)
    rec = np.zeros((2, 8), np.uint32)
    rec[0, :6] = np.array([0, 1, 1, 1, 2, 2], np.float32).view(np.uint32)          # touches body 0 in x, y and z
    rec[1, :6] = np.array([np.nextafter(np.float32(0), np.float32(1)), 0, 0, 1, 1, 1], np.float32).view(np.uint32)
    rec[:, 6] = (7, 9)
    shape = np.full(2, hr.SHAPE_BOX)
    assert hr.cross_pairs(box, [0, 2], shape, rec).tolist() == [[0, 7]]
    assert hr.cross_pairs(box, [8, 2], shape, rec).tolist() == []                   # the record's gid is the smaller one
    assert hr.cross_pairs(box, [0, 2], [hr.SHAPE_NONE, hr.SHAPE_BOX], rec).tolist() == []
    assert hr.cross_pairs(box, [0, 2], shape, rec, skip_first=0, skip_count=1).tolist() == []
    rec[0, 6] = hr.EMPTY
    assert hr.cross_pairs(box, [0, 2], shape, rec).tolist() == []


def test_body_records_round_trip_through_ghost_slots_and_the_filter_decoder():
    from physics_amd import filters
    b = hr.ghost_bodies()
    x_lo, x_hi, reach = hr.GHOST_SLAB
    flt = (b["category"], b["mask"], b["group"])
    recs = hr.body_records(b["pos"], b["rot"], b["lin"], b["ang"], b["inv_mass"], b["half"], b["shape"], b["gid"],
                           b["inv_inertia"], flt, x_lo, x_hi, reach)
    x = b["pos"][:, 0]
    sel = np.nonzero((b["shape"] != hr.SHAPE_NONE) & ((x < np.float32(-6)) | (x > np.float32(6))))[0]
    assert 0.25 * len(x) < len(sel) < 0.40 * len(x), "about a third of the bodies are boundary bodies"
    assert np.array_equal(recs[:, 17], b["gid"][sel])
    assert (x[sel] != -6).all() and (x[sel] != 6).all() and (x == -6).sum() > 100 and (x == 6).sum() > 100
    low = hr.body_records(b["pos"], b["rot"], b["lin"], b["ang"], b["inv_mass"], b["half"], b["shape"], b["gid"],
                          b["inv_inertia"], flt, x_lo, x_hi, reach, face=-1)
    high = hr.body_records(b["pos"], b["rot"], b["lin"], b["ang"], b["inv_mass"], b["half"], b["shape"], b["gid"],
                           b["inv_inertia"], flt, x_lo, x_hi, reach, face=+1)
    assert np.array_equal(low, recs[x[sel] < 0]) and np.array_equal(high, recs[x[sel] > 0]) and len(low) and len(high)
    # a receiver whose slab takes every record gets every field back
    g = hr.ghost_slots(hr.record_buffer(recs, len(recs) + 100), 0, 0, -100.0, 100.0, 1.0, len(recs))
    assert np.array_equal(g["index"], np.arange(len(recs)))
    for name, src in (("pos", "pos"), ("rot", "rot"), ("lin", "lin"), ("ang", "ang"), ("half_extent", "half"),
                      ("gid", "gid"), ("shape", "shape")):
        assert np.array_equal(g[name], b[src][sel]), name
    full = (b["inv_inertia"][sel][:, [1, 2, 3, 5, 6, 7]] != 0).any(axis=1)
    assert 100 < full.sum() < len(sel) // 4
    assert np.array_equal(g["inv_mass"], np.where(full, np.float32(0), b["inv_mass"][sel]))
    assert np.array_equal(g["mass"][~full], np.float32(1) / b["inv_mass"][sel][~full])
    assert np.isposinf(g["mass"][full]).all()
    assert np.array_equal(recs[:, 20:23].view(np.float32), b["inv_inertia"][sel][:, [0, 4, 8]])
    cat, mask, group, flag = filters.halo_decode(recs[:, 19], recs[:, 23])
    assert np.array_equal(cat, b["category"][sel]) and np.array_equal(mask, b["mask"][sel])
    assert np.array_equal(group, b["group"][sel]) and (group < 0).sum() > 100 and np.array_equal(flag, full)
    # the inertia tensors really invert exactly
    I, inv = b["inertia"].reshape(-1, 3, 3).astype(np.float64), b["inv_inertia"].reshape(-1, 3, 3).astype(np.float64)
    assert np.array_equal(I @ inv, np.broadcast_to(np.eye(3), I.shape))


def test_ghost_record_blocks_reach_the_edges_of_the_unpack():
    recs, skip_first, skip_count, n_live = hr.ghost_record_blocks()
    x_lo, x_hi, reach = hr.GHOST_SLAB
    assert len(recs) == 70000 > 65536 and (recs[:, 17] != hr.EMPTY).sum() == n_live
    g = hr.ghost_slots(recs, skip_first, skip_count, x_lo, x_hi, reach, 10 ** 6)
    idx = g["index"]
    assert ((idx < skip_first) | (idx >= skip_first + skip_count)).all() and (idx >= 65536 + 256).sum() > 500
    own = hr.ghost_slots(recs[skip_first:skip_first + skip_count], 0, 0, x_lo, x_hi, reach, 10 ** 6)
    assert len(own["index"]) > 1000, "the skipped block would have given ghosts"
    x = g["pos"][:, 0]
    assert (x == -10).sum() > 50 and (x == 10).sum() > 50 and x.min() == -10 and x.max() == 10
    allx = recs[recs[:, 17] != hr.EMPTY].view(np.float32)[:, 0]
    assert (allx == np.nextafter(np.float32(-10), np.float32(-100))).sum() > 50
    assert (allx == np.nextafter(np.float32(10), np.float32(100))).sum() > 50
    assert (g["inv_mass"] == 0).sum() > 1000 and np.isposinf(g["mass"][g["inv_mass"] == 0]).all()
    flagged = (recs[idx, 19] & 1) != 0
    assert flagged.sum() > 500 and (g["inv_mass"][flagged] == 0).all()
    assert len(idx) < 45000, "fits the ghost slots of the GPU test"
    # empty records between live ones: every block ends in an empty tail
    assert recs[skip_first - 1, 17] == hr.EMPTY and recs[skip_first + skip_count - 1, 17] == hr.EMPTY and recs[-1, 17] == hr.EMPTY


# ---- the inputs of the GPU pairs tests ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def neighbours():
    return {0: hr.neighbour_rank(0), hr.N_GIANTS: hr.neighbour_rank(hr.N_GIANTS)}


@pytest.mark.parametrize("kind", ["slots", "sorted"])
@pytest.mark.parametrize("giants", [0, hr.N_GIANTS])
def test_pairs_scenes_give_enough_cross_pairs_on_both_ranks(kind, giants, neighbours):
    ranks = [hr.local_rank(kind), neighbours[giants]]
    assert ranks[0].n == {"slots": 3000, "sorted": 33000}[kind] and (ranks[0].pos[:, 0] < 0).all() and (ranks[1].pos[:, 0] >= 0).all()
    aabbs = [r.aabb for r in ranks]
    reach = hr.all_reduced_reach(*[(r.aabb, r.shape) for r in ranks])
    records, cross = hr.expected_exchange(ranks, aabbs, reach)
    assert sum(len(c) for c in cross) >= 500 and all(len(c) >= 100 for c in cross), [len(c) for c in cross]
    cell = hr.cell_size(ranks[0].aabb, ranks[0].shape)
    beyond = hr.cells_beyond_clamp(ranks[0].aabb, records[1], cross[0], cell).sum()
    if giants:
        assert float(reach) > 6.0 and beyond >= 50, beyond
    else:
        assert beyond == 0 and 0.6 < float(reach) < 0.7


def test_local_ranks_lie_on_both_sides_of_the_slot_grid_threshold():
    """Nothing a world reports names the grid its broad phase built, so what ties the 'sorted' cases to
    k_halo_pairs<false> and the 'slots' cases to k_halo_pairs<true> is the plan's threshold itself: if it moves, this
    fails and the sizes move with it."""
    plan = (pathlib.Path(__file__).resolve().parents[1] / "physics_amd" / "csrc" / "plan.hpp").read_text()
    found = re.findall(r"constexpr uint32_t kSlotGridMaxBodies = (\d+);", plan)
    assert len(found) == 1 and "n <= kSlotGridMaxBodies" in plan
    limit = int(found[0])
    assert hr.N_SLOTS <= limit < hr.N_SORTED and hr.N_SORTED % 256 != 0
    assert hr.local_rank("slots").n == hr.N_SLOTS and hr.local_rank("sorted").n == hr.N_SORTED
    scenes = (hr.pack_rank(True), hr.pack_rank(False), *hr.overflow_scene()[:2], *hr.clump_scene())
    assert all(r.n <= limit for r in scenes), "these worlds are slot-grid worlds"


@pytest.mark.parametrize("reach", [0.5, 0.0])
def test_pack_scenes_select_between_a_tenth_and_six_tenths(reach):
    for r in (hr.pack_rank(True), hr.pack_rank(False)):
        assert (r.shape == hr.SHAPE_NONE).sum() > 100
        assert r.n > 256 and r.n % 64 != 0, "more than one workgroup, and a last wave that is not full"
        eff = reach if reach > 0 else hr.cell_size(r.aabb, r.shape)
        k = len(hr.pack_records(r.aabb, r.shape, r.gid, r.x_lo, r.x_hi, eff))
        assert 0.10 * r.n <= k <= 0.60 * r.n, (k, r.n)


def test_overflow_scene_crowds_one_bucket_and_every_crowded_body_pairs():
    local, neighbour, cluster = hr.overflow_scene()
    cell = hr.cell_size(local.aabb, local.shape)
    centre = np.float32(0.5) * (local.aabb[:, :3] + local.aabb[:, 3:])
    cells = np.floor(centre * (np.float32(1) / cell)).astype(int)
    assert (cells[cluster] == (-1, 3, 3)).all() and len(cluster) == 20 >= 9
    assert ((cells == (-1, 3, 3)).all(axis=1)).sum() == 20
    reach = hr.all_reduced_reach((local.aabb, local.shape), (neighbour.aabb, neighbour.shape))
    _, cross = hr.expected_exchange([local, neighbour], [local.aabb, neighbour.aabb], reach)
    assert set(cluster) <= set(cross[0][:, 0].tolist()) and len(cross[0]) >= 500


def test_clump_scene_overflows_the_cross_pair_room_of_64_bodies():
    local, neighbour = hr.clump_scene()
    reach = hr.all_reduced_reach((local.aabb, local.shape), (neighbour.aabb, neighbour.shape))
    records, cross = hr.expected_exchange([local, neighbour], [local.aabb, neighbour.aabb], reach)
    assert len(records[1]) == 200 and len(cross[0]) == 64 * 200 > max(4 * 64, 4096)
    assert len(hr.cross_pairs(local.aabb, local.gid, local.shape, records[1][:40])) == 64 * 40 <= 4096
