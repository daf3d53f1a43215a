"""CPU: tests/pair_ref.py checked against the O(n^2) definition, its boxes measured against the CPU oracle's (which are
the device's, bit for bit) to set the tolerance of the GPU test, and the scenes of tests/test_gpu_pairs_independent.py
checked against the cases they are named for - with the constants read out of plan.hpp, setup.hpp and broadphase.hip and
the bucket table taken from grid_plan itself (tests/cpp/grid_plan_cli.cpp), so that the GPU tests cannot pass by missing
their case, and a constant that moves takes the scenes with it."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pair_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physics_amd", "csrc")


def _constant(file, pattern):
    found = re.findall(pattern, open(os.path.join(CSRC, file)).read())
    assert len(found) == 1, (file, pattern, found)
    return found[0]


@functools.lru_cache(maxsize=None)
def _constants():
    reg = _constant("plan.hpp", r"constexpr int kRegX = (\d+), kRegY = (\d+), kRegZ = (\d+), kRegCells = kRegX \* kRegY \* kRegZ;")
    bits = int(_constant("setup.hpp", r"g\.sx = ab\[0\] - (\d+)u; g\.sy = ab\[1\] - \1u;"))  # brick bits per axis
    assert _constant("plan.hpp", r"const uint32_t n_bricks = in\.grid_table_size >> (\d+);") == str(3 * bits)
    return dict(slot_max=int(_constant("plan.hpp", r"constexpr uint32_t kSlotGridMaxBodies = (\d+);")),
                region=tuple(int(x) for x in reg), brick=(1 << bits,) * 3,
                stage=int(_constant("plan.hpp", r"h\.max_region \+ h\.max_region / 4 : (\d+)u;")),
                stage_per_wave=int(_constant("broadphase.hip", r"constexpr int kStagePerWave = (\d+);")),
                few_pairs=int(_constant("plan.hpp", r"\(uint64_t\)h\.n_pairs < (\d+)ull \* in\.n\)")))


@pytest.fixture(scope="module")
def grid_plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_plan")
    exe = str(d / "grid_plan_cli")
    # the flags of tests/test_setup_cpu.py's build of the same header
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "grid_plan_cli.cpp"), "-o", exe], check=True)

    def plan(sc):
        path = str(d / "bodies.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(sc["pos"])) + sc["pos"].tobytes() + sc["he"].tobytes())
        table, *axes = (int(x) for x in subprocess.check_output([exe, path, repr(pr.MARGIN)]).split())
        return table, tuple(axes)
    return plan


@functools.lru_cache(maxsize=None)
def _measured(name):
    """The scene, the oracle's boxes and pairs (sort-and-sweep driver; the grid driver is held to the reference here), and the
    reference's."""
    import physics_amd
    from oracle import binding as ob
    sc = pr.scene(name)
    o = ob.OracleWorld(physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_BROADPHASE_ONLY,
                                                  max_pairs=pr.MAX_PAIRS.get(name, 0)), trig=ob.TRIG_DET)
    o.set_bodies(sc["pos"], rot=sc["rot"], shape_type=sc["shape"], half_extent=sc["he"])
    box = o.get_aabbs()
    pairs = pr.pairs(box)
    assert np.array_equal(o.broadphase_grid(), pairs), "the reference and the oracle's grid driver (half shell of 14 cells) disagree"
    return sc, box, o.broadphase(), pr.aabbs(sc["pos"], sc["rot"], sc["shape"], sc["he"]), pairs


# ---- the reference itself ---------------------------------------------------------------------------------------------
def test_pairs_equal_the_definition_with_touching_boxes_and_bodies_without_a_shape():
    rng = np.random.default_rng(21)
    n = 2000
    lo = rng.integers(0, 24, (n, 3)).astype(np.float32) * np.float32(0.25)   # a lattice: faces meet exactly
    hi = lo + rng.integers(1, 6, (n, 3)).astype(np.float32) * np.float32(0.25)
    box = np.concatenate([lo, hi], axis=1)
    none = rng.permutation(n)[:150]
    box[none, :3], box[none, 3:] = 3.0e38, -3.0e38
    box[rng.permutation(n)[:5]] = np.nan
    want = pr.brute_pairs(box)
    got = pr.pairs(box)
    assert np.array_equal(got, want) and len(want) > 5000
    assert not np.isin(got, none).any()
    touching = (box[want[:, 0], :3] == box[want[:, 1], 3:]).any(axis=1) | (box[want[:, 1], :3] == box[want[:, 0], 3:]).any(axis=1)
    assert touching.sum() > 500, "pairs that meet in a face, an edge or a corner only"
    for chunk in (1, 1000):  # the candidate ranges are cut into pieces: any cut gives the same set
        assert np.array_equal(pr.pairs(box, chunk=chunk), want)
    for axis in range(3):    # whichever axis is swept
        stretched = box.copy()
        with np.errstate(over="ignore"):  # (the inverted boxes' 3e38 become infinities: still inverted)
            stretched[:, [axis, axis + 3]] *= np.float32(64.0)
        assert np.array_equal(pr.pairs(stretched), pr.brute_pairs(stretched))
    gap = np.array([[0, 0, 0, 1, 1, 1], [np.nextafter(np.float32(1), np.float32(2)), 0, 0, 2, 1, 1], [1, 1, 1, 2, 2, 2]], np.float32)
    assert pr.pairs(gap).tolist() == [[0, 2], [1, 2]], "one ulp apart is apart; a shared corner or edge is a pair"


def test_boxes_by_hand():
    s = np.sqrt(0.5)
    pos = np.array([[1, 2, 3]] * 5, np.float32)
    rot = np.array([[0, 0, 0, 1], [0, 0, s, s], [0, 0, 0, 1], [0, 0, s, s], [0, 0, 0, 2]], np.float64)  # 90 degrees about z; norm 2
    he = np.array([[0.5, 9, 9], [1, 2, 3], [0.25, 1, 9], [0.25, 1, 9], [1, 2, 3]], np.float32)
    shape = [pr.SHAPE_SPHERE, pr.SHAPE_BOX, pr.SHAPE_CAPSULE, pr.SHAPE_CAPSULE, pr.SHAPE_BOX]
    e = (pr.aabbs(pos, rot, shape, he, 0.02)[:, 3:] - pos) - 0.02
    assert np.allclose(e, [[0.5, 0.5, 0.5], [2, 1, 3], [0.25, 1.25, 0.25], [1.25, 0.25, 0.25], [4, 8, 12]], atol=1e-12)
    assert np.isnan(pr.aabbs(pos[:1], rot[:1], [pr.SHAPE_NONE], he[:1])).all()


# ---- the boxes: tolerance measured on the oracle ------------------------------------------------------------------------
def test_oracle_boxes_set_the_tolerance():
    worst = {}
    for name in pr.SCENES:
        sc, box, _, ref, _ = _measured(name)
        worst[name] = pr.box_errors(box, ref, sc["shape"])
        none = sc["shape"] == pr.SHAPE_NONE
        assert none.sum() > 1000 and (box[none, :3] > box[none, 3:]).all()
        for t in (pr.SHAPE_SPHERE, pr.SHAPE_BOX, pr.SHAPE_CAPSULE):
            assert (sc["shape"] == t).sum() > 9000
    print({k: (round(a, 3), round(b, 3)) for k, (a, b) in worst.items()})
    measured = max(a for a, _ in worst.values())
    assert 0.9 * pr.MEASURED_AABB_ULPS < measured <= pr.MEASURED_AABB_ULPS, measured
    assert pr.AABB_TOL_ULPS == 4.0 * pr.MEASURED_AABB_ULPS
    assert max(b for _, b in worst.values()) <= pr.AABB_TOL_ULPS, "containment, as the GPU test asks it"


def test_a_box_one_percent_too_small_is_seen():
    sc, box, _, ref, _ = _measured("few_pairs")
    centre, half = 0.5 * (ref[:, :3] + ref[:, 3:]), 0.5 * (ref[:, 3:] - ref[:, :3])
    small = np.concatenate([centre - 0.99 * half, centre + 0.99 * half], axis=1).astype(np.float32)
    worst, short = pr.box_errors(small, ref, sc["shape"])
    assert short > 100 * pr.AABB_TOL_ULPS


# ---- the scenes reach their cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.SCENES))
def test_scene_reaches_its_case(name, grid_plan):
    c = _constants()
    sc, box, oracle_pairs, ref, pairs = _measured(name)
    n = len(sc["pos"])
    assert n == pr.N == 33000 and c["slot_max"] == 32768 < n, "the smallest round size above the slot grid"
    assert np.array_equal(pairs, oracle_pairs), "the reference and the oracle's sort-and-sweep disagree"
    assert len(pairs) >= n // 2
    assert len(pairs) <= pr.MAX_PAIRS.get(name, 24 * n)
    table, axes = grid_plan(sc)
    assert table == 131072 and axes[0] * axes[1] * axes[2] == table
    # the grid of the reference's own boxes (rounded to float32 as the device holds them)
    ids, cell = pr.cells(ref.astype(np.float32), sc["shape"])
    own, region = pr.brick_regions(cell, axes, c["brick"], c["region"])
    staged, unstaged = int((region <= c["stage"]).sum()), int((region > c["stage"]).sum())
    span = cell.max(axis=0) - cell.min(axis=0) + 1
    print(f"{name}: {len(pairs)} pairs, {len(pairs) / n:.2f} per body; table {axes}, cells in use {span.tolist()}; "
          f"{len(own)} bricks in use, regions of {region.min()} - {region.max()} records: {staged} staged, {unstaged} not")
    assert pr.SCENE_TABLE[name] == (len(pairs), staged, unstaged)
    if name in ("sparse", "far", "farther"):
        assert (region < c["stage"]).all()
    if name == "dense":
        assert (region > c["stage"]).all()
        # pairs of two bodies of one brick are found by that brick's workgroup, whichever body finds them: a quarter of them
        # falls to one of its four waves at least. kStagePerWave (512) is the stage of the lanes-per-body kernels, whose waves
        # (64 or 16 bodies of ~15 found pairs each, walk after walk) fill it as well; the brick kernel's own stage is its
        # template parameter, 128 or 256: more than 512 hits overflow either
        brick = np.full(n, -1, np.int64)
        b = np.mod(cell, axes) // np.asarray(c["brick"])
        brick[ids] = (b[:, 2] * (axes[1] // c["brick"][1]) + b[:, 1]) * (axes[0] // c["brick"][0]) + b[:, 0]
        inside = brick[pairs[:, 0]] == brick[pairs[:, 1]]
        assert np.bincount(brick[pairs[inside, 0]]).max() // 4 > c["stage_per_wave"]
    if name == "clump":
        assert staged >= 4 and unstaged >= 4
    if name.startswith("thin"):
        long_axes = [a for a in range(3) if span[a] > axes[a]]
        assert long_axes == ([1] if name == "thin_tall" else [0, 2]), (span, axes)
        wrapped = np.unique(np.mod(cell, axes), axis=0)
        assert len(np.unique(cell, axis=0)) > len(wrapped) + 100, "cells in use that share a bucket"
    if name == "few_pairs":
        assert len(pairs) < c["few_pairs"] * n
    if name == "many_pairs":
        assert len(pairs) >= c["few_pairs"] * n
    if name == "farther":
        assert cell[:, 0].min() > 2 ** 15 and cell[:, 2].max() < -2 ** 15
        inv = np.float32(1.0) / pr.cell_size(ref.astype(np.float32), sc["shape"])
        assert np.spacing(np.float32(199000.0) * inv) > 0.001, "an ulp of centre x 1 / cell above the cell's 0.1 % slack"
    if name in ("far", "farther"):
        near = _measured("sparse")[0]
        assert np.array_equal(sc["shape"], near["shape"]) and np.array_equal(sc["he"], near["he"])
    if name == "far":
        assert cell[:, 0].min() > 2 ** 13 and cell[:, 2].max() < -2 ** 13 and np.abs(sc["pos"][:, [0, 2]]).min() > 59000
        # the cell is 0.1 % wider than the widest box; here the roundings of two products centre x 1 / cell, half an ulp each,
        # add up to that slack
        inv = np.float32(1.0) / pr.cell_size(ref.astype(np.float32), sc["shape"])
        assert np.spacing(np.float32(59000.0) * inv) > 0.0009


def test_either_side_of_the_slot_grid_are_the_same_soup():
    limit = _constants()["slot_max"]
    a, b = pr.scene("many_pairs", limit), pr.scene("many_pairs", limit + 1)
    assert len(a["pos"]) == limit and len(b["pos"]) == limit + 1
    for sc in (a, b):
        p = pr.pairs(pr.aabbs(sc["pos"], sc["rot"], sc["shape"], sc["he"]).astype(np.float32))
        assert len(p) >= len(sc["pos"]) // 2
