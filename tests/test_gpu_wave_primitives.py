"""GPU: every primitive of physics_amd/csrc/wave.hpp and the exclusive scan of scan.hip, called directly through the probe
library (tests/cpp/wave_probe.hip) at the sizes where they change path, against the numpy reference of tests/wave_ref.py.
Integers and exact maxima: everything is compared for equality. No physics update runs here."""
import functools

import numpy as np
import pytest

import wave_probe
import wave_ref as wr

pytestmark = pytest.mark.gpu

U32 = np.uint32


@pytest.fixture(scope="module")
def world(hip_world_factory):
    w = hip_world_factory()
    yield w
    w.close()


# ---- launch_exclusive_scan ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan_case(count, kind):
    """(table, expected out[count + 1]), computed once and read-only."""
    v = wr.scan_values(count, kind)
    ref = wr.exclusive_scan(v)
    v.setflags(write=False)
    ref.setflags(write=False)
    return v, ref


def _run_scan(world, v, zero_in, with_used):
    count = v.size
    words = wave_probe.scan_scratch_words(count)
    in_buf = np.concatenate([v, np.full(wr.SCAN_PAD, 0xFFFFFFFF, U32)])
    out = np.full(count + 1 + wr.SCAN_GUARD, wr.POISON, U32)
    scratch = np.full(words + wr.SCAN_GUARD, wr.POISON, U32)
    used = np.full(words + wr.SCAN_GUARD, wr.POISON, U32) if with_used else None
    ctr = np.full(wave_probe.counters_layout()[0], 0xA5, np.uint8) if with_used else None
    wave_probe.exclusive_scan(world, in_buf, count, out, zero_in, scratch, used, ctr)
    return in_buf, out, scratch, used, ctr, words


@pytest.mark.parametrize("kind", wr.SCAN_KINDS)
@pytest.mark.parametrize("count", wr.SCAN_COUNTS)
def test_exclusive_scan(world, count, kind):
    v, ref = _scan_case(count, kind)
    in_buf, out, scratch, used, ctr, words = _run_scan(world, v, zero_in=False, with_used=True)
    one_launch = wave_probe.scan_is_one_launch(count)
    assert one_launch == (count <= wr.SCAN_ONE_LAUNCH_LIMIT)
    assert np.array_equal(out[:count], ref[:count]), "exclusive prefix sums"
    assert out[count] == ref[count], "grand total in out[count]"
    assert np.all(out[count + 1:] == wr.POISON), "guard behind out[count]"
    assert np.all(scratch[words:] == wr.POISON) and np.all(used[words:] == wr.POISON), "guard behind the scratch words"
    # nothing behind `count` was read into a sum (the padding is all ones), and the table itself stays
    assert np.array_equal(in_buf[:count], v) and np.all(in_buf[count:] == 0xFFFFFFFF)
    size, off = wave_probe.counters_layout()
    others = np.ones(size, bool)
    others[off:off + 4] = False
    assert np.all(ctr[others] == 0xA5), "the other step counters"
    if one_launch:  # block_used / ctr are honoured by the three-launch scan only, and it needs no scratch
        assert np.all(ctr == 0xA5) and np.all(scratch == wr.POISON) and np.all(used == wr.POISON)
    else:
        assert int(ctr[off:off + 4].view(U32)[0]) == np.count_nonzero(v), "n_used_buckets"


@pytest.mark.parametrize("zero_in", (True, False))
@pytest.mark.parametrize("count", (4, 2052, 32768, 32772, 2097156))
def test_exclusive_scan_zero_in(world, count, zero_in):
    """zero_in is honoured by the one-launch scan alone; and the three-launch scan without block_used / counters."""
    v, ref = _scan_case(count, "random")
    in_buf, out, scratch, _, _, words = _run_scan(world, v, zero_in=zero_in, with_used=False)
    assert np.array_equal(out[:count + 1], ref) and np.all(out[count + 1:] == wr.POISON)
    assert np.all(scratch[words:] == wr.POISON)
    assert np.all(in_buf[count:] == 0xFFFFFFFF)
    if zero_in and wave_probe.scan_is_one_launch(count):
        assert not in_buf[:count].any(), "the counters are left zeroed"
    else:
        assert np.array_equal(in_buf[:count], v), "the counters stay"


# ---- block_scan_in_place --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads,count", [(t, c) for t in (256, 1024) for c in wr.block_scan_counts(t)])
def test_block_scan_in_place(threads, count):
    p = wr.block_scan_values(threads, count)
    want, total = wr.block_scan_in_place(p, count)
    totals = wave_probe.block_scan(threads, p, count)
    assert np.array_equal(p, want), "the scan in place (the guard behind it included)"
    assert np.all(totals == total), "the total in every lane"


# ---- one wave ---------------------------------------------------------------------------------------------------------------
def _lanes_agree(got):
    g = got.reshape(-1, wr.WAVE)
    return bool(np.all(g == g[:, :1]))


@pytest.mark.parametrize("threads,blocks", wr.WAVE_GEOMETRIES)
def test_wave_scan_sum_max(threads, blocks):
    n = threads * blocks
    for kind in ("u32", "small"):
        v = wr.wave_values(kind, n)
        assert np.array_equal(wave_probe.wave_op("scan", threads, blocks, v), wr.wave_inclusive_scan(v)), kind
        s = wave_probe.wave_op("sum", threads, blocks, v)
        assert _lanes_agree(s) and np.array_equal(s, wr.wave_sum(v)), kind
        m = wave_probe.wave_op("max_u32", threads, blocks, v)
        assert _lanes_agree(m) and np.array_equal(m, wr.wave_max(v)), kind
    i = wr.wave_values("int", n)
    m = wave_probe.wave_op("max_int", threads, blocks, i)
    assert m.dtype == np.int32 and _lanes_agree(m) and np.array_equal(m, wr.wave_max(i))
    f = wr.wave_values("float", n)
    m = wave_probe.wave_op("max_float", threads, blocks, f)
    assert _lanes_agree(m) and np.array_equal(m, wr.wave_max(f))


def test_wave_max_float_with_nan_lanes():
    """The contract wave.hpp states for op_max: a NaN lane keeps its NaN, every other lane ends with a non-NaN value of its
    wave that is no smaller than its own. (Without NaN: the maximum in every lane, test_wave_scan_sum_max.)"""
    threads, blocks = 256, 3
    v = wr.nan_values(threads * blocks)
    got = wave_probe.wave_op("max_float", threads, blocks, v)
    assert wr.wave_max_nan_contract_holds(v, got)


@pytest.mark.parametrize("threads,blocks", wr.WAVE_GEOMETRIES)
def test_lane_rank(threads, blocks):
    masks = wr.lane_rank_masks(threads * blocks // wr.WAVE)
    got = wave_probe.lane_rank(threads, blocks, masks).reshape(-1, wr.WAVE)
    for k, mask in enumerate(masks):
        assert np.array_equal(got[k], wr.lane_rank(mask)), hex(int(mask))


# ---- one workgroup ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads,blocks", wr.BLOCK_GEOMETRIES)
def test_block_sum_put_get(threads, blocks):
    n = threads * blocks
    for kind in ("u32", "small"):
        v = wr.wave_values(kind, n)
        for op in ("block_sum", "put_get_sum"):
            assert np.array_equal(wave_probe.block_reduce(op, threads, blocks, v), wr.block_reduce(v, threads, "sum")), (op, kind)
        assert np.array_equal(wave_probe.block_reduce("put_get_max_u32", threads, blocks, v), wr.block_reduce(v, threads, "max")), kind
    f = np.abs(wr.wave_values("float", n))  # block_get folds from T(0): maxima of values that are never negative
    assert np.array_equal(wave_probe.block_reduce("put_get_max_float", threads, blocks, f), wr.block_reduce(f, threads, "max"))


def test_wave_append_base():
    flags = wr.append_flags()
    base, slot, end = wave_probe.append(wr.APPEND_BLOCKS, flags, 0)
    total = int(np.count_nonzero(flags))
    assert end == total, "the counter"
    assert np.array_equal(np.sort(slot[flags != 0]), np.arange(total, dtype=U32)), "a permutation of [0, total)"
    for f, b, s in zip(flags.reshape(-1, wr.WAVE), base.reshape(-1, wr.WAVE), slot.reshape(-1, wr.WAVE)):
        assert np.all(b == b[0]), "the base in every lane"
        assert np.array_equal(s[f != 0], b[0] + np.arange(np.count_nonzero(f), dtype=U32)), "consecutive in lane order"


@pytest.mark.parametrize("start", wr.RESERVE_STARTS)
@pytest.mark.parametrize("by_count", (False, True), ids=("flag", "count"))
def test_slots_reserve(by_count, start):
    counts = wr.reserve_counts(by_count)
    slots, end = wave_probe.reserve(by_count, counts, start)
    off, totals = wr.reserve_offsets(counts)
    total = int(totals.sum())
    assert end == start + total, "the cursor"
    bases = []
    for b in range(counts.shape[0]):
        for t in range(counts.shape[1]):
            has = counts[b, t] != 0
            if not has.any():
                continue
            base = slots[b, t][has][0] - off[b, t][has][0]
            # a lane's first slot: base + items of lower waves + items of lower lanes
            assert np.array_equal(slots[b, t][has], base + off[b, t][has]), (b, t)
            bases.append((int(base), int(totals[b, t])))
    assert len(bases) == counts.shape[0] * counts.shape[1] - 1  # one trip of one workgroup reserved nothing
    # the reserved ranges are disjoint and fill [start, start + total) ...
    at = start
    for base, n in sorted(bases):
        assert base == at
        at += n
    assert at == start + total
    # ... and so do the items' own slots, lane by lane
    c = counts.reshape(-1).astype(np.int64)
    first = np.repeat(slots.reshape(-1), c)
    within = np.arange(c.sum(), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    assert np.array_equal(np.sort(first + within.astype(np.uint64)), np.uint64(start) + np.arange(total, dtype=np.uint64))


@pytest.mark.parametrize("n_rec,first", wr.TILE_CASES)
@pytest.mark.parametrize("vec", (wr.VOL_REC_VEC, wr.FF_REC_VEC))
def test_tile_stage(vec, n_rec, first):
    rec = wr.tile_records(n_rec, vec)
    lds, read = wave_probe.tile_stage(vec, rec, first, wr.TILE_FILL)
    want_lds, want_read = wr.tile_stage(rec, vec, first, wr.TILE_FILL)
    assert np.array_equal(read, want_read), "every thread reads the staged records back"
    assert np.array_equal(lds, want_lds), "the tile: the records, and behind them what the tile before left"
