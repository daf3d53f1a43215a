"""CPU: the numpy reference of the wave primitives and the exclusive scan (tests/wave_ref.py) on hand-written cases, the
case tables the GPU tests run (tests/test_gpu_wave_primitives.py) against the conditions those tests rely on, and the
host side of scan.hip - where the one-launch scan ends and how many scratch words a table needs - through the probe
library, which loads without a GPU."""
import numpy as np

import wave_probe
import wave_ref as wr


# ---- the reference on cases written out by hand -------------------------------------------------------------------------
def test_exclusive_scan_by_hand():
    assert wr.exclusive_scan([3, 0, 2, 5]).tolist() == [0, 3, 3, 5, 10]
    assert wr.exclusive_scan([]).tolist() == [0]
    assert wr.exclusive_scan([0xFFFFFFFF, 2, 0xFFFFFFFF]).tolist() == [0, 0xFFFFFFFF, 1, 0]
    assert wr.exclusive_scan(np.zeros(8, np.uint32)).tolist() == [0] * 9


def test_block_scan_by_hand():
    p, total = wr.block_scan_in_place([1, 2, 3, 4, 9, 9], 4)
    assert p.tolist() == [0, 1, 3, 6, 9, 9] and total == 10
    p, total = wr.block_scan_in_place([7, 7], 0)
    assert p.tolist() == [7, 7] and total == 0


def test_wave_scan_sum_max_by_hand():
    v = np.zeros(128, np.uint32)
    v[0], v[5], v[63], v[64], v[127] = 1, 2, 4, 0xFFFFFFFF, 3
    inc = wr.wave_inclusive_scan(v)
    assert inc[0] == 1 and inc[4] == 1 and inc[5] == 3 and inc[62] == 3 and inc[63] == 7
    assert inc[64] == 0xFFFFFFFF and inc[126] == 0xFFFFFFFF and inc[127] == 2  # each wave on its own, modulo 2^32
    assert wr.wave_sum(v).tolist() == [7] * 64 + [2] * 64
    assert wr.wave_max(v).tolist() == [4] * 64 + [0xFFFFFFFF] * 64
    i = np.full(64, -5, np.int32)
    i[17] = -2
    assert wr.wave_max(i).tolist() == [-2] * 64 and wr.wave_max(i).dtype == np.int32
    f = np.full(64, -1.5, np.float32)
    f[40] = 0.25
    assert wr.wave_max(f).tolist() == [0.25] * 64


def test_lane_rank_and_ballot_by_hand():
    assert wr.lane_rank(0).tolist() == [0] * 64
    assert wr.lane_rank((1 << 64) - 1).tolist() == list(range(64))
    assert wr.lane_rank(1).tolist() == [0] + [1] * 63
    assert wr.lane_rank(1 << 63).tolist() == [0] * 64  # nothing lies below lane 63's own bit
    assert wr.lane_rank(0b1011)[:5].tolist() == [0, 1, 2, 2, 3]
    flags = np.zeros(128, np.uint32)
    flags[[0, 3, 63, 64 + 63]] = 1
    assert wr.ballot(flags).tolist() == [(1 << 63) | 0b1001, 1 << 63]


def test_block_reduce_and_reserve_offsets_by_hand():
    v = np.arange(512, dtype=np.uint32)
    assert wr.block_reduce(v, 256, "sum").tolist() == [255 * 128] * 256 + [(256 + 511) * 128] * 256
    assert wr.block_reduce(v, 256, "max").tolist() == [255] * 256 + [511] * 256
    c = np.zeros((1, 2, 256), np.uint32)
    c[0, 0, [0, 1, 70]] = 2, 3, 4
    c[0, 1, 255] = 9
    off, total = wr.reserve_offsets(c)
    assert off[0, 0, :3].tolist() == [0, 2, 5] and off[0, 0, 70] == 5 and off[0, 0, 71] == 9 and off[0, 1, 255] == 0
    assert total.tolist() == [[9, 9]]


def test_wave_max_nan_contract_by_hand():
    v = np.arange(64, dtype=np.float32)
    v[0] = np.nan
    full = np.full(64, 63.0, np.float32)
    full[0] = np.nan
    assert wr.wave_max_nan_contract_holds(v, full)           # every other lane found the whole maximum
    part = full.copy()
    part[32] = 62.0                                          # a lane that missed what lay behind the NaN lane: allowed
    assert wr.wave_max_nan_contract_holds(v, part)
    bad = full.copy()
    bad[0] = 63.0                                            # the NaN lane must end with NaN ...
    assert not wr.wave_max_nan_contract_holds(v, bad)
    bad = full.copy()
    bad[40] = 39.0                                           # ... no lane below its own value ...
    assert not wr.wave_max_nan_contract_holds(v, bad)
    bad = full.copy()
    bad[40] = 62.5                                           # ... or with a value no lane held
    assert not wr.wave_max_nan_contract_holds(v, bad)


def test_tile_stage_by_hand():
    rec = wr.tile_records(40, 6)
    assert rec[3, 2].tolist() == [3080.0, 3081.0, 3082.0, 3083.0]
    assert np.unique(rec).size == rec.size
    lds, read = wr.tile_stage(rec, 6, 0, wr.TILE_FILL)
    assert lds.shape == (2, 192, 4) and read.shape == (2, 256, 4)
    assert np.array_equal(lds[0], rec[:32].reshape(-1, 4))
    assert np.array_equal(lds[1, :48], rec[32:].reshape(-1, 4)) and np.array_equal(lds[1, 48:], lds[0, 48:])
    assert np.array_equal(read[1, 0], rec[32:].reshape(-1, 4)[67 % 48]) and np.array_equal(read[0, 200], rec[:32].reshape(-1, 4)[75])
    lds, _ = wr.tile_stage(rec[:5], 6, 0, wr.TILE_FILL)
    assert np.array_equal(lds[0, 30:], np.tile(np.float32(wr.TILE_FILL), (162, 1)))


# ---- the case tables ----------------------------------------------------------------------------------------------------
def test_scan_tables_meet_their_conditions():
    assert all(c % 4 == 0 for c in wr.SCAN_COUNTS)
    for count in wr.SCAN_COUNTS:
        tables = {k: wr.scan_values(count, k) for k in wr.SCAN_KINDS}
        for k, v in tables.items():
            assert v.dtype == np.uint32 and v.size == count
            assert np.array_equal(v, wr.scan_values(count, k))  # fixed seeds
        total = {k: int(v.astype(np.uint64).sum()) for k, v in tables.items()}
        assert total["random"] < 1 << 32 and int(tables["random"].max()) <= 3
        zeros = np.count_nonzero(tables["random"] == 0) / count
        assert count < 2048 or 0.4 < zeros < 0.6
        assert total["zero"] == 0
        assert np.count_nonzero(tables["last"]) == 1 and tables["last"][-1] != 0
        assert total["wrap"] > 1 << 32


def test_block_scan_tables_meet_their_conditions():
    for t in (256, 1024):
        counts = wr.block_scan_counts(t)
        assert {0, 1, 63, 64, 65, t - 1, t, t + 1, 2 * t, 2 * t + 1, 3 * t + 5} == set(counts)
        for count in counts:
            v = wr.block_scan_values(t, count)
            assert v.size == count + wr.BLOCK_SCAN_GUARD and np.all(v[count:] == wr.POISON)
            assert count < 64 or (np.any(v[:count] == 0) and np.any(v[:count] != 0))


def test_wave_tables_meet_their_conditions():
    for threads, blocks in wr.WAVE_GEOMETRIES:
        n = threads * blocks
        assert int(wr.wave_values("u32", n).astype(np.uint64).reshape(-1, 64).sum(axis=1).max()) > 1 << 32  # sums wrap
        assert int(wr.wave_values("small", n).max()) <= 32
        i, f = wr.wave_values("int", n), wr.wave_values("float", n)
        assert i.dtype == np.int32 and np.all(i[:64] < 0) and np.any(i > 0)
        assert f.dtype == np.float32 and np.all(np.isfinite(f)) and np.all(f[:64] < 0) and np.any(f > 0)
        m = wr.lane_rank_masks(n // 64)
        assert m.size == n // 64 and m.dtype == np.uint64
        assert m[:5].tolist() == [0, (1 << 64) - 1, 1, 1 << 63, 0x5555555555555555]
    nan = wr.nan_values(256 * 3).reshape(-1, 64)
    assert np.isnan(nan[0, 0]) and not np.isnan(nan[0, 1:]).any() and np.isnan(nan[1, 63]) and np.isnan(nan[3]).all()
    assert np.isnan(nan[4:]).any() and not np.isnan(nan[4:]).all(axis=1).any()


def test_append_and_reserve_tables_meet_their_conditions():
    f = wr.append_flags().reshape(-1, 64)
    assert f.shape[0] == wr.APPEND_BLOCKS * wr.APPEND_THREADS // 64
    assert np.all(f.sum(axis=1) >= 1)  # wave_append_base needs a non-zero ballot
    assert f[0].sum() == 1 and f[0, 63] == 1 and f[1].sum() == 1 and f[1, 0] == 1 and f[2].sum() == 64
    for by_count in (False, True):
        c = wr.reserve_counts(by_count)
        assert c.shape == (wr.RESERVE_BLOCKS, wr.RESERVE_TRIPS, wr.RESERVE_THREADS) and c.shape[1] >= 3
        assert int(c.max()) == (32 if by_count else 1)
        per_trip = c.reshape(c.shape[0], c.shape[1], -1).sum(axis=2)
        assert per_trip[wr.RESERVE_EMPTY] == 0 and np.count_nonzero(per_trip == 0) == 1
        per_wave = c.reshape(c.shape[0], c.shape[1], 4, 64).sum(axis=3)
        assert np.count_nonzero((per_wave == 0) & (per_trip[:, :, None] != 0)) >= 4  # waves with nothing in trips with something
        assert per_wave.max() == (32 * 64 if by_count else 64)
        total = int(c.sum())
        lo, hi = wr.RESERVE_STARTS
        assert lo == 0 and hi < 1 << 32 < hi + total  # the second run carries into the cursor's high word


def test_tile_cases_meet_their_conditions():
    (n0, first0), (n1, first1) = wr.TILE_CASES
    assert first0 > 0 and -(-(n0 - first0) // wr.TILE_RECORDS) == 3 and (n0 - first0) % wr.TILE_RECORDS != 0
    assert 0 < n1 - first1 < wr.TILE_RECORDS
    assert 7 * wr.TILE_RECORDS <= wr.TILE_THREADS


# ---- scan.hip, host side ------------------------------------------------------------------------------------------------
def test_scan_hand_over_and_scratch_words():
    assert wave_probe.scan_is_one_launch(wr.SCAN_ONE_LAUNCH_LIMIT) and not wave_probe.scan_is_one_launch(wr.SCAN_ONE_LAUNCH_LIMIT + 4)
    for count in wr.SCAN_COUNTS:
        assert wave_probe.scan_is_one_launch(count) == (count <= wr.SCAN_ONE_LAUNCH_LIMIT)
    for k in (1, 16, 17, 1024, 1025, 2048):
        assert wave_probe.scan_scratch_words(wr.SCAN_CHUNK * k) == k
        assert wave_probe.scan_scratch_words(wr.SCAN_CHUNK * k + 4) == k + 1
    # the three workgroup counts of k_scan_block_sums' one, two and three trips
    assert [wave_probe.scan_scratch_words(c) for c in wr.SCAN_COUNTS[-3:]] == [1024, 1025, 2049]
    size, off = wave_probe.counters_layout()
    assert size % 4 == 0 and off % 4 == 0 and off + 4 <= size
