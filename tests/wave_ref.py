"""Plain numpy restatement of the wave and workgroup primitives of physics_amd/csrc/wave.hpp and of the exclusive scan of
scan.hip, and the case tables (fixed seeds) that tests/test_wave_ref_cpu.py checks and tests/test_gpu_wave_primitives.py
runs through tests/cpp/wave_probe.hip. Everything is integer arithmetic or an exact maximum: the GPU results are compared
for equality. numpy only."""
import numpy as np

WAVE = 64
M32 = (1 << 32) - 1


# ---- the primitives ---------------------------------------------------------------------------------------------------
def exclusive_scan(values):
    """scan.hip: out[count + 1] of `values` (uint32), out[count] the grand total, everything modulo 2^32."""
    v = np.asarray(values, np.uint64)
    out = np.zeros(v.size + 1, np.uint64)
    np.cumsum(v, out=out[1:])
    return (out & np.uint64(M32)).astype(np.uint32)


def block_scan_in_place(p, count):
    """block_scan_in_place: (the buffer behind it, the total every lane gets); words from `count` on are untouched."""
    p = np.asarray(p, np.uint32).copy()
    s = exclusive_scan(p[:count])
    p[:count] = s[:count]
    return p, int(s[count])


def _waves(values):
    v = np.asarray(values)
    assert v.size % WAVE == 0
    return v.reshape(-1, WAVE)


def wave_inclusive_scan(values):
    """uint32 per lane -> inclusive prefix sum inside each wave of 64 consecutive lanes, modulo 2^32."""
    w = _waves(np.asarray(values, np.uint32)).astype(np.uint64)
    return (np.cumsum(w, axis=1) & np.uint64(M32)).astype(np.uint32).reshape(-1)


def wave_sum(values):
    w = _waves(np.asarray(values, np.uint32)).astype(np.uint64)
    t = (w.sum(axis=1) & np.uint64(M32)).astype(np.uint32)
    return np.repeat(t, WAVE)


def wave_max(values):
    """Maximum of each wave in every lane (uint32, int32 or float32 WITHOUT NaN; the dtype is kept)."""
    w = _waves(values)
    return np.repeat(w.max(axis=1), WAVE)


def lane_rank(mask):
    """The 64 ranks of one ballot: set bits of `mask` below each lane."""
    mask = int(mask)
    return np.array([bin(mask & ((1 << lane) - 1)).count("1") for lane in range(WAVE)], np.uint32)


def ballot(flags):
    """One 64-bit mask per wave of the per-lane flags (lane 0 = bit 0)."""
    w = _waves(np.asarray(flags) != 0)
    return np.array([sum(1 << l for l in range(WAVE) if row[l]) for row in w], np.uint64)


def block_reduce(values, threads, op):
    """block_sum / block_put + block_get: the workgroup's sum (mod 2^32) or maximum, in every thread."""
    v = np.asarray(values)
    g = v.reshape(-1, threads)
    if op == "sum":
        t = (g.astype(np.uint64).sum(axis=1) & np.uint64(M32)).astype(np.uint32)
    else:
        t = g.max(axis=1)
    return np.repeat(t, threads)


def reserve_offsets(counts):
    """slots_reserve: counts[block, trip, thread] -> (offset of each lane's first slot from its (workgroup, trip) base =
    items of lower waves + items of lower lanes, total[block, trip])."""
    c = np.asarray(counts, np.uint64)
    incl = np.cumsum(c, axis=2)
    return incl - c, incl[:, :, -1]


def wave_max_nan_contract_holds(values, got):
    """What wave.hpp promises of wave_max<float> when lanes hold NaN, per wave: a NaN lane ends with NaN; every other lane
    ends with one of the wave's non-NaN values that is no smaller than its own (and so no larger than their maximum)."""
    for v, g in zip(_waves(np.asarray(values, np.float32)), _waves(np.asarray(got, np.float32))):
        nan = np.isnan(v)
        if not np.all(np.isnan(g[nan])):
            return False
        clean = set(v[~nan].tolist())
        for own, res in zip(v[~nan], g[~nan]):
            if np.isnan(res) or res < own or float(res) not in clean:
                return False
    return True


def tile_stage(rec, vec, first, fill, tile=32, threads=256, shift=67):
    """The probe's walk over the tiles of `tile` records [first, n): rec[n, vec, 4]. Returns (lds[k, tile * vec, 4]: the LDS
    tile behind the staging of tile k - its first tn * vec vectors the records, the rest what was there before -,
    read[k, threads, 4]: the vector (x + shift) % (tn * vec) of it for every thread x)."""
    rec = np.asarray(rec, np.float32).reshape(-1, vec, 4)
    lds_now = np.tile(np.asarray(fill, np.float32), (tile * vec, 1))
    lds, read = [], []
    for t0 in range(first, rec.shape[0], tile):
        tn = min(tile, rec.shape[0] - t0)
        lds_now = lds_now.copy()
        lds_now[:tn * vec] = rec[t0:t0 + tn].reshape(-1, 4)
        lds.append(lds_now)
        read.append(lds_now[(np.arange(threads) + shift) % (tn * vec)])
    return np.stack(lds), np.stack(read)


# ---- case tables --------------------------------------------------------------------------------------------------------
SCAN_ONE_LAUNCH_LIMIT = 32768  # k_scan_small: 1024 threads x 32 counters
SCAN_CHUNK = 2048              # counters per workgroup of the three-launch scan = per scratch word
# one launch up to 32768; 17 blocks; 1024 blocks = one trip of block_scan_in_place<1024> over the block sums; 1025 = a second
# trip with a carry; 2049 = a third, which uses the first set of wave totals again
SCAN_COUNTS = (4, 60, 64, 2044, 2048, 2052, 32764, 32768, 32772, 34816, 2097152, 2097156, 4194308)
SCAN_KINDS = ("random", "zero", "last", "wrap")
SCAN_PAD = 64                  # words of 0xFFFFFFFF behind the counters
SCAN_GUARD = 64                # poisoned words behind out[count] and behind the scratch words
POISON = 0xA5A5A5A5


def scan_values(count, kind):
    """The table of a scan case (uint32[count])."""
    rng = np.random.default_rng([1801, count, SCAN_KINDS.index(kind)])
    if kind == "random":  # 0..3, about half zeros
        v = rng.integers(1, 4, count, dtype=np.uint32)
        v[rng.random(count) < 0.5] = 0
        return v
    if kind == "zero":
        return np.zeros(count, np.uint32)
    if kind == "last":
        v = np.zeros(count, np.uint32)
        v[-1] = 7
        return v
    assert kind == "wrap"  # every word at least 2^30: four of them already pass 2^32
    return rng.integers(1 << 30, 1 << 32, count, dtype=np.uint64).astype(np.uint32)


def block_scan_counts(threads):
    t = threads
    return (0, 1, 63, 64, 65, t - 1, t, t + 1, 2 * t, 2 * t + 1, 3 * t + 5)


BLOCK_SCAN_GUARD = 16


def block_scan_values(threads, count):
    """uint32[count + guard]: small numbers with zeros among them; the guard behind them is POISON."""
    rng = np.random.default_rng([1802, threads, count])
    v = rng.integers(0, 5, count + BLOCK_SCAN_GUARD, dtype=np.uint32)
    v[count:] = POISON
    return v


WAVE_GEOMETRIES = ((64, 9), (256, 3), (1024, 2))  # (threads per workgroup, workgroups)
BLOCK_GEOMETRIES = ((256, 3), (1024, 2))


def wave_values(kind, n):
    """One word per thread. "u32": full range, sums wrap; "small": 0..32 (a wave's sum fits); "int": int32 with negatives,
    one wave of them all negative; "float": finite float32 of both signs, one wave all negative."""
    rng = np.random.default_rng([1803, ("u32", "small", "int", "float").index(kind), n])
    if kind == "u32":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "small":
        return rng.integers(0, 33, n, dtype=np.uint32)
    if kind == "int":
        v = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
        v[:WAVE] = -np.abs(v[:WAVE].astype(np.int64)).astype(np.int32) - 1
        return v
    assert kind == "float"
    v = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    v[:WAVE] = -np.abs(v[:WAVE]) - np.float32(1.0)
    return v


def nan_values(n):
    """float32 per thread with NaN lanes: wave 0 has one in lane 0, wave 1 in lane 63, wave 2 in every odd lane, wave 3 is all
    NaN, the others have random ones; needs n >= 4 waves."""
    rng = np.random.default_rng([1804, n])
    v = rng.standard_normal(n).astype(np.float32).reshape(-1, WAVE)
    assert v.shape[0] >= 4
    v[0, 0] = np.nan
    v[1, 63] = np.nan
    v[2, 1::2] = np.nan
    v[3, :] = np.nan
    v[4:][rng.random(v[4:].shape) < 0.2] = np.nan
    return v.reshape(-1)


def lane_rank_masks(n_waves):
    """uint64 per wave: 0, all ones, bit 0 only, bit 63 only, the two alternating patterns, then random ones."""
    fixed = [0, (1 << 64) - 1, 1, 1 << 63, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    rng = np.random.default_rng([1805, n_waves])
    rnd = rng.integers(0, 1 << 64, max(n_waves - len(fixed), 0), dtype=np.uint64)
    return np.concatenate([np.array(fixed, np.uint64), rnd])[:n_waves]


APPEND_BLOCKS, APPEND_THREADS = 8, 256


def append_flags():
    """uint32[8 * 256] hit flags: every wave has a hit; wave 0 has exactly one (lane 63), wave 1 only lane 0, wave 2 all 64."""
    rng = np.random.default_rng(1806)
    f = (rng.random((APPEND_BLOCKS * APPEND_THREADS // WAVE, WAVE)) < 0.4).astype(np.uint32)
    f[0] = 0
    f[0, 63] = 1
    f[1] = 0
    f[1, 0] = 1
    f[2] = 1
    for row in f:
        if not row.any():
            row[rng.integers(0, WAVE)] = 1
    return f.reshape(-1)


RESERVE_BLOCKS, RESERVE_TRIPS, RESERVE_THREADS = 6, 5, 256
RESERVE_EMPTY = (2, 3)  # the (workgroup, trip) with nothing to reserve
RESERVE_STARTS = (0, (1 << 32) - 100)


def reserve_counts(by_count):
    """uint32[6, 5, 256] items per lane: 0..32 (by_count) or 0 / 1. RESERVE_EMPTY has none; other trips have waves without
    any; with by_count one wave holds 32 in every lane."""
    rng = np.random.default_rng([1807, int(by_count)])
    shape = (RESERVE_BLOCKS, RESERVE_TRIPS, RESERVE_THREADS // WAVE, WAVE)
    if by_count:
        c = rng.integers(0, 33, shape, dtype=np.uint32)
        c[rng.random(shape) < 0.5] = 0
    else:
        c = (rng.random(shape) < 0.3).astype(np.uint32)
    c[rng.random(shape[:3]) < 0.25] = 0  # whole waves with nothing
    c[0, 1, 2] = 32 if by_count else 1   # a full wave
    c[1, 0, 0] = 0                       # nothing in the first wave of a trip, and ...
    c[1, 0, 1, 5] = 3 if by_count else 1
    c[4, 4, 3] = 0                       # ... the last wave of the last trip
    c[4, 4, 0, 63] = 32 if by_count else 1
    c[RESERVE_EMPTY] = 0
    return c.reshape(RESERVE_BLOCKS, RESERVE_TRIPS, RESERVE_THREADS)


VOL_REC_VEC, FF_REC_VEC = 6, 7  # include/spec/volume.h, force_field.h (the probe refuses any other width)
TILE_RECORDS, TILE_THREADS, TILE_SHIFT = 32, 256, 67
TILE_FILL = (-1.0, -2.0, -3.0, -4.0)
# (records, first): tiles of 32, 32 and 11 records from t0 = 32; one tile of 5 records, the fill behind them
TILE_CASES = ((107, 32), (101, 96))


def tile_records(n_rec, vec):
    """float32[n_rec, vec, 4], every word different: record * 1024 + vector * 4 + word (exact in float32)."""
    return np.arange(n_rec * vec * 4, dtype=np.float32).reshape(n_rec, vec, 4) + \
        (np.arange(n_rec, dtype=np.float32) * (1024 - vec * 4)).reshape(-1, 1, 1)
