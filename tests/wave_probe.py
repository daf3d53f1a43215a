"""ctypes view of tests/cpp/libwave_probe.so (tests/cpp/wave_probe.hip, built by __graft_entry__.build()): numpy arrays in,
numpy arrays out. The product library is loaded first (physics_amd._abi.load_library), so the process maps one ROCm
runtime and the probe's scan calls resolve to libphysics_hip.so's own code."""
import ctypes as C
import os

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "libwave_probe.so")
_lib = None

WAVE_OPS = {"scan": 0, "sum": 1, "max_u32": 2, "max_int": 3, "max_float": 4}
BLOCK_OPS = {"block_sum": 0, "put_get_sum": 1, "put_get_max_u32": 2, "put_get_max_float": 3}


class ProbeError(RuntimeError):
    pass


def load():
    """The probe library. A missing file is an error, not a skip: build() makes it."""
    global _lib
    if _lib is not None:
        return _lib
    from physics_amd import _abi
    _abi.load_library()
    if not os.path.exists(LIB_PATH):
        raise ProbeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    for name, res, args in (
            ("wave_probe_scan_is_one_launch", C.c_int32, [C.c_uint32]),
            ("wave_probe_scan_scratch_words", C.c_uint64, [C.c_uint32]),
            ("wave_probe_counters_layout", None, [p, p]),
            ("wave_probe_exclusive_scan", C.c_int32, [p, p, C.c_uint64, C.c_uint32, p, C.c_uint64, C.c_int32, p, C.c_uint64, p, C.c_uint64,
                                                      p, C.c_uint64]),
            ("wave_probe_block_scan", C.c_int32, [C.c_int32, p, C.c_uint64, C.c_uint32, p]),
            ("wave_probe_wave_op", C.c_int32, [C.c_int32, C.c_int32, C.c_uint32, p, p]),
            ("wave_probe_lane_rank", C.c_int32, [C.c_int32, C.c_uint32, p, p]),
            ("wave_probe_block_reduce", C.c_int32, [C.c_int32, C.c_int32, C.c_uint32, p, p]),
            ("wave_probe_append", C.c_int32, [C.c_uint32, p, p, p, p]),
            ("wave_probe_reserve", C.c_int32, [C.c_int32, C.c_uint32, C.c_uint32, p, p, p]),
            ("wave_probe_tile_stage", C.c_int32, [C.c_int32, p, C.c_uint32, C.c_uint32, C.c_uint32, p, p, p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _ptr(a):
    assert a.flags.c_contiguous and a.flags.writeable
    return a.ctypes.data_as(C.c_void_p)


def _ck(rc, what):
    if rc != 0:
        raise ProbeError(f"{what}: {'arguments refused' if rc < 0 else 'hipError_t ' + str(rc)}")


def scan_is_one_launch(count):
    return bool(load().wave_probe_scan_is_one_launch(count))


def scan_scratch_words(count):
    return int(load().wave_probe_scan_scratch_words(count))


def counters_layout():
    """(sizeof(StepCounters), offsetof(StepCounters, n_used_buckets))"""
    size, off = C.c_uint32(), C.c_uint32()
    load().wave_probe_counters_layout(C.byref(size), C.byref(off))
    return size.value, off.value


def exclusive_scan(world, in_buf, count, out_buf, zero_in, scratch, block_used=None, counters=None):
    """launch_exclusive_scan on the world's stream; every uint32 / uint8 array is changed in place to what the device left."""
    used_words = 0 if block_used is None else block_used.size
    _ck(load().wave_probe_exclusive_scan(world.h, _ptr(in_buf), in_buf.size, count, _ptr(out_buf), out_buf.size, int(zero_in),
                                         _ptr(scratch), scratch.size, None if block_used is None else _ptr(block_used), used_words,
                                         None if counters is None else _ptr(counters), 0 if counters is None else counters.nbytes),
        "wave_probe_exclusive_scan")


def block_scan(threads, p, count):
    """block_scan_in_place<threads> over p[:count] in place; returns the total each of the `threads` lanes got."""
    totals = np.full(threads, 0xDEADBEEF, np.uint32)
    _ck(load().wave_probe_block_scan(threads, _ptr(p), p.size, count, _ptr(totals)), "wave_probe_block_scan")
    return totals


def wave_op(op, threads, blocks, values):
    """One 32-bit word per thread (uint32, int32 or float32) through the wave primitive `op`; the same dtype back."""
    v = np.ascontiguousarray(values).copy()
    assert v.size == threads * blocks and v.dtype.itemsize == 4
    out = np.full(v.size, 0xDEADBEEF, np.uint32)
    _ck(load().wave_probe_wave_op(WAVE_OPS[op], threads, blocks, _ptr(v), _ptr(out)), "wave_probe_wave_op")
    return out.view(v.dtype)


def lane_rank(threads, blocks, masks):
    m = np.ascontiguousarray(masks, np.uint64).copy()
    assert m.size * 64 == threads * blocks
    out = np.full(threads * blocks, 0xDEADBEEF, np.uint32)
    _ck(load().wave_probe_lane_rank(threads, blocks, _ptr(m), _ptr(out)), "wave_probe_lane_rank")
    return out


def block_reduce(op, threads, blocks, values):
    v = np.ascontiguousarray(values).copy()
    assert v.size == threads * blocks and v.dtype.itemsize == 4
    out = np.full(v.size, 0xDEADBEEF, np.uint32)
    _ck(load().wave_probe_block_reduce(BLOCK_OPS[op], threads, blocks, _ptr(v), _ptr(out)), "wave_probe_block_reduce")
    return out.view(v.dtype)


def append(blocks, flags, counter_start):
    """wave_append_base in workgroups of 256: (base per lane, slot per lane, the counter afterwards)."""
    f = np.ascontiguousarray(flags, np.uint32).copy()
    assert f.size == blocks * 256
    counter = np.array([counter_start], np.uint32)
    base = np.full(f.size, 0xDEADBEEF, np.uint32)
    slot = np.full(f.size, 0xDEADBEEF, np.uint32)
    _ck(load().wave_probe_append(blocks, _ptr(f), _ptr(counter), _ptr(base), _ptr(slot)), "wave_probe_append")
    return base, slot, int(counter[0])


def reserve(by_count, counts, cursor_start):
    """slots_reserve_count / _flag over counts[block, trip, 256]: (first slot per lane, uint64 in the same shape; the cursor
    afterwards)."""
    c = np.ascontiguousarray(counts, np.uint32).copy()
    blocks, trips, threads = c.shape
    assert threads == 256
    cursor = np.array([cursor_start], np.uint64)
    slots = np.full(c.shape, 0xDEADBEEFDEADBEEF, np.uint64)
    _ck(load().wave_probe_reserve(int(by_count), blocks, trips, _ptr(c), _ptr(cursor), _ptr(slots)), "wave_probe_reserve")
    return slots, int(cursor[0])


def tile_stage(vec, rec, first, fill):
    """tile_stage<vec> over the tiles of 32 records [first, n): (lds[k, 32 * vec, 4], read[k, 256, 4]) as wave_ref.tile_stage."""
    r = np.ascontiguousarray(rec, np.float32).copy()
    n_rec = r.shape[0]
    n_tiles = (n_rec - first + 31) // 32
    f = np.array(fill, np.float32)
    lds = np.full((n_tiles, 32 * vec, 4), np.nan, np.float32)
    read = np.full((n_tiles, 256, 4), np.nan, np.float32)
    _ck(load().wave_probe_tile_stage(vec, _ptr(r), n_rec, first, n_tiles, _ptr(f), _ptr(lds), _ptr(read)), "wave_probe_tile_stage")
    return lds, read
