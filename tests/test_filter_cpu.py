"""CPU: collision filters (include/physics_hip.h) without a GPU: the new symbols are declared,
exported and bound; argument errors of a NULL world; the Python layer's checks before the library is reached; the numpy
rule against a hand table; the halo record encoding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from physics_amd import _abi, filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["phys_set_body_filters", "phys_get_body_filters", "phys_set_static_filters", "phys_set_ground_filter",
       "phys_raycast_filtered", "phys_raycast_device_filtered", "phys_spherecast_filtered", "phys_spherecast_device_filtered",
       "phys_overlap_filtered"]


def test_symbols_declared_exported_bound_and_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "physics_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    lib = _abi.load_library()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert len(re.findall(rf"pub fn {n}\s*\(", rust)) == 1, n
        assert hasattr(lib, n) and n in _abi.PROTOTYPES, n
    assert "#define PHYS_FILTER_DEFAULT_CATEGORY 0x0001u" in header and "#define PHYS_FILTER_DEFAULT_MASK 0xFFFFu" in header
    assert lib.phys_abi_version() == 2 == _abi.PHYS_ABI_VERSION
    assert (_abi.FILTER_DEFAULT_CATEGORY, _abi.FILTER_DEFAULT_MASK) == (0x0001, 0xFFFF)


def test_null_world_is_an_argument_error():
    lib = _abi.load_library()
    E = _abi.PHYS_ERR_INVALID_ARG
    u16 = (C.c_uint16 * 4)()
    i16 = (C.c_int16 * 4)()
    f = (C.c_float * 12)()
    u32 = (C.c_uint32 * 4)()
    u64 = (C.c_uint64 * 5)()
    assert lib.phys_set_body_filters(None, 0, None, None, None) == E
    assert lib.phys_set_body_filters(None, 4, u16, u16, i16) == E
    assert lib.phys_get_body_filters(None, u16, u16, i16) == E
    assert lib.phys_set_static_filters(None, 0, None, None, None) == E
    assert lib.phys_set_ground_filter(None, 1, 0xFFFF) == E
    assert lib.phys_raycast_filtered(None, 4, f, f, None, None, u16, u32, f, None) == E
    assert lib.phys_raycast_device_filtered(None, 4, None, None, None, None, None, None, None, None) == E
    assert lib.phys_spherecast_filtered(None, 4, f, f, f, None, None, u16, u32, f, None) == E
    assert lib.phys_spherecast_device_filtered(None, 4, None, None, None, None, None, None, None, None, None) == E
    assert lib.phys_overlap_filtered(None, 4, u32, f, None, f, None, u16, 0, u64, None) == E
    assert b"null world" in lib.phys_last_error()


class _NoLib:
    """Stands in for the library: any call reaching it is a failure of the Python checks."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def _world(n=4, n_static=2):
    from physics_amd.world import World
    w = World.__new__(World)
    w.lib, w.h, w.n, w.n_static = _NoLib(), C.c_void_p(), n, n_static
    return w


@pytest.mark.parametrize("kw", [dict(category=[1, 2, 3]), dict(mask=np.ones((4, 1), np.uint16)), dict(category=[1, 2, 3, 0x10000]),
                                dict(mask=[-1, 0, 0, 0]), dict(group=[0, 0, 0, 40000]), dict(group=[0, 0, 0, -32769]),
                                dict(category=[1.0, 2.0, 3.0, 4.0]), dict(group=["a", "b", "c", "d"])])
def test_python_rejects_bad_filters_before_the_library(kw):
    w = _world()
    with pytest.raises(ValueError):
        w.set_body_filters(**kw)
    with pytest.raises(ValueError):
        w.set_static_filters(**kw)  # two statics: every case is mis-shaped or out of range for them too


@pytest.mark.parametrize("args", [(1.5, 3), (-1, 3), (1, 0x10000), (True, 3), (None, 3)])
def test_python_rejects_bad_ground_filter(args):
    with pytest.raises(ValueError):
        _world().set_ground_filter(*args)


@pytest.mark.parametrize("mask", [[1, 2, 3], 0x10000, -1, [1.0, 1.0, 1.0, 1.0], np.ones((4, 2), np.uint16)])
def test_python_rejects_bad_query_masks(mask):
    w = _world()
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    with pytest.raises(ValueError):
        w.raycast(o, d, mask=mask)
    with pytest.raises(ValueError):
        w.spherecast(o, d, 0.5, mask=mask)
    with pytest.raises(ValueError):
        w.overlap(1, o, half_extent=[1, 0, 0], mask=mask)


# (category, mask, group) of A, of B, collide?
TABLE = [
    ((0x0001, 0xFFFF, 0), (0x0001, 0xFFFF, 0), True),     # defaults
    ((0x0002, 0xFFFF, 0), (0x0001, 0xFFFD, 0), False),    # A's category misses B's mask
    ((0x0002, 0xFFFD, 0), (0x0001, 0xFFFF, 0), True),     # ... only one direction matters per side: B in A's mask, A in B's
    ((0x0004, 0x0004, 0), (0x0004, 0x0004, 0), True),     # a layer that only collides with itself
    ((0x0004, 0x0004, 0), (0x0001, 0xFFFF, 0), False),    # ... and not with the default layer
    ((0x0001, 0x0000, 3), (0x0002, 0x0000, 3), True),     # same positive group overrides masks
    ((0x0001, 0xFFFF, -2), (0x0001, 0xFFFF, -2), False),  # same negative group overrides masks
    ((0x0001, 0xFFFF, -2), (0x0001, 0xFFFF, -3), True),   # different negative groups: category / mask
    ((0x0001, 0x0002, 5), (0x0001, 0xFFFF, 6), False),    # different positive groups: category / mask
    ((0x0001, 0xFFFF, 7), (0x0001, 0xFFFF, 0), True),     # group against no group: category / mask
    ((0x0000, 0xFFFF, 0), (0x0001, 0xFFFF, 0), False),    # category 0 collides with nothing outside a positive group
]


def test_numpy_rule_matches_the_hand_table():
    A = np.array([r[0] for r in TABLE])
    B = np.array([r[1] for r in TABLE])
    want = np.array([r[2] for r in TABLE])
    got = filters.collide(A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1], B[:, 2])
    assert got.tolist() == want.tolist()
    assert filters.collide(B[:, 0], B[:, 1], B[:, 2], A[:, 0], A[:, 1], A[:, 2]).tolist() == want.tolist()  # symmetric


def test_halo_encoding_round_trips_and_defaults_are_zero():
    q4, q5 = filters.halo_encode(0x0001, 0xFFFF, 0, False)
    assert (int(q4), int(q5)) == (0, 0)
    q4, q5 = filters.halo_encode(0x0001, 0xFFFF, 0, True)
    assert (int(q4), int(q5)) == (1, 0)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 0x10000, 1000)
    m = rng.integers(0, 0x10000, 1000)
    g = rng.integers(-0x8000, 0x8000, 1000)
    full = rng.integers(0, 2, 1000).astype(bool)
    q4, q5 = filters.halo_encode(c, m, g, full)
    assert q4.dtype == np.uint32 and q5.dtype == np.uint32
    c2, m2, g2, f2 = filters.halo_decode(q4, q5)
    assert np.array_equal(c2, c) and np.array_equal(m2, m) and np.array_equal(g2, g) and np.array_equal(f2, full)
