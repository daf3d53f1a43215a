"""CPU: the surface of the static colliders (phys_set_static_bodies / phys_get_static_stats) - header, exported symbols,
ctypes prototypes, World methods, the Rust shim and the id space - and the argument checks, which the library makes
before it looks at the world, so they run without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import physics_amd
from physics_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "physics_hip.h")
RUST = os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")
NAMES = ("phys_set_static_bodies", "phys_get_static_stats")


def test_header_declares_the_static_calls_and_the_id_bit():
    text = open(HEADER).read()
    for n in NAMES:
        assert re.search(rf"\bint32_t {n}\(", text), n
    m = re.search(r"#define PHYS_STATIC_ID_BIT (0x[0-9A-Fa-f]+)u", text)
    assert m and int(m.group(1), 16) == 0x80000000 == _abi.STATIC_ID_BIT == physics_amd.STATIC_ID_BIT


def test_library_exports_and_binds_the_static_calls():
    lib = _abi.load_library()
    for n in NAMES:
        assert hasattr(lib, n) and n in _abi.PROTOTYPES
    assert _abi.PROTOTYPES["phys_set_static_bodies"][1][1] is C.c_uint64
    assert len(_abi.PROTOTYPES["phys_get_static_stats"][1]) == 4


def test_rust_shim_declares_the_static_calls():
    text = open(RUST).read()
    for n in NAMES:
        assert len(re.findall(rf"\bpub fn {n}\(", text)) == 1, n
    assert "PHYS_STATIC_ID_BIT: u32 = 0x8000_0000" in text


def test_world_has_the_static_methods():
    assert callable(physics_amd.World.set_static_bodies) and callable(physics_amd.World.get_static_stats)


def test_static_ids_sort_between_bodies_and_ground():
    bit = physics_amd.STATIC_ID_BIT
    largest_body = 0x7FFFFFFE - 1  # phys_set_bodies caps bodies + ghosts below 0x7FFFFFFF
    largest_static = bit | (0x7FFFFFFE - 1)
    assert largest_body < bit <= largest_static < physics_amd.GROUND_ID
    assert largest_static != physics_amd.RAY_MISS and (bit | 0) != physics_amd.RAY_MISS


def _call(n, pos, rot, shape, he):
    lib = _abi.load_library()
    f = lambda a, t=_abi.f32p: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    rc = lib.phys_set_static_bodies(None, n, f(pos), f(rot), f(shape, _abi.u32p), f(he))
    return rc, lib.phys_last_error().decode()


def _valid(n=3):
    pos = np.zeros((n, 3), np.float32)
    rot = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))
    shape = np.full(n, physics_amd.SHAPE_BOX, np.uint32)
    he = np.ones((n, 3), np.float32)
    return pos, rot, shape, he


def test_valid_arguments_reach_the_world_check():
    pos, rot, shape, he = _valid()
    rc, msg = _call(3, pos, rot, shape, he)
    assert rc == _abi.PHYS_ERR_INVALID_ARG and msg == "null world"
    rc, msg = _call(3, pos, None, shape, he)  # rot NULL = identity
    assert msg == "null world"
    rc, msg = _call(0, None, None, None, None)  # n = 0 clears the set
    assert msg == "null world"


@pytest.mark.parametrize("case", ["count", "shape_none", "shape_other", "pos_nan", "pos_inf", "rot_nan", "he_inf",
                                  "he_negative", "null_shape", "null_he", "null_pos"])
def test_invalid_arguments_are_rejected(case):
    pos, rot, shape, he = _valid()
    n = 3
    want = {"count": "too many static", "shape_none": "neither SPHERE nor BOX", "shape_other": "neither SPHERE nor BOX",
            "pos_nan": "non-finite", "pos_inf": "non-finite", "rot_nan": "non-finite", "he_inf": "non-finite",
            "he_negative": "negative half extent", "null_shape": "need pos", "null_he": "need pos", "null_pos": "need pos"}[case]
    if case == "count":
        n = 0x7FFFFFFE
    elif case == "shape_none":
        shape[1] = physics_amd.SHAPE_NONE
    elif case == "shape_other":
        shape[2] = 7
    elif case == "pos_nan":
        pos[1, 2] = np.nan
    elif case == "pos_inf":
        pos[0, 0] = -np.inf
    elif case == "rot_nan":
        rot[2, 3] = np.nan
    elif case == "he_inf":
        he[1, 1] = np.inf
    elif case == "he_negative":
        he[2, 0] = -0.5
    elif case == "null_shape":
        shape = None
    elif case == "null_he":
        he = None
    elif case == "null_pos":
        pos = None
    rc, msg = _call(n, pos, rot, shape, he)
    assert rc == _abi.PHYS_ERR_INVALID_ARG
    assert want in msg, msg


def test_world_method_checks_array_sizes():
    w = physics_amd.World.__new__(physics_amd.World)  # no device: only the Python-side checks
    w.lib, w.h = _abi.load_library(), C.c_void_p()
    with pytest.raises(ValueError):
        w.set_static_bodies(np.zeros((2, 3)), shape_type=[1], half_extent=np.ones((2, 3)))
    with pytest.raises(ValueError):
        w.set_static_bodies(np.zeros((2, 3)), rot=np.zeros((3, 4)), shape_type=[1, 1], half_extent=np.ones((2, 3)))
