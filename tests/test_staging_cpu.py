"""The query calls' host-only part without a GPU: physics_amd/csrc/staging.hpp (the batches of the casts, move-and-slide,
character walking and depenetration, their argument checks, the layout of a call's arrays in its staging buffers and the bound
on their number) held to hand-worked values by tests/cpp/staging_probe.cpp, and the ctypes prototypes of the twelve cast and
eight capsule query entry points, which _abi.py generates, held to the lists as they were written out by hand."""
import ctypes as C
import os
import subprocess

from physics_amd import _abi
from physics_amd._abi import f32p, u16p, u32p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_layout_bound_and_cast_arguments(tmp_path):
    # address and undefined-behaviour sanitizers: the probe declares one array more than a layout holds
    exe = str(tmp_path / "staging_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "staging_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout


def test_cast_prototypes_are_the_hand_written_ones():
    vp = C.c_void_p
    want = {
        "phys_raycast": [vp, C.c_uint64, f32p, f32p, f32p, u32p, u32p, f32p, f32p],
        "phys_raycast_device": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp],
        "phys_spherecast": [vp, C.c_uint64, f32p, f32p, f32p, f32p, u32p, u32p, f32p, f32p],
        "phys_spherecast_device": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp],
        "phys_capsulecast": [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, f32p, u32p, u32p, f32p, f32p, f32p],
        "phys_capsulecast_device": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "phys_capsulecast_filtered": [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, f32p, u32p, u16p, u32p, f32p, f32p, f32p],
        "phys_capsulecast_device_filtered": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "phys_raycast_filtered": [vp, C.c_uint64, f32p, f32p, f32p, u32p, u16p, u32p, f32p, f32p],
        "phys_raycast_device_filtered": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp],
        "phys_spherecast_filtered": [vp, C.c_uint64, f32p, f32p, f32p, f32p, u32p, u16p, u32p, f32p, f32p],
        "phys_spherecast_device_filtered": [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        # the capsule query calls, as they stood written out by hand before their table
        "phys_move_and_slide": [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, C.c_float, C.c_uint32, u32p, u16p,
                                f32p, f32p, u32p, u32p, f32p, f32p],
        "phys_move_and_slide_device": [vp, C.c_uint64] + [vp] * 5 + [C.c_float, C.c_uint32] + [vp] * 8,
        "phys_character_move": [vp, C.c_uint64, f32p, f32p, f32p, f32p, f32p, u32p, C.c_float, C.c_uint32,
                                C.c_float, C.c_float, C.c_float, u32p, u16p, f32p, f32p, u32p, u32p, f32p, f32p,
                                u32p, f32p, f32p],
        "phys_character_move_device": [vp, C.c_uint64] + [vp] * 6 + [C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_float] + [vp] * 11,
        "phys_penetration": [vp, C.c_uint64, f32p, f32p, f32p, f32p, C.c_float, u32p, u16p, u32p, f32p, f32p],
        "phys_penetration_device": [vp, C.c_uint64] + [vp] * 4 + [C.c_float] + [vp] * 5,
        "phys_depenetrate": [vp, C.c_uint64, f32p, f32p, f32p, f32p, C.c_float, C.c_uint32, u32p, u16p,
                             f32p, u32p, u32p, f32p, f32p],
        "phys_depenetrate_device": [vp, C.c_uint64] + [vp] * 4 + [C.c_float, C.c_uint32] + [vp] * 7,
    }
    assert {k for k in _abi.PROTOTYPES if any(s in k for s in ("cast", "slide", "character", "penetrat"))} == set(want)
    for name, args in want.items():
        res, got = _abi.PROTOTYPES[name]
        assert res is C.c_int32, name
        assert len(got) == len(args) and all(g is a for g, a in zip(got, args)), (name, got)
