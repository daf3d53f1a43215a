"""World set-up and read-out arithmetic (physics_amd/csrc/setup.hpp, readout.hpp) without a GPU: both headers compile with a
host compiler alone, and tests/cpp/setup_probe.cpp holds every function to values worked out by hand from the code the headers
replaced, to a brute-force restatement, or - the volume records of include/spec/volume.h - to bits derived by hand (DESIGN.md
sections 17 and 20). The validation messages are also reached through the
library: phys_set_static_bodies and phys_set_triggers check their arguments before they look at the world."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physics_amd", "csrc")


@pytest.mark.parametrize("header", ["setup.hpp", "readout.hpp", "staging.hpp"])
def test_header_needs_no_hip(header):
    # no include path at all: the standard library, the C header of the ABI, plan.hpp and include/spec, by relative path
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", "-"],
                   input=f'#include "{os.path.join(CSRC, header)}"\n', text=True, check=True)


def test_setup_matches_the_code_it_replaced(tmp_path):
    exe = str(tmp_path / "setup_probe")
    # -ffp-contract=off: the library's own flag (st_cell must give the device's cells)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "setup_probe.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout


def _arrays(n):
    return (C.c_uint32 * n)(*([2] * n)), (C.c_float * (3 * n))(), (C.c_float * (4 * n))(*([0.0, 0.0, 0.0, 1.0] * n)), (C.c_float * (3 * n))()


@pytest.mark.parametrize("call,noun", [("phys_set_static_bodies", "static collider"), ("phys_set_triggers", "trigger")])
def test_validation_messages_through_the_abi(call, noun):
    from physics_amd import _abi
    lib = _abi.load_library()
    E = _abi.PHYS_ERR_INVALID_ARG

    def run(shape, pos, rot, he):
        if call == "phys_set_static_bodies":
            return lib.phys_set_static_bodies(None, 3, pos, rot, shape, he)
        return lib.phys_set_triggers(None, 3, shape, pos, rot, he, None)

    def err():
        return lib.phys_last_error().decode()

    shape, pos, rot, he = _arrays(3)
    assert run(shape, pos, rot, he) == E and err() == "null world"  # every item passes: the world is looked at next
    assert run(shape, pos, None, he) == E and err() == "null world"
    shape[2] = 0
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 2: shape is neither SPHERE nor BOX nor CAPSULE"
    he[3 * 2] = float("nan")  # the shape is checked first
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 2: shape is neither SPHERE nor BOX nor CAPSULE"
    shape[2] = 3
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 2: non-finite pose or half extent"
    he[3 * 2] = 0.0
    pos[3 * 1 + 1] = float("inf")
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 1: non-finite pose or half extent"
    pos[3 * 1 + 1] = 0.0
    rot[4 * 2 + 1] = float("nan")
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 2: non-finite pose or half extent"
    assert run(shape, pos, None, he) == E and err() == "null world"  # rot NULL: not looked at
    rot[4 * 2 + 1] = 0.0
    he[3 * 1 + 2] = -1.0
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 1: negative half extent"
    he[3 * 1 + 0] = float("-inf")  # non-finite and negative: non-finite is said first
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 1: non-finite pose or half extent"
    he[3 * 1 + 0] = 0.0
    he[0] = -2.0  # several offend: the first index
    assert run(shape, pos, rot, he) == E and err() == f"{noun} 0: negative half extent"
