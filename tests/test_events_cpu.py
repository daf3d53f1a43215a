"""CPU: the contact-event surface of the C ABI (symbols, prototypes, the 48-byte struct, argument errors that need no
device) and tests/events_ref.py, the numpy-only reference the GPU tests compare the drained events with, on hand-written
sequences."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import events_ref as er
from physics_amd import _abi
from physics_amd import world as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("phys_contact_events_enable", "phys_get_contact_events", "phys_get_contact_impulses")
G = 0xFFFFFFFF


def test_symbols_exported_and_prototyped():
    lib = _abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _abi.PROTOTYPES, name
    assert _abi.PROTOTYPES["phys_get_contact_events"][1][1] == C.POINTER(_abi.PhysContactEvent)
    assert (_abi.CONTACT_BEGIN, _abi.CONTACT_END) == (1, 2)


def test_event_struct_matches_the_c_compiler(tmp_path):
    fields = [n for n, _ in _abi.PhysContactEvent._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "physics_hip.h"\nint main(){printf("%zu %u %u", sizeof(phys_contact_event), '
           "PHYS_CONTACT_BEGIN, PHYS_CONTACT_END);" +
           "".join(f'printf(" %zu", offsetof(phys_contact_event, {f}));' for f in fields) + "}")
    exe = str(tmp_path / "event_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[:3] == [48, 1, 2] and C.sizeof(_abi.PhysContactEvent) == 48
    assert got[3:] == [getattr(_abi.PhysContactEvent, f).offset for f in fields]
    # ... and the numpy record World.get_contact_events returns
    assert pw.CONTACT_EVENT_DTYPE.itemsize == 48
    assert [pw.CONTACT_EVENT_DTYPE.fields[f][1] for f in fields] == got[3:]


def test_null_arguments_are_errors_without_a_device():
    lib = _abi.load_library()
    n = C.c_uint64(7)
    assert lib.phys_contact_events_enable(None, 16) == _abi.PHYS_ERR_INVALID_ARG
    assert b"null world" in lib.phys_last_error()
    assert lib.phys_get_contact_events(None, None, 0, C.byref(n), None) == _abi.PHYS_ERR_INVALID_ARG
    assert lib.phys_get_contact_impulses(None, None, 0, C.byref(n)) == _abi.PHYS_ERR_INVALID_ARG
    assert n.value == 7  # nothing written


def test_rust_shim_and_cpp_mirror_name_the_struct_and_the_calls():
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    assert "pub struct phys_contact_event" in rust and all(f"pub fn {s}(" in rust for s in SYMBOLS)
    body = rust.split("pub struct phys_contact_event", 1)[1].split("}", 1)[0]
    assert re.findall(r"pub (\w+):", body) == [n for n, _ in _abi.PhysContactEvent._fields_]
    hpp = open(os.path.join(ROOT, "include", "physics_state.hpp")).read()
    for name in ("enable_contact_events", "drain_contact_events", "contact_impulses"):
        assert name in hpp, name


def test_events_ref_imports_numpy_only():
    txt = open(os.path.join(ROOT, "tests", "events_ref.py")).read()
    assert set(re.findall(r"^\s*(?:from|import)\s+([A-Za-z0-9_\.]+)", txt, flags=re.M)) == {"numpy"}


def _tuples(ev):
    return [tuple(int(x) for x in r) for r in ev]


def test_ref_touch_persist_part_touch_again():
    seq = [[(0, G)], [(0, G)], [], [(0, G)]]
    assert _tuples(er.expected_events(seq)) == [(1, er.BEGIN, 0, G), (3, er.END, 0, G), (4, er.BEGIN, 0, G)]


def test_ref_orders_by_step_kind_a_b_and_counts_steps_from_first_step():
    seq = [[(3, 9), (1, 2), (1, G)], [(1, 2), (0, 5), (0, 0x80000001)]]
    assert _tuples(er.expected_events(seq, first_step=10)) == [
        (10, er.BEGIN, 1, 2), (10, er.BEGIN, 1, G), (10, er.BEGIN, 3, 9),
        (11, er.BEGIN, 0, 5), (11, er.BEGIN, 0, 0x80000001), (11, er.END, 1, G), (11, er.END, 3, 9)]


def test_ref_reset_in_the_middle_forgets_the_history():
    seq = [[(0, 1), (2, G)], er.RESET, [(0, 1), (2, G)], [(0, 1)]]
    assert _tuples(er.expected_events(seq)) == [
        (1, er.BEGIN, 0, 1), (1, er.BEGIN, 2, G), (2, er.BEGIN, 0, 1), (2, er.BEGIN, 2, G), (3, er.END, 2, G)]


def test_ref_empty_updates_and_a_previous_set():
    assert len(er.expected_events([[], [], []])) == 0
    assert len(er.expected_events([])) == 0
    got = er.expected_events([[(4, 5)], []], first_step=7, previous=[(4, 5), (6, 7)])
    assert _tuples(got) == [(7, er.END, 6, 7), (8, er.END, 4, 5)]


def test_ref_refuses_a_pair_listed_twice_and_keys_of_reads_drained_records():
    try:
        er.expected_events([[(1, 2), (1, 2)]])
        raise AssertionError("duplicate accepted")
    except ValueError:
        pass
    ev = np.zeros(2, pw.CONTACT_EVENT_DTYPE)
    ev["body_a"], ev["body_b"], ev["kind"], ev["step"] = [1, 1], [2, G], [1, 1], [1, 1]
    assert np.array_equal(er.keys_of(ev), er.expected_events([[(1, 2), (1, G)]]))
