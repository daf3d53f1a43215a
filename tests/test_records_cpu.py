"""The records the collision kernels exchange (physics_amd/csrc/records.hpp) without a GPU: the header compiles with a host
compiler alone, and tests/cpp/records_probe.cpp holds every word's bit positions and every record's offsets to the layouts
of DESIGN.md section 21, encode-then-decode over the whole domain of each word."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = os.path.join(ROOT, "physics_amd", "csrc", "records.hpp")


def test_records_header_needs_no_hip():
    # no include path at all: what it includes is the standard library and the planner's header, by relative path
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", "-"], input=f'#include "{RECORDS}"\n', text=True, check=True)


def test_records_match_their_stated_layouts(tmp_path):
    exe = str(tmp_path / "records_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "records_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
