"""The per-update planner (physics_amd/csrc/plan.hpp) without a GPU: the header compiles with a host compiler alone, and
tests/cpp/plan_probe.cpp holds every threshold, size and debug switch to values worked out from the launch functions the
planner replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "physics_amd", "csrc", "plan.hpp")


def test_plan_header_needs_no_hip():
    # no include path at all: what it includes is the standard library and the C header of the ABI, by relative path
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", "-"], input=f'#include "{PLAN}"\n', text=True, check=True)


def test_plan_matches_the_launch_functions_it_replaced(tmp_path):
    exe = str(tmp_path / "plan_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
