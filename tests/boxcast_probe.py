"""Builds and runs tests/cpp/boxcast_probe.cpp for the tests: the box cast's own statement of its arithmetic
(include/spec/box_cast.h), compiled by the host compiler alone, every query against every target with no grid. The scene
travels as a text file of 32-bit words in hex, floats by their bits."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "boxcast_probe.cpp")


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _bits(a):
    return [f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def write_scene(path, case):
    """case: a dict of boxcast_cases (tg holds the targets with their ids; a centre is added back: the probe works in float32
    world coordinates as the kernel does)."""
    tg = case["tg"]
    m, n = len(tg["pos"]), len(case["o"])
    ground = case["ground"]
    lines = [f"{m:x} {n:x} {int(ground is not None):x} {_bits(0.0 if ground is None else ground)[0]}"]
    for k in range(m):
        lines.append(" ".join([f"{int(tg['shape'][k]):x}", f"{int(tg['id'][k]):x}"] + _bits(tg["pos"][k]) + _bits(tg["rot"][k])
                              + _bits(tg["half_extent"][k])))
    rot, mt, ig = case["rot"], case["max_t"], case["ignore"]
    for i in range(n):
        q = [0, 0, 0, 1] if rot is None else rot[i]
        lines.append(" ".join(_bits(case["o"][i]) + _bits(case["d"][i]) + [f"{int(rot is not None):x}"] + _bits(q) + _bits(case["he"][i])
                              + _bits(np.inf if mt is None else mt[i]) + [f"{0xFFFFFFFF if ig is None else int(ig[i]):x}"]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run(exe, scene_path):
    """(body (n,) uint32, t (n,), normal (n, 3), point (n, 3)) as the probe prints them."""
    out = subprocess.run([exe, scene_path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(-1, 8)
    f = w[:, 1:].copy().view(np.float32)
    return w[:, 0].copy(), f[:, 0].copy(), f[:, 1:4].copy(), f[:, 4:7].copy()


def evaluate(exe, tmp_dir, case):
    """write_scene + run in one call; the scene file goes to tmp_dir."""
    path = os.path.join(str(tmp_dir), f"boxcast_scene_{len(os.listdir(str(tmp_dir)))}.txt")
    write_scene(path, case)
    return run(exe, path)
