"""Builds and runs tests/cpp/liquid_probe.cpp for the tests: the liquids' own statement of their arithmetic
(include/spec/liquid.h) and of the checks and staging of a set (physics_amd/csrc/setup.hpp), compiled by the host compiler
alone. The scene travels as a text file of 32-bit words in hex, floats by their bits."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "liquid_probe.cpp")


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _bits(a):
    return [f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def write_scene(path, liquids, bodies, category=None, force=None, torque=None):
    """liquids, bodies: the dicts of liquid_ref.evaluate."""
    pos = np.asarray(bodies["pos"], np.float32).reshape(-1, 3)
    n, T = len(pos), len(liquids["density"])
    z = np.zeros((n, 3), np.float32)
    vel = z if bodies.get("vel") is None else bodies["vel"]
    ang = z if bodies.get("ang") is None else bodies["ang"]
    force, torque = (z if force is None else force), (z if torque is None else torque)
    cat = np.broadcast_to(np.asarray(1 if category is None else category, np.uint32), (n,))
    rot, mask = liquids.get("rot"), liquids.get("mask")
    lines = [f"{n:x} {T:x} {int(rot is not None):x} {int(mask is not None):x}"]
    for i in range(n):
        lines.append(" ".join([f"{int(bodies['shape'][i]):x}"] + _bits(pos[i]) + _bits(bodies["rot"][i]) + _bits(bodies["half_extent"][i])
                              + _bits(vel[i]) + _bits(ang[i]) + [f"{int(cat[i]):x}"] + _bits(force[i]) + _bits(torque[i])))
    for k in range(T):
        q = [0, 0, 0, 1] if rot is None else rot[k]
        m = 0xFFFF if mask is None else int(np.broadcast_to(mask, (T,))[k])
        lines.append(" ".join(_bits(liquids["pos"][k]) + _bits(q) + _bits(liquids["half_extent"][k]) + [f"{m:x}"] + _bits(liquids["density"][k])
                              + _bits(liquids["gravity"][k]) + _bits(liquids["flow"][k]) + _bits(liquids["drag"][k])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run(exe, scene_path):
    """(acted (n,) bool, force (n, 3), torque (n, 3), frac (n,) float32, liquid (n,) uint32) as the probe prints them."""
    out = subprocess.run([exe, scene_path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    acted = np.array([r[0] == "1" for r in rows], bool)
    w = np.array([[int(x, 16) for x in r[1:]] for r in rows], np.uint32).reshape(-1, 8)
    f = w[:, :7].copy().view(np.float32)
    return acted, f[:, :3].copy(), f[:, 3:6].copy(), f[:, 6].copy(), w[:, 7].copy()


def evaluate(exe, tmp_dir, liquids, bodies, **kw):
    """write_scene + run in one call; the scene file goes to tmp_dir."""
    path = os.path.join(str(tmp_dir), f"liquid_scene_{len(os.listdir(str(tmp_dir)))}.txt")
    write_scene(path, liquids, bodies, **kw)
    return run(exe, path)
