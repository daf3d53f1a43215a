"""Builds and runs tests/cpp/field_probe.cpp for the tests: the force fields' own statement of their arithmetic
(include/spec/force_field.h) and of the checks and staging of a set (physics_amd/csrc/setup.hpp), compiled by the host compiler
alone. The scene travels as a text file of 32-bit words in hex, floats by their bits."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "field_probe.cpp")


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _bits(a):
    return [f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def write_scene(path, fields, pos, vel=None, ang=None, mass=None, category=None, force=None, torque=None):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n, T = len(pos), len(fields["kind"])
    z = np.zeros((n, 3), np.float32)
    vel, ang = (z if vel is None else vel), (z if ang is None else ang)
    force, torque = (z if force is None else force), (z if torque is None else torque)
    mass = np.ones(n, np.float32) if mass is None else mass
    cat = np.broadcast_to(np.asarray(1 if category is None else category, np.uint32), (n,))
    rot, mask, ex = fields.get("rot"), fields.get("mask"), fields.get("exponent")
    lines = [f"{n:x} {T:x} {int(rot is not None):x} {int(mask is not None):x} {int(ex is not None):x}"]
    for i in range(n):
        lines.append(" ".join(_bits(pos[i]) + _bits(vel[i]) + _bits(ang[i]) + _bits(mass[i]) + [f"{int(cat[i]):x}"] + _bits(force[i])
                              + _bits(torque[i])))
    for k in range(T):
        q = [0, 0, 0, 1] if rot is None else rot[k]
        m = 0xFFFF if mask is None else int(np.broadcast_to(mask, (T,))[k])
        e = 0 if ex is None else int(ex[k])
        lines.append(" ".join([f"{int(fields['kind'][k]):x}", f"{int(fields['shape'][k]):x}"] + _bits(fields["pos"][k]) + _bits(q)
                              + _bits(fields["half_extent"][k]) + [f"{m:x}"] + _bits(fields["vec"][k]) + _bits(fields["coef"][k]) + [f"{e:x}"]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run(exe, scene_path):
    """(acted (n,) bool, force (n, 3) float32, torque (n, 3) float32) as the probe prints them."""
    out = subprocess.run([exe, scene_path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    acted = np.array([r[0] == "1" for r in rows], bool)
    w = np.array([[int(x, 16) for x in r[1:]] for r in rows], np.uint32).reshape(-1, 6).view(np.float32)
    return acted, w[:, :3].copy(), w[:, 3:].copy()
