"""Builds and runs tests/cpp/body_edit_probe.cpp for the tests: the body edits' own statement of their arithmetic
(include/spec/body_edit.h) and of the ordering and checks of a batch (physics_amd/csrc/setup.hpp), compiled by the host
compiler alone. The scene travels as a text file of 32-bit words in hex, floats by their bits."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "body_edit_probe.cpp")
LAYOUTS = {"shared": 0, "diag": 1, "full": 2}


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _bits(a):
    return [f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def write_scene(path, mode, layout, pos, ids, vec, point=None, third=None, vel=None, ang=None, mass=None, inv_mass=None, inertia=None,
                force=None, torque=None):
    """mode 'impulses' or 'forces'; layout a key of LAYOUTS; inertia (n, 3, 3) as set_bodies takes it (None: identity);
    inv_mass None: 1 / mass in float32, as the library stages it."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n, m = len(pos), len(ids)
    z = np.zeros((n, 3), np.float32)
    vel, ang = (z if vel is None else vel), (z if ang is None else ang)
    force, torque = (z if force is None else force), (z if torque is None else torque)
    mass = np.ones(n, np.float32) if mass is None else np.asarray(mass, np.float32)
    inv_mass = (np.float32(1.0) / mass).astype(np.float32) if inv_mass is None else np.asarray(inv_mass, np.float32)
    inertia = np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)) if inertia is None else np.asarray(inertia, np.float32)
    zm = np.zeros((m, 3), np.float32)
    lines = [f"{0 if mode == 'impulses' else 1:x} {n:x} {m:x} {LAYOUTS[layout]:x} {int(point is not None):x} {int(third is not None):x}"]
    for i in range(n):
        lines.append(" ".join(_bits(pos[i]) + _bits(vel[i]) + _bits(inv_mass[i]) + _bits(ang[i]) + _bits(mass[i]) + _bits(inertia[i])
                              + _bits(force[i]) + _bits(torque[i])))
    for k in range(m):
        lines.append(" ".join([f"{int(ids[k]):x}"] + _bits(vec[k]) + _bits((zm if point is None else point)[k])
                              + _bits((zm if third is None else third)[k])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run(exe, scene_path):
    """(a (n, 3), b (n, 3), inverse inertia (n, 3, 3)) float32 as the probe prints them: a, b = v, w or F, T."""
    out = subprocess.run([exe, scene_path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(-1, 15).view(np.float32)
    return w[:, :3].copy(), w[:, 3:6].copy(), w[:, 6:].reshape(-1, 3, 3).copy()
