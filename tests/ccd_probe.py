"""Builds and runs tests/cpp/ccd_probe.cpp for the tests: continuous collision's own statement of its arithmetic
(include/spec/ccd.h) and the staging of its list (physics_amd/csrc/setup.hpp stage_ccd), compiled by the host compiler alone. The
scene travels as a text file of 32-bit words in hex, floats by their bits."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "ccd_probe.cpp")
FILTER_DEFAULT = (0xFFFF0001, 0)  # category 0x0001 | mask 0xFFFF << 16, group 0


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _bits(a):
    return [f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def filter_words(category, mask, group):
    """the two words of a filter as the library packs them (setup.hpp pack_filters)"""
    return (int(category) & 0xFFFF) | ((int(mask) & 0xFFFF) << 16), int(group) & 0xFFFFFFFF


def write_scene(path, case):
    """case: a dict with dt, margin, ground (None or y), exact_rot, statics (shape, pos, rot, half_extent[, filt (m, 2)]) and
    bodies (shape, pos, rot, half_extent, lin, ang[, filt (n, 2)]); ground_filt: the ground's filter word. Filters anywhere
    make the scene a filtered one."""
    st, bd = case["statics"], case["bodies"]
    m, n = len(st["pos"]), len(bd["pos"])
    ground = case.get("ground")
    filtered = "filt" in st or "filt" in bd or "ground_filt" in case
    sf = np.asarray(st["filt"], np.uint64).reshape(m, 2) if "filt" in st else np.tile(np.array(FILTER_DEFAULT, np.uint64), (m, 1))
    bf = np.asarray(bd["filt"], np.uint64).reshape(n, 2) if "filt" in bd else np.tile(np.array(FILTER_DEFAULT, np.uint64), (n, 1))
    lines = [" ".join([f"{m:x}", f"{n:x}", f"{int(ground is not None):x}", _bits(0.0 if ground is None else ground)[0], _bits(case["dt"])[0],
                       _bits(case["margin"])[0], f"{int(bool(case.get('exact_rot'))):x}", f"{int(filtered):x}",
                       f"{int(case.get('ground_filt', FILTER_DEFAULT[0])):x}"])]
    for k in range(m):
        lines.append(" ".join([f"{int(st['shape'][k]):x}"] + _bits(st["pos"][k]) + _bits(st["rot"][k]) + _bits(st["half_extent"][k])
                              + [f"{int(sf[k, 0]):x}", f"{int(sf[k, 1]):x}"]))
    for i in range(n):
        lines.append(" ".join([f"{int(bd['shape'][i]):x}"] + _bits(bd["pos"][i]) + _bits(bd["rot"][i]) + _bits(bd["half_extent"][i])
                              + _bits(bd["lin"][i]) + _bits(bd["ang"][i]) + [f"{int(bf[i, 0]):x}", f"{int(bf[i, 1]):x}"]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run(exe, scene_path):
    """(frac (n,), target (n,) uint32, normal (n, 3), pos (n, 3), rot (n, 4)) as the probe prints them."""
    out = subprocess.run([exe, scene_path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(-1, 12)
    f = w.copy().view(np.float32)
    return f[:, 0].copy(), w[:, 1].copy(), f[:, 2:5].copy(), f[:, 5:8].copy(), f[:, 8:12].copy()


def evaluate(exe, tmp_dir, case):
    """write_scene + run in one call; the scene file goes to tmp_dir."""
    path = os.path.join(str(tmp_dir), f"ccd_scene_{len(os.listdir(str(tmp_dir)))}.txt")
    write_scene(path, case)
    return run(exe, path)


def staging(exe, n_owned, ids):
    """stage_ccd(ids, n_owned): (code, kept ids, message, code for null ids, code for n = 2^31)"""
    out = subprocess.run([exe, "--staging", str(int(n_owned))] + [str(int(i)) for i in ids], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    first = [int(x) for x in lines[0].split()]
    null_code, big_code = (int(x) for x in lines[2].split())
    return first[0], first[1:], lines[1], null_code, big_code
