"""Builds and runs tests/cpp/slide_probe.cpp for the tests: move-and-slide's own statement of its rule
(include/spec/slide.h), compiled by the host compiler alone. Every batch travels as a text file of 32-bit words in hex, floats
by their bits.

A state here is a dict of rows: p, m, m0, n_prev float32 (n, 3), have_prev and status uint32 (n,)."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "slide_probe.cpp")
MISS = 0xFFFFFFFE
BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
_KEYS = ("p", "m", "m0", "n_prev")


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _words(*cols):
    """rows of uint32 words: each column a float32 or uint32 array of n rows"""
    out = []
    for c in cols:
        c = np.asarray(c)
        c = np.ascontiguousarray(c, np.float32 if c.dtype.kind == "f" else np.uint32)
        out.append(c.reshape(len(c), -1).view(np.uint32))
    return np.concatenate(out, axis=1)


def _run(exe, op, rows, width):
    """the probe over rows of words (op prepended); its answer as (n, width) uint32"""
    if len(rows) == 0:
        return np.zeros((0, width), np.uint32)
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for r in rows:
            f.write(f"{op:x} " + " ".join(f"{int(x):x}" for x in r) + "\n")
        path = f.name
    try:
        out = subprocess.run([exe, path], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(len(rows), width)


def _state_words(s):
    return _words(s["p"], s["m"], s["m0"], s["n_prev"], np.asarray(s["have_prev"], np.uint32), np.asarray(s["status"], np.uint32))


def _state(w):
    f = np.ascontiguousarray(w[:, :12]).view(np.float32)
    s = {k: f[:, 3 * i:3 * i + 3].copy() for i, k in enumerate(_KEYS)}
    s["have_prev"], s["status"] = w[:, 12].copy(), w[:, 13].copy()
    return s


def take(s, rows):
    return {k: v[rows] for k, v in s.items()}


def put(s, rows, part):
    for k in s:
        s[k][rows] = part[k]


def valid(exe, pos, motion, rot, R, h):
    """sl_valid per row; rot (n, 4) or None (identity)"""
    n = len(pos)
    q = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)) if rot is None else rot
    has = np.full(n, 0 if rot is None else 1, np.uint32)
    return _run(exe, 0, _words(pos, motion, has, q, R, h), 1)[:, 0].astype(bool)


def begin(exe, pos, motion):
    return _state(_run(exe, 4, _words(pos, motion), 14))


def before_cast(exe, s, skin):
    """(L, max_t, go) per row: the length of the motion left, how far its cast looks, and whether there is a cast at all"""
    n = len(s["status"])
    w = _run(exe, 1, np.concatenate([_state_words(s), _words(np.full(n, skin, np.float32))], axis=1), 3)
    f = np.ascontiguousarray(w[:, :2]).view(np.float32)
    return f[:, 0].copy(), f[:, 1].copy(), w[:, 2].astype(bool)


def after_cast(exe, s, skin, body, t, normal):
    """(state, go) per row after the cast's answer: a miss makes the whole motion, a hit stops, projects and goes on (go) or
    blocks"""
    n = len(s["status"])
    w = _run(exe, 2, np.concatenate([_state_words(s), _words(np.full(n, skin, np.float32), np.asarray(body, np.uint32),
                                                             np.asarray(t, np.float32), np.asarray(normal, np.float32))], axis=1), 15)
    return _state(w[:, :14]), w[:, 14].astype(bool)


def ran_out(exe, s):
    return _state(_run(exe, 3, _state_words(s), 14))


def host_loop(exe, cast, pos, motion, radius, half_length, rot, skin, max_slides, ignore=None, mask=None):
    """The loop of include/spec/slide.h on the host: max_slides rounds of `cast(origins, dirs, radius, half_length, rot, max_t,
    ignore, mask) -> (body, t, normal, point)` (World.capsulecast's keywords) with the probe's steps between them. Returns what
    World.move_and_slide returns."""
    f = np.float32
    pos, motion = np.asarray(pos, f).reshape(-1, 3), np.asarray(motion, f).reshape(-1, 3)
    n = len(pos)
    radius, half_length = np.broadcast_to(np.asarray(radius, f), (n,)).copy(), np.broadcast_to(np.asarray(half_length, f), (n,)).copy()
    rot = None if rot is None else np.asarray(rot, f).reshape(-1, 4)
    s = begin(exe, pos, motion)
    ok = valid(exe, pos, motion, rot, radius, half_length)
    s["status"][~ok] = INVALID
    body = np.full((max_slides, n), MISS, np.uint32)
    nrm, pnt = np.zeros((max_slides, n, 3), f), np.zeros((max_slides, n, 3), f)
    live = ok.copy()
    for k in range(max_slides):
        rows = np.nonzero(live)[0]
        if len(rows) == 0:
            break
        part = take(s, rows)
        _, max_t, go = before_cast(exe, part, skin)
        live[rows[~go]] = False
        rows, part, max_t = rows[go], take(part, go), max_t[go]
        if len(rows) == 0:
            break
        sub = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
        b, t, nn, pp = cast(part["p"], part["m"], radius[rows], half_length[rows], rot=sub(rot), max_t=max_t, ignore=sub(ignore),
                            mask=mask if mask is None or np.ndim(mask) == 0 else sub(mask))
        hit = b != MISS
        body[k, rows[hit]], nrm[k, rows[hit]], pnt[k, rows[hit]] = b[hit], nn[hit], pp[hit]
        part, go = after_cast(exe, part, skin, b, t, nn)
        put(s, rows, part)
        live[rows[~go]] = False
    rows = np.nonzero(live)[0]  # the casts ran out for these
    if len(rows):
        put(s, rows, ran_out(exe, take(s, rows)))
    return s["p"], s["m"], s["status"], body, nrm, pnt
