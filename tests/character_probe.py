"""Builds and runs tests/cpp/character_probe.cpp for the tests: character walking's own statement of its rule
(include/spec/character.h), compiled by the host compiler alone. Every batch travels as a text file of 32-bit words in hex,
floats by their bits.

A state here is the probe's 36 words per row, uint32 (n, 36); field(state, name) reads one member."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "character_probe.cpp")
MISS = 0xFFFFFFFE
BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
GROUNDED, STEPPED, SNAPPED, ON_STEEP, HIT_WALL, HIT_CEILING = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000, 0x20000
SLOT_NONE, SLOT_FLOOR = -1, -2
MOVE, UP, LIFTED, DOWN, GROUND, DONE = range(6)
WORDS = 36
# member -> (first word, words, is it a float)
_FIELDS = {"p": (0, 3, True), "m": (3, 3, True), "m0": (6, 3, True), "n_prev": (9, 3, True), "have_prev": (12, 1, False),
           "sl_status": (13, 1, False), "pos": (14, 3, True), "p_move": (17, 3, True), "m_move": (20, 3, True), "lift": (23, 1, True),
           "L": (24, 1, True), "skin": (25, 1, True), "step_height": (26, 1, True), "snap_distance": (27, 1, True),
           "min_floor_ny": (28, 1, True), "max_slides": (29, 1, False), "k": (30, 1, False), "phase": (31, 1, False),
           "walking": (32, 1, False), "ended": (33, 1, False), "floor_found": (34, 1, False), "status": (35, 1, False)}


def build(path, sanitize=False):
    """The probe at `path`. -ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


def _words(*cols):
    """rows of uint32 words: each column a float32 or integer array of n rows"""
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


def field(state, name):
    """one member of every row: float32 (n, 3) or (n,), or uint32 (n,)"""
    at, width, real = _FIELDS[name]
    w = np.ascontiguousarray(state[:, at:at + width])
    w = w.view(np.float32) if real else w
    return w.copy() if width > 1 else w[:, 0].copy()


def valid(exe, pos, motion, rot, R, h):
    """ch_valid per row; rot (n, 4) or None (identity)"""
    n = len(pos)
    q = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)) if rot is None else rot
    has = np.full(n, 0 if rot is None else 1, np.uint32)
    return _run(exe, 0, _words(pos, motion, has, q, R, h), 1)[:, 0].astype(bool)


def begin(exe, pos, motion, grounded, skin, max_slides, step_height, snap_distance, min_floor_ny):
    n = len(pos)
    f = lambda x: np.full(n, x, np.float32)
    return _run(exe, 1, _words(pos, motion, np.asarray(grounded, np.uint32), f(skin), np.full(n, max_slides, np.uint32), f(step_height),
                               f(snap_distance), f(min_floor_ny)), WORDS)


def next_cast(exe, state):
    """ch_next per row: (state, go, origin, dir, len, max_t, slot)"""
    w = _run(exe, 2, state, WORDS + 10)
    f = np.ascontiguousarray(w[:, WORDS + 1:WORDS + 9]).view(np.float32)
    return (w[:, :WORDS].copy(), w[:, WORDS].astype(bool), f[:, 0:3].copy(), f[:, 3:6].copy(), f[:, 6].copy(), f[:, 7].copy(),
            w[:, WORDS + 9].astype(np.int32))


def answer(exe, state, body, t, normal, point):
    """ch_answer per row: (state, floor_found)"""
    w = _run(exe, 3, np.concatenate([state, _words(np.asarray(body, np.uint32), np.asarray(t, np.float32), np.asarray(normal, np.float32),
                                                   np.asarray(point, np.float32))], axis=1), WORDS + 1)
    return w[:, :WORDS].copy(), w[:, WORDS].astype(bool)


def host_loop(exe, cast, pos, motion, radius, half_length, rot, grounded, skin, max_slides, step_height, snap_distance, min_floor_ny,
              ignore=None, mask=None, trace=None):
    """The loop of include/spec/character.h on the host: the probe's ch_next / ch_answer around `cast(origins, dirs, radius,
    half_length, rot, max_t, ignore, mask) -> (body, t, normal, point)` (World.capsulecast's keywords). Returns what
    World.character_move returns. trace: a list that receives (rows, phase, origin, dir, max_t, body, t, normal) per round."""
    f = np.float32
    pos, motion = np.asarray(pos, f).reshape(-1, 3), np.asarray(motion, f).reshape(-1, 3)
    n = len(pos)
    radius, half_length = np.broadcast_to(np.asarray(radius, f), (n,)).copy(), np.broadcast_to(np.asarray(half_length, f), (n,)).copy()
    rot = None if rot is None else np.asarray(rot, f).reshape(-1, 4)
    gr = np.zeros(n, np.uint32) if grounded is None else (np.asarray(grounded) != 0).astype(np.uint32)
    s = begin(exe, pos, motion, gr, skin, max_slides, step_height, snap_distance, min_floor_ny)
    ok = valid(exe, pos, motion, rot, radius, half_length)
    k = 2 * max_slides
    body = np.full((k, n), MISS, np.uint32)
    nrm, pnt = np.zeros((k, n, 3), f), np.zeros((k, n, 3), f)
    fbody, fnrm, fpnt = np.full(n, MISS, np.uint32), np.zeros((n, 3), f), np.zeros((n, 3), f)
    live = ok.copy()
    for _ in range(2 * max_slides + 4):
        rows = np.nonzero(live)[0]
        if len(rows) == 0:
            break
        part, go, origin, d, _, max_t, slot = next_cast(exe, s[rows])
        s[rows] = part
        live[rows[~go]] = False
        rows, origin, d, max_t, slot = rows[go], origin[go], d[go], max_t[go], slot[go]
        if len(rows) == 0:
            break
        sub = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
        b, t, nn, pp = cast(origin, d, radius[rows], half_length[rows], rot=sub(rot), max_t=max_t, ignore=sub(ignore),
                            mask=mask if mask is None or np.ndim(mask) == 0 else sub(mask))
        if trace is not None:
            trace.append((rows, field(s[rows], "phase"), origin, d, max_t, b, t, nn))
        fill = (b != MISS) & (slot >= 0)
        body[slot[fill], rows[fill]], nrm[slot[fill], rows[fill]], pnt[slot[fill], rows[fill]] = b[fill], nn[fill], pp[fill]
        part, found = answer(exe, s[rows], b, t, nn, pp)
        s[rows] = part
        floor = found & (slot == SLOT_FLOOR)
        fbody[rows[floor]], fnrm[rows[floor]], fpnt[rows[floor]] = b[floor], nn[floor], pp[floor]
    assert not live.any(), "the machine asked for more than 2 max_slides + 3 casts"
    status = field(s, "status")
    status[~ok] = INVALID
    return field(s, "p"), field(s, "m"), status, fbody, fnrm, fpnt, body, nrm, pnt
