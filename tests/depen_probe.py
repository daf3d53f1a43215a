"""Builds and runs tests/cpp/depen_probe.cpp for the tests: depenetration's own statement of its rule
(include/spec/depenetrate.h), compiled by the host compiler alone. Every batch travels as a text file of 32-bit words in hex,
floats by their bits.

Targets here are a dict(id u32 (m,), shape u32 (m,), pos f32 (m, 3), rot f32 (m, 4), half_extent f32 (m, 3)) or None, in the order
the probe tests them; ground is a height or None."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "depen_probe.cpp")
MISS, GROUND = 0xFFFFFFFE, 0xFFFFFFFF
STUCK, INVALID = 0x100, 0x400
F = np.float32


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
        c = np.ascontiguousarray(c, F if c.dtype.kind == "f" else np.uint32)
        out.append(c.reshape(len(c), -1).view(np.uint32))
    return np.concatenate(out, axis=1)


def _run(exe, op, rows, width, tail=()):
    """the probe over rows of words (op prepended, `tail` appended to every row); its answer as (n, width) uint32"""
    if len(rows) == 0:
        return np.zeros((0, width), np.uint32)
    tail = " ".join(f"{int(x):x}" for x in tail)
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for r in rows:
            f.write(f"{op:x} " + " ".join(f"{int(x):x}" for x in r) + " " + tail + "\n")
        path = f.name
    try:
        out = subprocess.run([exe, path], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(len(rows), width)


def _query_words(pos, rot, R, h):
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    q = np.tile(np.array([0, 0, 0, 1], F), (n, 1)) if rot is None else np.asarray(rot, F).reshape(-1, 4)
    has = np.full(n, 0 if rot is None else 1, np.uint32)
    return _words(pos, has, q, np.broadcast_to(np.asarray(R, F), (n,)), np.broadcast_to(np.asarray(h, F), (n,)))


def _target_words(targets, ground):
    """the words of a target list (one flat row, the same for every query)"""
    head = _words(np.array([0 if ground is None else 1], np.uint32), np.array([0.0 if ground is None else ground], F))[0]
    m = 0 if targets is None else len(targets["id"])
    if m == 0:
        return np.concatenate([head, np.zeros(1, np.uint32)])
    body = _words(np.asarray(targets["id"], np.uint32), np.asarray(targets["shape"], np.uint32), np.asarray(targets["pos"], F),
                  np.asarray(targets["rot"], F), np.asarray(targets["half_extent"], F))
    return np.concatenate([head, np.array([m], np.uint32), body.reshape(-1)])


def _f(w):
    return np.ascontiguousarray(w).view(F)


def valid(exe, pos, rot, R, h):
    """dp_valid per row; rot (n, 4) or None (identity)"""
    return _run(exe, 0, _query_words(pos, rot, R, h), 1)[:, 0].astype(bool)


def step(exe, p, status, k, max_iters, skin, body, depth, normal):
    """dp_step per row at round k: (p, status, go)"""
    n = len(p)
    w = _run(exe, 1, _words(np.asarray(p, F), np.asarray(status, np.uint32), np.full(n, k, np.uint32), np.full(n, max_iters, np.uint32),
                            np.full(n, skin, F), np.asarray(body, np.uint32), np.asarray(depth, F), np.asarray(normal, F)), 5)
    return _f(w[:, :3]).copy(), w[:, 3].copy(), w[:, 4].astype(bool)


def deepest(exe, pos, rot, R, h, gap, targets, ground):
    """the probe's dp_deepest per query over the explicit list: (id, depth, normal)"""
    w = _run(exe, 2, np.concatenate([_query_words(pos, rot, R, h), _words(np.full(len(np.asarray(pos).reshape(-1, 3)), gap, F))], axis=1), 5,
             tail=_target_words(targets, ground))
    return w[:, 0].copy(), _f(w[:, 1]).copy(), _f(w[:, 2:5]).copy()


def run(exe, pos, rot, R, h, skin, max_iters, targets, ground):
    """the whole loop per query over the explicit list: what World.depenetrate returns"""
    n = len(np.asarray(pos).reshape(-1, 3))
    w = _run(exe, 3, np.concatenate([_query_words(pos, rot, R, h), _words(np.full(n, skin, F), np.full(n, max_iters, np.uint32))], axis=1),
             4 + 5 * max_iters, tail=_target_words(targets, ground))
    slots = w[:, 4:].reshape(n, max_iters, 5)
    return (_f(w[:, :3]).copy(), w[:, 3].copy(), np.ascontiguousarray(slots[:, :, 0].T),
            np.ascontiguousarray(_f(slots[:, :, 1:4]).transpose(1, 0, 2)), np.ascontiguousarray(_f(slots[:, :, 4]).T))


def host_loop(exe, penetration, pos, radius, half_length, rot, skin, max_iters, ignore=None, mask=None):
    """The loop of include/spec/depenetrate.h on the host: max_iters + 1 rounds of `penetration(pos, radius, half_length, rot,
    max_gap, ignore, mask) -> (body, depth, normal)` (World.penetration's keywords) with the probe's dp_step between them.
    Returns what World.depenetrate returns."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    radius, half_length = np.broadcast_to(np.asarray(radius, F), (n,)).copy(), np.broadcast_to(np.asarray(half_length, F), (n,)).copy()
    rot = None if rot is None else np.asarray(rot, F).reshape(-1, 4)
    p, status = pos.copy(), np.zeros(n, np.uint32)
    ok = valid(exe, pos, rot, radius, half_length)
    status[~ok] = INVALID
    body = np.full((max_iters, n), MISS, np.uint32)
    nrm, dep = np.zeros((max_iters, n, 3), F), np.zeros((max_iters, n), F)
    live = ok.copy()
    for k in range(max_iters + 1):
        rows = np.nonzero(live)[0]
        if len(rows) == 0:
            break
        sub = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
        b, d, nn = penetration(p[rows], radius[rows], half_length[rows], rot=sub(rot), max_gap=skin, ignore=sub(ignore),
                               mask=mask if mask is None or np.ndim(mask) == 0 else sub(mask))
        p[rows], status[rows], go = step(exe, p[rows], status[rows], k, max_iters, skin, b, d, nn)
        if k < max_iters:
            body[k, rows[go]], nrm[k, rows[go]], dep[k, rows[go]] = b[go], nn[go], d[go]
        else:
            assert not go.any()
        live[rows[~go]] = False
    return p, status, body, nrm, dep
