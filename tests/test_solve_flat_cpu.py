"""CPU: the cluster solver's flat row driver (solve_manifold_flat, include/spec/contact_solve.h) against the driver it restates
(solve_manifold_geo), bit for bit, through tests/cpp/solve_flat_probe.cpp: the spec header and a host compiler alone, built once
plain and once under the address and undefined-behaviour sanitizers (a stand-alone program, run here).

What is compared after EVERY sweep of a solve: vA, wA, the twelve accumulated impulses; after the first sweep the twelve row
masses; vB and wB only when the manifold has a body B (the flat driver leaves them unspecified otherwise - its contract).
Where there is no body B, solve_manifold_geo gets live garbage for it, as oracle/oracle_api.cpp passes it, and must not have
touched vB and wB; the flat driver gets the zeros its caller owes it.

Every manifold is solved four ways: full and diagonal inverse inertia tensors (inertia_mul branches on it), cold (the first
sweep makes the masses and relaxes, then 8 regular sweeps) and warm (the first sweep makes the masses and applies non-zero
starting impulses, then 8 sweeps): the three instantiations the kernel chooses among."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "solve_flat_probe.cpp")
F = np.float32
SWEEPS = 8
SIDE = 12 + (1 + SWEEPS) * 24  # words of one driver's record


def build(path, sanitize=False):
    """-ffp-contract=off: the library's own flag, so the host rounds as the device does."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, SOURCE, "-o", path], check=True)
    return path


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("solve_flat") / "solve_flat_probe"), sanitize=request.param == "sanitized")


def manifold(count, has_b, n, pts, bias, xA, imA, IA, xB, imB, IB, vel, friction, imp):
    """one manifold as float32 words (everything but the four leading integers of a probe line)"""
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in
                           (n, pts, bias, xA, [imA], IA, xB, [imB], IB, vel, [friction], imp)]).astype(F), count, has_b


def lines_of(m):
    """the four solves of one manifold: (full, diagonal) tensors x (cold, warm)"""
    words, count, has_b = m
    out = []
    for diag in (0, 1):
        w = words.copy()
        if diag:
            for at in (23, 36):  # IA, IB: keep the diagonal
                t = w[at:at + 9].reshape(3, 3).copy()
                w[at:at + 9] = np.diag(np.diag(t)).reshape(-1)
        for warm in (0, 1):
            out.append((count, has_b, warm, w))
    return out


def run(exe, lines, tmp_path):
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        for count, has_b, warm, w in lines:
            assert len(w) == 70
            f.write(f"{count:x} {has_b:x} {warm:x} {SWEEPS:x} " + " ".join(f"{int(x):x}" for x in w.view(np.uint32)) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return np.array([[int(x, 16) for x in ln.split()] for ln in out.stdout.splitlines()], np.uint32).reshape(len(lines), 2 * SIDE)


def check(exe, lines, tmp_path):
    """geo and flat agree in every word the flat driver's contract specifies; returns the geo records"""
    got = run(exe, lines, tmp_path)
    geo, flat = got[:, :SIDE], got[:, SIDE:]
    for row, (count, has_b, warm, w) in enumerate(lines):
        what = (row, count, has_b, warm)
        assert np.array_equal(geo[row, :12], flat[row, :12]), ("row masses", what)
        g, f = geo[row, 12:].reshape(1 + SWEEPS, 24), flat[row, 12:].reshape(1 + SWEEPS, 24)
        assert np.array_equal(g[:, 0:6], f[:, 0:6]), ("vA, wA", what)
        assert np.array_equal(g[:, 12:24], f[:, 12:24]), ("impulses", what)
        if has_b:
            assert np.array_equal(g[:, 6:12], f[:, 6:12]), ("vB, wB", what)
        else:  # the spec's driver leaves the velocities of a body that is not there alone
            assert np.array_equal(g[:, 6:12], np.tile(w.view(np.uint32)[51:57], (1 + SWEEPS, 1))), ("geo touched vB, wB", what)
        # masses of the points that exist were made (> 0: positive definite tensors), the others stay zero
        m = geo[row, :12].view(F).reshape(4, 3)
        assert (m[:count] > 0).all() and not m[count:].any(), what
    return geo


def _bias(depth):
    """contact_bias for dt = 1/60, baumgarte 0.2, slop 0.01, max_bias 3 (the KAT's parameters)"""
    dt, slop = F(0.016666668), F(0.01)
    if depth > slop:
        return min((F(0.2) / dt) * (F(depth) - slop), F(3.0))
    return F(depth) / dt if depth < 0 else F(0.0)


def random_manifolds(seed, trials):
    """drawn as tests/test_collide_kat.py draws its manifolds for the three older drivers"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(trials):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        count = int(rng.integers(1, 5))
        has_b = int(rng.integers(0, 2))
        pts = rng.uniform(-1, 1, (4, 3))
        depth = rng.uniform(-0.02, 0.05, 4)
        xB = rng.uniform(-2, 2, 3)
        xA = np.array([0.25 * xB[1], -0.5 * xB[2], 0.125 * xB[0]])
        im = rng.uniform(0.3, 2.0, 2)
        a = rng.normal(scale=0.3, size=(2, 3, 3))
        inertia = [np.eye(3) * rng.uniform(0.5, 2.0) + m @ m.T for m in a]
        vel = rng.normal(scale=2.0, size=12)
        friction = rng.uniform(0.0, 1.0)
        pn = rng.uniform(0.05, 2.0, 4)  # starting impulses of a warm solve: normal >= 0, friction inside or outside its box
        pt = rng.normal(scale=0.5, size=8)
        out.append(manifold(count, has_b, n, pts, [_bias(d) for d in depth], xA, im[0], inertia[0], xB, im[1], inertia[1], vel,
                            friction, np.concatenate([pn, pt])))
    return out


def test_flat_driver_equals_geo_on_300_random_manifolds(exe, tmp_path):
    ms = random_manifolds(5, 300)
    assert {(c, b) for _, c, b in ms} == set(itertools.product((1, 2, 3, 4), (0, 1)))  # every count with and without a body B
    lines = [ln for m in ms for ln in lines_of(m)]
    geo = check(exe, lines, tmp_path)
    # the solves did something: a warm first sweep always moves body A (non-zero impulses), most cold ones do (a pair that
    # separates with nothing to push out gets no impulse), and the warm solves differ from the cold ones
    moved = np.array([not np.array_equal(geo[row, 12:18], w.view(np.uint32)[45:51]) for row, (_, _, _, w) in enumerate(lines)])
    assert moved[1::2].all() and moved[0::2].mean() > 0.5
    cold, warm = geo[0::2], geo[1::2]
    assert (cold[:, 12:] != warm[:, 12:]).any(axis=1).all()


def test_flat_driver_keeps_the_sign_of_zero(exe, tmp_path):
    """Where a zero's sign could tell the two apart: axis-aligned normals of either sign (tangents with +-0 components,
    negative direction components), contact points on the lattice (lever arms and cross products with exact zeros), bodies at
    rest (every relative velocity a signed zero in the first sweep) and moving along one axis, with and without a body B,
    every count, the caller's zeros against the spec's ignored garbage."""
    rng = np.random.default_rng(17)
    axes = [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    rest = np.zeros(12)
    ms = []
    for n, count, has_b in itertools.product(axes, (1, 2, 3, 4), (0, 1)):
        for vel in (rest, -rest, np.concatenate([-n, np.zeros(3), n, np.zeros(3)]), np.concatenate([np.zeros(3), -n, np.zeros(3), n])):
            pts = rng.integers(-2, 3, (4, 3)) * 0.5
            xA = rng.integers(-1, 2, 3) * 0.5
            xB = rng.integers(-1, 2, 3) * 1.0
            bias = rng.choice([0.0, 0.0, 0.25, -0.5], 4)
            IA, IB = np.eye(3) * 0.5, np.eye(3) * 2.0
            IA[0, 1] = IA[1, 0] = 0.125  # the full-tensor pass takes the general product; lines_of strips it for the diagonal pass
            IB[1, 2] = IB[2, 1] = -0.25
            imp = np.concatenate([rng.choice([0.0, 0.5, 1.0], 4), rng.choice([0.0, -0.25, 0.25], 8)])
            ms.append(manifold(count, has_b, n, pts, bias, xA, 1.0, IA, xB, 0.5, IB, vel, 0.5, imp))
    geo = check(exe, [ln for m in ms for ln in lines_of(m)], tmp_path)
    # the cases do hold signed zeros: both signs of zero among the velocities the spec's driver returns for body A
    va = geo[:, 12:].reshape(len(geo), 1 + SWEEPS, 24)[:, :, 0:6]
    assert (va == 0x80000000).any() and (va == 0).any()
