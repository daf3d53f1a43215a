"""CPU: depenetration's rule (include/spec/depenetrate.h, compiled alone by the host compiler: tests/cpp/depen_probe.cpp) against
the float64 statement of tests/depen_ref.py.

1. the probe builds plain and under the address and undefined-behaviour sanitizers, and both give the same words;
2. every branch of the loop, on closed-form target lists: the branch the reference takes, positions within tolerance;
3. depth and normal of the probe against float64 on the seeded capsules of tests/depen_cases.py where the core lies outside
   the target; properties where it enters a box;
4. the seeded sets: the reference's own near ties stay under 1 %, and the push counts fill the bins the GPU test needs.

Tolerances. One probe: capsulecast_accept.tol_of for a query that does not move, tol = 1e-5 (1 + |pos|_inf + h);
measured worst deviation of collide.h's depths from the reference over the seeded sets, core outside the target: 0.007 tol. A whole
loop of up to 8 pushes (a crease multiplies an error at every push): measured worst 2.35 tol, bound LOOP_TOL = 10 tol (4 x, rounded up).
A core inside a box: the overlap one push n d leaves to that box (collide_capsule_box prefers a face within a band of 5 % + 0.01 and
clips the core to the face before it measures): measured worst 28.3 tol (0.0028), bound BOX_TOL = 120 tol (4 x, rounded up), for that
one-push property alone; the depth never exceeded the least face exit by more than 0.005 tol, bound 1 tol. The final separation of a
loop that ends clear (the core is then outside every target): never below skin / 2 (least 0.010136 and 0.010383), bound skin / 2 - tol."""
import math

import numpy as np
import pytest

import depen_cases as cases
import depen_probe as probe
import depen_ref as ref
from capsulecast_ref import query_ref

F = np.float32
MISS, GROUND, STATIC = probe.MISS, probe.GROUND, 0x80000000
STUCK, INVALID = probe.STUCK, probe.INVALID
SKIN = F(cases.SKIN)
LOOP_TOL = 10.0
BOX_TOL = 120.0
BOX, SPHERE, CAPSULE = 2, 1, 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("depen") / "depen_probe"))


def _statics(shape, pos, he, rot=None):
    m = len(shape)
    rot = np.tile([0.0, 0.0, 0.0, 1.0], (m, 1)) if rot is None else rot
    return query_ref.targets(None, dict(pos=np.asarray(pos, F), rot=np.asarray(rot, F), shape=np.asarray(shape, np.uint32),
                                        half_extent=np.asarray(he, F)))


def _rot_z(deg):
    t = math.radians(deg) / 2
    return [0.0, 0.0, math.sin(t), math.cos(t)]


FLOOR = ([0.0, -0.5, 0.0], [10.0, 0.5, 10.0])
WALL = ([-0.5, 5.0, 0.0], [0.5, 5.0, 10.0])


def _both(exe, pos, R, h, tg, ground, skin, max_iters, rot=None):
    """(the probe's loop, the reference's loop) for one query"""
    got = probe.run(exe, np.asarray([pos], F), None if rot is None else np.asarray([rot], F), F(R), F(h), skin, max_iters,
                    cases.probe_targets(tg), ground)
    want = ref.depenetrate(np.asarray(pos, F).astype(np.float64), ref.axis(None if rot is None else np.asarray(rot, F)), float(F(R)), float(F(h)),
                           tg, ground, float(skin), max_iters)
    return got, want


def _agree(got, want, pos, h, what):
    p, status, body, nrm, dep = got
    tol = LOOP_TOL * cases.tol_of(np.asarray(pos), h)
    assert int(status[0]) == want[1], (what, hex(int(status[0])), hex(want[1]))
    assert np.abs(p[0] - want[0]).max() <= tol, (what, p[0], want[0])
    k = want[1] & 0xF
    assert [int(b) for b in body[:k, 0]] == [s[0] for s in want[2]], what
    for j, (_, n, d, _) in enumerate(want[2]):
        assert np.abs(nrm[j, 0] - n).max() <= 1e-4 and abs(dep[j, 0] - d) <= tol, (what, j)
    assert (body[k:, 0] == MISS).all() and not nrm[k:].any() and not dep[k:].any(), what


# ---- 1. the probe under the sanitizers ------------------------------------------------------------------------------------------
def test_probe_under_sanitizers_gives_the_same_words(exe, tmp_path):
    san = probe.build(str(tmp_path / "depen_probe_san"), sanitize=True)
    c = cases.case("soup")
    k = slice(0, 200)
    pt = cases.probe_targets(c["tg"])
    for mi in (1, 8):
        a = probe.run(exe, c["pos"][k], c["rot"][k], c["rad"][k], c["hq"][k], SKIN, mi, pt, c["ground"])
        b = probe.run(san, c["pos"][k], c["rot"][k], c["rad"][k], c["hq"][k], SKIN, mi, pt, c["ground"])
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    bad = np.array([[np.nan, 0, 0], [0, 0, 0]], F)
    assert list(probe.valid(san, bad, None, F(0.1), F(0.1))) == [False, True]


# ---- 2. the loop's branches -----------------------------------------------------------------------------------------------------
def test_clear_at_once_and_a_miss(exe):
    tg = _statics([BOX], [FLOOR[0]], [FLOOR[1]])
    # skin clear of the floor: within the gap, not within skin / 2
    got, want = _both(exe, [0, 0.3 + 0.8 * float(SKIN), 0], 0.3, 0.0, tg, None, SKIN, 4)
    _agree(got, want, [0, 0.32, 0], 0.0, "clear")
    assert got[1][0] == 0 and np.array_equal(got[0][0], np.array([0, 0.3 + 0.8 * float(SKIN), 0], F))
    # nothing within the gap at all
    got, want = _both(exe, [0, 5, 0], 0.3, 0.5, tg, None, SKIN, 4)
    _agree(got, want, [0, 5, 0], 0.5, "miss")
    assert got[1][0] == 0
    b, d, n = probe.deepest(exe, np.array([[0, 5, 0]], F), None, F(0.3), F(0.5), SKIN, cases.probe_targets(tg), None)
    assert b[0] == MISS and d[0] == -np.inf and not n.any()
    # no targets, no ground
    got = probe.run(exe, np.array([[0, 0, 0]], F), None, F(0.3), F(0.5), SKIN, 8, None, None)
    assert got[1][0] == 0 and (got[2] == MISS).all()


def test_one_push_out_of_the_ground(exe):
    got, want = _both(exe, [1, 0.7, 2], 0.3, 0.5, _statics([], np.zeros((0, 3)), np.zeros((0, 3))), 0.0, SKIN, 4)
    _agree(got, want, [1, 0.7, 2], 0.5, "ground")
    assert got[1][0] == 1 and got[2][0, 0] == GROUND and np.array_equal(got[3][0, 0], [0, 1, 0])
    assert abs(got[4][0, 0] - 0.1) < 1e-6 and abs(got[0][0, 1] - (0.7 + 0.1 + float(SKIN))) < 1e-6


def test_two_perpendicular_planes_take_two_pushes(exe):
    tg = _statics([BOX, BOX], [FLOOR[0], WALL[0]], [FLOOR[1], WALL[1]])
    got, want = _both(exe, [0.2, 0.25, 0], 0.3, 0.0, tg, None, SKIN, 4)
    _agree(got, want, [0.2, 0.25, 0], 0.0, "corner")
    assert got[1][0] == 2 and list(got[2][:2, 0]) == [STATIC | 1, STATIC | 0]  # the wall is deeper: first


def test_an_exact_tie_goes_to_the_smaller_id(exe):
    # two equal statics at one place, their top in the ground plane: three targets at the same depth, in either list order
    tg = _statics([BOX, BOX], [FLOOR[0], FLOOR[0]], [FLOOR[1], FLOOR[1]])
    pt = cases.probe_targets(tg)
    back = {k: v[::-1].copy() for k, v in pt.items()}
    for lst in (pt, back):
        b, d, n = probe.deepest(exe, np.array([[0.0, 0.25, 0.0]], F), None, F(0.5), F(0.0), F(0.0), lst, 0.0)
        assert b[0] == STATIC | 0 and d[0] == F(0.25) and np.array_equal(n[0], [0, 1, 0])
    b, _, _ = probe.deepest(exe, np.array([[0.0, 0.25, 0.0]], F), None, F(0.5), F(0.0), F(0.0), {k: v[1:] for k, v in pt.items()}, 0.0)
    assert b[0] == STATIC | 1  # the ground, at the same depth to the bit, loses the tie with any static
    b, d, _ = probe.deepest(exe, np.array([[0.0, 0.25, 0.0]], F), None, F(0.5), F(0.0), F(0.0), None, 0.0)
    assert b[0] == GROUND and d[0] == F(0.25)
    assert ref.deepest([0.0, 0.25, 0.0], [0, 1, 0], 0.5, 0.0, tg, 0.0, 0.0)[0] == STATIC | 0


def _crease():
    # the floor and a ceiling that slopes up at 60 degrees from the line x = y = 0: their normals make 120 degrees, a push out of
    # one drives the ball half as deep into the other
    n2 = np.array([math.sin(math.radians(60)), -math.cos(math.radians(60)), 0.0])
    t = np.array([math.cos(math.radians(60)), math.sin(math.radians(60)), 0.0])
    centre = -0.5 * n2 + 4.0 * t
    rot = np.array([[0, 0, 0, 1], _rot_z(60)], F)
    tg = _statics([BOX, BOX], [FLOOR[0], centre], [FLOOR[1], [5.0, 0.5, 5.0]], rot)
    y = 0.2
    x = (0.29 + 0.5 * y) / n2[0]
    return tg, [x, y, 0.0]


def test_an_acute_crease_converges_and_is_stuck_with_too_few_rounds(exe):
    tg, pos = _crease()
    got, want = _both(exe, pos, 0.3, 0.0, tg, None, SKIN, 8)
    _agree(got, want, pos, 0.0, "crease")
    assert 3 <= (got[1][0] & 0xF) <= 8 and not got[1][0] & STUCK
    sep = ref.separation(got[0][0].astype(np.float64), ref.axis(None), 0.3, 0.0, tg, None)
    assert sep >= 0.5 * float(SKIN) - 1e-5
    got, want = _both(exe, pos, 0.3, 0.0, tg, None, SKIN, 2)
    _agree(got, want, pos, 0.0, "crease, 2 rounds")
    assert got[1][0] == (2 | STUCK)


def test_a_sandwich_ends_stuck_and_finite(exe):
    tg = _statics([BOX, BOX], [FLOOR[0], [0, 1.0, 0]], [FLOOR[1], [10, 0.5, 10]])  # a slot 0.5 high, a ball of 0.6
    for mi in (1, 4, 8):
        got, want = _both(exe, [0, 0.26, 0], 0.3, 0.0, tg, None, SKIN, mi)
        _agree(got, want, [0, 0.26, 0], 0.0, f"sandwich {mi}")
        assert got[1][0] == (mi | STUCK) and np.isfinite(got[0]).all()


def test_skin_zero_acts_on_penetration_alone(exe):
    tg = _statics([SPHERE], [[0, 0, 0]], [[1.0, 0, 0]])
    got, want = _both(exe, [0, 1.2, 0], 0.3, 0.0, tg, None, F(0.0), 4)  # 0.1 deep: pushed to touching, then touching or STUCK
    assert (got[1][0] & 0xF) >= 1 and abs(got[0][0, 1] - 1.3) < 1e-5
    assert got[4][0, 0] == pytest.approx(0.1, abs=1e-6) and want[1] & 0xF >= 1
    got, _ = _both(exe, [0, 1.3 + 1e-4, 0], 0.3, 0.0, tg, None, F(0.0), 4)  # apart: nothing within a gap of 0
    assert got[1][0] == 0


def test_depth_exactly_at_half_a_skin(exe):
    skin = F(0.02)
    edge = F(-0.5) * skin
    d = np.array([edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(-1))], F)
    p = np.zeros((3, 3), F)
    n = np.tile(np.array([0, 1, 0], F), (3, 1))
    p2, status, go = probe.step(exe, p, np.zeros(3, np.uint32), 0, 4, skin, np.array([7, 7, 7], np.uint32), d, n)
    assert list(go) == [False, True, False] and list(status) == [0, 1, 0]
    assert p2[1, 1] == F(d[1] + skin) and not p2[0].any() and not p2[2].any()
    # round max_iters: no push is left: STUCK, the position stays
    p2, status, go = probe.step(exe, p, np.full(3, 4, np.uint32), 4, 4, skin, np.array([7, 7, 7], np.uint32), np.full(3, 0.1, F), n)
    assert not go.any() and (status == (4 | STUCK)).all() and not p2.any()
    # a miss ends the loop whatever its depth field holds
    _, status, go = probe.step(exe, p, np.zeros(3, np.uint32), 0, 4, skin, np.full(3, MISS, np.uint32), np.full(3, 1.0, F), n)
    assert not go.any() and not status.any()


def test_every_invalid_kind(exe):
    ok = dict(pos=[0, 0.1, 0], rot=[0, 0, 0, 1], R=0.3, h=0.5)
    kinds = [dict(pos=[np.nan, 0, 0]), dict(pos=[0, np.inf, 0]), dict(pos=[0, 0, -np.inf]), dict(rot=[np.nan, 0, 0, 1]), dict(rot=[0, 0, 0, np.inf]),
             dict(R=np.nan), dict(R=np.inf), dict(R=-0.1), dict(h=np.nan), dict(h=np.inf), dict(h=-0.1), dict(h=3.402e38)]
    fine = [dict(), dict(R=0.0), dict(h=0.0), dict(h=3.4e38), dict(rot=[0, 0, 0, 0]), dict(rot=[0.3, 0.1, 2.0, 0.5])]
    for kind, expect in [(k, False) for k in kinds] + [(k, True) for k in fine]:
        q = dict(ok, **kind)
        with np.errstate(all="ignore"):
            v = probe.valid(exe, np.array([q["pos"]], F), np.array([q["rot"]], F), F(q["R"]), F(q["h"]))[0]
            assert v == expect == ref.valid(np.array(q["pos"], F), np.array(q["rot"], F), F(q["R"]), F(q["h"])), kind
            if "h" in kind and expect:
                continue  # (a half-length of 3.4e38 is valid and reaches everything; its arithmetic is not the loop's business here)
            got = probe.run(exe, np.array([q["pos"]], F), np.array([q["rot"]], F), F(q["R"]), F(q["h"]), SKIN, 4, None, 0.0)
        if not expect:
            assert got[1][0] == INVALID and np.array_equal(got[0].view(np.uint32), np.array([q["pos"]], F).view(np.uint32))
            assert (got[2] == MISS).all() and not got[3].any() and not got[4].any()
    # a NaN rot does not matter without a rot
    assert probe.valid(exe, np.array([[0, 0, 0]], F), None, F(0.3), F(0.5))[0]


# ---- 3. depth and normal against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "statics"])
def test_depth_and_normal_against_float64(name, exe):
    c = cases.case(name)
    n = len(c["pos"])
    b, d, nrm = probe.deepest(exe, c["pos"], c["rot"], c["rad"], c["hq"], SKIN, cases.probe_targets(c["tg"]), c["ground"])
    tol = np.array([cases.tol_of(c["pos"][i], c["hq"][i]) for i in range(n)])
    worst, compared, entered, left, over, turn = 0.0, 0, 0, -np.inf, -np.inf, 0.0
    for i in range(n):
        rid, rd, rn, rd2, inside = c["first"][i]
        if not inside:
            # the core lies outside every near target: depth = R + r_T - dist, the normal along the closest points
            near_tie = math.isfinite(rd2) and rd - rd2 < tol[i]
            assert near_tie or b[i] == rid, (i, hex(int(b[i])), hex(rid))
            if b[i] != rid or rid == MISS:
                continue
            compared += 1
            worst = max(worst, abs(d[i] - rd) / tol[i])
            assert abs(d[i] - rd) <= tol[i], (i, d[i], rd)
            shape = c["tg"]["shape"][c["tg"]["id"] == rid]
            if rid == GROUND:
                assert np.array_equal(nrm[i], [0, 1, 0])
            elif shape[0] != BOX:
                # the direction of two points each off by tol, `dist` apart
                dist = float(c["rad"][i]) + float(c["tg"]["half_extent"][c["tg"]["id"] == rid][0, 0]) - rd
                turn = max(turn, np.abs(nrm[i] - rn).max() * dist / tol[i])
                assert np.abs(nrm[i] - rn).max() <= 1e-6 + 2.0 * tol[i] / dist, (i, nrm[i], rn, dist)
            continue
        k = np.nonzero(c["tg"]["id"] == b[i])[0]
        if len(k) == 0 or c["tg"]["shape"][k[0]] != BOX:
            continue
        # the core enters a box: the push n d leaves the box, and d is no more than the least face exit
        entered += 1
        one = {key: v[k] for key, v in c["tg"].items()}
        p, a, R, h = c["pos"][i].astype(np.float64), c["a"][i], float(c["rad"][i]), float(c["hq"][i])
        _, dep0, _, ins0 = ref.depths(p, a, R, h, one, None)
        _, dep1, _, _ = ref.depths(p + nrm[i].astype(np.float64) * float(d[i]), a, R, h, one, None)
        left = max(left, dep1[0] / tol[i])
        assert -dep1[0] >= -BOX_TOL * tol[i], (i, dep1[0], tol[i])
        if ins0[0]:
            most = ref.face_exit(p, a, R, h, one["pos"][0], c["frames"][k[0]], one["half_extent"][0])
            over = max(over, (d[i] - most) / tol[i])
            assert d[i] <= most + tol[i], (i, d[i], most)
    print(name, "compared", compared, "worst deviation / tol", worst, "core inside a box", entered, "overlap left / tol", left,
          "depth over the least face exit / tol", over, "normal deviation x dist / tol", turn)
    assert compared > 200 and entered > 50


# ---- 4. the seeded sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.SCENES)
def test_seeded_sets_near_ties_and_loops(name, exe):
    c = cases.case(name)
    n = len(c["pos"])
    ties = cases.near_ties(c)
    print(name, "near ties of the reference", ties, "of", n)
    assert ties <= n // 100
    got = probe.run(exe, c["pos"], c["rot"], c["rad"], c["hq"], SKIN, cases.MAX_ITERS, cases.probe_targets(c["tg"]), c["ground"])
    want_status = np.array([o[1] for o in c["out"]], np.uint32)
    plain = np.array([not any(s[3] for s in o[2]) and not c["first"][i][4] for i, o in enumerate(c["out"])])
    tol = np.array([LOOP_TOL * cases.tol_of(c["pos"][i], c["hq"][i]) for i in range(n)])
    dev = np.abs(got[0] - np.array([o[0] for o in c["out"]])).max(1)
    print(name, "loops compared", int(plain.sum()), "worst position deviation / (tol_of)", float((dev / tol * LOOP_TOL)[plain].max()))
    assert np.array_equal(got[1][plain], want_status[plain])
    assert (dev[plain] <= tol[plain]).all()
    # every loop that ends clear is skin / 2 - tol from every reference target (measured: none below skin / 2, least 0.010136)
    least = np.inf
    for i in np.nonzero((got[1] & (STUCK | INVALID)) == 0)[0]:
        sub = {k: v[c["near"][i]] for k, v in c["tg"].items()}
        sep = ref.separation(got[0][i].astype(np.float64), c["a"][i], float(c["rad"][i]), float(c["hq"][i]), sub, c["ground"], c["frames"][c["near"][i]])
        least = min(least, sep)
        assert sep >= 0.5 * float(SKIN) - tol[i] / LOOP_TOL, (i, sep)
    print(name, "least final separation", least)
    for mi in (1, 4, 8):
        st = probe.run(exe, c["pos"], c["rot"], c["rad"], c["hq"], SKIN, mi, cases.probe_targets(c["tg"]), c["ground"])[1]
        pushes, stuck = np.bincount(st & 0xF, minlength=9), int((st & STUCK != 0).sum())
        print(name, "max_iters", mi, "pushes", pushes, "stuck", stuck)
        if name != "empty" and mi == 4:
            assert pushes[0] >= n // 10 and pushes[2:].sum() >= n // 10 and stuck >= 5
        if name == "empty":
            assert not st.any()
