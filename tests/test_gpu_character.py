"""GPU: character walking (phys_character_move and its device variant) on the seeded scenes of tests/character_cases.py.

1. one launch equals the loop: a host loop that drives the spec header's ch_next / ch_answer (tests/character_probe.py) with
   World.capsulecast as the cast, every output bit for bit, over the slide scenes and the terrain, three slide counts, four
   query counts, filters, ignore, upright, the device variant and reversed order;
2. with grounded_in NULL it is move-and-slide bit for bit;
3. float64 properties that share no code with the kernels or the spec header (tests/capsulecast_ref.py, tests/character_ref.py);
4. closed forms: level ground, risers, ramps, ledges, ceilings, an overlapping start;
5. refusals, n = 0, NULL outputs and INVALID queries;
6. no side effects on the updates, and the poses of phys_set_body_poses are seen."""
import math

import numpy as np
import pytest

import capsulecast_ref as ccref
import character_cases as cases
import character_probe as probe
import slide_cases
from capsulecast_accept import tol_of

pytestmark = pytest.mark.gpu

F = np.float32
MISS, GROUND = 0xFFFFFFFE, 0xFFFFFFFF
BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
GROUNDED, STEPPED, SNAPPED, ON_STEEP, HIT_WALL, HIT_CEILING = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000, 0x20000
SKIN = F(cases.SKIN)
IDENT = [0.0, 0.0, 0.0, 1.0]
BOX = 2
ST0 = 0x80000000
NAMES = ("pos", "remaining", "status", "floor_body", "floor_normal", "floor_point", "hit_body", "hit_normal", "hit_point")


def _pa():
    import physics_amd
    return physics_amd


def _world(bodies=None, statics=None, ground=0.0):
    pa = _pa()
    flags = pa.FLAG_COLLISIONS | (pa.FLAG_GROUND_PLANE if ground is not None else 0)
    w = pa.World(pa.default_config(flags=flags, gravity_offset=(0.0, 0.0, 0.0), ground_height=0.0 if ground is None else ground))
    if bodies is not None:
        w.set_bodies(np.asarray(bodies["pos"], F), rot=np.asarray(bodies["rot"], F), shape_type=np.asarray(bodies["shape"], np.uint32),
                     half_extent=np.asarray(bodies["half_extent"], F))
    if statics is not None:
        w.set_static_bodies(np.asarray(statics["pos"], F), rot=np.asarray(statics["rot"], F), shape_type=np.asarray(statics["shape"], np.uint32),
                            half_extent=np.asarray(statics["half_extent"], F))
    return w


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        diff = np.nonzero(_bits(x).reshape(-1) != _bits(y).reshape(-1))[0]
        assert len(diff) == 0, (what, name, len(diff), diff[:6], x.reshape(-1)[diff[:6]], y.reshape(-1)[diff[:6]])


def _rows(out, r, n):
    """the outputs of a call with their query axis indexed by r"""
    return tuple(x[r] if x.ndim < 2 or x.shape[0] == n else x[:, r] for x in out)


def _counts(status):
    return {k: int((status & b != 0).sum()) for k, b in (("stepped", STEPPED), ("snapped", SNAPPED), ("grounded", GROUNDED), ("on steep", ON_STEEP),
                                                         ("wall", HIT_WALL), ("ceiling", HIT_CEILING), ("blocked", BLOCKED), ("exhausted", EXHAUSTED))}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("character") / "character_probe"))


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _world(*cases.scene(name))
        return made[name]

    yield get
    for w in made.values():
        w.close()


def _call(w, c, k=slice(None), max_slides=cases.MAX_SLIDES, rot=True, grounded=True, ignore=None, mask=None):
    sub = lambda a: None if a is None else np.ascontiguousarray(a[k])
    skin, _, step, snap, ny = cases.params()
    return w.character_move(sub(c["pos"]), sub(c["motion"]), sub(c["rad"]), sub(c["hq"]), rot=sub(c["rot"]) if rot else None,
                            grounded=sub(c["grounded"]) if grounded else None, skin=skin, max_slides=max_slides, step_height=step,
                            snap_distance=snap, min_floor_ny=ny, ignore=sub(ignore), mask=mask if mask is None or np.ndim(mask) == 0 else sub(mask))


def _loop(exe, w, c, k=slice(None), max_slides=cases.MAX_SLIDES, rot=True, ignore=None, mask=None):
    """(one launch, the host loop of casts) for rows k of case c"""
    sub = lambda a: None if a is None else np.ascontiguousarray(a[k])
    skin, _, step, snap, ny = cases.params()
    got = _call(w, c, k, max_slides, rot=rot, ignore=ignore, mask=mask)

    def cast(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        return w.capsulecast(origins, dirs, radius, half_length, rot=rot, max_t=max_t, ignore=ignore, mask=mask)

    want = probe.host_loop(exe, cast, sub(c["pos"]), sub(c["motion"]), sub(c["rad"]), sub(c["hq"]), sub(c["rot"]) if rot else None, sub(c["grounded"]),
                           skin, max_slides, step, snap, ny, ignore=sub(ignore), mask=mask if mask is None or np.ndim(mask) == 0 else sub(mask))
    return got, want


# ---- 1. one launch equals the loop, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_slides", [1, 4, 8])
@pytest.mark.parametrize("name", cases.SCENES)
def test_one_launch_equals_the_loop_of_casts(name, max_slides, exe, worlds):
    c = cases.case(name)
    got, want = _loop(exe, worlds(name), c, max_slides=max_slides)
    _same(got, want, f"{name} max_slides {max_slides}")
    status = got[2]
    n = len(status)
    found = _counts(status)
    print(name, max_slides, found)
    assert got[6].shape == (2 * max_slides, n) and got[7].shape == (2 * max_slides, n, 3)
    assert not (status & INVALID).any()
    # every slot: used below its slide's hit count, empty from there on
    for first, hits in ((0, status & 0xF), (max_slides, (status >> 4) & 0xF)):
        used = np.arange(max_slides)[:, None] < hits[None, :]
        part = slice(first, first + max_slides)
        assert ((got[6][part] != MISS) == used).all() and not got[7][part][~used].any() and not got[8][part][~used].any()
    # the floor outputs go with GROUNDED / ON_STEEP
    has_floor = (status & (GROUNDED | ON_STEEP)) != 0
    assert ((got[3] != MISS) == has_floor).all() and not got[4][~has_floor].any()
    assert not ((status & GROUNDED != 0) & (status & ON_STEEP != 0)).any() and not (status & BLOCKED != 0)[has_floor].any()
    assert ((status & SNAPPED == 0) | (status & GROUNDED != 0)).all() and ((status & STEPPED == 0) | (status & GROUNDED != 0)).all()
    if name == "terrain":
        # a phase nobody reaches is untested
        for what in ("stepped", "snapped", "grounded", "on steep", "wall", "ceiling"):
            assert found[what] >= 3, (what, found)
    if name == "empty":
        assert not status.any() and np.array_equal(got[0], c["pos"] + c["motion"])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_query_counts_around_the_workgroup_size(n, exe, worlds):
    c = cases.case("terrain")
    got, want = _loop(exe, worlds("terrain"), c, slice(100, 100 + n))
    _same(got, want, f"n = {n}")
    assert n == 1 or (got[2] & STEPPED).any()


def test_filters_ignore_and_upright(exe):
    c = cases.case("soup")
    cat, scat, gcat, masks, ignore = slide_cases.filters()
    w = _world(*cases.scene("soup"))
    got, want = _loop(exe, w, c, ignore=ignore)
    _same(got, want, "ignore")
    given = ignore != MISS + 1
    assert given.sum() > 100 and (got[6][:, given] != ignore[given][None, :]).all()
    plain = _call(w, c)
    assert (plain[6][0][given] == ignore[given]).sum() > 50
    got, want = _loop(exe, w, c, rot=False)
    _same(got, want, "upright")
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(gcat, 0xFFFF)
    got, want = _loop(exe, w, c, mask=masks)
    _same(got, want, "masks")
    for b in list(got[6]) + [got[3]]:
        dyn = b < 300
        assert ((cat[b[dyn]] & masks[dyn]) != 0).all()
        st = (b >= ST0) & (b < MISS)
        assert ((scat[b[st] - ST0] & masks[st]) != 0).all()
        assert ((masks[b == GROUND] & gcat) != 0).all()
    _same(_call(w, c, mask=0xFFFF), plain, "mask 0xFFFF")
    none = _call(w, c, mask=0)
    assert not none[2].any() and np.array_equal(none[0], c["pos"] + c["motion"])
    w.close()


def test_device_variant_and_reversed_order(worlds):
    import torch
    c = cases.case("terrain")
    w = worlds("terrain")
    n, k = len(c["pos"]), cases.MAX_SLIDES
    skin, _, step, snap, ny = cases.params()
    host = _call(w, c)
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()
    f3 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    i1 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device="cuda")
    tp, tr, ts, tfb, tfn, tfp, tb, tn, tq = f3(n, 3), f3(n, 3), i1(n), i1(n), f3(n, 3), f3(n, 3), i1(2 * k, n), f3(2 * k, n, 3), f3(2 * k, n, 3)
    torch.cuda.synchronize()
    common = dict(rot=dev(c["rot"]), grounded=dev(c["grounded"].view(np.int32)), skin=skin, max_slides=k, step_height=step, snap_distance=snap,
                  min_floor_ny=ny)
    w.character_move_device(dev(c["pos"]), dev(c["motion"]), dev(c["rad"]), dev(c["hq"]), tp, ts, tr, tfb, tfn, tfp, tb, tn, tq, **common)
    w.sync()
    _same(host, tuple(x.cpu().numpy() for x in (tp, tr, ts, tfb, tfn, tfp, tb, tn, tq)), "device")
    # with a mask of all ones and without the optional outputs
    tp2, ts2 = torch.empty_like(tp), torch.empty_like(ts)
    w.character_move_device(dev(c["pos"]), dev(c["motion"]), dev(c["rad"]), dev(c["hq"]), tp2, ts2, mask=dev(np.full(n, -1, np.int16)), **common)
    w.sync()
    assert torch.equal(tp, tp2) and torch.equal(ts, ts2)
    r = slice(None, None, -1)
    rev = _call(w, {key: (v[r] if isinstance(v, np.ndarray) and key in ("pos", "motion", "rot", "rad", "hq", "grounded") else v) for key, v in c.items()})
    _same(host, _rows(rev, r, n), "reversed")


# ---- 2. it is move-and-slide where it should be ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", slide_cases.SCENES)
def test_without_grounded_in_it_is_move_and_slide(name, worlds):
    c = cases.case(name)
    w = worlds(name)
    k = cases.MAX_SLIDES
    got = _call(w, c, grounded=False)
    want = w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=cases.params()[0], max_slides=k)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[2] & 0x70F, want[2])
    for a, b in ((got[6], want[3]), (got[7], want[4]), (got[8], want[5])):
        assert np.array_equal(_bits(a[:k]), _bits(b))
        assert (a[k:] == MISS).all() if a.dtype == np.uint32 else not a[k:].any()
    assert not (got[2] & (STEPPED | SNAPPED)).any()


# ---- 3. float64 properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["terrain", "statics"])
def test_float64_properties(name, worlds):
    c = cases.case(name)
    n = len(c["pos"])
    pos_out, rem, status, fbody, fnrm, fpnt, body, nrm, pnt = _call(worlds(name), c)
    skin, _, step, snap, ny = cases.params()
    # what lies below where each character ends, in float64: the tolerances are this cast's
    down = np.tile([0.0, -1.0, 0.0], (n, 1))
    h = ccref.capsulecast(pos_out, down, c["rot"], c["rad"], c["hq"], c["tg"], ground=c["ground"])
    tol = np.array([tol_of(h, i, 0.0) + 1e-5 * float(np.linalg.norm(c["motion"][i])) for i in range(n)])
    sep = slide_cases.separation(pos_out, c["rot"], c["rad"], c["hq"], c["tg"], c["ground"])
    print(name, "least separation", sep.min(), _counts(status))
    assert (sep >= -tol).all(), np.nonzero(sep < -tol)[0][:8]
    grounded = np.nonzero(status & GROUNDED)[0]
    assert len(grounded) > (n // 2 if name == "terrain" else 20)  # (the statics scene's characters fly: a third aim at the ground)
    bad = []
    for i in grounded:
        ok = h["t"][i] <= 2 * skin + tol[i] and h["normal"][i][1] >= ny - 1e-4
        named = int(fbody[i]) == int(h["body"][i]) or (math.isfinite(h["t2"][i]) and h["t2"][i] - h["t"][i] <= 4 * tol[i])
        if not (ok and named):
            bad.append((int(i), float(h["t"][i]), h["normal"][i], int(fbody[i]), int(h["body"][i])))
    assert not bad, bad[:4]
    # the branch flags are the float64 walk's, but for the near ties the CPU audit counted
    walks, tie = cases.reference(name)
    want = np.array([w["status"] for w in walks], np.uint32)
    flags = GROUNDED | STEPPED | SNAPPED | ON_STEEP | HIT_WALL | HIT_CEILING | BLOCKED
    differ = (status & flags) != (want & flags)
    print(name, "flags differ", int(differ.sum()), "of which near ties", int((differ & tie).sum()), "near ties", int(tie.sum()), "cap", cases.tie_cap(n))
    assert not (differ & ~tie).any(), [(int(i), hex(status[i]), hex(want[i]), walks[i]["branch"]) for i in np.nonzero(differ & ~tie)[0][:6]]
    assert int(tie.sum()) <= cases.tie_cap(n)
    # where the float64 walk met the same targets in the same order, it ends where the kernel's did: every cast adds at most its
    # own acceptance (4 tol: capsulecast_accept) to the difference
    k = cases.MAX_SLIDES
    far = []
    for i in np.nonzero(~differ & ~tie)[0]:
        ids = [int(b) for b in body[:k, i] if b != MISS], [int(b) for b in body[k:, i] if b != MISS]
        if ids != ([int(x[0]) for x in walks[i]["hits"]], [int(x[0]) for x in walks[i]["lifted"]]):
            continue
        casts = len(ids[0]) + len(ids[1]) + 3
        if np.abs(pos_out[i] - walks[i]["p"]).max() > casts * 4 * tol[i]:
            far.append((int(i), pos_out[i], walks[i]["p"], casts, tol[i]))
    assert not far, far[:4]


# ---- 4. closed forms ------------------------------------------------------------------------------------------------------------
R, H = 0.25, 0.5
STAND = R + H + float(SKIN)  # the centre of an upright character that stands skin above y = 0


def _boxes(*boxes):
    """statics: (lo, hi) axis-aligned boxes, or (pos, rot, half extent) triples as cases.ramp gives"""
    pos, rot, he = [], [], []
    for b in boxes:
        if len(b) == 2:
            lo, hi = np.asarray(b[0], np.float64), np.asarray(b[1], np.float64)
            pos.append((lo + hi) / 2); rot.append(IDENT); he.append((hi - lo) / 2)
        else:
            pos.append(b[0]); rot.append(b[1]); he.append(b[2])
    m = len(pos)
    return dict(pos=np.array(pos), rot=np.array(rot), shape=np.full(m, BOX), half_extent=np.array(he))


def _walk1(w, pos, motion, grounded=1, step_height=0.3, snap_distance=0.2, ny=cases.MIN_FLOOR_NY, max_slides=4):
    out = w.character_move(np.array([pos], F), np.array([motion], F), R, H, grounded=[grounded], skin=SKIN, max_slides=max_slides,
                           step_height=step_height, snap_distance=snap_distance, min_floor_ny=ny)
    p0, m0 = np.array(pos, F).astype(np.float64), np.array(motion, F).astype(np.float64)
    status = int(out[2][0])
    hits = (status & 0xF) + ((status >> 4) & 0xF)
    tol = (hits + 1) * 1e-5 * (1.0 + np.abs(p0).max() + H + np.linalg.norm(m0))
    print(pos, motion, "->", out[0][0], out[1][0], hex(status), "floor", hex(int(out[3][0])), out[4][0], "tol", tol)
    return out[0][0].astype(np.float64), out[1][0].astype(np.float64), status, int(out[3][0]), out[4][0], p0, m0, tol


def test_closed_forms_level_ground_and_risers():
    w = _world(None, _boxes(([2, -1, -5], [10, 0.2, 5])), 0.0)
    # level ground: the whole horizontal motion, y unchanged, GROUNDED on the ground
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [-3, STAND, 0], [1.0, 0.0, 0.3])
    assert status == GROUNDED and floor == GROUND and np.array_equal(p, p0 + m0) and not rem.any() and list(fn) == [0, 1, 0]
    # a riser of 0.2 with step_height 0.3: on top, skin above it
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [1, STAND, 0], [2.0, 0.0, 0.0])
    assert status & STEPPED and status & GROUNDED and floor == ST0 and not rem.any() and not status & (SNAPPED | BLOCKED)
    assert abs(p[0] - 3.0) <= tol and abs(p[1] - (0.2 + STAND)) <= tol and p[2] == 0 and abs(fn[1] - 1) <= 1e-6
    # the same riser with step_height 0.1: stops at it, no gain in y
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [1, STAND, 0], [2.0, 0.0, 0.0], step_height=0.1)
    assert status & HIT_WALL and not status & STEPPED and status & GROUNDED and floor == GROUND
    assert abs(p[1] - p0[1]) <= tol and p[0] < 2.0 - 0.2 and p[0] > 1.5
    w.close()
    # a wall far taller than the step, head on: the lifted slide stops where MOVE stopped, to the bit, so the landing on the
    # level left has made no more progress and is no step
    w = _world(None, _boxes(([2, -1, -5], [10, 3.0, 5])), 0.0)
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [1, STAND, 0], [2.0, 0.0, 0.0])
    assert status & HIT_WALL and not status & (STEPPED | SNAPPED) and status & GROUNDED and floor == GROUND and (status >> 4) & 0xF == 1
    assert abs(p[0] - (2.0 - R - float(SKIN))) <= tol and p[1] == p0[1] and not rem.any()
    w.close()
    # step-up under a low ceiling: the lift is what fits under it (0.25: the riser is taken; 0.05: it is not, the lower ball meets
    # the riser's edge with a normal that is too steep to land on)
    top = STAND + R + H
    for gap, taken in ((0.25, True), (0.05, False)):
        w = _world(None, _boxes(([2, -1, -5], [10, 0.2, 5]), ([-5, top + gap + float(SKIN), -5], [10, top + 3, 5])), 0.0)
        p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [1, STAND, 0], [2.0, 0.0, 0.0])
        assert bool(status & STEPPED) == taken and status & GROUNDED
        assert abs(p[1] - ((0.2 if taken else 0.0) + STAND)) <= tol
        # a jump under that ceiling: HIT_CEILING, stopped skin below it
        p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [0, STAND, 0], [0.3, 1.0, 0.0])
        assert status & HIT_CEILING and status & HIT_WALL and not status & GROUNDED and p[1] < p0[1] + gap + float(SKIN) + tol
        w.close()


def test_closed_forms_ramps():
    t30, t60 = math.tan(math.radians(30)), math.tan(math.radians(60))
    s30, c30 = math.sin(math.radians(30)), math.cos(math.radians(30))
    skin = float(SKIN)
    w = _world(None, _boxes(cases.ramp(2.0, 0.0, 30.0), cases.ramp(2.0, 20.0, 60.0)), 0.0)
    # a 30 degree ramp under a limit of 45: the lower ball (centre R + skin above the ground) touches the plane through (2, 0)
    # where its distance from it is R; the stop is skin short of that, and what is left slides up the ramp
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [0, STAND, 0], [3.0, 0.0, 0.0])
    x_touch = 2.0 - (R - c30 * (R + skin)) / s30
    a = x_touch - p0[0] - skin
    left = (3.0 - a) * c30
    want = p0 + [a, 0, 0] + left * np.array([c30, s30, 0.0])
    assert status & GROUNDED and floor == ST0 and not status & (HIT_WALL | STEPPED | SNAPPED) and (status & 0xF) >= 1
    assert np.abs(p - want).max() <= tol and abs((p[1] - p0[1]) - t30 * (p[0] - (p0[0] + a))) <= tol
    assert np.abs(fn - [-s30, c30, 0]).max() <= 1e-5
    # a 60 degree ramp, walking: no gain in y
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [0, STAND, 20], [3.0, 0.0, 0.5])
    assert status & HIT_WALL and not status & STEPPED and p[1] <= p0[1] + tol and p[0] < 2.0 and abs(p[2] - 20.5) <= tol
    # the same ramp, airborne and falling onto it: slides down it, and ends on it ON_STEEP
    y = (4.0 - 2.0) * t60 + 2.0
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [4, y, 20], [0.0, -1.5, 0.0], grounded=0)
    assert status & ON_STEEP and status & HIT_WALL and not status & GROUNDED and floor == ST0 + 1
    assert p[0] < p0[0] - 0.1 and p[1] < p0[1] - 0.5 and abs(fn[1] - 0.5) <= 1e-5
    w.close()


def test_closed_forms_ledges_and_overlap():
    skin = float(SKIN)
    w = _world(None, _boxes(([-6, -1, -5], [0, 0.1, 5]), ([-6, -1, 15], [0, 0.5, 25])), 0.0)
    # a ledge of 0.1 under a snap_distance of 0.2: down by 0.1 onto the ground
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [-0.5, 0.1 + STAND, 0], [1.5, 0.0, 0.0])
    assert status == GROUNDED | SNAPPED and floor == GROUND and abs(p[1] - (p0[1] - 0.1)) <= tol and abs(p[0] - 1.0) <= tol
    # ... and a character that does not walk is not snapped
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [-0.5, 0.1 + STAND, 0], [1.5, 0.0, 0.0], grounded=0)
    assert status == 0 and p[1] == p0[1] and floor == MISS
    # a ledge of 0.5: not grounded, y unchanged
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [-0.5, 0.5 + STAND, 20], [1.5, 0.0, 0.0])
    assert status == 0 and p[1] == p0[1] and floor == MISS and np.array_equal(p, p0 + m0)
    # an overlapping start: BLOCKED, nothing moves, no ground state
    p, rem, status, floor, fn, p0, m0, tol = _walk1(w, [-3, 0.3, 0], [1.0, 0.0, 0.0])
    assert status == 1 | BLOCKED and floor == MISS and np.array_equal(p, p0) and np.array_equal(rem, m0)
    w.close()


# ---- 5. refusals and INVALID ----------------------------------------------------------------------------------------------------
def test_refusals_n_zero_and_null_outputs(worlds):
    from physics_amd import _abi
    w = worlds("terrain")
    c = cases.case("terrain")
    n = 64
    p = lambda x, t=_abi.f32p: None if x is None else x.ctypes.data_as(t)
    a = {k: np.ascontiguousarray(c[k][:n]) for k in ("pos", "motion", "rot", "rad", "hq", "grounded")}
    full = _call(w, c, slice(0, n))
    out = dict(pos_out=np.zeros((n, 3), F), status_out=np.zeros(n, np.uint32))
    skin, k, step, snap, ny = cases.params()

    def call(n=n, skin=skin, k=k, step=step, snap=snap, ny=ny, **kw):
        x = dict(a, **out)
        x.update(kw)
        return w.lib.phys_character_move(w.h, n, p(x["pos"]), p(x["motion"]), p(x["rot"]), p(x["rad"]), p(x["hq"]), p(x["grounded"], _abi.u32p), skin, k,
                                         step, snap, ny, None, None, p(x["pos_out"]), None, p(x["status_out"], _abi.u32p), None, None, None, None,
                                         None, None)

    E = _abi.PHYS_ERR_INVALID_ARG
    assert call() == 0 and np.array_equal(_bits(out["pos_out"]), _bits(full[0])) and np.array_equal(out["status_out"], full[2])
    assert call(rot=None) == 0 and call(grounded=None) == 0 and call(ny=1.0) == 0 and call(step=0.0, snap=0.0) == 0
    refused = [dict(n=1 << 31), dict(pos=None), dict(motion=None), dict(rad=None), dict(hq=None), dict(pos_out=None), dict(status_out=None), dict(k=0),
               dict(k=9), dict(ny=0.0), dict(ny=-0.1), dict(ny=1.0001), dict(ny=math.nan)]
    refused += [{key: v} for key in ("skin", "step", "snap") for v in (-0.01, math.nan, math.inf)]
    for kw in refused:
        assert call(**kw) == E, kw
    # the device variant: the same call on device arrays gives the host variant's answer, and refuses the same list
    import ctypes as C
    import torch
    dev = {key: torch.from_numpy(np.array(v).view(np.int32) if v.dtype == np.uint32 else np.array(v)).cuda() for key, v in dict(a, **out).items()}
    d = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def dcall(n=n, skin=skin, k=k, step=step, snap=snap, ny=ny, **kw):
        x = dict(dev)
        x.update(kw)
        return w.lib.phys_character_move_device(w.h, n, d(x["pos"]), d(x["motion"]), d(x["rot"]), d(x["rad"]), d(x["hq"]), d(x["grounded"]), skin, k,
                                                step, snap, ny, None, None, d(x["pos_out"]), None, d(x["status_out"]), None, None, None, None,
                                                None, None)

    torch.cuda.synchronize()
    assert dcall() == 0
    w.sync()
    assert np.array_equal(_bits(dev["pos_out"].cpu().numpy()), _bits(full[0])) and np.array_equal(dev["status_out"].cpu().numpy().view(np.uint32), full[2])
    for kw in refused:
        assert dcall(**kw) == E, kw
    nulls = [None] * 6
    assert w.lib.phys_character_move_device(w.h, n, *nulls, 0.02, 4, 0.3, 0.2, 0.7, *[None] * 11) == E
    # n == 0 is a no-op, whatever the pointers
    assert w.lib.phys_character_move(w.h, 0, *nulls, 0.02, 4, 0.3, 0.2, 0.7, *[None] * 11) == 0
    assert w.lib.phys_character_move_device(w.h, 0, *nulls, 0.02, 4, 0.3, 0.2, 0.7, *[None] * 11) == 0
    empty = w.character_move(np.zeros((0, 3), F), np.zeros((0, 3), F), 0.25, 0.5)
    assert empty[0].shape == (0, 3) and empty[6].shape == (8, 0)
    w.sync()


def test_invalid_queries(worlds):
    w = worlds("terrain")
    c = cases.case("terrain")
    n = 11
    pos, motion = np.tile(c["pos"][0], (n, 1)), np.tile(c["motion"][0], (n, 1))
    rot = np.tile(np.array(IDENT, F), (n, 1))
    rad, hq = np.full(n, 0.25, F), np.full(n, 0.5, F)
    rad[:3] = [-1, np.nan, np.inf]
    hq[3:6] = [-1, np.nan, np.inf]
    rot[6, 2] = np.nan
    rot[7, 0] = np.inf
    motion[8, 1] = np.inf
    pos[9, 0] = np.nan
    motion[10] = [2e38, 2e38, 2e38]
    m = 40
    pos, motion, rot = np.vstack([pos, c["pos"][:m]]), np.vstack([motion, c["motion"][:m]]), np.vstack([rot, c["rot"][:m]])
    rad, hq = np.concatenate([rad, c["rad"][:m]]), np.concatenate([hq, c["hq"][:m]])
    grounded = np.concatenate([np.ones(n, np.uint32), c["grounded"][:m]])
    skin, k, step, snap, ny = cases.params()
    kw = dict(skin=skin, max_slides=k, step_height=step, snap_distance=snap, min_floor_ny=ny)
    with np.errstate(all="ignore"):
        got = w.character_move(pos, motion, rad, hq, rot=rot, grounded=grounded, **kw)
    assert list(got[2][:n]) == [INVALID] * n
    assert np.array_equal(_bits(got[0][:n]), _bits(pos[:n])) and np.array_equal(_bits(got[1][:n]), _bits(motion[:n]))
    assert (got[6][:, :n] == MISS).all() and not got[7][:, :n].any() and not got[8][:, :n].any()
    assert (got[3][:n] == MISS).all() and not got[4][:n].any() and not got[5][:n].any()
    alone = w.character_move(pos[n:], motion[n:], rad[n:], hq[n:], rot=rot[n:], grounded=grounded[n:], **kw)
    _same(_rows(got, slice(n, None), n + m), alone, "valid among invalid")
    assert (alone[2] & GROUNDED).any()


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------
def _snapshot(w):
    pos, rot = w.get_transforms()
    lin, ang = w.get_velocities()
    st = w.get_stats()
    return [pos, rot, lin, ang], {k: getattr(st, k) for k, _ in type(st)._fields_}, w.get_manifolds()


def test_updates_are_bit_identical_and_new_poses_are_seen():
    import torch
    pa = _pa()
    from physics_amd import scenes
    sc = scenes.c2()
    pair = []
    for _ in range(2):
        w = pa.World(sc.config())
        sc.populate(w)
        pair.append(w)
    quiet, probed = pair
    rng = np.random.default_rng(3)
    lo, hi = sc.pos.min(0) - 3, sc.pos.max(0) + 3
    n = 2000
    pos = rng.uniform(lo, hi, (n, 3)).astype(F)
    motion = rng.normal(size=(n, 3)).astype(F) * 3
    grounded = (rng.random(n) < 0.5).astype(np.uint32)
    tp, tm, tg = torch.from_numpy(pos).cuda(), torch.from_numpy(motion).cuda(), torch.from_numpy(grounded.view(np.int32)).cuda()
    tr = torch.full((n,), 0.25, dtype=torch.float32, device="cuda")
    th = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    to = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ts = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    found = 0
    for k in range(8):
        for w in pair:
            w.update_n(scenes.DT_NANOS, 2)
        status = probed.character_move(pos, motion, 0.25, 0.5, grounded=grounded, skin=SKIN)[2]
        probed.character_move_device(tp, tm, tr, th, to, ts, grounded=tg, skin=SKIN)
        found += int(((status & 0xF) > 0).sum())
    for w in pair:
        w.sync()
    a, b = _snapshot(quiet), _snapshot(probed)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    assert found > 0
    # after phys_set_body_poses the call sees the new poses: body 0 moved far away, alone in the character's way
    quiet.close()
    probed.set_body_poses([0], pos=[[500.0, 500.0, 500.0]], rot=[IDENT])
    out = probed.character_move([[500.0, 500.0, 480.0]], [[0.0, 0.0, 30.0]], 0.25, 0.5, skin=SKIN)
    assert (out[2][0] & 0xF) >= 1 and out[6][0, 0] == 0 and 480.0 < out[0][0][2] < 500.0
    probed.close()
