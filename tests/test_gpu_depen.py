"""GPU: depenetration (phys_penetration, phys_depenetrate and their device variants) on the seeded scenes of tests/depen_cases.py.

1. one launch equals the loop: max_iters + 1 rounds of World.penetration(max_gap = skin) with the spec header's dp_step on the CPU
   between them (tests/depen_probe.py), bit for bit, over three scenes, three round counts, four query counts, ignore, upright,
   filters, the device variant and reversed order; phys_penetration's answer is slot 0 of a depenetrate that pushed;
2. float64 properties that share no code with the kernels or the spec header (tests/depen_ref.py);
3. closed forms;
4. the hand-over: characters that phys_move_and_slide reports BLOCKED at their first cast move after a depenetrate;
5. refusals, n = 0, NULL outputs and INVALID queries among valid ones;
6. no side effects on the updates, and the poses of phys_set_body_poses are seen.

Tolerances: tests/test_depen_cpu.py (tol_of, LOOP_TOL)."""
import math

import numpy as np
import pytest

import depen_cases as cases
import depen_probe as probe
import depen_ref as ref
import slide_cases
from capsulecast_ref import query_ref, rotation_matrices

pytestmark = pytest.mark.gpu

F = np.float32
MISS, GROUND, STATIC = 0xFFFFFFFE, 0xFFFFFFFF, 0x80000000
STUCK, INVALID = 0x100, 0x400
SLIDE_BLOCKED = 0x100
SKIN = F(cases.SKIN)
LOOP_TOL = 10.0  # tests/test_depen_cpu.py: measured there
IDENT = [0.0, 0.0, 0.0, 1.0]
SPHERE, BOX, CAPSULE = 1, 2, 3
NAMES = ("pos", "status", "hit_body", "hit_normal", "hit_depth")


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


def _statics(shape, pos, he, rot=None):
    m = len(shape)
    return dict(pos=np.asarray(pos, F).reshape(m, 3), rot=np.tile(np.array(IDENT, F), (m, 1)) if rot is None else np.asarray(rot, F),
                shape=np.asarray(shape, np.uint32), half_extent=np.asarray(he, F).reshape(m, 3))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        diff = np.nonzero(_bits(x).reshape(-1) != _bits(y).reshape(-1))[0]
        assert len(diff) == 0, (what, name, len(diff), diff[:6], x.reshape(-1)[diff[:6]], y.reshape(-1)[diff[:6]])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("depen") / "depen_probe"))


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _world(*slide_cases.scene(name))
        return made[name]

    yield get
    for w in made.values():
        w.close()


def _loop(exe, w, c, k, max_iters, skin=SKIN, rot=True, ignore=None, mask=None):
    """(one launch, the host loop of probes) for rows k of case c"""
    sub = lambda a: None if a is None else np.ascontiguousarray(a[k])
    pos, rad, hq = sub(c["pos"]), sub(c["rad"]), sub(c["hq"])
    q = sub(c["rot"]) if rot else None
    ig = sub(ignore)
    m = mask if mask is None or np.ndim(mask) == 0 else sub(mask)
    got = w.depenetrate(pos, rad, hq, rot=q, skin=skin, max_iters=max_iters, ignore=ig, mask=m)
    want = probe.host_loop(exe, lambda p, r, h, **kw: w.penetration(p, r, h, **kw), pos, rad, hq, q, skin, max_iters, ignore=ig, mask=m)
    return got, want


def _slots_are_whole(got, max_iters):
    pos, status, body, nrm, dep = got
    pushes = status & 0xF
    assert body.shape == (max_iters, len(status)) and nrm.shape == (max_iters, len(status), 3) and dep.shape == (max_iters, len(status))
    used = np.arange(max_iters)[:, None] < pushes[None, :]
    assert ((body != MISS) == used).all() and not nrm[~used].any() and not dep[~used].any()
    assert np.isfinite(pos).all()


# ---- 1. one launch equals the loop, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iters", [1, 4, 8])
@pytest.mark.parametrize("name", cases.SCENES)
def test_one_launch_equals_the_loop_of_probes(name, max_iters, exe, worlds):
    c = cases.case(name)
    n = len(c["pos"])
    got, want = _loop(exe, worlds(name), c, slice(None), max_iters)
    _same(got, want, f"{name} max_iters {max_iters}")
    status = got[1]
    pushes, stuck = status & 0xF, status & STUCK != 0
    print(name, max_iters, "pushes", np.bincount(pushes, minlength=9), "stuck", int(stuck.sum()))
    _slots_are_whole(got, max_iters)
    assert not (status & INVALID).any() and (pushes[stuck] == max_iters).all()
    if name == "empty":
        assert not status.any() and np.array_equal(_bits(got[0]), _bits(c["pos"]))
    elif max_iters == 4:
        # the set fills three bins: clear at once, two pushes or more, STUCK
        assert (pushes == 0).sum() >= n // 10 and (pushes >= 2).sum() >= n // 10 and stuck.sum() >= 5
    # phys_penetration's answer is slot 0 of a depenetrate that pushed
    b, d, nn = worlds(name).penetration(c["pos"], c["rad"], c["hq"], rot=c["rot"], max_gap=SKIN)
    pushed = pushes > 0
    assert np.array_equal(b[pushed], got[2][0][pushed]) and np.array_equal(_bits(d[pushed]), _bits(got[4][0][pushed]))
    assert np.array_equal(_bits(nn[pushed]), _bits(got[3][0][pushed]))
    clear = ~pushed
    assert ((b[clear] == MISS) | ~(d[clear] > F(-0.5) * SKIN)).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_query_counts_around_the_workgroup_size(n, exe, worlds):
    c = cases.case("soup")
    got, want = _loop(exe, worlds("soup"), c, slice(100, 100 + n), 4)
    _same(got, want, f"n = {n}")
    assert n == 1 or (got[1] & 0xF).max() >= 2


def test_filters_ignore_and_upright(exe):
    c = cases.case("soup")
    n = len(c["pos"])
    cat, scat, gcat, masks, _ = slide_cases.filters()
    w = _world(*slide_cases.scene("soup"))
    plain = w.depenetrate(c["pos"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN)
    first = plain[2][0]
    rng = np.random.default_rng(5300)
    ignore = np.where((first < 300) & (rng.random(n) < 0.7), first, 0xFFFFFFFF).astype(np.uint32)
    got, want = _loop(exe, w, c, slice(None), 4, ignore=ignore)
    _same(got, want, "ignore")
    given = ignore != 0xFFFFFFFF
    assert given.sum() > 50 and (got[2][:, given] != ignore[given][None, :]).all()
    got, want = _loop(exe, w, c, slice(None), 4, rot=False)
    _same(got, want, "upright")
    # random categories, per-query masks
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(gcat, 0xFFFF)
    got, want = _loop(exe, w, c, slice(None), 4, mask=masks)
    _same(got, want, "masks")
    for k in range(4):
        b, m = got[2][k], masks
        dyn = b < 300
        assert ((cat[b[dyn]] & m[dyn]) != 0).all()
        st = (b >= STATIC) & (b < MISS)
        assert ((scat[b[st] - STATIC] & m[st]) != 0).all()
        assert ((m[b == GROUND] & gcat) != 0).all()
    # a mask of all ones is the unfiltered instance's answer; mask 0 sees nothing
    _same(w.depenetrate(c["pos"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, mask=0xFFFF), plain, "mask 0xFFFF")
    none = w.depenetrate(c["pos"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, mask=0)
    assert not none[1].any() and np.array_equal(_bits(none[0]), _bits(c["pos"]))
    b, d, _ = w.penetration(c["pos"], c["rad"], c["hq"], rot=c["rot"], max_gap=1.0, mask=0)
    assert (b == MISS).all() and (d == -np.inf).all()
    w.close()


def test_device_variant_and_reversed_order(worlds):
    import torch
    c = cases.case("soup")
    w = worlds("soup")
    n, k = len(c["pos"]), 4
    ignore = np.where(np.arange(n) % 3 == 0, np.arange(n) % 300, 0xFFFFFFFF).astype(np.uint32)
    host = w.depenetrate(c["pos"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, max_iters=k, ignore=ignore)
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()
    tp = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    ts = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    tb = torch.full((k, n), 7, dtype=torch.int32, device="cuda")
    tn = torch.full((k, n, 3), 7.0, dtype=torch.float32, device="cuda")
    td = torch.full((k, n), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ins = (dev(c["pos"]), dev(c["rad"]), dev(c["hq"]))
    w.depenetrate_device(*ins, tp, ts, tb, tn, td, rot=dev(c["rot"]), skin=SKIN, max_iters=k, ignore=dev(ignore.view(np.int32)))
    w.sync()
    _same(host, (tp.cpu().numpy(), ts.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32), tn.cpu().numpy(), td.cpu().numpy()), "device")
    # the device variant with a mask of all ones and without the optional outputs
    tp2, ts2 = torch.empty_like(tp), torch.empty_like(ts)
    w.depenetrate_device(*ins, tp2, ts2, rot=dev(c["rot"]), skin=SKIN, max_iters=k, ignore=dev(ignore.view(np.int32)),
                         mask=dev(np.full(n, -1, np.int16)))
    w.sync()
    assert torch.equal(tp, tp2) and torch.equal(ts, ts2)
    # the probe: device against host
    hb, hd, hn = w.penetration(c["pos"], c["rad"], c["hq"], rot=c["rot"], max_gap=0.3, ignore=ignore)
    pb, pd, pn = tb[0].clone(), td[0].clone(), tn[0].clone()
    w.penetration_device(*ins, pb, pd, pn, rot=dev(c["rot"]), max_gap=0.3, ignore=dev(ignore.view(np.int32)))
    w.sync()
    assert np.array_equal(hb, pb.cpu().numpy().view(np.uint32)) and np.array_equal(_bits(hd), _bits(pd.cpu().numpy()))
    assert np.array_equal(_bits(hn), _bits(pn.cpu().numpy()))
    assert (hd[hb != MISS] >= F(-0.3)).all() and (hb != MISS).sum() >= (host[1] & 0xF > 0).sum()
    # reversed order
    r = slice(None, None, -1)
    rev = w.depenetrate(c["pos"][r], c["rad"][r], c["hq"][r], rot=c["rot"][r], skin=SKIN, max_iters=k, ignore=ignore[r])
    _same(host, tuple(x[r] if x.ndim < 2 or x.shape[0] == n else x[:, r] for x in rev), "reversed")


# ---- 2. float64 properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "statics"])
def test_float64_properties(name, worlds):
    c = cases.case(name)
    n = len(c["pos"])
    pos_out, status, body, nrm, dep = worlds(name).depenetrate(c["pos"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, max_iters=cases.MAX_ITERS)
    tol = np.array([cases.tol_of(c["pos"][i], c["hq"][i]) for i in range(n)])
    pushes = status & 0xF
    skin = float(SKIN)
    checked = ties = started_clear = 0
    least = np.inf
    for i in range(n):
        sub = {k: v[c["near"][i]] for k, v in c["tg"].items()}
        fr = c["frames"][c["near"][i]]
        a, R, h = c["a"][i], float(c["rad"][i]), float(c["hq"][i])
        rid, rd, _, rd2, inside = c["first"][i]
        # a query that starts a skin clear of everything returns pos bit for bit with status 0
        if rid == MISS or rd <= -skin:
            started_clear += 1
            assert status[i] == 0 and np.array_equal(_bits(pos_out[i]), _bits(c["pos"][i])), i
        # slot 0's id is the reference's deepest (the reference's own near ties apart; a core inside a box: by the spec's face rule)
        if pushes[i] and not inside:
            if math.isfinite(rd2) and rd - rd2 < tol[i]:
                ties += 1
            else:
                assert body[0, i] == rid, (i, hex(int(body[0, i])), hex(rid))
        # |pos_out - pos| <= sum (d_k + skin)
        moved = np.linalg.norm(pos_out[i].astype(np.float64) - c["pos"][i].astype(np.float64))
        assert moved <= float(sum(dep[k, i] + SKIN for k in range(pushes[i]))) + LOOP_TOL * tol[i], i
        if status[i] & (STUCK | INVALID):
            continue
        # every result that is not STUCK is skin / 2 clear of every reference target (a loop ends clear with the core outside
        # every target, where the depths hold to tol: measured on the CPU, no result lies below skin / 2 at all)
        sep = ref.separation(pos_out[i].astype(np.float64), a, R, h, sub, c["ground"], fr)
        checked += 1
        least = min(least, sep)
        assert sep >= 0.5 * skin - tol[i], (i, sep, hex(int(status[i])))
    print(name, "checked", checked, "least separation", least, "started clear", started_clear, "near ties", ties)
    assert ties <= n // 100 and checked > n // 2 and started_clear > n // 20


# ---- 3. closed forms ------------------------------------------------------------------------------------------------------------
def _one(w, pos, R, h, rot=None, skin=SKIN, max_iters=4):
    out = w.depenetrate(np.array([pos], F), R, h, rot=None if rot is None else np.array([rot], F), skin=skin, max_iters=max_iters)
    return out[0][0], int(out[1][0]), out[2][:, 0], out[3][:, 0], out[4][:, 0]


def test_closed_forms_ground_ball_and_box():
    s = float(SKIN)
    # a capsule sunk 0.1 into the ground: one push, straight up
    w = _world(None, None, 0.0)
    p, status, body, nrm, dep = _one(w, [1.0, 0.65, -2.0], 0.25, 0.5)
    assert status == 1 and body[0] == GROUND and np.array_equal(nrm[0], [0, 1, 0]) and abs(dep[0] - 0.1) <= 1e-6
    assert abs(p[1] - (0.65 + 0.1 + s)) <= 1e-6 and p[0] == F(1.0) and p[2] == F(-2.0) and list(body[1:]) == [MISS] * 3
    b, d, n = w.penetration(np.array([[1.0, 0.65, -2.0], [0, 0.76, 0], [0, 0.78, 0]], F), 0.25, 0.5, max_gap=0.02)
    assert list(b) == [GROUND, GROUND, MISS] and abs(d[0] - 0.1) <= 1e-6 and abs(d[1] + 0.01) <= 1e-6 and d[2] == -np.inf
    w.close()
    # a ball in a ball; coincident centres: the narrow phase's (0,1,0) fallback from the query to the target, so the push is down
    w = _world(None, _statics([SPHERE], [[2, 3, 4]], [[1.0, 0, 0]]), None)
    u = np.array([1.0, 2.0, -2.0]) / 3.0
    p, status, body, nrm, dep = _one(w, np.array([2, 3, 4]) + 0.9 * u, 0.3, 0.0)
    assert status == 1 and body[0] == STATIC and np.abs(nrm[0] - u).max() <= 1e-6 and abs(dep[0] - 0.4) <= 1e-5
    assert np.abs(p - (np.array([2, 3, 4]) + (1.3 + s) * u)).max() <= 1e-5
    p, status, body, nrm, dep = _one(w, [2, 3, 4], 0.3, 0.0)
    assert status == 1 and np.array_equal(nrm[0], [0, -1, 0]) and np.isfinite(p).all() and abs(dep[0] - 1.3) <= 1e-5
    assert abs(p[1] - (3 - 1.3 - s)) <= 1e-5
    assert ref.separation(p.astype(np.float64), [0, 1, 0], 0.3, 0.0, query_ref.targets(None, _statics([SPHERE], [[2, 3, 4]], [[1.0, 0, 0]])), None) >= 0.5 * s - 1e-5
    w.close()
    # a capsule lying across a box face; a ball whose centre is deep inside the box leaves through the nearest face
    box = _statics([BOX], [[0, 1, 0]], [[2.0, 1.0, 3.0]])
    w = _world(None, box, None)
    lying = [math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5)]  # a quarter turn about x: the core along z
    p, status, body, nrm, dep = _one(w, [0.5, 2.2, 0.0], 0.25, 0.8, rot=lying)
    assert status == 1 and body[0] == STATIC and np.abs(nrm[0] - [0, 1, 0]).max() <= 1e-6 and abs(dep[0] - 0.05) <= 1e-5
    assert abs(p[1] - (2.25 + s)) <= 1e-5
    p, status, body, nrm, dep = _one(w, [1.6, 1.0, 0.5], 0.2, 0.0)
    assert status == 1 and np.abs(nrm[0] - [1, 0, 0]).max() <= 1e-6 and abs(dep[0] - 0.6) <= 1e-5 and abs(p[0] - (2.2 + s)) <= 1e-5
    w.close()


def test_closed_forms_corner_sandwich_and_equal_statics():
    s = float(SKIN)
    floor, wall = ([0.0, -0.5, 0.0], [10.0, 0.5, 10.0]), ([-0.5, 5.0, 0.0], [0.5, 5.0, 10.0])
    w = _world(None, _statics([BOX, BOX], [floor[0], wall[0]], [floor[1], wall[1]]), None)
    p, status, body, nrm, dep = _one(w, [0.2, 0.25, 0.0], 0.3, 0.0)
    assert status == 2 and list(body[:2]) == [STATIC | 1, STATIC | 0]
    assert np.abs(p - [0.3 + s, 0.3 + s, 0.0]).max() <= 1e-5
    w.close()
    # a slot 0.5 high, a ball of 0.6: STUCK at every round count, finite
    w = _world(None, _statics([BOX, BOX], [floor[0], [0, 1.0, 0]], [floor[1], [10, 0.5, 10]]), None)
    for mi in (1, 4, 8):
        p, status, body, _, _ = _one(w, [0, 0.26, 0], 0.3, 0.0, max_iters=mi)
        assert status == (mi | STUCK) and np.isfinite(p).all() and (body != MISS).all()
    w.close()
    # two equal statics at one place: an exact tie goes to the smaller id; the ground loses ties with both
    w = _world(None, _statics([BOX, BOX], [floor[0], floor[0]], [floor[1], floor[1]]), 0.0)
    b, d, _ = w.penetration(np.array([[0.0, 0.25, 0.0]], F), 0.5, 0.0, max_gap=0.0)  # (0.25 deep in all three, to the bit)
    assert b[0] == STATIC and d[0] == F(0.25)
    p, status, body, _, _ = _one(w, [0.0, 0.25, 0.0], 0.5, 0.0)
    assert status == 1 and body[0] == STATIC
    w.set_static_filters(category=np.array([2, 1], np.uint16))
    assert w.penetration(np.array([[0.0, 0.25, 0.0]], F), 0.5, 0.0, max_gap=0.0, mask=1)[0][0] == (STATIC | 1)
    w.close()


def test_long_thin_capsules_over_small_balls():
    """the candidate walk covers the capsule's whole AABB grown by the gap: long thin capsules whose contacts lie far from
    their centres, just touching and just clear"""
    import capsulecast_cases as cc
    c = cc.degenerate("long_thin")
    w = _world(c["bodies"], None, None)
    h = c["h"]
    hit = np.nonzero(np.isfinite(h["t"]))[0]
    assert len(hit) > 40
    u = c["d"].astype(np.float64) / np.linalg.norm(c["d"].astype(np.float64), axis=1, keepdims=True)
    tg = c["tg"]
    fr = query_ref._frames(tg)
    a = rotation_matrices(c["rot"].astype(np.float64))[:, :, 1]
    for back, gap in ((-0.02, 0.0), (0.2, 0.3)):
        pos = (c["o"][hit].astype(np.float64) + u[hit] * (h["t"][hit] - back)[:, None]).astype(F)
        b, d, n = w.penetration(pos, c["rad"][hit], c["hq"][hit], rot=c["rot"][hit], max_gap=gap)
        wrong = 0
        for j, i in enumerate(hit):
            rid, rd, rn, rd2, _ = ref.deepest(pos[j].astype(np.float64), a[i], float(c["rad"][i]), float(c["hq"][i]), tg, None, gap, frames_=fr)
            tol = cases.tol_of(pos[j], c["hq"][i])
            if abs(rd + gap) <= tol or (math.isfinite(rd2) and rd - rd2 < tol):
                continue  # at the edge of the gap, or a near tie
            wrong += int(b[j] != rid)
            assert b[j] != rid or abs(d[j] - rd) <= tol, (i, d[j], rd)
        assert wrong == 0, (back, wrong)
        assert (b != MISS).sum() > 40
    w.close()


# ---- 4. the hand-over to move-and-slide -----------------------------------------------------------------------------------------
def test_blocked_characters_move_after_depenetrate(worlds):
    c = slide_cases.case("soup")
    w = worlds("soup")
    first = w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], skin=SKIN, max_slides=4)  # upright: some start inside something
    blocked = np.nonzero(first[2] == (1 | SLIDE_BLOCKED))[0]
    assert len(blocked) >= 20
    out = w.depenetrate(c["pos"][blocked], c["rad"][blocked], c["hq"][blocked], skin=0.02, max_iters=8)
    clear = (out[1] & (STUCK | INVALID)) == 0
    assert clear.sum() >= (3 * len(blocked)) // 4 and (out[1][clear] & 0xF).min() >= 1
    k = blocked[clear]
    again = w.move_and_slide(out[0][clear], c["motion"][k], c["rad"][k], c["hq"][k], skin=SKIN, max_slides=4)
    print("blocked", len(blocked), "clear after depenetrate", int(clear.sum()), "statuses", np.unique(again[2]))
    assert (again[2] != (1 | SLIDE_BLOCKED)).all()


# ---- 5. refusals and INVALID ----------------------------------------------------------------------------------------------------
def test_refusals_n_zero_and_null_outputs(worlds):
    from physics_amd import _abi
    w = worlds("soup")
    c = cases.case("soup")
    n = 64
    p = lambda x, t=_abi.f32p: None if x is None else x.ctypes.data_as(t)
    a = {k: np.ascontiguousarray(c[k][:n]) for k in ("pos", "rot", "rad", "hq")}
    full = w.depenetrate(a["pos"], a["rad"], a["hq"], rot=a["rot"], skin=SKIN, max_iters=4)
    probe_full = w.penetration(a["pos"], a["rad"], a["hq"], rot=a["rot"], max_gap=SKIN)
    out = dict(pos_out=np.zeros((n, 3), F), status_out=np.zeros(n, np.uint32), body_out=np.zeros(n, np.uint32), depth_out=np.zeros(n, F))
    u32 = _abi.u32p

    def push(n=n, skin=float(SKIN), k=4, **kw):
        x = dict(a, **out)
        x.update(kw)
        return w.lib.phys_depenetrate(w.h, n, p(x["pos"]), p(x["rot"]), p(x["rad"]), p(x["hq"]), skin, k, None, None, p(x["pos_out"]),
                                      p(x["status_out"], u32), None, None, None)

    def look(n=n, gap=float(SKIN), **kw):
        x = dict(a, **out)
        x.update(kw)
        return w.lib.phys_penetration(w.h, n, p(x["pos"]), p(x["rot"]), p(x["rad"]), p(x["hq"]), gap, None, None, p(x["body_out"], u32),
                                      p(x["depth_out"]), None)

    E = _abi.PHYS_ERR_INVALID_ARG
    # NULL optional outputs: the calls work and the others are as before
    assert push() == 0 and np.array_equal(_bits(out["pos_out"]), _bits(full[0])) and np.array_equal(out["status_out"], full[1])
    assert look() == 0 and np.array_equal(out["body_out"], probe_full[0]) and np.array_equal(_bits(out["depth_out"]), _bits(probe_full[1]))
    assert push(rot=None) == 0 and look(rot=None) == 0
    for kw in (dict(n=1 << 31), dict(pos=None), dict(rad=None), dict(hq=None), dict(pos_out=None), dict(status_out=None), dict(skin=-0.01),
               dict(skin=math.nan), dict(skin=math.inf), dict(k=0), dict(k=9)):
        assert push(**kw) == E, kw
    for kw in (dict(n=1 << 31), dict(pos=None), dict(rad=None), dict(hq=None), dict(body_out=None), dict(depth_out=None), dict(gap=-0.01),
               dict(gap=math.nan), dict(gap=math.inf)):
        assert look(**kw) == E, kw
    n4, n5 = [None] * 4, [None] * 5
    assert w.lib.phys_depenetrate_device(w.h, n, *n4, 0.02, 4, *([None] * 7)) == E
    assert w.lib.phys_penetration_device(w.h, n, *n4, 0.02, *n5) == E
    # n == 0 is a no-op, whatever the pointers
    assert w.lib.phys_depenetrate(w.h, 0, *n4, 0.02, 4, *([None] * 7)) == 0 and w.lib.phys_depenetrate_device(w.h, 0, *n4, 0.02, 4, *([None] * 7)) == 0
    assert w.lib.phys_penetration(w.h, 0, *n4, 0.02, *n5) == 0 and w.lib.phys_penetration_device(w.h, 0, *n4, 0.02, *n5) == 0
    empty = w.depenetrate(np.zeros((0, 3), F), 0.25, 0.5)
    assert empty[0].shape == (0, 3) and empty[2].shape == (4, 0) and w.penetration(np.zeros((0, 3), F), 0.25, 0.5)[2].shape == (0, 3)
    # the Python surface refuses before the library is called
    for kw in (dict(skin=-1.0), dict(skin=math.nan), dict(max_iters=0), dict(max_iters=9), dict(rot=np.zeros((3, 4), F)), dict(ignore=np.zeros(3, np.uint32))):
        with pytest.raises(ValueError):
            w.depenetrate(a["pos"], a["rad"], a["hq"], **kw)
    with pytest.raises(ValueError):
        w.penetration(a["pos"], a["rad"], a["hq"], max_gap=-1.0)
    w.sync()


def test_invalid_queries_among_valid_ones(worlds):
    w = worlds("soup")
    c = cases.case("soup")
    n = 10
    pos = np.tile(c["pos"][0], (n, 1))
    rot = np.tile(np.array(IDENT, F), (n, 1))
    rad, hq = np.full(n, 0.25, F), np.full(n, 0.5, F)
    rad[:3] = [-1, np.nan, np.inf]
    hq[3:6] = [-1, np.nan, np.inf]
    rot[6, 2] = np.nan
    rot[7, 0] = np.inf
    pos[8, 1] = np.inf
    pos[9, 0] = np.nan
    pos, rot = np.vstack([pos, c["pos"][:5]]), np.vstack([rot, c["rot"][:5]])
    rad, hq = np.concatenate([rad, c["rad"][:5]]), np.concatenate([hq, c["hq"][:5]])
    with np.errstate(all="ignore"):
        got = w.depenetrate(pos, rad, hq, rot=rot, skin=SKIN, max_iters=3)
        b, d, nn = w.penetration(pos, rad, hq, rot=rot, max_gap=1.0)
    assert list(got[1][:n]) == [INVALID] * n and np.array_equal(_bits(got[0][:n]), _bits(pos[:n]))
    assert (got[2][:, :n] == MISS).all() and not got[3][:, :n].any() and not got[4][:, :n].any()
    assert (b[:n] == MISS).all() and (d[:n] == -np.inf).all() and not nn[:n].any()
    alone = w.depenetrate(pos[n:], rad[n:], hq[n:], rot=rot[n:], skin=SKIN, max_iters=3)
    _same(tuple(x[n:] if x.ndim < 2 or x.shape[0] == n + 5 else x[:, n:] for x in got), alone, "valid among invalid")


# ---- 6. no side effects ---------------------------------------------------------------------------------------------------------
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
    worlds = []
    for _ in range(2):
        w = pa.World(sc.config())
        sc.populate(w)
        worlds.append(w)
    quiet, probed = worlds
    rng = np.random.default_rng(3)
    lo, hi = sc.pos.min(0) - 1, sc.pos.max(0) + 1
    n = 2000
    pos = rng.uniform(lo, hi, (n, 3)).astype(F)
    tp = torch.from_numpy(pos).cuda()
    tr = torch.full((n,), 0.25, dtype=torch.float32, device="cuda")
    th = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    to = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ts = torch.empty(n, dtype=torch.int32, device="cuda")
    tdp = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    found = 0
    for k in range(8):
        for w in worlds:
            w.update_n(scenes.DT_NANOS, 2)
        status = probed.depenetrate(pos, 0.25, 0.5, skin=SKIN)[1]
        probed.penetration(pos, 0.25, 0.5, max_gap=0.1)
        probed.depenetrate_device(tp, tr, th, to, ts, skin=SKIN)
        probed.penetration_device(tp, tr, th, ts, tdp, max_gap=0.1)
        found += int(((status & 0xF) > 0).sum())
    for w in worlds:
        w.sync()
    a, b = _snapshot(quiet), _snapshot(probed)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    assert found > 0
    # after phys_set_body_poses moved a body onto a character, the probe reports that body
    quiet.close()
    probed.set_body_poses([0], pos=[[500.0, 500.0, 500.0]], rot=[IDENT])
    b, d, _ = probed.penetration([[500.0, 500.0, 500.0]], 0.25, 0.5, max_gap=0.0)
    assert b[0] == 0 and d[0] > 0.25
    out = probed.depenetrate([[500.0, 500.0, 500.0]], 0.25, 0.5, skin=SKIN)
    assert (out[1][0] & 0xF) >= 1 and out[2][0, 0] == 0 and not out[1][0] & STUCK
    probed.close()
