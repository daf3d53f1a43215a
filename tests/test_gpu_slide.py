"""GPU: move-and-slide (phys_move_and_slide and its device variant) on the seeded scenes of tests/slide_cases.py.

1. one launch equals the loop: a host loop of World.capsulecast calls with the spec header's steps between them
   (tests/slide_probe.py), bit for bit, over three scenes, five query counts, three slide counts, filters, ignore, the device
   variant and reversed order;
2. float64 properties that share no code with the kernels or the spec header (tests/capsulecast_ref.py);
3. closed forms: walls, creases, the ground, a grazed sphere, an overlapping start, too few slides;
4. refusals, n = 0, NULL outputs and INVALID queries;
5. no side effects on the updates, and the poses of phys_set_body_poses are seen."""
import math

import numpy as np
import pytest

import slide_cases as cases
import slide_probe as probe
from capsulecast_accept import tol_of
from query_accept import cast_cap

pytestmark = pytest.mark.gpu

F = np.float32
MISS, GROUND = 0xFFFFFFFE, 0xFFFFFFFF
BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
SKIN = F(cases.SKIN)
IDENT = [0.0, 0.0, 0.0, 1.0]
BOX = 2


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
    names = ("pos", "remaining", "status", "hit_body", "hit_normal", "hit_point")
    for name, x, y in zip(names, a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        diff = np.nonzero(_bits(x).reshape(-1) != _bits(y).reshape(-1))[0]
        assert len(diff) == 0, (what, name, len(diff), diff[:6], x.reshape(-1)[diff[:6]], y.reshape(-1)[diff[:6]])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return probe.build(str(tmp_path_factory.mktemp("slide") / "slide_probe"))


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


def _loop(exe, w, c, k, max_slides, skin=SKIN, rot=True, ignore=None, mask=None):
    """(one launch, the host loop of casts) for rows k of case c"""
    sub = lambda a: None if a is None else np.ascontiguousarray(a[k])
    pos, motion, rad, hq = sub(c["pos"]), sub(c["motion"]), sub(c["rad"]), sub(c["hq"])
    q = sub(c["rot"]) if rot else None
    ig = sub(ignore)
    m = mask if mask is None or np.ndim(mask) == 0 else sub(mask)
    got = w.move_and_slide(pos, motion, rad, hq, rot=q, skin=skin, max_slides=max_slides, ignore=ig, mask=m)

    def cast(origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        return w.capsulecast(origins, dirs, radius, half_length, rot=rot, max_t=max_t, ignore=ignore, mask=mask)

    want = probe.host_loop(exe, cast, pos, motion, rad, hq, q, skin, max_slides, ignore=ig, mask=m)
    return got, want


# ---- 1. one launch equals the loop, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_slides", [1, 4, 8])
@pytest.mark.parametrize("name", cases.SCENES)
def test_one_launch_equals_the_loop_of_casts(name, max_slides, exe, worlds):
    c = cases.case(name)
    got, want = _loop(exe, worlds(name), c, slice(None), max_slides)
    _same(got, want, f"{name} max_slides {max_slides}")
    status = got[2]
    hits = status & 0xF
    print(name, max_slides, "hits", np.bincount(hits, minlength=9), "blocked", int((status & BLOCKED != 0).sum()),
          "exhausted", int((status & EXHAUSTED != 0).sum()))
    assert got[3].shape == (max_slides, len(status)) and got[4].shape == (max_slides, len(status), 3)
    assert not (status & INVALID).any()
    # every slot: used below the hit count, empty from there on
    used = np.arange(max_slides)[:, None] < hits[None, :]
    assert ((got[3] != MISS) == used).all() and not got[4][~used].any() and not got[5][~used].any()
    if name == "soup":
        assert (hits >= 1).sum() > 250 and (max_slides == 1 or (hits >= 2).sum() > 20)
        assert (max_slides > 1) or (status & EXHAUSTED != 0).sum() > 100
    if name == "empty":
        assert not status.any() and np.array_equal(got[0], c["pos"] + c["motion"]) and not got[1].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_query_counts_around_the_workgroup_size(n, exe, worlds):
    c = cases.case("soup")
    got, want = _loop(exe, worlds("soup"), c, slice(100, 100 + n), 4)
    _same(got, want, f"n = {n}")
    assert n == 1 or (got[2] & 0xF).max() >= 2


def test_filters_ignore_and_upright(exe):
    c = cases.case("soup")
    cat, scat, gcat, masks, ignore = cases.filters()
    w = _world(*cases.scene("soup"))
    # ignore, and rot = None (every character upright: some now start inside something and are BLOCKED at once)
    got, want = _loop(exe, w, c, slice(None), 4, ignore=ignore)
    _same(got, want, "ignore")
    given = ignore != MISS + 1
    assert given.sum() > 100 and (got[3][:, given] != ignore[given][None, :]).all()
    plain = w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN)
    assert (plain[3][0][given] == ignore[given]).sum() > 50
    got, want = _loop(exe, w, c, slice(None), 4, rot=False)
    _same(got, want, "upright")
    # random categories, per-query masks
    w.set_body_filters(category=cat)
    w.set_static_filters(category=scat)
    w.set_ground_filter(gcat, 0xFFFF)
    got, want = _loop(exe, w, c, slice(None), 4, mask=masks)
    _same(got, want, "masks")
    body = got[3]
    for k in range(4):
        b, m = body[k], masks
        dyn = b < 300
        assert ((cat[b[dyn]] & m[dyn]) != 0).all()
        st = (b >= 0x80000000) & (b < MISS)
        assert ((scat[b[st] - 0x80000000] & m[st]) != 0).all()
        assert ((m[b == GROUND] & gcat) != 0).all()
    # a mask of all ones is the unfiltered instance's answer; mask 0 sees nothing
    _same(w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, mask=0xFFFF), plain, "mask 0xFFFF")
    none = w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, mask=0)
    assert not none[2].any() and np.array_equal(none[0], c["pos"] + c["motion"])
    w.close()


def test_device_variant_and_reversed_order(worlds):
    import torch
    c = cases.case("soup")
    w = worlds("soup")
    cat, scat, gcat, masks, ignore = cases.filters()
    n, k = len(c["pos"]), 4
    host = w.move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN, max_slides=k, ignore=ignore)
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()
    tp, tr = (torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
    ts = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    tb = torch.full((k, n), 7, dtype=torch.int32, device="cuda")
    tn, tq = (torch.full((k, n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    w.move_and_slide_device(dev(c["pos"]), dev(c["motion"]), dev(c["rad"]), dev(c["hq"]), tp, ts, tr, tb, tn, tq, rot=dev(c["rot"]),
                            skin=SKIN, max_slides=k, ignore=dev(ignore.view(np.int32)))
    w.sync()
    _same(host, tuple(x.cpu().numpy() for x in (tp, tr, ts, tb, tn, tq)), "device")
    # the device variant with a mask of all ones and without the optional outputs
    tp2, ts2 = torch.empty_like(tp), torch.empty_like(ts)
    w.move_and_slide_device(dev(c["pos"]), dev(c["motion"]), dev(c["rad"]), dev(c["hq"]), tp2, ts2, rot=dev(c["rot"]), skin=SKIN, max_slides=k,
                            ignore=dev(ignore.view(np.int32)), mask=dev(np.full(n, -1, np.int16)))
    w.sync()
    assert torch.equal(tp, tp2) and torch.equal(ts, ts2)
    # reversed order
    r = slice(None, None, -1)
    rev = w.move_and_slide(c["pos"][r], c["motion"][r], c["rad"][r], c["hq"][r], rot=c["rot"][r], skin=SKIN, max_slides=k, ignore=ignore[r])
    _same(host, tuple(x[r] if x.ndim < 2 or x.shape[0] == n else x[:, r] for x in rev), "reversed")


# ---- 2. float64 properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "statics"])
def test_float64_properties(name, worlds):
    c = cases.case(name)
    h = c["h"]
    n = len(c["pos"])
    pos_out, rem, status, body, nrm, pnt = worlds(name).move_and_slide(c["pos"], c["motion"], c["rad"], c["hq"], rot=c["rot"], skin=SKIN,
                                                                       max_slides=4)
    L = np.linalg.norm(c["motion"].astype(np.float64), axis=1)
    tol = np.array([1e-5 * (1.0 + np.abs(c["pos"][i]).max() + c["hq"][i] + L[i]) for i in range(n)])
    hits = status & 0xF
    sep = cases.separation(pos_out, c["rot"], c["rad"], c["hq"], c["tg"], c["ground"])
    moved = np.linalg.norm(pos_out.astype(np.float64) - c["pos"], axis=1)
    left = np.linalg.norm(rem.astype(np.float64), axis=1)
    print(name, "least separation", sep.min(), "worst moved - L", (moved - L).max(), "worst left - L", (left - L).max())
    assert (sep >= -tol).all(), np.nonzero(sep < -tol)[0][:8]
    assert (moved <= L + tol).all() and (left <= L + tol).all()
    free = ~(h["t"] <= L + float(SKIN) + 4 * tol)
    assert free.sum() > n // 4
    assert np.array_equal(pos_out[free], (c["pos"] + c["motion"])[free]) and not status[free].any() and not rem[free].any()
    early = np.nonzero(h["t"] < L - 4 * tol)[0]
    assert len(early) > (n // 3 if name == "soup" else n // 20)
    ties, bad = 0, []
    for i in early:
        if math.isfinite(h["t2"][i]) and h["t2"][i] - h["t"][i] <= 4 * tol_of(h, i):
            ties += 1
            continue
        ok = hits[i] >= 1 and int(body[0, i]) == int(h["body"][i]) and np.abs(nrm[0, i] - h["normal"][i]).max() <= 1e-4 \
            and np.abs(pnt[0, i] - h["point"][i]).max() <= tol[i]
        if not ok:
            bad.append((int(i), int(hits[i]), int(body[0, i]), int(h["body"][i]), nrm[0, i], h["normal"][i], pnt[0, i], h["point"][i]))
    print(name, len(early), "early hits,", ties, "near ties skipped")
    assert not bad, bad[:4]
    assert ties <= cast_cap(n)


# ---- 3. closed forms ------------------------------------------------------------------------------------------------------------
R, H = 0.25, 0.5


def _yquat(deg):
    a = math.radians(deg) / 2.0
    return [0.0, math.sin(a), 0.0, math.cos(a)]


def _walls(*faces):
    """static boxes of half extents (1, 50, 50): a wall per (point on its face, the turn about y that takes (-1, 0, 0) onto its
    outward normal); returns (statics, normals)"""
    pos, rot, normals = [], [], []
    for point, deg in faces:
        a = math.radians(deg)
        nrm = np.array([-math.cos(a), 0.0, math.sin(a)])  # R_y(deg) applied to (-1, 0, 0)
        pos.append(np.asarray(point, np.float64) - nrm)
        rot.append(_yquat(deg))
        normals.append(nrm)
    m = len(pos)
    return dict(pos=np.array(pos), rot=np.array(rot), shape=np.full(m, BOX), half_extent=np.tile([1.0, 50.0, 50.0], (m, 1))), normals


def _slide1(w, pos, motion, max_slides=4, skin=SKIN, rad=R, hq=H):
    out = w.move_and_slide(np.array([pos], F), np.array([motion], F), rad, hq, skin=skin, max_slides=max_slides)
    p0, m0 = np.array(pos, F).astype(np.float64), np.array(motion, F).astype(np.float64)
    L = np.linalg.norm(m0)
    hits = int(out[2][0]) & 0xF
    tol = (hits + 1) * 1e-5 * (1.0 + np.abs(p0).max() + hq + L)
    print(pos, motion, "->", out[0][0], out[1][0], hex(out[2][0]), out[3][:, 0], "tol", tol)
    return out[0][0].astype(np.float64), out[1][0].astype(np.float64), int(out[2][0]), out[3][:, 0], out[4][:, 0], out[5][:, 0], p0, m0, L, tol


def test_closed_forms_walls_and_creases():
    skin = float(SKIN)
    X = 4.0
    st, _ = _walls(([X, 0, 0], 0))
    w = _world(None, st, None)
    # oblique onto a wall: stops R + skin u_x short of it, and the tangential component arrives in full
    p, rem, status, body, nrm, _, p0, m0, L, tol = _slide1(w, [0.5, 1.0, -1.0], [5.0, 0.0, 3.0])
    u = m0 / L
    assert status == 1 and body[0] == 0x80000000 and np.abs(nrm[0] - [-1, 0, 0]).max() <= 1e-6 and not rem.any()
    assert abs(p[0] - (X - R - skin * u[0])) <= tol and abs(p[2] - (p0[2] + m0[2])) <= tol and abs(p[1] - p0[1]) <= tol
    # head-on: one hit, nothing left
    p, rem, status, body, _, _, p0, m0, L, tol = _slide1(w, [0.5, 1.0, -1.0], [6.0, 0.0, 0.0])
    assert status == 1 and not rem.any() and abs(p[0] - (X - R - skin)) <= tol and p[1] == p0[1] and p[2] == p0[2]
    w.close()
    # walls meeting at 60 degrees (the second wall's normal is (-1, 0, 0) turned by -120 degrees about y), motion with an upward
    # part: the wall, the second wall, then the crease: straight up along the vertical line
    Zc = 6.0
    for deg in (-120.0, -90.0):
        st, (nA, nB) = _walls(([X, 0, 0], 0), ([X, 0, Zc], deg))
        w = _world(None, st, None)
        start = [X - 3.0, 1.0, Zc - 2.5]
        p, rem, status, body, nrm, _, p0, m0, L, tol = _slide1(w, start, [5.0, 2.0, 3.0])
        assert status == 2 and list(body[:2]) == [0x80000000, 0x80000001] and not rem.any()
        assert np.abs(nrm[0] - nA).max() <= 1e-5 and np.abs(nrm[1] - nB).max() <= 1e-5
        u1 = m0 / L
        s1 = np.array([0.0, u1[1], u1[2]])
        u2 = s1 / np.linalg.norm(s1)
        assert abs(p[0] - (X - R - skin * u1[0])) <= tol                                      # the first stop's x is kept
        assert abs((p - [X, 0, Zc]) @ nB - (R + skin * abs(u2 @ nB))) <= tol               # the second stop's distance too
        assert abs(p[1] - (p0[1] + m0[1])) <= tol                                             # the rise arrives in full
        # with two casts only the rise is left over
        p2, rem2, status2, _, _, _, _, _, _, _ = _slide1(w, start, [5.0, 2.0, 3.0], max_slides=2)
        assert status2 == 2 | EXHAUSTED and rem2[1] > 0.1 and abs(rem2[0]) <= tol and abs(rem2[2]) <= tol
        assert abs(p2[1] + rem2[1] - p[1]) <= tol and np.abs(p2[[0, 2]] - p[[0, 2]]).max() <= tol
        w.close()
    # a corridor that takes three slides: the right-angled corner under a ceiling
    st, _ = _walls(([X, 0, 0], 0), ([X, 0, Zc], -90.0))
    Y = 4.6
    st = dict(pos=np.vstack([st["pos"], [0.0, Y + 1.0, 0.0]]), rot=np.vstack([st["rot"], IDENT]), shape=np.full(3, BOX),
              half_extent=np.vstack([st["half_extent"], [50.0, 1.0, 50.0]]))
    w = _world(None, st, None)
    start = [X - 3.0, 1.0, Zc - 2.5]
    p, rem, status, body, nrm, _, p0, m0, L, tol = _slide1(w, start, [5.0, 3.0, 2.5])
    assert status == 3 and list(body[:3]) == [0x80000000, 0x80000001, 0x80000002] and not rem.any()
    assert np.abs(nrm[2] - [0, -1, 0]).max() <= 1e-5 and abs(p[1] - (Y - R - H - skin)) <= tol
    p2, rem2, status2, body2, _, _, _, _, _, _ = _slide1(w, start, [5.0, 3.0, 2.5], max_slides=2)
    assert status2 == 2 | EXHAUSTED and rem2.any() and body2[1] == 0x80000001 and len(body2) == 2
    w.close()


def test_closed_forms_ground_sphere_and_overlap():
    skin = float(SKIN)
    ball = dict(pos=[[5.0, 3.0, 0.0]], rot=[IDENT], shape=[1], half_extent=[[1.0, 0.0, 0.0]])
    w = _world(ball, None, 0.0)
    # a level walk at skin above the ground: nothing is hit
    y0 = R + H + skin
    p, rem, status, _, _, _, p0, m0, L, tol = _slide1(w, [-3.0, y0, 4.0], [3.0, 0.0, 0.5])
    assert status == 0 and np.array_equal(p, p0 + m0) and not rem.any()
    # slightly downward: the ground, then level
    p, rem, status, body, nrm, pnt, p0, m0, L, tol = _slide1(w, [-3.0, R + H + 0.05, 4.0], [3.0, -0.1, 0.0])
    u = m0 / L
    assert status == 1 and body[0] == GROUND and list(nrm[0]) == [0.0, 1.0, 0.0] and not rem.any()
    assert abs(p[1] - (R + H + skin * abs(u[1]))) <= tol and abs(p[0] - (p0[0] + m0[0])) <= tol and p[2] == p0[2]
    assert abs(pnt[0][1]) <= tol
    # a sphere target (radius 1 at the height of the capsule's centre) passed with room to spare, then grazed: one hit, the slide
    # leaves along the tangent plane. In the plane of the centres this is a circle of radius 1 + R against a point.
    rr = 1.0 + R
    p, rem, status, _, _, _, p0, m0, L, tol = _slide1(w, [1.0, 3.0, rr + 0.03], [8.0, 0.0, 0.0])
    assert status == 0 and np.array_equal(p, p0 + m0)
    z0 = rr - 0.2
    p, rem, status, body, nrm, _, p0, m0, L, tol = _slide1(w, [1.0, 3.0, z0], [8.0, 0.0, 0.0])
    t = (5.0 - 1.0) - math.sqrt(rr * rr - z0 * z0)
    n = np.array([1.0 + t - 5.0, 0.0, z0]) / rr
    a = t - skin
    r = np.array([L - a, 0.0, 0.0])
    want = p0 + [a, 0, 0] + (r - n * (r @ n))
    assert status == 1 and body[0] == 0 and np.abs(nrm[0] - n).max() <= 1e-5 and not rem.any()
    assert np.abs(p - want).max() <= tol and np.linalg.norm(p - [5.0, 3.0, 0.0]) >= rr - tol
    # a start that overlaps: BLOCKED, one slot, nothing moves
    p, rem, status, body, nrm, pnt, p0, m0, L, tol = _slide1(w, [5.0, 3.0, 1.0], [1.0, 0.0, 2.0])
    assert status == 1 | BLOCKED and body[0] == 0 and list(body[1:]) == [MISS] * 3 and np.array_equal(p, p0) and np.array_equal(rem, m0)
    assert np.abs(nrm[0] + m0 / L).max() <= 1e-6 and not pnt.any()
    # skin 0 normally ends BLOCKED at the second cast
    p, rem, status, body, _, _, p0, m0, L, tol = _slide1(w, [-3.0, R + H + 0.05, 4.0], [3.0, -0.1, 0.0], skin=0.0)
    assert status in (2 | BLOCKED, 1) and abs(p[1] - (R + H)) <= tol
    w.close()


def test_long_thin_capsules_over_small_balls(exe):
    """the grid must be grown by R + h, not by R: long thin characters whose contacts lie far from their centre line"""
    import capsulecast_cases as cc
    c = cc.degenerate("long_thin")
    w = _world(c["bodies"], None, None)
    L = np.linalg.norm(c["d"].astype(np.float64), axis=1)
    motion = c["d"]
    got = w.move_and_slide(c["o"], motion, c["rad"], c["hq"], rot=c["rot"], skin=SKIN, max_slides=2)
    h = c["h"]
    early = np.nonzero(h["t"] < L - 1e-3)[0]
    assert len(early) > 40
    assert (got[3][0, early] == h["body"][early]).sum() >= len(early) - cast_cap(len(L))
    want = probe.host_loop(exe, lambda o, d, r, hl, **kw: w.capsulecast(o, d, r, hl, **kw), c["o"], motion, c["rad"], c["hq"], c["rot"], SKIN, 2)
    _same(got, want, "long thin")
    w.close()


# ---- 4. refusals and INVALID ----------------------------------------------------------------------------------------------------
def test_refusals_n_zero_and_null_outputs(worlds):
    from physics_amd import _abi
    w = worlds("soup")
    c = cases.case("soup")
    n = 64
    p = lambda x, t=_abi.f32p: None if x is None else x.ctypes.data_as(t)
    a = {k: np.ascontiguousarray(c[k][:n]) for k in ("pos", "motion", "rot", "rad", "hq")}
    full = w.move_and_slide(a["pos"], a["motion"], a["rad"], a["hq"], rot=a["rot"], skin=SKIN, max_slides=4)
    out = dict(pos_out=np.zeros((n, 3), F), status_out=np.zeros(n, np.uint32))

    def call(n=n, skin=float(SKIN), k=4, **kw):
        x = dict(a, **out)
        x.update(kw)
        return w.lib.phys_move_and_slide(w.h, n, p(x["pos"]), p(x["motion"]), p(x["rot"]), p(x["rad"]), p(x["hq"]), skin, k, None, None,
                                         p(x["pos_out"]), None, p(x["status_out"], _abi.u32p), None, None, None)

    E = _abi.PHYS_ERR_INVALID_ARG
    # NULL optional outputs: the call works and the others are as before
    assert call() == 0 and np.array_equal(_bits(out["pos_out"]), _bits(full[0])) and np.array_equal(out["status_out"], full[2])
    assert call(rot=None) == 0
    for kw in (dict(n=1 << 31), dict(pos=None), dict(motion=None), dict(rad=None), dict(hq=None), dict(skin=-0.01), dict(skin=math.nan),
               dict(skin=math.inf), dict(k=0), dict(k=9)):
        assert call(**kw) == E, kw
    x = dict(a, **out)
    assert w.lib.phys_move_and_slide(w.h, n, p(x["pos"]), p(x["motion"]), None, p(x["rad"]), p(x["hq"]), 0.02, 4, None, None, None, None,
                                     p(out["status_out"], _abi.u32p), None, None, None) == E
    assert w.lib.phys_move_and_slide(w.h, n, p(x["pos"]), p(x["motion"]), None, p(x["rad"]), p(x["hq"]), 0.02, 4, None, None, p(out["pos_out"]), None,
                                     None, None, None, None) == E
    assert w.lib.phys_move_and_slide_device(w.h, n, None, None, None, None, None, 0.02, 4, None, None, None, None, None, None, None, None) == E
    # n == 0 is a no-op, whatever the pointers
    assert w.lib.phys_move_and_slide(w.h, 0, None, None, None, None, None, 0.02, 4, None, None, None, None, None, None, None, None) == 0
    assert w.lib.phys_move_and_slide_device(w.h, 0, None, None, None, None, None, 0.02, 4, None, None, None, None, None, None, None, None) == 0
    empty = w.move_and_slide(np.zeros((0, 3), F), np.zeros((0, 3), F), 0.25, 0.5)
    assert empty[0].shape == (0, 3) and empty[3].shape == (4, 0)
    w.sync()


def test_invalid_queries(worlds):
    """The capsule cast test's kinds of invalid query: a bad radius, half-length (three each) or rot (two) and a non-finite dir; a
    zero motion is valid here and there is no max_t, so a non-finite pos and a motion beyond 3.0e38 stand in their place."""
    w = worlds("soup")
    c = cases.case("soup")
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
    # among valid ones, so that the grid is grown by theirs alone
    pos, motion, rot = np.vstack([pos, c["pos"][:5]]), np.vstack([motion, c["motion"][:5]]), np.vstack([rot, c["rot"][:5]])
    rad, hq = np.concatenate([rad, c["rad"][:5]]), np.concatenate([hq, c["hq"][:5]])
    with np.errstate(all="ignore"):
        got = w.move_and_slide(pos, motion, rad, hq, rot=rot, skin=SKIN, max_slides=3)
    assert list(got[2][:n]) == [INVALID] * n
    assert np.array_equal(_bits(got[0][:n]), _bits(pos[:n])) and np.array_equal(_bits(got[1][:n]), _bits(motion[:n]))
    assert (got[3][:, :n] == MISS).all() and not got[4][:, :n].any() and not got[5][:, :n].any()
    alone = w.move_and_slide(pos[n:], motion[n:], rad[n:], hq[n:], rot=rot[n:], skin=SKIN, max_slides=3)
    _same(tuple(x[n:] if x.ndim < 2 or x.shape[0] == n + 5 else x[:, n:] for x in got), alone, "valid among invalid")
    # a zero motion is valid: status 0, nothing moves
    z = w.move_and_slide(c["pos"][:3], np.zeros((3, 3), F), 0.25, 0.5)
    assert not z[2].any() and np.array_equal(z[0], c["pos"][:3]) and not z[1].any() and (z[3] == MISS).all()


# ---- 5. no side effects -----------------------------------------------------------------------------------------------------------
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
    lo, hi = sc.pos.min(0) - 3, sc.pos.max(0) + 3
    n = 2000
    pos = rng.uniform(lo, hi, (n, 3)).astype(F)
    motion = rng.normal(size=(n, 3)).astype(F) * 3
    tp, tm = torch.from_numpy(pos).cuda(), torch.from_numpy(motion).cuda()
    tr = torch.full((n,), 0.25, dtype=torch.float32, device="cuda")
    th = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    to = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ts = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    found = 0
    for k in range(8):
        for w in worlds:
            w.update_n(scenes.DT_NANOS, 2)
        status = probed.move_and_slide(pos, motion, 0.25, 0.5, skin=SKIN)[2]
        probed.move_and_slide_device(tp, tm, tr, th, to, ts, skin=SKIN)
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
    # after phys_set_body_poses the call sees the new poses: body 0 moved far away, alone in the character's way
    quiet.close()
    probed.set_body_poses([0], pos=[[500.0, 500.0, 500.0]], rot=[IDENT])
    out = probed.move_and_slide([[500.0, 500.0, 480.0]], [[0.0, 0.0, 30.0]], 0.25, 0.5, skin=SKIN)
    he = float(sc.half_extent[0][2]) if hasattr(sc, "half_extent") else None
    assert (out[2][0] & 0xF) >= 1 and out[3][0, 0] == 0 and 480.0 < out[0][0][2] < 500.0
    if he is not None:
        assert abs(out[0][0][2] - (500.0 - he - 0.25 - float(SKIN))) <= 1e-3
    probed.close()
