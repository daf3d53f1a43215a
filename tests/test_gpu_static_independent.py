"""GPU: the static-collider pair search (physics_amd/csrc/static.hip: k_static_count, k_static_scan, k_static_fill and the
visit they share) and its capacity protocol held to the numpy reference of tests/static_ref.py - the pair set by dense
comparison of the world's own body boxes (get_aabbs()) with the float32 static boxes the world uploads (written out by
tests/cpp/static_set_cli.cpp) - on scenes in which a body meets several statics in several cells, statics lie in several
cells, the LARGE list and the grid answer together, bodies reach outside the grid, the grid is coarsened to a thousand cells
on one axis, boxes touch exactly, and a lane has dozens of pairs. The scenes, and the case each one reaches, are checked
on the CPU in tests/test_static_ref_cpu.py. Counts and sets are compared exactly; manifold contents go through
shape_pair_ref.check, per kind and index order, with its tolerances as they are.

Two limits, both stated where they apply: shape_pair_ref's tolerances hold "on coordinates below ~100" (its docstring),
so in the `line` scenes, whose coordinates reach 1500 (a float32 ulp of 1.2e-4, above its TOL of 1e-4), the CONTENTS are
checked for the pairs within 100 of the origin (every other body is put there) and existence alone (with the same BAND)
for the others; and `touching` has
a margin of its own, so there existence alone is checked. The body path (statics as bodies n + k) is compared for every
scene but `mixed_1000` (BODY_PATH_LEFT_OUT), whose floor slab as a body would have 82 manifolds, past the 64 a body may have.

The solve against statics that several bodies share (a floor slab under a heap, a body in a corner) is held to float64 in
tests/test_gpu_solver_independent.py::test_heap_in_a_static_container_against_the_float64_solver. The 33k tower on the
cluster solver is not repeated there: test_gpu_static.py::test_every_solver_path_gives_the_same_bits_in_a_static_container
ties it to the paths checked there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pair_ref as pr
import shape_pair_ref as spr
import static_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 16_666_667
BIT = sr.STATIC_ID_BIT
NAMES = list(sr.SCENES)
NEAR = 100.0  # shape_pair_ref's tolerances are stated for coordinates below this
BODY_PATH_LEFT_OUT = ("mixed_1000",)  # its floor slab as a body would have 82 manifolds, past the 64 a body may have (the CPU
# oracle's count; test_static_ref_cpu.py holds it, and that no static of any other scene passes 64: mixed_257 43, only_large 58)
_KIND = {frozenset(v): k for k, v in spr.KINDS.items()}


# ---- shared with tests/test_static_ref_cpu.py (nothing here needs a GPU) ---------------------------------------------------
def build_cli(directory):
    exe = os.path.join(str(directory), "static_set_cli")
    # the flags of tests/test_pair_ref_cpu.py's build of grid_plan_cli
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "static_set_cli.cpp"), "-o", exe], check=True)
    return exe


def cli_boxes(exe, directory, tag, sc):
    """(float32 static boxes as the world uploads them, the grid figures) of a scene's static set"""
    src, dst = os.path.join(str(directory), tag + ".bin"), os.path.join(str(directory), tag + ".box")
    sr.write_static_file(src, sc["static"])
    facts = sr.parse_cli(subprocess.check_output([exe, src, repr(sc["margin"]), dst]).decode())
    return np.fromfile(dst, np.float32).reshape(-1, 6), facts


def by_kind(sc, pairs, idx):
    """{(kind, type of the body): [pair index]} - shape_pair_ref's checks run per kind and index order"""
    groups = {}
    for e in idx:
        ta, tb = int(sc["body"]["shape"][pairs[e, 0]]), int(sc["static"]["shape"][pairs[e, 1]])
        groups.setdefault((_KIND[frozenset((ta, tb))], ta), []).append(e)
    return groups


def check_manifolds(name, sc, pairs, man):
    """`man`: {(i, BIT | k): manifold} of one update from the poses of the scene. They join pairs of the reference only;
    every pair whose float64 gap is below -BAND has one and none whose gap is above margin + BAND; shape_pair_ref.check
    accepts the contents. Returns (contacts, clear misses, skipped or under an exception)."""
    margin = sc["margin"]
    want = {(int(i), BIT | int(k)) for i, k in pairs}
    stray = set(man) - want
    assert not stray, f"{name}: {len(stray)} manifolds that join no pair of the reference, e.g. {sorted(stray)[:3]}"
    A = spr.shapes(sc["body"]["shape"], sc["body"]["pos"], sc["body"]["rot"], sc["body"]["he"])
    B = spr.shapes(sc["static"]["shape"], sc["static"]["pos"], sc["static"]["rot"], sc["static"]["he"])
    contents = margin == spr.MARGIN
    near, hits, misses, skipped = [], 0, 0, 0
    for e, (i, k) in enumerate(pairs):
        a, b = A[i], B[k]
        if contents and max(np.abs(a.c).max(), np.abs(b.c).max()) < NEAR:
            near.append(e)
            continue
        gap = spr.pair_gap(a, b)[0]
        got = (int(i), BIT | int(k)) in man
        if gap < -spr.BAND:
            hits += 1
            assert got, f"{name}: body {i} and static {k} overlap by {-gap:.5f}, no manifold"
        elif gap > margin + spr.BAND:
            misses += 1
            assert not got, f"{name}: body {i} and static {k} are {gap:.5f} apart, yet a manifold"
        else:
            skipped += 1
    for (kind, ta), idx in sorted(by_kind(sc, pairs, near).items()):
        keys = [(int(pairs[e, 0]), BIT | int(pairs[e, 1])) for e in idx]
        rep = spr.check(kind, [A[pairs[e, 0]] for e in idx], [B[pairs[e, 1]] for e in idx], keys,
                        {k: man[k] for k in keys if k in man}, what=f"{name} {kind}, body of type {ta}")
        rep.assert_ok(shares=False)
        hits, misses, skipped = hits + rep.hits, misses + rep.misses, skipped + rep.skipped + rep.excepted
    total = max(len(pairs), 1)
    print(f"{name}: {len(pairs)} pairs ({len(near)} with contents checked): {hits} contacts ({hits / total:.1%}), {misses} clear misses "
          f"({misses / total:.1%}), {skipped} skipped or under an exception ({skipped / total:.1%})")
    assert skipped <= spr.MAX_SKIPPED * len(pairs)
    return hits, misses, skipped


# ---- the worlds ---------------------------------------------------------------------------------------------------------
def _pa():
    import physics_amd
    return physics_amd


def _world(sc, statics=True, body=None, **cfg):
    pa = _pa()
    kw = dict(flags=pa.FLAG_COLLISIONS, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0), contact_margin=sc["margin"])
    kw.update(cfg)
    w = pa.World(pa.default_config(**kw))
    b = body if body is not None else sc["body"]
    w.set_bodies(b["pos"], rot=b["rot"], shape_type=b["shape"], half_extent=b["he"], lin_vel=b.get("lin"))
    if statics:
        s = sc["static"]
        w.set_static_bodies(s["pos"], rot=s["rot"], shape_type=s["shape"], half_extent=s["he"])
    return w


def _static_manifolds(w):
    return {k: v for k, v in spr.manifolds_of(w).items() if k[1] & BIT and k[1] != 0xFFFFFFFF}


def _same(m1, m2):
    return set(m1) == set(m2) and all(m1[k][0] == m2[k][0] and np.array_equal(m1[k][1], m2[k][1]) and np.array_equal(m1[k][2], m2[k][2])
                                      for k in m1)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("static_set")
    exe = build_cli(d)
    _cache = {}

    def get(name):
        """One update of the scene from set_bodies + set_static_bodies, gravity off: everything the tests of (a) read."""
        if name in _cache:
            return _cache[name]
        sc = sr.scene(name)
        box, facts = cli_boxes(exe, d, name, sc)
        w = _world(sc)
        body_box = w.get_aabbs()
        w.update(DT)
        w.sync()
        r = dict(sc=sc, box=box, facts=facts, body_box=body_box, pairs=sr.static_pairs(body_box, box), stats=w.get_static_stats(),
                 man=_static_manifolds(w), overflow=w.get_stats().overflow)
        # a second update of the same world, the pair buffer now sized, from the poses the first one left (its solve moved
        # the bodies in contact): the count of the boxes of those poses
        r["second_box"] = w.get_aabbs()
        w.update(DT)
        w.sync()
        r["second_count"] = w.get_static_stats()[1]
        w.close()
        _cache[name] = r
        return r
    return get


def _write_pos(w, pos, rot=None):
    """positions (and rotations) through the device view (tests/test_gpu_raycast.py::test_current_poses_not_the_last_broad_phase)"""
    from physics_amd import _abi
    paths = _abi.rocm_runtime_mapped()
    assert paths, "no HIP runtime mapped"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    w.get_transforms()  # (waits for the world's stream; phys_sync would report the update's errors a second time)
    v = w.device_view()
    for dst, arr in ((v.pos, pos), (v.rot, rot)):
        if arr is not None:
            src = np.ascontiguousarray(arr, np.float32)
            assert hip.hipMemcpy(C.c_void_p(dst), src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0
    assert hip.hipDeviceSynchronize() == 0


# ---- (a) the pair set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pair_count_is_the_reference_count(name, run):
    r = run(name)
    n_static, n_pairs, n_man = r["stats"]
    print(f"{name}: {n_pairs} pairs, reference {len(r['pairs'])}; {n_man} static manifolds; grid {r['facts']['dim']}, "
          f"{r['facts']['n_large']} on the LARGE list")
    assert n_static == len(r["box"]) and r["overflow"] == 0
    assert len(r["pairs"]) == sr.SCENE_TABLE[name][0], "the boxes of the device are the CPU checker's: the table's count"
    assert n_pairs == len(r["pairs"])
    assert n_man == len(r["man"])
    # the second update of the same world, its pair buffer sized by the first
    assert r["second_count"] == len(sr.static_pairs(r["second_box"], r["box"]))


@pytest.mark.parametrize("name", NAMES)
def test_static_manifolds_join_reference_pairs_and_hold_to_float64(name, run):
    r = run(name)
    hits, misses, _ = check_manifolds(name, r["sc"], r["pairs"], r["man"])
    if sr.SCENE_TABLE[name][8]:
        assert hits >= spr.MIN_CONTACTS * len(r["pairs"]) and misses >= spr.MIN_MISSES * len(r["pairs"])
    assert hits >= 1


@pytest.mark.parametrize("name", [n for n in NAMES if n not in BODY_PATH_LEFT_OUT])
def test_the_body_path_gives_the_same_bits(name, run):
    """A second world holds the statics as bodies n + k: its manifold (i, n + k) has the bits of (i, BIT | k)."""
    r = run(name)
    sc = r["sc"]
    b, s = sc["body"], sc["static"]
    n, ns = len(b["pos"]), len(s["pos"])
    both = {k: np.concatenate([b[k], s[k]]) for k in ("pos", "rot", "shape", "he")}
    w = _world(sc, statics=False, body=both, max_pairs=64 * (n + ns), max_manifolds=32 * (n + ns))
    w.update(DT)
    w.sync()
    man = spr.manifolds_of(w)
    w.close()
    keys = [(int(i), BIT | int(k)) for i, k in r["pairs"]]
    same = spr.check_same(r["man"], keys, man, [(int(i), n + int(k)) for i, k in r["pairs"]], f"{name} static vs body path")
    same.assert_ok(shares=False)
    assert same.hits == len(r["man"]) >= 1


@pytest.mark.parametrize("name", NAMES)
def test_empty_ghost_slots_change_nothing(name, run):
    """max_ghosts > 0 and nothing exchanged: the ghost slots hold inverted boxes, the lanes of k_static_count run over
    them, and count and manifolds are those of the plain world."""
    r = run(name)
    w = _world(r["sc"], max_ghosts=100)
    w.update(DT)
    w.sync()
    assert w.get_static_stats() == r["stats"]
    assert _same(_static_manifolds(w), r["man"])
    w.close()


@pytest.mark.parametrize("name", ["tiles_65", "mixed_257"])
def test_update_n_gives_the_manifolds_of_two_single_updates(name, run):
    sc = run(name)["sc"]
    body = dict(sc["body"], lin=np.tile(np.float32([0.3, 0.0, -0.2]), (len(sc["body"]["pos"]), 1)))
    res = []
    for twice in (False, True):
        w = _world(sc, body=body)
        if twice:
            w.update_n(DT, 2)
        else:
            w.update(DT)
            w.update(DT)
        w.sync()
        res.append((w.get_static_stats(), _static_manifolds(w), w.get_transforms()[0]))
        w.close()
    assert res[0][0] == res[1][0] and res[0][0][2] >= 10
    assert _same(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2])
    assert not _same(res[0][1], run(name)["man"]), "the bodies moved: the second update's manifolds are not the first's"


# ---- (b) the capacity protocol -----------------------------------------------------------------------------------------------
def test_pairs_beyond_the_buffer_are_reported_once_and_the_next_update_has_room(run):
    """tiles(257) with the bodies 3 above the floor: the first update measures no pairs and the buffer gets its floor of
    max(4 n, 1024) = 1028. The bodies are then put onto the tiles behind the world's back: the update overflows (every store
    of k_static_fill is guarded by `at < cap`), says so once, and the next one has room."""
    pa = _pa()
    r = run("tiles_257")
    sc, box = r["sc"], r["box"]
    n = len(sc["body"]["pos"])
    vel = np.tile(np.float32([0.25, 0.0, -0.125]), (n, 1))
    up = dict(sc["body"], pos=sc["body"]["pos"] + np.float32([0.0, 3.0, 0.0]), lin=vel)
    w = _world(sc, body=up)
    w.update(DT)
    w.sync()
    assert w.get_static_stats()[1] == 0 and max(4 * n, 1024) == 1028
    down = sc["body"]["pos"]
    _write_pos(w, down)
    now = w.get_aabbs()
    want = sr.static_pairs(now, box)
    ulps = pr.ulp_error(now, r["body_box"]).max()
    print(f"boxes of the poses written back: up to {ulps:.3g} ulps from the boxes of set_bodies; {len(want)} pairs, there {len(r['pairs'])}")
    assert len(want) > 1028 + 500
    rot = w.get_transforms()[1]
    lin0, ang0 = w.get_velocities()
    here = dict(sc, body=dict(sc["body"], rot=rot))  # (bodies that touch each other were turned by the first update's solve)
    # update 2: more pairs than the buffer holds
    w.update(DT)
    assert w.get_stats().overflow & 1
    with pytest.raises(pa.PhysError) as e:
        w.sync()
    assert e.value.code == pa._abi.PHYS_ERR_CAPACITY
    # the bits of the LAST update stay in phys_stats.overflow until the next update (the header says so), and a phys_sync
    # with no update in between reports them again; "once" is that the sync behind update 3 below is clean
    assert w.get_stats().overflow & 1
    with pytest.raises(pa.PhysError) as e:
        w.sync()
    assert e.value.code == pa._abi.PHYS_ERR_CAPACITY
    assert w.get_static_stats()[1] == len(want), "the full count, not the stored one"
    lin, ang = w.get_velocities()
    pos, _ = w.get_transforms()
    assert np.array_equal(lin, lin0) and np.array_equal(ang, ang0), "the solve was skipped"
    moved = pos.astype(np.float64) - down
    assert np.abs(moved - lin0.astype(np.float64) * (DT * 1e-9)).max() < 1e-6, "the bodies were integrated"
    # update 3 from the same poses (the skipped solve left the spin of the bodies that touch: they turned): room for all
    _write_pos(w, down, rot)
    assert np.array_equal(w.get_aabbs().view(np.uint32), now.view(np.uint32))
    w.update(DT)
    w.sync()
    assert w.get_stats().overflow == 0
    assert w.get_static_stats()[1] == len(want)
    man = _static_manifolds(w)
    hits, misses, _ = check_manifolds("tiles_257 behind an overflow", here, want, man)
    assert len(man) >= 500 and hits >= spr.MIN_CONTACTS * len(want) and misses >= spr.MIN_MISSES * len(want)
    assert w.get_static_stats()[2] == len(man)
    lin, _ = w.get_velocities()
    assert (np.abs(lin - lin0).max(axis=1) > 1e-3).sum() >= 100, "this time the solve ran"
    w.close()
