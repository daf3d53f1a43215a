"""GPU: the sharding kernels of physics_amd/csrc/halo.hip against the numpy reference of tests/halo_ref.py, which is
written from the header's contracts and shares no code with the kernels. Two worlds on one GPU play two ranks (cut
plane x = 0, ownership by centre, gids 2i and 2j + 1 so that both emit); the "all-gather" is a device copy. Everything
is a gather or a comparison, so everything is compared exactly: record sets and ghost slots as bits, pair sets as sets.
The boxes come from get_aabbs() of the world under test; the conditions the inputs must meet are checked on the CPU in
tests/test_halo_ref_cpu.py and, where they hang on the world's own cell, again here.

The wide-record tests fail on the commit before the sweep of k_halo_pairs was made complete (it stopped after 8 cells
per axis): there the local rank of the slot-grid scene found 1 489 of its 2 051 pairs and that of the sorted-grid scene
2 070 of 2 775. The two capacity tests fail there too: a synchronous call that followed one that
overflowed reported that overflow again."""
import ctypes as C

import numpy as np
import pytest

import halo_ref as hr

pytestmark = pytest.mark.gpu
ERR_CAPACITY = -5


def _pa():
    import physics_amd
    return physics_amd


def _world(rank, max_ghosts=0):
    pa = _pa()
    flags = pa.FLAG_COLLISIONS | (0 if max_ghosts else pa.FLAG_BROADPHASE_ONLY)
    w = pa.World(pa.default_config(flags=flags, gravity_offset=(0, 0, 0), max_ghosts=max_ghosts,
                                   max_pairs=max(24 * rank.n, 65536)))  # room for the pairs of a clump
    w.set_bodies(rank.pos, shape_type=rank.shape, half_extent=rank.half)
    w.set_global_ids(rank.gid)
    return w


def _device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return t


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _d2h(ptr, offset_bytes, shape, dtype):
    """Device memory of a phys_device_view pointer -> numpy (the world is idle: every caller synchronised it)."""
    from physics_amd import _abi
    paths = _abi.rocm_runtime_mapped()
    assert paths, "no HIP runtime mapped"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(shape, dtype)
    base = C.cast(ptr, C.c_void_p).value
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(base + offset_bytes), out.nbytes, 2) == 0
    return out


def _sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


def _check_pairs(w, records_dev, n_records, expect, skip_first=0, skip_count=0):
    n = w.halo_pairs(records_dev.data_ptr(), n_records, skip_first, skip_count)
    got = w.get_cross_pairs()
    assert n == len(got) == w.get_stats().n_cross_pairs
    assert len(np.unique(got, axis=0)) == len(got), "a cross pair twice"
    missing = len(set(map(tuple, expect.tolist())) - set(map(tuple, got.tolist())))
    assert np.array_equal(got, expect), f"{len(got)} pairs, expected {len(expect)}; {missing} expected pairs missing"


class Exchange:
    """Two ranks as worlds after one broad phase, what each packs with the all-reduced reach (device buffers), and what
    the reference expects of both calls."""

    def __init__(self, ranks, cap):
        self.ranks, self.cap = ranks, cap
        self.worlds = [_world(r) for r in ranks]
        for w in self.worlds:
            w.broadphase()
        self.aabbs = [w.get_aabbs() for w in self.worlds]
        self.cells = [np.float32(w.get_stats().max_extent) * np.float32(1.001) for w in self.worlds]
        for a, r, c in zip(self.aabbs, ranks, self.cells):
            assert c == hr.cell_size(a, r.shape)
        self.reach = max(self.cells)  # the all-reduce of phys_stats.max_extent the contract asks for
        self.records, self.pairs = hr.expected_exchange(ranks, self.aabbs, self.reach)
        import torch
        self.bufs, self.counts = [], []
        for w, r in zip(self.worlds, ranks):
            buf = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self.counts.append(w.halo_pack(r.x_lo, r.x_hi, float(self.reach), buf.data_ptr(), cap))
            self.bufs.append(buf)

    def check_pack(self):
        for buf, n, rec in zip(self.bufs, self.counts, self.records):
            got = _host(buf)
            assert n == len(rec) and np.array_equal(_sorted_rows(got[:n]), _sorted_rows(rec))
            assert (got[n:] == hr.EMPTY).all()

    def check_pairs(self, least=100):
        for k, w in enumerate(self.worlds):
            assert len(self.pairs[k]) >= least, "a rank that emits nothing checks nothing"
            _check_pairs(w, self.bufs[1 - k], self.cap, self.pairs[k])

    def close(self):
        for w in self.worlds:
            w.close()


# ---- AABB records: pack ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [0.5, 0.0])
def test_pack_is_the_reference_record_set(reach):
    for rank in (hr.pack_rank(True), hr.pack_rank(False)):
        w = _world(rank)
        w.broadphase()
        aabb = w.get_aabbs()
        eff = np.float32(reach) if reach > 0 else np.float32(w.get_stats().max_extent) * np.float32(1.001)
        expect = hr.pack_records(aabb, rank.shape, rank.gid, rank.x_lo, rank.x_hi, eff)
        assert 0.10 * rank.n <= len(expect) <= 0.60 * rank.n
        cap = 2048
        buf = _device(np.full((cap, 8), 0x5A5A5A5A, np.uint32))
        n = w.halo_pack(rank.x_lo, rank.x_hi, reach, buf.data_ptr(), cap)
        got = _host(buf)
        assert n == len(expect) == w.get_stats().n_halo_records
        assert (got[:n, 7] == 0).all(), "pad"
        assert np.array_equal(_sorted_rows(got[:n, [6, 0, 1, 2, 3, 4, 5]]), _sorted_rows(expect[:, [6, 0, 1, 2, 3, 4, 5]]))
        assert (got[n:] == hr.EMPTY).all(), "the tail is empty records"
        w.close()


def test_pack_beyond_its_capacity_reports_it_and_stays_inside():
    rank = hr.pack_rank(True)
    w = _world(rank)
    w.broadphase()
    need = len(hr.pack_records(w.get_aabbs(), rank.shape, rank.gid, rank.x_lo, rank.x_hi, 0.5))
    cap = need - 37
    buf = _device(np.full((cap + 64, 8), 0x5A5A5A5A, np.uint32))
    with pytest.raises(_pa().PhysError) as e:
        w.halo_pack(rank.x_lo, rank.x_hi, 0.5, buf.data_ptr(), cap)
    assert e.value.code == ERR_CAPACITY
    got = _host(buf)
    assert (got[cap:] == 0x5A5A5A5A).all(), "rows behind the capacity were written"
    assert (got[:cap, 6] != hr.EMPTY).all() and (got[:cap, 7] == 0).all()
    # the same call with room, right after: it reports its own overflow only
    assert w.halo_pack(rank.x_lo, rank.x_hi, 0.5, buf.data_ptr(), cap + 64) == need
    w.close()


# ---- AABB records: pairs -----------------------------------------------------------------------------------------------
# 'sorted' is k_halo_pairs<false> because hr.N_SORTED lies above kSlotGridMaxBodies of physics_amd/csrc/plan.hpp, 'slots'
# is k_halo_pairs<true> because hr.N_SLOTS does not: tests/test_halo_ref_cpu.py reads the constant and holds both to it.
@pytest.mark.parametrize("kind", ["slots", "sorted"])
def test_cross_pairs_of_uniform_sizes(kind):
    ex = Exchange([hr.local_rank(kind), hr.neighbour_rank(0)], cap=4096)
    ex.check_pack()
    assert sum(len(p) for p in ex.pairs) >= 500
    ex.check_pairs()
    ex.close()


@pytest.mark.parametrize("kind", ["slots", "sorted"])
def test_cross_pairs_with_records_wider_than_eight_cells(kind):
    """The neighbour holds a few boxes of half extent 3 beside bodies of 0.2 - 0.3: their records span 11 of the local
    rank's cells per axis. Every local body they overlap must be found, also those beyond the eighth cell."""
    ex = Exchange([hr.local_rank(kind), hr.neighbour_rank(hr.N_GIANTS)], cap=24576)  # half the sorted world is within reach
    assert float(ex.reach) > 6.0 and float(ex.cells[0]) < 0.7
    beyond = hr.cells_beyond_clamp(ex.aabbs[0], ex.records[1], ex.pairs[0], ex.cells[0])
    assert beyond.sum() >= 50, "the scene does not reach beyond the eighth cell"
    ex.check_pack()
    ex.check_pairs()
    ex.close()


def test_bodies_of_the_slot_grids_overflow_list_pair_once():
    local, neighbour, cluster = hr.overflow_scene()
    ex = Exchange([local, neighbour], cap=512)
    centre = np.float32(0.5) * (ex.aabbs[0][:, :3] + ex.aabbs[0][:, 3:])
    cells = np.floor(centre * (np.float32(1.0) / ex.cells[0])).astype(int)
    assert (cells[cluster] == cells[cluster[0]]).all() and len(cluster) >= 9 + 8, "more centres in one cell than a bucket has slots"
    assert set(cluster) <= set(ex.pairs[0][:, 0].tolist()) and len(ex.pairs[0]) >= 500
    ex.check_pairs(least=1)  # the neighbour's few pairs are checked too; the crowded bucket is the local rank's
    ex.close()


def test_skip_window_in_the_middle_and_empty_records_between_live_ones():
    """[neighbour A | own | neighbour B]: the own block holds this rank's own records, which overlap its own bodies and
    must be skipped; A and B hold the neighbour's records with an empty record after every live one."""
    ex = Exchange([hr.local_rank("slots"), hr.neighbour_rank(0)], cap=4096)
    cap = ex.cap
    rec = ex.records[1]
    half = len(rec) // 2
    assert 2 * half <= cap
    gathered = np.full((3 * cap, 8), hr.EMPTY, np.uint32)
    gathered[0:2 * half:2] = rec[:half]
    gathered[cap:cap + len(ex.records[0])] = ex.records[0]
    gathered[2 * cap + 1:2 * cap + 1 + 2 * (len(rec) - half):2] = rec[half:]
    unskipped = hr.cross_pairs(ex.aabbs[0], ex.ranks[0].gid, ex.ranks[0].shape, gathered)
    assert len(unskipped) > len(ex.pairs[0]) + 100, "the own block would have given pairs"
    expect = hr.cross_pairs(ex.aabbs[0], ex.ranks[0].gid, ex.ranks[0].shape, gathered, cap, cap)
    assert np.array_equal(expect, ex.pairs[0])
    _check_pairs(ex.worlds[0], _device(gathered), 3 * cap, expect, cap, cap)
    ex.close()


def test_cross_pairs_beyond_their_capacity_are_reported_and_the_next_call_is_right():
    local, neighbour = hr.clump_scene()
    ex = Exchange([local, neighbour], cap=256)
    assert len(ex.pairs[0]) == 64 * 200
    w = ex.worlds[0]
    with pytest.raises(_pa().PhysError) as e:
        w.halo_pairs(ex.bufs[1].data_ptr(), ex.cap)
    assert e.value.code == ERR_CAPACITY
    # no broad phase or update in between: a call reports its own overflow only
    few = hr.record_buffer(ex.records[1][:40], ex.cap)
    _check_pairs(w, _device(few), ex.cap, hr.cross_pairs(ex.aabbs[0], local.gid, local.shape, few))
    assert len(w.get_cross_pairs()) == 64 * 40
    # what overflowed is still owed to phys_sync, once
    assert w.get_stats().overflow & 8
    with pytest.raises(_pa().PhysError) as e:
        w.sync()
    assert e.value.code == ERR_CAPACITY
    w.sync()
    assert w.get_stats().overflow == 0
    ex.close()


# ---- ghost records -----------------------------------------------------------------------------------------------------
def _ghost_world(b, max_ghosts):
    pa = _pa()
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS, gravity_offset=(0, 0, 0), max_ghosts=max_ghosts))
    w.set_bodies(b["pos"], rot=b["rot"], lin_vel=b["lin"], ang_vel=b["ang"], mass=b["mass"], inertia=b["inertia"],
                 shape_type=b["shape"], half_extent=b["half"])
    w.set_global_ids(b["gid"])
    w.set_body_filters(b["category"], b["mask"], b["group"])
    w.set_slab(*hr.GHOST_SLAB)
    return w


def test_pack_bodies_is_the_reference_buffer_byte_for_byte():
    import torch
    b = hr.ghost_bodies()
    x_lo, x_hi, reach = hr.GHOST_SLAB
    w = _ghost_world(b, 64)
    cap = 32768
    for face in (0, -1, +1):
        expect = hr.body_records(b["pos"], b["rot"], b["lin"], b["ang"], b["inv_mass"], b["half"], b["shape"], b["gid"],
                                 b["inv_inertia"], (b["category"], b["mask"], b["group"]), x_lo, x_hi, reach, face)
        assert 5000 < len(expect) < cap
        assert face != 0 or expect[-1, 17] > 3 * 65536 + 3 * 256, "records from behind workgroup 256"
        buf = torch.zeros((cap, 24), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if face == 0:
            w.halo_pack_bodies(buf.data_ptr(), cap)
        else:
            w.halo_pack_bodies_face(buf.data_ptr(), cap, face)
        w.sync()
        assert w.get_stats().n_halo_records == len(expect)
        got = _host(buf)
        want = hr.record_buffer(expect, cap)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, f"face {face}: {len(bad)} records differ, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    w.close()


def test_unpack_fills_the_ghost_slots_in_record_order_field_by_field():
    pa = _pa()
    recs, skip_first, skip_count, _ = hr.ghost_record_blocks()
    x_lo, x_hi, reach = hr.GHOST_SLAB
    G, n_owned = 45000, 100
    owned = hr.ghost_bodies(n=n_owned)
    w = _ghost_world(owned, G)
    dev = _device(recs)
    g = hr.ghost_slots(recs, skip_first, skip_count, x_lo, x_hi, reach, G)
    m = len(g["index"])
    assert 30000 < m < G

    def check(g, m):
        w.sync()
        assert w.get_stats().n_ghosts == m
        gids = w.get_global_ids()
        assert np.array_equal(gids[:n_owned], owned["gid"])
        assert np.array_equal(gids[n_owned:n_owned + m], g["gid"]), "ghost order"
        assert (gids[n_owned + m:] == hr.EMPTY).all()
        v = w.device_view()
        assert v.vel_stride == 8
        assert np.array_equal(_d2h(v.pos, 12 * n_owned, (m, 3), np.uint32), g["pos"].view(np.uint32))
        assert np.array_equal(_d2h(v.rot, 16 * n_owned, (m, 4), np.uint32), g["rot"].view(np.uint32))
        vel = np.concatenate([g["lin"], g["inv_mass"][:, None], g["ang"], g["mass"][:, None]], 1).astype(np.float32)
        assert np.array_equal(_d2h(v.lin_vel, 32 * n_owned, (m, 8), np.uint32), vel.view(np.uint32))
        # the broad phase sees a ghost as it sees an owned body of the same pose, shape and half extent
        w.broadphase()
        ghost_aabb = _d2h(v.aabb, 24 * n_owned, (G, 6), np.float32)
        plain = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_BROADPHASE_ONLY, gravity_offset=(0, 0, 0)))
        plain.set_bodies(g["pos"], rot=g["rot"], shape_type=g["shape"], half_extent=g["half_extent"])
        assert np.array_equal(ghost_aabb[:m].view(np.uint32), plain.get_aabbs().view(np.uint32))
        plain.close()
        assert (ghost_aabb[m:, :3] > ghost_aabb[m:, 3:]).all(), "an empty ghost slot has no shape: the inverted box"

    w.halo_unpack_ghosts(dev.data_ptr(), len(recs), skip_first, skip_count)
    check(g, m)
    # fewer records: the slots they no longer fill are empty again
    fewer = 20000
    g2 = hr.ghost_slots(recs[:fewer], 0, 0, x_lo, x_hi, reach, G)
    assert 5000 < len(g2["index"]) < m - 5000
    w.halo_unpack_ghosts(dev.data_ptr(), fewer, 0, 0)
    check(g2, len(g2["index"]))
    w.close()
