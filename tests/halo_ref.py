"""The sharding kernels of physics_amd/csrc/halo.hip in plain numpy, written from the contracts in
include/physics_hip.h (the halo section) and from the record layout above `struct BodyRecord`. Every operation is a
gather or a comparison, so everything here is exact: records are compared as bits. Imports numpy only.

Also the input builders of tests/test_gpu_halo_independent.py, so that tests/test_halo_ref_cpu.py can check on the CPU
that those inputs reach the cases they are meant to reach."""
import numpy as np

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, 1, 2, 3
EMPTY = 0xFFFFFFFF
MARGIN = 0.02                       # phys_config.contact_margin's default
FILTER_DEFAULT_WORD = 0xFFFF0001    # category 0x0001 | mask 0xFFFF << 16
FAR = np.float32(3.0e38)            # where phys_halo_pack_bodies_face moves the other face
F32 = np.float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _bits(a):
    return _f32(a).view(np.uint32)


# ---- 32-byte AABB records ---------------------------------------------------------------------------------------------
def pack_records(aabb, shape, gid, x_lo, x_hi, reach):
    """(k, 8) uint32: {lo xyz, hi xyz, gid, pad = 0} of the bodies with a shape whose box comes within `reach` of a slab
    face, in body order (the device appends them in any order: compare as a set)."""
    aabb = _f32(aabb).reshape(-1, 6)
    lo_x, hi_x = aabb[:, 0], aabb[:, 3]
    take = (np.asarray(shape) != SHAPE_NONE) & ((lo_x < F32(x_lo) + F32(reach)) | (hi_x > F32(x_hi) - F32(reach)))
    idx = np.nonzero(take)[0]
    out = np.zeros((len(idx), 8), np.uint32)
    out[:, :6] = aabb[idx].view(np.uint32)
    out[:, 6] = np.asarray(gid, np.uint32)[idx]
    return out


def cross_pairs(local_aabb, local_gid, local_shape, records, skip_first=0, skip_count=0, chunk=2048):
    """(m, 2) uint32 {local index, record gid}, sorted: every local body with a shape against every live record outside
    [skip_first, skip_first + skip_count), closed-interval overlap on all three axes, kept where the local gid is the
    smaller one."""
    box = _f32(local_aabb).reshape(-1, 6)
    gid = np.asarray(local_gid, np.uint32)
    records = np.asarray(records, np.uint32).reshape(-1, 8)
    k = np.arange(len(records))
    live = ((k < skip_first) | (k >= skip_first + skip_count)) & (records[:, 6] != EMPTY)
    rec = records[live]
    rbox = np.ascontiguousarray(rec[:, :6]).view(np.float32)
    rgid = rec[:, 6]
    has_shape = np.asarray(local_shape) != SHAPE_NONE
    out = []
    for s in range(0, len(box), chunk):
        b = box[s:s + chunk]
        hit = has_shape[s:s + chunk, None] & (gid[s:s + chunk, None] < rgid[None, :])
        for a in range(3):
            hit &= (b[:, None, a] <= rbox[None, :, 3 + a]) & (rbox[None, :, a] <= b[:, None, 3 + a])
        i, j = np.nonzero(hit)
        out.append(np.stack([(i + s).astype(np.uint32), rgid[j]], 1))
    out = np.concatenate(out) if out else np.zeros((0, 2), np.uint32)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def cell_size(aabb, shape):
    """The grid cell a world derives from its boxes: the largest edge of a body with a shape, times 1.001 (float32)."""
    aabb = _f32(aabb).reshape(-1, 6)[np.asarray(shape) != SHAPE_NONE]
    return F32((aabb[:, 3:] - aabb[:, :3]).max()) * F32(1.001)


def _cell_coord(c, cell):
    return np.floor(_f32(c) * (F32(1.0) / F32(cell))).astype(np.int64)


def cells_beyond_clamp(local_aabb, records, pairs, cell):
    """For each pair of `pairs` (local index, record gid): does the cell of the local body's box centre lie more than 7
    cells above the first cell of the record's sweep (lo - cell / 2) on some axis? An 8-cell sweep cannot reach it."""
    box = _f32(local_aabb).reshape(-1, 6)
    records = np.asarray(records, np.uint32).reshape(-1, 8)
    records = records[records[:, 6] != EMPTY]
    order = np.argsort(records[:, 6])
    row = order[np.searchsorted(records[order, 6], pairs[:, 1])]
    rbox = np.ascontiguousarray(records[row, :6]).view(np.float32)
    b = box[pairs[:, 0]]
    centre = F32(0.5) * (b[:, :3] + b[:, 3:])
    first = _cell_coord(rbox[:, :3] - F32(0.5) * F32(cell), cell)
    return ((_cell_coord(centre, cell) - first) > 7).any(axis=1)


def scene_aabbs(pos, shape, half, margin=MARGIN):
    """Boxes of unrotated boxes and of spheres as the world fattens them (float32, the same order of operations); a body
    without a shape has the inverted box that overlaps nothing."""
    pos, half, shape = _f32(pos), _f32(half), np.asarray(shape)
    e = np.where((shape == SHAPE_SPHERE)[:, None], half[:, :1], half)
    out = np.concatenate([(pos - e) - F32(margin), (pos + e) + F32(margin)], 1)
    out[shape == SHAPE_NONE] = [3.0e38] * 3 + [-3.0e38] * 3
    return _f32(out)


def brute_pairs(aabb, shape):
    """Sorted (i, j), i < j, of one scene: the closed-interval overlap over every pair of bodies with a shape."""
    box = _f32(aabb).reshape(-1, 6)
    ok = np.asarray(shape) != SHAPE_NONE
    hit = ok[:, None] & ok[None, :]
    for a in range(3):
        hit &= (box[:, None, a] <= box[None, :, 3 + a]) & (box[None, :, a] <= box[:, None, 3 + a])
    i, j = np.nonzero(np.triu(hit, 1))
    return np.stack([i, j], 1).astype(np.uint32)


# ---- 96-byte body records ---------------------------------------------------------------------------------------------
def body_records(pos, rot, lin, ang, inv_mass, half_extent, shape, gid, inv_inertia, filters, x_lo, x_hi, reach, face=0):
    """(k, 24) uint32, in body order: the records of the bodies with a shape whose centre lies within `reach` of a slab
    face (strictly). face > 0: the high face only, < 0: the low face only. inv_inertia is (n, 9), filters is
    (category, mask, group) per body.
      words 0-2 pos, 3-6 rot ijkw, 7-9 lin, 10-12 ang, 13-15 half extent, 16 shape, 17 gid, 18 inverse mass,
      19 full-inertia flag | group << 16, 20-22 inverse inertia diagonal, 23 (category | mask << 16) ^ the default word"""
    pos = _f32(pos).reshape(-1, 3)
    lo = -FAR if face > 0 else F32(x_lo)
    hi = FAR if face < 0 else F32(x_hi)
    x = pos[:, 0]
    take = (np.asarray(shape) != SHAPE_NONE) & ((x < lo + F32(reach)) | (x > hi - F32(reach)))
    idx = np.nonzero(take)[0]
    I = _f32(inv_inertia).reshape(-1, 9)[idx]
    cat, mask, group = (np.asarray(f)[idx] for f in filters)
    full = (I[:, [1, 2, 3, 5, 6, 7]] != 0).any(axis=1)
    out = np.zeros((len(idx), 24), np.uint32)
    out[:, 0:3] = _bits(pos[idx])
    out[:, 3:7] = _bits(_f32(rot).reshape(-1, 4)[idx])
    out[:, 7:10] = _bits(_f32(lin).reshape(-1, 3)[idx])
    out[:, 10:13] = _bits(_f32(ang).reshape(-1, 3)[idx])
    out[:, 13:16] = _bits(_f32(half_extent).reshape(-1, 3)[idx])
    out[:, 16] = np.asarray(shape, np.uint32)[idx]
    out[:, 17] = np.asarray(gid, np.uint32)[idx]
    out[:, 18] = _bits(_f32(inv_mass)[idx])
    out[:, 19] = full.astype(np.uint32) | (group.astype(np.int64) & 0xFFFF).astype(np.uint32) << np.uint32(16)
    out[:, 20:23] = _bits(I[:, [0, 4, 8]])
    out[:, 23] = (cat.astype(np.uint32) | mask.astype(np.uint32) << np.uint32(16)) ^ np.uint32(FILTER_DEFAULT_WORD)
    return out


def record_buffer(records, cap):
    """`records` at the front of a buffer of `cap` rows, the rest empty (every byte 0xFF)."""
    out = np.full((cap, records.shape[1]), EMPTY, np.uint32)
    out[:len(records)] = records
    return out


def ghost_slots(records, skip_first, skip_count, x_lo, x_hi, reach, max_ghosts):
    """The records that become ghosts, in record order: not in the skip window, not empty, centre within `reach` of the
    slab (inclusive). Returns a dict: index (rows of `records`), pos, rot, lin, ang, inv_mass, mass, gid, shape,
    half_extent. A record with the full-inertia flag, or whose inverse mass is not above 0, is kinematic: inverse mass 0,
    mass +inf; every other has mass 1 / inverse mass in float32."""
    rec = np.asarray(records, np.uint32).reshape(-1, 24)
    f = rec.view(np.float32)
    k = np.arange(len(rec))
    x = f[:, 0]
    take = ((k < skip_first) | (k >= skip_first + skip_count)) & (rec[:, 17] != EMPTY)
    with np.errstate(invalid="ignore"):
        take &= (x >= F32(x_lo) - F32(reach)) & (x <= F32(x_hi) + F32(reach))
    idx = np.nonzero(take)[0][:max_ghosts]
    g = f[idx]
    inv_mass = g[:, 18].copy()
    kinematic = ((rec[idx, 19] & 1) != 0) | ~(inv_mass > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mass = (F32(1.0) / inv_mass).astype(np.float32)
    inv_mass[kinematic] = 0.0
    mass[kinematic] = np.inf
    return dict(index=idx, pos=g[:, 0:3].copy(), rot=g[:, 3:7].copy(), lin=g[:, 7:10].copy(), ang=g[:, 10:13].copy(),
                inv_mass=inv_mass, mass=mass, gid=rec[idx, 17].copy(), shape=rec[idx, 16].copy(),
                half_extent=g[:, 13:16].copy())


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------
DENSITY = 3.0   # bodies per unit volume: a body of edge ~0.55 then overlaps three or four others
SIDE = 31.0     # the y and z range every slab of a pairs scene fills
N_SORTED, N_SLOTS, N_NEIGHBOUR, N_GIANTS = 33000, 3000, 4000, 8


def small_bodies(rng, n, x_from, x_to, none_every=0, side=SIDE, sizes=(0.2, 0.3)):
    """n spheres and unrotated boxes with half extents in `sizes`, centres uniform in the slab [x_from, x_to) x
    [0, side)^2. none_every: every so-manieth body has no shape."""
    pos = np.stack([rng.uniform(x_from, x_to, n), rng.uniform(0, side, n), rng.uniform(0, side, n)], 1).astype(np.float32)
    pos[:, 0] = np.clip(pos[:, 0], x_from, np.nextafter(F32(x_to), F32(x_from)))
    shape = np.where(rng.random(n) < 0.5, SHAPE_SPHERE, SHAPE_BOX).astype(np.uint32)
    half = rng.uniform(sizes[0], sizes[1], (n, 3)).astype(np.float32)
    half[0] = sizes[1]   # the cell size does not hang on the draw (nor on the order: some body has the largest box)
    if none_every:
        shape[5::none_every] = SHAPE_NONE
    return pos, shape, half


class Rank:
    """One rank's bodies: pos, shape, half, gid, its slab [x_lo, x_hi] and its boxes as computed here."""

    def __init__(self, pos, shape, half, gid, x_lo, x_hi):
        self.pos, self.shape, self.half, self.gid = _f32(pos), shape.astype(np.uint32), _f32(half), gid.astype(np.uint32)
        self.x_lo, self.x_hi = x_lo, x_hi
        self.aabb = scene_aabbs(self.pos, self.shape, self.half)
        self.n = len(self.pos)


def local_rank(kind, seed=1, none_every=0):
    """The rank in x < 0 of a pairs scene, gids 2i. kind 'sorted': N_SORTED bodies, more than the slot grid takes, ordered
    by distance from the cut so that the bodies at the cut hold the smallest gids (they then emit against every record
    of the neighbour's last bodies); 'slots': N_SLOTS bodies in a slab four cells deep."""
    n = N_SORTED if kind == "sorted" else N_SLOTS
    rng = np.random.default_rng(seed)
    pos, shape, half = small_bodies(rng, n, -n / (DENSITY * SIDE * SIDE), 0.0, none_every)
    if kind == "sorted":
        order = np.argsort(-pos[:, 0], kind="stable")
        pos, shape, half = pos[order], shape[order], half[order]
    return Rank(pos, shape, half, 2 * np.arange(n), -1.0e6, 0.0)


def neighbour_rank(giants=0, seed=2, none_every=0):
    """The rank in x >= 0, gids 2j + 1: N_NEIGHBOUR small bodies, then `giants` boxes of half extent 3 whose centres lie
    just behind the cut and spread over the cross-section."""
    rng = np.random.default_rng(seed)
    n = N_NEIGHBOUR
    pos, shape, half = small_bodies(rng, n, 0.0, n / (DENSITY * SIDE * SIDE), none_every)
    if giants:
        side = int(np.ceil(np.sqrt(giants)))
        gy, gz = np.divmod(np.arange(giants), side)
        gpos = np.stack([np.full(giants, 0.5), (gy + 0.5) * SIDE / side, (gz + 0.5) * SIDE / side], 1)
        pos = np.concatenate([pos, gpos.astype(np.float32)])
        shape = np.concatenate([shape, np.full(giants, SHAPE_BOX, np.uint32)])
        half = np.concatenate([half, np.full((giants, 3), 3.0, np.float32)])
    return Rank(pos, shape, half, 2 * np.arange(len(pos)) + 1, 0.0, 1.0e6)


def pack_rank(low, seed=7):
    """A rank of the pack tests: 3000 bodies (eleven workgroups and a last wave of 56 lanes), every seventh without a
    shape, in a slab 2.5 deep on the low (x < 0) or the high side of the cut."""
    rng = np.random.default_rng(seed + low)
    pos, shape, half = small_bodies(rng, 3000, -2.5 if low else 0.0, 0.0 if low else 2.5, none_every=7, side=20.0)
    return Rank(pos, shape, half, 2 * np.arange(3000) + (0 if low else 1), -1.0e6 if low else 0.0, 0.0 if low else 1.0e6)


def all_reduced_reach(*aabbs_and_shapes):
    """What the ranks agree on as `reach`: the largest cell of any of them."""
    return max(cell_size(a, s) for a, s in aabbs_and_shapes)


def expected_exchange(ranks, aabbs, reach):
    """Two ranks, their boxes (the world's own, or scene_aabbs) and the agreed reach -> (records, pairs): what each rank
    packs, and the cross pairs each finds in the other's records."""
    records = [pack_records(a, r.shape, r.gid, r.x_lo, r.x_hi, reach) for r, a in zip(ranks, aabbs)]
    pairs = [cross_pairs(aabbs[k], ranks[k].gid, ranks[k].shape, records[1 - k]) for k in range(2)]
    return records, pairs


def overflow_scene(seed=3):
    """(local, neighbour, cluster): a slot-grid world of 300 small bodies in x < -2 plus `cluster` = its first 20 bodies,
    whose box centres all fall in the grid cell (-1, 3, 3) next to the cut - more than the 8 slots of a bucket - and a
    neighbour of 200 bodies packed around that cell behind the cut. The cell is the one this scene's boxes give."""
    rng = np.random.default_rng(seed)
    pos, shape, half = small_bodies(rng, 320, -6.0, -2.0)
    cell = float(cell_size(scene_aabbs(pos, shape, half), shape))
    at = np.array([-1.0, 3.0, 3.0]) * cell
    pos[:20] = (at + rng.uniform(0.15, 0.85, (20, 3)) * cell).astype(np.float32)
    local = Rank(pos, shape, half, 2 * np.arange(320), -1.0e6, 0.0)
    npos, nshape, nhalf = small_bodies(rng, 200, 0.0, 0.3)
    npos[:, 1:] = (at[1:] + rng.uniform(-0.5, 1.5, (200, 2)) * cell).astype(np.float32)
    return local, Rank(npos, nshape, nhalf, 2 * np.arange(200) + 1, 0.0, 1.0e6), np.arange(20)


def clump_scene(seed=4):
    """64 bodies in a clump at the cut and 200 neighbours whose boxes overlap every one of them, with larger gids:
    12800 cross pairs on the local rank, more than the 4096 a world of 64 bodies has room for."""
    rng = np.random.default_rng(seed)
    pos = (np.array([-0.3, 5.0, 5.0]) + rng.uniform(-0.05, 0.05, (64, 3))).astype(np.float32)
    local = Rank(pos, np.full(64, SHAPE_BOX, np.uint32), np.full((64, 3), 0.25, np.float32), 2 * np.arange(64), -1.0e6, 0.0)
    npos = (np.array([0.1, 5.0, 5.0]) + rng.uniform(0.0, 0.05, (200, 3))).astype(np.float32)
    neighbour = Rank(npos, np.full(200, SHAPE_SPHERE, np.uint32), np.full((200, 3), 0.25, np.float32),
                     2 * np.arange(200) + 129, 0.0, 1.0e6)
    return local, neighbour


def exact_inverse_inertia(rng, n, full_every):
    """(inertia, inverse), both (n, 9) float32, whose inversion is exact in float32 whatever the formula: diagonals of
    powers of two, and every full_every-th body s * [[2, 1, 0], [1, 1, 0], [0, 0, 1]] with inverse
    [[1, -1, 0], [-1, 2, 0], [0, 0, 1]] / s."""
    d = np.exp2(rng.integers(-2, 3, (n, 3))).astype(np.float32)
    inertia = np.zeros((n, 9), np.float32)
    inertia[:, [0, 4, 8]] = d
    inverse = np.zeros((n, 9), np.float32)
    inverse[:, [0, 4, 8]] = F32(1.0) / d
    full = np.arange(n) % full_every == 3
    s = d[full, :1]
    inertia[full] = s * np.array([2, 1, 0, 1, 1, 0, 0, 0, 1], np.float32)
    inverse[full] = np.array([1, -1, 0, -1, 2, 0, 0, 0, 1], np.float32) / s
    return inertia, inverse


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


GHOST_SLAB = (-8.0, 8.0, 2.0)   # x_lo, x_hi, reach of the ghost tests
N_GHOST_BODIES = 70000          # > 65536: the workgroups behind number 256 take the second trip of the ordered compaction


def ghost_bodies(seed=5, n=None):
    """The owned bodies of the pack-bodies test, as a dict of set_bodies / set_body_filters arguments plus what the
    record holds of them (inv_mass, inv_inertia): centres uniform in the slab, some exactly on x = -6 and x = 6 (not
    boundary bodies: the comparison is strict), all three shapes and some without, some full inertia tensors, filters
    with negative groups."""
    rng = np.random.default_rng(seed)
    n = N_GHOST_BODIES if n is None else n
    x_lo, x_hi, reach = GHOST_SLAB
    pos = np.stack([rng.uniform(x_lo, x_hi, n), rng.uniform(-200, 200, n), rng.uniform(-200, 200, n)], 1).astype(np.float32)
    pos[7::97, 0] = x_lo + reach
    pos[11::97, 0] = x_hi - reach
    pos[13::97, 0] = np.nextafter(F32(x_lo + reach), F32(-100))   # the last float inside reach
    pos[17::97, 0] = np.nextafter(F32(x_hi - reach), F32(100))
    # about a third within reach of a face: the middle is thinned out
    middle = (np.abs(pos[:, 0]) < 6.0) & (rng.random(n) < 0.13)
    pos[middle, 0] = np.where(rng.random(middle.sum()) < 0.5, -1.0, 1.0) * rng.uniform(6.01, 8.0, middle.sum())
    shape = rng.integers(1, 4, n).astype(np.uint32)
    shape[3::11] = SHAPE_NONE
    mass = np.exp2(rng.integers(-2, 3, n)).astype(np.float32) * rng.uniform(1.0, 2.0, n).astype(np.float32)
    inertia, inverse = exact_inverse_inertia(rng, n, 13)
    return dict(pos=pos, rot=random_rotations(rng, n), lin=rng.normal(size=(n, 3)).astype(np.float32),
                ang=rng.normal(size=(n, 3)).astype(np.float32), mass=mass, inv_mass=(F32(1.0) / mass).astype(np.float32),
                inertia=inertia, inv_inertia=inverse, shape=shape, half=rng.uniform(0.2, 0.5, (n, 3)).astype(np.float32),
                gid=(3 * np.arange(n) + 1).astype(np.uint32),
                category=rng.integers(1, 0x10000, n).astype(np.uint16), mask=rng.integers(0, 0x10000, n).astype(np.uint16),
                group=rng.integers(-0x8000, 0x8000, n).astype(np.int16))


def ghost_record_blocks(seed=6):
    """(records (70000, 24) uint32, skip_first, skip_count, n_live): a gathered buffer of three blocks
    [neighbour A: 30000 | own: 10000 | neighbour B: 30000], each with live records in front and an empty tail. The
    centres run from x = -14 to 14 around the slab [-8, 8] with reach 2, some exactly on -10 and 10 (taken) and on the floats just
    outside (not taken); some records with inverse mass 0 and some with the full-inertia flag."""
    rng = np.random.default_rng(seed)
    blocks, live = (30000, 10000, 30000), (26000, 9000, 28500)
    n = sum(live)
    x_lo, x_hi, reach = GHOST_SLAB
    pos = np.stack([rng.uniform(-14, 14, n), rng.uniform(-200, 200, n), rng.uniform(-200, 200, n)], 1).astype(np.float32)
    pos[5::89, 0] = x_lo - reach
    pos[9::89, 0] = x_hi + reach
    pos[14::89, 0] = np.nextafter(F32(x_lo - reach), F32(-100))
    pos[19::89, 0] = np.nextafter(F32(x_hi + reach), F32(100))
    inv_mass = (F32(1.0) / rng.uniform(0.3, 5.0, n).astype(np.float32)).astype(np.float32)
    inv_mass[4::17] = 0.0
    _, inverse = exact_inverse_inertia(rng, n, 19)
    recs = body_records(pos, random_rotations(rng, n), rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), inv_mass,
                        rng.uniform(0.2, 0.5, (n, 3)), rng.integers(1, 4, n), 5 * np.arange(n) + 2, inverse,
                        (rng.integers(1, 0x10000, n), rng.integers(0, 0x10000, n), rng.integers(-0x8000, 0x8000, n)),
                        -1.0e30, 1.0e30, 1.0e31)   # every body is a "boundary body" of this make-believe sender
    assert len(recs) == n
    out, at = [], 0
    for cap, k in zip(blocks, live):
        out.append(record_buffer(recs[at:at + k], cap))
        at += k
    return np.concatenate(out), blocks[0], blocks[1], n
