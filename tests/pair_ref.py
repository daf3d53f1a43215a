"""Reference of the broad phase for tests/test_gpu_pairs_independent.py: the fattened boxes in float64 and the pair set
by sort-and-sweep, written from the definitions in the ABI header (shapes, half extents, contact margin) and sharing no
code with the collision header or the CPU checker; numpy only. Also the scenes of those tests, and a numpy model of the
uniform grid (cell of a box, bucket table split, brick regions) that tests/test_pair_ref_cpu.py uses to show that every
scene reaches the case it is named for.

    aabbs(pos, rot, shape, he, margin)   float64 boxes [lo xyz, hi xyz]; NaN rows for bodies without a shape
        sphere    centre +- (r + margin),                          r = he[0]
        box       centre +- (|R| he + margin)
        capsule   centre +- (|he[1] R[:, 1]| + r + margin),        r = he[0], core half-length he[1] along local y
        R is the matrix of the quaternion [i, j, k, w] AS GIVEN, not normalised (the library never normalises a rotation
        it is handed: a quaternion of norm s scales the box by s^2).
    pairs(aabb)                          {(i, j), i < j: closed intervals overlap on all three axes}, sorted, from the
                                         boxes as given (float32 from the device; an inverted or NaN box meets nobody)

TOLERANCE of the boxes, in float32 ulps of max(1, |coordinate|): the worst deviation of the CPU checker's get_aabbs()
(bit-equal to the device) from aabbs() over every scene below, measured by tests/test_pair_ref_cpu.py, never against a
kernel; the GPU gets four times that.

    measured 2.47 ulps (sparse / far / farther 2.461, clump 2.402, many_pairs 2.328, dense 2.316, thin_flat 2.300, thin_tall 2.100,
    few_pairs 2.048; every deviation is also a shortfall: some face lies that far INSIDE the float64 box)
    -> tolerance 9.88 ulps, for the deviation and for the shortfall

Pair counts of the scenes (n = 33 000, seeds as committed; on the CPU, from the checker's boxes; SCENE_TABLE below, held by
test_pair_ref_cpu.py), the bucket table grid_plan gives them and the cells they use, and the bricks in use whose region
(6 x 6 x 5 cells) holds at most the 1024 records staged without a hint (staged) or more (walked in global memory):

    scene         pairs  per body   table (cells)   cells in use   bricks staged / not   records per region
    sparse        35 673    1.08    64 x 32 x 64    22 x 22 x 22        216 / 0              101 - 651
    thin_tall    571 704   17.32    64 x 64 x 32     4 x 106 x 4          8 / 56             832 - 3417
    thin_flat     42 559    1.29    64 x 32 x 64    72 x 2 x 72         512 / 0              152 - 668
    dense      1 006 287   30.49    32 x 64 x 64     8 x 8 x 8            0 / 8             6439 - 8465
    clump        131 383    3.98    64 x 64 x 32    24 x 24 x 24        212 / 4              173 - 3526
    few_pairs     85 912    2.60    64 x 64 x 32    16 x 16 x 16         24 / 40             681 - 1515
    many_pairs   273 970    8.30    64 x 32 x 64    12 x 12 x 12         32 / 32             175 - 4827
    far           35 705    1.08    64 x 32 x 64    23 x 22 x 23        254 / 0                1 - 648
    farther       35 637    1.08    64 x 32 x 64    22 x 22 x 22        216 / 0               78 - 658

With a hint (after an update) the stage holds a quarter more than the largest region met, up to 5000 records: then only
`dense` still has unstaged bricks - all of its eight.
"""
import numpy as np

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, 1, 2, 3
MARGIN = 0.02  # phys_config.contact_margin's default
N = 33000      # the smallest round size above the slot grid's 32768 bodies

MEASURED_AABB_ULPS = 2.47
# name -> (pairs, bricks staged, bricks not staged)
SCENE_TABLE = {"sparse": (35673, 216, 0), "thin_tall": (571704, 8, 56), "thin_flat": (42559, 512, 0), "dense": (1006287, 0, 8),
               "clump": (131383, 212, 4), "few_pairs": (85912, 24, 40), "many_pairs": (273970, 32, 32), "far": (35705, 254, 0),
               "farther": (35637, 216, 0)}
AABB_TOL_ULPS = 4.0 * MEASURED_AABB_ULPS

FAR_SHIFT = (60000.0, 0.0, -60000.0)
FARTHER_SHIFT = (200000.0, 0.0, -200000.0)


# ------------------------------------------------------------------------------------------------ the reference
def rotation_matrices(rot):
    """(n, 3, 3) float64 matrices of quaternions [i, j, k, w], not normalised."""
    q = np.asarray(rot, np.float64).reshape(-1, 4)
    i, j, k, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = w * w + i * i - j * j - k * k
    R[:, 0, 1] = 2 * (i * j - w * k)
    R[:, 0, 2] = 2 * (i * k + w * j)
    R[:, 1, 0] = 2 * (i * j + w * k)
    R[:, 1, 1] = w * w - i * i + j * j - k * k
    R[:, 1, 2] = 2 * (j * k - w * i)
    R[:, 2, 0] = 2 * (i * k - w * j)
    R[:, 2, 1] = 2 * (j * k + w * i)
    R[:, 2, 2] = w * w - i * i - j * j + k * k
    return R


def aabbs(pos, rot, shape, he, margin=MARGIN):
    c = np.asarray(pos, np.float64).reshape(-1, 3)
    h = np.asarray(he, np.float64).reshape(-1, 3)
    shape = np.asarray(shape)
    R = np.abs(rotation_matrices(rot))
    e = np.full_like(c, np.nan)
    s, b, k = shape == SHAPE_SPHERE, shape == SHAPE_BOX, shape == SHAPE_CAPSULE
    e[s] = h[s, :1]
    e[b] = np.einsum("nab,nb->na", R[b], h[b])
    e[k] = R[k][:, :, 1] * h[k, 1:2] + h[k, :1]
    e += float(margin)
    return np.concatenate([c - e, c + e], axis=1)


def pairs(aabb, chunk=1 << 22):
    """Sort-and-sweep along the axis the boxes spread most on: behind a box in the order of the lower faces, every box
    whose lower face is not above this one's upper face is a candidate; the other two axes decide."""
    box = np.asarray(aabb)
    lo, hi = box[:, :3], box[:, 3:]
    live = (lo <= hi).all(axis=1)  # an inverted box (no shape) or a NaN row meets nobody
    ids = np.nonzero(live)[0]
    if len(ids) < 2:
        return np.zeros((0, 2), np.uint32)
    lo, hi = lo[ids], hi[ids]
    axis = int(np.argmax(lo.max(axis=0).astype(np.float64) - lo.min(axis=0)))
    order = np.argsort(lo[:, axis], kind="stable")
    lo, hi, ids = lo[order], hi[order], ids[order]
    n = len(ids)
    end = np.searchsorted(lo[:, axis], hi[:, axis], side="right")  # closed intervals: touching counts
    count = np.maximum(end - np.arange(1, n + 1), 0)
    start = np.concatenate([[0], np.cumsum(count)])
    o1, o2 = [a for a in range(3) if a != axis]
    out = []
    a0 = 0
    while a0 < n:
        a1 = int(np.searchsorted(start, start[a0] + chunk, side="right")) - 1
        a1 = min(max(a1, a0 + 1), n)
        cnt = count[a0:a1]
        total = int(cnt.sum())
        if total:
            i = np.repeat(np.arange(a0, a1), cnt)
            j = np.arange(total) - np.repeat(start[a0:a1] - start[a0], cnt) + i + 1
            keep = (lo[i, o1] <= hi[j, o1]) & (lo[j, o1] <= hi[i, o1])
            i, j = i[keep], j[keep]
            keep = (lo[i, o2] <= hi[j, o2]) & (lo[j, o2] <= hi[i, o2])
            out.append(np.stack([ids[i[keep]], ids[j[keep]]], axis=1))
        a0 = a1
    if not out:
        return np.zeros((0, 2), np.uint32)
    p = np.concatenate(out)
    p = np.stack([p.min(axis=1), p.max(axis=1)], axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.uint32)


def brute_pairs(aabb):
    """The definition, O(n^2): for the test of pairs() itself."""
    box = np.asarray(aabb)
    lo, hi = box[:, None, :3], box[None, :, 3:]
    meet = (lo <= hi).all(axis=2)          # meet[i, j]: lo_i <= hi_j on every axis
    both = meet & meet.T
    i, j = np.nonzero(np.triu(both, 1))
    return np.stack([i, j], axis=1).astype(np.uint32)


def ulp_error(value, ref):
    """|value - ref| in float32 ulps of max(1, |ref|), elementwise."""
    ref = np.asarray(ref, np.float64)
    unit = np.spacing(np.maximum(1.0, np.abs(ref)).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(value, np.float64) - ref) / unit


def box_errors(got, ref, shape):
    """(worst deviation, worst shortfall) of float32 boxes from the float64 ones, both in ulps, over the bodies with a
    shape: the shortfall is how far a face of `got` lies INSIDE the reference box (a box too small loses contacts)."""
    has = np.asarray(shape) != SHAPE_NONE
    g, r = np.asarray(got, np.float64)[has], np.asarray(ref, np.float64)[has]
    unit = np.spacing(np.maximum(1.0, np.abs(r)).astype(np.float32)).astype(np.float64)
    inside = np.concatenate([g[:, :3] - r[:, :3], r[:, 3:] - g[:, 3:]], axis=1) / unit
    return float((np.abs(g - r) / unit).max()), float(max(inside.max(), 0.0))


# ------------------------------------------------------------------------------------------------ the scenes
# name -> (seed, half-box of the body centres, share of the bodies in a clump and the clump's half-box,
#          half extent given to the bodies WITHOUT a shape, shift of the whole scene)
# Shapes: one in 16 none, the others sphere / box / capsule in equal shares; random unit rotations (rounded to float32: as
# given, norm 1 to a few 1e-8); half extents 0.3 - 1.2 per component. The half extent of a body without a shape means
# nothing to the broad phase - no box, no cell - but the split of the bucket table over the axes, made once per body set
# from the uploaded half extents, reads it: in the two `thin` scenes those bodies carry 500, the split comes out nearly
# even, and the scene is longer than the table on its long axes (far cells share buckets).
SCENES = {
    "sparse": (1, (50.0, 50.0, 50.0), 0.0, None, None, None),
    "thin_tall": (2, (5.0, 250.0, 5.0), 0.0, None, 500.0, None),
    "thin_flat": (3, (170.0, 3.0, 170.0), 0.0, None, 500.0, None),
    "dense": (4, (16.0, 16.0, 16.0), 0.0, None, None, None),
    "clump": (5, (55.0, 55.0, 55.0), 0.1, (7.0, 7.0, 7.0), None, None),
    "few_pairs": (6, (37.0, 37.0, 37.0), 0.0, None, None, None),
    "many_pairs": (7, (25.0, 25.0, 25.0), 0.0, None, None, None),
    "far": (1, (50.0, 50.0, 50.0), 0.0, None, None, FAR_SHIFT),
    # with these extents the cell is 4.7 wide: at 60 000 the cell index is 12 700 and the float32 product centre x 1 / cell
    # has an ulp of 2^-10, just under the 0.1 % the cell is wider than the widest box. At 200 000 the index passes 2^15 and
    # the ulp is four times that slack
    "farther": (1, (50.0, 50.0, 50.0), 0.0, None, None, FARTHER_SHIFT),
}
MAX_PAIRS = {"dense": 1 << 21}  # the default capacity of 24 pairs per body holds the others


def scene(name, n=N):
    seed, half, clump_share, clump_half, none_he, shift = SCENES[name]
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half)
    if clump_share:
        m = int(n * clump_share)
        pos[:m] = rng.uniform(-1.0, 1.0, (m, 3)) * np.asarray(clump_half) + np.asarray(half) * 0.5
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    he = rng.uniform(0.3, 1.2, (n, 3))
    shape = rng.integers(1, 4, n).astype(np.uint32)
    shape[rng.permutation(n)[: n // 16]] = SHAPE_NONE
    if none_he:
        he[shape == SHAPE_NONE] = none_he
    if shift:
        pos += np.asarray(shift)
    return dict(pos=pos.astype(np.float32), rot=q.astype(np.float32), shape=shape, he=he.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the grid, as the header says
def cell_size(aabb, shape):
    """Edge of the grid cell: the largest box edge of the bodies with a shape, times 1.001, in float32."""
    box = np.asarray(aabb, np.float32)[np.asarray(shape) != SHAPE_NONE]
    return np.float32((box[:, 3:] - box[:, :3]).max()) * np.float32(1.001)


def cells(aabb, shape):
    """(ids, integer cell per axis) of the bodies with a shape: floor(centre / cell), float32 arithmetic throughout."""
    ids = np.nonzero(np.asarray(shape) != SHAPE_NONE)[0]
    box = np.asarray(aabb, np.float32)[ids]
    inv = np.float32(1.0) / cell_size(aabb, shape)
    centre = np.float32(0.5) * (box[:, :3] + box[:, 3:])
    return ids, np.floor(centre * inv).astype(np.int64)


def brick_regions(cell, axis_cells, brick=(4, 4, 4), region=(6, 6, 5)):
    """Per occupied brick of the wrapped grid (axis_cells per axis): (records in the brick, records in its region). The
    region of a brick is the brick and its half-shell halo: one cell below and above on x and y, one above on z."""
    dims = tuple(int(a) for a in axis_cells)
    grid = np.zeros(dims, np.int64)
    w = np.mod(cell, dims)
    np.add.at(grid, (w[:, 0], w[:, 1], w[:, 2]), 1)
    # records in the cells [c + first, c + first + length) of each axis in turn, wrapped
    first = (-(region[0] - brick[0]) // 2, -(region[1] - brick[1]) // 2, 0)
    reg = grid
    for a in range(3):
        reg = sum(np.roll(reg, -(first[a] + k), axis=a) for k in range(region[a]))
    own = grid.reshape(dims[0] // brick[0], brick[0], dims[1] // brick[1], brick[1], dims[2] // brick[2], brick[2]).sum(axis=(1, 3, 5))
    reg = reg[::brick[0], ::brick[1], ::brick[2]]
    return own[own > 0], reg[own > 0]
