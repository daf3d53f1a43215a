"""Scenes built for the branches of the colouring stage (tests/test_gpu_coloring.py; conditions checked without a device
by tests/test_color_ref_cpu.py). Pure numpy. Spheres only, no gravity, zero restitution: a sphere contact is closed-form,
so the manifold graph of every update is the designer's.

The pieces
  lattice     spheres at pitch 1 whose surfaces are a GAP apart that lies inside the contact margin (0.02): a manifold per
              lattice edge, speculative (negative depth), so nothing moves. Radii and positions are jittered from a
              committed seed; every gap stays in [0.004, 0.016]. With `ground`, the bottom layer also lies inside the
              margin of the ground plane (one-sided manifolds).
  movers      smaller spheres above the hollows of a lattice's top face, falling at 0.04 per update: at the start of update
              k each is inside the margin of the four spheres around its hollow (gap 0.004 to 0.016), one update earlier it
              is 0.03 away or more. The four new manifolds of a mover share bodies with its neighbours', so a group of
              movers is ONE connected piece of new work that takes several rounds. A `drop` is a mover straight above one
              sphere: exactly one new manifold.
  implosion   a block lattice that contracts about its centre by 2 % of its size per update: all its edges enter the margin
              in the same update.
  hub         one large sphere with k small ones around it: k manifolds at one body, k colours.
  slab / far  a static box beside a lattice's +x face (a static partner per sphere of that face) / a static sphere far away
              (changes nothing but triggers the full re-colouring that phys_set_static_bodies brings).

MARGIN_BAND: every gap the generators make is at least 0.002 away from 0 and from the margin, in float64; float32
positions (relative error 6e-8 at coordinates up to 300: 2e-5) and 70 accumulated position updates (70 x 2e-5) cannot
carry a pair across. contacts() finds the manifolds of an update in float64 and refuses a scene that breaks the band."""
import numpy as np

MARGIN = 0.02
MARGIN_BAND = 0.002
DT_NANOS = 16_666_667
DT = float(np.float32(np.float32(DT_NANOS) / np.float32(1e9)))
FALL = 0.04          # a mover's travel per update
SHRINK = 0.02        # an implosion's contraction per update
MOVER_RADIUS = 0.45
MOVER_MASS = 1.0e-4  # a mover is stopped by what it lands on and all but leaves it where it was
GROUND = 0xFFFFFFFF
STATIC_ID_BIT = 0x80000000
SEED = 20240611


class Scene:
    def __init__(self, ground=False, seed=SEED):
        self.ground = ground
        self.rng = np.random.default_rng(seed)
        self.pos, self.vel, self.radius, self.mass, self.arrive = [], [], [], [], []
        self.n = 0
        self.statics = {}  # name -> dict(pos, shape_type, half_extent)

    def _add(self, pos, radius, vel=None, mass=1.0, arrive=0):
        pos = np.asarray(pos, np.float64).reshape(-1, 3)
        first = self.n
        self.mass.append(np.full(len(pos), mass))
        self.arrive.append(np.full(len(pos), arrive, np.int64))
        self.pos.append(pos)
        self.radius.append(np.broadcast_to(np.asarray(radius, np.float64), (len(pos),)).copy())
        self.vel.append(np.zeros_like(pos) if vel is None else np.asarray(vel, np.float64).reshape(-1, 3))
        self.n += len(pos)
        return np.arange(first, self.n)

    # ---- pieces
    def lattice(self, nx, ny, nz, origin=(0.0, 0.0, 0.0)):
        """ids[nx, ny, nz]. The bottom layer's centres are 0.504 above origin.y: with origin.y = 0 and a ground plane at 0
        they lie inside its margin."""
        g = self.rng.uniform(0.006, 0.014, nx * ny * nz)
        jitter = self.rng.uniform(-0.001, 0.001, (nx * ny * nz, 3))
        ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        cells = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1).astype(np.float64)
        pos = cells + jitter + np.asarray(origin, np.float64) + np.array([0.0, 0.504, 0.0])
        return self._add(pos, (1.0 - g) / 2).reshape(nx, ny, nz)

    def _arrive(self, target, radius, k, down):
        """Bodies that reach `target` at the start of update k, moving by `down` (a vector) per update."""
        step = np.asarray(down, np.float64)
        return self._add(target - k * step, radius, np.broadcast_to(step / DT, target.shape), MOVER_MASS, k)

    def movers(self, top, hollows, k):
        """top: ids[nx, nz] of a lattice's top layer; hollows: (ix, iz) pairs, the hollow between top[ix:ix+2, iz:iz+2]."""
        pos, rad = self.positions(0), np.concatenate(self.radius)
        hollows = np.asarray(hollows).reshape(-1, 2)
        corner = np.stack([top[hollows[:, 0] + dx, hollows[:, 1] + dz] for dx in (0, 1) for dz in (0, 1)], 1)  # (m, 4)
        c, r = pos[corner], rad[corner]
        xz = c[:, :, [0, 2]].mean(1)
        lo, hi = c[:, :, 1].max(1), c[:, :, 1].max(1) + 1.0
        for _ in range(40):  # the height at which the mean gap to the four spheres is 0.010
            y = 0.5 * (lo + hi)
            p = np.stack([xz[:, 0], y, xz[:, 1]], 1)
            gap = (np.linalg.norm(c - p[:, None, :], axis=2) - r - MOVER_RADIUS).mean(1)
            lo, hi = np.where(gap < 0.010, y, lo), np.where(gap < 0.010, hi, y)
        return self._arrive(np.stack([xz[:, 0], y, xz[:, 1]], 1), MOVER_RADIUS, k, (0.0, -FALL, 0.0))

    def drop(self, body, k):
        """One mover straight above `body`, 0.010 from its surface at the start of update k."""
        pos, rad = self.positions(0), np.concatenate(self.radius)
        target = pos[body] + np.array([0.0, rad[body] + MOVER_RADIUS + 0.010, 0.0])
        return self._arrive(target[None, :], MOVER_RADIUS, k, (0.0, -FALL, 0.0))

    def implosion(self, n, k, origin):
        """An n x n x n lattice as lattice() lays it out at the start of update k, scaled about its centre before."""
        g = self.rng.uniform(0.006, 0.014, n ** 3)
        jitter = self.rng.uniform(-0.001, 0.001, (n ** 3, 3))
        ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        rel = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1).astype(np.float64) + jitter - (n - 1) / 2
        start = rel / (1.0 - k * SHRINK)
        centre = np.asarray(origin, np.float64) + (n - 1) / 2
        return self._add(centre + start, (1.0 - g) / 2, -start * SHRINK / DT, 1.0, k)

    def hub(self, partners, centre, big=3.0, small=0.5):
        i = np.arange(partners) + 0.5
        phi = np.arccos(1 - 2 * i / partners)
        theta = np.pi * (1 + 5 ** 0.5) * i
        d = np.stack([np.cos(theta) * np.sin(phi), np.cos(phi), np.sin(theta) * np.sin(phi)], 1)
        gap = self.rng.uniform(0.006, 0.014, partners)
        centre = np.asarray(centre, np.float64)
        hub = self._add(centre[None, :], big)
        return hub, self._add(centre + d * (big + small + gap)[:, None], small)

    def static_far(self, name):
        self.statics[name] = dict(pos=np.array([[0.0, 1000.0, 0.0]], np.float32), shape_type=np.array([1], np.uint32),
                                  half_extent=np.array([[0.5, 0.5, 0.5]], np.float32))

    def static_slab(self, name, face, axis=0):
        """A box beside the +axis face of a lattice (face: the ids of that layer): its near side is 0.506 beyond the mean
        centre plane of the layer, 0.008 to 0.014 from every sphere of it."""
        pos = self.positions(0)[np.asarray(face).ravel()]
        lo, hi = pos.min(0), pos.max(0)
        half = (hi - lo) / 2 + 1.0
        half[axis] = 0.5
        centre = (hi + lo) / 2
        centre[axis] = pos[:, axis].mean() + 0.506 + half[axis]
        self.statics[name] = dict(pos=centre[None, :].astype(np.float32), shape_type=np.array([2], np.uint32),
                                  half_extent=half[None, :].astype(np.float32))

    # ---- what the world gets
    def bodies(self):
        r = np.concatenate(self.radius).astype(np.float32)
        return dict(pos=np.concatenate(self.pos).astype(np.float32), lin_vel=np.concatenate(self.vel).astype(np.float32),
                    mass=np.concatenate(self.mass).astype(np.float32), shape_type=np.full(self.n, 1, np.uint32),
                    half_extent=np.stack([r, r, r], 1))

    def positions(self, k):
        """float64 positions at the start of update k. A moving body is taken to stay where it arrived (the solver stops it
        inside the margin of what it met; a mover is too light to push that away)."""
        travel = np.minimum(k, np.concatenate(self.arrive))[:, None] if self.n else 0
        return np.concatenate(self.pos) + travel * DT * np.concatenate(self.vel).astype(np.float32).astype(np.float64)


# ---- the manifolds of an update, in float64 ----------------------------------------------------------------------------
def _sphere_pairs(pos, rad, reach_extra):
    """(i, j, gap) with i < j for every pair of spheres whose gap is at most reach_extra. Cell list; the few spheres larger
    than 0.51 are tested against everyone."""
    large = np.flatnonzero(rad > 0.51)
    small = np.flatnonzero(rad <= 0.51)
    out_i, out_j = [], []
    for b in large:
        d = np.linalg.norm(pos - pos[b], axis=1) - rad - rad[b]
        hit = np.flatnonzero((d <= reach_extra) & (np.arange(len(pos)) != b) & ~((rad > 0.51) & (np.arange(len(pos)) < b)))
        out_i.append(np.full(len(hit), b)); out_j.append(hit)
    if len(small):
        cell = 1.25
        c = np.floor(pos[small] / cell).astype(np.int64)
        c -= c.min(0)
        dims = c.max(0) + 3
        key = ((c[:, 0] + 1) * dims[1] + (c[:, 1] + 1)) * dims[2] + (c[:, 2] + 1)
        order = np.argsort(key, kind="stable")
        skey, sid = key[order], small[order]
        offsets = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) >= (0, 0, 0)]
        for dx, dy, dz in offsets:
            other = skey + (dx * dims[1] + dy) * dims[2] + dz
            lo, hi = np.searchsorted(skey, other, "left"), np.searchsorted(skey, other, "right")
            for s in range(int((hi - lo).max()) if len(lo) else 0):
                ok = lo + s < hi
                i, j = sid[ok], sid[(lo + s)[ok]]
                if (dx, dy, dz) == (0, 0, 0):
                    keep = i < j
                    i, j = i[keep], j[keep]
                d = np.linalg.norm(pos[i] - pos[j], axis=1) - rad[i] - rad[j]
                hit = d <= reach_extra
                out_i.append(i[hit]); out_j.append(j[hit])
    i, j = np.concatenate(out_i or [np.zeros(0, np.int64)]), np.concatenate(out_j or [np.zeros(0, np.int64)])
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return lo, hi, np.linalg.norm(pos[lo] - pos[hi], axis=1) - rad[lo] - rad[hi]


def contacts(scene, k, statics=None):
    """Unordered keys (min << 32 | max; the ground and statics as the device names them) of the manifolds of update k, from
    float64 positions; valid while no moving body has touched anything before update k. Refuses a scene in which a gap lies
    inside MARGIN_BAND of the margin or of zero."""
    pos, rad = scene.positions(k), np.concatenate(scene.radius)
    i, j, gap = _sphere_pairs(pos, rad, MARGIN + MARGIN_BAND)
    gaps = [gap]
    keys = [(i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)]
    if scene.ground:
        g = pos[:, 1] - rad
        near = np.flatnonzero(g <= MARGIN + MARGIN_BAND)
        gaps.append(g[near])
        keys.append((near.astype(np.uint64) << np.uint64(32)) | np.uint64(GROUND))
    if statics is not None:
        st = scene.statics[statics]
        for s in range(len(st["pos"])):
            c, h = st["pos"][s].astype(np.float64), st["half_extent"][s].astype(np.float64)
            if st["shape_type"][s] == 1:
                g = np.linalg.norm(pos - c, axis=1) - rad - h[0]
            else:  # an axis-aligned box: distance of the centre to the box, less the radius
                g = np.linalg.norm(np.maximum(np.abs(pos - c) - h, 0.0), axis=1) - rad
            near = np.flatnonzero(g <= MARGIN + MARGIN_BAND)
            gaps.append(g[near])
            keys.append((near.astype(np.uint64) << np.uint64(32)) | np.uint64(STATIC_ID_BIT | s))
    gap, keys = np.concatenate(gaps), np.concatenate(keys)
    assert np.all(gap >= MARGIN_BAND) and np.all(np.abs(gap - MARGIN) >= MARGIN_BAND), "a gap inside the band: float32 may decide otherwise"
    return np.sort(keys[gap < MARGIN])


def unordered_keys(a, b):
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    body = (b & np.uint64(STATIC_ID_BIT)) == 0
    lo, hi = np.where(body, np.minimum(a, b), a), np.where(body, np.maximum(a, b), b)
    return np.sort((lo << np.uint64(32)) | hi)


def split_keys(keys):
    """(a, b) of unordered keys, for contact_ref.color_manifolds (whose priority hashes the pair as the device orders it:
    use it for counts and sizes only, not for colours)."""
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def lattice_edges(nx, ny, nz, ground=False):
    return 3 * nx * ny * nz - nx * ny - ny * nz - nx * nz + (nx * nz if ground else 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def exact(M, ground=False):
    """A scene with exactly M manifolds on every update: the largest cube lattice below M and a chain for the rest."""
    sc = Scene(ground=False)
    n = 1
    while lattice_edges(n + 1, n + 1, n + 1) <= M and n < 40:
        n += 1
    rest = M - (lattice_edges(n, n, n) if n > 1 else 0)
    if n > 1:
        sc.lattice(n, n, n)
    if rest:
        sc.lattice(rest + 1, 1, 1, origin=(0.0, 0.0, -10.0))
    sc.expect = {k: M for k in range(8)}
    return sc


def hollow_block(x0, z0, nx, nz):
    return [(x0 + i, z0 + j) for i in range(nx) for j in range(nz)]


# (each returns a Scene with the handles its test needs as attributes; `arrivals`: {update: new manifolds expected then})
def probe_20k():
    sc = Scene(ground=True)
    sc.lattice(19, 19, 19)
    sc.expect_M = lattice_edges(19, 19, 19, ground=True)
    return sc


def small_incremental():
    """Nothing new (updates 1, 4, 6), one new manifold (2), 400 (3), 6400 (5) on a base of 20 450."""
    sc = Scene(ground=True)
    top = sc.lattice(48, 3, 48)[:, 2, :]
    chain = sc.lattice(3, 1, 1, origin=(0.0, 0.0, -10.0)).ravel()
    sc.drop(chain[1], 2)
    sc.movers(top, hollow_block(42, 0, 5, 20), 3)
    sc.movers(top, hollow_block(0, 0, 40, 40), 5)
    sc.expect_M = lattice_edges(48, 3, 48, ground=True) + 2 + 3  # (the chain also lies on the ground)
    sc.arrivals = {2: 1, 3: 400, 5: 6400}
    return sc


SMALL_FULL_SIZES = (1000, 2047, 2048, 2049, 6150, 39744)


def small_full(M):
    if M == 39744:
        sc = Scene()
        sc.lattice(24, 24, 24)
        assert lattice_edges(24, 24, 24) == M
    else:
        sc = exact(M)
    sc.static_far("far")
    sc.expect_M = M
    return sc


def beyond_registers():
    """36 480 manifolds, then 15 876 more in update 2."""
    sc = Scene(ground=True)
    top = sc.lattice(64, 3, 64)[:, 2, :]
    sc.movers(top, hollow_block(0, 0, 63, 63), 2)
    sc.expect_M = lattice_edges(64, 3, 64, ground=True)
    sc.arrivals = {2: 4 * 63 * 63}
    return sc


KNOWN_BASE = lattice_edges(70, 3, 70, ground=True)  # 43 680


def known_incremental():
    sc = Scene(ground=True)
    top = sc.lattice(70, 3, 70)[:, 2, :]
    chain = sc.lattice(5, 1, 1, origin=(0.0, 0.0, -10.0)).ravel()
    sc.hub_id, _ = sc.hub(64, (-20.0, 10.0, 0.0))
    sc.drop(chain[0], 2)
    sc.drop(chain[4], 4)
    sc.movers(top, hollow_block(0, 0, 20, 20), 14)
    sc.movers(top, hollow_block(25, 0, 10, 10), 64)
    sc.movers(top, hollow_block(25, 15, 10, 10), 65)
    sc.expect_M = KNOWN_BASE + 4 + 5 + 64
    sc.arrivals = {2: 1, 4: 1, 14: 1600, 64: 400, 65: 400}
    return sc


def known_full():
    sc = Scene(ground=True)
    ids = sc.lattice(70, 3, 70)
    sc.movers(ids[:, 2, :], hollow_block(0, 0, 40, 40), 3)
    sc.static_far("far")
    sc.static_slab("slab", ids[-1], 0)
    sc.expect_M = KNOWN_BASE
    sc.arrivals = {3: 6400}
    sc.slab_manifolds = 3 * 70
    return sc


IMPLOSION = 57


def stage_overflow():
    sc = Scene(ground=True)
    ids = sc.lattice(70, 3, 70)
    sc.movers(ids[:, 2, :], hollow_block(0, 0, 10, 10), 2)
    sc.implosion(IMPLOSION, 4, (300.0, 50.0, 0.0))
    sc.expect_M = KNOWN_BASE
    sc.arrivals = {2: 400, 4: lattice_edges(IMPLOSION, IMPLOSION, IMPLOSION)}
    return sc


def hub_scene(partners):
    sc = Scene()
    sc.lattice(8, 8, 8)
    sc.hub_id, _ = sc.hub(partners, (-20.0, 10.0, 0.0))
    sc.expect_M = lattice_edges(8, 8, 8) + partners
    return sc


def cluster_scene():
    sc = Scene()
    ids = sc.lattice(32, 32, 32)
    sc.movers(ids[:, 31, :], hollow_block(0, 0, 10, 10), 2)
    sc.expect_M = lattice_edges(32, 32, 32)
    sc.arrivals = {2: 400}
    return sc
