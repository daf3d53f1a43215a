"""The committed inputs of the continuous-collision tests with their float64 answers (tests/ccd_ref.py), computed once per
process and shared, unchanged, by tests/test_ccd_cpu.py. numpy and the references only.

A case is the dict tests/ccd_probe.py writes as a scene, plus label, expect (per body: what the situation must come to, see
SITUATIONS) and h, the reference's answer. One case per (mover, target kind): each mover shape (sphere, capsule, box, turned
box) against each target kind (static sphere, turned capsule, box, turned box, and the ground), every situation of the list
one body; and two seeded soups of mixed bodies against mixed statics and the ground, unfiltered, with both rotation modes."""
import functools

import numpy as np

import ccd_ref as ref
from raycast_ref import GROUND, MISS

NONE, SPHERE, BOX, CAPSULE = ref.SHAPE_NONE, ref.SHAPE_SPHERE, ref.SHAPE_BOX, ref.SHAPE_CAPSULE
DT = 1.0 / 60.0
MARGIN = 0.02
IDENT = (0.0, 0.0, 0.0, 1.0)


def axis_quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return tuple(np.append(a * np.sin(angle / 2), np.cos(angle / 2)))


TURN_A, TURN_B = axis_quat((1.0, 2.0, -0.5), 0.9), axis_quat((-0.3, 0.4, 1.0), 2.1)
MOVERS = {  # shape, half extent, rotation, bounding radius
    "sphere": (SPHERE, (0.1, 0.0, 0.0), IDENT, 0.1),
    "capsule": (CAPSULE, (0.08, 0.15, 0.0), TURN_A, 0.23),
    "box": (BOX, (0.1, 0.15, 0.07), IDENT, 0.2),
    "turned box": (BOX, (0.1, 0.15, 0.07), TURN_B, 0.2),
}
TARGETS = {  # shape, half extent, rotation, bounding radius
    "sphere": (SPHERE, (0.3, 0.0, 0.0), IDENT, 0.3),
    "capsule": (CAPSULE, (0.2, 0.4, 0.0), TURN_B, 0.6),
    "box": (BOX, (0.5, 0.05, 0.4), IDENT, 0.65),
    "turned box": (BOX, (0.5, 0.05, 0.4), TURN_A, 0.65),
}
# the situations of every case, one body each, and what each must come to: "hit" the target, "miss", "tie" (two statics at equal t:
# the lower id), "solid" (a filtered-out static in front: the solid one behind it), "front" (a body that does collide with the
# front static stops there), "any" (grazing: whatever the reference says)
SITUATIONS = ("head-on", "grazing", "clear miss", "beyond L", "inside margin", "penetrating", "collides with front", "zero velocity",
              "nan velocity", "inf velocity", "shape none")
EXPECT = dict(zip(SITUATIONS, ("solid", "any", "miss", "miss", "solid", "miss", "front", "miss", "miss", "miss", "miss")))
CENTRE = np.array([0.3, 2.0, -0.2])
FRONT_FILTER = (0x00020002, 0)   # category 2, mask 2: a default body (category 1) does not collide with it
BOTH_FILTER = (0xFFFF0003, 0)    # categories 1 and 2: collides with everything


def _body(rows, shape, pos, rot, he, lin, filt=ref.FILTER_DEFAULT, ang=(0.3, -0.2, 0.5)):
    rows.append((shape, tuple(pos), tuple(rot), tuple(he), tuple(lin), tuple(ang), filt))


def _pack(rows):
    f = np.float32
    return dict(shape=np.array([r[0] for r in rows], np.uint32), pos=np.array([r[1] for r in rows], f), rot=np.array([r[2] for r in rows], f),
                half_extent=np.array([r[3] for r in rows], f), lin=np.array([r[4] for r in rows], f), ang=np.array([r[5] for r in rows], f),
                filt=np.array([r[6] for r in rows], np.uint64))


def _perp(u):
    p = np.cross(u, [0.0, 1.0, 0.0])
    return p / np.linalg.norm(p)


def _static_case(mname, tname):
    shape, he, rot, bm = MOVERS[mname]
    tshape, the, trot, bt = TARGETS[tname]
    u = np.array([0.6, -0.3, 0.74])
    u /= np.linalg.norm(u)
    p = _perp(u)
    reach = bt + bm
    D = 3.0 * reach + 1.5
    front_c = CENTRE - u * (2.0 * bt + bm + 0.3)
    f = np.float32
    # statics: the target, its twin at the same pose (equal t: the lower id wins), the filtered-out one in front
    statics = dict(shape=np.array([tshape, tshape, tshape], np.uint32), pos=np.array([CENTRE, CENTRE, front_c], f),
                   rot=np.array([trot, trot, trot], f), half_extent=np.array([the, the, the], f),
                   filt=np.array([ref.FILTER_DEFAULT, ref.FILTER_DEFAULT, FRONT_FILTER], np.uint64))
    x0 = CENTRE - u * D
    fast = u * (2.5 * D / DT)
    # where the head-on body touches, from the reference itself: the starts inside the margin and penetrating are placed by it
    probe = dict(dt=DT, margin=MARGIN, ground=None, statics=statics, bodies=_pack([(shape, tuple(x0), rot, he, tuple(fast), (0, 0, 0), ref.FILTER_DEFAULT)]))
    t_hit = float(ref.sweep(probe)["t"][0])
    assert np.isfinite(t_hit), (mname, tname)
    rows = []
    _body(rows, shape, x0, rot, he, fast)                                          # head-on
    _body(rows, shape, x0 + p * 0.45 * reach, rot, he, fast)                       # grazing
    _body(rows, shape, x0 + p * (1.5 * reach + 0.5), rot, he, fast)                # clear miss
    _body(rows, shape, x0, rot, he, u * (0.5 * (D - reach) / DT))                  # beyond L
    _body(rows, shape, x0 + u * (t_hit - 0.01), rot, he, fast)                     # inside margin
    _body(rows, shape, x0 + u * (t_hit + 0.03), rot, he, fast)                     # penetrating
    _body(rows, shape, x0, rot, he, fast, filt=BOTH_FILTER)                        # collides with front
    _body(rows, shape, x0, rot, he, (0.0, 0.0, 0.0))                               # zero velocity
    _body(rows, shape, x0, rot, he, (np.nan, 1.0, 0.0))                            # nan velocity
    _body(rows, shape, x0, rot, he, (np.inf, 1.0, 0.0))                            # inf velocity
    _body(rows, NONE, x0, rot, he, fast)                                           # shape none
    return dict(label=f"{mname} at {tname}", dt=DT, margin=MARGIN, ground=None, exact_rot=False, statics=statics, bodies=_pack(rows),
                expect=[EXPECT[s] for s in SITUATIONS], ids=dict(solid=ref.STATIC_ID_BIT | 0, front=ref.STATIC_ID_BIT | 2))


def _ground_case(mname):
    shape, he, rot, bm = MOVERS[mname]
    gy = 0.25
    hc, rho = ref.mover(shape, he)
    from raycast_ref import rotation_matrices
    R = rotation_matrices(np.asarray(rot, np.float64)[None])[0]
    low = float((hc * np.abs(R[1, :])).sum() + rho)  # the lowest point below the centre
    u = np.array([0.3, -0.8, 0.52])
    u /= np.linalg.norm(u)
    g = np.array([0.9, -0.05, 0.43])
    g /= np.linalg.norm(g)
    x0 = np.array([0.3, gy + low + 1.0, -0.2])
    fast = u * (2.5 * (1.0 / -u[1]) / DT)
    f = np.float32
    statics = dict(shape=np.zeros(0, np.uint32), pos=np.zeros((0, 3), f), rot=np.zeros((0, 4), f), half_extent=np.zeros((0, 3), f),
                   filt=np.zeros((0, 2), np.uint64))
    rows = []
    _body(rows, shape, x0, rot, he, fast)                                                       # head-on
    _body(rows, shape, x0, rot, he, g * (2.5 * (1.0 / -g[1]) / DT))                             # grazing: a shallow approach
    _body(rows, shape, x0, rot, he, np.array([0.5, 0.6, 0.2]) * 100.0)                          # clear miss: it rises
    _body(rows, shape, x0, rot, he, u * (0.5 * (1.0 / -u[1]) / DT))                             # beyond L
    _body(rows, shape, [0.3, gy + low + 0.01, -0.2], rot, he, fast)                             # inside margin
    _body(rows, shape, [0.3, gy + low - 0.03, -0.2], rot, he, fast)                             # penetrating
    _body(rows, shape, x0, rot, he, fast, filt=(0xFFFE0001, 0))                                 # its mask leaves the ground out
    _body(rows, shape, x0, rot, he, (0.0, 0.0, 0.0))                                            # zero velocity
    _body(rows, shape, x0, rot, he, (1.0, np.nan, 0.0))                                         # nan velocity
    _body(rows, shape, x0, rot, he, (1.0, -np.inf, 0.0))                                        # inf velocity
    _body(rows, NONE, x0, rot, he, fast)                                                        # shape none
    expect = ["solid", "solid", "miss", "miss", "solid", "miss", "miss", "miss", "miss", "miss", "miss"]
    return dict(label=f"{mname} at the ground", dt=DT, margin=MARGIN, ground=gy, exact_rot=False, statics=statics, bodies=_pack(rows),
                expect=expect, ids=dict(solid=GROUND, front=GROUND))


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def soup(seed, n_bodies, n_statics, ground=0.0, exact_rot=False, filtered=False, speed=(20.0, 200.0), lo_y=0.8):
    """Mixed bodies in a box of 8 x 4 x 8 m above mixed statics scattered through it, fast in every direction. Unfiltered unless
    asked; filtered: random categories and masks on bodies and statics. Also the scene of the GPU comparison (tests/test_gpu_ccd.py)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    sshape = rng.choice([SPHERE, BOX, CAPSULE], size=n_statics).astype(np.uint32)
    she = np.zeros((n_statics, 3))
    she[sshape == SPHERE, 0] = rng.uniform(0.1, 0.5, int((sshape == SPHERE).sum()))
    she[sshape == BOX] = rng.uniform(0.03, 0.7, (int((sshape == BOX).sum()), 3))
    she[sshape == CAPSULE, 0] = rng.uniform(0.05, 0.3, int((sshape == CAPSULE).sum()))
    she[sshape == CAPSULE, 1] = rng.uniform(0.1, 0.6, int((sshape == CAPSULE).sum()))
    statics = dict(shape=sshape, pos=(rng.uniform(-4, 4, (n_statics, 3)) * [1, 0.5, 1] + [0, 2.6, 0]).astype(f), rot=_quats(rng, n_statics).astype(f),
                   half_extent=she.astype(f))
    shape = rng.choice([SPHERE, BOX, CAPSULE], size=n_bodies).astype(np.uint32)
    he = np.zeros((n_bodies, 3))
    he[shape == SPHERE, 0] = rng.uniform(0.05, 0.2, int((shape == SPHERE).sum()))
    he[shape == BOX] = rng.uniform(0.03, 0.25, (int((shape == BOX).sum()), 3))
    he[shape == CAPSULE, 0] = rng.uniform(0.04, 0.12, int((shape == CAPSULE).sum()))
    he[shape == CAPSULE, 1] = rng.uniform(0.05, 0.25, int((shape == CAPSULE).sum()))
    d = rng.normal(size=(n_bodies, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bodies = dict(shape=shape, pos=(rng.uniform(-4, 4, (n_bodies, 3)) * [1, 0.5, 1] + [0, lo_y + 2.0, 0]).astype(f), rot=_quats(rng, n_bodies).astype(f),
                  half_extent=he.astype(f), lin=(d * rng.uniform(*speed, (n_bodies, 1))).astype(f), ang=rng.normal(size=(n_bodies, 3)).astype(f))
    if filtered:
        for d_, k in ((statics, n_statics), (bodies, n_bodies)):
            cat, mask = rng.integers(1, 4, k), rng.choice([0xFFFF, 0xFFFE, 0xFFFD], k)
            d_["filt"] = np.stack([cat | (mask << 16), np.zeros(k, np.int64)], 1).astype(np.uint64)
    return dict(label=f"soup seed {seed}", dt=DT, margin=MARGIN, ground=ground, exact_rot=exact_rot, statics=statics, bodies=bodies,
                expect=None, ids=None)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_static_case(m, t) for m in MOVERS for t in TARGETS] + [_ground_case(m) for m in MOVERS]
    out += [soup(11, 96, 40), soup(12, 96, 40, ground=None, exact_rot=True, filtered=True)]
    for c in out:
        c["h"] = ref.sweep(c)
    return tuple(out)
