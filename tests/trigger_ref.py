"""Float64 reference of the trigger volumes (include/physics_hip.h, phys_set_triggers ...), written for the tests.

Occupancy is tests/query_ref.py's brute-force `overlap` with the triggers as the query shapes and the bodies as the
targets, applied to poses (the ones read back from a world after an update, or the ballistic scene's own), body ids
only, masks applied. Events are the set difference of two consecutive occupancies.

Tolerance: the project's existing one (tests/test_gpu_query.py compare_overlaps). A GPU / reference disagreement on a
(trigger, body) pair is allowed only where the reference's separation is within NEAR = 1e-4 of touching, and over a test
there may be at most near_cap(reference_events) = max(2, reference_events // 100) such pairs."""
import numpy as np

import query_ref as ref

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 0, 1, 2, 3
ENTER, EXIT = 1, 2
NEAR = 1e-4
DT = 1.0 / 60.0
DT_NANOS = 16_666_667


def near_cap(reference_events):
    return max(2, reference_events // 100)


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def soup_triggers(rng):
    """Six volumes - 2 boxes, 2 spheres, 2 capsules - rotated, at non-lattice coordinates inside the cage."""
    return dict(shape=np.array([2, 2, 1, 1, 3, 3], np.uint32),
                pos=np.array([[-3.37, -2.11, 1.93], [4.21, 2.87, -3.59], [0.43, -5.17, -4.31], [-4.69, 3.23, 4.07],
                              [2.71, -3.83, 3.41], [-1.13, 4.61, -1.77]], np.float32),
                rot=_quats(rng, 6),
                half_extent=np.array([[2.3, 1.7, 2.9], [1.9, 3.1, 1.3], [2.7, 0, 0], [3.3, 0, 0], [1.3, 2.9, 0], [1.7, 2.1, 0]],
                                     np.float32))


def soup(seed=7, n=192, cage=8.0):
    """The ballistic scene: n bodies of mixed shapes (5 % NONE) with speeds 5 to 15 inside a cage of +-cage, six triggers."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-cage + 1.0, cage - 1.0, (n, 3)).astype(np.float32)
    shape = rng.choice([1, 2, 3, 0], n, p=[0.3, 0.35, 0.3, 0.05]).astype(np.uint32)
    he = rng.uniform(0.15, 0.45, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    vel = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5.0, 15.0, (n, 1))).astype(np.float32)
    return dict(pos=pos, rot=_quats(rng, n), vel=vel, shape=shape, half_extent=he, cage=cage, triggers=soup_triggers(rng))


def ballistic(sc, steps, dt=DT):
    """Positions after each of `steps` steps of straight flight, reflected at the cage walls (float64; rotations stay)."""
    p = sc["pos"].astype(np.float64)
    v = sc["vel"].astype(np.float64)
    c = sc["cage"]
    for _ in range(steps):
        p = p + v * dt
        out = np.abs(p) > c
        p = np.where(out, np.sign(p) * (2 * c) - p, p)
        v = np.where(out, -v, v)
        yield p.copy()


def occupancy(trig, pos, rot, shape, half_extent, category=None, mask=None):
    """(pairs, near): the set of (trigger, body) occupant pairs at these poses, and {(trigger, body): separation} of the
    pairs within 1e-3 of touching. mask (per trigger) / category (per body): body i is seen iff category[i] & mask[k]."""
    tg = ref.targets(dict(pos=pos, rot=rot, half_extent=half_extent, shape=shape))
    finite = np.isfinite(np.asarray(pos, np.float64)).all(1) & np.isfinite(np.asarray(rot, np.float64)).all(1)
    tg["shape"] = np.where(finite, tg["shape"], SHAPE_NONE)  # a non-finite pose is never an occupant
    res = ref.overlap(trig["shape"], trig["pos"], trig.get("rot"), trig["half_extent"], tg)
    n = len(np.asarray(pos).reshape(-1, 3))
    cat = np.full(n, 1, np.int64) if category is None else np.broadcast_to(np.asarray(category, np.int64), (n,))
    pairs, near = set(), {}
    for k, (ids, close) in enumerate(res):
        m = 0xFFFF if mask is None else int(np.broadcast_to(np.asarray(mask), (len(res),))[k])
        pairs |= {(k, i) for i in ids if cat[i] & m}
        near.update({(k, i): s for i, s in close.items() if cat[i] & m})
    return pairs, near


def events(before, after):
    """[(kind, trigger, body)] of the transition between two occupancies, in the drain's order."""
    return sorted([(ENTER, k, i) for k, i in after - before] + [(EXIT, k, i) for k, i in before - after])


def csr_pairs(offsets, ids):
    """The (trigger, body) set of a get_trigger_overlaps result; asserts the CSR convention (ascending unique ids)."""
    assert offsets[0] == 0 and offsets[-1] == len(ids)
    out = set()
    for k in range(len(offsets) - 1):
        seg = [int(x) for x in ids[int(offsets[k]):int(offsets[k + 1])]]
        assert seg == sorted(set(seg)), (k, seg)
        out |= {(k, i) for i in seg}
    return out


def disagreements(got, want, near, label=""):
    """Pairs on which `got` and the reference's `want` differ; each must be within NEAR of touching. Returns their count."""
    diff = got ^ want
    for pair in diff:
        assert pair in near and abs(near[pair]) <= NEAR, (label, pair, pair in got, near.get(pair))
    return len(diff)
