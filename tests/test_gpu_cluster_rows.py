"""GPU: the cluster solver's three row bodies (k_solve_cluster chooses one instantiation of solve_manifold_flat per kind of
sweep: regular, first of a cold solve, first of a warm one; include/spec/contact_solve.h) against the sequential CPU oracle,
bit for bit, on the smallest world that kernel accepts: the 16 x 130 x 16 tower (33 280 bodies, kClusterMinBodies is 32 768).

The top layer is spheres, so the scene has manifolds of one point (sphere on box, sphere beside sphere) next to the boxes' four,
and the bottom layer rests on the ground plane: rows without a body B, whose B side the flat driver computes from zeros and
throws away. Four worlds of six updates each, poses and velocities equal to the oracle's:

  default        warm-started: first-warm + regular bodies, diagonal tensors, one friction for all
  cold           PHYS_FLAG_NO_WARM_START: the first-cold body
  materials      the configured friction set explicitly on bodies and ground: the kernel's MAT instances (the friction rides in
                 the row); the oracle has no materials and needs none - a value combined with itself is that value, bit for bit
  full tensor    one body with a non-diagonal inverse inertia: the kernel's non-diagonal instances, two workgroups per CU"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 16_666_667
UPDATES = 6


def _scene():
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5(16, 130, 16)
    top = np.arange(sc.n) // (16 * 16) == 129
    sc.shape_type = sc.shape_type.copy()
    sc.shape_type[top] = physics_amd.SHAPE_SPHERE
    return sc


def _inertia(sc, full):
    if not full:
        return None
    inertia = np.tile(np.eye(3, dtype=np.float32).reshape(-1), (sc.n, 1))
    a = np.array([[0.3, -0.2, 0.1], [0.0, 0.25, -0.15], [0.2, 0.1, 0.3]])
    inertia[16 * 16 * 64 + 16 * 7 + 5] = (np.eye(3) * 1.2 + a @ a.T).astype(np.float32).reshape(-1)  # inside the tower
    return inertia


def _populate(x, sc, full):
    x.set_bodies(sc.pos, inertia=_inertia(sc, full), shape_type=sc.shape_type, half_extent=sc.half_extent)


@functools.lru_cache(maxsize=None)
def _oracle(cold, full):
    """(poses and velocities, stats) after UPDATES updates of the sequential oracle; computed once per kind of world"""
    import physics_amd
    from oracle import binding as ob
    sc = _scene()
    o = ob.OracleWorld(sc.config(flags=sc.flags | (physics_amd.FLAG_NO_WARM_START if cold else 0)), trig=ob.TRIG_DET)
    o.set_threads(16)
    _populate(o, sc, full)
    o.update_n(DT, UPDATES)
    state = tuple(a.copy() for a in o.get_transforms() + o.get_velocities())
    for a in state:
        a.setflags(write=False)
    s = o.get_stats()
    stats = (s.n_pairs, s.n_manifolds, s.n_contacts, s.n_colors, s.n_ground_manifolds)
    o.close()
    return state, stats


@pytest.mark.parametrize("kind", ["default", "cold", "materials", "full_tensor"])
def test_cluster_rows_bit_exact_against_the_oracle(kind):
    import physics_amd
    sc = _scene()
    cold, full = kind == "cold", kind == "full_tensor"
    flags = sc.flags | physics_amd.FLAG_SOLVER_CLUSTER | (physics_amd.FLAG_NO_WARM_START if cold else 0)
    w = physics_amd.World(sc.config(flags=flags))
    _populate(w, sc, full)
    if kind == "materials":
        f = w.cfg.friction
        w.set_body_materials(np.full(sc.n, f, np.float32), np.zeros(sc.n, np.float32))
        w.set_ground_material(f, 0.0)
    w.profile_enable(True)
    w.update_n(DT, UPDATES)
    w.sync()
    assert "solve_cluster" in w.profile_get()[0], f"the cluster solver did not run: {sorted(w.profile_get()[0])}"
    want, want_stats = _oracle(cold, full)
    for name, a, b in zip(("pos", "rot", "lin_vel", "ang_vel"), w.get_transforms() + w.get_velocities(), want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{kind}: {name} differs from the oracle"
    s = w.get_stats()
    assert (s.n_pairs, s.n_manifolds, s.n_contacts, s.n_colors, s.n_ground_manifolds) == want_stats
    # rows without a body B, and rows of fewer than four points
    assert s.n_ground_manifolds > 0 and s.n_contacts < 4 * s.n_manifolds and s.n_manifolds > 90_000
    w.close()
