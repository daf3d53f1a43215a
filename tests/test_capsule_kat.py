"""CPU: known answers for capsules (include/spec/collide.h, PHYS_SPEC_SHAPE_CAPSULE) through the oracle, which compiles
the same header the narrow phase does. Margin 0.02; capsule radius 0.5 and core half-length 1 unless stated."""
import numpy as np
import pytest

from oracle import binding as ob
from physics_amd import (FLAG_COLLISIONS, FLAG_GROUND_PLANE, GROUND_ID, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_SPHERE,
                         default_config)

MARGIN = 0.02
S = np.float32(np.sqrt(0.5))
Q_ID = [0, 0, 0, 1]
Q_X = [0, 0, S, S]   # 90 deg about z: the capsule's axis along x
Q_Z = [S, 0, 0, S]   # 90 deg about x: the capsule's axis along z


def manifolds(pos, rot, shape, he, ground=False):
    flags = FLAG_COLLISIONS | (FLAG_GROUND_PLANE if ground else 0)
    w = ob.OracleWorld(default_config(flags=flags, gravity_offset=(0, 0, 0), contact_margin=MARGIN), trig=ob.TRIG_DET)
    w.set_bodies(np.array(pos, np.float32), rot=np.array(rot, np.float32), shape_type=np.array(shape, np.uint32),
                 half_extent=np.array(he, np.float32))
    w.collide_now()
    ids, counts, normals, points = w.get_manifolds()
    aabbs = w.get_aabbs()
    w.close()
    return ids, counts, normals, points, aabbs


def one(pos, rot, shape, he, ground=False):
    ids, counts, normals, points, _ = manifolds(pos, rot, shape, he, ground)
    assert len(ids) == 1, ids
    return ids[0], int(counts[0]), normals[0], points[0, :counts[0]]


CAP = [0.5, 1.0, 0.0]


def test_lying_capsule_on_the_ground_has_two_points():
    ids, n, normal, pts = one([[0, 0.45, 0]], [Q_X], [SHAPE_CAPSULE], [CAP], ground=True)
    assert ids[1] == GROUND_ID and n == 2
    assert np.allclose(normal, [0, -1, 0])
    assert np.allclose(sorted(pts[:, 0]), [-1, 1], atol=1e-6)
    assert np.allclose(pts[:, 1], -0.025, atol=1e-6) and np.allclose(pts[:, 2], 0, atol=1e-6)
    assert np.allclose(pts[:, 3], 0.05, atol=1e-6)


def test_standing_capsule_on_the_ground_has_one_point():
    ids, n, normal, pts = one([[0, 1.48, 0]], [Q_ID], [SHAPE_CAPSULE], [CAP], ground=True)
    assert n == 1
    assert np.allclose(pts[0, :3], [0, -0.01, 0], atol=1e-6) and abs(pts[0, 3] - 0.02) < 1e-6


def test_zero_length_capsule_is_a_sphere_on_the_ground():
    _, n, _, pts = one([[0, 0.45, 0]], [Q_X], [SHAPE_CAPSULE], [[0.5, 0.0, 0.0]], ground=True)
    _, ns, _, ptss = one([[0, 0.45, 0]], [Q_X], [SHAPE_SPHERE], [[0.5, 0.5, 0.5]], ground=True)
    assert n == 1 and ns == 1
    assert pts[0, 3] == ptss[0, 3]
    assert np.array_equal(pts, ptss)


def test_capsule_against_sphere():
    ids, n, normal, pts = one([[0, 0, 0], [0.9, 0.5, 0]], [Q_ID, Q_ID], [SHAPE_CAPSULE, SHAPE_SPHERE], [CAP, [0.5, 0.5, 0.5]])
    assert tuple(ids) == (0, 1) and n == 1
    assert np.allclose(normal, [1, 0, 0], atol=1e-6)
    assert np.allclose(pts[0], [0.45, 0.5, 0, 0.1], atol=1e-6)


def test_parallel_capsules_give_the_ends_of_the_overlap():
    _, n, normal, pts = one([[0, 0, 0], [0.9, 0.5, 0]], [Q_ID, Q_ID], [SHAPE_CAPSULE] * 2, [CAP, CAP])
    assert n == 2
    assert np.allclose(normal, [1, 0, 0], atol=1e-6)
    assert np.allclose(sorted(pts[:, 1]), [-0.5, 1.0], atol=1e-6)
    assert np.allclose(pts[:, 3], 0.1, atol=1e-6)
    assert np.allclose(pts[:, 0], 0.45, atol=1e-6)


def test_crossed_capsules_give_one_point():
    _, n, normal, pts = one([[0, 0, 0], [0, 0.9, 0]], [Q_X, Q_Z], [SHAPE_CAPSULE] * 2, [CAP, CAP])
    assert n == 1
    assert np.allclose(normal, [0, 1, 0], atol=1e-6)
    assert np.allclose(pts[0], [0, 0.45, 0, 0.1], atol=1e-6)


def test_coincident_capsules_take_the_fallback_normal():
    _, n, normal, pts = one([[0, 0, 0], [0, 0, 0]], [Q_X, Q_X], [SHAPE_CAPSULE] * 2, [CAP, CAP])
    assert n == 2 and np.array_equal(normal, np.float32([0, 1, 0]))
    assert np.isfinite(pts).all()


def test_capsule_lying_on_a_box_face():
    _, n, normal, pts = one([[0, 0.7, 0], [0, 0, 0]], [Q_X, Q_ID], [SHAPE_CAPSULE, SHAPE_BOX], [[0.25, 1, 0], [2, 0.5, 2]])
    assert n == 2
    assert np.allclose(normal, [0, -1, 0], atol=1e-6)
    assert np.allclose(sorted(pts[:, 0]), [-1, 1], atol=1e-6)
    assert np.allclose(pts[:, 1], 0.475, atol=1e-6) and np.allclose(pts[:, 3], 0.05, atol=1e-6)


def test_capsule_hanging_over_a_box_edge_is_clipped_to_the_face():
    _, n, normal, pts = one([[2, 0.7, 0], [0, 0, 0]], [Q_X, Q_ID], [SHAPE_CAPSULE, SHAPE_BOX], [[0.25, 1, 0], [2, 0.5, 2]])
    assert n == 2
    assert np.allclose(sorted(pts[:, 0]), [1, 2], atol=1e-6)
    assert np.allclose(pts[:, 3], 0.05, atol=1e-6)


def test_capsule_beside_a_box_edge_falls_back_to_one_point():
    # axis along z through (2.3, 0.8): parallel to the box's edge (x = 2, y = 0.5), at distance sqrt(0.3^2 + 0.3^2)
    _, n, normal, pts = one([[2.3, 0.8, 0], [0, 0, 0]], [Q_Z, Q_ID], [SHAPE_CAPSULE, SHAPE_BOX], [[0.5, 1, 0], [2, 0.5, 2]])
    assert n == 1
    d = np.hypot(0.3, 0.3)
    assert np.allclose(pts[:, 3], 0.5 - d, atol=1e-5)
    assert np.allclose(normal, [-np.sqrt(0.5), -np.sqrt(0.5), 0], atol=1e-5)


def test_capsule_across_a_box_edge_gives_one_edge_point():
    # axis along (-1, 1, 0) / sqrt 2 (45 deg about z), crossing the box's edge (x = 2, y = 0.5) at distance 0.4
    c, s = np.cos(np.pi / 8), np.sin(np.pi / 8)
    q = [0, 0, s, c]
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    centre = np.array([2.0, 0.5, 0.0]) + 0.4 * u
    _, n, normal, pts = one([centre, [0, 0, 0]], [q, Q_ID], [SHAPE_CAPSULE, SHAPE_BOX], [[0.45, 1, 0], [2, 0.5, 2]])
    assert n == 1
    assert np.allclose(normal, -u, atol=1e-5)
    assert abs(pts[0, 3] - 0.05) < 1e-5
    assert np.allclose(pts[0, :3], np.array([2.0, 0.5, 0.0]) - 0.025 * u, atol=1e-5)


@pytest.mark.parametrize("other,he", [(SHAPE_CAPSULE, CAP), (SHAPE_SPHERE, [0.7, 0.7, 0.7]), (SHAPE_BOX, [0.6, 0.8, 0.5])])
def test_deep_overlap_is_finite(other, he):
    ids, counts, normals, points, _ = manifolds([[0, 0, 0], [0.01, 0.02, 0.0]], [Q_ID, Q_X], [SHAPE_CAPSULE, other], [CAP, he])
    assert len(ids) == 1 and counts[0] >= 1
    assert np.isfinite(normals).all() and np.isfinite(points).all()
    assert abs(np.linalg.norm(normals[0]) - 1) < 1e-5
    assert (points[0, :counts[0], 3] > 0.5).all()


def test_aabb_of_rotated_capsules():
    q = np.array([0, 0, np.sin(np.pi / 12), np.cos(np.pi / 12)], np.float32)  # 30 deg about z
    _, _, _, _, a = manifolds([[0, 0, 0], [10, 0, 0], [20, 0, 0]], [Q_ID, Q_X, q], [SHAPE_CAPSULE] * 3, [CAP, CAP, [0.5, 2, 9]])
    m = MARGIN
    assert np.allclose(a[0], [-0.5 - m, -1.5 - m, -0.5 - m, 0.5 + m, 1.5 + m, 0.5 + m], atol=1e-6)
    assert np.allclose(a[1], [8.5 - m, -0.5 - m, -0.5 - m, 11.5 + m, 0.5 + m, 0.5 + m], atol=1e-6)
    ex, ey = 2 * np.sin(np.pi / 6) + 0.5, 2 * np.cos(np.pi / 6) + 0.5
    assert np.allclose(a[2], [20 - ex - m, -ey - m, -0.5 - m, 20 + ex + m, ey + m, 0.5 + m], atol=1e-5)


@pytest.mark.parametrize("other,he,rot", [(SHAPE_SPHERE, [0.5, 0.5, 0.5], Q_ID), (SHAPE_BOX, [0.6, 0.5, 0.7], [0.1, 0.2, 0.3, 0.927]),
                                          (SHAPE_CAPSULE, [0.4, 0.7, 0], Q_Z)])
def test_swapped_order_negates_the_normal(other, he, rot):
    rot = np.array(rot, np.float32) / np.linalg.norm(rot)
    cap = ([0, 0, 0], Q_X, SHAPE_CAPSULE, [0.5, 0.8, 0])
    oth = ([0.3, 0.9, 0.2], rot, other, he)
    a = one(*[list(x) for x in zip(cap, oth)])
    b = one(*[list(x) for x in zip(oth, cap)])
    assert a[1] == b[1]
    if other == SHAPE_CAPSULE:  # the capsule pair measures along A's axis: the same normal up to rounding
        assert np.allclose(a[2], -b[2], atol=1e-6)
    else:  # the pair is tested with the capsule as A either way
        assert np.array_equal(a[2], -b[2])
