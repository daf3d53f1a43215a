"""Float64 reference of the in-place body edits (include/physics_hip.h, phys_apply_impulses / phys_apply_forces), written for
the tests in numpy alone: one entry after another in the order given. It shares no code with the library's own statement of the
arithmetic (include/spec/body_edit.h).

An impulse entry J at world point p (None: the centre) with angular impulse A (None: zero) on a body at x with inverse mass
1/m and inverse inertia Iinv:   v += J / m,   w += Iinv (A + (p - x) x J).
A force entry f at p with torque t:   T += (p - x) x f (only with a point),   F += f,   T += t.

The bound (`bound`). Inputs are float32 values, exact in float64, so the whole difference is float32 rounding, unit roundoff
u = 2^-24. Per entry and component the float32 side performs at most: p - x (1 rounding), the cross product (2 products, 1
difference, and the rounding of p - x carried through both products: 5), A + c (1), the row sum of Iinv L (3 products, 2 sums:
5), and the final sum into w (1): 13 roundings, each relative to a magnitude that the entry's scale
    S = |Iinv|_F * (|A| + (|p| + |x|) |J|)        (forces: |t| + (|p| + |x|) |f|;  linear parts: |J| / m, |f|)
bounds (Cauchy-Schwarz for the row sums). The K running sums into the body's state each round relative to at most the
starting magnitude plus the sum of the scales. With 16 for 13 and a factor 2 for second-order terms:
    |float32 - float64| <= (16 + K) * 2^-23 * (|start| + sum of S)      per component."""
import numpy as np


def apply_impulses(x, v, w, inv_mass, inv_inertia, ids, impulse, point=None, ang_impulse=None):
    """x, v, w (n, 3), inv_mass (n,), inv_inertia (n, 3, 3); ids (m,), impulse (m, 3), point / ang_impulse (m, 3) or None.
    Returns dict(v, w float64; K entries per body; Sv, Sw the scales of `bound`, starting magnitudes included)."""
    x = np.asarray(x, np.float64)
    v = np.array(v, np.float64)
    w = np.array(w, np.float64)
    inv_mass = np.asarray(inv_mass, np.float64)
    Iinv = np.asarray(inv_inertia, np.float64)
    n = len(x)
    K = np.zeros(n, np.int64)
    Sv = np.linalg.norm(v, axis=1)
    Sw = np.linalg.norm(w, axis=1)
    for k, i in enumerate(np.asarray(ids, np.int64)):
        J = np.asarray(impulse[k], np.float64)
        p = None if point is None else np.asarray(point[k], np.float64)
        A = np.zeros(3) if ang_impulse is None else np.asarray(ang_impulse[k], np.float64)
        r = np.zeros(3) if p is None else p - x[i]
        L = A + np.cross(r, J)
        v[i] += J * inv_mass[i]
        w[i] += Iinv[i] @ L
        K[i] += 1
        Sv[i] += np.linalg.norm(J) * abs(inv_mass[i])
        reach = 0.0 if p is None else np.linalg.norm(p) + np.linalg.norm(x[i])
        Sw[i] += np.linalg.norm(Iinv[i]) * (np.linalg.norm(A) + reach * np.linalg.norm(J))
    return dict(v=v, w=w, K=K, Sv=Sv, Sw=Sw)


def apply_forces(x, F, T, ids, force, point=None, torque=None):
    """x, F, T (n, 3); ids (m,), force (m, 3), point / torque (m, 3) or None. Returns dict(F, T, K, SF, ST)."""
    x = np.asarray(x, np.float64)
    F = np.array(F, np.float64)
    T = np.array(T, np.float64)
    n = len(x)
    K = np.zeros(n, np.int64)
    SF = np.linalg.norm(F, axis=1)
    ST = np.linalg.norm(T, axis=1)
    for k, i in enumerate(np.asarray(ids, np.int64)):
        f = np.asarray(force[k], np.float64)
        if point is not None:
            p = np.asarray(point[k], np.float64)
            T[i] += np.cross(p - x[i], f)
            ST[i] += (np.linalg.norm(p) + np.linalg.norm(x[i])) * np.linalg.norm(f)
        F[i] += f
        SF[i] += np.linalg.norm(f)
        if torque is not None:
            t = np.asarray(torque[k], np.float64)
            T[i] += t
            ST[i] += np.linalg.norm(t)
        K[i] += 1
    return dict(F=F, T=T, K=K, SF=SF, ST=ST)


def bound(K, S):
    """(n, 1): what float32 may differ by, per body and component (the docstring's derivation)."""
    return ((16 + np.asarray(K)) * 2.0 ** -23 * np.asarray(S))[:, None]


def inertia_tensors(layout, n, rng):
    """(n, 3, 3) float32 inertia tensors, as phys_set_bodies takes them, that put the library into each of its three layouts:
    'shared' one diagonal tensor for every body, 'diag' a diagonal per body, 'full' a symmetric positive definite 3x3 per body.
    (The library inverts them in float32; the tests take that inverse from the probe and hand it to apply_impulses.)"""
    if layout == "shared":
        d = rng.uniform(0.5, 2.0, 3)
        return np.broadcast_to(np.diag(d), (n, 3, 3)).astype(np.float32)
    if layout == "diag":
        d = rng.uniform(0.5, 2.0, (n, 3))
        return np.stack([np.diag(r) for r in d]).astype(np.float32)
    if layout == "full":
        a = rng.normal(size=(n, 3, 3))
        return (a @ a.transpose(0, 2, 1) + 0.5 * np.eye(3)).astype(np.float32)
    raise ValueError(layout)
