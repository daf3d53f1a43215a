"""Float64 statement of the material rules (friction and restitution per body, static collider and ground plane),
written for the tests from the documented definitions (include/physics_hip.h). numpy only: it shares
no code with the spec header, the oracle or the kernels.

  * a manifold's friction is the geometric mean of its two sides': mu = sqrt(fa fb); its restitution the larger: max(ea, eb);
  * per contact point, from the velocities the solve starts from: vn = n . ((vB + wB x rB) - (vA + wA x rA)), body B at
    rest for statics and the ground. The point bounces iff e > 0, vn < -threshold and depth - vn dt >= 0; a bouncing
    point asks for bias = max(contact_bias(depth), -e vn), every other point for contact_bias(depth).

MaterialSolverRef feeds the per-manifold mu and the per-point bias into the float64 sequential-impulse reference of
tests/contact_ref.py: its colouring, warm starting and rows are used as they are; `solve` below is contact_ref.solve with
the one scalar `friction` replaced by a value per manifold (tests/test_material_cpu.py holds the two against each other).
Manifolds against static colliders are solved like ground manifolds (body B does not move), so a body may have at most one
manifold against a static or the ground in an update given to this reference."""
import numpy as np

import contact_ref as cr

STATIC_ID_BIT = 0x80000000


def combine_friction(fa, fb):
    return np.sqrt(np.asarray(fa, np.float64) * np.asarray(fb, np.float64))


def combine_restitution(ea, eb):
    return np.maximum(np.asarray(ea, np.float64), np.asarray(eb, np.float64))


class Materials:
    """friction / restitution of the bodies (n,), the statics (n_static,) and the ground (two numbers), and the threshold."""

    def __init__(self, body_friction, body_restitution, static_friction=(), static_restitution=(), ground=(0.5, 0.0), threshold=1.0):
        self.bf = np.asarray(body_friction, np.float64)
        self.be = np.asarray(body_restitution, np.float64)
        self.sf = np.asarray(static_friction, np.float64)
        self.se = np.asarray(static_restitution, np.float64)
        self.ground = (float(ground[0]), float(ground[1]))
        self.threshold = float(threshold)

    def of_manifolds(self, a, b):
        """(mu, e) per manifold (a[m], b[m]): b a body index, STATIC_ID_BIT | k, or contact_ref.GROUND."""
        a = np.asarray(a, np.int64)
        b = np.asarray(b, np.int64)
        gnd = b == cr.GROUND
        st = ~gnd & (b >= STATIC_ID_BIT)
        bb = ~gnd & ~st
        fb = np.full(len(a), self.ground[0])
        eb = np.full(len(a), self.ground[1])
        fb[bb], eb[bb] = self.bf[b[bb]], self.be[b[bb]]
        if st.any():
            k = b[st] - STATIC_ID_BIT
            fb[st], eb[st] = self.sf[k], self.se[k]
        return combine_friction(self.bf[a], fb), combine_restitution(self.be[a], eb)


def normal_velocity(n, vA, wA, rA, vB, wB, rB):
    """n . ((vB + wB x rB) - (vA + wA x rA)); arrays (..., 3)."""
    return ((vB + np.cross(wB, rB) - vA - np.cross(wA, rA)) * n).sum(-1)


def pushout_and_rebound(depth, vn, e, threshold, p):
    """The two terms of a point's bias: contact_bias(depth), and the rebound -e vn where the point bounces (else -inf)."""
    depth, vn, e = (np.asarray(x, np.float64) for x in (depth, vn, e))
    push = cr.contact_bias(depth, p)
    bounces = (e > 0.0) & (vn < -threshold) & (depth - vn * p.dt >= 0.0)
    return push, np.where(bounces, -e * vn, -np.inf)


def restitution_bias(depth, vn, e, threshold, p):
    push, rebound = pushout_and_rebound(depth, vn, e, threshold, p)
    return np.maximum(push, rebound)


def solve(a, b, count, colors, n_colors, rows, lin, ang, mu, iterations, P0=None):
    """contact_ref.solve with a friction coefficient per manifold (mu, shape (m,))."""
    v = np.array(lin, np.float64)
    w = np.array(ang, np.float64)
    M = len(a)
    mu = np.broadcast_to(np.asarray(mu, np.float64), (M,))
    P = np.zeros((M, 4, 3)) if P0 is None else np.array(P0, np.float64)
    dyn = b != cr.GROUND
    bb = np.where(dyn, b, 0)
    for sweep in range(0 if P0 is not None else 1, iterations + 1):
        for c in range(n_colors):
            idx = np.flatnonzero(colors == c)
            if not len(idx):
                continue
            A, B, hb = a[idx], bb[idx], dyn[idx][:, None]
            vA, wA = v[A], w[A]
            vB, wB = v[B] * hb, w[B] * hb
            Pc = P[idx]
            for k in range(4):
                act = rows["active"][idx, k]
                for d in range(3):
                    dirv = rows["D"][idx, d]
                    aA, aB, mA, mB = rows["aA"][idx, k, d], rows["aB"][idx, k, d], rows["mA"][idx, k, d], rows["mB"][idx, k, d]
                    if sweep == 0:
                        lam = np.where(act, Pc[:, k, d], 0.0)
                    else:
                        vrel = ((dirv * vB).sum(1) + (aB * wB).sum(1)) - ((dirv * vA).sum(1) + (aA * wA).sum(1))
                        old = Pc[:, k, d]
                        if d < 2:
                            lim = mu[idx] * Pc[:, k, 2]
                            new = np.maximum(-lim, np.minimum(old - rows["mass"][idx, k, d] * vrel, lim))
                        else:
                            new = np.maximum(old + rows["mass"][idx, k, d] * (rows["bias"][idx, k] - vrel), 0.0)
                        new = np.where(act, new, 0.0)
                        lam = new - old
                        Pc[:, k, d] = new
                    vA = vA - dirv * (rows["imA"][idx] * lam)[:, None]
                    wA = wA - mA * lam[:, None]
                    vB = vB + dirv * (rows["imB"][idx] * lam)[:, None]
                    wB = wB + mB * lam[:, None]
            P[idx] = Pc
            v[A], w[A] = vA, wA
            h = dyn[idx]
            v[B[h]], w[B[h]] = vB[h], wB[h]
    return v, w, P


class MaterialSolverRef(cr.SolverRef):
    """contact_ref.SolverRef with materials: one call is one update (see contact_ref); `materials` may change between calls."""

    def update(self, manifolds, pos, lin, ang, inv_mass, inv_inertia, force=None, materials=None):
        m = cr.unpack_manifolds(manifolds)
        mu, e = materials.of_manifolds(m["a"], m["b"])
        static = (m["b"] != cr.GROUND) & (m["b"] >= STATIC_ID_BIT)
        m["b"] = np.where(static, cr.GROUND, m["b"])  # a static does not move: solved like the ground
        m["keys"] = cr.pair_keys(m["a"], m["b"])
        assert (m["keys"][1:] > m["keys"][:-1]).all(), "manifolds must be sorted by pair, one static-or-ground manifold per body"
        prev = self.prev
        colors, n_colors, rounds, n_new = cr.color_manifolds(m["a"], m["b"], self.n, None if prev is None else prev["keys"],
                                                             None if prev is None else prev["colors"])
        inv_mass = np.broadcast_to(np.asarray(inv_mass, np.float64), (self.n,))
        inv_inertia = np.broadcast_to(np.asarray(inv_inertia, np.float64), (self.n, 3, 3))
        x = np.asarray(pos, np.float64).reshape(-1, 3)
        rows = cr.build_rows(m["a"], m["b"], m["count"], m["normal32"], m["pts"], m["depth"], x, inv_mass, inv_inertia, self.p)
        v = np.asarray(lin, np.float64).reshape(-1, 3)
        if force is not None:
            v = v + self.p.dt * np.asarray(force, np.float64) * inv_mass[:, None]
        w = np.asarray(ang, np.float64).reshape(-1, 3)
        # the restitution bias, from the velocities the solve starts from
        dyn = m["b"] != cr.GROUND
        bb = np.where(dyn, m["b"], 0)
        n = m["normal32"].astype(np.float64)[:, None, :]
        rA = m["pts"] - x[m["a"]][:, None, :]
        rB = np.where(dyn[:, None, None], m["pts"] - x[bb][:, None, :], 0.0)
        vB = np.where(dyn[:, None], v[bb], 0.0)[:, None, :]
        wB = np.where(dyn[:, None], w[bb], 0.0)[:, None, :]
        vn = normal_velocity(n, v[m["a"]][:, None, :], w[m["a"]][:, None, :], rA, vB, wB, rB)
        bias = restitution_bias(m["depth"], vn, e[:, None], materials.threshold, self.p)
        rows["bias"] = np.where(rows["active"], bias, 0.0)
        P0, amb = cr.warm_match(m, prev) if self.warm else (None, np.zeros(len(m["a"]), bool))
        v, w, P = solve(m["a"], m["b"], m["count"], colors, n_colors, rows, v, w, mu, self.iterations, P0)
        self.prev = dict(keys=m["keys"], colors=colors, normal32=m["normal32"], count=m["count"], pts=m["pts"], imp=P)
        return dict(lin=v, ang=w, colors=colors, n_colors=n_colors, color_rounds=rounds, n_new_manifolds=n_new, impulses=P,
                    ambiguous=amb | rows["basis_amb"], a=m["a"], b=m["b"], count=m["count"], P0=P0, mu=mu, e=e, vn=vn,
                    bias=rows["bias"], bounces=rows["active"] & (bias > cr.contact_bias(m["depth"], self.p)))
