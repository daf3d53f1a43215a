#!/usr/bin/env python3
"""Run by the GPU tests in a FRESH process, with PHYS_DEBUG_* switches in the environment (the library reads them once
per process; tools/solver_probe.py): the material instances of ONE solver path on one scene.

    material_probe.py c5:16:130:16 --path percolour [--pre 4] [--steps 8] [--ref 3] [--inertia full]

paths: default | cluster (PHYS_FLAG_SOLVER_CLUSTER) | percolour (PHYS_FLAG_SOLVER_PER_COLOR)
What it does, every world stepped pre + steps updates and compared on every bit of poses, velocities and manifolds:
  * defaults:   no material call against (cfg.friction, 0) set on bodies and ground;
  * uniform f': a world configured with cfg.friction = f' against the default configuration with the material f' on
                bodies and ground, f' in 0, 0.2, 0.9;
  * --ref N:    random materials (friction in [0, 1.2], restitution in [0, 0.8] on half the bodies, ground 0.7 / 0.3,
                threshold 0.1 so that settling contacts do bounce), N warm-started updates against the float64 reference
                (tests/material_ref.py feeding tests/contact_ref.py).
  * --inertia full: every body gets a symmetric positive definite, non-diagonal tensor (the DIAG = false instances).
Output (one line): defaults=identical|different uniform=identical|different plain_ran=<stages> mat_ran=<stages>
[ref_err=<worst velocity difference> ref_ambiguous=<share> ref_bounces=<points>] manifolds=<n> colours=<n>"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import physics_amd  # noqa: E402
from physics_amd import scenes  # noqa: E402

DT = 16_666_667
DT_S = float(np.float32(np.float32(DT) / np.float32(1e9)))
G = (0.0, -9.81, 0.0)
FLAGS = {"default": 0, "cluster": physics_amd.FLAG_SOLVER_CLUSTER, "percolour": physics_amd.FLAG_SOLVER_PER_COLOR}


def make_scene(spec):
    parts = spec.split(":")
    dims = [int(x) for x in parts[1:]]
    return {"c5": scenes.c5, "c3": scenes.c3}[parts[0]](*dims) if dims else scenes.SCENES[parts[0]]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--path", default="percolour")
    ap.add_argument("--pre", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--ref", type=int, default=0)
    ap.add_argument("--inertia", default="identity")
    args = ap.parse_args()
    sc = make_scene(args.scene)
    n = len(sc.pos)
    bodies = dict(pos=sc.pos, shape_type=sc.shape_type, half_extent=sc.half_extent)
    if args.inertia == "full":
        rng = np.random.default_rng(31)
        A = rng.normal(size=(n, 3, 3))
        bodies["inertia"] = (A @ A.transpose(0, 2, 1) + 1.5 * np.eye(3)).reshape(n, 9).astype(np.float32)
    flags = physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_GROUND_PLANE | FLAGS[args.path]

    def world(**cfg):
        w = physics_amd.World(physics_amd.default_config(flags=flags, gravity_force=G, gravity_offset=(0.0, 0.0, 0.0), **cfg))
        w.set_bodies(**bodies)
        return w

    def run(w):
        w.update_n(DT, args.pre)
        w.profile_enable(True)
        w.update_n(DT, args.steps)
        w.sync()
        prof, _ = w.profile_get()
        st = w.get_stats()
        assert st.overflow == 0, st.overflow
        out = [x.view(np.uint32) for x in list(w.get_transforms()) + list(w.get_velocities()) + list(w.get_manifolds())]
        w.close()
        return out, "+".join(sorted(s for s in prof if s.startswith("solve"))), st

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    plain, plain_ran, st = run(world())
    w = world()
    w.set_body_materials(np.full(n, w.cfg.friction, np.float32), np.zeros(n, np.float32))
    w.set_ground_material(w.cfg.friction, 0.0)
    mat, mat_ran, _ = run(w)
    line = f"defaults={'identical' if same(plain, mat) else 'different'}"
    uniform = True
    for fr in (0.0, 0.2, 0.9):
        a, ran_a, _ = run(world(friction=fr))
        w = world()
        w.set_body_materials(friction=fr)
        w.set_ground_material(fr, 0.0)
        b, ran_b, _ = run(w)
        uniform = uniform and same(a, b) and ran_a == plain_ran and ran_b == mat_ran
    line += f" uniform={'identical' if uniform else 'different'} plain_ran={plain_ran} mat_ran={mat_ran}"
    if args.ref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import contact_ref as cr
        import material_ref as mr
        rng = np.random.default_rng(32)
        fr = rng.uniform(0.0, 1.2, n).astype(np.float32)
        re = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.8, n), 0.0).astype(np.float32)
        mats = mr.Materials(fr, re, ground=(np.float32(0.7), np.float32(0.3)), threshold=np.float32(0.1))
        w = world()
        w.set_body_materials(fr, re)
        w.set_ground_material(0.7, 0.3)
        w.set_restitution_threshold(0.1)
        sref = mr.MaterialSolverRef(n, cr.Params(DT_S), 8)
        inv_m, inv_I = cr.body_inverses(n, None, bodies.get("inertia"))
        worst, amb_share, bounces = 0.0, 0.0, 0
        for u in range(args.ref):
            if u == 1:
                w.profile_enable(True)  # (a world's first update has no counts of an earlier one to choose its path by)
            pos, _r = w.get_transforms()
            lin, ang = w.get_velocities()
            w.update(DT)
            w.sync()
            out = sref.update(w.get_manifolds(), pos, lin, ang, inv_m, inv_I, np.array(G), materials=mats)
            lin1, ang1 = w.get_velocities()
            err, amb = cr.velocity_error(out, lin1, ang1)
            worst = max(worst, err)
            amb_share = max(amb_share, amb / max(1, len(out["a"])))
            bounces += int(out["bounces"].sum())
        prof, _ = w.profile_get()
        ref_ran = "+".join(sorted(s for s in prof if s.startswith("solve")))
        w.close()
        line += f" ref_err={worst:.3g} ref_ambiguous={amb_share:.4f} ref_bounces={bounces} ref_ran={ref_ran}"
    print(line + f" manifolds={st.n_manifolds} colours={st.n_colors}")


if __name__ == "__main__":
    main()
