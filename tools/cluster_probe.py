#!/usr/bin/env python3
"""Run by tests/test_gpu_cluster_variants.py in a FRESH process, with PHYS_DEBUG_* switches in the environment (the library
reads them once per process): the varied tower of tests/contact_ref.py under PHYS_FLAG_SOLVER_CLUSTER, and per update what
the float64 reference needs to restate it, written to one .npz file for the parent to judge. Nothing is compared here.

    cluster_probe.py --out OUT.npz --inertia diag|uniform|full [--updates 4] [--iterations 8]

OUT, per update u = 1..: u<u>.pos / .lin / .ang (the bodies in front of the update), u<u>.ids / .counts / .normals / .points
(get_manifolds), u<u>.pos1 / .rot1 / .lin1 / .ang1 (behind it), u<u>.stages (the solver stages that ran, joined by '+'),
u<u>.stats = [n_manifolds, n_colors, color_rounds, n_new_manifolds, overflow] and u<u>.color_counts.
Exit code 3, after printing the code and the overflow bits: an update ended with an error (no file is written)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import physics_amd  # noqa: E402

DT = 16_666_667


def main():
    import contact_ref as cr
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--inertia", required=True, choices=["diag", "uniform", "full"])
    ap.add_argument("--updates", type=int, default=cr.VARIED_UPDATES)
    ap.add_argument("--iterations", type=int, default=8)
    args = ap.parse_args()
    bodies = cr.varied_tower(cr.VARIED_SEED, args.inertia)
    flags = physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_GROUND_PLANE | physics_amd.FLAG_SOLVER_CLUSTER
    w = physics_amd.World(physics_amd.default_config(flags=flags, gravity_force=(0, -9.81, 0), gravity_offset=(0, 0, 0),
                                                     solver_iterations=args.iterations))
    w.set_bodies(**bodies)
    out = {}
    for u in range(1, args.updates + 1):
        out[f"u{u}.pos"] = w.get_transforms()[0]
        out[f"u{u}.lin"], out[f"u{u}.ang"] = w.get_velocities()
        w.profile_enable(True)
        try:
            w.update(DT)
            w.sync()
        except physics_amd.PhysError as e:
            print("update %d: error %d overflow=%d" % (u, e.code, w.get_stats().overflow))
            sys.exit(3)
        stages = sorted(s for s in w.profile_get()[0] if s.startswith("solve"))
        for field, a in zip(("ids", "counts", "normals", "points"), w.get_manifolds()):
            out[f"u{u}.{field}"] = a
        out[f"u{u}.pos1"], out[f"u{u}.rot1"] = w.get_transforms()
        out[f"u{u}.lin1"], out[f"u{u}.ang1"] = w.get_velocities()
        st = w.get_stats()
        out[f"u{u}.stages"] = np.array("+".join(stages))
        out[f"u{u}.stats"] = np.array([st.n_manifolds, st.n_colors, st.color_rounds, st.n_new_manifolds, st.overflow], np.uint64)
        out[f"u{u}.color_counts"] = np.asarray(w.get_color_counts())
        print(f"update {u}: {st.n_manifolds} manifolds, {st.n_colors} colours, {'+'.join(stages)}, overflow {st.overflow}")
    w.close()
    np.savez(args.out, **out)


if __name__ == "__main__":
    main()
