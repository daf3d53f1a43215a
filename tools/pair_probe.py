#!/usr/bin/env python3
"""Run by the GPU tests in a FRESH process, with PHYS_DEBUG_* switches in the environment (the library reads them once
per process): what the pair search and the narrow phase give under those switches, written to .npz files for the
parent to judge. Nothing is compared here.

    pair_probe.py pairs --out DIR --scenes sparse,dense [--n 33000] [--updates 0,3] [--capacity 10000]
        the scenes of tests/pair_ref.py in broad-phase-only worlds without gravity. Per scene and update count k one
        file DIR/<scene>_n<n>_u<k>.npz: `aabb` (get_aabbs) and `pairs` (broadphase, sorted) of the world as it stands
        after k updates and a sync - with k > 0 a hint exists, and the boxes read in front of the last of those updates
        (`aabb_before`) go with that update's pair count (`n_pairs_update`).
        --capacity: first a world of the scene with that max_pairs; the code broadphase() ends with is `capacity_code` of
        the scene's k = 0 file (0: no error), whose pairs then come from a correctly sized world in the same process.
    pair_probe.py narrow --input IN.npz --out OUT.npz
        IN: `names`, and per name <name>.pos / .rot / .shape / .he, optionally <name>.s_pos / .s_rot / .s_shape / .s_he
        (static colliders) and <name>.ground. Worlds as tests/test_gpu_independent.py's pair_world; two updates each.
        OUT: per name and update u = 1, 2 <name>.<u>.ids / .counts / .normals / .points (get_manifolds: sorted by ids),
        and <name>.stats = [manifolds, new manifolds] of update 2."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import physics_amd  # noqa: E402

DT = 16_666_667


def pair_world(sc, max_pairs):
    cfg = physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS | physics_amd.FLAG_BROADPHASE_ONLY,
                                     gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0), max_pairs=max_pairs)
    w = physics_amd.World(cfg)
    w.set_bodies(sc["pos"], rot=sc["rot"], shape_type=sc["shape"], half_extent=sc["he"])
    return w


def run_pairs(args):
    import pair_ref
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        sc = pair_ref.scene(name, args.n)
        code = 0
        if args.capacity:
            w = pair_world(sc, args.capacity)
            try:
                w.broadphase()
            except physics_amd.PhysError as e:
                code = e.code
            w.close()
        for k in [int(x) for x in args.updates.split(",")]:
            w = pair_world(sc, pair_ref.MAX_PAIRS.get(name, 0))
            out = {"capacity_code": code}
            if k > 0:
                if k > 1:
                    w.update_n(DT, k - 1)
                w.sync()
                out["aabb_before"] = w.get_aabbs()
                w.update(DT)
                w.sync()
                out["n_pairs_update"] = w.get_stats().n_pairs
            out["aabb"] = w.get_aabbs()
            out["pairs"] = w.broadphase()
            out["n_pairs"] = w.get_stats().n_pairs
            w.close()
            np.savez(os.path.join(args.out, f"{name}_n{args.n}_u{k}.npz"), **out)
            print(f"{name} n={args.n} updates={k}: {len(out['pairs'])} pairs, capacity code {code}")


def run_narrow(args):
    src = np.load(args.input)
    out = {}
    for name in src["names"].tolist():
        ground = f"{name}.ground" in src.files and bool(src[f"{name}.ground"])
        flags = physics_amd.FLAG_COLLISIONS | (physics_amd.FLAG_GROUND_PLANE if ground else 0)
        w = physics_amd.World(physics_amd.default_config(flags=flags, gravity_force=(0, 0, 0), gravity_offset=(0, 0, 0)))
        w.set_bodies(src[f"{name}.pos"], rot=src[f"{name}.rot"], shape_type=src[f"{name}.shape"], half_extent=src[f"{name}.he"])
        if f"{name}.s_pos" in src.files:
            w.set_static_bodies(src[f"{name}.s_pos"], rot=src[f"{name}.s_rot"], shape_type=src[f"{name}.s_shape"],
                                half_extent=src[f"{name}.s_he"])
        for u in (1, 2):
            w.update(DT)
            w.sync()
            for field, a in zip(("ids", "counts", "normals", "points"), w.get_manifolds()):
                out[f"{name}.{u}.{field}"] = a
        st = w.get_stats()
        out[f"{name}.stats"] = np.array([st.n_manifolds, st.n_new_manifolds], np.uint64)
        w.close()
        print(f"{name}: {len(out[f'{name}.1.ids'])} manifolds, then {st.n_manifolds}, {st.n_new_manifolds} of them new")
    np.savez(args.out, **out)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("pairs")
    p.add_argument("--out", required=True)
    p.add_argument("--scenes", required=True)
    p.add_argument("--n", type=int, default=33000)
    p.add_argument("--updates", default="0")
    p.add_argument("--capacity", type=int, default=0)
    q = sub.add_parser("narrow")
    q.add_argument("--input", required=True)
    q.add_argument("--out", required=True)
    args = ap.parse_args()
    (run_pairs if args.mode == "pairs" else run_narrow)(args)


if __name__ == "__main__":
    main()
