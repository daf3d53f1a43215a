"""Cost of static colliders (phys_set_static_bodies) on C5, in steps/s.

    python tools/static_bench.py [--steps 100] [--warmup 30] [--reps 3] [--json out.json]

Variants of C5 (16 x 1000 x 16 falling cubes, bench.py's flagship scene):
  c5          as it is (ground plane, no static set ever given)
  c5_zero     phys_set_static_bodies with n = 0 (the static-pair pass must not run)
  c5_slab     the ground plane replaced by one static slab with its top at the plane's height
  c5_box      no ground plane: a static box of five walls (floor + four sides) around the tower, and 400 small static
              pillars standing on the floor around it (the grid and the large list both in use)
Each variant: `warmup` updates, then `reps` timed runs of `steps` back-to-back updates (phys_update_n + phys_sync,
wall clock); the median run gives steps/s. The time of the static-pair kernels themselves comes from phys_profile
(stage PHYS_STAGE_PAIRS also holds k_find_pairs): --profile adds one profiled run per variant."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def statics_for(variant, sc):
    import physics_amd
    box, sph = physics_amd.SHAPE_BOX, physics_amd.SHAPE_SPHERE
    lo, hi = sc.pos.min(axis=0), sc.pos.max(axis=0)
    cx, cz = (lo[0] + hi[0]) / 2, (lo[2] + hi[2]) / 2
    if variant == "c5_zero":
        return np.zeros((0, 3), np.float32), None, np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)
    if variant == "c5_slab":
        return (np.array([[cx, -1.0, cz]], np.float32), None, np.array([box], np.uint32),
                np.array([[200.0, 1.0, 200.0]], np.float32))
    # c5_box: floor + four walls with 8 units of room on every side, pillars on the floor outside the tower's footprint
    x0, x1, z0, z1 = lo[0] - 8, hi[0] + 8, lo[2] - 8, hi[2] + 8
    hx, hz, hh = (x1 - x0) / 2, (z1 - z0) / 2, (hi[1] + 20) / 2
    pos = [[cx, -1, cz], [x0 - 1, hh, cz], [x1 + 1, hh, cz], [cx, hh, z0 - 1], [cx, hh, z1 + 1]]
    he = [[hx + 2, 1, hz + 2], [1, hh, hz + 2], [1, hh, hz + 2], [hx, hh, 1], [hx, hh, 1]]
    shape = [box] * 5
    rng = np.random.default_rng(0)
    k = 0
    while k < 400:
        x, z = rng.uniform(x0 + 0.5, x1 - 0.5), rng.uniform(z0 + 0.5, z1 - 0.5)
        if lo[0] - 2 < x < hi[0] + 2 and lo[2] - 2 < z < hi[2] + 2:
            continue
        r = rng.uniform(0.2, 0.5)
        if k % 2:
            pos.append([x, r, z]); he.append([r, r, r]); shape.append(sph)
        else:
            pos.append([x, 1.5, z]); he.append([r, 1.5, r]); shape.append(box)
        k += 1
    return np.array(pos, np.float32), None, np.array(shape, np.uint32), np.array(he, np.float32)


def make_world(variant):
    import physics_amd
    from physics_amd import scenes
    sc = scenes.c5()
    flags = sc.flags
    if variant in ("c5_slab", "c5_box"):
        flags &= ~physics_amd.FLAG_GROUND_PLANE
    w = physics_amd.World(sc.config(flags=flags))
    sc.populate(w)
    if variant != "c5":
        pos, rot, shape, he = statics_for(variant, sc)
        w.set_static_bodies(pos, rot=rot, shape_type=shape, half_extent=he)
    return w


def run(variant, steps, warmup, reps, profile):
    from physics_amd import scenes
    w = make_world(variant)
    w.update_n(scenes.DT_NANOS, warmup)
    w.sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        w.update_n(scenes.DT_NANOS, steps)
        w.sync()
        times.append(time.perf_counter() - t0)
    out = {"variant": variant, "steps_per_s": steps / statistics.median(times), "runs_s": times}
    out["static_stats"] = list(w.get_static_stats())
    st = w.get_stats()
    out["n_manifolds"] = int(st.n_manifolds)
    if profile:
        w.profile_enable(True)
        w.update_n(scenes.DT_NANOS, 10)
        w.sync()
        prof, n = w.profile_get()
        out["profile_ms_per_update"] = {k: v[0] / max(n, 1) for k, v in prof.items() if v[1]}
        w.profile_enable(False)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="c5,c5_zero,c5_slab,c5_box")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = []
    for v in a.variants.split(","):
        r = run(v, a.steps, a.warmup, a.reps, a.profile)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
