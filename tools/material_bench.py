"""Cost of materials on C5, the benchmark's 256k-box tower, and C3, the 100k mixed pile.

    python tools/material_bench.py [--scenes c5,c3] [--steps 200] [--warmup 60] [--reps 3] [--json out.json]

Three variants of each scene, each a fresh world stepped `warmup` updates and then timed over `steps` updates on the wall
clock (the timing of bench.py), `reps` times, followed by 10 profiled updates for the device time of the stages:
  - plain: no material call (the plain solver kernels);
  - defaults: (cfg.friction, 0) set explicitly on bodies and ground - the material kernels, producing the same bits;
  - random: friction in [0, 1.2] on every body, restitution in [0, 0.8] on half of them, the ground 0.7 / 0.3.
Reported per variant: steps/s (median and every repetition), PHYS_STAGE_ROWS ms and the solve stages' ms per update, the
solver stages that ran, and the manifolds of the last update. `defaults` against `plain` is the price of the feature."""
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

DT = 16_666_667
SOLVE_STAGES = ("solve", "solve_tail", "solve_flow", "solve_cluster")


def run_variant(scene, name, args):
    import physics_amd as pa
    from physics_amd import scenes
    sc = getattr(scenes, scene)()
    w = pa.World(sc.config())
    sc.populate(w)
    n = sc.n
    if name == "defaults":
        w.set_body_materials(np.full(n, w.cfg.friction, np.float32), np.zeros(n, np.float32))
        w.set_ground_material(w.cfg.friction, 0.0)
    elif name == "random":
        rng = np.random.default_rng(7)
        w.set_body_materials(rng.uniform(0.0, 1.2, n), np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.8, n), 0.0))
        w.set_ground_material(0.7, 0.3)
    w.update_n(DT, args.warmup)
    w.sync()
    rates = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        w.update_n(DT, args.steps)
        w.sync()
        rates.append(args.steps / (time.perf_counter() - t0))
    w.profile_enable(True)
    w.update_n(DT, 10)
    w.sync()
    prof, steps = w.profile_get()
    w.profile_enable(False)
    st = w.get_stats()
    solve = {k: prof[k][0] / steps for k in SOLVE_STAGES if k in prof and prof[k][0] > 0.0}
    out = {"scene": scene, "variant": name, "bodies": n, "steps_per_s": statistics.median(rates), "steps_per_s_all": rates,
           "rows_ms": prof["rows"][0] / steps, "solve_ms": sum(solve.values()), "solve_stages_ms": solve,
           "manifolds": int(st.n_manifolds), "colors": int(st.n_colors)}
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5,c3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    for scene in args.scenes.split(","):
        for name in ("plain", "defaults", "random"):
            r = run_variant(scene, name, args)
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
