"""Cost of capsules (PHYS_SHAPE_CAPSULE) in steps/s and narrow-phase time.

    python tools/capsule_bench.py [--steps 100] [--warmup 30] [--reps 3] [--json out.json] [--variants ...] [--size 50,40,50]

Variants:
  capsules   scenes.capsule_pile on an nx x ny x nz lattice (default 50 x 40 x 50: 100 000 capsules), dropped on the plane
  boxes      the same lattice as unit cubes (scenes.falling_cubes): what the same drop costs with boxes
  c5         bench.py's flagship scene, unchanged: no capsule anywhere, so it runs the narrow phase without capsule code
Each variant: `warmup` updates, then `reps` timed runs of `steps` back-to-back updates (phys_update_n + phys_sync, wall
clock); the median run gives steps/s. Then 10 profiled updates (phys_profile) give the narrow-phase stage time
(PHYS_STAGE_NARROW, ms per update) and the other stages."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_scene(variant, size):
    from physics_amd import scenes
    nx, ny, nz = size
    if variant == "capsules":
        return scenes.capsule_pile(nx, ny, nz)
    if variant == "boxes":
        return scenes.falling_cubes(nx, ny, nz, f"BOXES_{nx * ny * nz}_pile")
    return scenes.c5()


def run(variant, size, steps, warmup, reps):
    import physics_amd
    from physics_amd import scenes
    sc = make_scene(variant, size)
    w = physics_amd.World(sc.config())
    sc.populate(w)
    w.update_n(scenes.DT_NANOS, warmup)
    w.sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        w.update_n(scenes.DT_NANOS, steps)
        w.sync()
        times.append(time.perf_counter() - t0)
    out = {"variant": variant, "scene": sc.name, "n": sc.n, "steps_per_s": steps / statistics.median(times), "runs_s": times}
    st = w.get_stats()
    out["n_manifolds"], out["n_contacts"] = int(st.n_manifolds), int(st.n_contacts)
    w.profile_enable(True)
    w.update_n(scenes.DT_NANOS, 10)
    w.sync()
    prof, n = w.profile_get()
    out["profile_ms_per_update"] = {k: v[0] / max(n, 1) for k, v in prof.items() if v[1]}
    out["narrow_ms"] = out["profile_ms_per_update"].get("narrow")
    w.profile_enable(False)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="capsules,boxes,c5")
    ap.add_argument("--size", default="50,40,50")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    size = tuple(int(x) for x in a.size.split(","))
    res = []
    for v in a.variants.split(","):
        r = run(v, size, a.steps, a.warmup, a.reps)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
