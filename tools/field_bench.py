"""Cost of force fields on C5, the benchmark's 256k-box tower, and on the settled 1M cubes.

    python tools/field_bench.py [--scenes c5,t1m_settled] [--cases none,drag,mixed64,small1024] [--steps 200] [--warmup 20]
                                [--reps 5] [--json out.json]

One case per (scene, field set), each in a FRESH process (this script again with --case): the scene is stepped to the state
bench.py measures (its preroll), the field set is given, `warmup` updates, then `reps` windows of `steps` updates each timed on
the wall clock around update_n + sync (the timing of bench.py), then 20 profiled updates for the device time of
PHYS_STAGE_MISC, where the field kernel is accounted, and of the velocity stage, whose FORCES instance reads and zeroes the
accumulators the fields wrote. The field sets:

    none       phys_set_force_fields is never called
    drag       one DRAG box over the whole scene: the damping the library lacked (velocity record read, every body acted on)
    mixed64    64 fields of mixed kinds and shapes, 2 to 8 body diameters, random rotations, spread over the scene's bounds
    small1024  1024 fields of 1 to 2 body diameters: the record loop at its longest, few bodies acted on

All strengths are small (a drag of 1e-3, accelerations of 1e-2), so the pile stays the pile the other cases measure. Reported
per case: steps per second and ms per update (median, min and max of the windows), misc and velocity-stage ms and launches per
update, and the bodies at least one field acts on at the end."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PROFILED = 20
CASES = ("none", "drag", "mixed64", "small1024")


def field_set(case, lo, hi):
    import physics_amd as pa
    if case == "drag":
        c, h = (lo + hi) / 2, (hi - lo) / 2 + 10.0
        return dict(kind=pa.FIELD_DRAG, shape_type=pa.SHAPE_BOX, pos=[c], half_extent=[h], coef=[1e-3, 1e-3])
    count, size = (64, (2.0, 8.0)) if case == "mixed64" else (1024, (1.0, 2.0))
    rng = np.random.default_rng(23)
    q = rng.normal(size=(count, 4))
    kind = rng.integers(0, 3, count).astype(np.uint32)
    coef = np.stack([np.full(count, 1e-3), np.full(count, 1.0)], axis=1).astype(np.float32)
    coef[kind == pa.FIELD_RADIAL, 0] = -1e-2  # weak attractors
    return dict(kind=kind, shape_type=rng.integers(1, 4, count).astype(np.uint32), pos=rng.uniform(lo, hi, (count, 3)).astype(np.float32),
                rot=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                half_extent=rng.uniform(*size, (count, 3)).astype(np.float32),  # the scenes' bodies are unit cubes
                vec=(rng.normal(size=(count, 3)) * 1e-2).astype(np.float32), coef=coef, exponent=rng.integers(0, 3, count).astype(np.uint32))


def run_case(scene, case, args):
    from physics_amd import scenes
    from raycast_bench import settled_world
    sc, w = settled_world(scene)
    n_fields = 0
    if case != "none":
        pos, _ = w.get_transforms()
        fs = field_set(case, pos.min(0), pos.max(0))
        w.set_force_fields(**fs)
        n_fields = w.n_fields
    w.update_n(scenes.DT_NANOS, args.warmup)
    w.sync()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        w.update_n(scenes.DT_NANOS, args.steps)
        w.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    w.profile_enable(True)
    w.update_n(scenes.DT_NANOS, PROFILED)
    w.sync()
    prof, steps = w.profile_get()
    w.profile_enable(False)
    med = statistics.median(ms)
    out = {"scene": scene, "case": case, "fields": n_fields, "bodies": int(sc.n), "steps_per_s": 1e3 / med, "ms_per_update": med,
           "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms, "misc_ms": prof.get("misc", (0.0, 0))[0] / steps,
           "misc_launches": prof.get("misc", (0.0, 0))[1] / steps, "velocity_ms": prof.get("velocity_aabb", (0.0, 0))[0] / steps,
           "velocity_launches": prof.get("velocity_aabb", (0.0, 0))[1] / steps}
    if n_fields:
        w.set_forces(np.zeros((sc.n, 3), np.float32), np.zeros((sc.n, 3), np.float32))
        w.apply_force_fields()
        f, t = w.get_forces()
        out["bodies_acted_on"] = int(((f != 0).any(1) | (t != 0).any(1)).sum())
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5,t1m_settled")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # scene:case, run in this process
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.case:
        scene, case = args.case.split(":")
        print(json.dumps(run_case(scene, case, args)), flush=True)
        return
    results = []
    for scene in args.scenes.split(","):
        for case in args.cases.split(","):
            if case not in CASES:
                raise SystemExit(f"unknown case {case}: one of {', '.join(CASES)}")
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{scene}:{case}", "--steps", str(args.steps), "--warmup",
                   str(args.warmup), "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"case {scene}:{case} failed (exit {r.returncode}): {r.stderr[-2000:]}")
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
