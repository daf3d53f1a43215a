"""Cost of liquids on C5, the benchmark's 256k-box tower, and on the settled 1M cubes, and of the
kernel alone per body shape.

    python tools/liquid_bench.py [--scenes c5,t1m_settled] [--cases none,ocean,pools64] [--steps 200] [--warmup 20] [--reps 5]
                                 [--shapes sphere,box,capsule] [--json out.json]

One case per (scene, liquid set), each in a FRESH process (this script again with --case): the scene is stepped to the state
bench.py measures (its preroll), the liquid set is given, `warmup` updates, then `reps` windows of `steps` updates each timed
on the wall clock around update_n + sync (the timing of bench.py), then 20 profiled updates for the device time of
PHYS_STAGE_MISC, where the liquid kernel is accounted, and of the velocity stage, whose FORCES instance reads and zeroes the
accumulators the liquids wrote. The liquid sets:

    none     phys_set_liquids is never called
    ocean    one liquid over the whole scene with drag, its surface at 90 % of the scene's height: most bodies wet, a layer cut
    pools64  64 tilted pools of 4 to 16 body diameters spread over the scene's bounds, with masks

All densities and drags are small (1e-3), so the pile stays the pile the other cases measure. Reported per case: steps per second
and ms per update (median, min and max of the windows), misc and velocity-stage ms and launches per update, the bodies a liquid
acts on at the end and how many of them are cut by a surface, and the bytes per body the kernel moves by its own code: 44 of pose
and shape, 32 more with drag, 8 more with masks, 48 of accumulators per acted-on body.

Then, per shape, the kernel alone: 262 144 bodies of that shape at random attitudes in a slab around an ocean's surface (a
third dry, a third cut, a third wet), phys_apply_liquids timed by the profiler over 20 calls; the ratio of the cut third's cost
shows whether the kernel is bound by its bytes or by the clip's instructions (the bytes per body are the same for all three)."""
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
CASES = ("none", "ocean", "pools64")
SHAPES = {"sphere": 1, "box": 2, "capsule": 3}


def liquid_set(case, lo, hi):
    if case == "ocean":
        c, h = (lo + hi) / 2, (hi - lo) / 2 + 10.0
        level = lo[1] + 0.9 * (hi[1] - lo[1])
        bottom = lo[1] - 10.0
        return dict(pos=[[c[0], (level + bottom) / 2, c[2]]], half_extent=[[h[0], (level - bottom) / 2, h[2]]], density=1e-3,
                    gravity=[0.0, -9.81, 0.0], drag=[1e-3, 1e-3])
    rng = np.random.default_rng(29)
    axis = rng.normal(size=(64, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.0, 0.5, 64)
    return dict(pos=rng.uniform(lo, hi, (64, 3)).astype(np.float32),
                rot=np.concatenate([axis * np.sin(half)[:, None], np.cos(half)[:, None]], axis=1).astype(np.float32),
                half_extent=rng.uniform(4.0, 16.0, (64, 3)).astype(np.float32), mask=rng.integers(1, 0x10000, 64).astype(np.uint16),
                density=1e-3, gravity=[0.0, -9.81, 0.0], flow=(rng.normal(size=(64, 3)) * 1e-2).astype(np.float32), drag=[1e-3, 1e-3])


def bytes_per_body(drag, masked):
    return 44 + (32 if drag else 0) + (8 if masked else 0)


def run_case(scene, case, args):
    from physics_amd import scenes
    from raycast_bench import settled_world
    sc, w = settled_world(scene)
    if case != "none":
        pos, _ = w.get_transforms()
        w.set_liquids(**liquid_set(case, pos.min(0), pos.max(0)))
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
    out = {"scene": scene, "case": case, "liquids": w.n_liquids, "bodies": int(sc.n), "steps_per_s": 1e3 / med, "ms_per_update": med,
           "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms, "misc_ms": prof.get("misc", (0.0, 0))[0] / steps,
           "misc_launches": prof.get("misc", (0.0, 0))[1] / steps, "velocity_ms": prof.get("velocity_aabb", (0.0, 0))[0] / steps,
           "velocity_launches": prof.get("velocity_aabb", (0.0, 0))[1] / steps}
    if w.n_liquids:
        frac, _ = w.get_submersion()
        out["bodies_acted_on"] = int((frac > 0).sum())
        out["bodies_cut"] = int(((frac > 0) & (frac < 1)).sum())
        out["bytes_per_body"] = bytes_per_body(True, case == "pools64")
        out["bytes_per_acted_on_body"] = 48
    w.close()
    return out


def run_shape(name, args):
    import physics_amd as pa
    n = 262144
    rng = np.random.default_rng(31)
    q = rng.normal(size=(n, 4))
    pos = rng.uniform([-200, -3, -200], [200, 3, 200], (n, 3)).astype(np.float32)
    w = pa.World(pa.default_config())
    w.set_bodies(pos, rot=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32), shape_type=np.full(n, SHAPES[name], np.uint32),
                 half_extent=np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (n, 1)))
    out = {"shape": name, "bodies": n}
    # the surface at y = +10: every body wet whole (the rule's short answer); at y = 0: a third of them cut
    for label, level in (("wet_ms", 10.0), ("cut_ms", 0.0)):
        w.set_liquids([[0, level - 20.0, 0]], half_extent=[300, 20, 300], density=1.0, gravity=[0.0, -9.81, 0.0], drag=[1.0, 1.0])
        for _ in range(3):
            w.apply_liquids()
        w.sync()
        w.profile_enable(True)
        for _ in range(PROFILED):
            w.apply_liquids()
        w.sync()
        prof, _ = w.profile_get()
        w.profile_enable(False)
        out[label] = prof.get("misc", (0.0, 0))[0] / PROFILED
        frac, _ = w.get_submersion()
        out[label.replace("_ms", "_cut_bodies")] = int(((frac > 0) & (frac < 1)).sum())
    out["bytes_per_body"] = bytes_per_body(True, False) + 48
    out["wet_GBps"] = out["bytes_per_body"] * n / (out["wet_ms"] * 1e-3) / 1e9 if out["wet_ms"] else None
    out["cut_GBps"] = out["bytes_per_body"] * n / (out["cut_ms"] * 1e-3) / 1e9 if out["cut_ms"] else None
    out["bound_by"] = "the clip's instructions" if out["cut_ms"] > 2 * out["wet_ms"] else "its bytes"
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5,t1m_settled")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # scene:case or shape:name, run in this process
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.case:
        scene, case = args.case.split(":")
        print(json.dumps(run_shape(case, args) if scene == "shape" else run_case(scene, case, args)), flush=True)
        return
    jobs = [f"{scene}:{case}" for scene in args.scenes.split(",") if scene for case in args.cases.split(",")]
    jobs += [f"shape:{name}" for name in args.shapes.split(",") if name]
    results = []
    for job in jobs:
        kind, case = job.split(":")
        if case not in (SHAPES if kind == "shape" else CASES):
            raise SystemExit(f"unknown case {case}")
        cmd = [sys.executable, os.path.abspath(__file__), "--case", job, "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps",
               str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"case {job} failed (exit {r.returncode}): {r.stderr[-2000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
