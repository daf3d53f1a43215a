"""Cost of continuous collision: a collision scene with static colliders, and 0 %, 1 % and 100 % of its
bodies listed.

    python tools/ccd_bench.py [--scenes c2,c5] [--statics 1024] [--cases 0,1,100] [--steps 200] [--warmup 20] [--reps 5] [--json out.json]

One case per (scene, listed share), each in a FRESH process (this script again with --case): the scene is stepped to the state
bench.py measures (its preroll); `statics` small boxes and spheres are scattered beside and over the pile (none touches it, so
the pile stays the pile the other cases measure); the listed share of the bodies, spread evenly over the ids, is given to
phys_set_ccd_bodies (0: the call is never made); `warmup` updates, then `reps` windows of `steps` updates each timed on the wall
clock around update_n + sync (the timing of bench.py), then 20 profiled updates for the device time of PHYS_STAGE_MISC, where
the sweep kernel is accounted, and of the position stage, whose CCD instance reads the share of dt per body. That stage also
holds the memset that restarts the extent bound in every 32nd update, so the sweep's own time is reported as what the case adds
to the stage over the scene's 0 % case (sweep_ms; run the 0 % case first, as the default order does).

Reported per case: steps per second and ms per update (median, min and max of the windows), the misc stage's, the sweep's and the
position stage's ms and launches per update, the listed bodies, the box rejects per update (listed x statics) and how many entries were stopped
at least once."""
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


def static_set(n, lo, hi):
    """n small boxes and spheres in a shell around the pile's bounds: beside it and over it, clear of every body"""
    rng = np.random.default_rng(31)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1])  # not under the ground
    d /= np.abs(d).max(1, keepdims=True)
    pos = c + d * (h + rng.uniform(2.0, 6.0, (n, 1)))
    shape = rng.choice([1, 2], size=n).astype(np.uint32)
    return dict(pos=pos.astype(np.float32), shape_type=shape, half_extent=rng.uniform(0.2, 0.8, (n, 3)).astype(np.float32))


def run_case(scene, share, args):
    from physics_amd import scenes
    from raycast_bench import settled_world
    sc, w = settled_world(scene)
    pos, _ = w.get_transforms()
    if args.statics:
        w.set_static_bodies(**static_set(args.statics, pos.min(0), pos.max(0)))
    n = int(sc.n)
    listed = 0
    if share > 0:
        ids = np.unique(np.linspace(0, n - 1, max(1, n * share // 100)).astype(np.uint32))
        w.set_ccd_bodies(ids)
        listed = len(ids)
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
    out = {"scene": scene, "listed_percent": share, "listed": listed, "statics": args.statics, "bodies": n, "steps_per_s": 1e3 / med,
           "ms_per_update": med, "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms, "misc_stage_ms": prof.get("misc", (0.0, 0))[0] / steps,
           "misc_stage_launches": prof.get("misc", (0.0, 0))[1] / steps, "position_ms": prof.get("position", (0.0, 0))[0] / steps,
           "position_launches": prof.get("position", (0.0, 0))[1] / steps, "box_rejects_per_update": listed * args.statics}
    if listed:
        out["entries_stopped"] = int((w.ccd_hits()[3] > 0).sum())
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5")
    ap.add_argument("--statics", type=int, default=1024)
    ap.add_argument("--cases", default="0,1,100")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # scene:share, run in this process
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.case:
        scene, share = args.case.split(":")
        print(json.dumps(run_case(scene, int(share), args)), flush=True)
        return
    results = []
    for job in [f"{scene}:{int(share)}" for scene in args.scenes.split(",") if scene for share in args.cases.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", job, "--statics", str(args.statics), "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"case {job} failed (exit {r.returncode}): {r.stderr[-2000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        # the stage also holds the memset that restarts the extent bound: the sweep's own time is what a list adds to the stage
        base = [x for x in results if x["scene"] == results[-1]["scene"] and x["listed_percent"] == 0]
        if base:
            results[-1]["sweep_ms"] = results[-1]["misc_stage_ms"] - base[0]["misc_stage_ms"]
            results[-1]["sweep_launches"] = results[-1]["misc_stage_launches"] - base[0]["misc_stage_launches"]
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
