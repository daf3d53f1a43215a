"""Cost of trigger volumes on C5, the benchmark's 256k-box tower, and on the settled 1M cubes.

    python tools/trigger_bench.py [--scenes c5,t1m_settled] [--triggers 0,16,256,1024] [--steps 200] [--warmup 20] [--reps 5]
                                  [--capacity 1048576] [--json out.json]

One case per (scene, trigger count), each in a FRESH process (this script again with --case): the scene is stepped to the
state bench.py measures (its preroll), `count` box triggers are spread over the scene's bounds (sizes 1 to 4 body
diameters, random rotations; 0: phys_set_triggers is never called) with trigger events on, `warmup` updates, then `reps`
windows of `steps` updates each timed on the wall clock around update_n + sync (the timing of bench.py), then 20 profiled
updates for the device time of PHYS_STAGE_MISC, where the trigger kernel is accounted. The events are drained after the
warm-up and after every window. Reported per case: ms per update (median, min and max of the windows), misc ms and
launches per update, occupant pairs at the end, events per update, dropped events, and the occupancy bytes on the device."""
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


def spread_triggers(rng, count, lo, hi):
    pos = rng.uniform(lo, hi, (count, 3)).astype(np.float32)
    q = rng.normal(size=(count, 4))
    rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    he = rng.uniform(1.0, 4.0, (count, 3)).astype(np.float32)  # the scenes' bodies are unit cubes: 1 to 4 diameters
    return pos, rot, he


def run_case(scene, count, args):
    import physics_amd as pa
    from physics_amd import scenes
    from raycast_bench import settled_world
    sc, w = settled_world(scene)
    if count:
        pos, _ = w.get_transforms()
        tp, tq, th = spread_triggers(np.random.default_rng(17), count, pos.min(0), pos.max(0))
        w.set_triggers(pa.SHAPE_BOX, tp, rot=tq, half_extent=th)
        w.enable_trigger_events(args.capacity)
    w.update_n(scenes.DT_NANOS, args.warmup)
    w.sync()
    events = dropped = 0
    if count:
        w.get_trigger_events()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        w.update_n(scenes.DT_NANOS, args.steps)
        w.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
        if count:
            ev, d = w.get_trigger_events()
            events += len(ev) + d
            dropped += d
    w.profile_enable(True)
    w.update_n(scenes.DT_NANOS, PROFILED)
    w.sync()
    prof, steps = w.profile_get()
    w.profile_enable(False)
    out = {"scene": scene, "triggers": count, "bodies": int(sc.n), "ms_per_update": statistics.median(ms), "ms_min": min(ms),
           "ms_max": max(ms), "ms_all": ms, "misc_ms": prof.get("misc", (0.0, 0))[0] / steps,
           "misc_launches": prof.get("misc", (0.0, 0))[1] / steps}
    if count:
        off, _ = w.get_trigger_overlaps()
        out.update({"occupant_pairs": int(off[-1]), "events_per_update": events / (args.reps * args.steps), "dropped": int(dropped),
                    "occupancy_bytes": 4 * ((count + 31) // 32) * int(sc.n)})
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5,t1m_settled")
    ap.add_argument("--triggers", default="0,16,256,1024")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # scene:count, run in this process
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.case:
        scene, count = args.case.split(":")
        print(json.dumps(run_case(scene, int(count), args)), flush=True)
        return
    results = []
    for scene in args.scenes.split(","):
        for count in args.triggers.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{scene}:{count}", "--steps", str(args.steps), "--warmup",
                   str(args.warmup), "--reps", str(args.reps), "--capacity", str(args.capacity)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"case {scene}:{count} failed (exit {r.returncode}): {r.stderr[-2000:]}")
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
