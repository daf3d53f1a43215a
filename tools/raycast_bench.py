"""Ray-cast throughput (phys_raycast_device / phys_raycast) on the benchmark scenes.

    python tools/raycast_bench.py [--scenes c2,c3,c5,t1m_settled] [--rays 1000000] [--warmup 5] [--calls 20] [--reps 5]
                                  [--stats] [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (its preroll: c2 / c3 settled after 150 updates, c5 after
30, the 1M cubes after 600), then 1M random rays - a third from inside the bodies' bounds, a third from outside aimed into
them, a third along the ground - are cast on the world's stream, timed with device events: `warmup` calls, then `reps`
repetitions of `calls` back-to-back calls of phys_raycast_device (grid build + traversal, device pointers). Reported: ms
per call (median, min, max over the repetitions) and rays/s from the median; the host variant phys_raycast (staging,
launches, copy-back, synchronisation) timed on the wall clock the same way.

--stats adds the mean cells and candidates visited per ray, counted by the kernel itself in a child process with
PHYS_DEBUG_RAYCAST_STATS set (the switch is read once per process). The split between the grid build and the traversal
comes from a run of its own under `rocprofv3 --kernel-trace --stats` (kernels k_rc_*; k_rc_trace is the traversal)."""
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

PREROLL = {"c2": 150, "c3": 150, "c5": 30, "t1m_settled": 600}


def make_rays(rng, n, lo, hi):
    k = n // 3
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, size = (lo + hi) / 2, float((hi - lo).max())
    o1 = rng.uniform(lo, hi, (k, 3))
    d1 = rng.normal(size=(k, 3))
    v = rng.normal(size=(k, 3))
    o2 = c + 2.0 * size * v / np.linalg.norm(v, axis=1, keepdims=True)
    d2 = rng.uniform(lo, hi, (k, 3)) - o2
    m = n - 2 * k
    o3 = np.column_stack([rng.uniform(lo[0], hi[0], m), rng.uniform(0.001, 0.5, m), rng.uniform(lo[2], hi[2], m)])
    d3 = np.column_stack([rng.normal(size=m), rng.uniform(-0.2, 0.2, m), rng.normal(size=m)])
    return np.concatenate([o1, o2, o3]).astype(np.float32), np.concatenate([d1, d2, d3]).astype(np.float32)


def settled_world(key):
    import physics_amd
    from physics_amd import scenes
    sc = scenes.SCENES[key]()
    w = physics_amd.World(sc.config())
    sc.populate(w)
    left = PREROLL[key]
    while left:
        k = min(left, 50)
        w.update_n(scenes.DT_NANOS, k)
        w.sync()
        left -= k
    return sc, w


def bench_scene(key, args):
    import torch
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    rng = np.random.default_rng(0)
    o, d = make_rays(rng, args.rays, pos.min(0) - 2.0, pos.max(0) + 2.0)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tb = torch.empty(args.rays, dtype=torch.int32, device=dev)
    tt = torch.empty(args.rays, dtype=torch.float32, device=dev)
    tn = torch.empty((args.rays, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    for _ in range(args.warmup):
        w.raycast_device(to, td, tb, tt, tn)
    w.sync()
    dev_ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            w.raycast_device(to, td, tb, tt, tn)
        b.record(stream)
        b.synchronize()
        dev_ms.append(a.elapsed_time(b) / args.calls)
    host_ms = []
    for _ in range(max(1, args.reps)):
        t0 = time.perf_counter()
        for _ in range(max(1, args.calls // 4)):
            body, t, _ = w.raycast(o, d)
        host_ms.append((time.perf_counter() - t0) * 1e3 / max(1, args.calls // 4))
    hits = int((body < sc.n).sum())
    ground = int((body == 0xFFFFFFFF).sum())
    med = statistics.median(dev_ms)
    out = {"scene": key, "bodies": int(sc.n), "rays": args.rays, "body_hits": hits, "ground_hits": ground,
           "device_ms_per_call": {"median": med, "min": min(dev_ms), "max": max(dev_ms)},
           "device_rays_per_s": args.rays / (med * 1e-3),
           "host_ms_per_call": {"median": statistics.median(host_ms), "min": min(host_ms), "max": max(host_ms)},
           "host_rays_per_s": args.rays / (statistics.median(host_ms) * 1e-3)}
    w.close()
    return out


def count_visits(key, args):
    """mean cells / candidates per ray: one call in a child process with the counting kernel switched on"""
    env = dict(os.environ, PHYS_DEBUG_RAYCAST_STATS="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--scenes", key, "--rays", str(args.rays), "--count-only"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    for line in r.stderr.splitlines()[::-1]:
        if line.startswith("PHYS_RAYCAST_STATS"):
            f = dict(kv.split("=") for kv in line.split()[1:])
            n = int(f["rays"])
            return {"cells_per_ray": int(f["cells"]) / n, "candidates_per_ray": int(f["candidates"]) / n}
    raise RuntimeError(f"no PHYS_RAYCAST_STATS line from the counting run (exit {r.returncode}): {r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c2,c3,c5,t1m_settled")
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats", action="store_true", help="also count cells and candidates per ray (child process)")
    ap.add_argument("--count-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    keys = args.scenes.split(",")
    if args.count_only:
        _, w = settled_world(keys[0])
        pos, _ = w.get_transforms()
        o, d = make_rays(np.random.default_rng(0), args.rays, pos.min(0) - 2.0, pos.max(0) + 2.0)
        w.raycast(o, d)
        w.close()
        return
    results = []
    for key in keys:
        r = bench_scene(key, args)
        if args.stats:
            r.update(count_visits(key, args))
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
