"""Sphere-cast and overlap-query throughput (phys_spherecast_device / phys_overlap) on the benchmark scenes.

    python tools/query_bench.py [--scenes c2,c3,c5,t1m_settled] [--queries 1000000] [--warmup 3] [--calls 10] [--reps 3]
                                [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (tools/raycast_bench.py's preroll), then
  - 1M sphere casts of radius 0.25 and of radius 1.0 (raycast_bench.py's rays) through phys_spherecast_device, timed with
    device events on the world's stream: `warmup` calls, then `reps` repetitions of `calls` back-to-back calls;
  - 1M overlap queries each of unit spheres (radius 1), unit boxes (half extent 1, random rotations) and capsules (radius
    0.5, core half-length 1, random rotations), centred uniformly in the bodies' bounds, through phys_overlap (host arrays:
    staging, both passes, the ordering and the copy-back), timed on the wall clock.
The split between the grid build (k_rc_*, k_sc_grow) and the traversal (k_rc_trace, k_ov_query, k_ov_order) comes from a
run of its own under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from raycast_bench import make_rays, settled_world  # noqa: E402


def time_device(w, stream, fn, args):
    import torch
    for _ in range(args.warmup):
        fn()
    w.sync()
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / args.calls)
    return out


def time_host(fn, args):
    fn()
    out = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(max(1, args.calls // 2)):
            r = fn()
        out.append((time.perf_counter() - t0) * 1e3 / max(1, args.calls // 2))
    return out, r


def summary(ms, n):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "per_s": n / (med * 1e-3)}


def bench_scene(key, args):
    import torch
    import physics_amd as pa
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    lo, hi = pos.min(0), pos.max(0)
    rng = np.random.default_rng(0)
    n = args.queries
    o, d = make_rays(rng, n, lo - 2.0, hi + 2.0)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tb = torch.empty(n, dtype=torch.int32, device=dev)
    tt = torch.empty(n, dtype=torch.float32, device=dev)
    tn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    out = {"scene": key, "bodies": int(sc.n), "queries": n}
    for rad in (0.25, 1.0):
        tr = torch.full((n,), rad, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ms = time_device(w, stream, lambda: w.spherecast_device(to, td, tr, tb, tt, tn), args)
        hits = int((tb.cpu().numpy().view(np.uint32) < sc.n).sum())
        out[f"spherecast_r{rad}"] = dict(summary(ms, n), body_hits=hits)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    qp = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    for name, st, he, rot in (("overlap_sphere", pa.SHAPE_SPHERE, [1.0, 0, 0], None), ("overlap_box", pa.SHAPE_BOX, [1.0, 1, 1], q),
                              ("overlap_capsule", pa.SHAPE_CAPSULE, [0.5, 1, 0], q)):
        ms, (off, ids) = time_host(lambda: w.overlap(st, qp, rot, he, cap=1 << 26), args)
        out[name] = dict(summary(ms, n), ids_per_query=float(off[-1]) / n)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c2,c3,c5,t1m_settled")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    for key in args.scenes.split(","):
        r = bench_scene(key, args)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
