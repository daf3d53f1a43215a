"""Depenetration throughput (phys_depenetrate_device) on the benchmark scenes, beside the same work done with the probe alone:
max_iters + 1 phys_penetration_device calls with the rule of include/spec/depenetrate.h in torch between them.

    python tools/depen_bench.py [--scenes c2,c3] [--queries 1000000] [--warmup 3] [--calls 10] [--reps 5] [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (tools/raycast_bench.py's preroll), then 1M upright characters
(R 0.25, h 0.5, skin 0.02, max_iters 4) are dropped INTO the settled pile: uniformly over its bounding box, so that most overlap a
body or the ground. Both ways run in the same process on the world's stream and are timed with device events
(tools/query_bench.py's time_device), grid builds included: one grid for the one launch, five for the loop. The loop's torch
arithmetic is the rule's own (one multiply and one add per component, nothing fused), so its statuses and positions must equal
the one launch's query for query: the tool counts the differences and fails on any. No ratio is fixed in advance: the figures go
into DESIGN.md section 27."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from query_bench import summary, time_device  # noqa: E402
from raycast_bench import settled_world  # noqa: E402

RADIUS, HALF_LENGTH, SKIN, MAX_ITERS = 0.25, 0.5, 0.02, 4
MISS = -2  # PHYS_RAY_MISS as int32
STUCK = 0x100


def bench_scene(key, args):
    import torch
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    rng = np.random.default_rng(0)
    n = args.queries
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    start = rng.uniform([lo[0] - 1.0, 0.0, lo[2] - 1.0], [hi[0] + 1.0, hi[1] + 1.0, hi[2] + 1.0], (n, 3)).astype(np.float32)
    dev = torch.device("cuda", 0)
    tp = torch.from_numpy(start).to(dev)
    tr = torch.full((n,), RADIUS, dtype=torch.float32, device=dev)
    th = torch.full((n,), HALF_LENGTH, dtype=torch.float32, device=dev)
    out_pos = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_status = torch.empty(n, dtype=torch.int32, device=dev)
    out_body = torch.empty((MAX_ITERS, n), dtype=torch.int32, device=dev)
    out_nrm = torch.empty((MAX_ITERS, n, 3), dtype=torch.float32, device=dev)
    out_dep = torch.empty((MAX_ITERS, n), dtype=torch.float32, device=dev)
    tb = torch.empty(n, dtype=torch.int32, device=dev)
    td = torch.empty(n, dtype=torch.float32, device=dev)
    tn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    loop = {}

    def one_launch():
        w.depenetrate_device(tp, tr, th, out_pos, out_status, out_body, out_nrm, out_dep, skin=SKIN, max_iters=MAX_ITERS)

    def probe_loop():
        with torch.cuda.stream(stream):
            p = tp.clone()
            active = torch.ones(n, dtype=torch.bool, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            half = torch.tensor(-0.5, dtype=torch.float32, device=dev) * torch.tensor(SKIN, dtype=torch.float32, device=dev)
            for k in range(MAX_ITERS + 1):
                w.penetration_device(p, tr, th, tb, td, tn, max_gap=SKIN)  # every character probed in every round
                near = active & (tb != MISS) & (td > half)
                if k == MAX_ITERS:
                    status = status + near.int() * STUCK
                    break
                status = status + near.int()
                p = torch.where(near[:, None], p + tn * (td + SKIN)[:, None], p)
                active = near
            loop["pos"], loop["status"] = p, status

    torch.cuda.synchronize()
    ms_one = time_device(w, stream, one_launch, args)
    ms_loop = time_device(w, stream, probe_loop, args)
    w.sync()
    status = out_status.cpu().numpy().view(np.uint32)
    loop_status = loop["status"].cpu().numpy().view(np.uint32)
    pushes = np.bincount(status & 0xF, minlength=MAX_ITERS + 1)
    status_differ = int((loop_status != status).sum())
    pos_differ = int((loop["pos"].cpu().numpy().view(np.uint32) != out_pos.cpu().numpy().view(np.uint32)).any(1).sum())
    one, many = summary(ms_one, n), summary(ms_loop, n)
    out = {"scene": key, "bodies": int(sc.n), "characters": n, "one_launch": one, "probe_loop": many,
           "loop_over_launch": many["median_ms"] / one["median_ms"], "push_counts": pushes.tolist(),
           "stuck": int((status & STUCK != 0).sum()), "loop_status_differ": status_differ, "loop_pos_differ": pos_differ}
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c2,c3")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results, bad = [], 0
    for key in args.scenes.split(","):
        r = bench_scene(key, args)
        results.append(r)
        bad += r["loop_status_differ"]
        print(json.dumps(r), flush=True)
        print(f"{key}: one launch {r['one_launch']['median_ms']:.2f} ms | probe loop {r['probe_loop']['median_ms']:.2f} ms | "
              f"loop / launch {r['loop_over_launch']:.2f} | statuses that differ {r['loop_status_differ']}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    if bad:
        sys.exit(f"{bad} statuses of the probe loop differ from the one launch's")


if __name__ == "__main__":
    main()
