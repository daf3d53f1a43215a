"""Box-cast throughput (phys_boxcast_device) on the benchmark scenes, beside phys_capsulecast_device.

    python tools/boxcast_bench.py [--scenes c2,c3,c5,t1m_settled] [--queries 1000000] [--warmup 2] [--calls 5] [--reps 3]
                                  [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (tools/raycast_bench.py's preroll), then 1M casts
(raycast_bench.py's rays) through the device calls, timed with device events on the world's stream, grid build included
(tools/query_bench.py's time_device): for half extents (0.25, 0.75, 0.25) and (0.5, 1.5, 0.5), the boxes axis-aligned (rot
NULL) and turned at random, and in the same process the capsule cast of comparable reach (R 0.25 h 0.5 and R 0.5 h 1.0:
the capsule inscribed in the box) beside each row. No time is fixed in advance: the figures go into DESIGN.md section 30."""
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
from raycast_bench import make_rays, settled_world  # noqa: E402


def bench_scene(key, args):
    import torch
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    lo, hi = pos.min(0), pos.max(0)
    rng = np.random.default_rng(0)
    n = args.queries
    o, d = make_rays(rng, n, lo - 2.0, hi + 2.0)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    dev = torch.device("cuda", 0)
    to, td, tq = (torch.from_numpy(x).to(dev) for x in (o, d, q))
    tb = torch.empty(n, dtype=torch.int32, device=dev)
    tt = torch.empty(n, dtype=torch.float32, device=dev)
    tn, tp = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(2))
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    out = {"scene": key, "bodies": int(sc.n), "queries": n}

    def hits():
        return int((tb.cpu().numpy().view(np.uint32) < sc.n).sum())

    for he, rad, hl in (((0.25, 0.75, 0.25), 0.25, 0.5), ((0.5, 1.5, 0.5), 0.5, 1.0)):
        the = torch.tensor(he, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
        tr = torch.full((n,), rad, dtype=torch.float32, device=dev)
        th = torch.full((n,), hl, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for name, rot in (("aligned", None), ("turned", tq)):
            ms = time_device(w, stream, lambda: w.boxcast_device(to, td, the, tb, tt, tn, tp, rot=rot), args)
            out[f"boxcast_he{he[0]}_{he[1]}_{name}"] = dict(summary(ms, n), body_hits=hits())
            ms = time_device(w, stream, lambda: w.capsulecast_device(to, td, tr, th, tb, tt, tn, tp, rot=rot), args)
            out[f"capsulecast_r{rad}_h{hl}_{name}"] = dict(summary(ms, n), body_hits=hits())
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c2,c3,c5,t1m_settled")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
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
