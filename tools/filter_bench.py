"""Cost of collision filters on C5, the benchmark's 256k-box tower.

    python tools/filter_bench.py [--steps 200] [--warmup 60] [--rays 1000000] [--reps 3] [--json out.json]

Three variants of C5, each a fresh world stepped `warmup` updates and then timed over `steps` updates on the wall clock
(the timing of bench.py), followed by 10 profiled updates for the narrow phase's device time:
  - plain: no filter ever set (the unfiltered narrow phase);
  - defaults: the default filters set explicitly on bodies and ground, which runs the filtered narrow phase;
  - debris: half the bodies, in a checkerboard, are debris (category 2, mask without 2) that ignores itself.
Reported per variant: steps/s, PHYS_STAGE_NARROW ms per update, candidate pairs and manifolds of the last update.
Then 1M ray casts (tools/raycast_bench.py's rays) against the defaults world, plain against masked (mask 0xFFFF: the same
answers through the filtered kernel), timed with device events on the world's stream."""
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

from raycast_bench import make_rays  # noqa: E402

DT = 16_666_667


def run_variant(name, args):
    import physics_amd as pa
    from physics_amd import scenes
    sc = scenes.c5()
    w = pa.World(sc.config())
    sc.populate(w)
    n = sc.n
    if name == "defaults":
        w.set_body_filters(np.full(n, pa.FILTER_DEFAULT_CATEGORY), np.full(n, pa.FILTER_DEFAULT_MASK), np.zeros(n, np.int16))
        w.set_ground_filter(pa.FILTER_DEFAULT_CATEGORY, pa.FILTER_DEFAULT_MASK)
    elif name == "debris":
        # a 3-D checkerboard of the lattice (ids run x fastest, then z, then y): the tower keeps standing, and the pairs
        # between two debris boxes (edges and corners of the checkerboard) are rejected
        i = np.arange(n)
        debris = ((i % 16) + (i // 16 % 16) + (i // 256)) % 2 == 1
        w.set_body_filters(category=np.where(debris, 2, 1), mask=np.where(debris, 0xFFFD, 0xFFFF))
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
    out = {"variant": name, "bodies": n, "steps_per_s": statistics.median(rates), "steps_per_s_all": rates,
           "narrow_ms": prof["narrow"][0] / steps, "pairs": int(st.n_pairs), "manifolds": int(st.n_manifolds)}
    return out, w


def bench_rays(w, args):
    import torch
    pos, _ = w.get_transforms()
    rng = np.random.default_rng(0)
    n = args.rays
    o, d = make_rays(rng, n, pos.min(0) - 2.0, pos.max(0) + 2.0)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tm = torch.full((n,), -1, dtype=torch.int16, device=dev)  # 0xFFFF
    tb = torch.empty(n, dtype=torch.int32, device=dev)
    tt = torch.empty(n, dtype=torch.float32, device=dev)
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    torch.cuda.synchronize()
    out = {"rays": n}
    for name, fn in (("plain", lambda: w.raycast_device(to, td, tb, tt)),
                     ("masked", lambda: w.raycast_device(to, td, tb, tt, mask=tm))):
        for _ in range(3):
            fn()
        w.sync()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(10):
                fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b) / 10)
        out[f"{name}_ms"] = statistics.median(ms)
        out[f"{name}_ms_all"] = ms
        out[f"{name}_hits"] = int((tb.cpu().numpy().view(np.uint32) < w.n).sum())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    for name in ("plain", "defaults", "debris"):
        r, w = run_variant(name, args)
        if name == "defaults":
            r["raycast"] = bench_rays(w, args)
        w.close()
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
