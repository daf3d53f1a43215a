"""Move-and-slide throughput (phys_move_and_slide_device) on the benchmark scenes, beside the same moves done the way a caller
had to do them before: four phys_capsulecast_device calls with torch arithmetic between them.

    python tools/slide_bench.py [--scenes c2,c3] [--queries 1000000] [--warmup 3] [--calls 10] [--reps 5] [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (tools/raycast_bench.py's preroll), then 1M upright characters
(R 0.25, h 0.5, skin 0.02, max_slides 4) start above and around the pile with motions of 4 to 10 aimed into it, so that most of
them hit. Both ways run in the same process on the world's stream and are timed with device events (tools/query_bench.py's
time_device), grid builds included: one grid for the one launch, four for the loop. The loop states the rule of
include/spec/slide.h in torch (masked, every character cast in every round); its answers are compared with the one launch's
(the share of equal statuses and the largest difference of the end positions: torch rounds its norms and sums in its own order,
so near ties may fall the other way). No ratio is fixed in advance: the figures go into DESIGN.md section 25."""
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

RADIUS, HALF_LENGTH, SKIN, MAX_SLIDES = 0.25, 0.5, 0.02, 4
MISS = -2  # PHYS_RAY_MISS as int32


def make_characters(rng, n, lo, hi):
    """starts in a slab above the pile and a margin around it, motions of 4 .. 10 towards points inside the pile"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    start = rng.uniform([lo[0] - 3.0, hi[1] + 1.0, lo[2] - 3.0], [hi[0] + 3.0, hi[1] + 4.0, hi[2] + 3.0], (n, 3))
    aim = rng.uniform(lo, hi, (n, 3))
    d = aim - start
    motion = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4.0, 10.0, (n, 1))
    return start.astype(np.float32), motion.astype(np.float32)


def bench_scene(key, args):
    import torch
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    rng = np.random.default_rng(0)
    n = args.queries
    start, motion = make_characters(rng, n, pos.min(0), pos.max(0))
    dev = torch.device("cuda", 0)
    tp, tm = torch.from_numpy(start).to(dev), torch.from_numpy(motion).to(dev)
    tr = torch.full((n,), RADIUS, dtype=torch.float32, device=dev)
    th = torch.full((n,), HALF_LENGTH, dtype=torch.float32, device=dev)
    out_pos, out_rem = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(2))
    out_status = torch.empty(n, dtype=torch.int32, device=dev)
    out_body = torch.empty((MAX_SLIDES, n), dtype=torch.int32, device=dev)
    out_nrm, out_pnt = (torch.empty((MAX_SLIDES, n, 3), dtype=torch.float32, device=dev) for _ in range(2))
    tb = torch.empty(n, dtype=torch.int32, device=dev)
    tt = torch.empty(n, dtype=torch.float32, device=dev)
    tn, tq = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(2))
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    loop = {}

    def one_launch():
        w.move_and_slide_device(tp, tm, tr, th, out_pos, out_status, out_rem, out_body, out_nrm, out_pnt, skin=SKIN, max_slides=MAX_SLIDES)

    def cast_loop():
        with torch.cuda.stream(stream):
            p, m = tp.clone(), tm.clone()
            n_prev = torch.zeros_like(p)
            have_prev = torch.zeros(n, dtype=torch.bool, device=dev)
            active = torch.ones(n, dtype=torch.bool, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            for _ in range(MAX_SLIDES):
                L = torch.sqrt((m * m).sum(1))
                max_t = L + SKIN
                w.capsulecast_device(p, m, tr, th, tb, tt, tn, tq, max_t=max_t)  # a zero motion misses
                hit = active & (tb != MISS)
                miss = active & ~hit
                p = torch.where(miss[:, None], p + m, p)
                blocked = hit & (tt == 0)
                go = hit & ~blocked
                status = status + hit.int() + blocked.int() * 0x100
                u = m / L.clamp_min(1e-30)[:, None]
                a = torch.minimum((tt - SKIN).clamp_min(0.0), L)
                p = torch.where(go[:, None], p + u * a[:, None], p)
                r = u * (L - a)[:, None]
                s = r - tn * (r * tn).sum(1, keepdim=True)
                c = torch.linalg.cross(n_prev, tn)
                cc = (c * c).sum(1)
                on_line = torch.where((cc > 1e-12)[:, None], c * ((r * c).sum(1) / cc.clamp_min(1e-30))[:, None], torch.zeros_like(c))
                s = torch.where((have_prev & ((s * n_prev).sum(1) < 0))[:, None], on_line, s)
                s = torch.where(((s * tm).sum(1) > 0)[:, None], s, torch.zeros_like(s))
                n_prev = torch.where(go[:, None], tn, n_prev)
                have_prev = have_prev | go
                m = torch.where(go[:, None], s, torch.where(miss[:, None], torch.zeros_like(m), m))
                active = go
            status = status + (active & (m != 0).any(1)).int() * 0x200
            loop["pos"], loop["status"] = p, status

    torch.cuda.synchronize()
    ms_one = time_device(w, stream, one_launch, args)
    ms_loop = time_device(w, stream, cast_loop, args)
    w.sync()
    status = out_status.cpu().numpy().view(np.uint32)
    hits = np.bincount(status & 0xF, minlength=MAX_SLIDES + 1)
    same = float((loop["status"].cpu().numpy().view(np.uint32) == status).mean())
    agree = loop["status"].cpu().numpy().view(np.uint32) == status
    apart = float(np.abs(loop["pos"].cpu().numpy() - out_pos.cpu().numpy())[agree].max())
    one, four = summary(ms_one, n), summary(ms_loop, n)
    out = {"scene": key, "bodies": int(sc.n), "characters": n, "one_launch": one, "four_cast_loop": four,
           "loop_over_launch": four["median_ms"] / one["median_ms"], "hit_counts": hits.tolist(),
           "blocked": int((status & 0x100 != 0).sum()), "exhausted": int((status & 0x200 != 0).sum()),
           "loop_same_status": same, "loop_pos_max_abs_diff_where_same": apart}
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
    results = []
    for key in args.scenes.split(","):
        r = bench_scene(key, args)
        results.append(r)
        print(json.dumps(r), flush=True)
        print(f"{key}: one launch {r['one_launch']['median_ms']:.2f} ms | four-cast loop {r['four_cast_loop']['median_ms']:.2f} ms | "
              f"loop / launch {r['loop_over_launch']:.2f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
