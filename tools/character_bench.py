"""Character walking throughput (phys_character_move_device) on the benchmark scenes with a static staircase and two ramps
added, beside the same walk composed on the device the way a caller had to before: two phys_move_and_slide_device calls, three
phys_capsulecast_device calls and torch between them.

    python tools/character_bench.py [--scenes c2,c3] [--queries 1000000] [--warmup 3] [--calls 10] [--reps 5] [--json out.json]

Per scene: the scene is stepped to the state bench.py measures (tools/raycast_bench.py's preroll); a staircase (risers of 0.2), a
ramp of 30 and one of 60 degrees are set as statics beside the pile; 1M upright characters (R 0.25, h 0.5, skin 0.02,
max_slides 4, step_height 0.3, snap_distance 0.2, the slope limit at 45 degrees) stand skin above the ground around the pile and
in front of the stairs and ramps and on the stairs' treads (walking 0.3 to 1.5) or in a frame around the pile (walking 1 to 4
into it), nine in ten of them grounded_in, all with a little gravity. Both ways run in the same process on the world's stream and are timed with device events (tools/query_bench.py's
time_device), grid builds included: one grid for the one launch, five for the composition. What the composition needs of its
inputs alone (who walks, the horizontal motions, the constant lengths) is made once outside the timed calls. Three things still
weigh against the composition, and any ratio read off this tool carries them: it casts every character in every call (masked
afterwards), its torch operations between the calls allocate their results from torch's caching allocator, and it leaves out
the no-climb rule, which has no place between two library calls, so its answers are not the launch's everywhere; the share of
equal flags is reported. No ratio is fixed in advance: the figures go into DESIGN.md section 28."""
import argparse
import json
import math
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
STEP_HEIGHT, SNAP_DISTANCE, MIN_FLOOR_NY = 0.3, 0.2, math.cos(math.radians(45.0))
MISS = -2  # PHYS_RAY_MISS as int32
GROUNDED, STEPPED, SNAPPED, ON_STEEP, HIT_WALL = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000


def terrain(x0, z0):
    """(pos, rot, half extent) of six static boxes: four stairs of 0.2 rising towards +x from x0, then two ramps beside them"""
    pos, rot, he = [], [], []
    for k in range(4):
        lo, hi = np.array([x0 + 0.6 * k, -1.0, z0 - 10.0 - 0.05 * k]), np.array([x0 + 8.0 + 0.1 * k, 0.2 * (k + 1), z0 + 10.0 + 0.05 * k])
        pos.append((lo + hi) / 2); rot.append([0.0, 0.0, 0.0, 1.0]); he.append((hi - lo) / 2)
    for deg, z in ((30.0, z0 + 25.0), (60.0, z0 - 25.0)):
        a = math.radians(deg)
        c, s = math.cos(a), math.sin(a)
        corner = (-4.0 * c - 0.5 * s, -4.0 * s + 0.5 * c)  # the turned box's upper edge on the ground line x = x0
        pos.append([x0 - corner[0], -corner[1], z]); rot.append([0.0, 0.0, math.sin(a / 2), math.cos(a / 2)]); he.append([4.0, 0.5, 10.0])
    return np.array(pos, np.float32), np.array(rot, np.float32), np.array(he, np.float32)


def make_characters(rng, n, lo, hi, x0, z0):
    """a third in a frame 1.5 to 4 around the pile's box of centres walking at it, a third in front of the stairs and ramps
    walking at them, a third on the treads, clear of the next riser"""
    stand = RADIUS + HALF_LENGTH + SKIN
    kind = rng.integers(0, 3, n)
    # the frame: a point of the box's outline pushed outwards
    side, out = rng.integers(0, 4, n), rng.uniform(1.5, 4.0, n)
    along_x, along_z = rng.uniform(lo[0] - 1.5, hi[0] + 1.5, n), rng.uniform(lo[2] - 1.5, hi[2] + 1.5, n)
    fx = np.where(side == 0, lo[0] - out, np.where(side == 1, hi[0] + out, along_x))
    fz = np.where(side == 2, lo[2] - out, np.where(side == 3, hi[2] + out, along_z))
    x = np.where(kind == 0, fx, np.where(kind == 1, rng.uniform(x0 - 1.5, x0 - 0.4, n), 0.0))
    z = np.where(kind == 0, fz, rng.uniform(z0 - 34.0, z0 + 34.0, n))
    tread = rng.integers(0, 4, n)
    on = kind == 2
    x = np.where(on, x0 + 0.6 * tread + np.where(tread == 3, rng.uniform(0.05, 3.0, n), rng.uniform(0.05, 0.3, n)), x)
    z = np.where(on, rng.uniform(z0 - 9.0, z0 + 9.0, n), z)
    y = stand + np.where(on, 0.2 * (tread + 1), 0.0)
    towards = np.arctan2(0.5 * (lo[2] + hi[2]) - fz, 0.5 * (lo[0] + hi[0]) - fx) + np.radians(rng.uniform(-40.0, 40.0, n))
    ang = np.where(kind == 0, towards, np.radians(rng.uniform(-50.0, 50.0, n)) + np.where(rng.random(n) < 0.7, 0.0, math.pi))
    length = np.where(kind == 0, rng.uniform(1.0, 4.0, n), rng.uniform(0.3, 1.5, n))
    motion = np.stack([length * np.cos(ang), np.full(n, -0.05), length * np.sin(ang)], axis=1)
    grounded = (rng.random(n) < 0.9).astype(np.int32)
    return np.stack([x, y, z], axis=1).astype(np.float32), motion.astype(np.float32), grounded


def bench_scene(key, args):
    import torch
    sc, w = settled_world(key)
    pos, _ = w.get_transforms()
    lo, hi = pos.min(0), pos.max(0)
    x0, z0 = float(hi[0]) + 6.0, float(0.5 * (lo[2] + hi[2]))
    st_pos, st_rot, st_he = terrain(x0, z0)
    w.set_static_bodies(st_pos, rot=st_rot, shape_type=np.full(len(st_pos), 2, np.uint32), half_extent=st_he)
    rng = np.random.default_rng(0)
    n = args.queries
    start, motion, grounded = make_characters(rng, n, lo, hi, x0, z0)
    dev = torch.device("cuda", 0)
    tp, tm, tg = torch.from_numpy(start).to(dev), torch.from_numpy(motion).to(dev), torch.from_numpy(grounded).to(dev)
    tr = torch.full((n,), RADIUS, dtype=torch.float32, device=dev)
    th = torch.full((n,), HALF_LENGTH, dtype=torch.float32, device=dev)
    f3 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i1 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out_pos, out_rem, out_status = f3(n, 3), f3(n, 3), i1(n)
    out_fb, out_fn, out_fp = i1(n), f3(n, 3), f3(n, 3)
    out_body, out_nrm, out_pnt = i1(2 * MAX_SLIDES, n), f3(2 * MAX_SLIDES, n, 3), f3(2 * MAX_SLIDES, n, 3)
    # the composition's own buffers
    p1, r1, s1, b1, n1 = f3(n, 3), f3(n, 3), i1(n), i1(MAX_SLIDES, n), f3(MAX_SLIDES, n, 3)
    p2, r2, s2 = f3(n, 3), f3(n, 3), i1(n)
    cb, ct, cn = i1(n), f3(n), f3(n, 3)
    up = torch.tensor([0.0, 1.0, 0.0], device=dev).expand(n, 3).contiguous()
    down = -up
    stream = torch.cuda.ExternalStream(w.device_view().stream, device=dev)
    loop = {}

    # what the composition needs of its inputs alone is made once, outside the timed calls
    walking = (tg != 0) & ~(tm[:, 1] > 0)
    l = tm.clone()
    l[:, 1] = 0.0
    has_l = (l != 0).any(1)
    up_max_t = torch.full((n,), STEP_HEIGHT + SKIN, dtype=torch.float32, device=dev)
    full_lift = torch.full((n,), STEP_HEIGHT, dtype=torch.float32, device=dev)
    reach = 2 * SKIN + torch.where(walking, torch.full_like(full_lift, SNAP_DISTANCE), torch.zeros_like(full_lift))

    def one_launch():
        with torch.cuda.stream(stream):
            w.character_move_device(tp, tm, tr, th, out_pos, out_status, out_rem, out_fb, out_fn, out_fp, out_body, out_nrm, out_pnt, grounded=tg,
                                    skin=SKIN, max_slides=MAX_SLIDES, step_height=STEP_HEIGHT, snap_distance=SNAP_DISTANCE,
                                    min_floor_ny=MIN_FLOOR_NY)

    def composed():
        with torch.cuda.stream(stream):
            w.move_and_slide_device(tp, tm, tr, th, p1, s1, r1, b1, n1, skin=SKIN, max_slides=MAX_SLIDES)
            blocked = (s1 & 0x100) != 0
            wall = ((b1 != MISS) & (n1[:, :, 1] < MIN_FLOOR_NY)).any(0)
            try_step = walking & wall & ~blocked & has_l
            w.capsulecast_device(tp, up, tr, th, cb, ct, cn, max_t=up_max_t)
            lift = torch.where(cb == MISS, full_lift, (ct - SKIN).clamp(0.0, STEP_HEIGHT))
            try_step = try_step & ~((cb != MISS) & (ct == 0)) & (lift > 0)
            lifted = tp + up * lift[:, None]
            w.move_and_slide_device(lifted, l, tr, th, p2, s2, r2, skin=SKIN, max_slides=MAX_SLIDES)
            try_step = try_step & ((s2 & 0x100) == 0)
            w.capsulecast_device(p2, down, tr, th, cb, ct, cn, max_t=lift + 2 * SKIN)
            further = ((p2 - tp) * l).sum(1) > ((p1 - tp) * l).sum(1)
            stepped = try_step & (cb != MISS) & (ct > 0) & (cn[:, 1] >= MIN_FLOOR_NY) & further
            landed = p2 - up * (ct - SKIN).clamp_min(0.0)[:, None]
            p = torch.where(stepped[:, None], landed, p1)
            w.capsulecast_device(p, down, tr, th, cb, ct, cn, max_t=reach)
            probe = ~stepped & ~blocked & (cb != MISS) & (ct > 0)
            floor = probe & (cn[:, 1] >= MIN_FLOOR_NY)
            snapped = floor & walking & (ct > 2 * SKIN)
            p = torch.where(snapped[:, None], p - up * (ct - SKIN)[:, None], p)
            steep = probe & ~floor & (cn[:, 1] > 0)
            loop["pos"] = p
            loop["flags"] = (stepped | floor).int() * GROUNDED + stepped.int() * STEPPED + snapped.int() * SNAPPED + steep.int() * ON_STEEP

    torch.cuda.synchronize()
    ms_one = time_device(w, stream, one_launch, args)
    ms_loop = time_device(w, stream, composed, args)
    w.sync()
    status = out_status.cpu().numpy().view(np.uint32)
    flags = GROUNDED | STEPPED | SNAPPED | ON_STEEP
    same = (loop["flags"].cpu().numpy().view(np.uint32) == (status & flags))
    one, five = summary(ms_one, n), summary(ms_loop, n)
    count = lambda bit: int((status & bit != 0).sum())
    out = {"scene": key, "bodies": int(sc.n), "characters": n, "one_launch": one, "composed": five,
           "composed_over_launch": five["median_ms"] / one["median_ms"], "grounded": count(GROUNDED), "stepped": count(STEPPED),
           "snapped": count(SNAPPED), "on_steep": count(ON_STEEP), "hit_wall": count(HIT_WALL), "blocked": count(0x100),
           "move_hits": np.bincount(status & 0xF, minlength=MAX_SLIDES + 1).tolist(), "composed_same_flags": float(same.mean()),
           "composed_pos_max_abs_diff_where_same": float(np.abs(loop["pos"].cpu().numpy() - out_pos.cpu().numpy())[same].max())}
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
        print(f"{key}: one launch {r['one_launch']['median_ms']:.2f} ms | composed {r['composed']['median_ms']:.2f} ms | "
              f"composed / launch {r['composed_over_launch']:.2f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
