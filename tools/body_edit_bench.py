"""Cost of the in-place body edits.

    python tools/body_edit_bench.py [--parts forces,rate,step] [--reps 5] [--calls 20] [--device-calls 2000] [--parent DIR]
                                    [--json out.json]

Three measurements, each a host clock around work that ends in phys_sync, after one untimed pass over the same shapes:

    forces  one phys_apply_forces of 10 000 entries (a point each) against 10 000 phys_apply_force_at_position calls, on 10 000
            bodies: milliseconds per 10 000 forces, median / min / max of `reps`, and the ratio of the medians.
    rate    entries per second of the host and the device variant of each edit call and of the read-back, at 1 000 and 100 000
            entries on the 1M-cube scene (scenes.target_1m as uploaded; an edit's cost does not depend on the pile's state): `calls`
            calls (device variant: `device-calls`, so that its window is milliseconds too) back to back and one phys_sync per
            window, ids drawn over the whole scene with repeats (the device variant's sorted once, outside the window, as a
            caller's nonzero() would be). The device rows measure the rate of enqueued launches, not the kernels.
    step    the plain benchmark, `python bench.py --gpus 1 --steps 20 --warmup 5`, in a process of its own: its result line. With
            --parent DIR (a built checkout of the parent commit) the same command runs there too, the two alternating `reps`
            times, and the medians of the step times are printed side by side: the edits add nothing to an update, so they are
            expected to agree within the spread.

One JSON line per measurement."""
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


def _window(fn, sync, reps):
    """Milliseconds of fn() + sync(), `reps` times after one untimed pass."""
    fn()
    sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def bench_forces(args):
    import physics_amd as pa
    n = 10_000
    rng = np.random.default_rng(0)
    w = pa.World(pa.default_config())
    w.set_bodies(rng.uniform(-50, 50, (n, 3)).astype(np.float32))
    ids = rng.permutation(n).astype(np.uint32)
    f = rng.normal(size=(n, 3)).astype(np.float32)
    p = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    zero = np.zeros((n, 3), np.float32)

    def single():
        for k in range(n):
            w.apply_force_at_position(int(ids[k]), f[k], p[k])

    w.set_forces(zero, zero)
    batch = _window(lambda: w.apply_forces(ids, f, point=p), w.sync, args.reps)
    w.set_forces(zero, zero)
    w.apply_forces(ids, f, point=p)
    one = w.get_forces()
    w.set_forces(zero, zero)
    calls = _window(single, w.sync, args.reps)
    w.set_forces(zero, zero)
    single()
    same = all(a.tobytes() == b.tobytes() for a, b in zip(one, w.get_forces()))
    w.close()
    return {"part": "forces", "entries": n, "batch": _stats(batch), "single_calls": _stats(calls),
            "ratio_of_medians": statistics.median(calls) / statistics.median(batch), "same_bits": same}


def bench_rate(args):
    import torch
    import physics_amd as pa
    from physics_amd import scenes
    sc = scenes.SCENES["t1m"]()
    w = pa.World(sc.config())
    sc.populate(w)
    n = sc.n
    out = []
    for m in (1_000, 100_000):
        rng = np.random.default_rng(m)
        ids = rng.integers(0, n, m).astype(np.uint32)
        a = rng.normal(size=(m, 3)).astype(np.float32) * np.float32(1e-3)
        pos, rot, lin, ang = w.get_body_states(ids)
        order = np.argsort(ids, kind="stable")
        dev = torch.device("cuda", 0)
        t = {k: torch.from_numpy(np.ascontiguousarray(v[order])).to(dev) for k, v in dict(a=a, pos=pos, rot=rot, lin=lin, ang=ang).items()}
        tid = torch.from_numpy(ids[order].astype(np.int32)).to(dev)
        outs = [torch.empty((m, c), dtype=torch.float32, device=dev) for c in (3, 4, 3, 3)]
        torch.cuda.synchronize()
        # every call writes back what is there or adds next to nothing: the scene stays the scene
        host = {"set_body_poses": lambda: w.set_body_poses(ids, pos=pos, rot=rot),
                "set_body_velocities": lambda: w.set_body_velocities(ids, lin=lin, ang=ang),
                "apply_impulses": lambda: w.apply_impulses(ids, a, point=pos),
                "apply_forces": lambda: w.apply_forces(ids, a, point=pos),
                "get_body_states": lambda: w.get_body_states(ids)}
        device = {"set_body_poses": lambda: w.set_body_poses_device(tid, pos=t["pos"], rot=t["rot"]),
                  "set_body_velocities": lambda: w.set_body_velocities_device(tid, lin=t["lin"], ang=t["ang"]),
                  "apply_impulses": lambda: w.apply_impulses_device(tid, t["a"], point=t["pos"]),
                  "apply_forces": lambda: w.apply_forces_device(tid, t["a"], point=t["pos"]),
                  "get_body_states": lambda: w.get_body_states_device(tid, *outs)}
        for variant, table in (("host", host), ("device", device)):
            for call, fn in table.items():
                calls = args.calls if variant == "host" else args.device_calls

                def many(fn=fn, calls=calls):
                    for _ in range(calls):
                        fn()
                ms = _window(many, w.sync, args.reps)
                med = statistics.median(ms) / calls
                out.append({"part": "rate", "bodies": n, "entries": m, "variant": variant, "call": call, "calls": calls, "ms_per_call": med,
                            "ms_per_call_min": min(ms) / calls, "ms_per_call_max": max(ms) / calls,
                            "entries_per_s": m / (med * 1e-3)})
                print(json.dumps(out[-1]), flush=True)
        w.set_forces(np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32))
    w.close()
    return out


def _bench_py(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed (exit {r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _step_ms(line):
    """The step time of a bench.py result line in milliseconds."""
    return float(line["ms_per_step"])


def bench_step(args):
    if not args.parent:
        line = _bench_py(ROOT)
        return {"part": "step", "this": line, "this_ms": _step_ms(line)}
    mine, theirs = [], []
    for _ in range(args.reps):  # alternating: other people's work shares the machine
        theirs.append(_bench_py(os.path.abspath(args.parent)))
        mine.append(_bench_py(ROOT))
    a, b = [_step_ms(x) for x in mine], [_step_ms(x) for x in theirs]
    return {"part": "step", "this": mine[-1], "parent": theirs[-1], "this_ms_all": a, "parent_ms_all": b, "this_ms": statistics.median(a),
            "parent_ms": statistics.median(b), "ratio": statistics.median(a) / statistics.median(b)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parts", default="forces,rate,step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window of the rate part")
    ap.add_argument("--device-calls", type=int, default=2000, help="calls per timed window of the rate part's device variant")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the step part")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    for part in args.parts.split(","):
        if part == "forces":
            results.append(bench_forces(args))
            print(json.dumps(results[-1]), flush=True)
        elif part == "rate":
            results += bench_rate(args)
        elif part == "step":
            results.append(bench_step(args))
            print(json.dumps(results[-1]), flush=True)
        else:
            raise SystemExit(f"unknown part {part}: forces, rate or step")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
