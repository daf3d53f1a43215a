"""Cost of contact events on C5, the benchmark's 256k-box tower, and C3, the 100k mixed pile.

    python tools/events_bench.py [--scenes c5,c3] [--steps 200] [--warmup 60] [--reps 3] [--capacity 1048576] [--json out.json]

Two variants of each scene - events off, events on with `capacity` - each repetition a FRESH world stepped `warmup`
updates and then timed over `steps` updates on the wall clock (the timing of bench.py), `reps` times; the last world of a
variant then runs 20 profiled updates for the device time of PHYS_STAGE_MISC (where the two event kernels are timed; the
rest of that stage is the memsets every world has). The events are drained after the warm-up and after the timed window.
Reported per variant: steps/s (median and every repetition), misc ms and launches per update, events per update of the
timed window and of the profiled updates, dropped events, and - from the profiled updates - the compulsory bytes of the
two kernels per update (32 M + 4 M' + 112 B + 8 X read, 4 (M - B) + 48 (B + X) written) and the bytes/s they amount to
over the misc time the variant adds to events off."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = 16_666_667
PROFILED = 20


def run_variant(scene, events_on, args):
    import physics_amd as pa
    from physics_amd import scenes
    rates, per_update, dropped_all = [], [], 0
    for rep in range(args.reps):
        sc = getattr(scenes, scene)()
        w = pa.World(sc.config())
        sc.populate(w)
        if events_on:
            w.enable_contact_events(args.capacity)
        w.update_n(DT, args.warmup)
        w.sync()
        if events_on:
            w.get_contact_events()
        t0 = time.perf_counter()
        w.update_n(DT, args.steps)
        w.sync()
        rates.append(args.steps / (time.perf_counter() - t0))
        if events_on:
            ev, dropped = w.get_contact_events()
            per_update.append((len(ev) + dropped) / args.steps)
            dropped_all += dropped
        if rep + 1 < args.reps:
            w.close()
    w.profile_enable(True)
    m_prev = int(w.get_stats().n_manifolds)
    w.update_n(DT, PROFILED)
    w.sync()
    prof, steps = w.profile_get()
    w.profile_enable(False)
    st = w.get_stats()
    out = {"scene": scene, "events": bool(events_on), "bodies": sc.n, "steps_per_s": statistics.median(rates), "steps_per_s_all": rates,
           "misc_ms": prof.get("misc", (0.0, 0))[0] / steps, "misc_launches": prof.get("misc", (0.0, 0))[1] / steps,
           "manifolds": int(st.n_manifolds)}
    if events_on:
        ev, dropped = w.get_contact_events()
        b = int((ev["kind"] == pa.CONTACT_BEGIN).sum()) / steps
        x = int((ev["kind"] == pa.CONTACT_END).sum()) / steps
        m = (m_prev + int(st.n_manifolds)) / 2.0  # the count barely moves over 20 updates of a settled scene
        out.update({"events_per_update": statistics.median(per_update), "dropped": int(dropped_all + dropped),
                    "profiled_begins_per_update": b, "profiled_ends_per_update": x,
                    "compulsory_read_bytes": 32 * m + 4 * m + 112 * b + 8 * x, "compulsory_write_bytes": 4 * (m - b) + 48 * (b + x)})
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="c5,c3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    for scene in args.scenes.split(","):
        off = run_variant(scene, False, args)
        on = run_variant(scene, True, args)
        added_ms = on["misc_ms"] - off["misc_ms"]
        on["added_misc_ms"] = added_ms
        on["added_share_of_update"] = added_ms / (1000.0 / off["steps_per_s"])
        if added_ms > 0:
            on["achieved_bytes_per_s"] = (on["compulsory_read_bytes"] + on["compulsory_write_bytes"]) / (added_ms * 1e-3)
        for r in (off, on):
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
