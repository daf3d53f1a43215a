"""k_halo_pairs<false> (the sorted-grid instance of phys_halo_pairs) on a C4-shaped world fed a neighbour slab's records.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/halo_pairs_bench.py [--calls 30]
                                                                       [--side 48] [--gids local-low|local-high]
    python tools/halo_pairs_bench.py --stats <dir>      # mean / min / max of the kernel's dispatches, us

Two worlds on one GPU play two ranks of the C4 lattice (spacing 2.2, jitter 0.3, unit cubes, broad phase only) cut at
x = 0: the local rank holds side^3 bodies in x < 0 (48^3 = 110 592: above the slot grid's limit), the neighbour the four
lattice layers behind the cut. Both run one broad phase, the neighbour packs its records with the reach both agree on
(a device buffer stands in for the all-gather), and the local rank runs `calls` asynchronous phys_halo_pairs on them.
--gids local-low (default) gives the local rank the smaller global ids, so it emits every cross pair and the timed kernel
runs its sweep, its candidate tests AND its wave appends; local-high leaves the emitting to the neighbour. The kernel's
time is the kernel trace's (the script itself times nothing); compare two builds by alternating runs."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {directory}")
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
          for f in files for r in csv.DictReader(open(f)) if "k_halo_pairs" in r["Kernel_Name"]]
    if not us:
        sys.exit("no dispatch of k_halo_pairs in the trace")
    us = us[len(us) // 6:]  # the first calls warm the caches
    print(f"k_halo_pairs: {len(us)} dispatches, mean {np.mean(us):.2f} us, min {min(us):.2f}, max {max(us):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--gids", choices=("local-low", "local-high"), default="local-low")
    ap.add_argument("--stats", metavar="DIR")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)

    import torch
    import physics_amd as pa
    from physics_amd import scenes

    s, layers = args.side, 4
    local = scenes.c4(s, s, s, x0=-1.1 * s)      # centres from -2.2 s + 1.1 to -1.1
    remote = scenes.c4(layers, s, s, x0=1.1 * layers)
    assert local.pos[:, 0].max() < 0.0 <= remote.pos[:, 0].min()
    gids = [np.arange(local.n, dtype=np.uint32), np.arange(remote.n, dtype=np.uint32)]
    gids[1 if args.gids == "local-low" else 0] += np.uint32(max(local.n, remote.n))
    worlds = []
    for sc, gid in zip((local, remote), gids):
        w = pa.World(pa.default_config(flags=sc.flags, gravity_offset=(0, 0, 0)))
        w.set_bodies(sc.pos, shape_type=sc.shape_type, half_extent=sc.half_extent)
        w.set_global_ids(gid)
        w.broadphase()
        worlds.append(w)
    reach = 1.001 * max(w.get_stats().max_extent for w in worlds)
    cap = remote.n
    buf = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_records = worlds[1].halo_pack(0.0, 1.0e30, reach, buf.data_ptr(), cap)
    w = worlds[0]
    for _ in range(args.calls):
        w.halo_pairs(buf.data_ptr(), cap, wait=False)
    w.sync()
    print(f"local bodies {local.n}, records {n_records} of {cap} slots, cross pairs per call {w.get_stats().n_cross_pairs} "
          f"({args.gids}), calls {args.calls}")
    for w in worlds:
        w.close()


if __name__ == "__main__":
    main()
