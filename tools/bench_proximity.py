#!/usr/bin/env python
"""Time ``instance_proximity`` on synthetic instance masks built on the device, beside the existing code that answers
pieces of the same question.

The masks are ``tools/bench_clean.py``'s: one ball per 32^3 cell (seeded centres and radii, ids a seeded permutation)
with specks and pockets, at (512, 512, 128) and at (1024, 1024, 256), 8192 balls.  The second mask of a pair is
``tools/bench_overlaps.py``'s: the first rolled by (3, 2, 1) voxels with its ids permuted.  The spacing is (1, 1, 3) and
the distances are 0, 2, 3 and 5, with two masks and with one (``b=None``).

Timed with device events after a warm-up, min / median / max over the repeats, the prologues (``id_rows``) computed
once outside the timed region:

  ``instance_proximity``  one direction; the time holds the launch, the read-back of the two counters, any retry at a
                          larger table, and the sort of the rows.  The report adds the rows found, the reach, and the
                          LDS bytes, the workgroup size and the workgroups per CU the library reports for that reach
                          (LDS, wave slots and registers), what the runtime's occupancy query says for the same
                          launch, and the offsets within the limit.  D = 0 stages a window without a halo and walks one
                          offset.
  ``staging_only``        the same call with an A of one voxel: every tile stages its window of B and leaves, one tile
                          walks -- what staging costs at that reach; the rest of a full call is the walk and the booking
  ``nearest_label``       ``nearest_label(b, spacing, D, where=a > 0)``: three passes with a double and an int per voxel;
                          it answers the union rows and the nearest partner only
  ``instance_overlaps``   the pair table at reach 0, geometry-free
  ``instance_sums``       existing code that reads one mask once

There is no pass or fail number.

    python tools/bench_proximity.py --out profiles/proximity_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_clean import build_mask, spread, timed  # noqa: E402
from tools.bench_overlaps import rolled_copy  # noqa: E402

SPACING = (1.0, 1.0, 3.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256),
                    help="X Y Z [X Y Z ...]")
    ap.add_argument("--distances", type=float, nargs="+", default=(0.0, 2.0, 3.0, 5.0))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_proximity needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import nearest_label
    from skoots_amd.validate.lib import id_rows, instance_overlaps, instance_proximity, instance_sums
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "spacing": list(SPACING),
              "masks": []}

    def series(fn, nbytes=None):
        fn()                                                             # warm-up: allocator, kernels loaded
        runs = []
        for _ in range(args.repeats):
            out, t = timed(fn, device)
            runs.append(t)
            del out
        return spread(runs, nbytes)

    def reach(distance):
        out = np.zeros(8, dtype=np.int32)
        _ffi.check(_ffi.lib.sk_instance_proximity_reach(*(s * s for s in SPACING), distance * distance, out.ctypes.data))
        return {"reach": out[:3].tolist(), "lds_bytes": int(out[4]), "workgroups_per_cu": int(out[5]),
                "threads_per_workgroup": int(out[6]), "workgroups_per_cu_by_runtime": resident(distance)}

    def resident(distance):
        n = np.zeros(1, dtype=np.int32)
        _ffi.check(_ffi.lib.sk_instance_proximity_resident(*(s * s for s in SPACING), distance * distance, n.ctypes.data))
        return int(n[0])

    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]
    for shape in shapes:
        a, cells = build_mask(shape, device)
        b = rolled_copy(a, cells, device)
        ra, rb = id_rows(a), id_rows(b)
        entry = {"shape": list(shape), "instances_a": int(ra[1][1].numel()), "instances_b": int(rb[1][1].numel()),
                 "foreground_fraction": float((a > 0).float().mean()), "distances": []}
        entry["instance_overlaps"] = series(lambda: instance_overlaps(a, b, False, ra, rb), 8 * a.numel())
        entry["instance_sums"] = series(lambda: instance_sums(a, ra), 4 * a.numel())
        where = a > 0
        lone = torch.zeros_like(a)                                       # one voxel of A: every tile is staged, one is walked
        lone[0, 0, 0] = 1
        rlone = id_rows(lone)
        for distance in args.distances:
            d = {"distance": distance, **reach(distance)}
            h = d["reach"]
            d["offsets_within_limit"] = sum(
                SPACING[0] ** 2 * float(i * i) + (SPACING[1] ** 2 * float(j * j) + SPACING[2] ** 2 * float(k * k))
                <= distance * distance
                for i in range(-h[0], h[0] + 1) for j in range(-h[1], h[1] + 1) for k in range(-h[2], h[2] + 1))
            d["two_masks"] = series(lambda: instance_proximity(a, b, distance, SPACING, ra, rb), 8 * a.numel())
            d["two_masks"]["rows"] = int(instance_proximity(a, b, distance, SPACING, ra, rb)[2].shape[0])
            d["one_mask"] = series(lambda: instance_proximity(a, None, distance, SPACING, ra), 4 * a.numel())
            d["one_mask"]["rows"] = int(instance_proximity(a, None, distance, SPACING, ra)[2].shape[0])
            d["staging_only"] = series(lambda: instance_proximity(lone, b, distance, SPACING, rlone, rb), 8 * a.numel())
            d["nearest_label"] = series(lambda: nearest_label(b, SPACING, distance, where=where, rows=rb))
            for k in ("two_masks", "one_mask"):
                d[k]["ratio_to_nearest_label"] = d[k]["median_s"] / d["nearest_label"]["median_s"]
                d[k]["ratio_to_instance_overlaps"] = d[k]["median_s"] / entry["instance_overlaps"]["median_s"]
                d[k]["ratio_to_instance_sums"] = d[k]["median_s"] / entry["instance_sums"]["median_s"]
            entry["distances"].append(d)
            print(f"{shape} D={distance}: staging only {d['staging_only']['median_s']:.6f} s, two masks "
                  f"{d['two_masks']['median_s']:.6f} s, one mask "
                  f"{d['one_mask']['median_s']:.6f} s, nearest_label {d['nearest_label']['median_s']:.6f} s",
                  file=sys.stderr, flush=True)
        report["masks"].append(entry)
        del a, b, ra, rb, where
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
