#!/usr/bin/env python
"""Time ``instance_intensity`` and ``intensity_ring`` on a synthetic instance mask built on the device, beside
``instance_sums`` on the same mask in the same process.

The mask is ``tools/bench_clean.py``'s: one ball per 32^3 cell (seeded centres and radii, ids a seeded permutation) with
specks and pockets, at (1024, 1024, 256), 8192 balls.  Three images of that shape:

  ``u8_noise``     uniform 8-bit noise: the histogram's atomics spread over 256 counters per instance
  ``u8_constant``  every sample 200: all voxels of an instance hit ONE counter, the worst case for the atomics
  ``u16_noise``    uniform 16-bit noise, binned with shift 8

Timed with device events after a warm-up, min / median / max over the repeats, the prologue (``id_rows``) computed once
outside the timed region and the shift given, so that the time is the pass itself (initialising the tables, the launch;
for the 16-bit image also once with ``shift=None``, which adds a pass that finds the largest sample):

  ``instance_sums``       the yardstick: existing code that reads the mask once (4 bytes per voxel)
  ``instance_intensity``  with and without the histogram; the pass must read 4 bytes of mask and 1 or 2 of image per voxel
  ``intensity_ring``      D = 3 at spacing (1, 1, 3): the nearest-instance transform, the ring volume and the same kernel

Every figure is printed beside ``instance_sums`` and beside the bytes the pass must read.  There is no pass or fail
number.

    python tools/bench_intensity.py --out profiles/intensity_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_clean import build_mask, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ring-distance", type=float, default=3.0)
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 3.0))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intensity needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd.validate.lib import id_rows, instance_intensity, instance_sums, intensity_ring
    shape = tuple(args.shape)
    voxels = shape[0] * shape[1] * shape[2]

    def series(fn, nbytes=None):
        fn()                                                             # warm-up: allocator, kernels loaded
        runs = []
        for _ in range(args.repeats):
            out, t = timed(fn, device)
            runs.append(t)
            del out
        return spread(runs, nbytes)

    mask = build_mask(shape, device)[0]
    rows = id_rows(mask)
    g = torch.Generator(device=device)
    g.manual_seed(5)
    images = {
        "u8_noise": (torch.randint(0, 256, shape, generator=g, device=device, dtype=torch.int32).to(torch.uint8), 0),
        "u8_constant": (torch.full(shape, 200, dtype=torch.uint8, device=device), 0),
        "u16_noise": (torch.randint(0, 65536, shape, generator=g, device=device, dtype=torch.int32).to(torch.uint16), 8),
    }
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "shape": list(shape),
              "instances": int(rows[1][1].numel()), "foreground_fraction": float((mask > 0).float().mean()),
              "instance_sums": series(lambda: instance_sums(mask, rows), 4 * voxels), "images": {}}
    base = report["instance_sums"]["median_s"]
    for name, (img, shift) in images.items():
        per_voxel = 4 + img.element_size()
        entry = {"bytes_per_voxel": per_voxel}
        for want_hist in (True, False):
            d = series(lambda: instance_intensity(mask, img, rows, want_hist, shift), per_voxel * voxels)
            d["ratio_to_instance_sums"] = d["median_s"] / base
            entry["with_histogram" if want_hist else "without_histogram"] = d
        if img.element_size() == 2:                                       # shift=None: one more pass finds image.max()
            d = series(lambda: instance_intensity(mask, img, rows, True, None), (per_voxel + 2) * voxels)
            d["ratio_to_instance_sums"] = d["median_s"] / base
            entry["with_histogram_auto_shift"] = d
        d = series(lambda: intensity_ring(mask, img, args.ring_distance, tuple(args.spacing), rows))
        d["ratio_to_instance_sums"] = d["median_s"] / base
        d["distance"], d["spacing"] = args.ring_distance, list(args.spacing)
        entry["ring"] = d
        report["images"][name] = entry
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
