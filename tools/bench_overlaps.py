#!/usr/bin/env python
"""Time ``instance_overlaps`` and what stands on it on synthetic instance masks built on the device, beside the dense
path and the torch statement it replaces.

The masks are ``tools/bench_clean.py``'s: one ball per 32^3 cell (seeded centres and radii, ids a seeded permutation)
with specks and pockets, at (512, 512, 128) and at (1024, 1024, 256), 8192 balls.  The second mask of a pair is the
first rolled by (3, 2, 1) voxels with its ids permuted, so every ball overlaps its own copy and little else.

Timed with device events after a warm-up, min / median / max over the repeats, the prologues (``id_rows``) computed
once outside the timed region where the function takes them:

  ``instance_overlaps``   with and without background; the time holds the launch, the read-back of the two counters,
                          any retry at a larger table, and the sort of the rows
  ``sparse_mask_iou``     the whole call, prologues included
  ``compare(sparse=True)``  the whole call
  ``mask_iou``, ``compare()``  the dense yardsticks, whole calls, as they stand
  ``instance_sums``       existing code that reads one mask once
  ``torch.unique``        ``torch.unique(ra * (M + 1) + rb, return_counts=True)`` on the two row volumes: the torch
                          statement the kernel replaces

The report also gives the peak device memory of the dense and the sparse ``compare`` above what is allocated before the
call (``torch.cuda.max_memory_allocated``), and the share of the HBM peak at which ``instance_overlaps`` reads its 8 bytes
per voxel.  There is no pass or fail number.

    python tools/bench_overlaps.py --out profiles/overlaps_bench.json
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


def rolled_copy(mask, cells, device, seed=12):
    """the mask rolled by (3, 2, 1) with its ids 1 .. cells permuted"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    perm = torch.cat((torch.zeros(1, dtype=torch.int32, device=device),
                      (torch.randperm(cells, generator=g, device=device) + 1).to(torch.int32)))
    return perm[torch.roll(mask, (3, 2, 1), (0, 1, 2))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256),
                    help="X Y Z [X Y Z ...]")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlaps needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd.validate.compare import compare
    from skoots_amd.validate.lib import (_Rows, id_rows, instance_overlaps, instance_sums, mask_iou, sparse_mask_iou)
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "masks": []}

    def series(fn, nbytes=None):
        fn()                                                             # warm-up: allocator, kernels loaded
        runs = []
        for _ in range(args.repeats):
            out, t = timed(fn, device)
            runs.append(t)
            del out
        return spread(runs, nbytes)

    def peak(fn):
        torch.cuda.synchronize(device)
        torch.cuda.reset_peak_memory_stats(device)
        before = torch.cuda.memory_allocated(device)
        out = fn()
        torch.cuda.synchronize(device)
        del out
        return int(torch.cuda.max_memory_allocated(device) - before)

    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]
    for shape in shapes:
        a, cells = build_mask(shape, device)
        b = rolled_copy(a, cells, device)
        ra, rb = id_rows(a), id_rows(b)
        N, M = int(ra[1][1].numel()), int(rb[1][1].numel())
        entry = {"shape": list(shape), "instances_a": N, "instances_b": M,
                 "foreground_fraction": float((a > 0).float().mean())}
        nbytes = 8 * a.numel()
        for background in (False, True):
            d = series(lambda: instance_overlaps(a, b, background, ra, rb), nbytes)
            d["pairs"] = int(instance_overlaps(a, b, background, ra, rb)[2].shape[0])
            entry["instance_overlaps" + ("_background" if background else "")] = d
        entry["sparse_mask_iou"] = series(lambda: sparse_mask_iou(a, b))
        entry["compare_sparse"] = series(lambda: compare(a, b, sparse=True))
        entry["mask_iou"] = series(lambda: mask_iou(a, b))
        entry["compare_dense"] = series(lambda: compare(a, b))
        entry["instance_sums"] = series(lambda: instance_sums(a, ra), 4 * a.numel())
        va, vb = _Rows(a, ra).row_volume(), _Rows(b, rb).row_volume()
        entry["torch_unique"] = series(lambda: torch.unique(va.long() * (M + 1) + vb, return_counts=True))
        del va, vb
        entry["compare_dense_peak_bytes"] = peak(lambda: compare(a, b))
        entry["compare_sparse_peak_bytes"] = peak(lambda: compare(a, b, sparse=True))
        base = entry["instance_sums"]["median_s"]
        for k in ("instance_overlaps", "instance_overlaps_background", "torch_unique"):
            entry[k]["ratio_to_instance_sums"] = entry[k]["median_s"] / base
        report["masks"].append(entry)
        del a, b, ra, rb
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
