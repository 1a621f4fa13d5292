#!/usr/bin/env python
"""Time the pieces of ``compare()`` (``sk_instance_surface_count``, ``sk_instance_surface_emit``, ``sk_surface_distances``,
DESIGN.md section 25) on a synthetic pair of 1024 x 1024 x 256 int32 masks: the ground truth is the blob mask of
tools/bench_instance_stats.py, the prediction is that mask shifted by (2, 1, 0) voxels with every second instance
eroded by one voxel.  In one process, alternating within every window:

  * the count pass, the emit pass and the ``torch.sort`` of the keys, of the ground truth (device events around each;
    ids, look-up table and buffers prepared before);
  * the two distance passes over the matched pairs, ground truth -> prediction and back, through
    ``lib.surface_distances`` (so with its launch splitting and the entry point's read-back of the offsets);
  * one worst case for the pruning: a single pair of random voxels of ONE x plane, where no tile can be skipped.  Its
    rate is what ``lib.LAUNCH_BUDGET`` has to be held against.

A pair evaluation is one (query, target) candidate of the definition, counted whether the kernel looked at it or pruned
it: queries x targets, summed over the pairs.  The JSON line gives evaluations per second at the median time for the
matched pairs (pruning included) and for the worst case (every candidate looked at), and how long one launch of
``LAUNCH_BUDGET`` evaluations takes at the worst-case rate.  One warm-up of every piece, then ``--repeats`` windows;
nothing is asserted about time.

    python tools/bench_compare.py --out profiles/compare_bench.json
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

from tools.bench_instance_stats import build_mask, summary, timed  # noqa: E402


def predict(gt):
    """the ground truth shifted by (2, 1, 0); every instance with an even id loses its surface voxels"""
    x = torch.roll(gt, (2, 1), (0, 1))
    x[:2] = 0
    x[:, :1] = 0
    keep = torch.ones_like(x, dtype=torch.bool)
    for axis in range(3):
        for shift in (-1, 1):
            keep &= torch.roll(x, shift, axis) == x
    return torch.where(keep | (x % 2 == 1), x, torch.zeros_like(x))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--blobs", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--worst-case-voxels", type=int, default=1 << 19, help="queries and targets of the one-plane pair")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL

    shape = tuple(args.shape)
    X, Y, Z = shape
    gt = build_mask(shape, args.blobs, device)
    pred = predict(gt)
    rows_g, rows_p = VL.id_rows(gt), VL.id_rows(pred)
    a, ids, lut, max_id = rows_g[1]
    N = int(ids.numel())
    st = _ffi.stream_ptr(device)
    sg, sp = VL.instance_surfaces(gt, rows_g), VL.instance_surfaces(pred, rows_p)        # warm-up, and the inputs
    K = int(sg[2].numel())
    rg, rp = rows_g[1][2][rows_g[1][0]], rows_p[1][2][rows_p[1][0]]
    match = VL.match_instances(VL.mask_iou(rg, rp))
    del rg, rp
    rows_m = torch.nonzero(match >= 0)[:, 0]
    pairs_gp = torch.stack((rows_m, match[rows_m]), 1)
    pairs_pg = pairs_gp.flip(1)
    ng, np_ = sg[1].diff().cpu().numpy(), sp[1].diff().cpu().numpy()
    r, c = pairs_gp.cpu().numpy().T
    evaluations = int((ng[r].astype(object) * np_[c].astype(object)).sum())
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs,
              "gt_instances": N, "pred_instances": int(rows_p[1][1].numel()), "matched_pairs": int(rows_m.numel()),
              "gt_surface_voxels": K, "pred_surface_voxels": int(sp[2].numel()),
              "largest_pair_evaluations": int((ng[r].astype(object) * np_[c].astype(object)).max()) if len(r) else 0,
              "pair_evaluations_per_direction": evaluations, "launch_budget": int(VL.LAUNCH_BUDGET),
              "launches_per_direction": len(VL._launches(sg[1].cpu().numpy(), sp[1].cpu().numpy(),
                                                         pairs_gp.cpu().numpy(), int(VL.LAUNCH_BUDGET))),
              "repeats": args.repeats}

    counts = torch.empty(N, dtype=torch.int64, device=device)
    keys = torch.empty(K, dtype=torch.int64, device=device)
    produced = torch.empty(1, dtype=torch.int64, device=device)

    def count():
        _ffi.check(_ffi.lib.sk_instance_surface_count(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(counts), st))

    def emit():
        _ffi.check(_ffi.lib.sk_instance_surface_emit(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N, K, _ffi.ptr(keys),
                                                     _ffi.ptr(produced), st))

    # the worst case: random distinct voxels of the plane x = 0 of a (1, 4096, 4096) volume, one pair
    n = int(args.worst_case_voxels)
    gen = torch.Generator().manual_seed(25)
    plane = torch.randperm(4096 * 4096, generator=gen)[:2 * n].to(device)
    wq = (torch.tensor([0, n], device=device), torch.sort(plane[:n])[0])
    wt = (torch.tensor([0, n], device=device), torch.sort(plane[n:])[0])

    def worst():
        return VL.surface_distances(wq, wt, [[0, 0]], (1, 4096, 4096))

    for fn in (count, emit, worst):
        fn()
    first_g = VL.surface_distances(sg, sp, pairs_gp, shape)[1]
    first_p = VL.surface_distances(sp, sg, pairs_pg, shape)[1]
    torch.cuda.synchronize(device)
    times = {k: [] for k in ("count", "emit", "sort", "distances_gt_to_pred", "distances_pred_to_gt", "worst_case_pair")}
    same = True
    for _ in range(args.repeats):
        times["count"].append(timed(count, device)[1])
        times["emit"].append(timed(emit, device)[1])
        s, t = timed(lambda: torch.sort(keys)[0], device)
        times["sort"].append(t)
        same &= bool(torch.equal(s, sg[2])) and bool(torch.equal(counts, sg[1].diff())) and int(produced.item()) == K
        d, t = timed(lambda: VL.surface_distances(sg, sp, pairs_gp, shape)[1], device)
        times["distances_gt_to_pred"].append(t)
        same &= bool(torch.equal(d, first_g))
        d, t = timed(lambda: VL.surface_distances(sp, sg, pairs_pg, shape)[1], device)
        times["distances_pred_to_gt"].append(t)
        same &= bool(torch.equal(d, first_p))
        times["worst_case_pair"].append(timed(worst, device)[1])
    report["every_run_equals_the_first"] = bool(same)
    for k, t in times.items():
        report[k] = summary(t)
    both = report["distances_gt_to_pred"]["median_s"] + report["distances_pred_to_gt"]["median_s"]
    report["pair_evaluations_per_s"] = 2 * evaluations / both if both > 0 else None
    report["worst_case_pair_evaluations"] = n * n
    report["worst_case_pair_launches"] = len(VL._launches(np.array([0, n]), np.array([0, n]), np.array([[0, 0]]),
                                                          int(VL.LAUNCH_BUDGET)))
    report["worst_case_pair_evaluations_per_s"] = n * n / report["worst_case_pair"]["median_s"]
    report["launch_budget_seconds_at_worst_case_rate"] = int(VL.LAUNCH_BUDGET) / report["worst_case_pair_evaluations_per_s"]

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
