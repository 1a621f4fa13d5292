#!/usr/bin/env python3
"""Times the validation matrices on a synthetic pair of the size the validate command keeps of a
1024 x 1024 x 256 volume (924 x 924 x 246, a few thousand instances).

    python tools/bench_validate.py [--reps 5] [--pairs 8] [--no-eager]

Prints one JSON line: mask_metrics and mask_iou times, bytes per pass against HBM rate, and a torch-eager
restatement of the reference's per-pair clDice loop (validate/lib.py:276-315) timed on a sample of touching pairs
and extrapolated to all of them.  Kernel times: run under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12


def synthetic_pair(shape, n_ids, seed=0, dev="cuda"):
    """blocky instances (a share of background blocks) with noise; pred is gt shifted, relabelled and noisier"""
    g = torch.Generator(device=dev).manual_seed(seed)
    X, Y, Z = shape
    block = (6, 23, 23)
    cs = [-(-s // b) for s, b in zip(shape, block)]
    coarse = torch.randint(1, n_ids + 1, cs, generator=g, device=dev, dtype=torch.int32)
    coarse[torch.rand(cs, generator=g, device=dev) < 0.5] = 0
    gt = coarse.repeat_interleave(block[0], 0).repeat_interleave(block[1], 1).repeat_interleave(block[2], 2)
    gt = gt[:X, :Y, :Z].contiguous()
    noise = torch.rand(shape, generator=g, device=dev) < 0.02
    gt[noise] = 0
    pred = torch.roll(gt, (1, 3, -2), (0, 1, 2))
    pred = torch.where(pred > 0, (pred * 13 + 5) % (n_ids + 50) + 1, pred)
    noise = torch.rand(shape, generator=g, device=dev) < 0.02
    pred[noise] = 0
    return gt[None].contiguous(), pred[None].contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


# the reference's soft skeleton and soft_cldice on (1, X, Y, Z) float masks (train/loss.py:269-338), restated
def _erode(img):
    return torch.min(-F.max_pool2d(-img, (3, 1), (1, 1), (1, 0)), -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1)))


def _skel(img, iters=3):
    skel = F.relu(img - F.max_pool2d(_erode(img), (3, 3), (1, 1), (1, 1)))
    for _ in range(iters):
        img = _erode(img)
        delta = F.relu(img - F.max_pool2d(_erode(img), (3, 3), (1, 1), (1, 1)))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def _cldice(pred, gt):
    sp, sg = _skel(pred), _skel(gt)
    tprec = (torch.sum((sp * gt)[:, 1:]) + 1.0) / (torch.sum(sp[:, 1:]) + 1.0)
    tsens = (torch.sum((sg * pred)[:, 1:]) + 1.0) / (torch.sum(sg[:, 1:]) + 1.0)
    return 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(924, 924, 246))
    ap.add_argument("--ids", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    from skoots_amd.validate import mask_dice, mask_iou, mask_metrics
    gt, pred = synthetic_pair(tuple(a.shape), a.ids)
    iou, dice, cl = mask_metrics(gt, pred)
    N, M = iou.shape
    touching = int((iou > 0).sum().item())
    vox = gt.numel()
    halo = 3 + 2
    stage = (32 + 2 * halo) * (64 + 2 * halo) / (32 * 64)
    res = {"shape": list(a.shape), "N": N, "M": M, "touching_pairs": touching,
           "ms_mask_metrics": timed(lambda: mask_metrics(gt, pred), a.reps),
           "ms_mask_iou": timed(lambda: mask_iou(gt, pred), a.reps),
           "ms_mask_dice": timed(lambda: mask_dice(gt, pred), a.reps),
           # two int32 volumes, staged with the iters + 2 halo; three tables written, re-read for the sums
           "metrics_volume_bytes": int(8 * vox * stage), "metrics_table_bytes": int(3 * 4 * (N + 1) * (M + 1) * 3)}
    res["metrics_hbm_floor_ms"] = (res["metrics_volume_bytes"] + res["metrics_table_bytes"]) / HBM_BYTES_PER_S * 1e3
    if not a.no_eager:
        pairs = torch.nonzero(iou > 0)[torch.randperm(touching, generator=torch.Generator().manual_seed(1))[:a.pairs]]
        ids_a, ids_b = torch.unique(gt), torch.unique(pred)
        ids_a, ids_b = ids_a[ids_a > 0], ids_b[ids_b > 0]

        def per_pair():
            for i, j in pairs.tolist():
                _a, _b = gt == ids_a[i], pred == ids_b[j]
                _cldice(_b.float(), _a.float())

        ms = timed(per_pair, 1)
        res["eager_ms_per_pair"] = ms / len(pairs)
        res["eager_pairs_timed"] = len(pairs)
        res["eager_extrapolated_s_all_pairs"] = ms / len(pairs) * touching / 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
