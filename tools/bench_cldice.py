#!/usr/bin/env python3
"""Times soft_dice_cldice value + gradient (skoots_amd/csrc/cldice.hip) against torch autograd of the reference
formula (skoots/train/loss.py:269-310, 344-391, restated below) on the same GPU.

    python tools/bench_cldice.py [--shape 256 256 256] [--batch 1] [--iter 3] [--reps 10] [--warmup 2]

Prints one JSON line: ms per value + gradient of both paths (HIP events after a warm-up), the bytes the HIP path
moves per voxel on paper and that traffic over its measured time."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_soft_skeletonize(img, iter_):
    def erode(x):
        p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
        p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
        return torch.min(torch.min(p1, p2), p3)

    def dilate(x):
        return F.max_pool3d(x, (3, 3, 3), (1, 1, 1), (1, 1, 1))

    skel = F.relu(img - dilate(erode(img)))
    for _ in range(iter_):
        img = erode(img)
        delta = F.relu(img - dilate(erode(img)))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def torch_soft_dice_cldice(pred, gt, iter_=3, alpha=0.5, smooth=1.0):
    dice = 1.0 - (2.0 * torch.sum(gt * pred) + 1) / (torch.sum(gt) + torch.sum(pred) + 1)
    sp, st = torch_soft_skeletonize(pred, iter_), torch_soft_skeletonize(gt, iter_)
    tprec = (torch.sum(sp * gt) + smooth) / (torch.sum(sp) + smooth)
    tsens = (torch.sum(st * pred) + smooth) / (torch.sum(st) + smooth)
    return (1.0 - alpha) * dice + alpha * (1.0 - 2.0 * (tprec * tsens) / (tprec + tsens))


def bytes_per_voxel(iter_):
    """HBM traffic of the HIP path per voxel, every stencil operand read once (caches absorb the neighbours)."""
    L = iter_ + 1
    fwd = L * 16 + L * 32 - 8 + 8          # erode (2 sides in, 2 out); skeleton (e, e', skel_prev in, skel out) x 2; sums
    b1 = 29 * iter_ + 21                   # e', e, skel_prev, dskel in; direct, dopen, dskel_prev, code out
    b2 = 13 * iter_ + 9                    # code, dopen, de_up in; T out
    b3 = 16 * L + 8                        # direct, e, T in; de out (+ gt, S_t at level 0)
    return fwd + b1 + b2 + b3


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 256, 256])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iter", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from skoots_amd.train import soft_dice_cldice
    dev = torch.device("cuda:0")
    X, Y, Z = args.shape
    shape = (args.batch, 1, X, Y, Z)
    gen = torch.Generator(device=dev).manual_seed(3)
    pred = torch.sigmoid(torch.randn(shape, device=dev, generator=gen) * 8.0)   # saturated plateaus of exactly 1.0
    gt = (torch.rand(shape, device=dev, generator=gen) > 0.7).float()
    fn = soft_dice_cldice(iter_=args.iter)
    hip_ms = timed(lambda: fn.value_and_grad(pred, gt), args.reps, args.warmup)
    hip_loss = fn(pred, gt).item()

    def ref():
        p = pred.detach().requires_grad_(True)
        loss = torch_soft_dice_cldice(p, gt, args.iter)
        loss.backward()
        return loss

    torch_ms = timed(ref, max(2, args.reps // 2), 1)
    torch_loss = ref().item()
    nvox = args.batch * X * Y * Z
    bpv = bytes_per_voxel(args.iter)
    print(json.dumps({"metric": "cldice_value_and_grad_ms", "value": round(hip_ms, 3), "unit": "ms",
                      "torch_autograd_ms": round(torch_ms, 3), "speedup": round(torch_ms / hip_ms, 2),
                      "bytes_per_voxel_on_paper": bpv, "effective_tb_per_s": round(bpv * nvox / (hip_ms * 1e-3) / 1e12, 2),
                      "loss_hip": hip_loss, "loss_torch": torch_loss,
                      "config": {"shape": [args.batch, 1, X, Y, Z], "iter_": args.iter, "alpha": 0.5, "smooth": 1.0}}))


if __name__ == "__main__":
    main()
