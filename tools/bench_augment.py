#!/usr/bin/env python3
"""Times one training sample's augmentation (skoots_amd/train/transforms.py, csrc/augment.hip) against a torch-eager
restatement of the reference's TransformFromCfg (skoots/train/merged_transform.py:402-762) on the same GPU.

    python tools/bench_augment.py [--volume 1024 1024 64] [--reps 20] [--warmup 3]

Default cfg (300 x 300 x 20 output, crop 1 = 600 x 600 x 20) from a uint8 volume with int16 masks, one plan with every
stage on.  Both legs do crop 1 .. normalise plus skeleton_to_mask (bake_skeleton, the same HIP call in both, is timed
apart).  Each leg is timed with the volume held on the CPU (the reference's layout: the crop-1 window is copied to
the device every sample) and with the volume already on the device.  Prints one JSON line of ms per sample (host
clock around work that ends in a device synchronise, after a warm-up)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = {"AUGMENTATION": dict(CROP_WIDTH=300, CROP_HEIGHT=300, CROP_DEPTH=20, FLIP_RATE=0.5, BRIGHTNESS_RATE=0.4,
                            BRIGHTNESS_RANGE=[-0.1, 0.1], NOISE_GAMMA=0.1, NOISE_RATE=0.2, CONTRAST_RATE=0.33,
                            CONTRAST_RANGE=[0.75, 2.0], AFFINE_RATE=0.66, AFFINE_SCALE=[0.85, 1.1],
                            AFFINE_YAW=[-180, 180], AFFINE_SHEAR=[-7, 7], ELASTIC_GRID_SHAPE=(6, 6, 2),
                            ELASTIC_GRID_MAGNITUDE=(0.05, 0.05, 0.01), ELASTIC_RATE=0.33,
                            BAKE_SKELETON_ANISOTROPY=(1.0, 1.0, 3.0)),
       "TRAIN": dict(SKELETON_MASK_RADIUS=9, SKELETON_MASK_FLANK_RADIUS=3)}


def torch_reference(t, image, masks, skeletons, plan, dev):
    """The reference's voxel stages in eager torch (grid_sample / interpolate / flips / reductions / index_put)."""
    from skoots_amd.lib.skeleton import get_cached_disk_coords
    from skoots_amd.train.transforms import _rss
    (w1, h1, d1), (w2, h2, d2) = t.crop_extents(image.shape)
    g = t.geometry(image.shape, skeletons, plan, dev)     # crop origins and the skeleton points (N points)
    x0, y0, z0 = g["crop1"]
    img = image[:, x0:x0 + w1, y0:y0 + h1, z0:z0 + d1].to(dev).float()
    msk = masks[:, x0:x0 + w1, y0:y0 + h1, z0:z0 + d1].to(dev).float()
    if plan.elastic:
        off = F.interpolate(plan.elastic_field, (w1, h1, d1), mode="trilinear").permute(0, 2, 3, 4, 1)
        off = off * torch.tensor((0.01, 0.05, 0.05), device=dev).view(1, 1, 1, 1, 3)
        mx, my, mz = torch.meshgrid(torch.linspace(-1, 1, w1, device=dev), torch.linspace(-1, 1, h1, device=dev),
                                    torch.linspace(-1, 1, d1, device=dev), indexing="ij")
        grid = torch.stack((mz, my, mx), 3).unsqueeze(0) + off
        img = F.grid_sample(img.unsqueeze(0), grid, mode="nearest", align_corners=True)[0]
        msk = F.grid_sample(msk.unsqueeze(0), grid, mode="nearest", align_corners=True)[0]
    if plan.affine:
        a, b, c, d = _rss(plan.angle, (plan.shear, 0.0), plan.scale)
        theta = torch.tensor([d, -b, 0.0, -c, a, 0.0], device=dev).view(1, 2, 3) / plan.scale
        base = torch.empty(1, w1, h1, 3, device=dev)
        base[..., 0].copy_(torch.linspace(-h1 * 0.5 + 0.5, h1 * 0.5 - 0.5, h1, device=dev))
        base[..., 1].copy_(torch.linspace(-w1 * 0.5 + 0.5, w1 * 0.5 - 0.5, w1, device=dev).unsqueeze(-1))
        base[..., 2].fill_(1)
        grid = base.view(1, -1, 3).bmm(theta.transpose(1, 2) / torch.tensor([0.5 * h1, 0.5 * w1], device=dev))
        grid = grid.view(1, w1, h1, 2)
        img = F.grid_sample(img.permute(0, 3, 1, 2), grid, mode="nearest", align_corners=False).permute(0, 2, 3, 1)
        msk = F.grid_sample(msk.permute(0, 3, 1, 2), grid, mode="nearest", align_corners=False).permute(0, 2, 3, 1)
    cx, cy, cz = g["crop2"]
    img, msk = img[:, cx:cx + w2, cy:cy + h2, cz:cz + d2], msk[:, cx:cx + w2, cy:cy + h2, cz:cz + d2]
    for axis, flip in ((1, plan.flip_x), (2, plan.flip_y), (3, plan.flip_z)):
        if flip:
            img, msk = img.flip(axis), msk.flip(axis)
    if plan.invert:
        img = img.sub(255).mul(-1)
    if plan.brightness:
        img = img.add(plan.brightness_val).clamp(0, 255)
    if plan.contrast:
        z = img.div(255).permute(3, 0, 1, 2)
        mean = z.mean(dim=(-3, -2, -1), keepdim=True)
        img = (plan.contrast_val * z + (1.0 - plan.contrast_val) * mean).clamp(0, 1).permute(1, 2, 3, 0).mul(255)
    if plan.noise is not None:
        img = img.add(plan.noise * t.NOISE_GAMMA)
    img = img.sub(img.mean())
    cached = get_cached_disk_coords(torch.device(dev), 9, 3)
    skm = torch.zeros((w2, h2, d2), device=dev)
    for v in g["skeletons"].values():
        ind = (v.T.unsqueeze(1) + cached.unsqueeze(2)).reshape(3, -1).long()
        ok = ((ind[0] >= 0) & (ind[0] < w2) & (ind[1] >= 0) & (ind[1] < h2) & (ind[2] >= 0) & (ind[2] < d2))
        skm[ind[0, ok], ind[1, ok], ind[2, ok]] = 1.0
    return img, msk, skm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, nargs=3, default=[1024, 1024, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs the MI355X")
    from skoots_amd.lib.skeleton import bake_skeleton, skeleton_to_mask
    from skoots_amd.train import AugmentPlan, TransformFromCfg
    dev = "cuda:0"
    X, Y, Z = args.volume
    gen = torch.Generator().manual_seed(0)
    image = torch.randint(0, 256, (1, X, Y, Z), generator=gen, dtype=torch.uint8)
    masks = torch.zeros((1, X, Y, Z), dtype=torch.int16)
    skeletons = {}
    for k in range(1, 41):
        c = [int(torch.randint(40, s - 40, (1,), generator=gen)) if s > 80 else s // 2 for s in (X, Y, Z)]
        masks[0, c[0] - 30:c[0] + 30, c[1] - 30:c[1] + 30, max(0, c[2] - 6):c[2] + 6] = k
        n = 60
        line = torch.stack([torch.linspace(c[0] - 25, c[0] + 25, n), torch.full((n,), float(c[1])),
                            torch.full((n,), float(c[2]))], 1)
        skeletons[k] = line
    t = TransformFromCfg(CFG, dev)
    (w1, h1, d1), (w2, h2, d2) = t.crop_extents(image.shape)
    g = torch.Generator(device=dev).manual_seed(1)
    plan = AugmentPlan(key=7, elastic=True, elastic_field=torch.rand((1, 3, 2, 6, 6), generator=g, device=dev),
                       affine=True, angle=37.0, shear=3.0, scale=0.95, flip_x=True, flip_y=True, flip_z=True,
                       invert=True, brightness=True, brightness_val=0.05, contrast=True, contrast_val=1.3,
                       noise=torch.rand((1, w2, h2, d2), generator=g, device=dev))
    vols = {"cpu": (image, masks), "gpu": (image.to(dev), masks.to(dev))}

    def hip(where):
        img, msk = vols[where]
        out, m, sk = t.augment(img, msk, skeletons, plan)
        return skeleton_to_mask(sk, (w2, h2, d2), device=dev, radius=9, flank_radius=3)

    def ref(where):
        img, msk = vols[where]
        return torch_reference(t, img, msk, skeletons, plan, dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.reps

    res = {}
    for where in ("cpu", "gpu"):   # alternate the two legs
        res[f"hip_ms_volume_{where}"] = round(timed(lambda: hip(where)), 3)
        res[f"torch_ms_volume_{where}"] = round(timed(lambda: ref(where)), 3)
    _, msk_out, sk_out = t.augment(vols["gpu"][0], vols["gpu"][1], skeletons, plan)
    res["bake_skeleton_ms"] = round(timed(lambda: bake_skeleton(msk_out, sk_out, (1.0, 1.0, 3.0), average=True)), 3)
    res["forward_ms_volume_cpu"] = round(timed(lambda: t({"image": image, "masks": masks, "skeletons": skeletons},
                                                         plan=plan)), 3)
    window = w1 * h1 * d1 * (image.element_size() + masks.element_size())
    print(json.dumps({"metric": "augment_ms_per_sample", "unit": "ms", "volume": [X, Y, Z],
                      "output": [w2, h2, d2], "crop1_window_bytes": window, **res,
                      "speedup_volume_cpu": round(res["torch_ms_volume_cpu"] / res["hip_ms_volume_cpu"], 2),
                      "speedup_volume_gpu": round(res["torch_ms_volume_gpu"] / res["hip_ms_volume_gpu"], 2)}))


if __name__ == "__main__":
    main()
