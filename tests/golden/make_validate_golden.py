#!/usr/bin/env python3
"""Generate the validation fixtures under tests/golden/ from the REFERENCE's own functions.

Run where the reference checkout is available (GPU tests read only the committed .npz), like make_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \\
        python tests/golden/make_validate_golden.py

``torch.compile`` is replaced by the identity: on binary masks the compiled soft_cldice cannot change the
integer-valued sums.  ``skimage.io.imread`` is a placeholder that returns the arrays handed to ``main()``.

  G13 validate_cldice.npz  mask_dice / mask_soft_cldice (validate/lib.py:232-315) on label pairs, per-instance
                           soft_skeletonize flags (train/loss.py:295-310) for iter_ 0/1/3/5, and the two CSV texts
                           of validate/__main__.py:main() on one 130x132x14 pair
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_IMAGES = {}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _ident(*a, **k):
    return a[0] if a and callable(a[0]) else (lambda f: f)


_stub("numba", njit=_ident, prange=range)
_sk = _stub("skimage")
_sk.morphology = _stub("skimage.morphology")
_sk.io = _stub("skimage.io", imread=lambda path: _IMAGES[os.path.basename(path)])
_stub("bism")
for _s in ("backends", "modules", "models", "models.spatial_embedding"):
    _stub("bism." + _s)
sys.modules["bism.models.spatial_embedding"].SpatialEmbedding = object
_y = _stub("yacs")
_y.config = _stub("yacs.config", CfgNode=dict)
torch.compile = lambda m, *a, **k: m

from skoots.train.loss import soft_skeletonize  # noqa: E402
from skoots.validate import __main__ as ref_main  # noqa: E402
from skoots.validate.lib import mask_dice, mask_soft_cldice  # noqa: E402


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def blocky(gen, shape, n_ids, block=(1, 6, 6), noise=0.15, bg=0.3, id_base=1):
    """(X, Y, Z) int32 labels: random blocks of ids (a share of them background), then per-voxel noise."""
    X, Y, Z = shape
    cs = [max(1, -(-s // b)) for s, b in zip(shape, block)]
    coarse = torch.randint(id_base, id_base + n_ids, cs, generator=gen, dtype=torch.int64)
    coarse[torch.rand(cs, generator=gen) < bg] = 0
    lab = coarse.repeat_interleave(block[0], 0).repeat_interleave(block[1], 1).repeat_interleave(block[2], 2)
    lab = lab[:X, :Y, :Z].clone()
    flip = torch.rand(shape, generator=gen) < noise
    lab[flip] = torch.randint(id_base - 1, id_base + n_ids, shape, generator=gen, dtype=torch.int64)[flip]
    lab[lab == id_base - 1] = 0
    return lab.to(torch.int32)


def skel_flags(lab4, iters):
    """union over ids of the reference's per-instance soft skeleton: uint8 (1, X, Y, Z)"""
    out = torch.zeros(lab4.shape, dtype=torch.uint8)
    for a in torch.unique(lab4):
        if a <= 0:
            continue
        s = soft_skeletonize((lab4 == a).float(), iters)
        assert bool(((s == 0) | (s == 1)).all())
        out[s > 0] = 1
    return out.numpy()


def pair_case(out, name, gt, pred):
    gt4, pred4 = gt[None].contiguous(), pred[None].contiguous()
    out[name + "_gt"], out[name + "_pred"] = gt4.numpy(), pred4.numpy()
    out[name + "_dice"] = mask_dice(gt4, pred4).numpy()
    out[name + "_cldice"] = mask_soft_cldice(gt4, pred4).numpy()


def perturbed(gen, gt, n_ids, shift=1):
    """a prediction made from gt: shifted along y, relabelled, noisy; no instance identical to a gt one"""
    p = torch.roll(gt, shift, dims=1).clone()
    pos = p > 0
    p[pos] = (p[pos] * 7 + 3) % (n_ids + 5) + 1
    noise = torch.rand(gt.shape, generator=gen) < 0.1
    p[noise] = torch.randint(0, n_ids + 6, gt.shape, generator=gen, dtype=torch.int32)[noise]
    return p


def g13():
    gen = torch.Generator().manual_seed(1313)
    out = {}
    names = []

    # random pairs: blocky and noisy labels, X = 1..5, Y / Z up to 40
    for k, (shape, n, block) in enumerate([((3, 24, 20), 12, (1, 5, 5)), ((5, 40, 36), 30, (1, 7, 6)),
                                           ((2, 17, 39), 9, (1, 4, 8)), ((4, 33, 28), 40, (2, 5, 5)),
                                           ((6, 40, 36), 25, (1, 8, 8))]):
        gt = blocky(gen, shape, n, block)
        pair_case(out, f"rand{k}", gt, perturbed(gen, gt, n, shift=k % 3))
        names.append(f"rand{k}")

    # X = 1: the only slice is x = 0, so every clDice sum is empty (tprec = tsens = 1)
    gt = blocky(gen, (1, 30, 26), 10)
    pair_case(out, "x1", gt, perturbed(gen, gt, 10))
    names.append("x1")

    # pairs that touch only at x = 0 (and pairs that touch only at x >= 1)
    gt = torch.zeros((3, 20, 20), dtype=torch.int32)
    pred = torch.zeros_like(gt)
    gt[:, 2:10, 2:12] = 5
    pred[0, 4:12, 4:14] = 8                          # touches 5 at x = 0 only
    pred[1:, 2:10, 14:19] = 9                        # touches nothing
    gt[1:, 12:18, 3:15] = 6
    pred[1:, 13:19, 5:17] = 11                       # touches 6 at x >= 1 only
    pred[0, 12:18, 3:10] = 12                        # x = 0, outside gt 6 (which starts at x = 1)
    pair_case(out, "touch_x0", gt, pred)
    names.append("touch_x0")

    # instances on the y / z borders, 1-voxel-wide lines and single voxels
    gt = torch.zeros((3, 16, 18), dtype=torch.int32)
    pred = torch.zeros_like(gt)
    gt[:, 0:6, 0:18] = 1                             # along the whole y = 0 border
    gt[:, 10:16, 12:18] = 2                          # in the (Y-1, Z-1) corner
    gt[:, 8, 0:10] = 3                               # a 1-voxel-wide line
    gt[1, 12, 3] = 4                                 # single voxels
    gt[2, 14, 8] = 4
    gt[:, 0:16, 11] = 7                              # a line across the whole slice
    pred[:, 0:5, 1:18] = 21
    pred[:, 11:16, 11:18] = 22
    pred[:, 8, 1:11] = 23
    pred[1, 12, 3:5] = 24
    pred[0:2, 0:16, 11] = 27
    pair_case(out, "border_thin", gt, pred)
    names.append("border_thin")

    # ids above 65535 (and negative values, which are not instances)
    gt = blocky(gen, (3, 28, 22), 14, id_base=70000)
    pred = blocky(gen, (3, 28, 22), 9, id_base=1 << 20)
    gt[0, 0, :3] = -4
    pair_case(out, "big_ids", gt, pred)
    names.append("big_ids")

    # one volume empty
    gt = blocky(gen, (2, 20, 20), 8)
    pair_case(out, "empty_pred", gt, torch.zeros_like(gt))
    names.append("empty_pred")
    out["pair_names"] = np.array(names)

    # per-instance soft skeletons, iter_ 0 / 1 / 3 / 5
    skn = []
    for k, (shape, n, block) in enumerate([((2, 39, 37), 15, (1, 9, 7)), ((4, 21, 33), 30, (1, 4, 4)),
                                           ((1, 40, 40), 6, (1, 14, 12)), ((3, 16, 39), 20, (1, 3, 10))]):
        lab = blocky(gen, shape, n, block, noise=0.05 if k % 2 else 0.2)[None].contiguous()
        out[f"skel{k}_labels"] = lab.numpy()
        for it in (0, 1, 3, 5):
            out[f"skel{k}_it{it}"] = skel_flags(lab, it)
        skn.append(f"skel{k}")
    for name in names:                               # the pair cases' own skeletons at the metric's iter_ 3
        for side in ("gt", "pred"):
            out[f"{name}_{side}_skel3"] = skel_flags(torch.from_numpy(out[f"{name}_{side}"]), 3)
    out["skel_names"] = np.array(skn)

    # the command on one 130 x 132 x 14 pair ([Z, X, Y] as a tif stores it); the crop keeps 30 x 32 x 4
    X, Y, Z = 130, 132, 14
    gt = blocky(gen, (X, Y, Z), 40, (4, 6, 2), noise=0.05, bg=0.25)
    pred = perturbed(gen, gt, 40)
    gt_zxy = gt.permute(2, 0, 1).contiguous().numpy().astype(np.uint16)
    pred_zxy = pred.permute(2, 0, 1).contiguous().numpy().astype(np.uint16)
    _IMAGES["gt.tif"], _IMAGES["pred.tif"] = gt_zxy, pred_zxy
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            sys.argv = ["skoots-validate", "--ground_truth", "gt.tif", "--predicted", "pred.tif"]
            open("gt.tif", "w").close()
            open("pred.tif", "w").close()
            ref_main.main()
            with open("pred_accuracy_stats.csv") as f:
                out["csv_accuracy"] = np.array(f.read())
            with open("pred_intersection_over_union.csv") as f:
                out["csv_iou"] = np.array(f.read())
        finally:
            os.chdir(cwd)
    out["csv_gt_zxy"], out["csv_pred_zxy"] = gt_zxy, pred_zxy
    gc, pc = gt[None, 50:-50, 50:-50, 5:-5].contiguous(), pred[None, 50:-50, 50:-50, 5:-5].contiguous()
    out["csv_dice"] = mask_dice(gc, pc).numpy()
    out["csv_cldice"] = mask_soft_cldice(gc, pc).numpy()
    from skoots.validate.lib import mask_iou
    out["csv_iou_matrix"] = mask_iou(gc, pc).numpy()
    ids = torch.unique(gc)
    out["csv_gt_ids"] = ids[ids > 0].numpy()
    save("validate_cldice.npz", **out)


if __name__ == "__main__":
    g13()
