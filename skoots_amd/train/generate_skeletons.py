"""``skoots.train.generate_skeletons`` on the MI355X: the per-object training skeletons of an instance mask
(reference: skoots/train/generate_skeletons.py:65-157 ``calculate_skeletons``, :188-215 ``create_gt_skeletons``).

The reference thins one object at a time with scikit-image's Lee thinning on the CPU; here every object is thinned in
one HIP launch (``skoots_amd.lib.morphology.thin_objects``), bit for bit the same skeleton.  The reference's quirks
are kept:

1. the mask is resampled (nearest, through fp32) only when ``scale.sum() != 3``; ids that vanish or appear in the
   resample raise ``ValueError("Downscaled too much!")``;
2. each object's crop is ``[min, max)`` per axis (``max += 1`` where ``max == min``), so its voxels on the maximum
   plane of an axis are not thinned;
3. other objects inside the crop are background;
4. points are ``nonzero(skeleton).div(scale).add(lower.div(scale))`` in fp32, in raster order of the crop;
5. an object whose skeleton is empty gets one row, the mean of its crop's voxels: NaN when the crop holds none of
   them, and small pieces can thin away entirely (the re-check counts a lone voxel as simple).
"""
from __future__ import annotations

import glob
import logging
import os
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from ..lib.morphology import thin_objects

log = logging.getLogger(__name__)


def _object_boxes(large: Tensor) -> Tuple[Tensor, np.ndarray, np.ndarray]:
    """Sorted ids of ``large`` (0 excluded) and, per id, the min / max index along x, y, z (n, 3) int64.  Background
    voxels are left out before the scatter: all of them would contend for one slot."""
    fg = large != 0
    ids, inv = torch.unique(large[fg], sorted=True, return_inverse=True)
    coords = torch.nonzero(fg)   # the row-major order of large[fg]
    idx = inv.reshape(-1, 1).expand(-1, 3)
    k = ids.numel()
    lower = torch.full((k, 3), 2**62, dtype=torch.int64, device=large.device).scatter_reduce_(0, idx, coords, "amin")
    upper = torch.full((k, 3), -1, dtype=torch.int64, device=large.device).scatter_reduce_(0, idx, coords, "amax")
    return ids, lower.cpu().numpy(), upper.cpu().numpy()


def calculate_skeletons(mask: Tensor, scale) -> Dict[int, Tensor]:
    """Skeleton of every object of an instance mask (skoots/train/generate_skeletons.py:65-157).

    mask (X, Y, Z) integer ids (read on the GPU; a CPU tensor is copied there); scale: 3 factors (fp32), the
    resample factors of x, y, z.  Returns {id: (K, 3) fp32 voxel coordinates / scale} for every id > 0 in ascending
    order, on the GPU."""
    scale = torch.as_tensor(scale, dtype=torch.float32).reshape(-1).cpu()
    if scale.numel() != 3:
        raise ValueError("scale must hold 3 values")
    if mask.ndim != 3:
        raise ValueError(f"mask must be (X, Y, Z), not shape {tuple(mask.shape)}")
    dev = mask.device if mask.is_cuda else torch.device("cuda")
    if mask.dtype != torch.int32:
        if mask.numel() and (int(mask.max()) > 2**31 - 1 or int(mask.min()) < -2**31):
            raise ValueError("ids must fit in int32")
    m = mask.to(dev, torch.int32).contiguous()
    x, y, z = m.shape
    if scale.sum() != 3:
        size = torch.tensor([x, y, z]).mul(scale).float().round().int().tolist()
        large = F.interpolate(m[None, None].float(), size=size, mode="nearest")[0, 0].int().contiguous()
        if not torch.equal(torch.unique(m), torch.unique(large)):
            raise ValueError("Downscaled too much!")
    else:
        large = m
    ids, lower, upper = _object_boxes(large)
    log.info("found %d objects to skeletonize", ids.numel())
    extent = np.maximum(upper - lower, 1)   # upper[upper - lower == 0] += 1
    boxes = np.concatenate([lower, lower + extent], 1)
    points, counts, _ = thin_objects(large, ids.cpu().numpy(), boxes)

    # The points' fp32 arithmetic runs on the CPU, where the reference runs it, so every rounding is the reference's:
    # the device's mean is a sum times a rounded reciprocal, not a division (it differs by an ulp, e.g. 5 / 3).
    offset = torch.from_numpy(lower).div(scale)                     # lower.cpu().div(scale), per object
    skel = points.cpu().float().div(scale).add(offset.repeat_interleave(torch.from_numpy(counts), dim=0))
    skel = skel.to(dev)
    output = {}
    start = 0
    for i, obj in enumerate(ids.tolist()):
        c = int(counts[i])
        if c:
            output[obj] = skel[start:start + c]
        else:   # quirk 5: the mean of the crop's voxels (NaN for an empty crop)
            (x0, y0, z0), (x1, y1, z1) = boxes[i, :3], boxes[i, 3:]
            crop = (large[x0:x1, y0:y1, z0:z1] == obj).cpu()
            output[obj] = torch.nonzero(crop).float().mean(0).div(scale).add(offset[i]).unsqueeze(0).to(dev)
        start += c
    return output


def create_gt_skeletons(base_dir: str, mask_filter: str, scale: Tuple[float, float, float]) -> None:
    """Write ``<file>.skeletons.trch`` ({id: (K, 3) fp32 CPU tensor}) next to every ``base_dir/*{mask_filter}.tif``
    label stack, or next to ``base_dir`` itself when it is a file (skoots/train/generate_skeletons.py:188-215).
    Stacks are read as int32 (Z, X, Y) and permuted to (X, Y, Z)."""
    from ..lib.eval import _read_image
    if os.path.isdir(base_dir):
        files = glob.glob(os.path.join(base_dir, f"*{mask_filter}.tif"))
        print(f"found the following files in dir: {base_dir} with mask_filer: {mask_filter}:\n{files}")
    else:
        files = [base_dir]
        print(f"skeletonizing: {base_dir}")
    scale = torch.tensor(scale, dtype=torch.float32)
    for f in files:
        mask = torch.from_numpy(_read_image(f).astype(np.int32)).permute((1, 2, 0))
        output = calculate_skeletons(mask.to("cuda"), scale)
        for u in mask.unique().tolist():
            if u != 0 and u not in output:
                raise RuntimeError(f"{f}: no skeleton for id {u}")
        torch.save({k: v.cpu() for k, v in output.items()}, f + ".skeletons.trch")
        print("SAVED", f + ".skeletons.trch")
