"""``python -m skoots_amd.utils.grow MASK.tif --distance D [--spacing SX SY SZ] [--within PATH] [--closed] [-o]``: move the
boundary of every instance of a mask by a physical distance.

``D > 0`` grows every instance without merging neighbours (what ``skimage.segmentation.expand_labels`` does): a
background voxel takes the id of the nearest instance when that lies within D (``lib.morphology.nearest_label``, the
exact nearest-instance transform of DESIGN.md section 27).  With ``--within`` only the voxels the other file allows are
given an id, which repairs the foreground that ``eval()`` left unassigned: the non-zero voxels of
``<base>_skoots_vectors.zarr`` are the gated foreground, so

    python -m skoots_amd.utils.grow I_instance_mask.tif --distance 3 --spacing 1 1 3 --within I_skoots_vectors.zarr

gives every orphan voxel within 3 units of an instance that instance's id.  ``D < 0`` shrinks every instance by |D|
without touching its neighbours (``lib.morphology.label_edt``).  The reference has no tool for either.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

# Whether the files are read on the device (tiff.read_stack, zarr_store.load_device) or on the host and uploaded.
READ_ON_DEVICE = False


@dataclasses.dataclass
class GrowReport:
    """What ``grow`` did, in Python ints: the positive ids before and after, the voxels that gained and lost an id,
    ``ids_removed`` the ids shrinking erased altogether and ``ids_grown`` the ids that gained at least one voxel."""
    instances_in: int = 0
    instances_out: int = 0
    voxels_added: int = 0
    voxels_removed: int = 0
    ids_removed: int = 0
    ids_grown: int = 0


def check_distance(distance) -> float:
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)):
        raise ValueError(f"distance must be a finite number, got {distance!r}")
    d = float(distance)
    if not math.isfinite(d):
        raise ValueError(f"distance must be a finite number, got {distance!r}")
    return d


def apply_grow(x: Tensor, nearest_id: Tensor, dist2: Tensor, limit2: float, within=None) -> Tensor:
    """The grow rule on tensors of one device: a zero voxel, inside ``within`` if given, takes ``nearest_id`` when
    ``dist2 <= limit2``; every other voxel keeps what it holds."""
    take = (x == 0) & (dist2 <= limit2)
    if within is not None:
        take &= within != 0
    return torch.where(take, nearest_id.to(x.dtype), x)


def apply_shrink(x: Tensor, edt_dist2: Tensor, limit2: float) -> Tensor:
    """The shrink rule: a voxel keeps its id iff its ``label_edt`` value exceeds ``limit2``."""
    return torch.where(edt_dist2 > limit2, x, torch.zeros_like(x))


def make_report(before: Tensor, after: Tensor) -> GrowReport:
    """Counts from integer reductions over the two volumes."""
    ids_in = torch.unique(before[before > 0])
    ids_out = torch.unique(after[after > 0])
    gained = (before == 0) & (after != 0)
    return GrowReport(instances_in=int(ids_in.numel()), instances_out=int(ids_out.numel()),
                      voxels_added=int(gained.sum().item()),
                      voxels_removed=int(((before != 0) & (after == 0)).sum().item()),
                      ids_removed=int((~torch.isin(ids_in, ids_out)).sum().item()),
                      ids_grown=int(torch.unique(after[gained & (after > 0)]).numel()))


def grow(mask: Tensor, distance, spacing=(1.0, 1.0, 1.0), within=None, closed: bool = False) -> Tuple[Tensor, GrowReport]:
    """Moves the boundary of every instance of a mask, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype,
    by ``distance`` in the units of ``spacing`` (sx, sy, sz): ``(mask_out (X, Y, Z), GrowReport)``, the output of the
    input's dtype and device.

    ``distance > 0`` grows: a zero voxel takes the id of the nearest instance when its squared distance to it is at most
    ``fl(d d)`` (``lib.morphology.nearest_label``, which also says which instance wins at equal distance).  Every
    non-zero voxel keeps its id, so no two instances merge and none changes its id.  ``within`` (bool or integer tensor
    of the volume's shape, non-zero = allowed) restricts which voxels may take an id; distances stay Euclidean, through
    anything: growth is not confined to a connected region.

    ``distance < 0`` shrinks by |d|: a voxel keeps its id iff ``label_edt(mask, spacing, closed)[0] > fl(d d)``, the
    squared distance to the nearest voxel that is not of its instance.  With ``closed=False`` a face of the volume does
    not erode an instance, with ``closed=True`` it does.  ``within`` is refused.

    ``distance == 0`` returns a copy.  All of it is exact: two runs give identical tensors and reports.  HIP kernels
    only, no CPU fallback."""
    d = check_distance(distance)
    if d < 0 and within is not None:
        raise ValueError("within restricts which voxels may take an id and has no meaning when shrinking (distance < 0)")
    from ..lib.morphology import label_edt, nearest_label
    from ..validate.lib import _as_volume, id_rows
    x = _as_volume(mask, "mask")
    if within is not None:
        if not isinstance(within, Tensor) or within.device != x.device:
            raise ValueError("within must be a tensor on the device of mask")
        within = within[0] if within.ndim == 4 and within.shape[0] == 1 else within
        if tuple(within.shape) != tuple(x.shape):
            raise ValueError(f"within must have the volume's shape {tuple(x.shape)}, got {tuple(within.shape)}")
    if x.numel() and int(x.min().item()) < 0:
        raise ValueError(f"mask holds the negative value {int(x.min().item())}: instance ids are positive and 0 is the "
                         "background")
    limit2 = d * d
    if d == 0 or x.numel() == 0:
        out = x.clone()
    elif d > 0:
        nearest_id, dist2 = nearest_label(x, spacing, abs(d), within, rows=id_rows(x))
        out = apply_grow(x, nearest_id, dist2, limit2, within)
    else:
        out = apply_shrink(x, label_edt(x, spacing, closed, rows=id_rows(x))[0], limit2)
    report = make_report(x, out)
    return out.to(mask.dtype), report


def output_path(mask_path: str, distance: float, overwrite: bool) -> str:
    if overwrite:
        return mask_path
    file, ext = os.path.splitext(mask_path)
    return file + ("_shrunk" if distance < 0 else "_grown") + ext


def load_within(path: str, device) -> Tensor:
    """(X, Y, Z) bool on ``device``: the allowed voxels of a TIFF mask stored [Z, X, Y] (non-zero), or of a
    ``*_skoots_vectors.zarr`` store (3, X, Y, Z) (any component non-zero: ``eval()`` stores ``vec * (prob > thr)``)."""
    if path.rstrip("/\\").endswith(".zarr"):
        from ..lib import zarr_store
        v = zarr_store.load_device(path, device) if READ_ON_DEVICE else torch.from_numpy(zarr_store.load(path)).to(device)
        if v.ndim != 4:
            raise ValueError(f"{path}: expected a (C, X, Y, Z) store, got shape {tuple(v.shape)}")
        return (v != 0).any(dim=0)
    from ..validate.__main__ import load_mask
    return load_mask(path, device if READ_ON_DEVICE else None)[0].to(device) != 0


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.grow",
                                     description="SKOOTS: grow (D > 0) or shrink (D < 0) every instance of a mask by a "
                                                 "physical distance, without merging neighbours")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif, stored [Z, X, Y])")
    parser.add_argument("--distance", type=float, required=True, metavar="D",
                        help="Distance in the units of --spacing: positive grows, negative shrinks")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--within", type=str, default=None, metavar="PATH",
                        help="Only voxels this file allows take an id: a .tif mask (non-zero) or a *_skoots_vectors.zarr "
                             "store of eval() (any component non-zero: the gated foreground)")
    parser.add_argument("--closed", action="store_true", help="When shrinking, the faces of the volume erode too")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the mask")
    args = parser.parse_args(argv)
    if not math.isfinite(args.distance):
        parser.error("--distance must be a finite number")
    if args.distance < 0 and args.within is not None:
        parser.error("--within has no meaning when shrinking (--distance < 0)")
    if not all(0 < v < float("inf") for v in args.spacing):
        parser.error("--spacing must be three positive finite numbers")
    args.spacing = tuple(args.spacing)
    return args


def main(argv=None) -> str:
    """Runs the command; returns the path written."""
    args = parse_args(argv)
    for path in (args.mask, args.within):
        if path is not None and not os.path.exists(path):
            raise FileNotFoundError(f"{path} does not exist")
    from ..lib import tiff
    from ..validate.__main__ import load_mask
    device = torch.device("cuda", torch.cuda.current_device())                # the HIP library: no CPU fallback
    mask = load_mask(args.mask, device if READ_ON_DEVICE else None)[0].to(device)          # (X, Y, Z) int32
    within = load_within(args.within, device) if args.within is not None else None
    out, report = grow(mask, args.distance, args.spacing, within, args.closed)
    path = output_path(args.mask, args.distance, args.overwrite)
    tiff.write_label_stack(path, out.permute(2, 0, 1).contiguous())
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value}")
    print(f"File Written: {path}", flush=True)
    return path


if __name__ == "__main__":
    main()
