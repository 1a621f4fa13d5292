"""``python -m skoots_amd.utils.resample FILE [FILE ...] (--factors FX FY FZ | --spacing SX SY SZ --to-spacing TX TY TZ |
--like OTHER) [--how auto|nearest|linear|area] [--labels] [--device D] [-o]``: bring volumes to another grid.

A SKOOTS model works in voxel units, so a volume acquired at another voxel size is rescaled before it is segmented
(``eval(..., rescale=)`` does that on the way), training pairs are brought to one voxel size

    python -m skoots_amd.utils.resample a.tif --spacing 0.1 0.1 0.5 --to-spacing 0.15 0.15 0.5
    python -m skoots_amd.utils.resample a.labels.tif --labels --like a_resampled.tif

and masks are made isotropic for viewing (``--labels --factors 1 1 3``).  The change of grid is
``lib.morphology.resample``: exact integer work, the same bits on the device and on the CPU.
Images (uint8, uint16) take ``--how``, by default linear on the axes that grow and area on those that shrink; with
``--labels`` every axis takes nearest and the ids stay what they are.  The reference has no tool for this.
"""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor


@dataclasses.dataclass
class ResampleReport:
    """What ``resample_file`` did to one file: shapes (X, Y, Z), the effective factors ``m / n``, the operator of every
    axis and, for labels, the ids before and after and how many ids of the input no longer occur in the output."""
    path: str = ""
    output: str = ""
    shape_in: Tuple[int, int, int] = (0, 0, 0)
    shape_out: Tuple[int, int, int] = (0, 0, 0)
    factors: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    operators: Tuple[str, str, str] = ("nearest", "nearest", "nearest")
    ids_in: Optional[int] = None
    ids_out: Optional[int] = None
    ids_lost: Optional[int] = None


def output_path(path: str, overwrite: bool = False) -> str:
    if overwrite:
        return path
    from .pyramid import _base_name
    where = os.path.dirname(os.path.normpath(path))
    return os.path.join(where, _base_name(path) + "_resampled.tif")


def as_labels(t: Tensor, path: str) -> Tensor:
    """A mask file's values in a dtype ``resample(how="nearest")`` takes"""
    if t.dtype in (torch.uint8, torch.int16, torch.int32, torch.uint16):
        return t
    raise TypeError(f"{path}: a mask of dtype {t.dtype} is not resampled: int32, int16, uint8 or uint16 ids only")


def target_shape(shape, factors=None, spacing=None, to_spacing=None, like_shape=None) -> Tuple[int, int, int]:
    """The (X, Y, Z) a volume of ``shape`` is brought to: by ``factors``, by ``spacing / to_spacing``, or ``like_shape``
    itself -- exactly one of the three."""
    from ..lib.morphology import resample_shape
    given = (factors is not None) + (spacing is not None or to_spacing is not None) + (like_shape is not None)
    if given != 1 or (spacing is None) != (to_spacing is None):
        raise ValueError("give exactly one of factors, spacing with to_spacing, and like")
    if like_shape is not None:
        return tuple(int(n) for n in like_shape)
    if factors is None:
        from .pyramid import check_spacing
        factors = tuple(s / t for s, t in zip(check_spacing(spacing), check_spacing(to_spacing)))
    return resample_shape(shape, factors)


def _wide(t: Tensor) -> Tensor:
    """int32 values of a label tensor, uint16 through its bit pattern"""
    return (t.view(torch.int16).to(torch.int32) & 0xFFFF) if t.dtype == torch.uint16 else t.to(torch.int32)


def count_ids(before: Tensor, after: Tensor) -> Tuple[int, int, int]:
    """(non-zero ids of ``before``, of ``after``, ids of ``before`` that ``after`` lacks)"""
    before, after = _wide(before), _wide(after)
    a, b = torch.unique(before[before != 0]), torch.unique(after[after != 0])
    return int(a.numel()), int(b.numel()), int((~torch.isin(a, b)).sum().item())


def resample_file(paths: Sequence[str], factors=None, spacing=None, to_spacing=None, like: Optional[str] = None,
                  how: str = "auto", labels: bool = False, device=None, overwrite: bool = False,
                  reports: Optional[List[ResampleReport]] = None) -> List[str]:
    """Resamples every file of ``paths`` (``.tif`` / ``.npy`` stored [Z, X, Y], or an (X, Y, Z) ``.zarr`` store: what
    ``utils.pyramid.load_volume`` opens) and writes ``<base>_resampled.tif`` next to it (the file itself with
    ``overwrite``, which only a ``.tif`` allows); returns the paths written.  ``labels``: nearest on every axis, through
    ``tiff.write_label_stack``; otherwise ``how`` and ``tiff.write_stack``.  ``reports``, if given, receives one
    ``ResampleReport`` per file.  Everything is checked before the first file is written."""
    from ..lib import tiff
    from ..lib.morphology import RESAMPLE_HOW, check_resample, resample
    from .pyramid import load_volume
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    if how not in RESAMPLE_HOW:
        raise ValueError(f"how = {how!r}, must be 'auto', 'nearest', 'linear' or 'area'")
    if labels and how not in ("auto", "nearest"):
        raise ValueError(f"labels are resampled by 'nearest', not by how={how!r}")
    for p in list(paths) + ([like] if like is not None else []):
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} does not exist")
    for p in paths:
        if overwrite and not str(p).lower().endswith((".tif", ".tiff")):
            raise ValueError(f"{p}: only a .tif can be written over")
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    like_shape = tuple(int(n) for n in load_volume(like, "cpu").shape) if like is not None else None
    how = "nearest" if labels else how
    jobs = []
    for p in paths:
        v = load_volume(p, dev)
        v = as_labels(v, p) if labels else v
        shape = target_shape(tuple(v.shape), factors, spacing, to_spacing, like_shape)
        _, ops = check_resample(v, shape, how, name=p)
        jobs.append((p, v, shape, ops))
    written = []
    for p, v, shape, ops in jobs:
        out = resample(v, shape=shape, how=how)
        path = output_path(p, overwrite)
        rep = ResampleReport(path=p, output=path, shape_in=tuple(int(n) for n in v.shape), shape_out=tuple(shape),
                             factors=tuple(m / n for n, m in zip(v.shape, shape)), operators=tuple(ops))
        if labels:
            rep.ids_in, rep.ids_out, rep.ids_lost = count_ids(v, out)
            tiff.write_label_stack(path, _wide(out).permute(2, 0, 1).contiguous())
        else:
            tiff.write_stack(path, out.permute(2, 0, 1).contiguous())
        written.append(path)
        if reports is not None:
            reports.append(rep)
    return written


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.resample",
                                     description="SKOOTS: bring images and masks to another voxel grid, exactly")
    parser.add_argument("files", type=str, nargs="+", metavar="FILE",
                        help="Volumes stored [Z, X, Y] (.tif, .npy) or (X, Y, Z) .zarr stores")
    parser.add_argument("--factors", type=float, nargs=3, default=None, metavar=("FX", "FY", "FZ"),
                        help="Output voxels per input voxel along x, y and z")
    parser.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing of the files; with --to-spacing the factors are spacing / target")
    parser.add_argument("--to-spacing", type=float, nargs=3, default=None, metavar=("TX", "TY", "TZ"),
                        help="Voxel spacing to bring the files to")
    parser.add_argument("--like", type=str, default=None, metavar="OTHER", help="Take the shape of this file")
    parser.add_argument("--how", choices=("auto", "nearest", "linear", "area"), default="auto",
                        help="Operator of every axis; auto: linear where an axis grows, area where it shrinks")
    parser.add_argument("--labels", action="store_true",
                        help="The files are masks (int32, int16, uint8, uint16): nearest on every axis, ids are kept")
    parser.add_argument("--device", type=str, default=None,
                        help="Where the volumes are resampled: cuda (default when there is one) or cpu")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the file")
    args = parser.parse_args(argv)
    given = (args.factors is not None) + (args.spacing is not None or args.to_spacing is not None) + (args.like is not None)
    if given != 1 or (args.spacing is None) != (args.to_spacing is None):
        parser.error("give exactly one of --factors, --spacing with --to-spacing, and --like")
    for name in ("factors", "spacing", "to_spacing"):
        value = getattr(args, name)
        if value is not None and not all(0 < v < float("inf") for v in value):
            parser.error(f"--{name.replace('_', '-')} must be three positive finite numbers")
    if args.labels and args.how not in ("auto", "nearest"):
        parser.error("--labels resamples by nearest; --how does not apply")
    return args


def main(argv=None) -> List[str]:
    """Runs the command; returns the paths written."""
    args = parse_args(argv)
    reports: List[ResampleReport] = []
    written = resample_file(args.files, factors=args.factors, spacing=args.spacing, to_spacing=args.to_spacing,
                            like=args.like, how=args.how, labels=args.labels, device=args.device,
                            overwrite=args.overwrite, reports=reports)
    for rep in reports:
        print(f"{rep.path}: shape (X, Y, Z) {rep.shape_in} -> {rep.shape_out}")
        print("factors: " + " ".join(f"{f:.6g}" for f in rep.factors))
        print("operators: " + " ".join(rep.operators))
        if rep.ids_in is not None:
            print(f"ids_in: {rep.ids_in}")
            print(f"ids_out: {rep.ids_out}")
            print(f"ids_lost: {rep.ids_lost}")
        print(f"File Written: {rep.output}", flush=True)
    return written


if __name__ == "__main__":
    main()
