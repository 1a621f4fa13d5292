"""``python -m skoots_amd.utils.filter FILE [FILE ...] (--median RX RY RZ | --mean RX RY RZ | --min RX RY RZ |
--max RX RY RZ | --gauss SX SY SZ) [--border zero|edge|mirror] [--device D] [-o]``: denoise image stacks, exactly.

EM and confocal stacks are noisy, and what is done to them before a network sees them is a small median, which removes
shot noise and hot pixels -- 3 x 3 x 1 or 3 x 3 x 3, because z is coarser -- or a light Gaussian:

    python -m skoots_amd.utils.filter a.tif --median 1 1 0
    python -m skoots_amd.utils.filter a.tif --gauss 1 1 0.5 --border edge

(``eval(..., denoise=)`` does the same on the way).  The filter is ``lib.morphology.filter_volume`` (DESIGN.md section
38): exact integer work, the same bits on the device and on the CPU.  Radii are voxels along x, y, z, up to 2 for
``--median``, ``--min`` and ``--max`` and up to 8 for ``--mean``; sigmas are voxels too.  The reference has no tool for
this.
"""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import torch

OPERATORS = ("median", "mean", "min", "max", "gauss")


@dataclasses.dataclass
class FilterReport:
    """What ``filter_file`` did to one file: shape (X, Y, Z), dtype, operator, the window (rank filters) or the taps
    (tap filters) of every axis, the border and the kernel path ``lib.morphology.filter_path`` names."""
    path: str = ""
    output: str = ""
    shape: Tuple[int, int, int] = (0, 0, 0)
    dtype: str = ""
    operator: str = ""
    border: str = "mirror"
    window: Optional[Tuple[int, int, int]] = None
    taps: Optional[Tuple[List[int], List[int], List[int]]] = None
    kernel_path: Tuple[str, str] = ("", "")


def output_path(path: str, overwrite: bool = False) -> str:
    if overwrite:
        return path
    from .pyramid import _base_name
    where = os.path.dirname(os.path.normpath(path))
    return os.path.join(where, _base_name(path) + "_filtered.tif")


def filter_file(paths: Sequence[str], how: str, numbers, border: str = "mirror", device=None, overwrite: bool = False,
                reports: Optional[List[FilterReport]] = None) -> List[str]:
    """Filters every file of ``paths`` (``.tif`` / ``.npy`` stored [Z, X, Y], or an (X, Y, Z) ``.zarr`` store: what
    ``utils.pyramid.load_volume`` opens) and writes ``<base>_filtered.tif`` next to it through ``tiff.write_stack`` (the
    file itself with ``overwrite``, which only a ``.tif`` allows); returns the paths written.  ``how`` is one of
    ``OPERATORS`` and ``numbers`` its three radii, or sigmas for ``"gauss"``.  ``reports``, if given, receives one
    ``FilterReport`` per file.  Everything is checked before the first file is written."""
    from ..lib import tiff
    from ..lib.eval import denoise_arguments
    from ..lib.morphology import check_filter, filter_path, filter_volume
    from .pyramid import load_volume
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    kwargs = denoise_arguments((how, numbers))
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} does not exist")
        if overwrite and not str(p).lower().endswith((".tif", ".tiff")):
            raise ValueError(f"{p}: only a .tif can be written over")
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    jobs = []
    for p in paths:
        v = load_volume(p, dev)
        if v.dtype.is_floating_point:
            raise TypeError(f"{p} is {v.dtype}: the integer samples of an image are filtered (uint8 / uint16), a float image "
                            "is not")
        shape, plan = check_filter(v, border=border, name=p, **kwargs)
        jobs.append((p, v, shape, plan))
    written = []
    for p, v, shape, plan in jobs:
        out = filter_volume(v, border=border, **kwargs)
        path = output_path(p, overwrite)
        tiff.write_stack(path, out.permute(2, 0, 1).contiguous())
        written.append(path)
        if reports is not None:
            rep = FilterReport(path=p, output=path, shape=tuple(shape), dtype=str(v.dtype).replace("torch.", ""), operator=how,
                               border=border, kernel_path=filter_path(v.dtype, shape, aligned=v.data_ptr() % 4 == 0, **kwargs))
            if plan[0] == "rank":
                rep.window = tuple(2 * r + 1 for r in plan[1])
            else:
                rep.taps = tuple(list(t) for t in plan[1])
            reports.append(rep)
    return written


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.filter",
                                     description="SKOOTS: median, mean, min, max and Gaussian filters of image stacks, exactly")
    parser.add_argument("files", type=str, nargs="+", metavar="FILE",
                        help="Volumes stored [Z, X, Y] (.tif, .npy) or (X, Y, Z) .zarr stores")
    group = parser.add_mutually_exclusive_group(required=True)
    for name, limit in (("median", 2), ("mean", 8), ("min", 2), ("max", 2)):
        group.add_argument("--" + name, type=int, nargs=3, default=None, metavar=("RX", "RY", "RZ"),
                           help=f"Radii of the {name} window along x, y and z, each 0 .. {limit}")
    group.add_argument("--gauss", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"),
                       help="Sigmas of the Gaussian along x, y and z in voxels (integer taps that sum to 256 per axis)")
    parser.add_argument("--border", choices=("zero", "edge", "mirror"), default="mirror",
                        help="What a window reads beyond the volume: zeros, the edge sample, or the volume mirrored")
    parser.add_argument("--device", type=str, default=None,
                        help="Where the volumes are filtered: cuda (default when there is one) or cpu")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the file")
    args = parser.parse_args(argv)
    args.how = next(name for name in OPERATORS if getattr(args, name) is not None)
    args.numbers = tuple(getattr(args, args.how))
    from ..lib.eval import denoise_arguments
    try:
        denoise_arguments((args.how, args.numbers))
    except ValueError as e:
        parser.error(str(e))
    return args


def main(argv=None) -> List[str]:
    """Runs the command; returns the paths written."""
    args = parse_args(argv)
    reports: List[FilterReport] = []
    written = filter_file(args.files, args.how, args.numbers, border=args.border, device=args.device,
                          overwrite=args.overwrite, reports=reports)
    for rep in reports:
        print(f"{rep.path}: shape (X, Y, Z) {rep.shape}, dtype {rep.dtype}")
        print(f"operator: {rep.operator}, border {rep.border}")
        if rep.window is not None:
            print("window: " + " x ".join(str(n) for n in rep.window))
        else:
            for axis, t in zip("xyz", rep.taps):
                print(f"taps {axis}: " + " ".join(str(w) for w in t))
        print("kernel path: " + " + ".join(rep.kernel_path))
        print(f"File Written: {rep.output}", flush=True)
    return written


if __name__ == "__main__":
    main()
