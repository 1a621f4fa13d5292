"""``python -m skoots_amd.utils.equalize FILE [FILE ...] (--stretch LOW HIGH | --clahe TX TY TZ [--clip C] | --equalize |
--match REF.tif | --slices) [--bins N] [--no-interpolate] [--device D] [-o]``: grey-value transforms of image stacks,
exactly.

A network normalised with its training set's mean and deviation sees what it was trained on only if a new volume has
the training data's grey values.  Another session has another gain and offset, serial sections flicker from slice to
slice, thick stacks fade with depth:

    python -m skoots_amd.utils.equalize a.tif --stretch 0.5 99.5        # percentiles to 0 and the maximum
    python -m skoots_amd.utils.equalize a.tif --clahe 64 64 16 --clip 3  # contrast-limited adaptive equalisation, 3-D
    python -m skoots_amd.utils.equalize a.tif --equalize                # global histogram equalisation
    python -m skoots_amd.utils.equalize a.tif --match train_volume.tif  # the histogram of another volume
    python -m skoots_amd.utils.equalize a.tif --slices                  # every z-plane to the whole stack: no flicker

(``eval(..., equalize=)`` does the same on the way).  The transform is ``lib.morphology.equalize`` (DESIGN.md section
39): a histogram per tile, a table per tile, one pass through the tables of the tiles around every voxel -- exact integer
work, the same bits on the device and on the CPU.  The reference has no tool for this.
"""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import torch

OPERATORS = ("stretch", "clahe", "equalize", "match", "slices")


@dataclasses.dataclass
class EqualizeReport:
    """What ``equalize_file`` did to one file: shape (X, Y, Z), dtype, operator, the tile grid, bins and shift, the
    kernel paths ``lib.morphology.equalize_path`` names, for a stretch the ``lo`` / ``hi`` bins of every tile, for a
    match the number of tiles."""
    path: str = ""
    output: str = ""
    shape: Tuple[int, int, int] = (0, 0, 0)
    dtype: str = ""
    operator: str = ""
    grid: Tuple[int, int, int] = (1, 1, 1)
    sides: Tuple[int, int, int] = (0, 0, 0)
    bins: int = 256
    shift: int = 0
    kernel_paths: Tuple[str, str] = ("", "")
    lo: Optional[list] = None
    hi: Optional[list] = None
    tiles: Optional[int] = None


def output_path(path: str, overwrite: bool = False) -> str:
    if overwrite:
        return path
    from .pyramid import _base_name
    where = os.path.dirname(os.path.normpath(path))
    return os.path.join(where, _base_name(path) + "_equalized.tif")


def operator_arguments(operator: str, numbers=(), clip=3.0, reference=None, bins=None, interpolate=True) -> dict:
    """One of ``OPERATORS`` and what came with it as the keywords of ``lib.morphology.equalize``"""
    if operator not in OPERATORS:
        raise ValueError(f"operator = {operator!r}, must be one of {OPERATORS}")
    kwargs = {"stretch": lambda: dict(how="stretch", low=numbers[0], high=numbers[1]),
              "clahe": lambda: dict(how="equalize", tile=tuple(int(v) for v in numbers), clip=clip),
              "equalize": lambda: dict(how="equalize", clip=None),
              "match": lambda: dict(how="match", target=reference),
              "slices": lambda: dict(how="match", tile="slices")}[operator]()
    kwargs.update(bins=bins, interpolate=bool(interpolate))
    return kwargs


def equalize_file(paths: Sequence[str], operator: str, numbers=(), clip=3.0, reference=None, bins=None,
                  interpolate: bool = True, device=None, overwrite: bool = False,
                  reports: Optional[List[EqualizeReport]] = None) -> List[str]:
    """Transforms every file of ``paths`` (``.tif`` / ``.npy`` stored [Z, X, Y], or an (X, Y, Z) ``.zarr`` store: what
    ``utils.pyramid.load_volume`` opens) and writes ``<base>_equalized.tif`` next to it through ``tiff.write_stack`` (the
    file itself with ``overwrite``, which only a ``.tif`` allows); returns the paths written.  ``reports``, if given,
    receives one ``EqualizeReport`` per file.  Everything is checked before the first file is written."""
    from ..lib import tiff
    from ..lib.eval import equalize_arguments
    from ..lib.morphology import check_equalize, equalize
    from .pyramid import load_volume
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    kwargs = equalize_arguments(operator_arguments(operator, numbers, clip, reference, bins, interpolate))
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} does not exist")
        if overwrite and not str(p).lower().endswith((".tif", ".tiff")):
            raise ValueError(f"{p}: only a .tif can be written over")
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    if operator == "match":
        kwargs["target"] = load_volume(reference, dev)
    jobs = []
    for p in paths:
        v = load_volume(p, dev)
        if v.dtype.is_floating_point:
            raise TypeError(f"{p} is {v.dtype}: the integer samples of an image are transformed (uint8 / uint16), a float "
                            "image is not")
        shape, _ = check_equalize(v, name=p, **kwargs)
        jobs.append((p, v, shape))
    written = []
    for p, v, shape in jobs:
        found = {}
        out = equalize(v, report=found, **kwargs)
        path = output_path(p, overwrite)
        tiff.write_stack(path, out.permute(2, 0, 1).contiguous())
        written.append(path)
        if reports is not None:
            rep = EqualizeReport(path=p, output=path, shape=tuple(shape), dtype=str(v.dtype).replace("torch.", ""),
                                 operator=operator, grid=tuple(found["grid"]), sides=tuple(found["sides"]), bins=found["bins"],
                                 shift=found["shift"], kernel_paths=tuple(found["paths"]))
            if kwargs["how"] == "stretch":
                rep.lo, rep.hi = found["lo"].ravel().tolist(), found["hi"].ravel().tolist()
            if kwargs["how"] == "match":
                rep.tiles = int(found["grid"][0] * found["grid"][1] * found["grid"][2])
            reports.append(rep)
    return written


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.equalize",
                                     description="SKOOTS: percentile stretch, histogram equalisation (global and CLAHE) and "
                                                 "histogram matching of image stacks, exactly")
    parser.add_argument("files", type=str, nargs="+", metavar="FILE",
                        help="Volumes stored [Z, X, Y] (.tif, .npy) or (X, Y, Z) .zarr stores")
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--stretch", type=float, nargs=2, default=None, metavar=("LOW", "HIGH"),
                       help="Percentiles (nearest rank) that go to 0 and to the dtype's maximum")
    group.add_argument("--clahe", type=int, nargs=3, default=None, metavar=("TX", "TY", "TZ"),
                       help="Contrast-limited adaptive equalisation in tiles of that size (0: the whole axis)")
    group.add_argument("--equalize", action="store_true", help="Global histogram equalisation")
    group.add_argument("--match", type=str, default=None, metavar="REF.tif", help="Match the histogram of that volume")
    group.add_argument("--slices", action="store_true", help="Match every z-plane to the histogram of the whole stack")
    parser.add_argument("--clip", type=float, default=3.0, help="--clahe: the histogram is clipped at this multiple of its "
                                                                "mean bin height (default 3)")
    parser.add_argument("--bins", type=int, default=None, help="Bins of a uint16 volume: 256, 1024 (default) or 4096")
    parser.add_argument("--no-interpolate", action="store_true",
                        help="Every voxel through the table of its own tile only: tile edges show")
    parser.add_argument("--device", type=str, default=None,
                        help="Where the volumes are transformed: cuda (default when there is one) or cpu")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the file")
    args = parser.parse_args(argv)
    args.operator = "stretch" if args.stretch is not None else "clahe" if args.clahe is not None else \
        "equalize" if args.equalize else "match" if args.match is not None else "slices"
    args.numbers = tuple(args.stretch or args.clahe or ())
    from ..lib.eval import equalize_arguments
    try:
        equalize_arguments(operator_arguments(args.operator, args.numbers, args.clip, args.match, args.bins,
                                              not args.no_interpolate))
    except (ValueError, FileNotFoundError) as e:
        parser.error(str(e))
    return args


def main(argv=None) -> List[str]:
    """Runs the command; returns the paths written."""
    args = parse_args(argv)
    reports: List[EqualizeReport] = []
    written = equalize_file(args.files, args.operator, args.numbers, clip=args.clip, reference=args.match, bins=args.bins,
                            interpolate=not args.no_interpolate, device=args.device, overwrite=args.overwrite, reports=reports)
    for rep in reports:
        print(f"{rep.path}: shape (X, Y, Z) {rep.shape}, dtype {rep.dtype}")
        print(f"operator: {rep.operator}")
        print("tile grid: " + " x ".join(str(n) for n in rep.grid) + " tiles of " + " x ".join(str(n) for n in rep.sides))
        print(f"bins: {rep.bins}, shift {rep.shift}")
        print("kernel paths: histograms " + rep.kernel_paths[0] + ", apply " + rep.kernel_paths[1])
        if rep.lo is not None:
            few = len(rep.lo) <= 8
            print("lo: " + (" ".join(str(v) for v in rep.lo) if few else f"{min(rep.lo)} .. {max(rep.lo)} over {len(rep.lo)} tiles"))
            print("hi: " + (" ".join(str(v) for v in rep.hi) if few else f"{min(rep.hi)} .. {max(rep.hi)} over {len(rep.hi)} tiles"))
        if rep.tiles is not None:
            print(f"tiles matched: {rep.tiles}")
        print(f"File Written: {rep.output}", flush=True)
    return written


if __name__ == "__main__":
    main()
