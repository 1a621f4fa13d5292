"""Per-instance measurements of an instance mask, and ``python -m skoots_amd.validate.compare MASK``.

The reference sketches this step in ``skoots/validate/compare.py``: ``stats_per_instance`` forms one full-volume mask
per id and hands it to ``get_volume`` (which raises ``TypeError``) and to a marching-cubes ``get_surface_area``;
``compare()`` raises ``NotImplementedError``.  Here one kernel pass (``sk_instance_stats``) gives 13
integer sums and a box per instance, and ``derive`` turns them into volume, centroid, face area and the axes of the
ellipsoid with the same second moments.  Every kernel output is an integer, so the measurement is exact and the same
on every run.

There is no marching-cubes surface area: ``face_area`` is the area of the exposed voxel faces, which is exact for what
it defines and overestimates a curved surface.
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .lib import check_shape, instance_sums

CSV_COLUMNS = ("id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,"
               "axis_minor")

# An eigenvalue of the covariance matrix below this share of the largest one is the round-off of an exactly flat
# object (a line, a one-voxel-thick sheet) and is set to 0 together with negative round-off: 2 sqrt(5 lambda) would
# otherwise turn 1e-16 of noise into 1e-8 of axis.
FLAT_EIGENVALUE = 1e-12

_LOG_LEVELS = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]


def _spacing(spacing) -> Tuple[float, float, float]:
    if isinstance(spacing, Tensor):
        spacing = spacing.detach().cpu().tolist()
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(v > 0 for v in s):
        raise ValueError(f"spacing must be three positive numbers (x, y, z), got {spacing}")
    return s


def derive(sums: Tensor, boxes: Tensor, shape, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The derived columns of ``stats_per_instance`` from the kernel's (N, 13) int64 sums and (N, 6) int32 boxes of a
    mask of ``shape`` (X, Y, Z), in float64, on the tensors' own device (host tensors included; ``stats_per_instance``
    calls it on host copies).

    ``axis_lengths`` are ``2 sqrt(5 lambda_k)``, descending, of the eigenvalues of the covariance matrix of the voxel
    centres in physical units: the full axes of the solid ellipsoid with the same second moments.  The eigenvalues
    of the N 3 x 3 matrices are computed by LAPACK on the host (a few KiB either way)."""
    sx, sy, sz = _spacing(spacing)
    X, Y, Z = (int(v) for v in shape)
    sums = sums.to(torch.int64)
    boxes = boxes.to(torch.int32)
    dev = sums.device
    s = torch.tensor([sx, sy, sz], dtype=torch.float64, device=dev)
    f = sums.to(torch.float64)
    n = f[:, 0]
    mean = f[:, 1:4] / n[:, None]                                   # index units
    diag = f[:, 4:7] / n[:, None] - mean * mean
    off = f[:, 7:10] / n[:, None] - torch.stack((mean[:, 0] * mean[:, 1], mean[:, 0] * mean[:, 2],
                                                 mean[:, 1] * mean[:, 2]), dim=1)
    cov = torch.empty((sums.shape[0], 3, 3), dtype=torch.float64, device=dev)
    for i in range(3):
        cov[:, i, i] = diag[:, i]
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        cov[:, i, j] = cov[:, j, i] = off[:, k]
    cov = cov * (s[:, None] * s[None, :])
    cov[sums[:, 0] == 1] = 0.0                                      # a single voxel has no extent
    lam = torch.linalg.eigvalsh(cov.cpu()).flip(-1).to(dev) if cov.shape[0] else cov.new_empty((0, 3))
    lam = torch.where(lam > FLAT_EIGENVALUE * lam[:, :1], lam, torch.zeros_like(lam))
    faces = sums[:, 10:13]
    lim = torch.tensor([X - 1, Y - 1, Z - 1], dtype=torch.int32, device=dev)
    return {
        "voxels": sums[:, 0],
        "volume": n * (sx * sy * sz),
        "bbox": boxes,
        "touches_border": ((boxes[:, :3] == 0) | (boxes[:, 3:] == lim)).any(dim=1),
        "centroid": mean * s,
        "face_area": f[:, 10] * (sy * sz) + f[:, 11] * (sx * sz) + f[:, 12] * (sx * sy),
        "faces": faces,
        "axis_lengths": 2.0 * torch.sqrt(5.0 * lam),
    }


def stats_per_instance(x: Tensor, anisotropy=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """Measures every instance of ``x``, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype, in one kernel
    pass; ``anisotropy`` is the voxel spacing along x, y and z of that tensor.

    Returns device tensors with one row per positive id, ascending like ``torch.unique``: ``id`` int64, ``voxels``
    int64, ``volume`` float64, ``bbox`` (N, 6) int32 ``[x0, y0, z0, x1, y1, z1]`` inclusive, ``touches_border`` bool,
    ``centroid`` (N, 3) float64 in physical units, ``face_area`` float64, ``faces`` (N, 3) int64 exposed faces with
    their normal along x / y / z, ``axis_lengths`` (N, 3) float64 descending, and ``sums`` (N, 13) int64, the raw
    accumulators.  (The reference's sketch of the same name returns ``id``, ``volume`` and a marching-cubes
    ``surface_area`` and cannot run: skoots/validate/compare.py:8-28.)"""
    spacing = _spacing(anisotropy)
    ids, sums, boxes = instance_sums(x)
    shape = tuple(x.shape[-3:])
    out = {"id": ids}
    # N rows of a few numbers: derived on the host, where the eigenvalues are computed anyway, and uploaded -- the
    # same machine code as format_csv runs, so the file and this dict agree to the last bit
    out.update({k: v.to(sums.device) for k, v in derive(sums.cpu(), boxes.cpu(), shape, spacing).items()})
    out["sums"] = sums
    return out


def format_csv(mask_path: str, ids, sums: Tensor, boxes: Tensor, shape, spacing=(1.0, 1.0, 1.0),
               min_voxels: int = 1) -> str:
    """The text of ``_instance_stats.csv``: two header lines (file, spacing), the column names, and one row per
    instance with at least ``min_voxels`` voxels; floats are printed with ``repr``."""
    spacing = _spacing(spacing)
    d = {k: v.cpu().tolist() for k, v in derive(sums.cpu(), boxes.cpu(), shape, spacing).items()}
    ids = ids.cpu().tolist() if isinstance(ids, Tensor) else list(ids)
    lines = [f"Mask File: {mask_path}\n", "Spacing: {} {} {}\n".format(*(repr(v) for v in spacing)),
             CSV_COLUMNS + "\n"]
    for i, u in enumerate(ids):
        if d["voxels"][i] < min_voxels:
            continue
        cells = [int(u), d["voxels"][i], repr(d["volume"][i]), *d["bbox"][i], int(d["touches_border"][i]),
                 *(repr(v) for v in d["centroid"][i]), repr(d["face_area"][i]),
                 *(repr(v) for v in d["axis_lengths"][i])]
        lines.append(",".join(str(c) for c in cells) + "\n")
    return "".join(lines)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.validate.compare",
                                     description="SKOOTS: volume, box, centroid, face area and axes of every instance")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif or .npy, stored [Z, X, Y])")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--min-voxels", type=int, default=1, help="Leave out instances with fewer voxels")
    parser.add_argument("--out", type=str, default=None, help="Output file (default: <mask>_instance_stats.csv)")
    parser.add_argument("--log", type=int, default=3, choices=range(5),
                        help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    return parser.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> str:
    """Runs the command; returns the path of the CSV file.  The whole mask is measured: there is no border crop."""
    args = parse_args(argv)
    logging.basicConfig(level=_LOG_LEVELS[args.log],
                        format="[%(asctime)s] skoots-instance-stats [%(levelname)s]: %(message)s")
    if not os.path.exists(args.mask):
        raise RuntimeError(f"{args.mask} does not exist")
    spacing = _spacing(args.spacing)
    from .__main__ import load_mask
    mask = load_mask(args.mask)
    logging.debug(f"Mask Shape: {tuple(mask.shape)}")
    check_shape(mask.shape[-3:])
    ids, sums, boxes = instance_sums(mask.to("cuda"))       # the HIP library: no CPU fallback
    text = format_csv(args.mask, ids, sums, boxes, tuple(mask.shape[-3:]), spacing, args.min_voxels)
    out_path = args.out or f"{os.path.splitext(args.mask)[0]}_instance_stats.csv"
    with open(out_path, "w") as file:
        file.write(text)
    print(f"File Written: {out_path}")
    return out_path


if __name__ == "__main__":
    main()
