#!/usr/bin/env python
"""Time ``label_components`` and ``clean`` on one synthetic (1024, 1024, 256) instance mask built on the device.

The mask: one ball per 32^3 cell of the volume (8192 cells; seeded centres and radii, ids a seeded permutation), plus
specks (stray voxels of the cell's id outside its ball) and pockets (zero voxels inside the balls), each at a seeded
rate.  Timed with device events after a warm-up, min / median / max over the repeats:

  ``id_rows``          the torch prologue every per-instance function shares (``x.max()``, ``torch.unique``, the table)
  ``label_pieces``     ``sk_label_components`` + ``sk_component_table`` alone, positive values, per connectivity
  ``label_background`` the same for the zero voxels
  ``label_components`` the library call (prologue + kernels)
  ``clean``            ``clean(components="split", min_voxels=..., fill_holes=True)``: two labellings, two look-ups

The bytes a pass must move are counted per voxel of 4-byte words: tiles 8 (labels in, parents out), borders 4 (labels;
the parents it touches are a small share), flatten 4, rank 4, write 8, table 8 -- 36 for one labelling with its table,
and 8 for a look-up.  The report gives those bytes over the median time beside the HBM rate the stage rooflines of this
project use (8.0 TB/s).  There is no pass or fail number: nothing comparable exists to set one against.

    python tools/bench_clean.py --out profiles/clean_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
LABEL_BYTES_PER_VOXEL = 36
LUT_BYTES_PER_VOXEL = 8
CELL = 32


def build_mask(shape, device, seed=11, speck_rate=2e-4, pocket_rate=2e-4):
    """(X, Y, Z) int32 on the device, slab by slab along x so that the temporaries stay small."""
    X, Y, Z = shape
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    cx, cy, cz = (-(-n // CELL) for n in shape)
    cells = cx * cy * cz
    centre = torch.rand((cells, 3), generator=g, device=device) * 8 + 12          # 12 .. 20 inside the cell
    radius = torch.rand(cells, generator=g, device=device) * 6 + 6                # 6 .. 12: the ball stays in its cell
    ids = (torch.randperm(cells, generator=g, device=device) + 1).to(torch.int32)
    out = torch.empty(shape, dtype=torch.int32, device=device)
    y = torch.arange(Y, device=device)[None, :, None]
    z = torch.arange(Z, device=device)[None, None, :]
    for x0 in range(0, X, CELL):
        x = torch.arange(x0, min(x0 + CELL, X), device=device)[:, None, None]
        cell = ((x // CELL) * cy + y // CELL) * cz + z // CELL
        c = centre[cell]
        d2 = (x % CELL - c[..., 0]) ** 2 + (y % CELL - c[..., 1]) ** 2 + (z % CELL - c[..., 2]) ** 2
        inside = d2 < radius[cell] ** 2
        u = torch.rand(inside.shape, generator=g, device=device)
        keep = (inside & (u >= pocket_rate)) | (~inside & (u < speck_rate))
        out[x0:x0 + CELL] = torch.where(keep, ids[cell], ids.new_zeros(()))
    return out, cells


def timed(fn, device):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(device))
    out = fn()
    b.record(torch.cuda.current_stream(device))
    b.synchronize()
    return out, a.elapsed_time(b) * 1e-3


def spread(times, nbytes=None):
    d = {"min_s": min(times), "median_s": statistics.median(times), "max_s": max(times), "all_s": times}
    if nbytes is not None:
        d["floor_bytes"] = nbytes
        d["floor_bytes_per_s_at_median"] = nbytes / d["median_s"]
        d["floor_fraction_of_hbm_peak"] = nbytes / d["median_s"] / HBM_PEAK
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-voxels", type=int, default=8)
    ap.add_argument("--connectivities", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clean needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd.lib.morphology import _label_pieces, label_components
    from skoots_amd.utils.clean import clean
    from skoots_amd.validate.lib import id_rows
    shape = tuple(args.shape)
    mask, cells = build_mask(shape, device)
    n = mask.numel()
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "cells": cells,
              "foreground_fraction": float((mask > 0).float().mean()), "repeats": args.repeats,
              "hbm_peak_bytes_per_s": HBM_PEAK, "label_bytes_per_voxel": LABEL_BYTES_PER_VOXEL,
              "lut_bytes_per_voxel": LUT_BYTES_PER_VOXEL}

    def series(fn, nbytes=None):
        fn()                                                             # warm-up: allocator, kernels loaded
        runs = []
        for _ in range(args.repeats):
            out, t = timed(fn, device)
            runs.append(t)
            del out
        return spread(runs, nbytes)

    report["id_rows"] = series(lambda: id_rows(mask))
    report["label_pieces"] = {str(k): series(lambda k=k: _label_pieces(mask, k, 1), LABEL_BYTES_PER_VOXEL * n)
                              for k in args.connectivities}
    report["label_background"] = series(lambda: _label_pieces(mask, 6, 0), LABEL_BYTES_PER_VOXEL * n)
    report["label_components"] = {str(k): series(lambda k=k: label_components(mask, k)) for k in args.connectivities}
    kwargs = dict(components="split", min_voxels=args.min_voxels, fill_holes=True)
    report["clean"] = series(lambda: clean(mask, **kwargs), (2 * LABEL_BYTES_PER_VOXEL + 2 * LUT_BYTES_PER_VOXEL) * n)
    report["clean"]["options"] = kwargs
    a, ra = clean(mask, **kwargs)
    b, rb = clean(mask, **kwargs)
    report["clean"]["report"] = vars(ra)
    report["clean"]["two_runs_identical"] = bool(torch.equal(a, b)) and ra == rb
    piece, table = label_components(mask, 6)
    report["pieces_at_6"] = int(table.shape[0])
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
