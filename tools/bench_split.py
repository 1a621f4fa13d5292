#!/usr/bin/env python
"""Time ``geodesic_assign`` and ``split`` on synthetic instance masks built on the device, beside ``label_components``
on the same mask.

The masks are those of ``tools/bench_clean.py`` without the specks and pockets: one ball per 32^3 cell (seeded centres
and radii), at (512, 512, 128) -- about 1 000 blobs -- and at (1024, 1024, 256), 8192 balls.  The cells are paired along
z, and a seeded half of the pairs is fused: a neck of radius 2.25 voxels joins the two centres and both balls carry one
id, so that there is something to split at ``--radius`` 4.

Timed with device events after a warm-up, min / median / max over the repeats:

  ``label_pieces``      the yardstick: ``sk_label_components`` + ``sk_component_table`` at connectivity 6, one pass of the
                        same 4 x 8 x 64 tile scheme
  ``geodesic_assign``   alone, on the seed volume ``split`` makes, the prologue (``id_rows``) computed once outside the
                        timed region; the time holds the init, the rounds in their batches with one read-back per batch,
                        and the finish
  ``split``             the whole call: prologue, distance transform, labelling of the cores, plan, seeds, assignment

The report gives the rounds that changed a key, the rounds launched, the time of ``geodesic_assign`` per launched round
over the time of the yardstick, and the extent of the largest instance in tiles, which is what the rounds should follow.
There is no pass or fail number.

    python tools/bench_split.py --out profiles/split_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_clean import CELL, spread, timed  # noqa: E402

NECK = 2.25


def build_fused_mask(shape, device, seed=11, fused_share=0.5):
    """((X, Y, Z) int32 on the device, cells, fused pairs), slab by slab along x so that the temporaries stay small."""
    X, Y, Z = shape
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    cx, cy, cz = (-(-n // CELL) for n in shape)
    cells = cx * cy * cz
    centre = torch.rand((cells, 3), generator=g, device=device) * 8 + 12          # 12 .. 20 inside the cell
    radius = torch.rand(cells, generator=g, device=device) * 6 + 6                # 6 .. 12: the ball stays in its cell
    ids = (torch.randperm(cells, generator=g, device=device) + 1).to(torch.int32)
    index = torch.arange(cells, device=device)
    zc = index % cz
    first = index - (zc % 2)                                                      # the even cell of the pair along z
    has_pair = (first + 1) // cz == first // cz                                   # the odd one exists
    fused = has_pair & (torch.rand(cells, generator=g, device=device)[first] < fused_share)
    ids = torch.where(fused, ids[first], ids)
    origin = torch.stack(((index // (cy * cz)) * CELL, ((index // cz) % cy) * CELL, zc * CELL), 1).float()
    a = (centre + origin)[first]                                                  # the segment between the two centres
    b = (centre + origin)[torch.clamp(first + 1, max=cells - 1)]
    out = torch.empty(shape, dtype=torch.int32, device=device)
    y = torch.arange(Y, device=device)[None, :, None]
    z = torch.arange(Z, device=device)[None, None, :]
    for x0 in range(0, X, CELL):
        x = torch.arange(x0, min(x0 + CELL, X), device=device)[:, None, None]
        cell = ((x // CELL) * cy + y // CELL) * cz + z // CELL
        c = centre[cell]
        d2 = (x % CELL - c[..., 0]) ** 2 + (y % CELL - c[..., 1]) ** 2 + (z % CELL - c[..., 2]) ** 2
        inside = d2 < radius[cell] ** 2
        p = torch.stack(torch.broadcast_tensors(x, y, z), -1).float()
        ab = b[cell] - a[cell]
        t = (((p - a[cell]) * ab).sum(-1) / (ab * ab).sum(-1).clamp(min=1.0)).clamp(0.0, 1.0)
        neck = ((p - a[cell] - t[..., None] * ab) ** 2).sum(-1) < NECK * NECK
        out[x0:x0 + CELL] = torch.where(inside | (neck & fused[cell]), ids[cell], ids.new_zeros(()))
    return out, cells, int(fused.sum().item()) // 2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256),
                    help="X Y Z [X Y Z ...]")
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_split needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd.lib.morphology import GEODESIC_TILE, _label_pieces, geodesic_assign
    from skoots_amd.utils.clean import _apply
    from skoots_amd.utils.split import core_pieces, plan_split, split
    from skoots_amd.validate.lib import id_rows, instance_sums
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "radius": args.radius,
              "tile": list(GEODESIC_TILE), "masks": []}

    def series(fn):
        fn()                                                             # warm-up: allocator, kernels loaded
        runs = []
        for _ in range(args.repeats):
            out, t = timed(fn, device)
            runs.append(t)
            del out
        return spread(runs)

    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]
    for shape in shapes:
        mask, cells, pairs = build_fused_mask(shape, device)
        rows = id_rows(mask)
        ids, _, boxes = instance_sums(mask, rows)
        extent = (boxes[:, 3:] - boxes[:, :3] + 1).cpu()
        tiles = torch.stack([-(-extent[:, k] // GEODESIC_TILE[k]) for k in range(3)], 1)
        piece, table = core_pieces(mask, args.radius, rows=rows)
        lut, fields = plan_split(table, ids, int(ids[-1].item()))
        seeds = torch.zeros(shape, dtype=torch.int32, device=device)
        _apply(piece, lut, seeds, False)
        stats = {}
        geodesic_assign(mask, seeds, rows=rows, stats=stats)
        entry = {"shape": list(shape), "cells": cells, "fused_pairs": pairs, "instances": int(ids.numel()),
                 "foreground_fraction": float((mask > 0).float().mean()), "plan": fields,
                 "largest_instance_extent_in_tiles": [int(v) for v in tiles.max(0).values],
                 "rounds": stats["rounds"], "launched": stats["launched"], "tiles": stats["tiles"],
                 "label_pieces": series(lambda: _label_pieces(mask, 6, 1)),
                 "geodesic_assign": series(lambda: geodesic_assign(mask, seeds, rows=rows)),
                 "split": series(lambda: split(mask, args.radius))}
        a, ra = split(mask, args.radius)
        b, rb = split(mask, args.radius)
        entry["split"]["report"] = vars(ra)
        entry["split"]["two_runs_identical"] = bool(torch.equal(a, b)) and ra == rb
        base = entry["label_pieces"]["median_s"]
        entry["geodesic_per_launched_round_over_label_pieces"] = entry["geodesic_assign"]["median_s"] / stats["launched"] / base
        entry["split_over_label_pieces"] = entry["split"]["median_s"] / base
        report["masks"].append(entry)
        del mask, rows, piece, table, seeds, a, b
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
