#!/usr/bin/env python
"""Time ``instance_contacts`` on synthetic instance masks built on the device, beside ``instance_sums`` on the same mask.

The masks are ``tools/bench_clean.py``'s: one ball per 32^3 cell (seeded centres and radii, ids a seeded permutation)
with specks and pockets, at (512, 512, 128) and at (1024, 1024, 256), 8192 balls.  The balls stay inside their cells, so
they meet each other only through specks; a third mask, the cells themselves (every voxel carries the id of its cell),
is the opposite case: every instance shares six flat walls with its neighbours.

Timed with device events after a warm-up, min / median / max over the repeats, the prologue (``id_rows``) computed
once outside the timed region:

  ``instance_sums``      the yardstick: existing code that also reads the mask once with a halo
  ``instance_contacts``  at connectivity 6 and 26, with and without background; the time holds the launch, the read-back
                         of the two counters, any retry at a larger table, and the sort of the rows

The report gives both times, their ratio and the number of pairs.  There is no pass or fail number.

    python tools/bench_contacts.py --out profiles/contacts_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_clean import CELL, build_mask, spread, timed  # noqa: E402


def cell_mask(shape, device):
    """(X, Y, Z) int32: every voxel carries the id of its 32^3 cell -- flat walls everywhere, no background"""
    X, Y, Z = shape
    cy, cz = -(-Y // CELL), -(-Z // CELL)
    x = torch.arange(X, device=device)[:, None, None] // CELL
    y = torch.arange(Y, device=device)[None, :, None] // CELL
    z = torch.arange(Z, device=device)[None, None, :] // CELL
    return ((x * cy + y) * cz + z + 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256),
                    help="X Y Z [X Y Z ...]")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_contacts needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd.validate.lib import id_rows, instance_contacts, instance_sums
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "masks": []}

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
        for kind in ("balls", "cells"):
            mask = build_mask(shape, device)[0] if kind == "balls" else cell_mask(shape, device)
            rows = id_rows(mask)
            entry = {"mask": kind, "shape": list(shape), "instances": int(rows[1][1].numel()),
                     "foreground_fraction": float((mask > 0).float().mean()),
                     "instance_sums": series(lambda: instance_sums(mask, rows)), "instance_contacts": {}}
            base = entry["instance_sums"]["median_s"]
            for connectivity in (6, 26):
                for background in (False, True):
                    d = series(lambda: instance_contacts(mask, connectivity, background, rows))
                    d["pairs"] = int(instance_contacts(mask, connectivity, background, rows)[1].shape[0])
                    d["ratio_to_instance_sums"] = d["median_s"] / base
                    entry["instance_contacts"][f"{connectivity}{'_background' if background else ''}"] = d
            report["masks"].append(entry)
            del mask, rows
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
