"""``python -m skoots_amd.utils.merge MASK.tif [--spacing SX SY SZ] [--connectivity 6|18|26] [--min-contact-area A]
[--min-contact-fraction F] [--pairs A B [A B ...]] [--renumber] [-o]``: join the ids of a mask that are one body.

``eval()`` labels voxel by voxel and the stitch of ``flood_and_stitch`` is greedy, so one object can come out under two
ids that share a long flat wall; ``utils.clean`` splits an id into its pieces and nothing joined two.  The reference
states the purpose in ``skoots/lib/merge.py`` (objects that carry two labels) and leaves it there.  ``merge`` reads the
table of touching pairs off the device (``validate.lib.instance_contacts``), decides on that small table on the host
(``plan_merge``: a pure function) and rewrites the volume with one table look-up.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Dict, Tuple

import numpy as np
import torch
from torch import Tensor

_INT32_MAX = 2 ** 31 - 1


@dataclasses.dataclass
class MergeReport:
    """What ``merge`` found and did, in Python ints.  ``pairs_touching`` counts the pairs of instances that touch at the
    connectivity and ``pairs_merged`` those of them that met the criteria; ``pairs_explicit`` the distinct pairs given
    as ``pairs`` and ``pairs_explicit_not_touching`` those of them that do not touch (they are joined all the same);
    ``groups`` the sets of two or more ids that became one; ``voxels_relabelled`` the voxels whose id changed."""
    instances_in: int = 0
    pairs_touching: int = 0
    pairs_merged: int = 0
    pairs_explicit: int = 0
    pairs_explicit_not_touching: int = 0
    groups: int = 0
    voxels_relabelled: int = 0
    instances_out: int = 0


def _criterion(value, name: str):
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(value)) or float(value) < 0:
        raise ValueError(f"{name} must be a finite number >= 0, got {value!r}")
    return float(value)


def _pairs(pairs) -> np.ndarray:
    p = np.asarray(list(pairs) if not isinstance(pairs, np.ndarray) else pairs)
    if p.size == 0:
        return np.zeros((0, 2), np.int64)
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pairs must be pairs of integer ids, got {pairs!r}")
    return p.astype(np.int64)


def _request(min_contact_area, min_contact_fraction, pairs):
    area_min = _criterion(min_contact_area, "min_contact_area")
    fraction_min = _criterion(min_contact_fraction, "min_contact_fraction")
    explicit = _pairs(pairs)
    if area_min is None and fraction_min is None and explicit.shape[0] == 0:
        raise ValueError("nothing to decide: give min_contact_area, min_contact_fraction or pairs")
    return area_min, fraction_min, explicit


def plan_merge(table, ids, face_area, spacing=(1.0, 1.0, 1.0), min_contact_area=None, min_contact_fraction=None,
               pairs=()) -> Tuple[np.ndarray, Dict[str, int]]:
    """Which ids become one, from the (P, 9) contact table with ids in its first two columns
    (``stats_per_instance(contacts=...)["contact_table"]``), the (N) ascending ``ids`` and their ``face_area``.  Pure:
    numpy or CPU torch in, numpy out.

    A touching pair merges when every criterion that is given holds: its face-contact area
    (``validate.compare.contact_area``) is >= ``min_contact_area``, and the larger of its two fractions -- that area over
    the face area of either side -- is >= ``min_contact_fraction``.  The larger one, because a small fragment glued to a
    large body covers much of its OWN surface with the wall and little of the body's.  Explicit ``pairs`` of ids merge
    unconditionally, touching or not; an id that is not in the mask raises ``ValueError``.  The criteria are evaluated
    once, on the table as given (the fractions of a merged group are not looked at again); merging is transitive
    (union-find), and a group takes its smallest id.  Without a criterion and without pairs there is nothing to decide
    and the function raises.

    Returns ``(lut, fields)``: ``lut`` (N + 1) int64 with ``lut[0] == 0`` and ``lut[k]`` the id that ``ids[k - 1]``
    carries afterwards, and every field of ``MergeReport`` except ``voxels_relabelled``."""
    from ..validate.compare import _contact_pairs
    area_min, fraction_min, explicit = _request(min_contact_area, min_contact_fraction, pairs)
    ids = np.asarray(ids.cpu() if isinstance(ids, Tensor) else ids, dtype=np.int64).reshape(-1)
    t, ia, ib, area, fa = _contact_pairs(table, ids, face_area, spacing)
    n = ids.size
    missing = sorted(set(explicit.reshape(-1).tolist()) - set(ids.tolist()))
    if missing:
        raise ValueError(f"pairs names the ids {missing}, which are not in the mask")
    if explicit.shape[0] and (explicit[:, 0] == explicit[:, 1]).any():
        raise ValueError("pairs names one id twice in a pair")
    explicit = np.unique(np.sort(explicit, axis=1), axis=0) if explicit.shape[0] else explicit
    chosen = np.zeros(t.shape[0], bool)
    if area_min is not None or fraction_min is not None:
        chosen[:] = True
        if area_min is not None:
            chosen &= area >= area_min
        if fraction_min is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                chosen &= np.maximum(area / fa[ia], area / fa[ib]) >= fraction_min
    parent = list(range(n))

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    ea, eb = np.searchsorted(ids, explicit[:, 0]), np.searchsorted(ids, explicit[:, 1])
    for a, b in zip(np.concatenate((ia[chosen], ea)).tolist(), np.concatenate((ib[chosen], eb)).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:                                         # ids ascend with their position: the smaller root stays
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(k) for k in range(n)], np.int64)
    lut = np.zeros(n + 1, np.int64)
    lut[1:] = ids[root] if n else ids
    touching = set(zip(t[:, 0].tolist(), t[:, 1].tolist()))
    members = np.bincount(root, minlength=n) if n else np.zeros(0, np.int64)
    fields = dict(instances_in=int(n), pairs_touching=int(t.shape[0]), pairs_merged=int(chosen.sum()),
                  pairs_explicit=int(explicit.shape[0]),
                  pairs_explicit_not_touching=sum((a, b) not in touching for a, b in explicit.tolist()),
                  groups=int((members > 1).sum()), instances_out=int((members > 0).sum()))
    return lut, fields


def merge(mask: Tensor, *, spacing=(1.0, 1.0, 1.0), connectivity: int = 6, min_contact_area=None,
          min_contact_fraction=None, pairs=(), renumber: bool = False) -> Tuple[Tensor, MergeReport]:
    """Joins ids of an instance mask, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype without negative
    values: ``(merged (X, Y, Z) int32, MergeReport)``.  The pairs of instances that touch at ``connectivity`` 6, 18 or 26
    come from one kernel pass (``validate.lib.instance_contacts``), ``plan_merge`` decides which of them -- and which
    explicit ``pairs`` of ids -- become one, and one table look-up per voxel rewrites the volume; a group takes its
    smallest id.  Only shared FACES have an area, whatever the connectivity: at 18 or 26 a pair that meets in edges or
    corners only is touching, has area 0 and merges under ``min_contact_area=0`` or as an explicit pair.
    ``renumber`` numbers the result 1..K by first appearance in C order (``renumber_first_seen``).

    Ids beyond int32 raise ``ValueError`` unless ``renumber`` is set, as in ``utils.clean``.  Every step is exact integer
    work on the device and a pure function of a small table on the host: two runs give identical tensors and reports.
    HIP kernels only, no CPU fallback."""
    from ..validate.compare import _spacing, derive
    from ..validate.lib import _Rows, _as_volume, check_shape, instance_contacts, instance_sums
    from .renumber import renumber_first_seen
    x = _as_volume(mask, "mask")
    check_shape(x.shape)
    spacing = _spacing(spacing)
    _request(min_contact_area, min_contact_fraction, pairs)                 # the argument checks
    m = _Rows(x, name="mask", nonnegative=True)           # x is a volume already: it passes through
    dev, a, ids, lut = m.dev, m.a, m.ids, m.lut
    if m.empty:
        if len(_pairs(pairs)):                                # ids that are not in the mask: raises
            plan_merge(np.zeros((0, 9), np.int64), np.zeros(0, np.int64), np.zeros(0), spacing, pairs=pairs)
        return torch.zeros(m.shape, dtype=torch.int32, device=dev), MergeReport()
    top = int(ids[-1].item())
    if top > _INT32_MAX and not renumber:
        raise ValueError(f"the mask holds the id {top}, beyond int32; pass renumber=True to number the result 1..K")
    _, table = instance_contacts(x, connectivity, False, m.pair)
    _, sums, boxes = instance_sums(x, m.pair)
    face_area = derive(sums.cpu(), boxes.cpu(), tuple(x.shape), spacing)["face_area"].numpy()
    ids_h = ids.cpu().numpy()
    t = table.cpu().numpy()
    t = np.concatenate((ids_h[t[:, :2] - 1], t[:, 2:]), 1)   # rows 1..N -> ids
    new_id, fields = plan_merge(t, ids_h, face_area, spacing, min_contact_area, min_contact_fraction, pairs)
    new_row = np.concatenate(([0], np.searchsorted(ids_h, new_id[1:]) + 1))          # the row of the id a row takes
    if renumber:                                             # ranks among the surviving ids: 1..K, in int32 whatever they were
        uniq = np.unique(new_id[1:])
        new_id = np.concatenate(([0], np.searchsorted(uniq, new_id[1:]) + 1))
    rows_now = torch.from_numpy(new_row.astype(np.int32)).to(dev)[lut.long()]        # value of `a` -> the row it takes
    changed = rows_now != lut
    fields["voxels_relabelled"] = int(changed[a].sum().item())
    out = torch.from_numpy(np.asarray(new_id, np.int64).astype(np.int32)).to(dev)[lut.long()][a]
    if renumber:
        out = renumber_first_seen(out, fields["instances_out"])
    return out, MergeReport(**fields)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.merge",
                                     description="SKOOTS: join the ids of a mask that are one body -- pairs of instances "
                                                 "whose shared wall is large, or pairs named outright.  A group takes its "
                                                 "smallest id.")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif, stored [Z, X, Y])")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--connectivity", type=int, default=6, choices=(6, 18, 26),
                        help="Neighbourhood in which two instances count as touching")
    parser.add_argument("--min-contact-area", type=float, default=None, metavar="A",
                        help="Merge a touching pair whose shared voxel faces have at least this area")
    parser.add_argument("--min-contact-fraction", type=float, default=None, metavar="F",
                        help="Merge a touching pair whose shared area is at least this share of the face area of one of "
                             "the two (the larger share counts); with --min-contact-area both must hold")
    parser.add_argument("--pairs", type=int, nargs="+", default=None, metavar="ID",
                        help="Merge these pairs of ids, A B [A B ...], whether they touch or not")
    parser.add_argument("--renumber", action="store_true", help="Number the result 1..K by first appearance")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the mask")
    args = parser.parse_args(argv)
    if args.pairs is not None and len(args.pairs) % 2:
        parser.error("--pairs takes an even number of ids: A B [A B ...]")
    args.pairs = tuple(zip(args.pairs[0::2], args.pairs[1::2])) if args.pairs else ()
    if args.min_contact_area is None and args.min_contact_fraction is None and not args.pairs:
        parser.error("nothing was asked for: give at least one of --min-contact-area, --min-contact-fraction, --pairs "
                     "(the file was not rewritten)")
    for name in ("min_contact_area", "min_contact_fraction"):
        v = getattr(args, name)
        if v is not None and not (math.isfinite(v) and v >= 0):
            parser.error(f"--{name.replace('_', '-')} must be a finite number >= 0")
    return args


def main(argv=None) -> str:
    """Runs the command; returns the path written."""
    args = parse_args(argv)
    if not os.path.exists(args.mask):
        raise FileNotFoundError(f"{args.mask} does not exist")
    from ..lib import tiff
    device = torch.device("cuda", torch.cuda.current_device())                # the HIP library: no CPU fallback
    stack = tiff.read_stack(args.mask, device)
    if stack.ndim != 3:
        raise ValueError(f"{args.mask}: expected a [Z, X, Y] stack, got shape {tuple(stack.shape)}")
    if stack.dtype in (torch.uint16, torch.uint32):
        stack = stack.to(torch.int64)     # torch moves and compares no wider unsigned types
    merged, report = merge(stack.permute(1, 2, 0).contiguous(), spacing=args.spacing, connectivity=args.connectivity,
                           min_contact_area=args.min_contact_area, min_contact_fraction=args.min_contact_fraction,
                           pairs=args.pairs, renumber=args.renumber)
    path = args.mask
    if not args.overwrite:
        file, ext = os.path.splitext(path)
        path = file + "_merged" + ext
    tiff.write_label_stack(path, merged.permute(2, 0, 1).contiguous())
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value}")
    print(f"File Written: {path}", flush=True)
    return path


if __name__ == "__main__":
    main()
