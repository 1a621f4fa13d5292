"""``python -m skoots_amd.utils.split MASK.tif --radius R [--spacing SX SY SZ] [--closed] [--min-seed-voxels N]
[--costs CX CY CZ] [--ids ID ...] [--renumber] [-o]``: cut the instances of a mask at their necks.

Two objects that came out under one id and still hang together through a neck are the under-segmentation the method
exists to reduce; ``utils.clean`` splits an id into its connected pieces, ``utils.merge`` joins two ids, ``utils.grow``
moves boundaries, and nothing separated these.  ``split`` finds the cores of every instance -- the pieces that remain of
it at depth ``radius`` (``lib.morphology.label_edt``, ``label_components``) -- decides on the small table of cores on
the host (``plan_split``: a pure function) and hands every remaining voxel of a split instance to the core that is
nearest along paths inside the instance (``lib.morphology.geodesic_assign``), so that every id stays one body
(DESIGN.md section 33).  The reference has no counterpart.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

_INT32_MAX = 2 ** 31 - 1


@dataclasses.dataclass
class SplitReport:
    """What ``split`` found and did, in Python ints.  ``cores_found`` counts the cores of all ids at the radius and
    ``cores_dropped`` those of them below ``min_seed_voxels``; ``instances_split`` the ids that were cut (two or more
    cores left, and named by ``ids`` when that is given); ``instances_out`` = ``instances_in`` + the new ids;
    ``voxels_relabelled`` the voxels whose id changed; ``rounds`` the rounds of ``geodesic_assign`` that changed a key
    (0 when nothing was split)."""
    instances_in: int = 0
    instances_split: int = 0
    cores_found: int = 0
    cores_dropped: int = 0
    instances_out: int = 0
    voxels_relabelled: int = 0
    rounds: int = 0


def _radius2(radius) -> float:
    """The threshold on ``label_edt``'s squared distances: ``fl(r r)``, the rounding of ``max_distance_squared``."""
    from ..lib.morphology import max_distance_squared
    if radius is None:
        raise ValueError("radius must be a non-negative finite number, got None")
    try:
        return max_distance_squared(radius)
    except ValueError:
        raise ValueError(f"radius must be a non-negative finite number, got {radius!r}") from None


def _min_seed_voxels(value) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"min_seed_voxels must be a positive integer, got {value!r}")
    return int(value)


def _only_ids(ids) -> Optional[np.ndarray]:
    if ids is None:
        return None
    a = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.dtype.kind not in "iu" or a.ndim != 1 or (a <= 0).any():
        raise ValueError(f"ids must be positive integer ids, got {ids!r}")
    return np.unique(a.astype(np.int64))


def split_costs(costs, spacing) -> Tuple[int, int, int]:
    """The step costs of ``split``: ``costs`` when given, else the spacing when its three values are integers."""
    from ..lib.morphology import geodesic_costs
    if costs is not None:
        return geodesic_costs(costs)
    s = tuple(float(v) for v in spacing)
    if not all(v == int(v) and 1 <= v <= 255 for v in s):
        raise ValueError(f"the spacing {spacing} is not three integers in 1..255: pass costs=(cx, cy, cz), the integer "
                         "step costs along x, y and z in the same proportion")
    return tuple(int(v) for v in s)


def plan_split(table, ids, max_id: int, min_seed_voxels: int = 1, only_ids=None,
               renumber: bool = False) -> Tuple[np.ndarray, Dict[str, int]]:
    """Which cores become seeds and under which id, from the table of ``label_components`` on the cores ((P, 6): value,
    voxels, first_voxel, ...; core p is row p - 1) and the (N) ``ids`` of the mask.  Pure: numpy or CPU torch in, numpy
    out.

    A core with fewer than ``min_seed_voxels`` voxels is dropped.  An id with fewer than two cores left, or not in
    ``only_ids`` when that is given, is not touched: none of its cores becomes a seed.  Otherwise its cores are ordered
    by voxels descending, then first voxel ascending; the first keeps the id and the others take ``max_id + 1,
    max_id + 2, ...``, handed out over the ids ascending and within an id in that order.  An id beyond int32 raises
    ``ValueError`` unless ``renumber`` says that the caller compacts the ids anyway; so does an id in ``only_ids`` that
    the mask does not hold.

    Returns ``(lut, fields)``: ``lut`` (P + 1) int64 with ``lut[0] == 0``, the seed value core p carries or 0, and the
    fields of ``SplitReport`` but ``voxels_relabelled`` and ``rounds``."""
    from .clean import _table
    min_seed_voxels = _min_seed_voxels(min_seed_voxels)
    only = _only_ids(only_ids)
    ids = np.asarray(ids.cpu() if isinstance(ids, Tensor) else ids, dtype=np.int64).reshape(-1)
    t = _table(table)
    P = t.shape[0]
    value, voxels, first = t[:, 0], t[:, 1], t[:, 2]
    if P and (value <= 0).any():
        raise ValueError("plan_split takes the table of the positive values (label_components(background=False))")
    if only is not None:
        missing = sorted(set(only.tolist()) - set(ids.tolist()))
        if missing:
            raise ValueError(f"ids names {missing}, which are not in the mask")
    kept = voxels >= min_seed_voxels
    if only is not None:
        kept &= np.isin(value, only)
    dropped = int((voxels < min_seed_voxels).sum())
    order = np.lexsort((first, -voxels, value))              # by id, then voxels descending, then first voxel
    order = order[kept[order]]
    v = value[order]
    head = np.concatenate(([True], v[1:] != v[:-1])) if v.size else np.zeros(0, bool)
    count = np.diff(np.concatenate((np.flatnonzero(head), [v.size]))) if v.size else np.zeros(0, np.int64)
    several = np.repeat(count >= 2, count)                   # per core: its id has two or more cores left
    order, head = order[several], head[several]
    lut = np.zeros(P + 1, np.int64)
    extra = int((~head).sum())
    seed = value[order].copy()
    seed[~head] = int(max_id) + 1 + np.arange(extra, dtype=np.int64)
    top = int(seed.max()) if seed.size else 0
    if top > _INT32_MAX and not renumber:
        raise ValueError(f"the ids would reach {top}, beyond int32: {extra} cores need new ids above the largest id "
                         f"{int(max_id)}; pass renumber=True to number the result 1..K")
    lut[order + 1] = seed
    fields = dict(instances_in=int(ids.size), instances_split=int(head.sum()), cores_found=int(P), cores_dropped=dropped,
                  instances_out=int(ids.size) + extra)
    return lut, fields


def core_pieces(mask: Tensor, radius, spacing=(1.0, 1.0, 1.0), closed: bool = False, rows=None) -> Tuple[Tensor, Tensor]:
    """Steps 1 to 3 of ``split``: ``(piece_map (X, Y, Z) int32, table (P, 6) int64)`` of ``label_components`` at
    connectivity 6 on the mask with every voxel at depth ``<= radius`` set to 0 -- the cores of every instance.  A voxel
    is a core voxel when ``label_edt``'s squared distance exceeds ``fl(radius radius)``."""
    from ..lib.morphology import check_piece_shape, label_components, label_edt
    from ..validate.lib import _Rows
    limit2 = _radius2(radius)
    m = _Rows(mask, rows, check_piece_shape, "mask", nonnegative=True)
    d2, _ = label_edt(m.x, spacing, closed, m.pair)
    cores = torch.where(d2 > limit2, m.x, m.x.new_zeros(()))
    return label_components(cores, 6)


def split(mask: Tensor, radius, spacing=(1, 1, 1), closed: bool = False, min_seed_voxels: int = 1, costs=None, ids=None,
          renumber: bool = False) -> Tuple[Tensor, SplitReport]:
    """Cuts the instances of a mask, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype without negative
    values, at their necks: ``(mask_out (X, Y, Z) int32, SplitReport)``.  The steps, in this order:

    1. ``label_edt(mask, spacing, closed)``: the exact depth of every voxel inside its instance.
    2. The core voxels are those deeper than ``radius`` (squared distance above ``fl(radius radius)``).
    3. ``label_components`` at connectivity 6 on the mask with everything else set to 0: the cores and their table.
    4. ``plan_split`` decides: cores below ``min_seed_voxels`` voxels are dropped; an id with fewer than two cores left,
       or not named by ``ids`` when that is given, is not touched; otherwise the largest core keeps the id and the others
       take new ids above the largest id of the mask.
    5. One table look-up turns the core map into the seed volume.
    6. ``geodesic_assign(mask, seeds, costs)`` hands every voxel of a split instance to the core that is nearest along
       paths inside the instance.  ``costs=None`` takes the spacing when its three values are integers and raises
       ``ValueError`` otherwise: pass integer ``costs`` in the proportion of the spacing then.
    7. The output holds the owner where there is one and the mask elsewhere.
    8. ``renumber`` numbers the result 1..K by first appearance in C order (``renumber_first_seen``), as in ``clean``.

    A neck thinner than ``2 radius`` between bodies thicker than that is cut near its middle along the paths; choose
    ``radius`` between the neck's and the bodies' half-widths (``stats_per_instance(cores=radius)`` counts the cores of
    every id before anything is changed).  Every id of the result that came from a connected id is one 6-connected
    body.  A disconnected piece of a split id that holds no core is reached by no seed and keeps the old id: run
    ``clean`` first.  Ids beyond int32 -- in the mask, or made here -- raise ``ValueError`` unless ``renumber`` is set.
    Every step is exact: two runs give identical tensors and reports.  HIP kernels only, no CPU fallback."""
    from ..lib.morphology import check_piece_shape, geodesic_assign
    from ..validate.lib import _Rows, _as_volume
    from .clean import _apply
    from .renumber import renumber_first_seen
    x = _as_volume(mask, "mask")
    check_piece_shape(x.shape)
    _radius2(radius)
    step = split_costs(costs, spacing)
    plan_split(np.zeros((0, 6), np.int64), np.zeros(0, np.int64), 0, min_seed_voxels, None)      # the argument checks
    only = _only_ids(ids)
    m = _Rows(x, name="mask", nonnegative=True)              # x is a volume already: it passes through
    dev = m.dev
    if m.empty:
        if only is not None and only.size:                   # ids that are not in the mask: raises
            plan_split(np.zeros((0, 6), np.int64), np.zeros(0, np.int64), 0, min_seed_voxels, only)
        return torch.zeros(m.shape, dtype=torch.int32, device=dev), SplitReport()
    ids_h = m.ids.cpu().numpy()
    top = int(ids_h[-1])
    if top > _INT32_MAX and not renumber:
        raise ValueError(f"the mask holds the id {top}, beyond int32; pass renumber=True to number the result 1..K")
    piece, table = core_pieces(m.x, radius, spacing, closed, m.pair)
    lut, fields = plan_split(table, ids_h, top, min_seed_voxels, only, renumber)
    if renumber:
        # ranks among the ids of the result: 1..K, in int32 whatever they were
        uniq = np.unique(np.concatenate((ids_h, lut[lut > 0])))
        lut = np.where(lut > 0, np.searchsorted(uniq, lut) + 1, 0)
        rank = torch.from_numpy(np.concatenate(([0], np.searchsorted(uniq, ids_h) + 1)).astype(np.int32)).to(dev)
        base = rank[m.row_volume().long()]
    else:
        base = m.x.to(torch.int32)
    base = base.contiguous()
    stats = dict(rounds=0)
    if fields["instances_split"]:
        seeds = torch.zeros(m.shape, dtype=torch.int32, device=dev)
        _apply(piece, lut, seeds, False)
        owner, _ = geodesic_assign(m.x, seeds, step, rows=m.pair, stats=stats)
        out = torch.where(owner > 0, owner, base)
    else:
        out = base.clone()
    fields["voxels_relabelled"] = int((out != base).sum().item())
    fields["rounds"] = int(stats["rounds"])
    if renumber:
        out = renumber_first_seen(out, fields["instances_out"])
    return out, SplitReport(**fields)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.split",
                                     description="SKOOTS: cut the instances of a mask at their necks -- an id whose body "
                                                 "falls into several cores at depth R is divided among them along paths "
                                                 "inside the instance.  The largest core keeps the id.")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif, stored [Z, X, Y])")
    parser.add_argument("--radius", type=float, required=True, metavar="R",
                        help="Depth, in the units of the spacing, at which the cores are taken: between the half-width of "
                             "the necks and that of the bodies")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--closed", action="store_true",
                        help="Measure depth in the volume padded with background: a face of the volume bounds an instance")
    parser.add_argument("--min-seed-voxels", type=int, default=1, metavar="N", help="Drop every core with fewer voxels")
    parser.add_argument("--costs", type=int, nargs=3, default=None, metavar=("CX", "CY", "CZ"),
                        help="Integer step costs (1..255) along x, y and z; default: the spacing when it is integral")
    parser.add_argument("--ids", type=int, nargs="+", default=None, metavar="ID", help="Cut only these ids")
    parser.add_argument("--renumber", action="store_true", help="Number the result 1..K by first appearance")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the mask")
    args = parser.parse_args(argv)
    if not (0 <= args.radius < float("inf")):
        parser.error("--radius must be a non-negative finite number")
    if args.min_seed_voxels < 1:
        parser.error("--min-seed-voxels must be at least 1")
    if args.costs is not None and not all(1 <= c <= 255 for c in args.costs):
        parser.error("--costs must be three integers in 1..255")
    if args.ids is not None and any(i <= 0 for i in args.ids):
        parser.error("--ids must be positive")
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
    cut, report = split(stack.permute(1, 2, 0).contiguous(), args.radius, spacing=args.spacing, closed=args.closed,
                        min_seed_voxels=args.min_seed_voxels, costs=args.costs, ids=args.ids, renumber=args.renumber)
    path = args.mask
    if not args.overwrite:
        file, ext = os.path.splitext(path)
        path = file + "_split" + ext
    tiff.write_label_stack(path, cut.permute(2, 0, 1).contiguous())
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value}")
    print(f"File Written: {path}", flush=True)
    return path


if __name__ == "__main__":
    main()
