"""``python -m skoots_amd.utils.relate CHILDREN.tif PARENTS.tif [--min-fraction F] [--spacing SX SY SZ]
[--save-relabelled] [-o]``: which object of one mask lies in which object of another.

SKOOTS segments mitochondria and the biology is per cell: given a mask of mitochondria and a mask of cells, the cell
every mitochondrion belongs to, how many each cell holds and what share of the cell they fill.  ``contacts`` relates
the ids of one mask and ``compare`` matches two masks of the same objects; this relates two masks of different objects.
``relate`` reads the sparse table of overlapping pairs off the device (``validate.lib.instance_overlaps``, one kernel
pass over both masks), decides on that small table on the host (``plan_relate``: a pure function) and, when asked,
rewrites the children with one table look-up.  The reference has no counterpart.
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

CHILD_CSV_COLUMNS = "id,voxels,parent_id,inside_voxels,inside_fraction,parents_touched,outside_voxels"
PARENT_CSV_COLUMNS = "id,voxels,children,children_voxels,occupied_voxels,occupancy,children_volume"


@dataclasses.dataclass
class RelateReport:
    """What ``relate`` found, in Python ints.  ``children_assigned`` have a parent and ``children_without_parent`` have
    none -- they share no voxel with a parent, or too small a share; ``children_straddling`` share voxels with more than
    one parent, assigned or not; ``parents_without_children`` were assigned nobody.  ``voxels_children`` are the voxels
    of all children, ``voxels_inside`` those they share with the parent they were assigned to and ``voxels_outside``
    those over the parents' background."""
    children: int = 0
    parents: int = 0
    children_assigned: int = 0
    children_without_parent: int = 0
    children_straddling: int = 0
    parents_without_children: int = 0
    voxels_children: int = 0
    voxels_inside: int = 0
    voxels_outside: int = 0


def _min_fraction(value) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(value) <= 1.0:
        raise ValueError(f"min_fraction must be a share in [0, 1], got {value!r}")
    return float(value)


def plan_relate(table, N: int, M: int, min_fraction: float = 0.0) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """Who belongs to whom, from the (P, 3) table ``ra, rb, voxels`` of ``instance_overlaps(children, parents,
    background=True)`` -- rows 1 .. N of the children, 1 .. M of the parents, 0 the background of either -- and nothing
    else.  Pure: numpy or CPU torch in, numpy out.  Returns ``(children, parents)``, dicts of arrays with one entry per
    row 1 .. N and 1 .. M, in ascending order.

    Per child: ``voxels`` int64, the sum of its rows over all partners, background included; ``parent_row`` int64, the
    parent it shares most voxels with, the lowest row on a tie, and 0 when it shares none or when ``inside_voxels /
    voxels < min_fraction`` in float64; ``inside_voxels`` int64, the voxels shared with that parent (0 without one) and
    ``inside_fraction`` float64 = ``inside_voxels / voxels``; ``parents_touched`` int64, the parents it shares a voxel
    with; ``outside_voxels`` int64, its voxels over the parents' background.

    Per parent: ``voxels`` int64, its voxel count (the sum of its rows, the children's background included);
    ``children`` int64, the children assigned to it; ``children_voxels`` int64, the sum of those children's ``voxels``
    -- all of each, the parts outside the parent too; ``occupied_voxels`` int64, its voxels under any child, assigned to
    it or not; ``occupancy`` float64 = ``occupied_voxels / voxels``."""
    min_fraction = _min_fraction(min_fraction)
    N, M = int(N), int(M)
    t = np.asarray(table.cpu() if isinstance(table, Tensor) else table)
    t = t.astype(np.int64).reshape(-1, 3) if t.size else np.zeros((0, 3), np.int64)
    if t.shape[0] and (t.min() < 0 or t[:, 0].max() > N or t[:, 1].max() > M or ((t[:, 0] == 0) & (t[:, 1] == 0)).any()):
        raise ValueError(f"the table names a row outside 0 .. {N} / 0 .. {M}, or the pair (0, 0)")
    ra, rb, v = t[:, 0], t[:, 1], t[:, 2]
    size_c, size_p = np.zeros(N + 1, np.int64), np.zeros(M + 1, np.int64)
    np.add.at(size_c, ra, v)
    np.add.at(size_p, rb, v)
    both = (ra > 0) & (rb > 0)
    touched, outside, occupied = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64), np.zeros(M + 1, np.int64)
    np.add.at(touched, ra[both], 1)
    np.add.at(outside, ra[rb == 0], v[rb == 0])
    np.add.at(occupied, rb[both], v[both])
    # per child: most shared voxels first, then the lower parent row
    a, b, w = ra[both], rb[both], v[both]
    order = np.lexsort((b, -w, a))
    first = order[np.concatenate(([True], a[order][1:] != a[order][:-1]))] if order.size else order
    parent, inside = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    parent[a[first]], inside[a[first]] = b[first], w[first]
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = inside.astype(np.float64) / size_c.astype(np.float64)
    reject = (parent > 0) & (fraction < min_fraction)
    parent[reject], inside[reject] = 0, 0
    fraction[(parent == 0) | (size_c == 0)] = 0.0
    n_children, children_voxels = np.zeros(M + 1, np.int64), np.zeros(M + 1, np.int64)
    np.add.at(n_children, parent[1:], 1)
    np.add.at(children_voxels, parent[1:], size_c[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        occupancy = occupied.astype(np.float64) / size_p.astype(np.float64)
    occupancy[size_p == 0] = 0.0
    children = {"voxels": size_c[1:], "parent_row": parent[1:], "inside_voxels": inside[1:],
                "inside_fraction": fraction[1:], "parents_touched": touched[1:], "outside_voxels": outside[1:]}
    parents = {"voxels": size_p[1:], "children": n_children[1:], "children_voxels": children_voxels[1:],
               "occupied_voxels": occupied[1:], "occupancy": occupancy[1:]}
    return children, parents


def _voxel_volume(spacing) -> float:
    from ..validate.compare import _spacing
    sx, sy, sz = _spacing(spacing)
    return sx * sy * sz


def relate(children: Tensor, parents: Tensor, min_fraction: float = 0.0, spacing=(1.0, 1.0, 1.0), *,
           relabel: bool = False, rows_children=None, rows_parents=None):
    """Relates the instances of ``children`` to those of ``parents``, two device tensors of one shape, (X, Y, Z) or
    (1, X, Y, Z), of any integer dtype: ``(child_table, parent_table, RelateReport)``.  One kernel pass over both masks
    gives the sparse table of overlapping pairs (``validate.lib.instance_overlaps`` with the background rows) and
    ``plan_relate`` decides on it.

    ``child_table`` has one row per child id, ascending, as device tensors: ``id``, ``voxels``, ``parent_id`` (0: none),
    ``inside_voxels``, ``parents_touched``, ``outside_voxels`` int64 and ``inside_fraction`` float64.  ``parent_table``
    one per parent id: ``id``, ``voxels``, ``children``, ``children_voxels``, ``occupied_voxels`` int64, ``occupancy``
    float64 and ``children_volume`` float64 = ``children_voxels`` times the voxel volume of ``spacing``.  ``plan_relate``
    says what each means.  ``relabel=True`` adds ``child_table["by_parent"]``, (X, Y, Z) int32: every child voxel
    carrying its parent's id (0 without one), written with one table look-up on the device; it needs children without
    negative values and parent ids within int32.  ``rows_children`` / ``rows_parents`` are ``id_rows`` of the masks when
    the caller already has them.

    Every step is exact integer work on the device and a pure function of a small table on the host: two runs give
    identical tensors and reports.  HIP kernels only, no CPU fallback."""
    from ..validate.lib import _Rows, check_voxels, instance_overlaps
    min_fraction = _min_fraction(min_fraction)
    volume = _voxel_volume(spacing)
    mc = _Rows(children, rows_children, check_voxels, name="children", nonnegative=relabel)
    mp = _Rows(parents, rows_parents, check_voxels, name="parents")
    ids_c, ids_p, table = instance_overlaps(mc.x, mp.x, True, mc.pair, mp.pair)
    N, M, dev = mc.N, mp.N, mc.dev
    c, p = plan_relate(table.cpu().numpy(), N, M, min_fraction)
    ids_p_h = np.concatenate(([0], ids_p.cpu().numpy().astype(np.int64)))
    parent_id = ids_p_h[c["parent_row"]]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    child_table = {"id": ids_c, "voxels": up(c["voxels"]), "parent_id": up(parent_id),
                   "inside_voxels": up(c["inside_voxels"]), "inside_fraction": up(c["inside_fraction"]),
                   "parents_touched": up(c["parents_touched"]), "outside_voxels": up(c["outside_voxels"])}
    parent_table = {"id": ids_p, **{k: up(v) for k, v in p.items()},
                    "children_volume": up(p["children_voxels"].astype(np.float64) * volume)}
    if relabel:
        if M and int(ids_p_h[-1]) > _INT32_MAX:
            raise ValueError(f"the parents hold the id {int(ids_p_h[-1])}, beyond int32: the relabelled volume is int32")
        if mc.empty:
            child_table["by_parent"] = torch.zeros(mc.shape, dtype=torch.int32, device=dev)
        else:                                                # value of `a` -> its row -> the id of that row's parent
            new_id = torch.from_numpy(np.concatenate(([0], parent_id)).astype(np.int32)).to(dev)
            child_table["by_parent"] = new_id[mc.lut.long()][mc.a]
    assigned = int((c["parent_row"] > 0).sum())
    report = RelateReport(children=N, parents=M, children_assigned=assigned, children_without_parent=N - assigned,
                          children_straddling=int((c["parents_touched"] > 1).sum()),
                          parents_without_children=int((p["children"] == 0).sum()),
                          voxels_children=int(c["voxels"].sum()), voxels_inside=int(c["inside_voxels"].sum()),
                          voxels_outside=int(c["outside_voxels"].sum()))
    return child_table, parent_table, report


def _header(children_path: str, parents_path: str, spacing, min_fraction: float):
    from ..validate.compare import _spacing
    return [f"Children File: {children_path} Parents File: {parents_path}\n",
            "Spacing: {} {} {} Min Fraction: {}\n".format(*(repr(v) for v in _spacing(spacing)), repr(float(min_fraction)))]


def _columns(table: Dict, names) -> list:
    return [(v.cpu().tolist() if isinstance(v, Tensor) else np.asarray(v).tolist()) for v in (table[k] for k in names)]


def format_parents_csv(children_path: str, parents_path: str, child_table: Dict, spacing=(1.0, 1.0, 1.0),
                       min_fraction: float = 0.0) -> str:
    """The text of ``<children>_parents.csv``: two header lines (the files; spacing and ``min_fraction``), the column
    names ``CHILD_CSV_COLUMNS`` and one row per child in ascending id order.  Floats are printed with ``repr``.  A pure
    function of its arguments."""
    lines = _header(children_path, parents_path, spacing, min_fraction) + [CHILD_CSV_COLUMNS + "\n"]
    for row in zip(*_columns(child_table, CHILD_CSV_COLUMNS.split(","))):
        lines.append(",".join(repr(float(v)) if k == 4 else str(int(v)) for k, v in enumerate(row)) + "\n")
    return "".join(lines)


def format_children_csv(children_path: str, parents_path: str, parent_table: Dict, spacing=(1.0, 1.0, 1.0),
                        min_fraction: float = 0.0) -> str:
    """The text of ``<parents>_children.csv``: the same two header lines, ``PARENT_CSV_COLUMNS`` and one row per parent
    in ascending id order.  Floats are printed with ``repr``.  A pure function of its arguments."""
    lines = _header(children_path, parents_path, spacing, min_fraction) + [PARENT_CSV_COLUMNS + "\n"]
    for row in zip(*_columns(parent_table, PARENT_CSV_COLUMNS.split(","))):
        lines.append(",".join(repr(float(v)) if k >= 5 else str(int(v)) for k, v in enumerate(row)) + "\n")
    return "".join(lines)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.relate",
                                     description="SKOOTS: which object of one mask lies in which object of another -- "
                                                 "the parent of every child, and what every parent holds")
    parser.add_argument("children", type=str, help="Path to the mask of the smaller objects (.tif, stored [Z, X, Y])")
    parser.add_argument("parents", type=str, help="Path to the mask of the larger objects, of the same shape")
    parser.add_argument("--min-fraction", type=float, default=0.0, metavar="F",
                        help="A child with less than this share of its voxels inside its parent gets parent 0")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--save-relabelled", action="store_true",
                        help="Also write <children>_by_parent.tif: every child voxel carrying its parent's id")
    parser.add_argument("-o", "--overwrite", action="store_true",
                        help="With --save-relabelled: write the relabelled volume over the children file")
    args = parser.parse_args(argv)
    if not (math.isfinite(args.min_fraction) and 0.0 <= args.min_fraction <= 1.0):
        parser.error("--min-fraction takes a share in [0, 1]")
    if args.overwrite and not args.save_relabelled:
        parser.error("-o writes the volume of --save-relabelled over the children file")
    return args


def _load(path: str, device) -> Tensor:
    from ..lib import tiff
    stack = tiff.read_stack(path, device)
    if stack.ndim != 3:
        raise ValueError(f"{path}: expected a [Z, X, Y] stack, got shape {tuple(stack.shape)}")
    if stack.dtype in (torch.uint16, torch.uint32):
        stack = stack.to(torch.int64)     # torch moves and compares no wider unsigned types
    return stack.permute(1, 2, 0).contiguous()


def main(argv=None) -> Tuple[str, str]:
    """Runs the command; returns the paths of the two CSV files."""
    args = parse_args(argv)
    for path in (args.children, args.parents):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} does not exist")
    device = torch.device("cuda", torch.cuda.current_device())                # the HIP library: no CPU fallback
    children, parents = _load(args.children, device), _load(args.parents, device)
    if tuple(children.shape) != tuple(parents.shape):
        raise ValueError(f"{args.children} has (X, Y, Z) = {tuple(children.shape)} and {args.parents} "
                         f"{tuple(parents.shape)}: the two masks need one shape")
    child_table, parent_table, report = relate(children, parents, args.min_fraction, args.spacing,
                                               relabel=args.save_relabelled)
    out = (f"{os.path.splitext(args.children)[0]}_parents.csv", f"{os.path.splitext(args.parents)[0]}_children.csv")
    texts = (format_parents_csv(args.children, args.parents, child_table, args.spacing, args.min_fraction),
             format_children_csv(args.children, args.parents, parent_table, args.spacing, args.min_fraction))
    for path, text in zip(out, texts):
        with open(path, "w") as file:
            file.write(text)
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value}")
    for path in out:
        print(f"File Written: {path}")
    if args.save_relabelled:
        from ..lib import tiff
        file, ext = os.path.splitext(args.children)
        path = args.children if args.overwrite else file + "_by_parent" + ext
        tiff.write_label_stack(path, child_table["by_parent"].permute(2, 0, 1).contiguous())
        print(f"File Written: {path}", flush=True)
    return out


if __name__ == "__main__":
    main()
