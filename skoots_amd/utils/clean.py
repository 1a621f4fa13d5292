"""``python -m skoots_amd.utils.clean MASK.tif [--components keep|largest|split] [--connectivity 6|18|26] [--min-voxels N]
[--clear-border [x y z]] [--fill-holes] [--renumber] [-o]``: make every instance id of a mask one solid body.

The measurements of ``validate/compare.py`` assume that an id marks one body; nothing upstream makes it so (``eval()``
labels voxel by voxel, the stitch of ``watershed_and_stitch`` is greedy), and the reference has no tool for it.
``clean`` labels the connected pieces of all ids at once on the device (``lib.morphology.label_components``), decides on
the small table of pieces on the host (``plan_relabel``, ``plan_fill``: pure functions) and rewrites the volume with one
table look-up per step.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, Tuple

import numpy as np
import torch
from torch import Tensor

COMPONENTS = ("keep", "largest", "split")
_INT32_MAX = 2 ** 31 - 1
_AXIS_BITS = (3, 12, 48)       # border_bits of the table: the two faces of x, of y, of z


@dataclasses.dataclass
class CleanReport:
    """What ``clean`` found and did, in Python ints.  ``pieces`` counts the connected pieces of all ids of the input and
    ``ids_in_pieces`` the ids with more than one; ``pieces_removed`` (largest) and ``ids_added`` (split) are the pieces
    step 1 took from their ids; ``ids_removed_small`` and ``ids_removed_border`` the ids steps 2 and 3 cleared, each id
    counted in the first step that cleared it; ``holes_ambiguous`` the enclosed pockets left alone because more than one
    id touches them; ``voxels_cleared`` the voxels steps 1 to 3 set to 0 and ``voxels_filled`` those step 4 set."""
    instances_in: int = 0
    pieces: int = 0
    ids_in_pieces: int = 0
    pieces_removed: int = 0
    ids_added: int = 0
    ids_removed_small: int = 0
    ids_removed_border: int = 0
    holes_filled: int = 0
    holes_ambiguous: int = 0
    voxels_cleared: int = 0
    voxels_filled: int = 0
    instances_out: int = 0


def _border_axes(clear_border) -> Tuple[bool, bool, bool]:
    if isinstance(clear_border, (bool, np.bool_)):
        return (bool(clear_border),) * 3
    try:
        axes = tuple(clear_border)
    except TypeError:
        axes = ()
    if len(axes) != 3 or not all(isinstance(v, (bool, np.bool_)) for v in axes):
        raise ValueError(f"clear_border must be a bool or three bools (x, y, z), got {clear_border!r}")
    return tuple(bool(v) for v in axes)


def _table(table) -> np.ndarray:
    t = table.cpu().numpy() if isinstance(table, Tensor) else np.asarray(table)
    t = t.astype(np.int64).reshape(-1, 6) if t.size else np.zeros((0, 6), np.int64)
    return t


def plan_relabel(table, max_id: int, components: str = "keep", min_voxels: int = 0, clear_border=False,
                 renumber: bool = False) -> Tuple[np.ndarray, Dict[str, int]]:
    """Steps 1 to 3 of ``clean`` on the table of ``label_components`` ((P, 6): value, voxels, first_voxel, border_bits,
    ...; piece p is row p - 1 and the pieces are numbered by first voxel).  Pure: numpy or CPU torch in, numpy out.

    Returns ``(lut, fields)``: ``lut`` (P + 1) int64 with ``lut[0] == 0``, the id piece p carries afterwards or 0, and
    the report fields these steps own.  ``max_id`` is the largest id of the mask: ``split`` numbers its new ids
    ``max_id + 1, max_id + 2, ...`` in the order of the pieces' first voxels.  An id beyond int32 raises ``ValueError``
    unless ``renumber`` says that the caller compacts the ids anyway."""
    if components not in COMPONENTS:
        raise ValueError(f"components must be one of {COMPONENTS}, got {components!r}")
    if isinstance(min_voxels, bool) or not isinstance(min_voxels, (int, np.integer)) or min_voxels < 0:
        raise ValueError(f"min_voxels must be a non-negative integer, got {min_voxels!r}")
    axes = _border_axes(clear_border)
    t = _table(table)
    P = t.shape[0]
    value, voxels, first, bits = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if P and (value <= 0).any():
        raise ValueError("plan_relabel takes the table of the positive values (label_components(background=False))")
    # the piece an id keeps: most voxels, on a tie the first in raster order
    order = np.lexsort((first, -voxels, value))
    main = np.zeros(P, bool)
    if P:
        v = value[order]
        main[order[np.concatenate(([True], v[1:] != v[:-1]))]] = True
    instances_in = int(main.sum())
    per_id = np.unique(value, return_counts=True)[1] if P else np.zeros(0, np.int64)
    new = value.copy()
    extra = int(P - instances_in)
    if components == "largest":
        new[~main] = 0
    elif components == "split":
        new[~main] = int(max_id) + 1 + np.arange(extra, dtype=np.int64)      # rows are in order of first voxel
    top = int(new.max()) if P else 0
    if top > _INT32_MAX and not renumber:
        raise ValueError(f"the ids would reach {top}, beyond int32"
                         + (f": {extra} pieces need new ids above the largest id {int(max_id)}" if components == "split"
                            else "") + "; pass renumber=True to number the result 1..K")
    # steps 2 and 3 look at ids as they stand now: an id's voxels and faces are those of all its pieces
    uniq, inv = np.unique(new, return_inverse=True)
    total = np.zeros(uniq.size, np.int64)
    faces = np.zeros(uniq.size, np.int64)
    np.add.at(total, inv, voxels)
    np.bitwise_or.at(faces, inv, bits)
    live = uniq > 0
    small = live & (total < int(min_voxels))
    mask = sum(b for b, on in zip(_AXIS_BITS, axes) if on)
    border = live & ~small & ((faces & mask) != 0)
    keep = live & ~small & ~border
    lut = np.zeros(P + 1, np.int64)
    lut[1:] = np.where(keep[inv], new, 0)
    fields = dict(instances_in=instances_in, pieces=int(P), ids_in_pieces=int((per_id > 1).sum()),
                  pieces_removed=extra if components == "largest" else 0,
                  ids_added=extra if components == "split" else 0,
                  ids_removed_small=int(small.sum()), ids_removed_border=int(border.sum()),
                  voxels_cleared=int(voxels[lut[1:] == 0].sum()), instances_out=int(keep.sum()))
    return lut, fields


def plan_fill(table_zero) -> Tuple[np.ndarray, Dict[str, int]]:
    """Step 4 of ``clean`` on the table of ``label_components(background=True)`` of the result so far.  Pure.

    A hole is a 6-connected piece of zero voxels that touches no face of the volume (``border_bits == 0``) and whose
    positive 6-neighbours all carry one id (``min_neighbour_id == max_neighbour_id``); it takes that id.  An enclosed
    pocket between two or more ids is left alone and counted.  Returns ``(lut, fields)``: ``lut`` (P + 1) int64, the id
    zero piece p is filled with or 0."""
    t = _table(table_zero)
    P = t.shape[0]
    if P and (t[:, 0] != 0).any():
        raise ValueError("plan_fill takes the table of the zero voxels (label_components(background=True))")
    inside = t[:, 3] == 0
    hole = inside & (t[:, 4] == t[:, 5]) & (t[:, 4] > 0)
    lut = np.zeros(P + 1, np.int64)
    lut[1:] = np.where(hole, t[:, 4], 0)
    return lut, dict(holes_filled=int(hole.sum()), holes_ambiguous=int((inside & (t[:, 4] != t[:, 5])).sum()),
                     voxels_filled=int(t[hole, 1].sum()))


def _apply(piece: Tensor, lut: np.ndarray, out: Tensor, only_pieces: bool) -> None:
    from .. import _ffi
    lut_d = torch.from_numpy(lut.astype(np.int32)).to(piece.device)
    _ffi.check(_ffi.lib.sk_apply_piece_lut(_ffi.ptr(piece), _ffi.ptr(lut_d), int(lut_d.numel()), _ffi.ptr(out),
                                           piece.numel(), int(only_pieces), _ffi.stream_ptr(piece.device)))


def clean(mask: Tensor, *, components: str = "keep", connectivity: int = 6, min_voxels: int = 0, clear_border=False,
          fill_holes: bool = False, renumber: bool = False) -> Tuple[Tensor, CleanReport]:
    """Cleans an instance mask, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype without negative values:
    ``(cleaned (X, Y, Z) int32, CleanReport)``.  The steps run in this order, and the result depends on it -- a speck
    inside a cavity is removed before the cavity is filled, so the body comes out solid:

    1. pieces.  The connected pieces of every id at ``connectivity`` 6, 18 or 26.  ``"keep"`` leaves the ids as they are;
       ``"largest"`` keeps, for every id, the piece with the most voxels (on a tie the one whose first voxel comes first
       in C order) and clears the others; ``"split"`` keeps that piece under its id and gives the others the new ids
       ``max id + 1, max id + 2, ...`` in the order of their first voxels over the whole volume.
    2. ``min_voxels``.  Every id, as it stands after step 1, with fewer voxels in total is cleared.
    3. ``clear_border``.  Every id with a voxel on a face of a selected axis is cleared: ``True`` selects all three,
       ``(True, True, False)`` spares the z faces of a cut stack.
    4. ``fill_holes``.  A 6-connected piece of zero voxels of the result so far that touches no face of the volume and
       whose positive 6-neighbours all carry one id takes that id; pockets between several ids are left and counted
       (``holes_ambiguous``).  The background is 6-connected whatever ``connectivity`` is, as in
       ``scipy.ndimage.binary_fill_holes``, which the result equals for a mask of one id.
    5. ``renumber``.  1..K by first appearance in C order (``renumber_first_seen``).

    Ids beyond int32 -- in the mask, or made by ``"split"`` -- raise ``ValueError`` unless ``renumber`` is set.  Every
    step is exact integer work: two runs give identical tensors and reports.  HIP kernels only, no CPU fallback."""
    from ..lib.morphology import CONNECTIVITIES, _label_pieces, check_piece_shape, label_components
    from ..validate.lib import _Rows, _as_volume
    from .renumber import renumber_first_seen
    x = _as_volume(mask, "mask")
    check_piece_shape(x.shape)
    if connectivity not in CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    plan_relabel(np.zeros((0, 6), np.int64), 0, components, min_voxels, clear_border)      # the argument checks
    m = _Rows(x, name="mask", nonnegative=True)           # x is a volume already: it passes through
    out = torch.zeros(m.shape, dtype=torch.int32, device=m.dev)
    if m.empty:
        return out, CleanReport()
    piece, table = label_components(m.x, connectivity, rows=m.pair)
    lut, fields = plan_relabel(table, int(m.ids[-1].item()), components, min_voxels, clear_border, renumber)
    k = fields["instances_out"]
    if renumber:                                             # ranks among the surviving ids: 1..K, in int32 whatever they were
        uniq = np.unique(lut[lut > 0])
        lut = np.where(lut > 0, np.searchsorted(uniq, lut) + 1, 0)
    _apply(piece, lut, out, False)
    if fill_holes and k:
        zero_piece, zero_table = _label_pieces(out, 6, 0)
        zero_lut, zero_fields = plan_fill(zero_table)
        fields.update(zero_fields)
        if zero_fields["holes_filled"]:
            _apply(zero_piece, zero_lut, out, True)
    if renumber:
        out = renumber_first_seen(out, k)
    return out, CleanReport(**fields)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.clean",
                                     description="SKOOTS: make every instance id of a mask one solid body -- split or drop "
                                                 "stray pieces, drop specks and instances on the border, fill enclosed "
                                                 "holes.  The steps run in the order of the options below.")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif, stored [Z, X, Y])")
    parser.add_argument("--components", type=str, default=None, choices=COMPONENTS,
                        help="largest: keep only the largest connected piece of every id; split: give the other pieces "
                             "new ids above the largest id; keep (default): leave the ids as they are")
    parser.add_argument("--connectivity", type=int, default=6, choices=(6, 18, 26), help="Neighbourhood of the pieces")
    parser.add_argument("--min-voxels", type=int, default=None, metavar="N", help="Clear every id with fewer voxels")
    parser.add_argument("--clear-border", type=str, nargs="*", default=None, choices=("x", "y", "z"), metavar="AXIS",
                        help="Clear every id that touches a face of the volume; with axes (x y z), only the faces of those")
    parser.add_argument("--fill-holes", action="store_true",
                        help="Fill every enclosed background pocket that touches exactly one id with that id")
    parser.add_argument("--renumber", action="store_true", help="Number the result 1..K by first appearance")
    parser.add_argument("-o", "--overwrite", action="store_true", help="Write the result over the mask")
    args = parser.parse_args(argv)
    if (args.components in (None, "keep") and args.min_voxels is None and args.clear_border is None
            and not args.fill_holes and not args.renumber):
        parser.error("nothing was asked for: give at least one of --components largest|split, --min-voxels, "
                     "--clear-border, --fill-holes, --renumber (the file was not rewritten)")
    if args.min_voxels is not None and args.min_voxels < 0:
        parser.error("--min-voxels must not be negative")
    args.components = args.components or "keep"
    args.min_voxels = args.min_voxels or 0
    if args.clear_border is None:
        args.clear_border = False
    else:
        args.clear_border = tuple(a in args.clear_border for a in "xyz") if args.clear_border else True
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
    cleaned, report = clean(stack.permute(1, 2, 0).contiguous(), components=args.components,
                            connectivity=args.connectivity, min_voxels=args.min_voxels, clear_border=args.clear_border,
                            fill_holes=args.fill_holes, renumber=args.renumber)
    path = args.mask
    if not args.overwrite:
        file, ext = os.path.splitext(path)
        path = file + "_cleaned" + ext
    tiff.write_label_stack(path, cleaned.permute(2, 0, 1).contiguous())
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value}")
    print(f"File Written: {path}", flush=True)
    return path


if __name__ == "__main__":
    main()
