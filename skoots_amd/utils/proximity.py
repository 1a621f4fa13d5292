"""``python -m skoots_amd.utils.proximity A.tif [B.tif] --distance D [--spacing SX SY SZ] [--save-sites] [-o]``: which
objects lie within a distance of each other, how close they come and how much of each lies that close.

``contacts`` says which instances of one mask touch and ``relate`` which instances of two masks share voxels; a membrane
contact site is neither -- it is a gap of some tens of nanometres between a mitochondrion and a second organelle.
``proximity`` reads the table of pairs within the distance off the device (``validate.lib.instance_proximity``: one
kernel pass per direction), joins the two directions on the host and derives the per-instance columns from that small
table (``validate.lib.plan_proximity``: a pure function).  With one mask it answers the same inside it: nearest-
neighbour gaps and crowding.  The reference has no counterpart.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

PAIR_CSV_COLUMNS = "a_id,b_id,gap,a_near_voxels,a_near_fraction,b_near_voxels,b_near_fraction"
NEAR_CSV_COLUMNS = "id,voxels,partners,nearest_id,nearest_gap,near_voxels,near_fraction"


@dataclasses.dataclass
class ProximityReport:
    """What ``proximity`` found, in Python ints and floats.  ``pairs`` are the pairs of instances within the distance;
    ``a_with_partner`` / ``b_with_partner`` the instances that have one; ``a_near_voxels`` / ``b_near_voxels`` the
    voxels within the distance of any instance of the other mask; ``min_gap`` the smallest gap of all (``inf`` without
    a pair).  In the one-mask mode the ``b`` fields repeat the ``a`` fields."""
    instances_a: int = 0
    instances_b: int = 0
    pairs: int = 0
    a_with_partner: int = 0
    b_with_partner: int = 0
    a_near_voxels: int = 0
    b_near_voxels: int = 0
    min_gap: float = math.inf


def _voxels(m, voxels=None) -> np.ndarray:
    """(N) int64: the voxel count of every row of a ``_Rows`` -- the caller's, or column 0 of ``instance_sums``"""
    from ..validate.lib import instance_sums
    if voxels is None:
        voxels = instance_sums(m.x, m.pair)[1][:, 0]
    voxels = torch.as_tensor(voxels).reshape(-1)
    if voxels.numel() != m.N:
        raise ValueError(f"{voxels.numel()} voxel counts for {m.N} instances")
    return voxels.cpu().numpy().astype(np.int64)


def _side_table(ids: Tensor, voxels: np.ndarray, plan: Dict[str, np.ndarray], other_ids: np.ndarray, dev) -> Dict:
    lut = np.concatenate(([0], other_ids.astype(np.int64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = plan["near_voxels"].astype(np.float64) / voxels.astype(np.float64)
    fraction[voxels == 0] = 0.0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {"id": ids, "voxels": up(voxels), "partners": up(plan["partners"]), "nearest_id": up(lut[plan["nearest_row"]]),
            "nearest_gap": up(np.sqrt(plan["nearest_gap2"])), "near_voxels": up(plan["near_voxels"]),
            "near_fraction": up(fraction)}


def proximity(a: Tensor, b: Optional[Tensor] = None, distance=None, spacing=(1.0, 1.0, 1.0), *, rows_a=None,
              rows_b=None, voxels_a=None, voxels_b=None):
    """Relates the instances of ``a`` to those of ``b`` -- or, with ``b=None``, to the other instances of ``a`` -- by
    distance: ``(pair_table, a_table, b_table, ProximityReport)`` for device tensors of one shape, (X, Y, Z) or
    (1, X, Y, Z), of any integer dtype.  ``distance`` is in the units of ``spacing``, centre to centre, and a pair at
    exactly the distance counts.

    ``pair_table`` has one row per pair of instances within the distance, sorted by ``(a_id, b_id)``, as device tensors:
    ``a_id``, ``b_id`` int64, ``gap`` float64 (the smallest distance between a voxel of one and a voxel of the other, 0
    where they overlap), ``a_near_voxels`` / ``b_near_voxels`` int64 (the voxels of each within the distance of the
    other) and ``a_near_fraction`` / ``b_near_fraction`` float64 (their share of the instance).  ``a_table`` and
    ``b_table`` have one row per id, ascending: ``id``, ``voxels``, ``partners`` (instances within the distance),
    ``nearest_id`` (0: none; the lowest id on a tie), ``nearest_gap`` (``inf``: none), ``near_voxels`` (within the
    distance of ANY partner) and ``near_fraction``.  In the one-mask mode ``b_table`` is ``None``, every unordered pair
    appears in both orders and an instance is never its own partner.

    ``rows_a`` / ``rows_b`` are ``id_rows`` of the masks and ``voxels_a`` / ``voxels_b`` their (N) voxel counts when the
    caller already has them; without, the counts come from one ``instance_sums`` pass per mask.

    Two-mask mode runs the kernel in both directions and joins them by pair; the gap is found independently by each and
    the function asserts that they agree bit for bit.  Exact integer work on the device and pure functions of a small
    table on the host: two runs give identical tensors.  HIP kernels only, no CPU fallback."""
    from ..validate.lib import _Rows, check_voxels, instance_proximity, plan_proximity
    ma = _Rows(a, rows_a, check_voxels, name="a")
    same = b is None
    mb = ma if same else _Rows(b, rows_b, check_voxels, name="b")
    dev, N, M = ma.dev, ma.N, mb.N
    ids_a, ids_b, pairs_ab, gap2_ab = instance_proximity(ma.x, None if same else mb.x, distance, spacing, ma.pair,
                                                         None if same else mb.pair)
    p_ab, g_ab = pairs_ab.cpu().numpy(), gap2_ab.cpu().numpy()
    if same:
        p_ba, g_ba = p_ab, g_ab
    else:
        _, _, pairs_ba, gap2_ba = instance_proximity(mb.x, ma.x, distance, spacing, mb.pair, ma.pair)
        p_ba, g_ba = pairs_ba.cpu().numpy(), gap2_ba.cpu().numpy()
    # join the directions by pair: (ra, rb) of one is (rb, ra) of the other
    ab, ba = p_ab[:, 1] > 0, p_ba[:, 1] > 0
    q_ab, q_ba = p_ab[ab], p_ba[ba]
    back = np.lexsort((q_ba[:, 0], q_ba[:, 1]))              # the other direction in (ra, rb) order of this one
    q_ba, gq_ba = q_ba[back], g_ba[ba][back]
    if q_ab.shape != q_ba.shape or not np.array_equal(q_ab[:, :2], q_ba[:, 1::-1]):
        raise AssertionError("proximity: the two directions name different pairs")
    if not np.array_equal(g_ab[ab].view(np.int64), gq_ba.view(np.int64)):
        raise AssertionError("proximity: the two directions disagree about a gap")
    vox_a = _voxels(ma, voxels_a)
    vox_b = vox_a if same else _voxels(mb, voxels_b)
    ids_a_h, ids_b_h = ids_a.cpu().numpy().astype(np.int64), ids_b.cpu().numpy().astype(np.int64)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    ra, rb = q_ab[:, 0] - 1, q_ab[:, 1] - 1
    pair_table = {"a_id": up(ids_a_h[ra]), "b_id": up(ids_b_h[rb]), "gap": up(np.sqrt(g_ab[ab])),
                  "a_near_voxels": up(q_ab[:, 2]), "a_near_fraction": up(q_ab[:, 2] / vox_a[ra].astype(np.float64)),
                  "b_near_voxels": up(q_ba[:, 2]), "b_near_fraction": up(q_ba[:, 2] / vox_b[rb].astype(np.float64))}
    plan_a = plan_proximity(p_ab, g_ab, N, M)
    a_table = _side_table(ids_a, vox_a, plan_a, ids_b_h, dev)
    plan_b = plan_a if same else plan_proximity(p_ba, g_ba, M, N)
    b_table = None if same else _side_table(ids_b, vox_b, plan_b, ids_a_h, dev)
    report = ProximityReport(instances_a=N, instances_b=M, pairs=int(q_ab.shape[0]),
                             a_with_partner=int((plan_a["partners"] > 0).sum()),
                             b_with_partner=int((plan_b["partners"] > 0).sum()),
                             a_near_voxels=int(plan_a["near_voxels"].sum()), b_near_voxels=int(plan_b["near_voxels"].sum()),
                             min_gap=float(np.sqrt(g_ab[ab].min())) if q_ab.shape[0] else math.inf)
    return pair_table, a_table, b_table, report


def sites(a: Tensor, b: Tensor, distance, spacing=(1.0, 1.0, 1.0)) -> Tensor:
    """(X, Y, Z) int64, for device tensors (X, Y, Z) or (1, X, Y, Z): every voxel of ``a`` within ``distance`` of any instance of ``b`` carrying its own id, 0
    elsewhere -- from ``lib.morphology.nearest_label`` restricted to the voxels of ``a``, a kernel independent of the
    pair table; per id its voxel count equals the union row's ``near_voxels``."""
    from ..lib.morphology import nearest_label
    from ..validate.lib import _as_volume
    a, b = _as_volume(a, "a"), _as_volume(b, "b")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must have one shape")
    _, dist2 = nearest_label(b, spacing, distance, where=a > 0)
    return torch.where((a > 0) & (dist2 < float("inf")), a.to(torch.int64), torch.zeros((), dtype=torch.int64, device=a.device))


def _header(a_path: str, b_path: Optional[str], distance, spacing):
    from ..validate.compare import _spacing
    return [f"A File: {a_path} B File: {b_path if b_path is not None else a_path}\n",
            "Spacing: {} {} {} Distance: {}\n".format(*(repr(v) for v in _spacing(spacing)), repr(float(distance)))]


def _columns(table: Dict, names) -> list:
    return [(v.cpu().tolist() if isinstance(v, Tensor) else np.asarray(v).tolist()) for v in (table[k] for k in names)]


def _rows_text(table: Dict, names: str, floats) -> list:
    return [",".join(repr(float(v)) if k in floats else str(int(v)) for k, v in enumerate(row)) + "\n"
            for row in zip(*_columns(table, names.split(",")))]


def format_pairs_csv(a_path: str, b_path: Optional[str], pair_table: Dict, distance, spacing=(1.0, 1.0, 1.0)) -> str:
    """The text of ``<A>_proximity.csv``: two header lines (the files; spacing and distance), ``PAIR_CSV_COLUMNS`` and
    one row per pair in ``(a_id, b_id)`` order.  Floats are printed with ``repr``.  A pure function of its arguments."""
    return "".join(_header(a_path, b_path, distance, spacing) + [PAIR_CSV_COLUMNS + "\n"] +
                   _rows_text(pair_table, PAIR_CSV_COLUMNS, (2, 4, 6)))


def format_near_csv(a_path: str, b_path: Optional[str], table: Dict, distance, spacing=(1.0, 1.0, 1.0)) -> str:
    """The text of ``<A>_near.csv`` / ``<B>_near.csv``: the same two header lines, ``NEAR_CSV_COLUMNS`` and one row per
    id in ascending order.  Floats are printed with ``repr``.  A pure function of its arguments."""
    return "".join(_header(a_path, b_path, distance, spacing) + [NEAR_CSV_COLUMNS + "\n"] +
                   _rows_text(table, NEAR_CSV_COLUMNS, (4, 6)))


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.proximity",
                                     description="SKOOTS: which objects lie within a distance of each other, how close "
                                                 "they come, and how much of each lies that close")
    parser.add_argument("a", type=str, help="Path to a mask (.tif, stored [Z, X, Y])")
    parser.add_argument("b", type=str, nargs="?", default=None,
                        help="Path to a second mask of the same shape; without it the instances of A are set against "
                             "each other")
    parser.add_argument("--distance", type=float, required=True, metavar="D",
                        help="The distance, in the units of --spacing, centre to centre; a pair at exactly D counts")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--save-sites", action="store_true",
                        help="Also write <A>_sites.tif: every voxel of A within D of an instance of B carrying A's id")
    parser.add_argument("-o", "--overwrite", action="store_true",
                        help="With --save-sites: write the sites volume over the A file")
    args = parser.parse_args(argv)
    if not (math.isfinite(args.distance) and args.distance >= 0.0):
        parser.error("--distance takes a non-negative finite number")
    if args.save_sites and args.b is None:
        parser.error("--save-sites needs a second mask: the sites of A are its voxels near B")
    if args.overwrite and not args.save_sites:
        parser.error("-o writes the volume of --save-sites over the A file")
    return args


def _near_path(path: str) -> str:
    return f"{os.path.splitext(path)[0]}_near.csv"


def main(argv=None) -> Tuple[str, ...]:
    """Runs the command; returns the paths of the CSV files."""
    from .relate import _load
    args = parse_args(argv)
    for path in (args.a, args.b):
        if path is not None and not os.path.exists(path):
            raise FileNotFoundError(f"{path} does not exist")
    if args.b is not None and _near_path(args.a) == _near_path(args.b):
        raise ValueError(f"{args.a} and {args.b} would share {_near_path(args.a)}")
    device = torch.device("cuda", torch.cuda.current_device())                # the HIP library: no CPU fallback
    a = _load(args.a, device)
    b = None if args.b is None else _load(args.b, device)
    if b is not None and tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{args.a} has (X, Y, Z) = {tuple(a.shape)} and {args.b} {tuple(b.shape)}: the two masks need "
                         "one shape")
    pair_table, a_table, b_table, report = proximity(a, b, args.distance, args.spacing)
    out = [f"{os.path.splitext(args.a)[0]}_proximity.csv", _near_path(args.a)]
    texts = [format_pairs_csv(args.a, args.b, pair_table, args.distance, args.spacing),
             format_near_csv(args.a, args.b, a_table, args.distance, args.spacing)]
    if b_table is not None:
        out.append(_near_path(args.b))
        texts.append(format_near_csv(args.a, args.b, b_table, args.distance, args.spacing))
    for path, text in zip(out, texts):
        with open(path, "w") as file:
            file.write(text)
    for name, value in dataclasses.asdict(report).items():
        print(f"{name}: {value!r}" if isinstance(value, float) else f"{name}: {value}")
    for path in out:
        print(f"File Written: {path}")
    if args.save_sites:
        from ..lib import tiff
        file, ext = os.path.splitext(args.a)
        path = args.a if args.overwrite else file + "_sites" + ext
        volume = sites(a, b, args.distance, args.spacing)
        if volume.numel() and int(volume.max()) > 2 ** 31 - 1:
            raise ValueError(f"{args.a} holds the id {int(volume.max())}, beyond int32: the sites volume is int32")
        tiff.write_label_stack(path, volume.to(torch.int32).permute(2, 0, 1).contiguous())
        print(f"File Written: {path}", flush=True)
    return tuple(out)


if __name__ == "__main__":
    main()
