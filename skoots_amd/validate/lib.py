"""Validation metrics (reference: skoots/validate/lib.py:170-315,358-438).

``mask_iou``, ``mask_dice`` and ``mask_soft_cldice`` are the heavy part -- the reference loops over every
ground-truth instance in Python and forms full-volume masks (and, for clDice, two soft skeletons) per touching
pair; here one kernel pass builds the (gt, pred) contingency tables and a second one turns them into the matrices
(``mask_metrics`` gives all three from one pass).  The bookkeeping on the small matrix
(``accuracies_from_iou``, ``f1_score``, ``get_segmentation_errors``) is host logic on its values.

``instance_sums`` measures every instance of one mask in a single kernel pass; ``mask_to_bbox`` is the
reference's function of that name on top of it, and ``validate/compare.py`` derives the per-instance statistics.
``instance_mesh_cells`` counts every instance's marching-cubes cells per class in one more pass.
``instance_meshes`` writes those meshes out: vertices and faces of every instance from a count and an emit pass
(DESIGN.md §24).
``instance_skeleton_graph`` thins every instance in its box and reads the skeletons as graphs.
``instance_skeleton_branches`` traces them into node and branch tables, or traces saved skeletons.
``instance_thickness`` is the exact distance transform of every instance and its maximum per instance.
``instance_local_thickness`` is the local thickness of every instance voxel and its distribution per instance
(DESIGN.md §28).
``instance_contacts`` says which instances touch and across how many shared faces, edges and corners, one row per pair
(DESIGN.md §29).
``instance_overlaps`` says which instance of one mask shares voxels with which instance of another, one row per pair;
``sparse_mask_iou`` is ``mask_iou`` on those pairs alone, the function the reference declares and leaves unwritten, and
``match_instances_sparse`` is ``match_instances`` on them.
``instance_proximity`` says which instances lie within a distance of each other, how close they come and how many voxels
of each lie that close, one row per pair; ``proximity_reach`` is the reach of a distance in voxels and ``plan_proximity``
the per-instance summary of the table.
``instance_intensity`` reads the image under every instance -- count, sums, extrema and a 256-bin histogram -- and
``intensity_ring`` the image over the background around it.
``instance_surfaces``, ``surface_distances``, ``match_instances`` and ``pair_summaries`` are the parts of
``validate/compare.py: compare()``: every instance's surface voxels as sorted keys, the exact squared distance from
every surface voxel of one instance to the surface of another for many pairs at once, the matching rule, and the
reduction to Hausdorff / ASSD / surface Dice.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _ffi


def _lut(mask: Tensor) -> Tuple[Tensor, Tensor, int]:
    ids = torch.unique(mask)
    ids = ids[ids > 0]                       # lib.py:201-205: sorted positive ids
    mx = int(ids.max().item()) if ids.numel() else 0
    lut = torch.zeros(mx + 1, dtype=torch.int32, device=mask.device)
    if ids.numel():
        lut[ids.long()] = torch.arange(1, ids.numel() + 1, dtype=torch.int32, device=mask.device)
    return ids, lut, mx


def mask_iou(gt: Tensor, pred: Tensor) -> Tensor:
    """(N, M) fp32 IoU of every ground-truth instance against every predicted one (rows / columns in ascending id
    order, 0 where they do not touch) -- skoots/validate/lib.py:190-229."""
    assert gt.shape == pred.shape, "Input tensors must be the same shape"
    assert gt.device == pred.device, "Input tensors must be on the same device"
    a = gt.to(torch.int32).contiguous()
    b = pred.to(torch.int32).contiguous()
    _ffi.require_gpu(a, "gt")
    ids_a, lut_a, max_a = _lut(a)
    ids_b, lut_b, max_b = _lut(b)
    N, M = int(ids_a.numel()), int(ids_b.numel())
    iou = torch.zeros((N, M), dtype=torch.float32, device=a.device)
    ws_bytes = int(_ffi.lib.sk_mask_iou_workspace_bytes(N, M))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    _ffi.check(_ffi.lib.sk_mask_iou(_ffi.ptr(a), _ffi.ptr(b), a.numel(), _ffi.ptr(lut_a), max_a, N, _ffi.ptr(lut_b), max_b, M,
                                    _ffi.ptr(iou), _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(a.device)))
    return iou


def _require_slices(t: Tensor, name: str) -> None:
    if t.ndim != 4 or t.shape[0] != 1:
        raise ValueError(f"{name} must be a (1, X, Y, Z) mask (the layout whose per-slice soft skeleton the "
                         f"reference computes), got shape {tuple(t.shape)}")


def _metrics(gt: Tensor, pred: Tensor, want_iou: bool, want_dice: bool, want_cldice: bool,
             iters: int = 3) -> Tuple[Tensor, Tensor, Tensor]:
    """One sk_mask_metrics call; the matrices not asked for come back as None."""
    assert gt.shape == pred.shape, "Input tensors must be the same shape"
    assert gt.device == pred.device, "Input tensors must be on the same device"
    _ffi.require_gpu(gt, "gt")
    if gt.numel() == 0:
        raise ValueError("mask_metrics: empty volume")
    if want_cldice:
        _require_slices(gt, "gt")
        X, Y, Z = (int(v) for v in gt.shape[1:])
    else:                                   # counts only: any shape, one line of voxels
        X, Y, Z = 1, 1, int(gt.numel())
    a = gt.to(torch.int32).contiguous()
    b = pred.to(torch.int32).contiguous()
    ids_a, lut_a, max_a = _lut(a)
    ids_b, lut_b, max_b = _lut(b)
    N, M = int(ids_a.numel()), int(ids_b.numel())
    out = [torch.empty((N, M), dtype=torch.float32, device=a.device) if w else None
           for w in (want_iou, want_dice, want_cldice)]
    ws_bytes = int(_ffi.lib.sk_mask_metrics_workspace_bytes(N, M))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    _ffi.check(_ffi.lib.sk_mask_metrics(_ffi.ptr(a), _ffi.ptr(b), X, Y, Z, _ffi.ptr(lut_a), max_a, N,
                                        _ffi.ptr(lut_b), max_b, M, iters, *(_ffi.ptr(o) for o in out),
                                        _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(a.device)))
    return tuple(out)


def mask_metrics(gt: Tensor, pred: Tensor, iters: int = 3) -> Tuple[Tensor, Tensor, Tensor]:
    """(iou, dice, cldice), each (N, M) fp32, from one pass over two (1, X, Y, Z) instance masks: ``mask_iou``,
    ``mask_dice`` and ``mask_soft_cldice`` of the reference (lib.py:190-315) with ``soft_cldice(iter_=iters)``."""
    return _metrics(gt, pred, True, True, True, iters)


def mask_dice(gt: Tensor, pred: Tensor) -> Tensor:
    """(N, M) fp32 Dice, ``float(2 |A & B|) / float(|A| + |B|)``, 0 where the instances do not touch --
    lib.py:232-273.  Deliberate difference: an instance identical to its match gives 1.0 where the reference's
    ``assert numerator < denominator`` raises."""
    return _metrics(gt, pred, False, True, False)[1]


def mask_soft_cldice(gt: Tensor, pred: Tensor) -> Tensor:
    """(N, M) fp32 soft-clDice LOSS ``1 - clDice`` (``soft_cldice()(pred == b, gt == a)``, iter_ 3, smooth 1) of
    every touching pair, 0 elsewhere -- lib.py:276-315.  gt and pred are (1, X, Y, Z): the skeleton is the
    reference's per-(Y, Z)-slice one and the x = 0 slice is out of the sums."""
    return _metrics(gt, pred, False, False, True)[2]


def label_soft_skeleton(labels: Tensor, iters: int = 3) -> Tensor:
    """(1, X, Y, Z) uint8: 1 where a voxel lies on the soft skeleton of its own instance, i.e. the union over ids
    a > 0 of ``soft_skeletonize((labels == a).float(), iters) > 0`` (train/loss.py:295-310, 4-D branch)."""
    _ffi.require_gpu(labels, "labels")
    _require_slices(labels, "labels")
    a = labels.to(torch.int32).contiguous()
    skel = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
    if a.numel() == 0:
        return skel
    _, X, Y, Z = (int(v) for v in a.shape)
    _ffi.check(_ffi.lib.sk_label_soft_skeleton2d(_ffi.ptr(a), X, Y, Z, iters, _ffi.ptr(skel),
                                                 _ffi.stream_ptr(a.device)))
    return skel


def accuracies_from_iou(iou: Tensor, thr: float = 0.1) -> Tuple[float, float, float]:
    """(true positives, false positives, false negatives) at an IoU threshold -- lib.py:170-187."""
    n, m = iou.shape
    gt_miss = torch.logical_not(iou.max(dim=1)[0].gt(thr)) if m > 0 else torch.ones(0)
    pred_miss = torch.logical_not(iou.max(dim=0)[0].gt(thr)) if n > 0 else torch.ones(0)
    tp = torch.sum(torch.logical_not(gt_miss))
    return tp.cpu().item(), torch.sum(pred_miss).cpu().item(), torch.sum(gt_miss).cpu().item()


def f1_score(tp, fp, fn):
    """lib.py:358-361."""
    return 2 * tp / (2 * tp + fp + fn)


def get_segmentation_errors(ground_truth: Tensor, predicted: Tensor) -> Tuple[float, float]:
    """(over-, under-segmentation rate): the share of ground-truth (predicted) instances that more than one
    predicted (ground-truth) instance overlaps with IoU > 0.2 -- lib.py:400-438."""
    iou = mask_iou(ground_truth, predicted)
    n, m = iou.shape
    over = (iou.gt(0.2).sum(dim=1) > 1).sum().item() / n
    under = (iou.gt(0.2).sum(dim=0) > 1).sum().item() / m
    return over, under


# ---- per-instance measurements ----

N_SUMS, N_BOX = 13, 6      # int64 / int32 values per instance of sk_instance_stats (checked against the library below)
_INT32_MAX = 2 ** 31 - 1


def check_shape(shape) -> None:
    """The library's guard, applied before any call: X Y Z max(X, Y, Z)^2 < 2^63 keeps the second moments in int64."""
    X, Y, Z = (int(v) for v in shape)
    if min(X, Y, Z) < 0 or max(X, Y, Z) > _INT32_MAX or X * Y * Z * max(X, Y, Z) ** 2 >= 2 ** 63:
        raise ValueError(f"a mask of shape {(X, Y, Z)} is too large to measure: X*Y*Z*max(X, Y, Z)^2 must stay below "
                         "2^63, or the second moments leave int64")


def _as_volume(x: Tensor, name: str) -> Tensor:
    """(X, Y, Z) view of an integer device tensor given as (X, Y, Z) or (1, X, Y, Z)."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError(f"{name} must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU "
                         "fallback")
    if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
        raise TypeError(f"{name} must have an integer dtype, got {x.dtype}")
    if x.ndim == 4 and x.shape[0] == 1:
        x = x[0]
    if x.ndim != 3:
        raise ValueError(f"{name} must be (X, Y, Z) or (1, X, Y, Z), got shape {tuple(x.shape)}")
    if x.dtype in (getattr(torch, n) for n in ("uint16", "uint32", "uint64") if hasattr(torch, n)):
        x = x.to(torch.int64)
    return x


def _id_rows(x: Tensor):
    """The prologue of the per-instance kernels: ``(a, ids, lut, max_id)`` for an (X, Y, Z) integer device tensor --
    ``a`` int32 contiguous, ``ids`` (N) int64 ascending, and the table that takes a value of ``a`` to its row 1..N --
    or ``None`` when x has no positive id.

    Ids reach the kernel through the ``_lut`` table, which has ``max id + 1`` entries; when the largest id exceeds four
    times the voxel count (or int32) the mask is relabelled through ``torch.unique(return_inverse=True)`` instead, so
    that a few huge ids do not allocate a huge table."""
    dev = x.device
    mx = int(x.max().item()) if x.numel() else 0
    if mx <= 0:
        return None
    if mx > 4 * x.numel() or mx > _INT32_MAX:
        u, inv = torch.unique(x, return_inverse=True)
        k = int((u <= 0).sum().item())                       # sorted: the non-positive values come first
        ids = u[k:].to(torch.int64)
        a = (inv - (k - 1)).clamp_(min=0).to(torch.int32).contiguous()    # the row itself
        lut = torch.arange(ids.numel() + 1, dtype=torch.int32, device=dev)
        max_id = int(ids.numel())
    else:
        a = x.to(torch.int32).contiguous()
        ids, lut, max_id = _lut(a)
        ids = ids.to(torch.int64)
    return a, ids, lut, max_id


def id_rows(x: Tensor):
    """``(volume, rows)`` of an integer device tensor (X, Y, Z) or (1, X, Y, Z): its (X, Y, Z) view and ``_id_rows`` of
    it.  ``instance_sums`` and ``instance_mesh_cells`` take the pair as ``rows=``, so a caller that runs both kernels
    on one mask pays for ``x.max()``, ``torch.unique`` and the table once."""
    x = _as_volume(x, "x")
    return x, _id_rows(x)


def check_voxels(shape) -> None:
    """X Y Z < 2^62: the library's guard where a pass keeps no sums over the voxels."""
    X, Y, Z = (int(v) for v in shape)
    if X * Y * Z >= 2 ** 62:
        raise ValueError(f"a mask of shape {(X, Y, Z)} is too large to measure: X*Y*Z must stay below 2^62")


class _Rows:
    """The prologue of every per-instance function, done once.  ``rows`` is the caller's ``id_rows(x)``; without it ``x``
    goes through ``_as_volume`` and ``_id_rows``.  ``guard`` is the function's size guard (``check_shape``,
    ``check_voxels``, ...): it sees the shape before anything touches the device.  ``nonnegative`` refuses a mask with a
    negative value.  ``x`` is the (X, Y, Z) view, ``shape`` its extents, ``dev`` its device, ``pair`` what to hand on
    as ``rows=``; ``a``, ``ids``, ``lut``, ``max_id`` are ``_id_rows``' and ``N`` the number of instances.  A mask
    without a positive id is ``empty``: N = 0, ``ids`` an empty tensor, no ``a`` and no ``lut``."""

    def __init__(self, x, rows=None, guard=None, name: str = "x", nonnegative: bool = False):
        x = _as_volume(x, name) if rows is None else rows[0]
        if guard is not None:
            guard(x.shape)
        if rows is None:
            if nonnegative and x.numel() and int(x.min().item()) < 0:
                raise ValueError(f"{name} holds the negative value {int(x.min().item())}: instance ids are positive and "
                                 "0 is the background")
            rows = (x, _id_rows(x))
        self.x, r = self.pair = rows
        self.shape = tuple(int(v) for v in x.shape)
        self.dev = x.device
        self.empty = r is None
        if self.empty:
            r = (None, torch.empty(0, dtype=torch.int64, device=self.dev), None, 0)
        self.a, self.ids, self.lut, self.max_id = r
        self.N = int(self.ids.numel())

    def call(self, fn, *args) -> None:
        """``fn(labels, X, Y, Z, lut, max_id, N, *args, stream)``, checked: the mask header every per-instance entry
        point of the library begins with, and the stream it ends with."""
        _ffi.check(fn(_ffi.ptr(self.a), *self.shape, _ffi.ptr(self.lut), self.max_id, self.N, *args,
                      _ffi.stream_ptr(self.dev)))

    def values(self) -> Tensor:
        """(N) int64: the value ``a`` holds for row k + 1 -- the id itself, or the row where ``_id_rows`` relabelled."""
        return torch.nonzero(self.lut)[:, 0]

    def row_volume(self) -> Tensor:
        """(X, Y, Z) int32: every voxel's row 1..N, 0 for the background and for negative values; int32 indices and
        results, so no 8-byte-per-voxel temporary."""
        return self.lut[self.a.clamp(min=0)]


def instance_sums(x: Tensor, rows=None) -> Tuple[Tensor, Tensor, Tensor]:
    """(ids (N) int64 ascending, sums (N, 13) int64, boxes (N, 6) int32) of the positive ids of an (X, Y, Z) integer
    device tensor: one ``sk_instance_stats`` launch for every instance (include/skoots_hip.h names the columns).
    ``_id_rows`` says how the ids reach the kernel; ``rows`` is ``id_rows(x)`` when the caller already has it."""
    assert _ffi.lib.sk_instance_stats_row_values(0) == N_SUMS and _ffi.lib.sk_instance_stats_row_values(1) == N_BOX
    m = _Rows(x, rows, check_shape)
    sums = torch.zeros((m.N, N_SUMS), dtype=torch.int64, device=m.dev)
    boxes = torch.zeros((m.N, N_BOX), dtype=torch.int32, device=m.dev)
    if not m.empty:
        m.call(_ffi.lib.sk_instance_stats, _ffi.ptr(sums), _ffi.ptr(boxes))
    return m.ids, sums, boxes


def instance_mesh_cells(x: Tensor, closed: bool = False, rows=None) -> Tuple[Tensor, Tensor]:
    """(ids (N) int64 ascending, cells (N, 30) int64) of the positive ids of an (X, Y, Z) integer device tensor: how
    many marching-cubes cells of each class of ``mc_table.CLASS_TRIANGLES`` every instance has, from one
    ``sk_instance_mesh_cells`` launch.  ``cells.double() @ class_areas(spacing)`` is the area of the
    mesh scikit-image's marching cubes gives ``x == id``.

    ``closed=False`` is the reference's meaning: the cells lie inside the volume, so a surface cut by a face of the
    volume stays open there.  ``closed=True`` measures the mask padded with one layer of background.  ``rows`` is
    ``id_rows(x)`` when the caller already has it."""
    from .mc_table import CLASS_OF, CLASS_TRIANGLES
    m = _Rows(x, rows, check_voxels)
    n_classes = len(CLASS_TRIANGLES)
    cells = torch.zeros((m.N, n_classes), dtype=torch.int64, device=m.dev)
    if not m.empty:
        class_of = torch.tensor(CLASS_OF, dtype=torch.uint8, device=m.dev)
        m.call(_ffi.lib.sk_instance_mesh_cells, _ffi.ptr(class_of), n_classes, int(bool(closed)), _ffi.ptr(cells))
    return m.ids, cells


CONTACT_CONNECTIVITIES = (6, 18, 26)
N_CONTACT = 9                  # int64 values per row of sk_instance_contacts: lo, hi, c0 .. c6
MAX_CONTACT_CAPACITY = 1 << 30


def _pow2_at_least(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


def instance_contacts(x: Tensor, connectivity: int = 6, background: bool = False, rows=None,
                      capacity=None) -> Tuple[Tensor, Tensor]:
    """(ids (N) int64 ascending, table (P, 9) int64) of the positive ids of an (X, Y, Z) integer device tensor: which
    instances touch and across how many voxel pairs, from ``sk_instance_contacts`` (include/skoots_hip.h has the
    definition).  A row of ``table`` is ``lo, hi, c0 .. c6``: two ROWS of ``ids`` (1 .. N; 0 is the
    background, which appears only with ``background=True``), ``lo < hi``, and the contacts between them by class --
    shared faces with the normal along x / y / z, shared edges in the xy / xz / yz planes, shared corners.
    ``connectivity`` 6 fills the faces, 18 the edges too, 26 all seven.  The table is sorted by ``(lo, hi)`` with
    torch, so two runs give equal tensors.  ``rows`` is ``id_rows(x)`` when the caller already has it.

    The kernel collects the pairs in a hash table of ``capacity`` slots, a power of two; ``None`` starts at the next
    power of two >= ``max(1024, 8 N)``, a given value is where the search STARTS.  After the launch the function reads
    the two counters back; if insertions were refused it runs again at the next power of two >=
    ``2 * (stored + refused)`` -- at least twice the distinct pairs, and never more than twice the pairs the mask can
    hold -- and raises ``RuntimeError`` rather than go past 2^30 slots."""
    assert _ffi.lib.sk_instance_contacts_row_values() == N_CONTACT
    if connectivity not in CONTACT_CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be one of {CONTACT_CONNECTIVITIES}, got {connectivity!r}")
    m = _Rows(x, rows, check_voxels)
    dev, N, (X, Y, Z) = m.dev, m.N, m.shape
    if m.empty:
        return m.ids, torch.empty((0, N_CONTACT), dtype=torch.int64, device=dev)
    if capacity is None:
        capacity = _pow2_at_least(max(1024, 8 * N))
    capacity = int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError(f"capacity must be a power of two >= 1, got {capacity}")
    most = min((N + 1) * N // 2, 13 * X * Y * Z)             # distinct pairs the mask can hold, background included
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    while True:
        if capacity > MAX_CONTACT_CAPACITY:
            raise RuntimeError(f"instance_contacts: the pair table would need {capacity} slots, more than 2^30")
        ws_bytes = int(_ffi.lib.sk_instance_contacts_workspace_bytes(capacity))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((capacity, N_CONTACT), dtype=torch.int64, device=dev)
        m.call(_ffi.lib.sk_instance_contacts, int(connectivity), int(bool(background)), _ffi.ptr(out), capacity,
               _ffi.ptr(counts), _ffi.ptr(ws), ws_bytes)
        stored, refused = (int(v) for v in counts.tolist())
        if refused == 0:
            break
        del ws, out
        capacity = max(2 * capacity, _pow2_at_least(2 * min(stored + refused, most)))
    table = out[:stored]
    order = torch.argsort(table[:, 0] * (N + 1) + table[:, 1])     # lo, hi <= N: one int64 key
    return m.ids, table[order].contiguous()


# ---- the instances of two masks against each other ----

N_OVERLAP = 3                  # int64 values per row of sk_instance_overlaps: ra, rb, voxels
MAX_OVERLAP_CAPACITY = 1 << 30


def instance_overlaps(a: Tensor, b: Tensor, background: bool = False, rows_a=None, rows_b=None,
                      capacity=None) -> Tuple[Tensor, Tensor, Tensor]:
    """(ids_a (N) int64 ascending, ids_b (M) int64 ascending, table (P, 3) int64) of two integer device tensors of one
    shape, (X, Y, Z) or (1, X, Y, Z): which instance of ``a`` shares voxels with which instance of ``b``, from
    ``sk_instance_overlaps`` (include/skoots_hip.h has the definition).  A row of ``table`` is
    ``ra, rb, voxels``: a ROW of ``ids_a`` (1 .. N), a row of ``ids_b`` (1 .. M) and the voxels that carry both.  With
    ``background=True`` the rows with exactly one side 0, the background, are there too, so that the rows of one
    instance sum to its voxel count; (0, 0) never is.  These are the nonzero entries of the (N + 1) x (M + 1)
    contingency table that ``mask_iou`` keeps densely.  The table is sorted by ``(ra, rb)`` with torch, so two runs give
    equal tensors.  ``rows_a`` / ``rows_b`` are ``id_rows(a)`` / ``id_rows(b)`` when the caller already has them.

    The kernel collects the pairs in a hash table of ``capacity`` slots, a power of two; ``None`` starts at the next
    power of two >= ``max(1024, 8 max(N, M))``, a given value is where the search STARTS.  After the launch the function
    reads the two counters back; if insertions were refused it runs again at the next power of two >=
    ``2 * (stored + refused)`` -- at least twice the distinct pairs, and never more than twice the
    ``min((N + 1)(M + 1) - 1, X Y Z)`` pairs two masks can hold -- and raises ``RuntimeError`` rather than go past 2^30
    slots.  Two masks of different shape or device raise ``ValueError``."""
    assert _ffi.lib.sk_instance_overlaps_row_values() == N_OVERLAP
    ma = _Rows(a, rows_a, check_voxels, name="a")
    mb = _Rows(b, rows_b, check_voxels, name="b")
    if ma.shape != mb.shape or ma.dev != mb.dev:
        raise ValueError(f"a {ma.shape} on {ma.dev} and b {mb.shape} on {mb.dev} must have one shape and one device")
    dev, N, M, (X, Y, Z) = ma.dev, ma.N, mb.N, ma.shape
    n = X * Y * Z
    if n == 0 or (N == 0 and M == 0) or (not background and (N == 0 or M == 0)):
        return ma.ids, mb.ids, torch.empty((0, N_OVERLAP), dtype=torch.int64, device=dev)
    if capacity is None:
        capacity = _pow2_at_least(max(1024, 8 * max(N, M)))
    capacity = int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError(f"capacity must be a power of two >= 1, got {capacity}")
    most = min((N + 1) * (M + 1) - 1, n)                     # distinct pairs two masks can hold, background included
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    while True:
        if capacity > MAX_OVERLAP_CAPACITY:
            raise RuntimeError(f"instance_overlaps: the pair table would need {capacity} slots, more than "
                               f"{MAX_OVERLAP_CAPACITY}")
        ws_bytes = int(_ffi.lib.sk_instance_overlaps_workspace_bytes(capacity))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((capacity, N_OVERLAP), dtype=torch.int64, device=dev)
        # a side without instances has no volume and no table here: the library reads it as background
        ma.call(_ffi.lib.sk_instance_overlaps, _ffi.ptr(mb.a), _ffi.ptr(mb.lut), mb.max_id, M, int(bool(background)),
                _ffi.ptr(out), capacity, _ffi.ptr(counts), _ffi.ptr(ws), ws_bytes)
        stored, refused = (int(v) for v in counts.tolist())
        if refused == 0:
            break
        del ws, out
        capacity = max(2 * capacity, _pow2_at_least(2 * min(stored + refused, most)))
    table = out[:stored]
    order = torch.argsort(table[:, 0] * (M + 1) + table[:, 1])     # ra <= N, rb <= M: one int64 key
    return ma.ids, mb.ids, table[order].contiguous()


def overlap_ious(table: Tensor, N: int, M: int) -> Tuple[Tensor, Tensor]:
    """(pairs (Q, 3) int64, values (Q) fp32) from the (P, 3) table of ``instance_overlaps(a, b, background=True)``: its
    rows between two instances, in the table's order, and the IoU of each -- ``(float)inter / (float)union`` in fp32, the
    expression of ``sk_mask_iou``'s kernel, with ``union = |a| + |b| - inter`` and the voxel counts ``|a|``, ``|b|`` the
    table's own row and column sums (that is why it needs the background rows).  The quotient is formed on the host:
    one correctly rounded fp32 division per pair, the same bits as the kernel's.  Host tensors in, host tensors out;
    device tensors in, device tensors out."""
    t = torch.as_tensor(table).to(torch.int64).reshape(-1, N_OVERLAP)
    size_a = torch.zeros(int(N) + 1, dtype=torch.int64, device=t.device).index_add_(0, t[:, 0], t[:, 2])
    size_b = torch.zeros(int(M) + 1, dtype=torch.int64, device=t.device).index_add_(0, t[:, 1], t[:, 2])
    pairs = t[(t[:, 0] > 0) & (t[:, 1] > 0)]
    inter = pairs[:, 2].cpu()
    union = (size_a[pairs[:, 0]] + size_b[pairs[:, 1]]).cpu() - inter
    values = inter.to(torch.float32) / union.to(torch.float32)
    return pairs, values.to(t.device)


def sparse_mask_iou(a: Tensor, b: Tensor) -> Tensor:
    """``mask_iou(a, b)`` as a coalesced ``torch.sparse_coo_tensor`` of shape (N, M), fp32: one stored value per pair of
    instances that share a voxel, and ``.to_dense()`` equal to ``mask_iou(a, b)`` bit for bit -- the function the
    reference declares under this name and leaves unwritten (skoots/validate/lib.py:317).  One ``instance_overlaps``
    pass with the background rows gives intersections and, as row and column sums, the voxel counts; nothing of size
    N x M is allocated."""
    ids_a, ids_b, table = instance_overlaps(a, b, background=True)
    N, M = int(ids_a.numel()), int(ids_b.numel())
    pairs, values = overlap_ious(table, N, M)
    # sorted by (ra, rb) and distinct: coalesce() finds nothing to add up
    return torch.sparse_coo_tensor((pairs[:, :2] - 1).t().contiguous(), values, (N, M)).coalesce()


def match_instances_sparse(table: Tensor, iou_values: Tensor, N: int, M: int, iou_threshold: float = 0.1) -> Tensor:
    """``match_instances`` on the pairs that exist: ``table`` (Q, >= 2) int64 holds a row 1 .. N and a row 1 .. M per
    pair (rows with a 0, the background, are ignored; a pair appears once) and ``iou_values`` (Q) its fp32 IoU, which is
    positive -- ``overlap_ious`` gives both.  Returns the (N) int64 result of ``match_instances(dense, iou_threshold)``
    for the (N, M) matrix that holds these values and 0 elsewhere: per row the column (0-based) of the largest value
    when that is > ``iou_threshold``, the lowest column on a tie, -1 otherwise.  A pure function of its tensors, on
    their device, host tensors included; N or M may be 0."""
    t = torch.as_tensor(table).to(torch.int64)
    t = t.reshape(-1, t.shape[-1] if t.ndim == 2 else N_OVERLAP)
    v = torch.as_tensor(iou_values).to(device=t.device, dtype=torch.float32).reshape(-1)
    N, M = int(N), int(M)
    if N == 0 or M == 0:
        return torch.full((N,), -1, dtype=torch.int64, device=t.device)
    keep = (t[:, 0] > 0) & (t[:, 1] > 0)
    r, c, v = t[keep, 0] - 1, t[keep, 1] - 1, v[keep]
    # a row without a pair is a row of zeros: its largest value is 0, first met in column 0
    best = torch.zeros(N, dtype=torch.float32, device=t.device).scatter_reduce_(0, r, v, "amax", include_self=True)
    first = torch.full((N,), M, dtype=torch.int64, device=t.device)
    first.scatter_reduce_(0, r, torch.where(v == best[r], c, c.new_tensor(M)), "amin", include_self=True)
    first = torch.where(best > 0, first, first.new_tensor(0))
    return torch.where(best > iou_threshold, first, first.new_tensor(-1))


# ---- instances within a distance of each other ----

N_PROXIMITY = 4                # int64 values per row of sk_instance_proximity: ra, rb, near_voxels, gap2_bits
MAX_PROXIMITY_CAPACITY = 1 << 30


def _proximity_metric(distance, spacing) -> Tuple[Tuple[float, float, float], float]:
    """((wx, wy, wz), limit2) of a distance and a spacing, as ``nearest_label`` forms them: the spacing squared and
    ``fl(d d)``; the distance must be a non-negative finite number whose square is finite."""
    from ..lib.morphology import max_distance_squared, squared_spacing
    w = squared_spacing(spacing)
    if distance is None:
        raise ValueError("distance must be a non-negative finite number, got None")
    try:
        limit2 = max_distance_squared(distance)
    except ValueError:
        raise ValueError(f"distance must be a non-negative finite number, got {distance!r}") from None
    if not limit2 < float("inf"):
        raise ValueError(f"distance must be a non-negative finite number with a finite square, got {distance!r}")
    return w, limit2


def _reach_query(w, limit2):
    out = np.zeros(8, dtype=np.int32)
    _ffi.check(_ffi.lib.sk_instance_proximity_reach(w[0], w[1], w[2], limit2, out.ctypes.data))
    return tuple(int(v) for v in out)


def proximity_reach(distance, spacing=(1.0, 1.0, 1.0)) -> Tuple[int, int, int]:
    """(hx, hy, hz): how many voxels ``distance`` reaches along every axis at ``spacing`` -- per axis the largest k with
    ``fl(w k^2) <= fl(d d)``, the library's own search (``sk_instance_proximity_reach``; a host function, no GPU).
    Raises ``ValueError`` when the kernel does not stage a window that large; the message names the distance below
    which it does at that spacing.  A reach is never truncated."""
    w, limit2 = _proximity_metric(distance, spacing)
    hx, hy, hz, taken = _reach_query(w, limit2)[:4]
    if taken:
        return hx, hy, hz
    # the reach grows where d passes a multiple of a spacing: the first such distance that is refused
    steps = sorted({wk * float(k * k) for wk in w for k in range(1, 257)})
    first = next((t for t in steps if t <= limit2 and not _reach_query(w, t)[3]), limit2)
    raise ValueError(f"distance {distance!r} reaches ({hx}, {hy}, {hz}) voxels at spacing {tuple(spacing)}, beyond the "
                     f"window the proximity kernel stages; at this spacing it takes every distance below "
                     f"{float(np.sqrt(first))!r}")


def instance_proximity(a: Tensor, b=None, distance=None, spacing=(1.0, 1.0, 1.0), rows_a=None, rows_b=None,
                       capacity=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(ids_a (N) int64 ascending, ids_b (M) int64 ascending, pairs (P, 3) int64, gap2 (P) float64) of two integer
    device tensors of one shape, (X, Y, Z) or (1, X, Y, Z): which instance of ``a`` lies within ``distance`` of which
    instance of ``b``, from ``sk_instance_proximity`` (include/skoots_hip.h has the definition).  A row
    of ``pairs`` is ``ra, rb, near_voxels``: a ROW of ``ids_a`` (1 .. N), a row of ``ids_b`` (1 .. M) and the voxels of
    ``ra`` that have a voxel of ``rb`` within the distance (``<=``; centre to centre at ``spacing``); ``gap2`` is the
    smallest squared distance between the two, 0 where they overlap.  The rows with ``rb = 0`` are the union rows: the
    voxels of ``ra`` within the distance of ANY instance of ``b``, and the smallest squared distance to one.  Only the
    voxels of ``a`` are counted; swap the masks for the other side -- ``gap2`` is the same from both.  ``b=None`` is
    the one-mask mode: ``a`` against itself, an instance never its own partner.  Sorted by ``(ra, rb)`` with torch, so
    two runs give equal tensors.  ``rows_a`` / ``rows_b`` are ``id_rows(a)`` / ``id_rows(b)`` when the caller has them.

    ``distance`` must be within ``proximity_reach``; the capacity and its retry are ``instance_overlaps``'.  Two masks
    of different shape or device raise ``ValueError``."""
    assert _ffi.lib.sk_instance_proximity_row_values() == N_PROXIMITY
    ma = _Rows(a, rows_a, check_voxels, name="a")
    same = b is None
    mb = ma if same else _Rows(b, rows_b, check_voxels, name="b")
    if ma.shape != mb.shape or ma.dev != mb.dev:
        raise ValueError(f"a {ma.shape} on {ma.dev} and b {mb.shape} on {mb.dev} must have one shape and one device")
    w, limit2 = _proximity_metric(distance, spacing)
    proximity_reach(distance, spacing)
    dev, N, M, (X, Y, Z) = ma.dev, ma.N, mb.N, ma.shape
    n = X * Y * Z
    if n == 0 or N == 0 or M == 0:
        return (ma.ids, mb.ids, torch.empty((0, 3), dtype=torch.int64, device=dev),
                torch.empty((0,), dtype=torch.float64, device=dev))
    if capacity is None:
        capacity = _pow2_at_least(max(1024, 8 * max(N, M)))
    capacity = int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError(f"capacity must be a power of two >= 1, got {capacity}")
    most = min(N * (M + 1), n * (M + 1))                     # distinct keys, the union rows included
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    while True:
        if capacity > MAX_PROXIMITY_CAPACITY:
            raise RuntimeError(f"instance_proximity: the pair table would need {capacity} slots, more than "
                               f"{MAX_PROXIMITY_CAPACITY}")
        ws_bytes = int(_ffi.lib.sk_instance_proximity_workspace_bytes(capacity))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((capacity, N_PROXIMITY), dtype=torch.int64, device=dev)
        ma.call(_ffi.lib.sk_instance_proximity, _ffi.ptr(mb.a), _ffi.ptr(mb.lut), mb.max_id, M, *w, limit2, int(same),
                _ffi.ptr(out), capacity, _ffi.ptr(counts), _ffi.ptr(ws), ws_bytes)
        stored, refused = (int(v) for v in counts.tolist())
        if refused == 0:
            break
        del ws, out
        capacity = max(2 * capacity, _pow2_at_least(2 * min(stored + refused, most)))
    table = out[:stored]
    table = table[torch.argsort(table[:, 0] * (M + 1) + table[:, 1])]     # ra <= N, rb <= M: one int64 key
    return ma.ids, mb.ids, table[:, :3].contiguous(), table[:, 3].contiguous().view(torch.float64)


def plan_proximity(pairs, gap2, N: int, M: int) -> Dict[str, np.ndarray]:
    """What the table of ``instance_proximity`` says about every row 1 .. N of ``a``, numpy in and numpy out:
    ``partners`` (N) int64, the instances of ``b`` within the distance; ``nearest_row`` (N) int64, the one with the
    smallest ``gap2`` and on a tie the lowest row, 0 without a partner; ``nearest_gap2`` (N) float64, that gap, ``inf``
    without a partner; ``near_voxels`` (N) int64, the union row's count.  ``pairs`` is (P, 3), ``gap2`` (P)."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    g = np.asarray(gap2, dtype=np.float64).reshape(-1)
    N, M = int(N), int(M)
    if p.shape[0] != g.shape[0]:
        raise ValueError(f"pairs has {p.shape[0]} rows and gap2 {g.shape[0]} values")
    if p.shape[0] and (p[:, 0].min() < 1 or p[:, 0].max() > N or p[:, 1].min() < 0 or p[:, 1].max() > M):
        raise ValueError(f"pairs holds rows outside 1 .. {N} of a or 0 .. {M} of b")
    partners, near_voxels = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    nearest_row, nearest_gap2 = np.zeros(N + 1, np.int64), np.full(N + 1, np.inf)
    union = p[:, 1] == 0
    near_voxels[p[union, 0]] = p[union, 2]
    q, qg = p[~union], g[~union]
    np.add.at(partners, q[:, 0], 1)
    order = np.lexsort((q[:, 1], qg, q[:, 0]))[::-1]         # the last write wins: smallest gap, then lowest row
    nearest_row[q[order, 0]] = q[order, 1]
    nearest_gap2[q[order, 0]] = qg[order]
    return {"partners": partners[1:], "nearest_row": nearest_row[1:], "nearest_gap2": nearest_gap2[1:],
            "near_voxels": near_voxels[1:]}


# ---- the image under every instance ----

N_MOMENTS, N_EXTREMA, N_BINS = 6, 2, 256       # values per instance of sk_instance_intensity (checked against the library)
_SIGNED_IMAGE_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64)


def _volume_shape(x):
    """(X, Y, Z) of a tensor given as (X, Y, Z) or (1, X, Y, Z), or None when it is neither"""
    if not isinstance(x, Tensor):
        return None
    s = tuple(int(v) for v in x.shape)
    s = s[1:] if len(s) == 4 and s[0] == 1 else s
    return s if len(s) == 3 else None


def check_image(image, shape) -> None:
    """What an image must be to be measured under a mask of ``shape`` (X, Y, Z), checked on the tensor's description
    alone, before any device is touched: a tensor of dtype uint8 or uint16, or of a signed integer dtype (its values
    are checked later), of shape (X, Y, Z) or (1, X, Y, Z).  Floating, bool and complex images raise ``TypeError``: the
    measurement is exact integer work, and that is the contract."""
    if not isinstance(image, Tensor):
        raise TypeError(f"image must be a tensor, got {type(image).__name__}")
    if image.dtype not in (torch.uint8, getattr(torch, "uint16", torch.uint8)) + _SIGNED_IMAGE_DTYPES:
        raise TypeError(f"image must be uint8 or uint16 (or a signed integer dtype with values in 0 .. 65535), got "
                        f"{image.dtype}: intensities are measured in exact integer arithmetic")
    got = _volume_shape(image)
    if got is None or got != tuple(int(v) for v in shape):
        raise ValueError(f"image has the shape {tuple(image.shape)}, the mask {tuple(int(v) for v in shape)}: the image "
                         "must be (X, Y, Z) or (1, X, Y, Z) with the mask's extents")


def check_intensity_shape(shape, elem_bytes: int) -> None:
    """The guard of ``sk_instance_intensity``, applied before any call: with V = 255 or 65535 the largest sample,
    X Y Z V max(V, X, Y, Z) < 2^63 keeps every sum in int64."""
    X, Y, Z = (int(v) for v in shape)
    V = 255 if elem_bytes == 1 else 65535
    if min(X, Y, Z) < 0 or max(X, Y, Z) > _INT32_MAX or X * Y * Z * V * max(V, X, Y, Z) >= 2 ** 63:
        raise ValueError(f"a mask of shape {(X, Y, Z)} is too large to measure a {8 * elem_bytes}-bit image under: "
                         f"X*Y*Z*V*max(V, X, Y, Z) with V = {V} must stay below 2^63, or the sums leave int64")


def _as_image(image: Tensor, shape, device):
    """(samples, elem_bytes, largest sample or None) of a checked image: the (X, Y, Z) contiguous uint8 or uint16 device
    tensor the kernel reads.  A signed image is checked to lie in 0 .. 65535 and converted (int8 to uint8)."""
    check_image(image, shape)
    if image.device != device:
        raise ValueError(f"image is on {image.device} and the mask on {device}: both must be on one device")
    img = image[0] if image.ndim == 4 else image
    top = None
    if img.dtype in _SIGNED_IMAGE_DTYPES:
        if img.numel():
            low, top = int(img.min().item()), int(img.max().item())
            if low < 0 or top > 65535:
                raise ValueError(f"image is {img.dtype} with values in {low} .. {top}: only 0 .. 65535 can be measured")
        img = img.to(torch.uint8 if img.dtype == torch.int8 else torch.uint16)
    return img.contiguous(), int(img.element_size()), top


def _image_shift(img: Tensor, elem_bytes: int, top, shift) -> int:
    """The histogram's bin shift: 0 for 8-bit samples; for 16-bit samples the caller's, or the smallest one that brings
    the largest sample below 256 (one pass over the image, through its int16 bit patterns with the sign bit flipped)"""
    if shift is not None and (isinstance(shift, bool) or int(shift) != shift or not 0 <= int(shift) <= 8):
        raise ValueError(f"shift must be an integer in 0 .. 8, got {shift!r}")
    if elem_bytes == 1:
        if shift not in (None, 0):
            raise ValueError(f"shift must be 0 for an 8-bit image, got {shift}")
        return 0
    if shift is not None:
        return int(shift)
    if top is None:
        top = int((img.view(torch.int16) ^ -32768).max().item()) + 32768 if img.numel() else 0
    return max(int(top).bit_length() - 8, 0)


def _check_shift(extrema: Tensor, shift: int) -> None:
    """A given shift is held against the largest sample the pass itself found under an instance: the kernel books a
    sample beyond the last bin in the last bin, and quantiles read from that would be wrong without a word"""
    top = int(extrema[:, 1].max().item()) if extrema.numel() else -1
    if top >> shift >= N_BINS:
        raise ValueError(f"shift = {shift} leaves the sample {top} outside the {N_BINS} bins: it needs at least "
                         f"{max(top.bit_length() - 8, 0)}")


def _intensity_launch(m: _Rows, img, elem_bytes, shift, want_hist):
    """(moments, extrema, hist or None) of the image under the rows of ``m``; empty tables for an empty mask"""
    moments = torch.zeros((m.N, N_MOMENTS), dtype=torch.int64, device=m.dev)
    extrema = torch.zeros((m.N, N_EXTREMA), dtype=torch.int32, device=m.dev)
    hist = torch.zeros((m.N, N_BINS), dtype=torch.int64, device=m.dev) if want_hist else None
    if not m.empty:
        m.call(_ffi.lib.sk_instance_intensity, _ffi.ptr(img), elem_bytes, shift, _ffi.ptr(moments), _ffi.ptr(extrema),
               _ffi.ptr(hist))
    return moments, extrema, hist


def instance_intensity(x: Tensor, image: Tensor, rows=None, want_hist: bool = True, shift=None):
    """(ids (N) int64 ascending, moments (N, 6) int64, extrema (N, 2) int32, hist (N, 256) int64 or None, shift) of the
    positive ids of an (X, Y, Z) integer device tensor and an image of the same shape on the same device: the image
    under every instance from one ``sk_instance_intensity`` launch (include/skoots_hip.h names the columns; DESIGN.md
    §30).  ``moments`` is ``n, S v, S v^2, S v x, S v y, S v z`` with x, y, z the voxel indices, ``extrema`` the smallest
    and largest sample, ``hist`` the voxels per bin ``v >> shift``.  ``x`` and ``rows`` are ``instance_sums``'.

    ``image`` is uint8 or uint16, (X, Y, Z) or (1, X, Y, Z); a signed integer image whose values all lie in 0 .. 65535
    is converted; floating, bool and complex images raise ``TypeError`` (``check_image``).  ``shift=None`` is 0 for an
    8-bit image and the smallest shift with ``image.max() >> shift < 256`` for a 16-bit one, which costs a pass over the
    image; a given shift that leaves a sample under an instance outside the 256 bins raises ``ValueError`` after the
    launch.  ``want_hist=False`` skips the histogram work and returns ``None``
    for it.  An empty mask returns empty tables."""
    L = _ffi.lib
    assert [L.sk_instance_intensity_row_values(k) for k in range(3)] == [N_MOMENTS, N_EXTREMA, N_BINS]
    shape = _volume_shape(rows[0] if rows is not None else x)
    if shape is not None:
        check_image(image, shape)                            # before anything touches the device
    # the guard before anything touches the device; a signed image is measured as what _as_image makes of it
    m = _Rows(x, rows, lambda s: check_intensity_shape(s, 1 if image.dtype in (torch.uint8, torch.int8) else 2))
    img, elem_bytes, top = _as_image(image, m.shape, m.dev)
    given = shift is not None
    shift = _image_shift(img, elem_bytes, top, shift)
    moments, extrema, hist = _intensity_launch(m, img, elem_bytes, shift, bool(want_hist))
    if given and want_hist:
        _check_shift(extrema, shift)
    return m.ids, moments, extrema, hist, shift


def intensity_ring(x: Tensor, image: Tensor, distance, spacing=(1.0, 1.0, 1.0), rows=None) -> Tuple[Tensor, Tensor]:
    """(moments (N, 6) int64, extrema (N, 2) int32) of the image over the RING of every instance: the voxels with a mask
    value <= 0 whose nearest instance it is, as ``lib.morphology.nearest_label(x, spacing, max_distance=distance)``
    decides it, its tie rule included.  The same kernel as ``instance_intensity`` measures the ring
    volume, without a histogram.  The rows are those of the mask's N instances; an instance with an empty ring has
    ``n = 0`` (and the extrema ``INT32_MAX`` / -1).  ``distance`` is a positive finite number in the units of
    ``spacing``; ``rows`` is ``id_rows(x)`` when the caller already has it."""
    from ..lib.morphology import nearest_label
    try:
        d = float(distance)
    except (TypeError, ValueError):
        d = float("nan")
    if isinstance(distance, bool) or not (0.0 < d < float("inf")):
        raise ValueError(f"distance must be a positive finite number, got {distance!r}")
    shape = _volume_shape(rows[0] if rows is not None else x)
    if shape is not None:
        check_image(image, shape)
    m = _Rows(x, rows)
    x, ids, N = m.x, m.ids, m.N
    img, elem_bytes, _ = _as_image(image, m.shape, m.dev)
    check_intensity_shape(m.shape, elem_bytes)
    if not m.empty:
        nearest = nearest_label(x, spacing, d, None, m.pair)[0]
        ring = torch.where(x > 0, torch.zeros_like(nearest), nearest)
        del nearest
        # ids -> rows 1 .. N (every non-zero value of the ring is one of ids), 0 stays 0
        ring = torch.where(ring > 0, torch.searchsorted(ids, ring) + 1, torch.zeros_like(ring)).to(torch.int32).contiguous()
        m = _Rows(None, (ring, (ring, ids, torch.arange(N + 1, dtype=torch.int32, device=m.dev), N)))
    return _intensity_launch(m, img, elem_bytes, 0, False)[:2]


MESH_BUDGET = 4 << 30          # bytes of vertex and triangle records instance_meshes may ask for
_VERTEX_BYTES, _TRIANGLE_BYTES = 16, 40       # a record of sk_instance_mesh_emit: 2 and 5 int64


def packed_triangle_table() -> np.ndarray:
    """(256) uint64: ``mc_triangles.TRIANGLES`` as ``sk_instance_mesh_count`` / ``_emit`` read it -- bits 4 i .. 4 i + 3
    hold edge number i % 3 of triangle i / 3, bits 60 .. 63 the number of triangles."""
    from .mc_triangles import TRIANGLES
    out = np.zeros(256, np.uint64)
    for c, tris in enumerate(TRIANGLES):
        v = len(tris) << 60
        for j, t in enumerate(tris):
            for i, e in enumerate(t):
                v |= e << (4 * (3 * j + i))
        out[c] = v
    return out


def _mesh_prologue(x: Tensor, rows, ids):
    """(x, rows, (X, Y, Z)) for the mesh kernels, the shape checked; with ``ids`` the look-up table of ``rows`` is
    replaced by one in which every other instance is background and the chosen ones are the rows 1..len(ids), ascending."""
    x, rows = id_rows(x) if rows is None else rows
    X, Y, Z = (int(v) for v in x.shape)
    if X * Y * Z >= 2 ** 62 or (X + 2) * (Y + 2) * (Z + 2) >= 2 ** 60:
        raise ValueError(f"a mask of shape {(X, Y, Z)} is too large to mesh: X*Y*Z must stay below 2^62 and "
                         "(X+2)*(Y+2)*(Z+2) below 2^60")
    if ids is not None:
        want = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        want = torch.unique(want).to(x.device)               # ascending
        if want.numel() == 0:
            return x, None, (X, Y, Z)
        have = rows[1] if rows is not None else want.new_empty(0)
        at = torch.searchsorted(have, want).clamp_(max=max(int(have.numel()) - 1, 0))
        if have.numel() == 0 or not bool((have[at] == want).all()):
            missing = want.tolist() if have.numel() == 0 else want[have[at] != want].tolist()
            raise ValueError(f"ids {missing} are not in the mask")
        m = _Rows(None, (x, rows))
        sub = torch.zeros_like(m.lut)                        # every other instance is background
        sub[m.values()[at]] = torch.arange(1, want.numel() + 1, dtype=torch.int32, device=x.device)
        rows = (m.a, want, sub, m.max_id)
    return x, rows, (X, Y, Z)


def instance_mesh_counts(x: Tensor, closed: bool = True, rows=None, ids=None) -> Tuple[Tensor, Tensor]:
    """(ids (N) int64 ascending, counts (N, 2) int64): vertices and triangles of the marching-cubes mesh of every
    instance, from one ``sk_instance_mesh_count`` launch.  The arguments are ``instance_meshes``'."""
    x, rows, _ = _mesh_prologue(x, rows, ids)
    m = _Rows(None, (x, rows))
    counts = torch.zeros((m.N, 2), dtype=torch.int64, device=m.dev)
    if not m.empty:
        table = torch.from_numpy(packed_triangle_table().view(np.int64)).to(m.dev)
        m.call(_ffi.lib.sk_instance_mesh_count, _ffi.ptr(table), int(bool(closed)), _ffi.ptr(counts))
    return m.ids, counts


def instance_meshes(x: Tensor, closed: bool = True, rows=None, ids=None,
                    budget_bytes: int = MESH_BUDGET) -> Dict[str, Tensor]:
    """The marching-cubes mesh of every instance of an (X, Y, Z) integer device tensor -- what scikit-image's
    ``marching_cubes((x == id) * 255)`` gives each id, vertices welded -- from two kernel passes over the mask
    (``sk_instance_mesh_count``, ``sk_instance_mesh_emit``).  Device tensors:

    ``ids`` (N) int64 ascending; ``vertices`` (V, 3) int32 in DOUBLED index coordinates (every vertex is the midpoint
    of two neighbouring voxels: twice its x, y, z are integers, and -1 occurs in closed mode); ``faces`` (F, 3) int32,
    indices LOCAL to the instance; ``vertex_offsets`` and ``face_offsets`` (N + 1) int64: instance k owns
    ``vertices[vertex_offsets[k]:vertex_offsets[k + 1]]`` and likewise its faces.

    Canonical order, the same on every run: instances ascending by id; within one, vertices ascending by edge key (x,
    then y, then z of the edge's low voxel, then the axis) and faces ascending by order key (x, y, z of the cell, then
    the triangle's place in ``mc_triangles.TRIANGLES``); each face keeps scikit-image's vertex order, whose right-hand
    normal points INTO the object.

    ``closed=True`` meshes the mask padded with one layer of background, so every surface is closed; ``closed=False``
    is the reference's meaning (``instance_mesh_cells``).  ``rows`` is ``id_rows(x)`` when the caller has it.  ``ids``
    meshes only those instances: the others are background to the kernels, and each result equals that instance's
    slice of the full result.  The kernels emit records that carry edge keys; the sort by (row, key) and the
    look-up that turns keys into local indices are torch calls on the device.

    Raises ``ValueError`` before anything is allocated when the count pass shows that the records would exceed
    ``budget_bytes`` (16 bytes per vertex, 40 per triangle; sorting needs about as much again), or when
    N * 8 * (X+2)(Y+2)(Z+2) reaches 2^63 and the sort keys would leave int64."""
    x, rows, (X, Y, Z) = _mesh_prologue(x, rows, ids)
    m = _Rows(None, (x, rows))
    dev, N = m.dev, m.N
    padded = (X + 2) * (Y + 2) * (Z + 2)
    if N * 8 * padded >= 2 ** 63:
        raise ValueError(f"{N} instances in a mask of shape {(X, Y, Z)}: N * 8 * (X+2)(Y+2)(Z+2) = {N * 8 * padded} "
                         "must stay below 2^63 for the sort keys; mesh fewer instances at a time with ids=[...]")
    ids_out, counts = instance_mesh_counts(x, closed, m.pair)
    out = {"ids": ids_out}
    V, F = (int(v) for v in counts.sum(0).tolist()) if N else (0, 0)
    need = V * _VERTEX_BYTES + F * _TRIANGLE_BYTES
    if need > int(budget_bytes):
        raise ValueError(f"the meshes have {V} vertices and {F} triangles: {need} bytes of records, more than "
                         f"budget_bytes = {int(budget_bytes)}; mesh fewer instances at a time with ids=[...], or raise "
                         "the budget")
    if V >= 2 ** 31:
        raise ValueError(f"the meshes have {V} vertices; indices are int32: mesh fewer instances at a time with "
                         "ids=[...]")
    zeros = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if V == 0:
        out.update(vertices=torch.empty((0, 3), dtype=torch.int32, device=dev),
                   faces=torch.empty((0, 3), dtype=torch.int32, device=dev), vertex_offsets=zeros,
                   face_offsets=zeros.clone())
        return out
    vrec = torch.empty((V, 2), dtype=torch.int64, device=dev)
    trec = torch.empty((F, 5), dtype=torch.int64, device=dev)
    produced = torch.zeros(2, dtype=torch.int64, device=dev)
    table = torch.from_numpy(packed_triangle_table().view(np.int64)).to(dev)
    m.call(_ffi.lib.sk_instance_mesh_emit, _ffi.ptr(table), int(bool(closed)), _ffi.ptr(vrec), V, _ffi.ptr(trec), F,
           _ffi.ptr(produced))
    if produced.tolist() != [V, F]:
        raise RuntimeError(f"sk_instance_mesh_emit produced {produced.tolist()} records where the count pass gave "
                           f"{[V, F]}")
    # canonical order: (row, edge key) and (row, order key) as one int64 each
    vkey = torch.sort((vrec[:, 0] - 1) * (3 * padded) + vrec[:, 1])[0]
    torder = torch.argsort((trec[:, 0] - 1) * (8 * padded) + trec[:, 4])
    trec = trec[torder]
    voff = torch.cat((zeros[:1], torch.cumsum(counts[:, 0], 0)))
    foff = torch.cat((zeros[:1], torch.cumsum(counts[:, 1], 0)))
    trow = trec[:, 0] - 1
    glob = torch.searchsorted(vkey, (trow[:, None] * (3 * padded) + trec[:, 1:4]).contiguous())
    if not bool((vkey[glob.clamp(max=V - 1)] == trow[:, None] * (3 * padded) + trec[:, 1:4]).all()):
        raise RuntimeError("sk_instance_mesh_emit: a triangle names a vertex that was not emitted")
    faces = (glob - voff[trow][:, None]).to(torch.int32)
    key = vkey % (3 * padded)
    axis, vox = key % 3, key // 3
    px, py, pz = vox // ((Y + 2) * (Z + 2)), vox // (Z + 2) % (Y + 2), vox % (Z + 2)
    vertices = torch.stack((px, py, pz), 1) * 2 - 2           # the padded index is the coordinate + 1
    vertices[torch.arange(V, device=dev), axis] += 1
    out.update(vertices=vertices.to(torch.int32), faces=faces, vertex_offsets=voff, face_offsets=foff)
    return out


SKELETON_BUDGET = 1 << 30   # bytes of thinning workspace per batch of instance_skeleton_graph
N_GRAPH = 12                # int64 values per instance of sk_skeleton_graph (lib/morphology.py checks the library's)


def _skeleton_batches(boxes: np.ndarray, budget_bytes: int):
    """[(first, last + 1)] over the rows of ``boxes`` (N, 6) int32, in row order: each batch is the longest run whose
    ``sk_skeletonize_workspace_bytes`` stays within ``budget_bytes``, and an instance that alone exceeds the budget is
    its own batch.  The bytes grow with the run, so the end of a run is found by bisection."""
    def nbytes(a, b):
        return int(_ffi.lib.sk_skeletonize_workspace_bytes(boxes[a:b].ctypes.data_as(_ffi.ip), b - a))

    out, a, n = [], 0, boxes.shape[0]
    while a < n:
        lo, hi = a + 1, n                                    # the run [a, lo) is taken in any case
        if nbytes(a, hi) > budget_bytes:
            while lo < hi:                                   # the largest b in [lo, hi] with nbytes(a, b) <= budget
                mid = (lo + hi + 1) // 2
                if nbytes(a, mid) <= budget_bytes:
                    lo = mid
                else:
                    hi = mid - 1
            hi = lo
        out.append((a, hi))
        a = hi
    return out


def _thinning_boxes(m: "_Rows", boxes):
    """``(boxes (N, 6) int32 [x0, x1 + 1) on the host, values (N) int32)`` for the thinning of every instance of ``m``:
    the inclusive boxes of ``instance_sums`` (computed when ``boxes`` is ``None``) opened by one, refused with
    ``ValueError`` and the instance's id where the library would refuse the crop, and the value ``m.a`` holds per row."""
    ids, N = m.ids, m.N
    if boxes is None:
        boxes = instance_sums(m.x, m.pair)[2]
    b = boxes.cpu().numpy().astype(np.int64).reshape(N, N_BOX)
    b[:, 3:] += 1                                            # inclusive -> [x0, x1 + 1)
    ext = b[:, 3:] - b[:, :3]
    words = (ext[:, 0] + 2) * (ext[:, 1] + 2) * ((ext[:, 2] + 2 + 31) >> 5)
    refused = np.flatnonzero((ext.prod(1) >= 2 ** 30) | (words * 6 >= 2 ** 31))     # the guard of sk_skeletonize
    if refused.size:
        i = int(refused[0])
        raise ValueError(f"instance {int(ids[i].item())} has a box of {tuple(int(v) for v in ext[i])} voxels, too large "
                         "to thin: a crop must stay below 2^30 voxels (and 2^31 / 6 words of padded bit plane)")
    b = np.ascontiguousarray(b.astype(np.int32))
    values = m.values().to(torch.int32).cpu().numpy()
    assert values.shape[0] == N
    return b, values


def instance_skeleton_graph(x: Tensor, rows=None, boxes=None, budget_bytes: int = SKELETON_BUDGET,
                            want_volume: bool = False):
    """(ids (N) int64 ascending, graph (N, 12) int64[, skeleton (X, Y, Z) int32]) of the positive ids of an (X, Y, Z)
    integer device tensor: every instance is Lee-thinned in its full box ``[x0, x1 + 1) x ...`` with other ids as
    background -- ``skimage.morphology.skeletonize_3d(x == id)`` of scikit-image 0.18.3 on the whole volume -- and
    ``sk_skeleton_graph`` reads the skeleton as a graph: its voxels, the voxels of degree 0 / 1 / 2 / >= 3 and the
    links per direction class (include/skoots_hip.h names the columns).  ``ids`` and the rows are those
    of ``instance_sums``; ``rows`` is ``id_rows(x)`` and ``boxes`` the (N, 6) inclusive boxes of ``instance_sums`` when
    the caller already has them.

    The instances are thinned in batches, in row order, of at most ``budget_bytes`` of thinning workspace (an instance
    that alone needs more is a batch of its own); the result does not depend on the budget.  A box whose crop the
    library refuses (2^30 voxels or more, or 2^31 / 6 words of padded bit plane) raises ``ValueError`` with the
    instance's id before anything is launched.  ``want_volume`` adds a volume that is 0 outside the skeletons and the
    instance's row (1 .. N) on its skeleton voxels."""
    from ..lib.morphology import skeleton_graph
    m = _Rows(x, rows, check_shape)
    a, ids, N, dev = m.a, m.ids, m.N, m.dev
    volume = torch.zeros(m.shape, dtype=torch.int32, device=dev) if want_volume else None
    if m.empty:
        out = (ids, torch.empty((0, N_GRAPH), dtype=torch.int64, device=dev))
        return out + (volume,) if want_volume else out
    b, values = _thinning_boxes(m, boxes)
    graph = torch.empty((N, N_GRAPH), dtype=torch.int64, device=dev)
    for first, last in _skeleton_batches(b, int(budget_bytes)):
        g, counts, points = skeleton_graph(a, values[first:last], b[first:last], want_points=want_volume)
        graph[first:last] = g
        if want_volume and points.shape[0]:
            row = torch.repeat_interleave(torch.arange(first, last, device=dev),
                                          torch.from_numpy(counts).to(dev))
            p = points.long() + torch.from_numpy(b[first:last, :3]).to(dev).long()[row - first]
            volume[p[:, 0], p[:, 1], p[:, 2]] = (row + 1).to(torch.int32)
    return (ids, graph, volume) if want_volume else (ids, graph)


N_NODE, N_BRANCH = 8, 18     # int32 values per row of the node and branch tables (lib/morphology.py checks the library's)


def instance_skeleton_branches(x: Tensor, rows=None, boxes=None, budget_bytes: int = SKELETON_BUDGET, skeleton=None):
    """``(ids, graph, nodes, branches, points, owner)`` of the positive ids of an (X, Y, Z) integer device tensor: every
    instance thinned as in ``instance_skeleton_graph`` and its skeleton traced into nodes and branches
    (``lib.morphology.skeleton_branches``; include/skoots_hip.h states the definitions).

    ``ids`` (N) int64 ascending and ``graph`` (N, 12) int64 are those of ``instance_skeleton_graph``.  ``nodes`` (Nn, 8)
    and ``branches`` (Nb, 18) int32 are the library's tables with column 0 the instance's index into ``ids`` and the
    node rows of a branch counted over the whole table; ``points`` (P, 3) int32 the skeleton voxels in volume
    coordinates, instance by instance in (x, y, z) order, and ``owner`` (P) int32 a chain voxel's branch row or -1 - the
    node row of a node voxel.  All device tensors.  The instances go in the batches of ``instance_skeleton_graph``; rows
    are rebased across them, so the result does not depend on ``budget_bytes``.

    ``skeleton`` is an (X, Y, Z) integer device volume that holds an instance's id on its skeleton voxels and 0
    elsewhere, the kind ``--save-skeletons`` writes: it is traced as it is, inside every instance's box, and nothing is
    thinned (thinning is the slow part).  Ids that ``x`` does not have are ignored."""
    from ..lib.morphology import skeleton_branches
    m = _Rows(x, rows, check_shape)
    a, ids, N, dev = m.a, m.ids, m.N, m.dev
    empty = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    if m.empty:
        return (ids, torch.empty((0, N_GRAPH), dtype=torch.int64, device=dev), empty(0, N_NODE), empty(0, N_BRANCH),
                empty(0, 3), empty(0))
    b, values = _thinning_boxes(m, boxes)
    if skeleton is not None:
        skeleton = _as_volume(skeleton, "skeleton")
        if tuple(skeleton.shape) != m.shape or skeleton.device != dev:
            raise ValueError(f"skeleton must be a {m.shape} volume on {dev}, got shape {tuple(skeleton.shape)} on "
                             f"{skeleton.device}")
        # into the values of `a`: the id itself, or its row where _id_rows relabelled
        at = torch.searchsorted(ids, skeleton.to(torch.int64).clamp(min=0)).clamp_(max=N - 1)
        a = torch.where(ids[at] == skeleton, torch.from_numpy(values).to(dev)[at], 0).to(torch.int32).contiguous()
    graph = torch.empty((N, N_GRAPH), dtype=torch.int64, device=dev)
    parts = ([], [], [], [])
    n_nodes = n_branches = 0
    for first, last in _skeleton_batches(b, int(budget_bytes)):
        g, counts, points, nodes, branches, owner = skeleton_branches(a, values[first:last], b[first:last],
                                                                      thin=skeleton is None)
        graph[first:last] = g
        nodes[:, 0] += first
        branches[:, 0] += first
        branches[:, 1:3] += n_nodes
        owner = torch.where(owner >= 0, owner + n_branches, owner - n_nodes)
        which = torch.repeat_interleave(torch.arange(last - first, device=dev), torch.from_numpy(counts).to(dev))
        points = points + torch.from_numpy(b[first:last, :3]).to(dev)[which]
        n_nodes, n_branches = n_nodes + int(nodes.shape[0]), n_branches + int(branches.shape[0])
        for part, t in zip(parts, (nodes, branches, points, owner)):
            part.append(t)
    if max(n_nodes, n_branches) >= 2 ** 31:
        raise ValueError(f"{n_nodes} nodes and {n_branches} branches: rows are int32")
    nodes, branches, points, owner = (torch.cat(part) for part in parts)
    return ids, graph, nodes, branches, points, owner


def instance_thickness(x: Tensor, spacing=(1.0, 1.0, 1.0), closed: bool = False, rows=None, skeleton=None):
    """(ids (N) int64 ascending, max_d2 (N) float64, dist2 (X, Y, Z) float64[, skeleton_stats (N, 3) float64 on the
    host]) of the positive ids of an (X, Y, Z) integer device tensor: ``lib.morphology.label_edt`` -- the exact squared
    distance of every instance voxel to the nearest voxel that is not of its instance, at the voxel spacing -- and its
    largest value per instance, the squared radius of the largest sphere around a voxel centre that holds voxel centres
    of the instance only.  ``closed`` and ``rows`` are those of ``label_edt``; in open mode an instance
    that is alone in the volume has ``inf``.

    ``skeleton`` is the (X, Y, Z) int32 row volume of ``instance_skeleton_graph(..., want_volume=True)``; with it the
    mean, minimum and maximum of ``sqrt(dist2)`` over every instance's skeleton voxels follow as a host tensor.  The
    values are gathered on the device in raster order (``nonzero``), copied, and reduced per row in row-then-raster
    order with numpy, so the mean is the same on every run (a plain left-to-right sum over the count, kept inside
    [minimum, maximum]); a row without skeleton voxels has 0.0 in all three columns (no real radius is 0)."""
    from ..lib.morphology import label_edt
    m = _Rows(x, rows)
    ids, N = m.ids, m.N
    if skeleton is not None and (tuple(skeleton.shape) != m.shape or skeleton.device != m.dev):
        raise ValueError(f"skeleton must be the {m.shape} row volume of instance_skeleton_graph on {m.dev}, got "
                         f"shape {tuple(skeleton.shape)} on {skeleton.device}")
    dist2, max_d2 = label_edt(m.x, spacing, closed, m.pair)
    if skeleton is None:
        return ids, max_d2, dist2
    at = torch.nonzero(skeleton.reshape(-1))[:, 0]           # raster order
    row = skeleton.reshape(-1)[at].cpu().numpy().astype(np.int64)
    radius = np.sqrt(dist2.reshape(-1)[at].cpu().numpy())
    order = np.argsort(row, kind="stable")                   # row, then raster
    row, radius = row[order], radius[order]
    stats = np.zeros((N, 3), np.float64)
    first = np.searchsorted(row, np.arange(1, N + 2))
    for r in range(N):
        v = radius[first[r]:first[r + 1]]
        if v.size:
            total = 0.0
            for t in v.tolist():                             # a plain left-to-right sum: one order, whatever numpy does
                total += t
            # rounding can put the mean of equal values a unit outside them: keep it inside [min, max]
            stats[r] = (min(max(total / v.size, v.min()), v.max()), v.min(), v.max())
    return ids, max_d2, dist2, torch.from_numpy(stats)


def instance_local_thickness(x: Tensor, spacing=(1.0, 1.0, 1.0), closed: bool = False, rows=None, dist2=None):
    """(ids (N) int64 ascending, table (K, 3) int64 on the host, thick2 (X, Y, Z) float64, max_d2 (N) float64) of the
    positive ids of an (X, Y, Z) integer device tensor: ``lib.morphology.local_thickness`` -- for every instance voxel
    the squared radius of the largest ball inside its instance that holds it -- and its distribution per
    instance.  ``closed`` and ``rows`` are those of ``label_edt``; ``dist2`` is the pair ``(dist2, max_d2)`` of
    ``label_edt`` / ``instance_thickness`` in the same mode when the caller already has it.

    ``table`` has one row per (instance, distinct value): ``(row 1..N, the value's float64 bit pattern, voxels)``, sorted
    by row and then by value (non-negative doubles order like their bit patterns).  It is built on the device from
    integers only -- ``unique`` of the foreground bit patterns with the inverse, then ``unique`` with counts of
    ``row * n_values + inverse`` -- so it is exact and the same on every run; ``compare.local_thickness_columns`` turns
    it into the columns on the host."""
    from ..lib.morphology import local_thickness
    m = _Rows(x, rows)
    thick2, _, max_d2 = local_thickness(m.x, spacing, closed, m.pair, dist2)
    if m.empty:
        return m.ids, np.zeros((0, 3), np.int64), thick2, max_d2
    row = m.row_volume().reshape(-1).long()
    fg = torch.nonzero(row)[:, 0]
    values, inverse = torch.unique(thick2.reshape(-1)[fg].view(torch.int64), return_inverse=True)
    n_values = int(values.numel())
    keys, counts = torch.unique(row[fg] * n_values + inverse, return_counts=True)
    table = torch.stack((torch.div(keys, max(n_values, 1), rounding_mode="floor"), values[keys % max(n_values, 1)],
                         counts), 1)
    return m.ids, table.cpu().numpy().astype(np.int64), thick2, max_d2


# ---- compare(): surfaces, matching and surface distances ----

# Pair evaluations (queries x targets, before pruning) one ``sk_surface_distances`` launch may be asked for.  The work
# of a call has no bound of its own -- one instance with 10^7 surface voxels against its twin is 10^14 evaluations --
# so ``surface_distances`` splits the pair list, and the queries of a very large pair, into launches of at most this
# many.  The value is meant to keep a launch well under a second.  It was chosen on an estimate of 1e12 evaluations
# per second and has since been held against one measurement (tools/bench_compare.py on one MI355X,
# profiles/compare_bench.json): a pair of 2^19 x 2^19 voxels in which no tile can be pruned, four launches of 2^36, ran
# at 1.86e12 evaluations per second, 37 ms a launch; that is the worst case, and pruning only shortens it.  The value stays; the result
# does not depend on it.
LAUNCH_BUDGET = 1 << 36
_MAX_EXTENT = 1 << 26


def _require_device(t, name: str, dtype) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU "
                         "fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def instance_surfaces(x: Tensor, rows=None) -> Tuple[Tensor, Tensor, Tensor]:
    """(ids (N) int64 ascending, offsets (N + 1) int64, keys int64) of the positive ids of an (X, Y, Z) integer device
    tensor: the surface voxels of every instance -- the voxels of the instance with a face neighbour that is not,
    outside the volume included (scipy: ``m & ~binary_erosion(m)``) -- as surface keys
    ``row * X Y Z + ((x Y + y) Z + z)``, row 0-based, sorted ascending: instance k owns
    ``keys[offsets[k]:offsets[k + 1]]``, its voxels in x-major order.  One count pass, one emit pass
    (``sk_instance_surface_count``, ``sk_instance_surface_emit``) and one ``torch.sort``.  ``rows`` is ``id_rows(x)``
    when the caller already has it."""
    m = _Rows(x, rows)
    dev, N, (X, Y, Z) = m.dev, m.N, m.shape
    if m.empty:
        return m.ids, torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    if max(X, Y, Z) > _MAX_EXTENT or N * X * Y * Z >= 2 ** 63:
        raise ValueError(f"{N} instances in a mask of shape {(X, Y, Z)}: every extent must stay within 2^26 and "
                         "N*X*Y*Z below 2^63, or the surface keys leave int64")
    counts = torch.zeros(N, dtype=torch.int64, device=dev)
    m.call(_ffi.lib.sk_instance_surface_count, _ffi.ptr(counts))
    total = int(counts.sum().item())
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    produced = torch.zeros(1, dtype=torch.int64, device=dev)
    m.call(_ffi.lib.sk_instance_surface_emit, total, _ffi.ptr(keys), _ffi.ptr(produced))
    if int(produced.item()) != total:
        raise RuntimeError(f"sk_instance_surface_emit produced {int(produced.item())} keys where the count pass gave "
                           f"{total}")
    keys = torch.sort(keys)[0]
    offsets = torch.cat((counts.new_zeros(1), torch.cumsum(counts, 0)))
    return m.ids, offsets, keys


def _launches(qo: np.ndarray, to: np.ndarray, pairs: np.ndarray, budget: int):
    """The launches of ``surface_distances``: a list of (q_begin, q_end, target segment) int64 arrays, in output order.
    A pair of more than ``budget`` evaluations is cut into runs of ``budget // targets`` queries (at least one); the
    items are then packed greedily, in order, into launches of at most ``budget`` evaluations (an item that alone
    exceeds it -- one query against more than ``budget`` targets -- is a launch of its own).

    A query segment may appear in several pairs -- a prediction that several ground-truth instances chose -- and be cut
    differently in each, or not at all.  The query segments of a launch are the offsets refined by ALL its cuts, so
    every item of a launch is finally split at every cut of that launch that falls inside it: each item is then exactly
    one of the launch's segments.  Splitting an item changes neither the evaluations nor the order of the outputs."""
    items = []
    for qs, ts in pairs.tolist():
        qb, qe, nt = int(qo[qs]), int(qo[qs + 1]), max(int(to[ts + 1] - to[ts]), 1)
        per = qe - qb if (qe - qb) * nt <= budget else max(1, budget // nt)
        for b in range(qb, qe, max(per, 1)):
            items.append((b, min(b + per, qe), ts, (min(b + per, qe) - b) * nt))
    out, cur, cost = [], [], 0
    for it in items:
        if cur and cost + it[3] > budget:
            out.append(cur)
            cur, cost = [], 0
        cur.append(it)
        cost += it[3]
    if cur:
        out.append(cur)
    launches = []
    for launch in out:
        cuts = np.unique(np.array([v for it in launch for v in it[:2]], np.int64))
        qb, qe, ts = [], [], []
        for b, e, t, _ in launch:
            at = [b, *cuts[np.searchsorted(cuts, b, "right"):np.searchsorted(cuts, e, "left")].tolist(), e]
            qb += at[:-1]
            qe += at[1:]
            ts += [t] * (len(at) - 1)
        launches.append(tuple(np.array(v, np.int64) for v in (qb, qe, ts)))
    return launches


def surface_distances(query, target, pairs, shape, spacing=(1.0, 1.0, 1.0)) -> Tuple[Tensor, Tensor]:
    """(out_offsets (P + 1) int64, d2 float64), device tensors: for pair k = (query segment, target segment) of
    ``pairs`` ((P, 2) integers, 0-based), ``d2[out_offsets[k] + i]`` is the exact squared distance, at the voxel
    ``spacing``, from the i-th voxel of the query segment to the nearest voxel of the target segment (``inf`` for an
    empty one) -- ``sk_surface_distances``, DESIGN.md §25.  ``query`` and ``target`` are results of
    ``instance_surfaces`` of masks of ``shape`` (X, Y, Z), or their ``(offsets, keys)``.  The pairs, and the queries
    of a very large pair, are split into launches of at most ``LAUNCH_BUDGET`` evaluations; the result does not depend
    on the split."""
    q_off, q_keys = (_require_device(t, f"query[{k - 2}]", torch.int64) for k, t in enumerate(query[-2:]))
    t_off, t_keys = (_require_device(t, f"target[{k - 2}]", torch.int64) for k, t in enumerate(target[-2:]))
    dev = q_keys.device
    X, Y, Z = (int(v) for v in shape)
    sx, sy, sz = (float(v) for v in spacing)
    if not all(np.isfinite(v) and v > 0 for v in (sx, sy, sz)):
        raise ValueError(f"spacing must be three positive numbers (x, y, z), got {spacing}")
    w = (sx * sx, sy * sy, sz * sz)
    p = torch.as_tensor(pairs).cpu().to(torch.int64).reshape(-1, 2).numpy()
    qo, to = q_off.cpu().numpy(), t_off.cpu().numpy()
    if qo.size < 1 or to.size < 1 or np.any(np.diff(qo) < 0) or np.any(np.diff(to) < 0) or qo[0] < 0 or to[0] < 0:
        raise ValueError("offsets must be non-negative, monotone and have one entry more than segments")
    if qo[-1] > q_keys.numel() or to[-1] > t_keys.numel():
        raise ValueError("offsets reach beyond the keys")
    if p.size and (p.min() < 0 or p[:, 0].max() >= qo.size - 1 or p[:, 1].max() >= to.size - 1):
        raise ValueError(f"pairs must name segments in [0, {qo.size - 1}) x [0, {to.size - 1})")
    n_q = qo[p[:, 0] + 1] - qo[p[:, 0]] if p.size else np.zeros(0, np.int64)
    out = np.concatenate((np.zeros(1, np.int64), np.cumsum(n_q, dtype=np.int64)))
    d2 = torch.empty(int(out[-1]), dtype=torch.float64, device=dev)
    done = 0
    for qb, qe, ts in _launches(qo, to, p, int(LAUNCH_BUDGET)):
        # the launch's own query segments: the offsets refined by the cuts, so that they stay monotone
        breaks = np.unique(np.concatenate((qo, qb, qe)))
        seg = np.searchsorted(breaks, qb)
        if not np.array_equal(breaks[seg + 1], qe):
            raise RuntimeError("surface_distances: an item of a launch is not one of the launch's query segments")
        lp = torch.from_numpy(np.stack((seg, ts), 1).astype(np.int32)).to(dev)
        lo = np.concatenate((np.zeros(1, np.int64), np.cumsum(qe - qb, dtype=np.int64)))
        lq, lo_dev, part = torch.from_numpy(breaks).to(dev), torch.from_numpy(lo).to(dev), d2[done:]   # alive over the call
        _ffi.check(_ffi.lib.sk_surface_distances(
            _ffi.ptr(q_keys), _ffi.ptr(lq), int(breaks.size - 1), _ffi.ptr(t_keys), _ffi.ptr(t_off), int(to.size - 1),
            _ffi.ptr(lp), int(lp.shape[0]), _ffi.ptr(lo_dev), X, Y, Z, *w, _ffi.ptr(part), _ffi.stream_ptr(dev)))
        done += int(lo[-1])
    if done != int(out[-1]):
        raise RuntimeError(f"surface_distances: the launches wrote {done} of {int(out[-1])} distances")
    return torch.from_numpy(out).to(dev), d2


def match_instances(iou: Tensor, iou_threshold: float = 0.1) -> Tensor:
    """(N) int64, on the matrix's device: for every row of the (N, M) IoU matrix the column with the largest value when
    that value is > ``iou_threshold`` (strictly, as ``accuracies_from_iou``), the lowest such column on a tie, and -1
    otherwise.  Several rows may name one column: an under-segmentation shows as such.  A pure function of the matrix;
    N or M may be 0."""
    iou = torch.as_tensor(iou)
    n, m = (int(v) for v in iou.shape)
    if n == 0 or m == 0:
        return torch.full((n,), -1, dtype=torch.int64, device=iou.device)
    best = iou.max(dim=1)[0]
    cols = torch.arange(m, dtype=torch.int64, device=iou.device)
    first = torch.where(iou == best[:, None], cols[None, :], cols.new_tensor(m)).min(dim=1)[0]
    return torch.where(best > iou_threshold, first, first.new_tensor(-1))


def nearest_rank(n: int, percent: int = 95) -> int:
    """0-based index of the nearest-rank percentile of n ascending values: ceil(percent n / 100) - 1, in integers"""
    return (percent * n + 99) // 100 - 1


def pair_summaries(out_offsets: Tensor, d2: Tensor, n_g: int, tolerance2: float) -> Dict[str, Tensor]:
    """The surface-distance columns of ``n_g`` matched pairs (host tensors) from the squared distances of both
    directions: ``out_offsets`` (2 n_g + 1) and ``d2`` hold the ground-truth -> prediction distances of the pairs as
    segments 0 .. n_g - 1 and the prediction -> ground-truth ones as segments n_g .. 2 n_g - 1.  With dg / dp the
    ASCENDING ``sqrt`` of a pair's two segments:

    ``hausdorff`` = max(dg[-1], dp[-1]); ``hausdorff95`` = max of the nearest-rank 95th percentiles,
    ``d[ceil(0.95 n) - 1]``, one of the values themselves; ``assd`` = (sum dg + sum dp) / (|dg| + |dp|), each sum taken
    left to right over the ascending values in float64, so it is the same on every run; ``nsd`` = the share of the
    |dg| + |dp| squared distances that are <= ``tolerance2``, from integer counts; ``gt_surface_voxels`` and
    ``pred_surface_voxels`` (int64) = |dg| and |dp|.  An empty segment makes the pair's floats ``nan``.

    The segmented sort is two stable ``torch.sort`` calls on the tensors' device (by value, then by segment); the sums
    are numpy's ``cumsum`` on the host, which adds strictly left to right."""
    n_g = int(n_g)
    off = out_offsets.cpu().to(torch.int64)
    if off.numel() != 2 * n_g + 1:
        raise ValueError(f"out_offsets has {off.numel()} entries, {n_g} pairs in two directions need {2 * n_g + 1}")
    counts = off.diff().to(d2.device)
    seg = torch.repeat_interleave(torch.arange(2 * n_g, device=d2.device), counts)
    within = torch.bincount(seg[d2 <= tolerance2], minlength=2 * n_g).cpu().numpy() if n_g else np.zeros(0, np.int64)
    v, order = torch.sort(d2, stable=True)
    v = v[torch.sort(seg[order], stable=True)[1]]            # ascending inside every segment
    # numpy's square root is the correctly rounded one at every length of the array (compare.thickness_columns)
    d = np.sqrt(v.cpu().numpy())
    off = off.numpy()
    n = np.diff(off)
    out = {k: np.full(n_g, np.nan) for k in ("hausdorff", "hausdorff95", "assd", "nsd")}
    for k in range(n_g):
        ng, npr = int(n[k]), int(n[n_g + k])
        if ng == 0 or npr == 0:
            continue
        dg, dp = d[off[k]:off[k + 1]], d[off[n_g + k]:off[n_g + k + 1]]
        out["hausdorff"][k] = max(dg[-1], dp[-1])
        out["hausdorff95"][k] = max(dg[nearest_rank(ng)], dp[nearest_rank(npr)])
        out["assd"][k] = (np.cumsum(dg)[-1] + np.cumsum(dp)[-1]) / (ng + npr)
        out["nsd"][k] = int(within[k] + within[n_g + k]) / (ng + npr)
    res = {k: torch.from_numpy(a) for k, a in out.items()}
    res["gt_surface_voxels"] = torch.from_numpy(n[:n_g].astype(np.int64))
    res["pred_surface_voxels"] = torch.from_numpy(n[n_g:].astype(np.int64))
    return res


def mask_to_bbox(mask: Tensor) -> Tuple[Tensor, Tensor]:
    """(unique positive ids (N), boxes (6, N) as [x0, y0, z0, x1, y1, z1], inclusive) of a (1, X, Y, Z) instance mask
    -- skoots/validate/lib.py:12-54, from the one-pass kernel instead of one Python iteration per instance.
    Deliberate difference: the boxes are int32; the reference's int16 wraps beyond 32 767."""
    assert mask.ndim == 4, "Mask ndim != 4"
    ids, _, boxes = instance_sums(mask)
    return ids.to(mask.dtype), boxes.t().contiguous()
