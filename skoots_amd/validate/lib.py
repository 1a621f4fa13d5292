"""Validation metrics (reference: skoots/validate/lib.py:170-315,358-438).

``mask_iou``, ``mask_dice`` and ``mask_soft_cldice`` are the heavy part -- the reference loops over every
ground-truth instance in Python and forms full-volume masks (and, for clDice, two soft skeletons) per touching
pair; here one kernel pass builds the (gt, pred) contingency tables and a second one turns them into the matrices
(``mask_metrics`` gives all three from one pass).  The bookkeeping on the small matrix
(``accuracies_from_iou``, ``f1_score``, ``get_segmentation_errors``) is host logic on its values.
"""
from __future__ import annotations

from typing import Tuple

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
