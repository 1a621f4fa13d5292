"""``python -m skoots_amd.validate --ground_truth G --predicted P [--log 0-4]``: scores a predicted instance mask
against a ground-truth one, the reference's ``skoots-validate`` (skoots/validate/__main__.py:19-152).

Both masks are read as (1, X, Y, Z) int32 and cropped to ``[:, 50:-50, 50:-50, 5:-5]``.  One ``mask_metrics`` pass
gives the IoU, Dice and soft-clDice matrices; the segmentation rates come from the same IoU matrix.  It writes
``<P without extension>_accuracy_stats.csv`` and ``..._intersection_over_union.csv`` with the reference's text,
and the precision / recall / F1 plots when matplotlib is importable.
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

# Whether the masks are read by tiff.read_stack on the device or on the host and uploaded.
READ_ON_DEVICE = False

_LOG_LEVELS = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.validate",
                                     description="SKOOTS validation: instance-mask accuracy statistics")
    parser.add_argument("--ground_truth", type=str, required=True, help="Path to ground truth instance mask")
    parser.add_argument("--predicted", type=str, required=True, help="Path to predicted instance mask")
    parser.add_argument("--log", type=int, default=3, choices=range(5),
                        help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    return parser.parse_args(argv)


def load_mask(path: str, device=None) -> Tensor:
    """(C = 1, X, Y, Z) int32 tensor from a .tif or .npy stored [Z, X, Y(, C)] (validate/utils.py:8-26): on the host, or
    with ``device`` read by ``tiff.read_stack`` (deflate strips are inflated on the device; permute and cast happen
    there) -- the same values either way."""
    if device is not None:
        from ..lib.tiff import read_stack
        t = read_stack(path, device)
        t = t.unsqueeze(-1) if t.ndim == 3 else t
        t = t.permute(3, 1, 2, 0)
        t = t[[2], ...] if t.shape[0] > 3 else t
        if t.dtype == torch.uint16:   # through the bit pattern: int16 storage holds the uint16 values
            return (t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF)
        return t.contiguous().to(torch.int32)
    from ..lib.eval import _read_image
    image = _read_image(path)
    image = image[..., np.newaxis] if image.ndim == 3 else image
    image = image.transpose(-1, 1, 2, 0)
    image = image[[2], ...] if image.shape[0] > 3 else image
    return torch.from_numpy(np.ascontiguousarray(image).astype(np.int32))


def crop(mask: Tensor) -> Tensor:
    """The command's border crop (__main__.py:62-63); an empty result is an error, not a later crash."""
    out = mask[:, 50:-50, 50:-50, 5:-5]
    if out.numel() == 0:
        raise ValueError(f"a mask of shape {tuple(mask.shape)} leaves nothing after the [:, 50:-50, 50:-50, 5:-5] "
                         "crop: X and Y must exceed 100 and Z must exceed 10")
    return out.contiguous()


def segmentation_errors(iou: Tensor) -> Tuple[float, float]:
    """get_segmentation_errors (lib.py:400-438) on an IoU matrix already computed."""
    n, m = iou.shape
    over = (iou.gt(0.2).sum(dim=1) > 1).sum().item() / n
    under = (iou.gt(0.2).sum(dim=0) > 1).sum().item() / m
    return over, under


def accuracy_curves(iou: Tensor):
    """(tp, fp, fn) per threshold 0.00 .. 0.99, with precision, recall and F1 (__main__.py:86-89)."""
    from .lib import accuracies_from_iou, f1_score
    tfp = [accuracies_from_iou(iou, thr / 100) for thr in range(100)]
    precision = [(tp / (tp + fp)) for (tp, fp, fn) in tfp]
    recall = [(tp / (tp + fn)) for (tp, fp, fn) in tfp]
    f1 = [f1_score(*a) for a in tfp]
    return tfp, precision, recall, f1


def format_reports(gt_path: str, pred_path: str, iou: Tensor, dice: Tensor, cldice: Tensor,
                   gt_ids: Sequence[int]) -> Tuple[str, str]:
    """The text of ``_accuracy_stats.csv`` and ``_intersection_over_union.csv`` (__main__.py:122-152) from host
    copies of the three (N, M) matrices, with the reference's torch calls so that every float prints the same.
    ``gt_ids`` are the N positive ground-truth ids in ascending order (the matrix rows); a per-label row follows
    them whether or not the ground truth has background (the reference indexes ``i - 1`` of ``gt.unique()``)."""
    iou, dice, cldice = (t.detach().cpu() for t in (iou, dice, cldice))
    n, m = iou.shape
    if n == 0 or m == 0:
        raise ValueError(f"no {'ground-truth' if n == 0 else 'predicted'} instances inside the crop: "
                         "precision and recall are undefined")
    if len(gt_ids) != n or dice.shape != (n, m) or cldice.shape != (n, m):
        raise ValueError("format_reports: matrices and ids disagree in shape")
    over, under = segmentation_errors(iou)
    tfp, precision, recall, f1 = accuracy_curves(iou)
    acc: List[str] = [f"Ground Truth File: {gt_path}\n", f"Predicted File: {pred_path}\n",
                      f"Over Segmentation Rate: {over}\n", f"Under Segmentation Rate: {under}\n",
                      "thr,true_positive,false_positive,false_negative,precision,recall,f1\n"]
    for i, ((tp, fp, fn), _precision, _recall, _f1) in enumerate(zip(tfp, precision, recall, f1)):
        acc.append(f"{i / 100},{tp},{fp},{fn},{_precision},{_recall},{_f1}\n")
    tab: List[str] = [f"Ground Truth File: {gt_path}\n", f"Predicted File: {pred_path}\n",
                      f"Average IOU: {iou.max(1)[0].mean().item()}\n",
                      f"Average Dice: {dice.max(1)[0].mean().item()}\n",
                      f"Average clDice: {cldice.max(1)[0].mean().item()}\n",
                      "gt_label,best_iou,best_dice,best_cldice\n"]
    for i, u in enumerate(gt_ids):
        tab.append(f"{int(u)},{iou[i, :].max().item()},{dice[i, :].max().item()},{cldice[i, :].max().item()}\n")
    return "".join(acc), "".join(tab)


def _plots(base: str, precision, recall, f1) -> None:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logging.warning("matplotlib is not importable: the precision / recall / F1 plots were skipped")
        return
    _x = np.arange(0, 100)
    # the reference titles the recall plot "Precision" (__main__.py:107); kept
    for values, title, suffix in ((precision, "Precision", "precision"), (recall, "Precision", "recall"),
                                  (f1, "F1 Score", "f1")):
        plt.figure()
        plt.plot(_x, values, "k-")
        plt.title(title)
        plt.xlabel("Threshold (%)")
        plt.ylabel("Score")
        plt.tight_layout()
        plt.savefig(f"{base}_{suffix}.png", dpi=300)
        plt.close()


def main(argv: Optional[Sequence[str]] = None) -> Tuple[str, str]:
    """Runs the command; returns the paths of the two CSV files."""
    args = parse_args(argv)
    logging.basicConfig(level=_LOG_LEVELS[args.log],
                        format="[%(asctime)s] skoots-validate [%(levelname)s]: %(message)s")
    gt_path, pred_path = args.ground_truth, args.predicted
    if not (os.path.exists(gt_path) and os.path.exists(pred_path)):
        raise RuntimeError(f"{os.path.exists(gt_path)=}, {os.path.exists(pred_path)=}")
    base = os.path.splitext(pred_path)[0]
    dev = "cuda" if READ_ON_DEVICE else None
    gt, pred = crop(load_mask(gt_path, dev)), crop(load_mask(pred_path, dev))
    logging.debug(f"Ground Truth Shape: {gt.shape}, Predicted Shape: {pred.shape}")
    if gt.shape != pred.shape:
        raise ValueError(f"ground truth {tuple(gt.shape)} and prediction {tuple(pred.shape)} differ in shape")

    from .lib import mask_metrics           # the HIP library: no CPU fallback
    print("Calculating Instance Intersection over Union, Dice and clDice...")
    gt_dev, pred_dev = gt.to("cuda"), pred.to("cuda")
    iou, dice, cldice = mask_metrics(gt_dev, pred_dev)
    ids = torch.unique(gt_dev)
    gt_ids = ids[ids > 0].cpu().tolist()

    print("Calculating Accuracy Statistics...")
    acc_text, iou_text = format_reports(gt_path, pred_path, iou, dice, cldice, gt_ids)
    _, precision, recall, f1 = accuracy_curves(iou.cpu())
    _plots(base, precision, recall, f1)

    print("Writing File...")
    acc_path, iou_path = f"{base}_accuracy_stats.csv", f"{base}_intersection_over_union.csv"
    with open(acc_path, "w") as file:
        file.write(acc_text)
    print(f"File Written: {acc_path}")
    with open(iou_path, "w") as file:
        file.write(iou_text)
    print(f"File Written: {iou_path}")
    return acc_path, iou_path


if __name__ == "__main__":
    main()
