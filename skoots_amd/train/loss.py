"""Loss functions of the training step (reference: skoots/train/loss.py).

The two losses the reference registers for a config's three terms (train/engine.py:44-47,
``_valid_loss_functions``) are built: ``tversky`` (the defaults' choice for all three terms,
skoots/config.py:49-59) and ``soft_dice_cldice`` (soft Dice + soft clDice over a soft skeleton).
The training step itself uses the fused kernels behind ``engine.TrainStep``; these are the
reference's stand-alone callables with the same constructors and call signatures, and
``loss_from_cfg`` builds one from a config's name / keyword / value lists (engine.py:315-335).
"""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _ffi


class tversky:
    """``tversky(alpha, beta, eps)(predicted, ground_truth)`` (train/loss.py:95-212).

    predicted (B, 1, X, Y, Z) probabilities; ground_truth (B, 1, X, Y, Z), 0 = background (the
    reference's callers pass ``masks.gt(0).float()``, engine.py:468).  Per sample
    1 - (TP + eps) / (TP + alpha (FP + 1e-10) + beta FN + eps), then the batch mean.  Value only.

    Every non-zero value of ground_truth counts as one foreground (sk_train_tversky, ``!= 0``).  The reference
    expands a ground truth that holds several ids into one mask per id (train/loss.py:175-182), so the two agree
    for binary ground truth only -- pass ``masks.gt(0)`` as the reference's callers do.  The fused step
    (``fused_loss``, sk_train_loss) counts ``> 0``: a negative value is background there and foreground here.
    tests/test_hip_train_loss.py pins both rules.
    """

    def __init__(self, alpha: float, beta: float, eps: float):
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)

    def __call__(self, predicted: Tensor, ground_truth: Tensor) -> Tensor:
        if predicted.ndim != 5 or predicted.shape[1] != 1 or predicted.shape != ground_truth.shape:
            raise ValueError("tversky: predicted and ground_truth must both be (B, 1, X, Y, Z)")
        p = predicted.float().contiguous()
        g = ground_truth.float().contiguous()
        _ffi.require_gpu(p, "predicted")
        _ffi.require_gpu(g, "ground_truth")
        B = p.shape[0]
        n = p[0].numel()
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        ws = torch.empty(int(_ffi.lib.sk_train_loss_workspace_floats(B, n)), dtype=torch.float32, device=p.device)
        _ffi.check(_ffi.lib.sk_train_tversky(_ffi.ptr(p), _ffi.ptr(g), B, n, self.alpha, self.beta, self.eps,
                                             _ffi.ptr(loss), _ffi.ptr(ws), _ffi.stream_ptr(p.device)))
        return loss[0]

    def __repr__(self):
        return f"LossFn[name=tversky, alpha={self.alpha}, beta={self.beta}, eps={self.eps}"


def _check_volume(t: Tensor, name: str) -> Tensor:
    if t.ndim != 5:
        raise ValueError(f"{name} must be (B, C, X, Y, Z)")
    t = t.float().contiguous()
    _ffi.require_gpu(t, name)
    return t


def soft_skeletonize(img: Tensor, iter_: int) -> Tensor:
    """Soft skeleton of ``img`` (B, C, X, Y, Z), every channel on its own (train/loss.py:295-310).  fp32, bit-identical
    to the reference; forward only.  ``iter_`` in [0, SK_CLDICE_MAX_ITER]."""
    x = _check_volume(img, "img")
    B, Cc, X, Y, Z = x.shape
    out = torch.empty_like(x)
    ws = torch.empty(int(_ffi.lib.sk_train_soft_skeleton_workspace_floats(B * Cc, X, Y, Z)), dtype=torch.float32,
                     device=x.device)
    _ffi.check(_ffi.lib.sk_train_soft_skeleton(_ffi.ptr(x), _ffi.ptr(out), B * Cc, X, Y, Z, int(iter_), _ffi.ptr(ws),
                                               _ffi.stream_ptr(x.device)))
    return out


class soft_dice_cldice:
    """``soft_dice_cldice(iter_=3, alpha=0.5, smooth=1.0)(predicted, ground_truth)`` (train/loss.py:361-391).

    predicted, ground_truth (B, C, X, Y, Z); (1 - alpha) soft Dice (smooth fixed at 1, as the reference calls it) +
    alpha soft clDice on the soft skeletons of both; every sum runs over the whole batch.  ``value_and_grad`` also
    returns d loss / d predicted (no gradient into ground_truth)."""

    def __init__(self, iter_: int = 3, alpha: float = 0.5, smooth: float = 1.0):
        self.iter, self.alpha, self.smooth = int(iter_), float(alpha), float(smooth)

    def _run(self, predicted: Tensor, ground_truth: Tensor, grad: bool):
        if predicted.shape != ground_truth.shape:
            raise ValueError("soft_dice_cldice: predicted and ground_truth must have the same shape")
        p = _check_volume(predicted, "predicted")
        g = _check_volume(ground_truth, "ground_truth")
        B, Cc, X, Y, Z = p.shape
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        dp = torch.empty_like(p) if grad else None
        ws = torch.empty(int(_ffi.lib.sk_train_soft_dice_cldice_workspace_floats(B * Cc, X, Y, Z, min(max(self.iter, 0), 16))),
                         dtype=torch.float32, device=p.device)
        _ffi.check(_ffi.lib.sk_train_soft_dice_cldice(_ffi.ptr(p), _ffi.ptr(g), B * Cc, X, Y, Z, self.iter, self.alpha,
                                                      self.smooth, _ffi.ptr(loss), _ffi.ptr(dp), _ffi.ptr(ws),
                                                      _ffi.stream_ptr(p.device)))
        return loss[0], dp

    def __call__(self, predicted: Tensor, ground_truth: Tensor) -> Tensor:
        return self._run(predicted, ground_truth, False)[0]

    def value_and_grad(self, predicted: Tensor, ground_truth: Tensor):
        """(loss, d loss / d predicted)."""
        return self._run(predicted, ground_truth, True)

    def __repr__(self):
        return f"LossFn[name=soft_cldice, iter_={self.iter}, alpha={self.alpha}, smooth={self.smooth}"


LOSS_FUNCTIONS = {"soft_cldice": soft_dice_cldice, "tversky": tversky}


def loss_from_cfg(name: str, keywords, values):
    """The loss a config names, built from its keyword / value lists (train/engine.py:315-335), e.g.
    ``loss_from_cfg(cfg.TRAIN.LOSS_SKELETON, cfg.TRAIN.LOSS_SKELETON_KEYWORDS, cfg.TRAIN.LOSS_SKELETON_VALUES)``."""
    if name not in LOSS_FUNCTIONS:
        raise ValueError(f"unknown loss function {name!r}; valid: {sorted(LOSS_FUNCTIONS)}")
    return LOSS_FUNCTIONS[name](**{k: v for k, v in zip(keywords, values)})
