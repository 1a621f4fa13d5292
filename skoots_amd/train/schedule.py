"""Learning-rate schedule of the training loop (reference: skoots/train/engine.py:308-310, 512)."""
from __future__ import annotations

import math


def cosine_annealing_warm_restarts(base_lr: float, T_0: int, epoch: int, eta_min: float = 0.0, T_mult: int = 1) -> float:
    """The learning rate ``torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0, T_mult, eta_min)``
    holds after ``epoch`` calls of ``.step()``: eta_min + (base_lr - eta_min) (1 + cos(pi T_cur / T_i)) / 2, with
    T_cur counting the steps since the last restart and T_i the current period (T_0, multiplied by T_mult at every
    restart).  The reference steps its scheduler at the end of every epoch, so epoch ``e`` trains with the value for
    ``epoch = e``."""
    if T_0 <= 0 or not isinstance(T_0, int):
        raise ValueError(f"Expected positive integer T_0, but got {T_0}")
    if T_mult < 1 or not isinstance(T_mult, int):
        raise ValueError(f"Expected integer T_mult >= 1, but got {T_mult}")
    if epoch < 0:
        raise ValueError(f"Expected non-negative epoch, but got {epoch}")
    t_cur, t_i = 0, T_0
    for _ in range(int(epoch)):
        t_cur += 1
        if t_cur >= t_i:
            t_cur = t_cur % t_i
            t_i = t_i * T_mult
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * t_cur / t_i)) / 2
