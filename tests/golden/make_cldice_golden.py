#!/usr/bin/env python3
"""Generate the soft-clDice fixtures under tests/golden/ from the REFERENCE's own functions.

Run where the reference checkout is available (GPU tests read only the committed .npz), like make_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 PYTORCH_JIT=0 \\
        python tests/golden/make_cldice_golden.py

The placeholders for absent third-party modules are make_golden.py's; none is
reached by the functions called here.

  G11 cldice.npz         soft_skeletonize / soft_dice_cldice in fp32 with their autograd gradient,
                         inputs full of exact ties                                        train/loss.py:269-310,344-391
  G12 cldice_step.npz    G8's composition (train/engine.py:461-496) with LOSS_SKELETON = soft_cldice and,
                         separately, LOSS_EMBED = soft_cldice: losses and d loss / d out
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _ident(*a, **k):
    return a[0] if a and callable(a[0]) else (lambda f: f)


_stub("numba", njit=_ident, prange=range)
_sk = _stub("skimage")
_sk.morphology = _stub("skimage.morphology")
_stub("bism")
for _s in ("backends", "modules", "models", "models.spatial_embedding"):
    _stub("bism." + _s)
sys.modules["bism.models.spatial_embedding"].SpatialEmbedding = object
_y = _stub("yacs")
_y.config = _stub("yacs.config", CfgNode=dict)

from skoots.lib.embedding_to_prob import baked_embed_to_prob  # noqa: E402
from skoots.lib.vector_to_embedding import vector_to_embedding  # noqa: E402
from skoots.train.loss import soft_dice_cldice, soft_skeletonize, tversky  # noqa: E402


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def _tied(gen, shape):
    """A probability volume made of exact ties: blocks of exactly 1.0 and 0.0, plateaus along each single axis,
    27-windows with several equal maxima, a few quantised levels; the rest uniform."""
    B, C, X, Y, Z = shape
    p = torch.rand(shape, generator=gen)
    q = torch.randint(0, 5, shape, generator=gen).float() / 4.0        # 0, .25, .5, .75, 1 exactly
    p = torch.where(torch.rand(shape, generator=gen) < 0.4, q, p)
    p[:, :, : X // 2, : Y // 2, : Z // 2] = 1.0                        # a saturated block
    p[:, :, X // 2:, Y // 2:, :2] = 0.0                                # a dead block
    if X >= 3:
        p[:, :, 0:3, Y - 1, Z - 1] = 0.75                              # plateau along x
    if Y >= 3:
        p[:, :, X - 1, 0:3, 0] = 0.5                                   # plateau along y
    if Z >= 3:
        p[:, :, X - 1, Y - 1, Z - 3:] = 0.25                           # plateau along z
    if X >= 3 and Y >= 3 and Z >= 3:
        p[:, :, X - 3:, :3, Z - 3:] = 0.6                              # a whole 27-window of equal values
    return p.contiguous()


def g11():
    gen = torch.Generator().manual_seed(1111)
    cases = [  # (shape, iter_, alpha, smooth)
        ((2, 1, 9, 8, 7), 3, 0.5, 1.0),
        ((1, 1, 1, 10, 9), 1, 0.5, 1.0),      # an axis of extent 1
        ((1, 1, 6, 2, 8), 0, 0.5, 1.0),       # an axis of extent 2, no iteration
        ((2, 1, 8, 7, 6), 3, 0.3, 2.5),       # smooth != 1 (dice keeps 1), alpha != 0.5
        ((1, 1, 12, 11, 10), 3, 0.5, 1.0),    # sigmoid-like field with saturated plateaus
    ]
    out = {"n": np.array(len(cases))}
    for i, (shape, it, alpha, smooth) in enumerate(cases):
        if i == 4:
            logit = torch.randn(shape, generator=gen) * 12.0
            pred = torch.sigmoid(logit)                                  # exactly 1.0 / ~0 where saturated
        else:
            pred = _tied(gen, shape)
        gt = (torch.rand(shape, generator=gen) > 0.5).float()
        gt[:, :, : shape[2] // 2 + 1, : shape[3] // 2 + 1, : shape[4] // 2 + 1] = 1.0   # a solid block
        p = pred.clone().requires_grad_(True)
        loss = soft_dice_cldice(iter_=it, alpha=alpha, smooth=smooth)(p, gt)
        loss.backward()
        with torch.no_grad():
            sp = soft_skeletonize(pred.clone(), it)
            st = soft_skeletonize(gt.clone(), it)
        out.update({f"pred_{i}": pred.numpy(), f"gt_{i}": gt.numpy(), f"iter_{i}": np.array(it),
                    f"alpha_{i}": np.array(alpha), f"smooth_{i}": np.array(smooth), f"skel_pred_{i}": sp.numpy(),
                    f"skel_gt_{i}": st.numpy(), f"loss_{i}": np.array(loss.item()), f"grad_{i}": p.grad.numpy()})
    save("cldice.npz", **out)


def g12():
    """G8's inputs (make_golden.py g8) and composition, one term's loss replaced by soft_dice_cldice()."""
    gen = torch.Generator().manual_seed(88)
    B, X, Y, Z = 2, 12, 10, 8
    out0 = torch.rand((B, 5, X, Y, Z), generator=gen)
    out0[:, 0:3] = out0[:, 0:3] * 2 - 1
    masks = (torch.rand((B, 1, X, Y, Z), generator=gen) > 0.6).float() * torch.randint(1, 5, (B, 1, X, Y, Z), generator=gen)
    skele = (torch.rand((B, 1, X, Y, Z), generator=gen) > 0.85).float()
    baked = torch.rand((B, 3, X, Y, Z), generator=gen) * torch.tensor([X, Y, Z]).view(1, 3, 1, 1, 1)
    scale = torch.tensor((60, 60, 12))
    sigma = torch.tensor([20.0, 20.0, 20.0])
    res = {}
    for tag, which in (("skel", 2), ("embed", 0)):
        out = out0.clone().requires_grad_(True)
        fns = [tversky(0.25, 0.75, 1e-8), tversky(0.5, 0.5, 1e-8), tversky(0.5, 1.5, 1e-8)]
        fns[which] = soft_dice_cldice()
        prob, vec, sk = out[:, [-1]], out[:, 0:3], out[:, [-2]]
        emb = vector_to_embedding(scale, vec)
        pe = baked_embed_to_prob(emb, baked, sigma)
        le = fns[0](pe, masks.gt(0).float())
        lp = fns[1](prob, masks.gt(0).float())
        ls = fns[2](sk, skele.gt(0).float())
        loss = 1.0 * le + 1.0 * lp + 1.0 * ls
        loss.backward()
        res[f"losses_{tag}"] = np.array([le.item(), lp.item(), ls.item(), loss.item()])
        res[f"grad_{tag}"] = out.grad.numpy()
    save("cldice_step.npz", out=out0.numpy(), masks=masks.numpy(), skele=skele.numpy(), baked=baked.numpy(),
         scale=scale.numpy(), sigma=sigma.numpy(), **res)


if __name__ == "__main__":
    torch.set_num_threads(8)
    g11(); g12()
