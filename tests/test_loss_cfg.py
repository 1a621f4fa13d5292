"""CPU tests of the loss registry (reference skoots/train/engine.py:44-47, 315-335) and of the soft-clDice entry
points' host side: no GPU compute is called here."""
import pytest
import torch


def test_loss_registry_matches_the_reference():
    from skoots_amd.train import LOSS_FUNCTIONS, soft_dice_cldice, tversky
    assert set(LOSS_FUNCTIONS) == {"tversky", "soft_cldice"}
    assert LOSS_FUNCTIONS["tversky"] is tversky and LOSS_FUNCTIONS["soft_cldice"] is soft_dice_cldice


def test_loss_from_cfg_maps_names_and_keywords():
    from skoots_amd.train import loss_from_cfg, soft_dice_cldice, tversky
    t = loss_from_cfg("tversky", ["alpha", "beta", "eps"], [0.5, 1.5, 1e-8])   # the reference's LOSS_SKELETON default
    assert isinstance(t, tversky) and (t.alpha, t.beta, t.eps) == (0.5, 1.5, 1e-8)
    c = loss_from_cfg("soft_cldice", [], [])                                   # soft_dice_cldice's own defaults
    assert isinstance(c, soft_dice_cldice) and (c.iter, c.alpha, c.smooth) == (3, 0.5, 1.0)
    c = loss_from_cfg("soft_cldice", ["iter_", "smooth", "alpha"], [5, 2.0, 0.25])
    assert (c.iter, c.alpha, c.smooth) == (5, 0.25, 2.0)
    with pytest.raises(ValueError, match="unknown loss"):
        loss_from_cfg("jaccard", [], [])
    with pytest.raises(TypeError):
        loss_from_cfg("soft_cldice", ["beta"], [1.0])


def test_soft_cldice_rejects_cpu_tensors():
    from skoots_amd.train import soft_dice_cldice, soft_skeletonize
    x = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soft_skeletonize(x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soft_dice_cldice()(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soft_dice_cldice().value_and_grad(x, x)


def test_train_step_keeps_a_cldice_term_and_tversky_tuples():
    from skoots_amd.train import engine, soft_dice_cldice, tversky
    c = soft_dice_cldice()
    assert engine._loss_term(c) == ("soft_cldice", c)
    assert engine._loss_term(tversky(0.5, 1.5, 1e-8)) == ("tversky", [0.5, 1.5, 1e-8])
    assert engine._loss_term((0.5, 1.5, 1e-8)) == ("tversky", [0.5, 1.5, 1e-8])
