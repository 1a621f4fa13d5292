"""GPU tests of the fused training step with a soft-clDice term (skoots_amd/train/engine.py).

The composed loss is pinned to tests/golden/cldice_step.npz (G8's composition with the reference's own
soft_dice_cldice as the skeleton term, and separately as the embedding term); the whole step against torch autograd
on oracle/unet_spec.py whose skeleton term is tests/test_hip_cldice.py's restatement."""
import numpy as np
import pytest
import torch

from tests.test_hip_cldice import ref_soft_dice_cldice
from tests.test_hip_train import _cf, _cl, _close, _golden_logits, _synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("tag,term", [("skel", 2), ("embed", 0)])
def test_fused_loss_with_cldice_term_vs_reference_golden(golden, tag, term):
    from skoots_amd.train import fused_loss, soft_dice_cldice
    d = golden("cldice_step.npz")
    logits, dact = _golden_logits(d)
    params = [(0.25, 0.75, 1e-8), (0.5, 0.5, 1e-8), (0.5, 1.5, 1e-8)]
    params[term] = soft_dice_cldice()
    lg = _cl(logits.float()).to(DEV)
    args = (lg, torch.tensor(d["masks"]).to(DEV), torch.tensor(d["skele"]).to(DEV), torch.tensor(d["baked"]).to(DEV),
            d["sigma"].tolist(), d["scale"].tolist(), params)
    losses, dl = fused_loss(*args)
    np.testing.assert_allclose(losses.cpu().numpy(), d[f"losses_{tag}"], rtol=0, atol=2e-6)
    want = torch.tensor(d[f"grad_{tag}"]).double() * dact
    _close(_cf(dl), want, 1e-4, f"d loss / d logits ({tag})")
    # need_grad=False: the same values, no gradient
    l2, dl2 = fused_loss(*args, need_grad=False)
    assert dl2 is None and torch.equal(l2, losses)


def test_tversky_objects_equal_the_default_tuples(golden):
    from skoots_amd.train import fused_loss, tversky
    d = golden("loss.npz")
    logits, _ = _golden_logits(d)
    args = (_cl(logits.float()).to(DEV), torch.tensor(d["masks"]).to(DEV), torch.tensor(d["skele"]).to(DEV),
            torch.tensor(d["baked"]).to(DEV), d["sigma"].tolist(), d["scale"].tolist())
    l0, g0 = fused_loss(*args)
    l1, g1 = fused_loss(*args, (tversky(0.25, 0.75, 1e-8), tversky(0.5, 0.5, 1e-8), tversky(0.5, 1.5, 1e-8)))
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


@pytest.mark.parametrize("precision", ["fp32", "mixed", "bf16"])
def test_cldice_step_finite_and_deterministic(precision):
    from skoots_amd.train import TrainStep, TrainUNet, soft_dice_cldice
    from skoots_amd.unet import random_state_dict
    sd = random_state_dict()
    images, masks, skele, baked = (t.to(DEV) for t in _synthetic_batch(1, 32, 20, 16, 9))
    runs = []
    for _ in range(2):
        model = TrainUNet(sd, DEV, precision=precision)
        step = TrainStep(model, loss_skele=soft_dice_cldice())
        losses = step(images, masks, skele, baked, [20.0, 20.0, 20.0])
        runs.append((losses.cpu(), model.flat_grad.clone(), model.flat_param.clone()))
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert 0.0 < runs[0][0][2].item() < 1.0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


def test_cldice_step_vs_oracle():
    """One fp32 step with the skeleton term as soft_dice_cldice() against torch autograd on oracle/unet_spec.py
    (tolerances of test_hip_train.py::test_train_step_vs_oracle: losses 1e-5, gradients 1e-3 of each tensor's max)."""
    from oracle import train_step as O
    from oracle import unet_spec
    from oracle.pipeline import vector_to_embedding
    from skoots_amd.train import TrainStep, TrainUNet, soft_dice_cldice
    ref = unet_spec.build().train()
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    B, X, Y, Z = 2, 16, 12, 8
    sigma, scale = torch.tensor([20.0, 20.0, 20.0]), torch.tensor((60, 60, 12))
    images, masks, skele, baked = _synthetic_batch(B, X, Y, Z, 40)
    # reference: engine.py:461-493 with LOSS_SKELETON = soft_cldice
    out = ref(images)
    prob, vec, sk = out[:, [-1]], out[:, 0:3], out[:, [-2]]
    emb = torch.cat([vector_to_embedding(scale, vec[b:b + 1]) for b in range(B)])
    pe = O.baked_embed_to_prob(emb, baked, sigma)
    fg = masks.gt(0).float()
    le = O.tversky(pe, fg, 0.25, 0.75, 1e-8)
    lp = O.tversky(prob, fg, 0.5, 0.5, 1e-8)
    ls = ref_soft_dice_cldice(sk, skele.gt(0).float())
    loss = le + lp + ls
    loss.backward()
    want = torch.stack([le, lp, ls, loss]).detach()
    ref_grads = {k: p.grad.clone() for k, p in ref.named_parameters()}

    model = TrainUNet(sd0, DEV)
    step = TrainStep(model, loss_skele=soft_dice_cldice())
    got = step(images.to(DEV), masks.to(DEV), skele.to(DEV), baked.to(DEV), sigma.tolist())
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=0, atol=1e-5)
    for k, g in model.grads().items():
        _close(g, ref_grads[k], 1e-3, f"grad {k}")
