"""GPU tests of the soft-clDice kernels (skoots_amd/csrc/cldice.hip).

Pinned to tests/golden/cldice.npz (the reference's own soft_skeletonize / soft_dice_cldice in fp32 with their
autograd gradient, on inputs full of exact ties); larger shapes against ``ref_soft_dice_cldice`` below, a float64
torch autograd restatement of the reference formula (train/loss.py:269-310, 344-391)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ----------------------------------------------------------------------------- restatement (torch autograd)
def ref_soft_skeletonize(img, iter_):
    def erode(x):
        p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
        p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
        return torch.min(torch.min(p1, p2), p3)

    def dilate(x):
        return F.max_pool3d(x, (3, 3, 3), (1, 1, 1), (1, 1, 1))

    skel = F.relu(img - dilate(erode(img)))
    for _ in range(iter_):
        img = erode(img)
        delta = F.relu(img - dilate(erode(img)))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def ref_soft_dice_cldice(pred, gt, iter_=3, alpha=0.5, smooth=1.0):
    dice = 1.0 - (2.0 * torch.sum(gt * pred) + 1) / (torch.sum(gt) + torch.sum(pred) + 1)
    sp, st = ref_soft_skeletonize(pred, iter_), ref_soft_skeletonize(gt, iter_)
    tprec = (torch.sum(sp * gt) + smooth) / (torch.sum(sp) + smooth)
    tsens = (torch.sum(st * pred) + smooth) / (torch.sum(st) + smooth)
    cl = 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)
    return (1.0 - alpha) * dice + alpha * cl


def plateau_volume(shape, seed):
    """Random multiples of 1/16 (every skeleton value is then exact in fp32 and float64 alike, so both take the same
    relu / tie branches) with saturated blocks of 1 and 0."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 17, shape, generator=gen).float() / 16.0
    X, Y, Z = shape[2:]
    for _ in range(6):
        o = [int(torch.randint(0, max(e - 4, 1), (1,), generator=gen)) for e in (X, Y, Z)]
        p[:, :, o[0]:o[0] + 6, o[1]:o[1] + 5, o[2]:o[2] + 4] = float(torch.randint(0, 2, (1,), generator=gen))
    gt = (torch.rand(shape, generator=gen) > 0.6).float()
    gt[:, :, X // 4:X // 2, Y // 4:Y // 2, :] = 1.0
    return p, gt


def _grad_close(got, want, rel, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
    assert err <= rel, f"{what}: max err / max |grad| = {err:.3e} > {rel}"


# ----------------------------------------------------------------------------- golden (the reference's own code)
def _cases(golden):
    d = golden("cldice.npz")
    return d, int(d["n"])


def test_soft_skeleton_bit_identical_to_reference(golden):
    from skoots_amd.train import soft_skeletonize
    d, n = _cases(golden)
    for i in range(n):
        it = int(d[f"iter_{i}"])
        for side in ("pred", "gt"):
            got = soft_skeletonize(torch.tensor(d[f"{side}_{i}"]).to(DEV), it).cpu().numpy()
            assert np.array_equal(got, d[f"skel_{side}_{i}"]), f"case {i} {side}: skeleton differs"


def test_soft_dice_cldice_value_and_grad_vs_reference(golden):
    from skoots_amd.train import soft_dice_cldice
    d, n = _cases(golden)
    for i in range(n):
        fn = soft_dice_cldice(iter_=int(d[f"iter_{i}"]), alpha=float(d[f"alpha_{i}"]), smooth=float(d[f"smooth_{i}"]))
        pred, gt = torch.tensor(d[f"pred_{i}"]).to(DEV), torch.tensor(d[f"gt_{i}"]).to(DEV)
        loss, dp = fn.value_and_grad(pred, gt)
        assert abs(loss.item() - float(d[f"loss_{i}"])) <= 2e-6, (i, loss.item(), float(d[f"loss_{i}"]))
        assert abs(fn(pred, gt).item() - float(d[f"loss_{i}"])) <= 2e-6, i
        _grad_close(dp, torch.tensor(d[f"grad_{i}"]), 1e-5, f"case {i}")


# ----------------------------------------------------------------------------- larger shapes (float64 restatement)
@pytest.mark.parametrize("shape,iter_,alpha,smooth", [((2, 1, 64, 48, 40), 3, 0.5, 1.0), ((1, 1, 256, 256, 32), 3, 0.5, 1.0),
                                                      ((1, 2, 20, 3, 33), 5, 0.25, 0.5)])
def test_soft_dice_cldice_vs_float64(shape, iter_, alpha, smooth):
    from skoots_amd.train import soft_dice_cldice, soft_skeletonize
    pred, gt = plateau_volume(shape, sum(shape) + iter_)
    p64 = pred.double().requires_grad_(True)
    want = ref_soft_dice_cldice(p64, gt.double(), iter_, alpha, smooth)
    want.backward()
    fn = soft_dice_cldice(iter_=iter_, alpha=alpha, smooth=smooth)
    loss, dp = fn.value_and_grad(pred.to(DEV), gt.to(DEV))
    assert abs(loss.item() - want.item()) <= 2e-6 * max(1.0, abs(want.item())), (loss.item(), want.item())
    _grad_close(dp, p64.grad, 1e-5, str(shape))
    # the skeleton of a 1/16-grid input is exact in fp32: equal to the float64 one
    sk = soft_skeletonize(pred.to(DEV), iter_).cpu().double()
    assert torch.equal(sk, ref_soft_skeletonize(pred.double(), iter_))


def test_gradient_is_deterministic():
    from skoots_amd.train import soft_dice_cldice
    pred, gt = plateau_volume((2, 1, 64, 48, 40), 5)
    fn = soft_dice_cldice()
    a = fn.value_and_grad(pred.to(DEV), gt.to(DEV))
    b = fn.value_and_grad(pred.to(DEV), gt.to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_errors_before_any_launch():
    """A bad argument returns SK_ERR_ARG with every output untouched (nothing was launched)."""
    from skoots_amd import _ffi
    st = _ffi.stream_ptr(torch.device(DEV))
    p = torch.rand((1, 4, 5, 6), device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    dp = torch.full_like(p, 7.0)
    sk = torch.full_like(p, 7.0)
    ws = torch.zeros(int(_ffi.lib.sk_train_soft_dice_cldice_workspace_floats(1, 4, 5, 6, 16)), device=DEV)
    bad = [(1, 4, 5, 6, 17, 0.5, 1.0), (1, 4, 5, 6, -1, 0.5, 1.0), (0, 4, 5, 6, 3, 0.5, 1.0), (1, 0, 5, 6, 3, 0.5, 1.0),
           (1, 4, 5, 6, 3, float("nan"), 1.0), (1, 4, 5, 6, 3, 0.5, float("inf"))]
    for B, X, Y, Z, it, alpha, smooth in bad:
        rc = _ffi.lib.sk_train_soft_dice_cldice(_ffi.ptr(p), _ffi.ptr(p), B, X, Y, Z, it, alpha, smooth, _ffi.ptr(loss),
                                                _ffi.ptr(dp), _ffi.ptr(ws), st)
        assert rc == -1, (B, X, Y, Z, it, alpha, smooth)
        if alpha == 0.5 and smooth == 1.0:   # the skeleton has no alpha / smooth
            rc = _ffi.lib.sk_train_soft_skeleton(_ffi.ptr(p), _ffi.ptr(sk), B, X, Y, Z, it, _ffi.ptr(ws), st)
            assert rc == -1, (B, X, Y, Z, it)
    assert _ffi.lib.sk_train_soft_dice_cldice(_ffi.ptr(p), _ffi.ptr(p), 1, 4, 5, 6, 3, 0.5, 1.0, _ffi.ptr(loss),
                                              _ffi.ptr(p), _ffi.ptr(ws), st) == -1   # dpred aliasing an input
    assert _ffi.lib.sk_train_soft_dice_cldice(None, _ffi.ptr(p), 1, 4, 5, 6, 3, 0.5, 1.0, _ffi.ptr(loss), None,
                                              _ffi.ptr(ws), st) == -1
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and bool((dp == 7.0).all()) and bool((sk == 7.0).all())
    from skoots_amd.train import soft_dice_cldice, soft_skeletonize
    with pytest.raises(ValueError, match="iter"):
        soft_dice_cldice(iter_=17)(p[None], p[None])
    with pytest.raises(ValueError, match="iter"):
        soft_skeletonize(p[None], -1)
    with pytest.raises(ValueError):
        soft_dice_cldice()(p[None], p[None, :, :3])
