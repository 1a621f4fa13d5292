"""GPU tests of conv3_upf_px_kernel, the plane-streaming form of the folded decoder conv (csrc/conv3d_up.hip): what
sk_conv3d_upfold runs in the fp16 precision for one skip chunk, one upsampled chunk and 32 output channels on the planes
of the production tile's level 0 (Zl 10: 3 low-resolution rows per workgroup, 176 staged positions per fine plane).

It sums a voxel's products in another order than conv3_upf_kernel (by input plane, not by tap row): on integer operands
every product and sum is exact, so there it must agree with torch and with sk_conv3d bit for bit, GroupNorm sums
included; on random data it stays inside the bound test_hip_upfold.py holds the folded kernel to.  A workgroup runs four
x-chunks of the plan and one cout half: the x extents below put chunk ends, ragged last chunks and planes past the tile
in every position of a step, and the partial rows must still be the plan's (sk_conv3d_upfold_num_blocks)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


# (B, out spatial): 32 + 32 -> 32, Zt 20 (Zl 10) or 16 (Zl 8: the same staged plane sizes)
SHAPES = [
    (1, (2, 12, 20)),      # x extent 2: one plan chunk, four steps, both end steps half outside the tile
    (3, (6, 14, 20)),      # x extent 6, B 3; Yl 7 is not a multiple of K = 3
    (1, (44, 30, 20)),     # plan chunks of 8 planes: a workgroup closes four partial rows, the second one two
    (1, (150, 8, 20)),     # x extent 150: 38 plan chunks of 4, a ragged last workgroup
    (1, (300, 12, 20)),    # x extent 300
    (2, (10, 20, 16)),     # Zl 8: K = 4
]


def _make(B, osp, integer, seed, c_skip=32, c_up=32, cout=32):
    gen = torch.Generator().manual_seed(seed)
    lo = tuple(s // 2 for s in osp)
    if integer:
        skip = torch.randint(-3, 4, (B, c_skip) + osp, generator=gen).half()
        up = torch.randint(-3, 4, (B, c_up) + lo, generator=gen).half()
        w = torch.randint(-2, 3, (cout, c_skip + c_up, 3, 3, 3), generator=gen).float()
        b = torch.randint(-4, 5, (cout,), generator=gen).float()
    else:
        skip = torch.randn((B, c_skip) + osp, generator=gen).half()
        up = torch.randn((B, c_up) + lo, generator=gen).half()
        w = torch.randn((cout, c_skip + c_up, 3, 3, 3), generator=gen) / ((c_skip + c_up) * 27) ** 0.5
        b = torch.randn(cout, generator=gen) * 0.1
    return skip, up, w, b


def _torch(skip, up, w, b):
    x = torch.cat([skip.float(), F.interpolate(up.float(), scale_factor=2, mode="nearest")], dim=1)
    return F.conv3d(x, w, b, padding=1)


def _direct(U, s_d, u_d, w, b, osp):
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    return U.conv3d([(s_d, 0), (u_d, 1)], U.pack_conv_weight(w, DEV), b.to(DEV), 32, 3, osp, zeros)


def test_production_plane_takes_the_plan_rows():
    """The plan the new kernel writes its partial rows for: 50 workgroups x 8 x-chunks at the benched tile."""
    from skoots_amd import _ffi
    assert _ffi.lib.sk_conv3d_upfold_num_blocks(300, 300, 20, 32) == 50 * 8


@pytest.mark.parametrize("shape", SHAPES)
def test_upfold_px_exact_on_integers(shape):
    """Integer operands: the kernel == torch fp32 == sk_conv3d bit for bit, and the GroupNorm sums of sk_conv3d."""
    from skoots_amd import unet as U
    B, osp = shape
    skip, up, w, b = _make(B, osp, True, 3 + osp[0])
    want = _torch(skip, up, w, b)
    assert want.abs().max() < 2048
    s_d, u_d = _cl(skip).to(DEV), _cl(up).to(DEV)
    got, partial = U.conv3d_upfold(s_d, u_d, U.pack_conv_weight_upfold(w, 32, DEV), b.to(DEV), 32)
    assert torch.equal(_cf(got.cpu().float()), want)
    ref, rpartial = _direct(U, s_d, u_d, w, b, osp)
    assert torch.equal(ref, got)
    ps, rs = partial.sum(dim=1).cpu(), rpartial.sum(dim=1).cpu()
    assert torch.equal(ps[..., 0], rs[..., 0])
    assert torch.allclose(ps[..., 1], rs[..., 1], rtol=1e-6)
    # every row of the plan is written (the buffer starts zeroed): per row the sum of squares of a real block is > 0
    assert bool((partial[..., 1].sum(dim=-1) > 0).all())


def test_upfold_px_exact_benched_tile():
    """The benched tile, 300 x 300 x 20, on integer operands against sk_conv3d: bit for bit, partial rows included
    (integer sums below 2^24 are order-free, row by row)."""
    from skoots_amd import unet as U
    osp = (300, 300, 20)
    skip, up, w, b = _make(1, osp, True, 5)
    s_d, u_d = _cl(skip).to(DEV), _cl(up).to(DEV)
    got, partial = U.conv3d_upfold(s_d, u_d, U.pack_conv_weight_upfold(w, 32, DEV), b.to(DEV), 32)
    ref, _ = _direct(U, s_d, u_d, w, b, osp)
    assert torch.equal(ref, got)
    # the rows of the plan: recompute each from the stored output (fp32 sums of integers, exact)
    B, nblk = partial.shape[:2]
    assert nblk == 400
    rows = partial[0, :, :, 0].double().reshape(8, 50, 8).sum(dim=1)      # [x-chunk][quad], over the 50 patches
    o = got[0].double().reshape(300, 300, 20, 8, 4)
    want = torch.stack([o[40 * c:40 * c + 40].sum(dim=(0, 1, 2, 4)) for c in range(8)])   # chunks of 40 planes, the last 20
    assert torch.equal(rows, want)


@pytest.mark.parametrize("shape", SHAPES)
def test_upfold_px_vs_torch_random(shape):
    """Random operands against torch fp32 with the unrounded weights: test_hip_upfold.py's bound."""
    from skoots_amd import unet as U
    B, osp = shape
    skip, up, w, b = _make(B, osp, False, 17 + osp[0])
    want = _torch(skip, up, w, b)
    got, partial = U.conv3d_upfold(_cl(skip).to(DEV), _cl(up).to(DEV), U.pack_conv_weight_upfold(w, 32, DEV), b.to(DEV), 32)
    got = _cf(got.cpu().float())
    err = (got - want).abs().max().item()
    assert err <= 3e-3 * max(1.0, want.abs().max().item()), err
    p = partial.sum(dim=1).cpu()
    wq = got.reshape(B, 8, 4, -1)
    assert torch.allclose(p[..., 0], wq.sum(dim=(2, 3)), rtol=1e-3, atol=2e-2 * wq.shape[-1] ** 0.5)
    assert torch.allclose(p[..., 1], (wq ** 2).sum(dim=(2, 3)), rtol=2e-3)


@pytest.mark.parametrize("osp", [(44, 30, 20), (6, 14, 20)])
def test_upfold_px_batch_invariant(osp):
    """A tile alone and the same tile inside a batch of three: the same bits, output and partial rows."""
    from skoots_amd import unet as U
    skip, up, w, b = _make(3, osp, False, 23)
    wp, bd = U.pack_conv_weight_upfold(w, 32, DEV), b.to(DEV)
    s_d, u_d = _cl(skip).to(DEV), _cl(up).to(DEV)
    got, partial = U.conv3d_upfold(s_d, u_d, wp, bd, 32)
    for i in range(3):
        one, p1 = U.conv3d_upfold(s_d[i:i + 1].contiguous(), u_d[i:i + 1].contiguous(), wp, bd, 32)
        assert torch.equal(one[0], got[i])
        assert torch.equal(p1[0], partial[i])


def test_network_vs_oracle_benched_tile():
    """The whole network on one tile of the benched geometry (300 x 300 x 20: dec0.0 on the plane-streaming kernel with
    the production plan) against the torch fp32 CPU oracle, to test_hip_unet.py::test_network_vs_oracle's bounds."""
    from oracle import unet_spec
    from skoots_amd import unet as U
    ref = unet_spec.build(101196)
    hip = U.HipUNet.from_module(ref, DEV)
    tile = (300, 300, 20)
    gen = torch.Generator().manual_seed(300)
    vol = torch.randint(0, 256, tile, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), [(0, 0, 0)], tile, mean, std).cpu().float()
    crop = vol[None, None].sub(mean).div(std).float()
    with torch.no_grad():
        want32 = ref(crop)[0]
        want16 = unet_spec.forward_fp16_storage(ref, crop)[0]
    e32 = (out5[0] - want32).abs()
    emu = (want16 - want32).abs()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    assert rms(e32) <= 1e-3 and e32.max().item() <= 1e-2
    assert rms(e32) <= 1.25 * rms(emu) + 1e-5
