"""GPU parity tests for the U-Net body: every kernel against a plain PyTorch fp32 CPU
reference of the same op (floating point: tolerances stated per test), and the whole
network against oracle/unet_spec.py at 1e-3 absolute (BASELINE.json north_star)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def U():
    from skoots_amd import unet
    return unet


def _cl(x):  # (B, C, X, Y, Z) -> channels-last (B, X, Y, Z, C)
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _ref_conv(srcs, w, b, ksize):
    xs = []
    for t, up in srcs:
        t = t.float()
        if up:
            t = F.interpolate(t, scale_factor=2, mode="nearest")
        xs.append(t)
    x = torch.cat(xs, dim=1)
    w16 = w.half().float()  # the kernel consumes fp16 weights; accumulate in fp32
    if ksize == 3:
        return F.conv3d(x, w16, b, padding=1)
    return F.conv3d(x, w16, b, stride=ksize)


CONV_CASES = [
    # (B, out spatial, [(c, up)], cout, ksize)
    (1, (8, 12, 20), [(32, 0)], 32, 3),          # linear mode, exact steps
    (2, (13, 11, 20), [(32, 0)], 32, 3),         # ragged x / ragged last patch, batch 2
    (1, (12, 20, 20), [(32, 0), (32, 1)], 32, 3),  # decoder concat with nearest upsample
    (1, (10, 14, 10), [(64, 0)], 64, 3),
    (1, (6, 16, 10), [(64, 0), (64, 1)], 64, 3),
    (1, (7, 19, 5), [(128, 0)], 128, 3),         # XS = 2 path, z = 5
    (1, (9, 8, 64), [(32, 0)], 32, 3),           # rectangle mode (z > 40)
    (1, (5, 6, 72), [(64, 0)], 64, 3),           # rectangle mode, ragged z chunk
    (2, (6, 7, 10), [(32, 0)], 64, 2),           # stride-2 down conv
    (1, (5, 9, 5), [(64, 0)], 128, 2),
    (1, (9, 10, 5), [(128, 0)], 64, 1),          # pointwise reducers
    (1, (12, 10, 10), [(64, 0)], 32, 1),
    # the plane-streaming 32 -> 32 kernel (conv3_px_kernel: 176-position planes, z 16 .. 20): x-chunks of 1, 2, 3 planes,
    # an odd chunk behind even ones, several chunks with interior chunk seams; z 22 / 23 (same plane size, too few padding
    # positions) stay on conv3_m16_kernel
    (1, (1, 12, 20), [(32, 0)], 32, 3),
    (1, (2, 9, 20), [(32, 0)], 32, 3),
    (1, (3, 12, 16), [(32, 0)], 32, 3),
    (2, (37, 14, 20), [(32, 0)], 32, 3),
    (1, (16, 30, 22), [(32, 0)], 32, 3),
    (1, (9, 7, 18), [(32, 0)], 32, 3),
    (1, (5, 8, 23), [(32, 0)], 32, 3),
    # COUT 32 on 8 x 16 rectangle patches (round 4: z > 40 keeps the six-plane ring): ragged rows (y % 8), a ragged z
    # chunk (z % 16), two chunks with an upsampled source, batch 2, several x-chunks
    (1, (9, 21, 48), [(32, 0)], 32, 3),
    (2, (5, 8, 70), [(32, 0)], 32, 3),
    (1, (6, 12, 44), [(32, 0), (32, 1)], 32, 3),
    (1, (40, 9, 128), [(32, 0)], 32, 3),
]


@pytest.mark.parametrize("B,osp,srcdef,cout,ksize", CONV_CASES)
def test_conv_vs_torch(U, B, osp, srcdef, cout, ksize):
    gen = torch.Generator().manual_seed(cout * 7 + ksize + osp[0])
    srcs_cpu, srcs_dev = [], []
    for c, up in srcdef:
        if ksize == 3:
            sp = tuple(s // 2 for s in osp) if up else osp
        else:
            sp = tuple(s * ksize for s in osp)
        t = (torch.randn((B, c) + sp, generator=gen)).half()
        srcs_cpu.append((t, up))
        srcs_dev.append((_cl(t).to(DEV), up))
    cin = sum(c for c, _ in srcdef)
    w = torch.randn((cout, cin, ksize, ksize, ksize), generator=gen) / (cin * ksize ** 3) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    want = _ref_conv(srcs_cpu, w, b, ksize)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    got, partial = U.conv3d(srcs_dev, U.pack_conv_weight(w, DEV), b.to(DEV), cout, ksize, osp, zeros)
    got = _cf(got.cpu().float())
    # fp16 inputs / weights, fp32 accumulate, fp16 store: 2^-11 relative on O(1) outputs
    err = (got - want).abs().max().item()
    assert err <= 2e-3 * max(1.0, want.abs().max().item()), err
    # GroupNorm partials: per channel-quad (sum, sumsq) of the fp32 results
    p = partial.sum(dim=1).cpu()  # (B, cout/4, 2)
    wq = want.reshape(B, cout // 4, 4, -1)
    assert torch.allclose(p[..., 0], wq.sum(dim=(2, 3)), rtol=1e-3, atol=2e-2 * wq.shape[-1] ** 0.5)
    assert torch.allclose(p[..., 1], (wq ** 2).sum(dim=(2, 3)), rtol=2e-3)


@pytest.mark.parametrize("B,osp,srcdef,cout,ksize", CONV_CASES)
def test_conv_split_vs_torch(U, B, osp, srcdef, cout, ksize):
    """precision "split": fp32 operands carried as fp16 hi + lo pairs, three MFMAs per product.  Against a float64
    conv of the SAME fp32 operands: the only approximations left are the dropped lo*lo term and the 22-bit
    representation, ~1e-6 relative (the plain fp16 kernel sits at 1e-3 on the same data)."""
    gen = torch.Generator().manual_seed(cout * 5 + ksize + osp[1])
    srcs_cpu, srcs_dev = [], []
    for c, up in srcdef:
        if ksize == 3:
            sp = tuple(s // 2 for s in osp) if up else osp
        else:
            sp = tuple(s * ksize for s in osp)
        t = torch.randn((B, c) + sp, generator=gen)
        t = U.join_pair(U.split_pair(t))   # what the pair can hold exactly
        srcs_cpu.append((t, up))
        srcs_dev.append((U.split_pair(_cl(t)).to(DEV), up))
    cin = sum(c for c, _ in srcdef)
    w = torch.randn((cout, cin, ksize, ksize, ksize), generator=gen) / (cin * ksize ** 3) ** 0.5
    w = U.join_pair(U.split_pair(w.unsqueeze(-1))).squeeze(-1)
    b = torch.randn(cout, generator=gen) * 0.1
    xs = [F.interpolate(t.double(), scale_factor=2, mode="nearest") if up else t.double() for t, up in srcs_cpu]
    x = torch.cat(xs, dim=1)
    want = F.conv3d(x, w.double(), b.double(), padding=1) if ksize == 3 else F.conv3d(x, w.double(), b.double(), stride=ksize)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    got, partial = U.conv3d(srcs_dev, U.pack_conv_weight(w, DEV, split=True), b.to(DEV), cout, ksize, osp, zeros,
                            split=True)
    got = _cf(U.join_pair(got.cpu())).double()
    err = (got - want).abs().max().item()
    assert err <= 2e-5 * max(1.0, want.abs().max().item()), err
    p = partial.sum(dim=1).cpu().double()
    wq = want.reshape(B, cout // 4, 4, -1)
    assert torch.allclose(p[..., 0], wq.sum(dim=(2, 3)), rtol=1e-4, atol=1e-3 * wq.shape[-1] ** 0.5)
    assert torch.allclose(p[..., 1], (wq ** 2).sum(dim=(2, 3)), rtol=1e-4)


@pytest.mark.parametrize("B,osp,cin,cout", [(1, (6, 7, 10), 32, 64), (2, (5, 9, 5), 64, 128), (1, (13, 11, 10), 32, 64),
                                            (1, (3, 4, 3), 64, 128)])
def test_down_conv_with_fused_activation(U, B, osp, cin, cout):
    """sk_conv3d_down_act: the stride-2 down conv that activates its RAW input while staging it (GroupNorm affine +
    SiLU in LDS) and writes the activated tensor back.  The written-back tensor equals sk_groupnorm_silu's result
    bit for bit; the conv output equals the plain kernel's on the activated tensor (same operands, same K order)."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(cin + cout + osp[0])
    isp = tuple(2 * v for v in osp)
    raw = (torch.randn((B,) + isp + (cin,), generator=gen) * 2).half().to(DEV)
    aff = torch.stack([torch.rand((B, cin), generator=gen) + 0.5, torch.randn((B, cin), generator=gen) * 0.5], dim=1).to(DEV)
    w = torch.randn((cout, cin, 2, 2, 2), generator=gen) / (cin * 8) ** 0.5
    bias = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    wp = U.pack_conv_weight(w, DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(torch.device(DEV))
    # reference path: in-place GroupNorm pass, then the plain conv on the activated tensor
    act = raw.clone()
    vox = isp[0] * isp[1] * isp[2]
    _ffi.check(_ffi.lib.sk_groupnorm_silu(_ffi.ptr(act), _ffi.ptr(aff), B, vox, cin, st))
    want, want_partial = U.conv3d([(act, 0)], wp, bias, cout, 2, osp, zeros)
    # fused path
    x = raw.clone()
    got = torch.empty((B,) + osp + (cout,), dtype=torch.float16, device=DEV)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, osp[0], osp[1], osp[2], cout, 2)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=DEV)
    _ffi.check(_ffi.lib.sk_conv3d_down_act(_ffi.ptr(x), _ffi.ptr(aff), _ffi.ptr(wp), _ffi.ptr(bias), _ffi.ptr(got), B,
                                           osp[0], osp[1], osp[2], cin, cout, _ffi.ptr(partial), _ffi.ptr(zeros), st))
    assert torch.equal(x, act), "written-back activation differs from sk_groupnorm_silu"
    assert torch.equal(got, want)
    assert torch.allclose(partial.sum(1), want_partial.sum(1), rtol=1e-5, atol=1e-4)
    # and against torch on the activated operands
    ref = F.conv3d(_cf(act.cpu().float()), w.half().float(), bias.cpu(), stride=2)
    assert (_cf(got.cpu().float()) - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,osp,cin,cout", [(1, (6, 7, 10), 32, 64), (2, (5, 9, 5), 64, 128), (1, (13, 11, 10), 32, 64),
                                            (1, (3, 4, 3), 64, 128), (1, (9, 16, 10), 64, 128)])
def test_down_conv_with_fused_activation_split(U, B, osp, cin, cout):
    """sk_conv3d_down_act_split (round 4): the split-precision stride-2 conv that activates its RAW [hi | lo] input in LDS
    and writes the pair back.  The written-back tensor equals sk_groupnorm_silu_split's bit for bit; the conv output
    agrees with the gather kernel's (sk_conv3d_split on the activated tensor: same operands, another summation order) to
    fp32 accumulation noise and with a float64 conv of the activated operands to 2e-5; block counts past the tensor's
    end, batch > 1 and both sub-blocks of a workgroup are covered by the shapes."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(cin + cout + osp[0] + 1)
    isp = tuple(2 * v for v in osp)
    raw = U.split_pair(torch.randn((B,) + isp + (cin,), generator=gen) * 2).to(DEV)
    aff = torch.stack([torch.rand((B, cin), generator=gen) + 0.5, torch.randn((B, cin), generator=gen) * 0.5], dim=1).to(DEV)
    w = torch.randn((cout, cin, 2, 2, 2), generator=gen) / (cin * 8) ** 0.5
    w = U.join_pair(U.split_pair(w.unsqueeze(-1))).squeeze(-1)
    bias = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    wp = U.pack_conv_weight(w, DEV, split=True)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(torch.device(DEV))
    act = raw.clone()
    vox = isp[0] * isp[1] * isp[2]
    _ffi.check(_ffi.lib.sk_groupnorm_silu_split(_ffi.ptr(act), _ffi.ptr(aff), B, vox, cin, st))
    want, want_partial = U.conv3d([(act, 0)], wp, bias, cout, 2, osp, zeros, split=True)
    x = raw.clone()
    got = torch.empty((B,) + osp + (2 * cout,), dtype=torch.float16, device=DEV)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, osp[0], osp[1], osp[2], cout, 2)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=DEV)
    _ffi.check(_ffi.lib.sk_conv3d_down_act_split(_ffi.ptr(x), _ffi.ptr(aff), _ffi.ptr(wp), _ffi.ptr(bias), _ffi.ptr(got), B,
                                                 osp[0], osp[1], osp[2], cin, cout, _ffi.ptr(partial), _ffi.ptr(zeros), st))
    torch.cuda.synchronize()
    assert torch.equal(x, act), "written-back activation differs from sk_groupnorm_silu_split"
    g64, w64 = U.join_pair(got.cpu()).double(), U.join_pair(want.cpu()).double()
    scale = max(1.0, w64.abs().max().item())
    assert (g64 - w64).abs().max().item() <= 2e-6 * scale
    assert torch.allclose(partial.sum(1), want_partial.sum(1), rtol=1e-5, atol=1e-4)
    ref = F.conv3d(_cf(U.join_pair(act.cpu())).double(), w.double(), bias.cpu().double(), stride=2)
    assert (_cf(g64) - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    # precision "mix8": the same conv with the activated input written back as mix8 lines (sk_groupnorm_silu_mix8's store)
    xm = raw.clone()
    gotm = torch.empty_like(got)
    partm = torch.zeros_like(partial)
    _ffi.check(_ffi.lib.sk_conv3d_down_act_mix8(_ffi.ptr(xm), _ffi.ptr(aff), _ffi.ptr(wp), _ffi.ptr(bias), _ffi.ptr(gotm), B,
                                                osp[0], osp[1], osp[2], cin, cout, _ffi.ptr(partm), _ffi.ptr(zeros), st))
    actm = raw.clone()
    _ffi.check(_ffi.lib.sk_groupnorm_silu_mix8(_ffi.ptr(actm), _ffi.ptr(aff), B, vox, cin, st))
    torch.cuda.synchronize()
    assert torch.equal(xm, actm), "written-back mix8 lines differ from sk_groupnorm_silu_mix8"
    assert torch.equal(gotm, got) and torch.equal(partm, partial)
    # the raw source of a 1x1x1 conv is activated on load by the split gather kernel (sk_conv3d_split, affine != NULL)
    if cin == 64:
        w1 = torch.randn((32, cin, 1, 1, 1), generator=gen) / cin ** 0.5
        wp1, b1 = U.pack_conv_weight(w1, DEV, split=True), (torch.randn(32, generator=gen) * 0.1).to(DEV)
        plain, _ = U.conv3d([(act, 0)], wp1, b1, 32, 1, isp, zeros, split=True)
        fused = torch.empty_like(plain)
        arr = (_ffi.ConvSrc * 1)()
        arr[0].data, arr[0].c, arr[0].upsample, arr[0].affine = raw.data_ptr(), cin, 0, aff.data_ptr()
        _ffi.check(_ffi.lib.sk_conv3d_split(arr, 1, _ffi.ptr(wp1), _ffi.ptr(b1), _ffi.ptr(fused), B, isp[0], isp[1], isp[2], 32, 1,
                                            None, _ffi.ptr(zeros), st))
        torch.cuda.synchronize()
        assert torch.equal(fused, plain), "activation on load (split gather) differs from pass + plain conv"


def _conv_ffi(srcs, wp, bias, out_shape, cout=32, box=None, affine=None, prefill=None):
    """sk_conv3d / sk_conv3d_box through the C ABI with everything the U.conv3d helper leaves out."""
    from skoots_amd import _ffi
    import ctypes as C
    B = srcs[0][0].shape[0]
    ox, oy, oz = out_shape
    dev = srcs[0][0].device
    out = torch.empty((B, ox, oy, oz, cout), dtype=torch.float16, device=dev)
    if prefill is not None:
        out.fill_(prefill)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, cout, 3)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=dev)
    arr = (_ffi.ConvSrc * len(srcs))()
    for i, (t, up) in enumerate(srcs):
        arr[i].data, arr[i].c, arr[i].upsample = t.data_ptr(), t.shape[-1], up
        arr[i].affine = affine.data_ptr() if (affine is not None and i == 0) else None
    zeros = torch.zeros(4096, dtype=torch.uint8, device=dev)
    bx = (C.c_int32 * 6)(*box) if box is not None else None
    _ffi.check(_ffi.lib.sk_conv3d_box(arr, len(srcs), _ffi.ptr(wp), _ffi.ptr(bias), _ffi.ptr(out), B, ox, oy, oz, cout, 3,
                                      _ffi.ptr(partial), _ffi.ptr(zeros), bx, _ffi.stream_ptr(dev)))
    torch.cuda.synchronize()
    return out, partial


@pytest.mark.parametrize("B,osp", [(1, (8, 12, 20)), (2, (37, 14, 20)), (1, (5, 9, 16)), (1, (6, 10, 10)), (1, (4, 11, 48))])
def test_conv_activates_a_raw_source_in_lds(U, B, osp):
    """A RAW source (sk_conv_src.affine != NULL) is activated by the staging lanes in LDS -- silu(a*x + b), the
    arithmetic of sk_groupnorm_silu op for op -- so the conv over it must equal, BIT FOR BIT, the conv over the tensor
    the separate pass produces.  Covers conv3_px_kernel (z 16 / 20) and conv3_m16_kernel (z 10; z 48: rectangle patches)."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(osp[0] * 31 + osp[2])
    x = torch.randn((B,) + osp + (32,), generator=gen).half().to(DEV)
    aff = torch.stack([torch.rand((B, 32), generator=gen) + 0.5, torch.randn((B, 32), generator=gen) * 0.3], dim=1).to(DEV).contiguous()
    w = torch.randn((32, 32, 3, 3, 3), generator=gen) / (32 * 27) ** 0.5
    wp, bias = U.pack_conv_weight(w, DEV), (torch.randn(32, generator=gen) * 0.1).to(DEV)
    fused, pf = _conv_ffi([(x, 0)], wp, bias, osp, affine=aff)
    act = x.clone()
    vox = osp[0] * osp[1] * osp[2]
    _ffi.check(_ffi.lib.sk_groupnorm_silu(_ffi.ptr(act), _ffi.ptr(aff), B, vox, 32, _ffi.stream_ptr(torch.device(DEV))))
    plain, pp = _conv_ffi([(act, 0)], wp, bias, osp)
    assert torch.equal(fused, plain) and torch.equal(pf, pp)
    a, b_ = aff[:, 0].cpu().view(B, 32, 1, 1, 1), aff[:, 1].cpu().view(B, 32, 1, 1, 1)
    ref = F.conv3d(F.silu(_cf(x.cpu().float()) * a + b_).half().float(), w.half().float(), bias.cpu(), padding=1)
    assert (_cf(fused.cpu().float()) - ref).abs().max().item() <= 3e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("osp,box", [((12, 30, 20), (3, 4, 2, 9, 25, 17)), ((37, 14, 20), (0, 0, 0, 37, 14, 20)),
                                     ((9, 12, 20), (9, 0, 0, 9, 12, 20)), ((8, 12, 10), (2, 2, 2, 6, 9, 8)),
                                     ((6, 9, 48), (1, 2, 5, 5, 8, 41)), ((10, 40, 24), (0, 3, 1, 7, 33, 24))])
def test_conv_store_box(U, osp, box):
    """sk_conv3d_box: the voxels inside the box hold exactly what the plain launch stores, the GroupNorm partial sums
    are those of the WHOLE tile (bit-identical to the plain launch), and the voxels outside the box stay untouched:
    conv3_px_kernel (z = 20: first three cases, the third with an empty box) and, since round 4, conv3_m16_kernel --
    linear patches (z = 10, 24) and rectangle patches (z = 48)."""
    gen = torch.Generator().manual_seed(osp[0] + 7 * osp[1])
    x = torch.randn((2,) + osp + (32,), generator=gen).half().to(DEV)
    w = torch.randn((32, 32, 3, 3, 3), generator=gen) / (32 * 27) ** 0.5
    wp, bias = U.pack_conv_weight(w, DEV), (torch.randn(32, generator=gen) * 0.1).to(DEV)
    full, pfull = _conv_ffi([(x, 0)], wp, bias, osp)
    got, pbox = _conv_ffi([(x, 0)], wp, bias, osp, box=box, prefill=7.0)
    assert torch.equal(pbox, pfull)
    x0, y0, z0, x1, y1, z1 = box
    assert torch.equal(got[:, x0:x1, y0:y1, z0:z1], full[:, x0:x1, y0:y1, z0:z1])
    outside = torch.ones(osp, dtype=torch.bool, device=DEV)
    outside[x0:x1, y0:y1, z0:z1] = False
    assert bool((got[:, outside] == 7.0).all())


@pytest.mark.parametrize("osp,box", [((12, 30, 20), (3, 4, 2, 9, 25, 17)), ((8, 12, 10), (2, 2, 2, 6, 9, 8))])
def test_conv_store_box_split(U, osp, box):
    """sk_conv3d_box_split: as test_conv_store_box on [hi | lo] tensors (the last block's conv of precision="split")."""
    from skoots_amd import _ffi
    import ctypes as C
    gen = torch.Generator().manual_seed(osp[0] + 5 * osp[2])
    B = 2
    x = U.split_pair(torch.randn((B,) + osp + (32,), generator=gen)).to(DEV)
    w = torch.randn((32, 32, 3, 3, 3), generator=gen) / (32 * 27) ** 0.5
    wp, bias = U.pack_conv_weight(w, DEV, split=True), (torch.randn(32, generator=gen) * 0.1).to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    full, pfull = U.conv3d([(x, 0)], wp, bias, 32, 3, osp, zeros, split=True)
    ox, oy, oz = osp
    out = torch.full((B, ox, oy, oz, 64), 7.0, dtype=torch.float16, device=DEV)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, 32, 3)
    partial = torch.zeros((B, nblk, 8, 2), dtype=torch.float32, device=DEV)
    arr = (_ffi.ConvSrc * 1)()
    arr[0].data, arr[0].c, arr[0].upsample, arr[0].affine = x.data_ptr(), 32, 0, None
    _ffi.check(_ffi.lib.sk_conv3d_box_split(arr, 1, _ffi.ptr(wp), _ffi.ptr(bias), _ffi.ptr(out), B, ox, oy, oz, 32, 3,
                                            _ffi.ptr(partial), _ffi.ptr(zeros), (C.c_int32 * 6)(*box),
                                            _ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert torch.equal(partial, pfull)
    x0, y0, z0, x1, y1, z1 = box
    assert torch.equal(out[:, x0:x1, y0:y1, z0:z1], full[:, x0:x1, y0:y1, z0:z1])
    outside = torch.ones(osp, dtype=torch.bool, device=DEV)
    outside[x0:x1, y0:y1, z0:z1] = False
    assert bool((out[:, outside] == 7.0).all())


def _e4m3(t):
    return t.to(torch.float8_e4m3fn)


@pytest.mark.parametrize("osp,ch", [((6, 9, 20), 32), ((12, 30, 20), 32), ((9, 21, 12), 32), ((6, 9, 10), 64), ((9, 14, 10), 64),
                                    ((7, 12, 5), 128), ((5, 9, 36), 64),
                                    ((7, 10, 100), 32), ((7, 9, 64), 64), ((5, 6, 48), 128),   # rectangle patches (z > 40; 64: XS = 3)
                                    ((7, 11, 20), 32), ((9, 13, 16), 32), ((5, 8, 18), 32), ((1, 7, 20), 32), ((2, 40, 20), 32),
                                    ((37, 9, 20), 32)])   # conv3_pxm_kernel (z 16 .. 20): odd plane counts, one plane, ragged patches, two x-chunks
def test_conv_mix8_fp8_phase_exact(U, osp, ch):
    """sk_conv3d_mix8, the block-scaled fp8 phase alone (hi = 0): with operands whose fp8 images are exact small integers
    the result 2^-(b+15) (conv(x8, 2^(b+11) w_lo) + conv(lo8, 2^b w)) is an integer multiple of 2^-(b+15) below 2^24 of
    them -- exact in the fp32 accumulators and in the [hi | lo] store: pins the K-block order (tap-row pair x {w_lo . x8,
    w . lo8}), the lane maps of both fp8 operands, the uniform E8M0 scales and the zero halo of the fp8 bytes.  ch = 64 | 128:
    conv3_kernel's fp8 phase (v_mfma_scale_f32_32x32x64_f8f6f4, K = 64 = one tap x {w_lo . x8, w . lo8} per 32-channel chunk)."""
    gen = torch.Generator().manual_seed(osp[0] * 7 + osp[2])
    B = 2
    # w = s (1 + m / 8) + j 2^-14: fp16(w) = s (1 + m / 8), w_lo = j 2^-14; e4m3(2^b w) = 2^b s (1 + m / 8) exactly
    base = (1 + torch.randint(0, 8, (ch, ch, 3, 3, 3), generator=gen).float() / 8) * (torch.randint(0, 2, (ch, ch, 3, 3, 3), generator=gen) * 2 - 1).float()
    j = torch.randint(-3, 4, (ch, ch, 3, 3, 3), generator=gen).float()
    w = base + j * 2.0 ** -14
    assert torch.equal(w.half().float(), base) and torch.equal(w - base, j * 2.0 ** -14)
    wp, b = U.pack_conv_weight_mix8(w, DEV)
    assert b == 6
    x8 = torch.randint(-3, 4, (B,) + osp + (ch,), generator=gen).float()
    lo8 = torch.randint(-3, 4, (B,) + osp + (ch,), generator=gen).float()
    src = U.mix8_line(torch.zeros((B,) + osp + (ch,), dtype=torch.float16), _e4m3(x8), _e4m3(lo8)).to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    bias = torch.zeros(ch, device=DEV)
    got, _ = U.conv3d_mix8(src, wp, b, bias, osp, zeros)
    torch.cuda.synchronize()
    want = (F.conv3d(_cf(x8).double(), (j * 2.0 ** -14 * 2.0 ** (b + 11)).double(), padding=1)
            + F.conv3d(_cf(lo8).double(), (base * 2.0 ** b).double(), padding=1)) * 2.0 ** -(b + 15)
    assert torch.equal(_cf(U.join_pair(got.cpu()).double()), want)


@pytest.mark.parametrize("osp,ch", [((6, 9, 20), 32), ((6, 9, 10), 64), ((7, 12, 5), 128)])
def test_conv_mix8_fp16_phase_exact(U, osp, ch):
    """sk_conv3d_mix8 with integer weights (w_lo = 0) and lo8 = 0: only the fp16 product contributes, whatever x8 holds."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (1,) + osp + (ch,), generator=gen).float()
    w = torch.randint(-2, 3, (ch, ch, 3, 3, 3), generator=gen).float()
    bias = torch.randint(-4, 5, (ch,), generator=gen).float()
    wp, b = U.pack_conv_weight_mix8(w, DEV)
    src = U.mix8_line(x.half(), _e4m3(x * 16), _e4m3(torch.zeros_like(x))).to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    got, _ = U.conv3d_mix8(src, wp, b, bias.to(DEV), osp, zeros)
    torch.cuda.synchronize()
    want = F.conv3d(_cf(x), w, bias, padding=1)
    assert torch.equal(_cf(U.join_pair(got.cpu())), want)


@pytest.mark.parametrize("B,osp,ch", [(2, (12, 30, 20), 32), (1, (40, 36, 20), 32), (1, (16, 24, 48), 32), (2, (14, 30, 10), 64),
                                      (1, (18, 20, 5), 128), (1, (10, 16, 40), 64)])
def test_conv_mix8_matches_split(U, B, osp, ch):
    """sk_conv3d_mix8 on realistic operands against a float64 conv of the same (hi + lo) activations and fp32 weights, next
    to sk_conv3d_split: the fp8 corrections (2^-4 relative on terms that are 2^-11 of the result) leave ~1/27 of the error
    of the uncorrected fp16 product (measured 5.0e-5 / 1.35e-3 / split 3.7e-6 at scale 4.5): asserted <= 1/10 of it and
    <= 3e-5 of the result's scale; the GroupNorm partial sums agree to 1e-4; the store box is honoured."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(osp[0] + osp[2])
    x = torch.nn.functional.silu(torch.randn((B,) + osp + (ch,), generator=gen) * 1.5)
    w = torch.randn((ch, ch, 3, 3, 3), generator=gen) / (ch * 27) ** 0.5
    bias = (torch.randn(ch, generator=gen) * 0.1).to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    xs = U.split_pair(x)
    xj = U.join_pair(xs)
    ref = F.conv3d(_cf(xj).double(), w.double(), bias.cpu().double(), padding=1)
    scale = max(1.0, ref.abs().max().item())
    sp, sp_partial = U.conv3d([(xs.to(DEV), 0)], U.pack_conv_weight(w, DEV, split=True), bias, ch, 3, osp, zeros, split=True)
    wp, b = U.pack_conv_weight_mix8(w, DEV)
    got, partial = U.conv3d_mix8(U.mix8_of(xj).to(DEV), wp, b, bias, osp, zeros)
    torch.cuda.synchronize()
    e_split = (_cf(U.join_pair(sp.cpu()).double()) - ref).abs().max().item()
    e_mix = (_cf(U.join_pair(got.cpu()).double()) - ref).abs().max().item()
    e_f16 = (F.conv3d(_cf(xj.half().float()), w.half().float(), bias.cpu(), padding=1).double() - ref).abs().max().item()
    print(f"mix8 conv {osp}: max-abs split {e_split:.2e} mix8 {e_mix:.2e} fp16 operands {e_f16:.2e} (scale {scale:.2f})")
    assert e_mix <= 3e-5 * scale and e_mix <= e_f16 / 10 and e_split <= e_mix
    # sums over B * voxels * 4 values that differ by <= 5e-5 each (random sign): a few 1e-3 .. 1e-2
    assert torch.allclose(partial.sum(1), sp_partial.sum(1), rtol=1e-4, atol=3e-2)
    ox, oy, oz = osp
    box = (2, 3, 1, ox - 3, oy - 2, oz - 2)
    out = torch.full((B, ox, oy, oz, 2 * ch), 7.0, dtype=torch.float16, device=DEV)
    _, pbox = U.conv3d_mix8(U.mix8_of(xj).to(DEV), wp, b, bias, osp, zeros, store_box=box, out=out)
    torch.cuda.synchronize()
    assert torch.equal(pbox, partial)
    x0, y0, z0, x1, y1, z1 = box
    assert torch.equal(out[:, x0:x1, y0:y1, z0:z1], got[:, x0:x1, y0:y1, z0:z1])
    if ch == 32:   # the wider kernels store the whole tile (which satisfies the contract too)
        outside = torch.ones(osp, dtype=torch.bool, device=DEV)
        outside[x0:x1, y0:y1, z0:z1] = False
        assert bool((out[:, outside] == 7.0).all())


@pytest.mark.parametrize("ch", [32, 64, 128])
def test_groupnorm_silu_mix8_store(U, ch):
    """sk_groupnorm_silu_mix8: the hi halves equal sk_groupnorm_silu_split's bit for bit; x8 / lo8 are the e4m3 images (RNE,
    saturating) of 16 x and 2^15 (x - hi) of the same fp32 value x = silu(a (hi + lo) + b)."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(11)
    B, vox = 2, 5 * 7 * 12
    raw = U.split_pair(torch.randn((B, vox, ch), generator=gen) * 2).to(DEV)
    aff = torch.stack([torch.rand((B, ch), generator=gen) + 0.5, torch.randn((B, ch), generator=gen) * 0.5], dim=1).to(DEV)
    aff[0, 0, 3], aff[0, 1, 3] = 40.0, 20.0   # |x| beyond the fp8 range of 16 x (28) and of the lo8 scale
    st = _ffi.stream_ptr(torch.device(DEV))
    want = raw.clone()
    _ffi.check(_ffi.lib.sk_groupnorm_silu_split(_ffi.ptr(want), _ffi.ptr(aff), B, vox, ch, st))
    got = raw.clone()
    _ffi.check(_ffi.lib.sk_groupnorm_silu_mix8(_ffi.ptr(got), _ffi.ptr(aff), B, vox, ch, st))
    torch.cuda.synchronize()
    want, got = want.cpu(), got.cpu()
    assert torch.equal(got[..., :ch], want[..., :ch])
    x = U.join_pair(want)   # hi + lo of the split store: x to ~2^-22
    tail = got[..., ch:].contiguous().view(torch.uint8).reshape(B, vox, ch // 32, 2, 32)   # per 32-channel chunk: x8 | lo8
    x8 = tail[..., 0, :].reshape(B, vox, ch).view(torch.float8_e4m3fn).float()
    lo8 = tail[..., 1, :].reshape(B, vox, ch).view(torch.float8_e4m3fn).float()
    assert not torch.isnan(x8).any() and not torch.isnan(lo8).any()
    want8 = (x * 16).clamp(-448, 448)
    assert ((x8 - want8).abs() <= want8.abs() / 16 + 2.0 ** -9).all()        # half an e4m3 ulp (2^-4 relative), subnormal step 2^-9
    wantl = (want[..., ch:].float() * 32768).clamp(-448, 448)
    assert ((lo8 - wantl).abs() <= wantl.abs() / 16 + 2.0 ** -9 + 1e-3 * 32768 * 2.0 ** -22 * x.abs().clamp(min=1)).all()


def test_conv_exact_integer_layout(U):
    """Asymmetric small-integer operands: checks the MFMA operand / accumulator maps exactly."""
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (1, 32, 6, 9, 20), generator=gen).half()
    w = torch.randint(-2, 3, (32, 32, 3, 3, 3), generator=gen).float()
    b = torch.randint(-4, 5, (32,), generator=gen).float()
    want = F.conv3d(x.float(), w, b, padding=1)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    got, _ = U.conv3d([(_cl(x).to(DEV), 0)], U.pack_conv_weight(w, DEV), b.to(DEV), 32, 3, (6, 9, 20), zeros)
    assert torch.equal(_cf(got.cpu().float()), want)  # all values are small integers: exact in fp16


@pytest.mark.parametrize("nblk,C", [(423, 32), (5000, 32), (131072, 32), (9000, 128)])
def test_groupnorm_finalize_many_rows(U, nblk, C):
    """More than 4096 partial rows per sample (256^3 training crops) take the two-level reduction: same statistics as
    a double-precision sum of the rows."""
    from skoots_amd import _ffi
    gen = torch.Generator().manual_seed(nblk + C)
    B, groups, vox = 2, 8, 1000
    part = torch.rand((B, nblk, C // 4, 2), generator=gen) * 3.0
    part[..., 1] += 5.0  # sum of squares > (sum)^2 / n
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    n = float(nblk * vox) * (C // groups)
    tot = part.double().sum(dim=1)                                    # (B, C/4, 2)
    gq = C // groups // 4                                              # quads per group
    gsum = tot.reshape(B, groups, gq, 2).sum(dim=2)                    # (B, groups, 2)
    mean = gsum[..., 0] / n
    var = (gsum[..., 1] / n - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    a_want = gamma.double().view(1, C) * rstd.repeat_interleave(C // groups, dim=1)
    b_want = beta.double().view(1, C) - mean.repeat_interleave(C // groups, dim=1) * a_want
    dev = torch.device(DEV)
    pd = part.to(dev).contiguous()
    affine = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
    gd, bd = gamma.to(dev), beta.to(dev)   # keep the device copies alive across the call
    _ffi.check(_ffi.lib.sk_groupnorm_finalize(_ffi.ptr(pd), B, nblk, groups, C, nblk * vox, _ffi.ptr(gd),
                                              _ffi.ptr(bd), 1e-5, _ffi.ptr(affine), _ffi.stream_ptr(dev)))
    got = affine.cpu().double()
    assert torch.allclose(got[:, 0], a_want, rtol=2e-5, atol=0)
    assert torch.allclose(got[:, 1], b_want, rtol=2e-5, atol=2e-5)


def test_groupnorm_silu_vs_torch(U):
    gen = torch.Generator().manual_seed(5)
    for C_, sp in ((32, (8, 12, 20)), (64, (6, 10, 10)), (128, (5, 9, 5))):
        x = torch.randn((2, C_) + sp, generator=gen).half()
        w = torch.zeros((C_, C_, 1, 1, 1))
        for i in range(C_):
            w[i, i] = 1.0
        zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
        raw, partial = U.conv3d([(_cl(x).to(DEV), 0)], U.pack_conv_weight(w, DEV),
                                torch.zeros(C_, device=DEV), C_, 1, sp, zeros)
        gamma = torch.rand(C_, generator=gen) + 0.5
        beta = torch.rand(C_, generator=gen) - 0.5
        got = U.groupnorm_silu_(raw, partial, gamma.to(DEV), beta.to(DEV))
        want = F.silu(F.group_norm(x.float(), 8, gamma, beta, eps=1e-5))
        assert (_cf(got.cpu().float()) - want).abs().max().item() <= 3e-3


def _oracle_and_hip(U, seed=101196):
    from oracle import unet_spec
    ref = unet_spec.build(seed)
    hip = U.HipUNet.from_module(ref, DEV)
    return ref, hip


def test_stem_vs_torch(U):
    ref, hip = _oracle_and_hip(U)
    gen = torch.Generator().manual_seed(2)
    vol = torch.randint(0, 256, (40, 36, 28), generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    origins = [(0, 0, 0), (8, 4, 8)]
    tile = (32, 32, 20)
    hip.forward_tiles(vol.to(DEV), origins, tile, mean, std, keep_features=True)
    got = hip.last_features["enc0.0"].cpu().float()
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + 32, y:y + 32, z:z + 20][None, None]
        crop = crop.sub(mean).div(std).float()  # eval.py:139 semantics (fp16 arithmetic)
        with torch.no_grad():
            want = ref.enc0[0](crop)
        # activated features reach |v| ~ 8 where one fp16 ulp is 7.8e-3: relative bound
        err = ((_cf(got[b:b + 1]) - want).abs() / (1.0 + want.abs())).max().item()
        assert err <= 1.5e-3, err


@pytest.mark.parametrize("tile,origins", [((64, 64, 20), [(0, 0, 0)]),
                                           ((32, 48, 20), [(3, 1, 2), (10, 0, 0)]),
                                           ((128, 128, 20), [(0, 0, 12)]),
                                           ((30, 45, 18), [(0, 0, 0)])])   # padded up to (32, 48, 20)
def test_network_vs_oracle(U, tile, origins):
    """Whole U-Net on the GPU against the torch fp32 CPU oracle (oracle/unet_spec.py).

    Tolerance: BASELINE.json's north_star states 1e-3 for the embedding / probability
    tensors.  With fp16 MFMA operands (the dtype BASELINE's configs name) that bound holds
    in the RMS sense and is asserted so: rms <= 1e-3 (measured 4.4e-4), plus a max-abs
    guard of 1e-2 (measured 4.9e-3).  A max-abs of 1e-3 against fp32 is not reachable with
    fp16 operands on this random-init network: rounding ONLY the weights to fp16 in the
    fp32 torch graph already moves the outputs by 2.8e-3 max-abs (DESIGN.md "numerics").
    Kernel correctness itself is pinned per layer in test_conv_vs_torch (1 fp16 ulp).
    The second check bounds the GPU path by the error of the same graph evaluated in torch
    with the HIP path's storage precision (forward_fp16_storage): the kernels add nothing
    beyond what fp16 storage costs.
    """
    from oracle import unet_spec
    ref, hip = _oracle_and_hip(U)
    gen = torch.Generator().manual_seed(tile[0])
    shape = tuple(max(o[k] for o in origins) + tile[k] for k in range(3))
    vol = torch.randint(0, 256, shape, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std).cpu().float()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + tile[0], y:y + tile[1], z:z + tile[2]][None, None].sub(mean).div(std).float()
        with torch.no_grad():
            want32 = ref(crop)[0]
            want16 = unet_spec.forward_fp16_storage(ref, crop)[0]
        e32 = (out5[b] - want32).abs()
        emu = (want16 - want32).abs()
        print(f"tile {b}: gpu vs fp32 rms {rms(e32):.2e} max {e32.max():.2e} | "
              f"fp16-storage emulation vs fp32 rms {rms(emu):.2e} max {emu.max():.2e}")
        assert rms(e32) <= 1e-3 and e32.max().item() <= 1e-2
        assert rms(e32) <= 1.25 * rms(emu) + 1e-5


@pytest.mark.parametrize("tile,origins", [((64, 64, 20), [(0, 0, 0)]), ((32, 48, 20), [(3, 1, 2), (10, 0, 0)]),
                                           ((30, 45, 18), [(0, 0, 0)]), ((13, 22, 7), [(0, 0, 0)])])
@pytest.mark.parametrize("precision", ["split", "mix8"])
def test_network_split_mode_vs_oracle(U, tile, origins, precision):
    """precision="split": matrix-core path (fp16 hi + lo operand pairs) that meets BASELINE.json's north_star
    tolerance -- max-abs <= 1e-3 against the fp32 oracle on every output channel.  "mix8": the same with the two 32 -> 32
    convs' correction products on the block-scaled fp8 matrix instruction (sk_conv3d_mix8), same bound."""
    from oracle import unet_spec
    ref = unet_spec.build(101196)
    hip = U.HipUNet.from_module(ref, DEV, precision=precision)
    gen = torch.Generator().manual_seed(tile[0])
    shape = tuple(max(o[k] for o in origins) + tile[k] for k in range(3))
    vol = torch.randint(0, 256, shape, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std).cpu().float()
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + tile[0], y:y + tile[1], z:z + tile[2]][None, None].sub(mean).div(std).float()
        with torch.no_grad():
            want = ref(crop)[0]
        e = (out5[b] - want).abs()
        print(f"{precision} mode tile {b}: max abs err {e.max().item():.2e} rms {e.pow(2).mean().sqrt().item():.2e}")
        assert e.max().item() <= 1e-3


@pytest.mark.parametrize("tile,origins", [((64, 64, 20), [(0, 0, 0)]), ((32, 48, 20), [(3, 1, 2), (10, 0, 0)]),
                                           ((30, 45, 18), [(0, 0, 0)]), ((13, 22, 7), [(0, 0, 0)])])
def test_network_fp32_mode_vs_oracle(U, tile, origins):
    """precision="fp32": the same tiling / normalisation / GroupNorm / heads plumbing on the exact-fp32
    matrix instruction.  Max-abs <= 1e-3 against the fp32 oracle -- the tolerance BASELINE.json's
    north_star states (measured ~1e-5) -- which pins every difference of the fp16 fast path on
    operand rounding."""
    from oracle import unet_spec
    ref = unet_spec.build(101196)
    hip = U.HipUNet.from_module(ref, DEV, precision="fp32")
    gen = torch.Generator().manual_seed(tile[0])
    shape = tuple(max(o[k] for o in origins) + tile[k] for k in range(3))
    vol = torch.randint(0, 256, shape, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std).cpu()
    assert out5.dtype == torch.float32
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + tile[0], y:y + tile[1], z:z + tile[2]][None, None].sub(mean).div(std).float()
        with torch.no_grad():
            want = ref(crop)[0]
        err = (out5[b] - want).abs().max().item()
        print(f"fp32 mode tile {b}: max abs err {err:.2e}")
        assert err <= 1e-3


@pytest.mark.parametrize("tile,origins", [((32, 48, 20), [(3, 1, 2), (10, 0, 0)]), ((13, 22, 7), [(0, 0, 0)])])
def test_network_fp32_mode_vs_float64_oracle(U, tile, origins):
    """precision="fp32" against the FLOAT64 oracle (the same module, .double(), on the same crop): max-abs <= 1e-4.
    The bound follows from the mode's role, not from a measurement of it: what certifies the 1e-3 claims of `split` and
    `mix8` (test_hip_geometry.py, bench.py's parity_vs_fp32_mode) has to be ten times finer than the claim, and has to
    stay below `split`'s own 2.5e-4 -- the 1e-3 of test_network_fp32_mode_vs_oracle would let it degrade to `split`'s
    accuracy unnoticed.  The fp32 CPU oracle's own distance from float64 is printed next to it.
    Measured: fp32 CPU oracle 2.1e-6 .. 3.6e-6 from float64; the MI355X fp32 mode 7.8e-6 and 8.7e-6 on the two
    (32, 48, 20) tiles, 6.4e-6 on (13, 22, 7)."""
    import copy

    from oracle import unet_spec
    ref = unet_spec.build(101196)
    ref64 = copy.deepcopy(ref).double()
    hip = U.HipUNet.from_module(ref, DEV, precision="fp32")
    gen = torch.Generator().manual_seed(tile[0])
    shape = tuple(max(o[k] for o in origins) + tile[k] for k in range(3))
    vol = torch.randint(0, 256, shape, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std).cpu()
    assert out5.dtype == torch.float32
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + tile[0], y:y + tile[1], z:z + tile[2]][None, None].sub(mean).div(std).float()
        with torch.no_grad():
            want64 = ref64(crop.double())[0]
            want32 = ref(crop)[0]
        err = (out5[b].double() - want64).abs().max().item()
        e_cpu = (want32.double() - want64).abs().max().item()
        print(f"fp32 mode tile {b} vs float64: max abs err {err:.2e} | fp32 CPU oracle vs float64 {e_cpu:.2e}")
        assert err <= 1e-4


@pytest.mark.parametrize("shape,precision", [((140, 132, 34), "fp32"), ((190, 186, 18), "fp32"),  # second: thinner than the
                                             ((140, 132, 34), "split")])                          # tile, no extent % 4 == 0
def test_end_to_end_with_network_fp32_mode(U, shape, precision):
    """Whole eval path WITH the network (no injected field) in the two <= 1e-3 modes against the CPU oracle on
    the same volume: vectors within 1e-3 wherever both gates agree, and the thresholded skeleton /
    final instance masks differ only where a probability sits within the mode's error (fp32 ~1e-5, split ~2.5e-4)
    of the 0.8 threshold."""
    import numpy as np
    from oracle import pipeline as O
    from oracle import unet_spec
    from skoots_amd.lib import eval as E
    ref = unet_spec.build(7)
    with torch.no_grad():  # open the semantic gate, put the skeleton map around its threshold
        ref.heads.bias[4] = 3.0
        ref.heads.bias[3] = 1.4
        ref.heads.weight[0:3].mul_(0.15)
    hip = U.HipUNet.from_module(ref, DEV, precision=precision)
    gen = torch.Generator().manual_seed(3)
    vol = torch.randint(0, 256, (1,) + shape, generator=gen).to(torch.float16)
    with torch.no_grad():
        want = O.eval_volume(vol, ref, (60, 60, 12))
    got = E.eval_volume(vol.to(DEV), hip, (60, 60, 12), keep_planar_vectors=True)
    sk_w, sk_g = want["skeleton"][0], got["skeleton"].cpu().numpy()
    assert sk_w.sum() > 1e-3 * sk_w.size
    flips = 1e-4 if precision == "fp32" else 2e-3   # voxels whose probability lies within the mode's error of 0.8
    assert (sk_w != sk_g).mean() < flips
    v_w, v_g = want["vectors"].astype(np.float32), got["state"].vec_planar.cpu().numpy().astype(np.float32)
    both = (np.abs(v_w).sum(0) > 0) == (np.abs(v_g).sum(0) > 0)
    assert both.mean() > 1 - flips
    assert np.abs(v_w - v_g)[:, both].max() <= 1e-3
    if (sk_w == sk_g).all() and both.all():
        # identical gates -> the integer stages must agree bit for bit
        assert np.array_equal(got["instance_mask"].cpu().numpy(), want["instance_mask"])
    else:
        assert (got["instance_mask"].cpu().numpy() != want["instance_mask"]).mean() < 5e-3


def test_eval_is_deterministic(U):
    """Same volume, same weights, two runs of the whole path (fast fp16 network included): bit-identical vectors,
    skeleton, labels and instance mask -- every reduction in the kernels has a fixed order, the label kernels'
    atomics are min/first-seen only."""
    from skoots_amd.lib import eval as E
    hip = U.smoke_model(DEV)
    gen = torch.Generator().manual_seed(11)
    vol = torch.randint(0, 256, (1, 150, 140, 30), generator=gen).to(torch.float16).to(DEV)
    a = E.eval_volume(vol, hip, (60, 60, 12), keep_planar_vectors=True)
    b = E.eval_volume(vol, hip, (60, 60, 12), keep_planar_vectors=True)
    assert torch.equal(a["state"].vec4, b["state"].vec4)
    assert torch.equal(a["skeleton"], b["skeleton"])
    assert torch.equal(a["labels"], b["labels"])
    assert torch.equal(a["instance_mask"], b["instance_mask"])
    assert a["n_instances"] == b["n_instances"]


@pytest.mark.parametrize("dims,depths", [((32, 32, 64, 32, 32), (1, 2, 3, 2, 1)), ((32, 64, 64, 64, 32), (3, 1, 1, 1, 3)),
                                         ((32, 128, 128, 128, 32), (2, 2, 1, 2, 2))])
@pytest.mark.parametrize("precision", ["fp16", "split", "mix8"])
def test_network_other_widths_and_depths_vs_oracle(U, dims, depths, precision):
    """MODEL.DIMS / MODEL.DEPTHS other than the default (lib/utils.py:46-57 reads them from the checkpoint's cfg): every width
    the kernels are built for on each level, blocks of depth 1 (the stem feeds the stride-2 conv directly; a decoder level is
    its concat conv alone) and 3 (a middle layer between two 3x3x3 convs), in the three fast precisions against the fp32
    oracle -- the fused-activation and mix8 hand-offs are decided per layer from these."""
    from oracle import unet_spec
    ref = unet_spec.build(11, dims=dims, depths=depths)
    hip = U.HipUNet.from_module(ref, DEV, precision=precision)
    tile, origins = (36, 40, 20), [(0, 0, 0), (5, 3, 2)]
    gen = torch.Generator().manual_seed(sum(dims) + sum(depths))
    shape = tuple(max(o[k] for o in origins) + tile[k] for k in range(3))
    vol = torch.randint(0, 256, shape, generator=gen).to(torch.float16)
    mean, std = float(vol.mean()), float(vol.std())
    out5 = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std).cpu().float()
    box = ([4, 6, 3], [30, 33, 17])
    boxed = hip.forward_tiles(vol.to(DEV), origins, tile, mean, std, out_box=box).cpu().float()
    for b, (x, y, z) in enumerate(origins):
        crop = vol[x:x + tile[0], y:y + tile[1], z:z + tile[2]][None, None].sub(mean).div(std).float()
        with torch.no_grad():
            want = ref(crop)[0]
        e = (out5[b] - want).abs().max().item()
        print(f"dims {dims} depths {depths} {precision} tile {b}: max abs err {e:.2e}")
        assert e <= (1e-2 if precision == "fp16" else 1e-3)
        (x0, y0, z0), (x1, y1, z1) = box
        assert torch.equal(boxed[b][:, x0:x1, y0:y1, z0:z1], out5[b][:, x0:x1, y0:y1, z0:z1])
