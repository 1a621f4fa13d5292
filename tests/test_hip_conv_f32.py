"""GPU tests of the fp32 kernels of skoots_amd/csrc/conv3d_f32.hip through the C ABI -- sk_conv3d_f32 (conv_f32_lds_kernel,
conv_f32_kernel), sk_train_conv_dgrad (the same two kernels transposed, conv_t2_f32_kernel, pointwise_dgrad_kernel<5>) and
sk_groupnorm_silu_f32 -- against float64 references of the same operations (tests/conv_f32_cases.py).

precision="fp32" is what every fast precision of this project is measured against, so these kernels are held tighter than
the ones they certify:

  * integer operands: v_mfma_f32_32x32x2_f32 is an fmaf chain, so with every partial sum an integer below 2^24
    (tests/test_conv_f32_cases_cpu.py) the result is the float64 result BIT FOR BIT in any summation order.  Zero tolerance
    on every tap, lane map, halo, x-plane window, tile seam, cout tile and GroupNorm partial row;
  * realistic operands: 1 / 20 of what rounding the operands to fp16 costs on the same data, computed from the reference;
  * every buffer the kernels write carries a sentinel tail that must survive.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import conv_f32_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0
TAIL = 4096               # sentinel elements behind every written buffer (more than a partial row of any case)
IDS = [K.case_id(c) for c in K.CASES]


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _st(ffi):
    return ffi.stream_ptr(torch.device(DEV))


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


def _tailed(shape, fill=SENT):
    """(whole allocation, view of `shape` at its start): `shape` elements followed by TAIL more, all `fill`"""
    n = 1
    for s in shape:
        n *= s
    big = torch.full((n + TAIL,), fill, dtype=torch.float32, device=DEV)
    return big, big[:n].view(shape)


def _tail_intact(big):
    return bool((big[-TAIL:] == SENT).all())


def _src_array(ffi, case, srcs):
    dev = [_cl(t.float()).to(DEV) for t in srcs]
    arr = (ffi.ConvSrc * len(dev))()
    for a, t, (c, up) in zip(arr, dev, case[2]):
        a.data, a.affine, a.c, a.upsample = t.data_ptr(), None, c, up
    return arr, dev


def _run_conv(ffi, case, srcs, w, b):
    """sk_conv3d_f32 on a case -> (out (B, ox, oy, oz, cout), partial (B, rows, cout / 4, 2) or None), both on the CPU,
    after asserting that the sentinel tails behind both are untouched"""
    B, (ox, oy, oz), _, cout, k = case
    arr, keep = _src_array(ffi, case, srcs)
    wd, bd = w.float().to(DEV).contiguous(), b.float().to(DEV)
    big_o, out = _tailed((B, ox, oy, oz, cout))
    rows = ffi.lib.sk_conv3d_f32_num_blocks(ox, oy, oz)
    assert rows == K.num_rows(case)
    big_p = partial = None
    if K.has_partials(case):
        big_p, partial = _tailed((B, rows, cout // 4, 2))
    ffi.check(ffi.lib.sk_conv3d_f32(arr, len(keep), ffi.ptr(wd), ffi.ptr(bd), ffi.ptr(out), B, ox, oy, oz, cout, k,
                                    ffi.ptr(partial), _st(ffi)))
    torch.cuda.synchronize()
    assert _tail_intact(big_o), "sk_conv3d_f32 wrote behind out"
    assert big_p is None or _tail_intact(big_p), "sk_conv3d_f32 wrote behind gn_partial"
    return out.cpu(), None if partial is None else partial.cpu()


# ============================================================================================ a: exact
@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_conv_f32_exact_on_integer_operands(ffi, case):
    """Integer activations in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]: `out` equals the float64 conv bit for
    bit; gn_partial, prefilled with 7.0, equals the float64 sum and sum of squares of every 128-voxel row and channel
    quad, row by row (the layout sk_conv3d_f32_num_blocks promises, not only its totals); nothing is written behind
    either buffer."""
    srcs, w, b, want, want_rows = K.integer_expected(case)
    out, partial = _run_conv(ffi, case, srcs, w, b)
    got = _cf(out).double()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        pytest.fail(f"{len(bad)} of {want.numel()} outputs differ; first at (b, c, x, y, z) = {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}")
    if want_rows is None:
        assert partial is None
        return
    gp = partial.double()
    if not torch.equal(gp, want_rows):
        bad = (gp != want_rows).nonzero()
        pytest.fail(f"{len(bad)} partial entries differ; first at (b, row, quad, sum | sumsq) = {bad[0].tolist()}: "
                    f"{gp[tuple(bad[0])].item()} != {want_rows[tuple(bad[0])].item()}")


# ============================================================================================ b: realistic
@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_conv_f32_realistic_vs_float64(ffi, case):
    """randn activations, randn / sqrt(cin k^3) weights, 0.1 randn biases against the float64 conv, max-abs error over
    max(1, max |ref|).  Bound: e16 / 20, e16 the error of the float64 conv of the fp16-rounded operands of this very
    case (2.5e-4 .. 4.2e-4, so the bound is 1.25e-5 .. 2.1e-5): any fp16 / bf16 operand fails it twentyfold.  Partial
    totals (the rows summed in float64) against the float64 totals: allclose(rtol = 1e-5, atol = 1e-4), what the split
    tests grant their totals.
    Measured on the MI355X (torch's fp32 CPU conv, e32, on the same data: 1.9e-7 .. 4.9e-7): the gather kernel and the
    k = 1 / k = 2 cases 1.8e-7 .. 1.1e-6; the 3x3x3 LDS cases 8.0e-7 (K = 864) .. 2.2e-6 (K = 3456) .. 3.1e-6 (K = 6912) --
    one sequential fmaf chain over K, where torch sums in blocks -- i.e. 5.5 .. 100 times below the bound and
    110 .. 2000 times below e16.  Partial totals: sums off by <= 1.2e-4 absolute and at most 0.33 of
    1e-4 + 1e-5 |ref|; sums of squares <= 5.6e-7 relative, at most 0.05 of theirs."""
    srcs, w, b, want, want_rows, e32, e16 = K.realistic_expected(case)
    out, partial = _run_conv(ffi, case, srcs, w, b)
    err = K.rel_err(_cf(out), want)
    print(f"{K.case_id(case)}: kernel {err:.2e} | torch fp32 {e32:.2e} | fp16 operands {e16:.2e} | bound {e16 / 20:.2e}")
    assert err <= e16 / 20, f"{err:.3e} > e16 / 20 = {e16 / 20:.3e}"
    if want_rows is None:
        return
    tot = partial.double().sum(dim=1)                                # (B, quads, 2)
    ref = want_rows.sum(dim=1)
    d = (tot - ref).abs()
    used = (d / (1e-4 + 1e-5 * ref.abs())).amax(dim=(0, 1))
    print(f"{K.case_id(case)}: partial totals: sums off by <= {d[..., 0].max().item():.2e} ({used[0].item():.3f} of the "
          f"allowance), sums of squares by <= {(d[..., 1] / ref[..., 1]).max().item():.2e} relative "
          f"({used[1].item():.3f} of the allowance)")
    assert torch.allclose(tot, ref, rtol=1e-5, atol=1e-4)


# ============================================================================================ c: data gradients
DGRAD_CASES = [
    # (B, out spatial, cout, cin_total, cin_lo, cin_n, ksize): shapes of rows 1, 2, 5, 6, 7 of test_hip_train.BWD_CASES
    (2, (6, 5, 4), 32, 96, 32, 64, 3),      # the transposed LDS kernel on a channel sub-range, two tiles of rows
    (1, (6, 8, 4), 32, 96, 32, 64, 3),
    (2, (3, 4, 2), 64, 32, 0, 32, 2),       # conv_t2_f32_kernel: all eight parity classes
    (1, (5, 3, 4), 64, 128, 0, 128, 1),     # 128 -> 64 pointwise
    (2, (6, 5, 4), 5, 32, 0, 32, 1),        # the heads: pointwise_dgrad_kernel<5>
]


@pytest.mark.parametrize("B,osp,cout,cin,lo,n,k", DGRAD_CASES, ids=[f"k{c[6]}-{c[3]}to{c[2]}-{c[4]}+{c[5]}-B{c[0]}" for c in DGRAD_CASES])
def test_conv_f32_dgrad_exact(ffi, B, osp, cout, cin, lo, n, k):
    """sk_train_conv_dgrad on integer dy in [-2, 2] and weights in {-1, 0, 1} (sum |dy||w| <= 2 * 27 * 64 < 2^24: exact in
    any order) equals float64 autograd of the conv bit for bit: accumulate = 0 onto a sentinel fill, then accumulate = 1
    onto an integer fill in [-8, 8].  Nothing is written behind dx."""
    g = torch.Generator().manual_seed(cout * 7 + cin + k + osp[0])
    s = 2 if k == 2 else 1
    isp = tuple(v * s for v in osp)
    w = torch.randint(-1, 2, (cout, cin, k, k, k), generator=g).double()
    dy = torch.randint(-2, 3, (B, cout) + osp, generator=g).double()
    x = torch.zeros((B, cin) + isp, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w, None, padding=1) if k == 3 else F.conv3d(x, w, None, stride=k)
    y.backward(dy)
    want = _cl(x.grad[:, lo:lo + n])                                  # (B, isp, n)
    assert want.abs().max() > 0 and torch.equal(want, want.round())
    dyd, wd = _cl(dy.float()).to(DEV), w.float().to(DEV).contiguous()
    ox, oy, oz = osp
    big, dx = _tailed((B,) + isp + (n,))
    call = lambda acc: ffi.check(ffi.lib.sk_train_conv_dgrad(ffi.ptr(dyd), ffi.ptr(wd), ffi.ptr(dx), B, ox, oy, oz, cout,
                                                              cin, lo, n, k, acc, _st(ffi)))
    call(0)
    torch.cuda.synchronize()
    assert _tail_intact(big)
    assert torch.equal(dx.cpu().double(), want), "accumulate = 0"
    pre = torch.randint(-8, 9, dx.shape, generator=g).float()
    dx.copy_(pre)
    call(1)
    torch.cuda.synchronize()
    assert _tail_intact(big)
    assert torch.equal(dx.cpu().double(), want + pre.double()), "accumulate = 1"


# ============================================================================================ d: GroupNorm + SiLU pass
EDGE_IMAGES = [0.0, 1e-30, -1e-30, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4]


def _ulp32(a):
    """fp32 ulp at magnitude |a| (float64 tensor): 2^(e - 23) for |a| in [2^e, 2^(e + 1)), 2^-149 below 2^-126"""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), (e - 24).to(torch.int32))


@pytest.mark.parametrize("vox", [420, 9600])
@pytest.mark.parametrize("Cc", [32, 64, 128])
def test_groupnorm_silu_f32_vs_float64(ffi, Cc, vox):
    """sk_groupnorm_silu_f32 in place, B = 2 with a different affine per sample, against float64 silu(a x + b) of the same
    fp32 a, x, b.  Planted in both samples, at the first and the last voxels: inputs whose affine image is 0, +-1e-30,
    +-88, +-104 (expf overflows) and +-1e4 -- exactly in channel 0 (b = 0), through a non-zero offset in channel 1 (a = 2).
    Every output is finite; an image <= -88 gives a result <= 0 of magnitude < 1e-34, not NaN.

    Bound per element: 8 x the error of torch's fp32 CPU evaluation of y / (1 + exp(-y)) (y the fp32 rounding of a x + b,
    which is what fmaf returns) against float64 -- with that error taken as at least half an fp32 ulp of the reference:
    the CPU value is the correctly rounded one for a good share of 2.4 M elements, and no fp32 result can be asked to
    beat the format -- and never more than 2e-5 max |ref|, what test_gn_silu_backward grants sk_train_gn_silu.  The factor
    covers a device expf an ulp or two off libm's.  Measured on the MI355X: the worst element uses 0.55 .. 0.62 of its
    bound over the six cases (2.5 ulp where the CPU evaluation is within half an ulp); the largest absolute error,
    4.4e-4, sits at |ref| = 1e4 (half an ulp there): 4.4e-8 max |ref|."""
    B = 2
    g = torch.Generator().manual_seed(Cc + vox)
    x = torch.randn((B, vox, Cc), generator=g) * 2
    aff = torch.stack([(torch.rand((B, Cc), generator=g) + 0.5) * torch.tensor([[1.0], [1.7]]),
                       torch.randn((B, Cc), generator=g) * 0.5 + torch.tensor([[0.0], [0.3]])], dim=1).contiguous()
    aff[:, 1, 0] = 0.0
    aff[:, 0, 1] = 2.0
    img = torch.tensor(EDGE_IMAGES, dtype=torch.float64)
    ne = len(EDGE_IMAGES)
    for at in (slice(0, ne), slice(vox - ne, vox)):
        for b in range(B):
            x[b, at, 0] = (img / aff[b, 0, 0].double()).float()
            x[b, at, 1] = ((img - aff[b, 1, 1].double()) / 2).float()
    a64, b64 = aff[:, 0:1].double(), aff[:, 1:2].double()
    y64 = a64 * x.double() + b64
    ref = y64 / (1 + torch.exp(-y64))
    y32 = y64.float()
    cpu = y32 / (1 + torch.exp(-y32))
    for b in range(B):                                               # the planted images are what they should be
        assert y32[b, 0, 0] == 0 and y32[b, 0, 1] == 0
        assert ((y32[b, :ne, 0].double() - img).abs() <= 1e-6 * img.abs()).all()
        big_img = img.abs() >= 88                                    # channel 1 cannot hold 1e-30 next to its offset
        assert ((y32[b, :ne, 1].double() - img).abs() <= 1e-6 * img.abs())[big_img].all()
    assert torch.isfinite(ref).all() and torch.isfinite(cpu).all()
    xd, ad = x.to(DEV), aff.to(DEV)
    big, xv = _tailed((B, vox, Cc))
    xv.copy_(xd)
    ffi.check(ffi.lib.sk_groupnorm_silu_f32(ffi.ptr(xv), ffi.ptr(ad), B, vox, Cc, _st(ffi)))
    torch.cuda.synchronize()
    assert _tail_intact(big)
    got = xv.cpu()
    assert torch.isfinite(got).all()
    neg = y64 <= -87.9                                               # the planted -88 may land an ulp short of it
    assert int(neg.sum()) == 12 * B
    assert (got[neg] <= 0).all() and (got[neg].abs() < 1e-34).all()
    e_cpu = (cpu.double() - ref).abs()
    cap = 2e-5 * ref.abs().max().item()
    bound = (8 * torch.maximum(e_cpu, 0.5 * _ulp32(ref))).clamp_max(cap)
    err = (got.double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"C {Cc} vox {vox}: worst err / bound {worst:.3f}; max err {err.max().item():.2e} = "
          f"{err.max().item() / ref.abs().max().item():.2e} max|ref|; max err in ulp {(err / _ulp32(ref)).max().item():.2f}; "
          f"torch fp32 CPU: max {e_cpu.max().item():.2e}, {(e_cpu / _ulp32(ref)).max().item():.2f} ulp")
    assert (err <= bound).all(), f"worst err / bound {worst:.3f}"


# ============================================================================================ e: the whole layer
@pytest.mark.parametrize("case", [K.TWO_SOURCE_CASE, K.STRIDE2_CASE], ids=[K.case_id(K.TWO_SOURCE_CASE), K.case_id(K.STRIDE2_CASE)])
def test_fp32_layer_vs_float64(ffi, case):
    """sk_conv3d_f32 -> sk_groupnorm_finalize -> sk_groupnorm_silu_f32 (what HipUNet runs per layer in precision="fp32")
    against float64 silu(group_norm(conv, 8, gamma, beta, 1e-5)) on realistic operands.  Bound: 1 / 20 of the max-abs error
    of the same float64 layer with the conv's activations and weights rounded to fp16 (1.54e-3 and 1.38e-3: bounds 7.7e-5
    and 6.9e-5).  Measured on the MI355X: 6.3e-6 and 2.4e-6."""
    B, (ox, oy, oz), _, cout, k = case
    srcs, w, b, y64, *_ = K.realistic_expected(case)
    g = torch.Generator().manual_seed(cout + k)
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.rand(cout, generator=g) * 0.6 - 0.3
    layer = lambda y: F.silu(F.group_norm(y, 8, gamma.double(), beta.double(), 1e-5))
    ref = layer(y64)
    ref16 = layer(K.conv(case, [K.half_rounded(t) for t in srcs], K.half_rounded(w), b.double()))
    e16 = (ref16 - ref).abs().max().item()
    arr, keep = _src_array(ffi, case, srcs)
    wd, bd, gd, btd = w.to(DEV).contiguous(), b.to(DEV), gamma.to(DEV), beta.to(DEV)
    rows, vox = K.num_rows(case), ox * oy * oz
    big_o, out = _tailed((B, ox, oy, oz, cout))
    big_p, partial = _tailed((B, rows, cout // 4, 2))
    big_a, aff = _tailed((B, 2, cout))
    st = _st(ffi)
    ffi.check(ffi.lib.sk_conv3d_f32(arr, len(keep), ffi.ptr(wd), ffi.ptr(bd), ffi.ptr(out), B, ox, oy, oz, cout, k,
                                    ffi.ptr(partial), st))
    ffi.check(ffi.lib.sk_groupnorm_finalize(ffi.ptr(partial), B, rows, 8, cout, vox, ffi.ptr(gd), ffi.ptr(btd), 1e-5,
                                            ffi.ptr(aff), st))
    ffi.check(ffi.lib.sk_groupnorm_silu_f32(ffi.ptr(out), ffi.ptr(aff), B, vox, cout, st))
    torch.cuda.synchronize()
    assert _tail_intact(big_o) and _tail_intact(big_p) and _tail_intact(big_a)
    err = (_cf(out.cpu()).double() - ref).abs().max().item()
    print(f"{K.case_id(case)}: layer error {err:.2e} | fp16 conv operands {e16:.2e} | bound {e16 / 20:.2e}")
    assert err <= e16 / 20, f"{err:.3e} > {e16 / 20:.3e}"


# ============================================================================================ f: refusals
REFUSALS = [
    # (name, changes to the valid call: B 1, out (4, 6, 4), sources [(32, 0), (32, 1)], cout 32, ksize 3, partials)
    ("n_src_3", dict(n_src=3)),
    ("ksize_4", dict(ksize=4)),
    ("cout_48_with_partials", dict(cout=48)),
    ("upsampled_odd_extent", dict(osp=(4, 5, 4))),
    ("upsampled_ksize_1", dict(ksize=1)),
    ("affine", dict(affine=True)),
    ("B_0", dict(B=0)),
    ("ox_0", dict(osp=(0, 6, 4))),
    ("oy_0", dict(osp=(4, 0, 4))),
    ("oz_0", dict(osp=(4, 6, 0))),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_conv_f32_refuses_bad_arguments(ffi, name, kw):
    """n_src = 3, ksize = 4, cout = 48 with partials, an upsampled source with an odd extent or with ksize 1, a non-NULL
    source affine and B, ox, oy or oz < 1 raise ValueError (SK_ERR_ARG) before any launch: out and gn_partial, real device
    buffers larger than the valid call needs, keep their sentinel fill.  The valid call itself succeeds and writes both."""
    def call(B=1, osp=(4, 6, 4), n_src=2, cout=32, ksize=3, affine=False):
        src = [torch.zeros((2, 8, 12, 8, 32), device=DEV) for _ in range(3)]     # room for every variant
        arr = (ffi.ConvSrc * 3)()
        aff = torch.ones((2, 2, 32), device=DEV)
        for i, (a, t) in enumerate(zip(arr, src)):
            a.data, a.affine, a.c, a.upsample = t.data_ptr(), (aff.data_ptr() if affine and i == 0 else None), 32, int(i == 1)
        w = torch.ones((64, 96, 4, 4, 4), device=DEV)
        bias = torch.ones(64, device=DEV)
        out = torch.full((2 * 8 * 12 * 8 * 64,), SENT, device=DEV)
        partial = torch.full((2 * 16 * 16 * 2,), SENT, device=DEV)
        rc = ffi.lib.sk_conv3d_f32(arr, n_src, ffi.ptr(w), ffi.ptr(bias), ffi.ptr(out), B, osp[0], osp[1], osp[2], cout, ksize,
                                   ffi.ptr(partial), _st(ffi))
        torch.cuda.synchronize()
        return rc, out, partial

    rc, out, partial = call()
    ffi.check(rc)
    assert bool((out[:4 * 6 * 4 * 32] != SENT).all()) and bool((partial[:16] != SENT).all())
    rc, out, partial = call(**kw)
    with pytest.raises(ValueError):
        ffi.check(rc)
    assert bool((out == SENT).all()) and bool((partial == SENT).all()), "a refused call wrote a buffer"
