"""GPU tests of the fp16 and split conv kernels of skoots_amd/csrc/conv3d.hip through the C ABI -- sk_conv3d, sk_conv3d_split and
sk_conv3d_box on every instantiation they can launch (conv3_px_kernel, conv3_m16_kernel, conv3_kernel, down2_act_kernel,
gather_gemm_kernel, pointwise_lds_kernel; tests/test_conv16_cases_cpu.py asks the library which case reaches which and
holds its name list to the table's) -- against float64 references of the
same operations (tests/conv16_cases.py).

  * integer operands: fp16 products of small integers are exact and the MFMAs accumulate in fp32, so with every partial
    sum an integer below 2^24 (tests/test_conv16_cases_cpu.py) the output is the float64 conv BIT FOR BIT in any summation
    order, and so are the GroupNorm totals.  Zero tolerance on every tap, lane map, halo, x-chunk seam, ragged patch, cout
    tile and on every mask of the statistics: a voxel wrongly counted or left out moves a total by a nonzero integer;
  * split_exact operands: the same for the three products of precision "split" with all lo halves in play;
  * realistic operands: the fp16 kernels' totals within d16 / 10 of the definition each implements (sums of the stored 16-bit
    values, or of the fp32 accumulators), d16 the distance between the two on this very case;
  * every buffer the kernels write carries a sentinel tail that must survive; out and gn_partial are prefilled with 7.0.

The 2e-3 / 2e-5 output bounds on realistic operands stay where they are, in tests/test_hip_unet.py.
"""
import ctypes as C

import pytest
import torch

from tests import conv16_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0
TAIL = 4096               # sentinel elements behind every written buffer (more than a voxel line or a partial row of any case)
IDS = [K.case_id(c) for c in K.ALL]


@pytest.fixture(scope="module")
def env():
    from skoots_amd import _ffi, unet
    return _ffi, unet


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


def _tailed(shape, dtype):
    """(whole allocation, view of `shape` at its start): `shape` elements followed by TAIL more, all 7.0"""
    n = 1
    for s in shape:
        n *= s
    big = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
    return big, big[:n].view(shape)


def _tail_intact(big):
    return bool((big[-TAIL:] == SENT).all())


def _run(env, case, precision, lines, w, b, box=None):
    """sk_conv3d (precision "fp16"; with `box`: sk_conv3d_box) or sk_conv3d_split on a case.  `lines`: the sources as
    channels-last fp16 voxel lines on the CPU, (B, x, y, z, C) or, for split, (B, x, y, z, 2C) = [hi | lo].
    -> (out (B, ox, oy, oz, cout or 2 cout) fp16, partial (B, rows, cout / 4, 2) fp32), both on the CPU, after asserting that
    the row count is the mirror's and that the sentinel tails behind both buffers are untouched"""
    ffi, U = env
    B, (ox, oy, oz), srcdef, cout, k = case
    split = precision == "split"
    dev = [t.to(DEV) for t in lines]
    arr = (ffi.ConvSrc * len(dev))()
    for a, t, (c, up) in zip(arr, dev, srcdef):
        assert t.dtype == torch.float16 and t.shape[-1] == (2 * c if split else c)
        a.data, a.affine, a.c, a.upsample = t.data_ptr(), None, c, up
    wp, bd = U.pack_conv_weight(w, DEV, split=split), b.float().to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    rows = ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, cout, k)
    assert rows == K.num_blocks(case), f"sk_conv3d_num_blocks {rows}, the mirror {K.num_blocks(case)}"
    big_o, out = _tailed((B, ox, oy, oz, cout * (2 if split else 1)), torch.float16)
    big_p, partial = _tailed((B, rows, cout // 4, 2), torch.float32)
    st = ffi.stream_ptr(torch.device(DEV))
    if box is not None:
        assert not split
        rc = ffi.lib.sk_conv3d_box(arr, len(dev), ffi.ptr(wp), ffi.ptr(bd), ffi.ptr(out), B, ox, oy, oz, cout, k, ffi.ptr(partial),
                                   ffi.ptr(zeros), (C.c_int32 * 6)(*box), st)
    else:
        fn = ffi.lib.sk_conv3d_split if split else ffi.lib.sk_conv3d
        rc = fn(arr, len(dev), ffi.ptr(wp), ffi.ptr(bd), ffi.ptr(out), B, ox, oy, oz, cout, k, ffi.ptr(partial), ffi.ptr(zeros), st)
    ffi.check(rc)
    torch.cuda.synchronize()
    assert _tail_intact(big_o), "the kernel wrote behind out"
    assert _tail_intact(big_p), "the kernel wrote behind gn_partial"
    return out.cpu(), partial.cpu()


def _fp16_lines(srcs):
    return [_cl(t).half() for t in srcs]


def _pair_lines(his, los):
    return [torch.cat([_cl(h).half(), _cl(l).half()], dim=-1) for h, l in zip(his, los)]


def _same(got, want, what, index):
    """fail with the count and the first differing index unless got == want (float64, same shape)"""
    if torch.equal(got, want):
        return
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    pytest.fail(f"{len(bad)} of {want.numel()} {what} differ; first at {index} = {bad[0].tolist()}: "
                f"{got[tuple(bad[0])].item()!r} != {want[tuple(bad[0])].item()!r}")


def _totals(partial):
    """the rows of gn_partial summed in float64 -> (B, cout / 4, 2)"""
    return partial.double().sum(dim=1)


# ============================================================================================ a: fp16, integers
@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_conv_fp16_exact_on_integer_operands(env, case):
    """sk_conv3d on integer activations in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]: `out` equals the float64 conv bit
    for bit; gn_partial has sk_conv3d_num_blocks rows, as many as the mirror says, and its rows summed in float64 equal the
    float64 sums and sums of squares per (sample, quad) exactly -- whichever definition the epilogue implements, the stored
    values being the accumulators here; nothing is written behind either buffer."""
    srcs, w, b, want, want_tot = K.integer_expected(case)
    out, partial = _run(env, case, "fp16", _fp16_lines(srcs), w, b)
    _same(_cf(out).double(), want, "outputs", "(b, c, x, y, z)")
    assert not bool((partial == SENT).all(dim=(2, 3)).any()), "a row of gn_partial was left unwritten"
    _same(_totals(partial), want_tot, "totals", "(b, quad, sum | sumsq)")


# ============================================================================================ b: split, integers
@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_conv_split_exact_on_integer_operands(env, case):
    """sk_conv3d_split on the same integers as pairs with lo = 0 (the weights' lo halves are zero as well): the joined output
    equals the float64 conv bit for bit, the stored lo halves are all zero, the totals are exact, the row count is the
    mirror's and nothing is written behind either buffer."""
    srcs, w, b, want, want_tot = K.integer_expected(case)
    out, partial = _run(env, case, "split", _pair_lines(srcs, [torch.zeros_like(t) for t in srcs]), w, b)
    _same(_cf(K.join_pair(out)).double(), want, "outputs", "(b, c, x, y, z)")
    lo = out[..., case[3]:]
    assert not bool(lo.any()), f"{int((lo != 0).sum())} stored lo halves are not zero"
    assert not bool((partial == SENT).all(dim=(2, 3)).any()), "a row of gn_partial was left unwritten"
    _same(_totals(partial), want_tot, "totals", "(b, quad, sum | sumsq)")


# ============================================================================================ c: split, all three products
@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_conv_split_exact_three_products(env, case):
    """sk_conv3d_split on the split_exact operands -- hi in {-1, 0, 1}, lo = j 2^-13, weights +-1 + j 2^-13 -- on every ksize-3
    case and on the gather kernel's ksize 1 / 2 cases: the joined output equals conv(x_hi, w_hi) + conv(x_hi, w_lo) +
    conv(x_lo, w_hi) + b in float64 bit for bit.  That fixes what the integer test cannot see: the lane maps, halo and
    upsample addressing of the lo operands, the [lo, hi, hi] fragment order of the packed weight against the phase order
    (x_hi, w_lo), (x_hi, w_hi), (x_lo, w_hi), and that no lo * lo product is formed.  The totals are not exact here (sum |y| in
    units of 2^-13 passes 2^24): the rows summed in float64 against the float64 totals of the reference with the allowance of
    test_conv_split_vs_torch, rtol 1e-4 + atol 1e-3 sqrt(voxels) for the sums and rtol 1e-4 for the sums of squares.
    Measured on the MI355X over the 42 cases: the sums use at most 2.2e-3 of that allowance (0 in 18 cases), the sums of
    squares 3.5e-4 .. 1.5e-3 of theirs -- fp32 summation noise; a voxel wrongly counted would still show in tests a and b."""
    his, los, w, b, want, want_tot = K.split_exact_expected(case)
    out, partial = _run(env, case, "split", _pair_lines(his, los), w, b)
    _same(_cf(K.join_pair(out)).double(), want, "outputs", "(b, c, x, y, z)")
    tot = _totals(partial)
    nvox = case[1][0] * case[1][1] * case[1][2]
    allow = torch.stack([1e-3 * nvox ** 0.5 + 1e-4 * want_tot[..., 0].abs(), 1e-8 + 1e-4 * want_tot[..., 1].abs()], dim=-1)
    used = ((tot - want_tot).abs() / allow).amax(dim=(0, 1))
    print(f"{K.case_id(case)} [{K.route(case, 'split')}]: allowance used: sums {used[0].item():.2e}, sums of squares {used[1].item():.2e}")
    assert torch.allclose(tot[..., 0], want_tot[..., 0], rtol=1e-4, atol=1e-3 * nvox ** 0.5)
    assert torch.allclose(tot[..., 1], want_tot[..., 1], rtol=1e-4)


# ============================================================================================ d: fp16, realistic totals
# families whose fp16 epilogue sums its fp32 accumulators (pointwise_lds_kernel's adds x0 .. x3 of `acc` next to the
# rounding store, as gather_gemm_kernel's does); px, m16, conv3: the stored values
ACCUMULATORS = ("down2", "gather", "pointwise")


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_conv_fp16_realistic_totals(env, case):
    """sk_conv3d on randn fp16 activations, randn / sqrt(cin k^3) weights, 0.1 randn biases: what gn_partial holds.
    conv3_px_kernel, conv3_m16_kernel and conv3_kernel sum the values as STORED (the rounded 16-bit results, on v_dot2c);
    gather_gemm_kernel, pointwise_lds_kernel and down2_act_kernel sum their fp32 ACCUMULATORS (read from the code;
    include/skoots_hip.h says so too).  The rows summed in float64 are held to d16 / 10 of the definition the kernel implements -- computed from the kernel's
    own stored output for the first, from the float64 conv of the same fp16 operands for the second -- with d16 the distance
    between the two definitions on this case (tests/test_conv16_cases_cpu.py: fp32 summation error is at least ten times
    smaller still).  An epilogue that implements the other definition misses the bound tenfold.
    Measured on the MI355X over the 42 cases, in units of d16 (the bound is 0.1): stored values (px, m16, conv3) sums
    0.0003 .. 0.0010, sums of squares 0.0009 .. 0.0076; accumulators (down2, gather, pointwise) sums 0.0003 .. 0.0017, sums of squares
    0.0006 .. 0.0044; absolute 1.9e-6 .. 2.3e-5 and 9.3e-6 .. 4.8e-4.  The other definition lies 0.94 .. 1.04 d16 away."""
    srcs, w, b, y, t_acc, t_st, d16, _ = K.realistic_expected(case)
    out, partial = _run(env, case, "fp16", _fp16_lines(srcs), w, b)
    fam = K.family(K.route(case, "fp16"))
    stored = K.gn_totals(_cf(out))
    want, other = (t_acc, stored) if fam in ACCUMULATORS else (stored, t_acc)
    tot = _totals(partial)
    err = (tot - want).abs().amax(dim=(0, 1))
    far = (tot - other).abs().amax(dim=(0, 1))
    print(f"{K.case_id(case)} [{K.route(case, 'fp16')}, {'accumulators' if fam in ACCUMULATORS else 'stored values'}]: "
          f"sums off by {err[0].item():.2e} = {(err[0] / d16[0]).item():.4f} d16 (other definition: {(far[0] / d16[0]).item():.2f} d16) | "
          f"sums of squares {err[1].item():.2e} = {(err[1] / d16[1]).item():.4f} d16 (other: {(far[1] / d16[1]).item():.2f} d16)")
    assert bool((err <= d16 / 10).all()), f"totals off by {err.tolist()} > d16 / 10 = {(d16 / 10).tolist()}"
    # (not the output's bound, which tests/test_hip_unet.py holds: only that `stored` is no empty statement -- fp32 against
    # float64 accumulation turns the fp16 rounding of about one result in a thousand)
    assert (_cf(out) == y.half()).double().mean().item() >= 0.9


# ============================================================================================ e: the store box
@pytest.mark.parametrize("case", K.BOX_CASES, ids=[K.case_id(c) for c in K.BOX_CASES])
def test_conv_box_exact_on_integer_operands(env, case):
    """sk_conv3d_box on the integer operands, one case per route that honours a box (px, m16<4,3,2>, m16<4,3,1>, m16<4,3,0>,
    m16<3>), the box one voxel inside the tile on every side: inside the box `out` equals the float64 conv bit for bit, the
    totals are the WHOLE tile's, exactly, and outside the box the 7.0 prefill survives."""
    srcs, w, b, want, want_tot = K.integer_expected(case)
    ox, oy, oz = case[1]
    box = (1, 1, 1, ox - 1, oy - 1, oz - 1)
    out, partial = _run(env, case, "fp16", _fp16_lines(srcs), w, b, box=box)
    got = _cf(out).double()
    inside = torch.zeros(want.shape, dtype=torch.bool)
    inside[:, :, 1:ox - 1, 1:oy - 1, 1:oz - 1] = True
    assert inside.any() and not inside.all()
    _same(torch.where(inside, got, want), want, "outputs inside the box", "(b, c, x, y, z)")
    _same(torch.where(inside, torch.full_like(got, SENT), got), torch.full_like(got, SENT), "voxels outside the box", "(b, c, x, y, z)")
    _same(_totals(partial), want_tot, "totals", "(b, quad, sum | sumsq)")
