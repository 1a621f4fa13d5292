"""GPU tests of the training step's conv gradients in skoots_amd/csrc/train.hip through the C ABI, bit for bit against float64
(tests/train_grad_cases.py; tests/test_train_grad_cases_cpu.py proves which case reaches which kernel and that the operands
make bit equality a fair demand).  Nothing here takes a tolerance: every comparison is torch.equal / np.array_equal.

  * the weight gradient: all 14 instantiations behind sk_train_conv_wgrad, sk_train_conv_wgrad_f16 (with and without a zero
    page) and sk_train_stem_wgrad_f16, fp16 build and bf16 twin, with a power-of-two dy_scale other than 1, without a scale,
    without dbias, on cases whose 16-rounded chunks leave the last chunks of an item empty, twice for determinism; the
    workspace, dweight and dbias carry sentinel tails that must survive and are prefilled with the sentinel; the exported
    workspace size equals the mirror's on every run (the probe sweep of that size is a host-only test:
    tests/test_train_grad_cases_cpu.py);
  * sk_train_pack_weight: transposed 0 against the host packer's bytes; transposed 1 and 2 through sk_conv3d (and
    sk_train_interleave2) against the float64 data gradient;
  * the 16-bit data-gradient chain -- sk_train_interleave2, _add16, _h, sk_train_sumpool2, _f16, _hh, sk_train_cast_f16_f32 --
    each against a numpy restatement on integer payloads and power-of-two scales.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_grad_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25            # no gradient of these cases is near it
TAIL = 4096               # sentinel elements behind every written buffer
K = T.SCALE_K
TWINS = [False, True]


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


def _dt(twin):
    return torch.bfloat16 if twin else torch.float16


def _fn(ffi, name, twin):
    return getattr(ffi.lib, name + ("_bf16" if twin else ""))


def _tailed(shape, dtype=torch.float32, fill=SENT):
    """(whole allocation, view of `shape` at its start): `shape` elements followed by TAIL more, all `fill`"""
    n = int(np.prod(shape))
    big = torch.full((n + TAIL,), fill, dtype=dtype, device=DEV)
    return big, big[:n].view(shape)


def _tail_intact(big, fill=SENT):
    return bool((big[-TAIL:] == fill).all())


def _scale(k):
    return torch.tensor([2.0 ** k, 2.0 ** -k, 0.0], device=DEV)


def _same(got, want, what):
    """fail with the count and the first differing index unless got == want (same shape, float64)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    pytest.fail(f"{what}: {len(bad)} of {want.numel()} differ; first at {bad[0].tolist()}: "
                f"{got[tuple(bad[0])].item()!r} != {want[tuple(bad[0])].item()!r}")


def _to16(t, dt):
    """t (fp32, on the CPU) in the 16-bit type on the device, after asserting that the type holds every value"""
    t16 = t.to(dt)
    assert torch.equal(t16.float(), t), "the operand is not exact in the 16-bit type"
    return t16.to(DEV)


def _srcs(ffi, tensors, ups):
    arr = (ffi.ConvSrc * len(tensors))()
    for a, t, up in zip(arr, tensors, ups):
        a.data, a.affine, a.c, a.upsample = t.data_ptr(), None, t.shape[-1], up
    return arr


# ============================================================================================ the weight gradient
def _wgrad(ffi, case, entry, zp, twin, with_bias=True, scaled=True):
    """One call of the entry point on the case's operands -> (dweight, dbias or None) float64 on the CPU, after asserting the
    exported workspace size and that the sentinel tails behind workspace, dweight and dbias are untouched (dbias as a whole
    where it is not passed).  `scaled`: dy16 = dy 2^K with dy_scale = [2^K, 2^-K, .]; else dy16 = dy and dy_scale = NULL."""
    B, (ox, oy, oz), srcdef, cout, k = case
    cin = T.cin_of(case)
    srcs, dy, _, _ = T.expected(case, entry)
    dt = _dt(twin)
    st = ffi.stream_ptr(torch.device(DEV))
    n_ws = int(_fn(ffi, "sk_train_conv_wgrad_workspace_floats", twin)(B, ox, oy, oz, cout, cin, k))
    assert n_ws == T.workspace_floats(case), f"sk_train_conv_wgrad_workspace_floats {n_ws}, the mirror {T.workspace_floats(case)}"
    big_ws, ws = _tailed((n_ws,))
    big_w, dw = _tailed((cout, cin, k, k, k))
    big_b, db = _tailed((cout,))
    dbp = ffi.ptr(db) if with_bias else None
    if entry == "fp32":
        assert not twin and scaled
        dev = [_cl(t).to(DEV) for t in srcs]
        dyd = _cl(dy).to(DEV)
        rc = ffi.lib.sk_train_conv_wgrad(_srcs(ffi, dev, [up for _, up in srcdef]), len(dev), ffi.ptr(dyd), B, ox, oy, oz, cout, k,
                                         ffi.ptr(dw), dbp, ffi.ptr(ws), st)
    else:
        dy16 = _to16(_cl(dy) * (2.0 ** K if scaled else 1.0), dt)
        sc = _scale(K) if scaled else None
        if entry == "stem_f16":
            img = srcs[0][:, 0].contiguous().to(DEV)
            rc = _fn(ffi, "sk_train_stem_wgrad_f16", twin)(ffi.ptr(img), ffi.ptr(dy16), ffi.ptr(sc), B, ox, oy, oz, ffi.ptr(dw), dbp,
                                                           ffi.ptr(ws), st)
        else:
            dev = [_to16(_cl(t), dt) for t in srcs]
            zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV) if zp else None
            rc = _fn(ffi, "sk_train_conv_wgrad_f16", twin)(_srcs(ffi, dev, [up for _, up in srcdef]), len(dev), ffi.ptr(dy16),
                                                           ffi.ptr(sc), B, ox, oy, oz, cout, k, ffi.ptr(dw), dbp, ffi.ptr(ws),
                                                           ffi.ptr(zeros), st)
    ffi.check(rc)
    torch.cuda.synchronize()
    assert _tail_intact(big_ws), "the kernels wrote behind the workspace"
    assert _tail_intact(big_w), "the kernels wrote behind dweight"
    assert _tail_intact(big_b), "the kernels wrote behind dbias"
    if not with_bias:
        assert bool((db == SENT).all()), "dbias = NULL, and yet something wrote a bias gradient"
    return dw.cpu().double(), db.cpu().double() if with_bias else None


WGRAD_RUNS = [(c, e, zp, tw) for c, e, zp in T.runs() for tw in ([False] if e == "fp32" else TWINS)]


def _run_id(r):
    case, entry, zp, twin = r
    return f"{T.case_id(case)}-{entry}{'-zp' if zp else ''}{'-bf16' if twin else ''}"


@pytest.mark.parametrize("run", WGRAD_RUNS, ids=_run_id)
def test_weight_gradient_equals_float64(ffi, run):
    """Every case through every entry point that takes it (the f16 one with a zero page and with zero_page = NULL, each on its
    own route; the 16-bit ones in the fp16 build and in the bf16 twin): dweight and dbias, prefilled with the sentinel, equal
    the float64 gradients bit for bit -- with dy_scale = [2^K, 2^-K, .], K = 2, and the device dy = dy 2^K, so that a kernel or
    reduction that drops the scale is off by a factor 4 -- and dweight does so again with dbias = NULL.  The empty-chunk
    cases are in the table: their last partial rows must have been written as zeros for the sum to come out."""
    case, entry, zp, twin = run
    _, _, dw64, db64 = T.expected(case, entry)
    dw, db = _wgrad(ffi, case, entry, zp, twin)
    _same(dw, dw64, f"dweight [{T.route(case, entry, zp)}]")
    _same(db, db64, f"dbias [{T.route(case, entry, zp)}]")
    dw, _ = _wgrad(ffi, case, entry, zp, twin, with_bias=False)
    _same(dw, dw64, f"dweight with dbias = NULL [{T.route(case, entry, zp)}]")


def _first_per_route(entry):
    seen, out = set(), []
    for c, e, zp in T.runs():
        if e == entry and T.route(c, e, zp) not in seen:
            seen.add(T.route(c, e, zp))
            out.append((c, e, zp))
    return out


UNSCALED = [(c, e, zp, tw) for c, e, zp in _first_per_route("f16") for tw in TWINS]


@pytest.mark.parametrize("run", UNSCALED, ids=_run_id)
def test_weight_gradient_without_a_scale(ffi, run):
    """sk_train_conv_wgrad_f16 with dy_scale = NULL (the device dy is dy itself), one case per route of the entry point"""
    case, entry, zp, twin = run
    _, _, dw64, db64 = T.expected(case, entry)
    dw, db = _wgrad(ffi, case, entry, zp, twin, scaled=False)
    _same(dw, dw64, f"dweight [{T.route(case, entry, zp)}]")
    _same(db, db64, f"dbias [{T.route(case, entry, zp)}]")


TWICE = [(c, e, zp, tw) for en in T.ENTRIES for c, e, zp in _first_per_route(en) for tw in ([False] if e == "fp32" else TWINS)]


@pytest.mark.parametrize("run", TWICE, ids=_run_id)
def test_weight_gradient_is_deterministic(ffi, run):
    """each of the 14 routes twice on the same input: equal bits"""
    case, entry, zp, twin = run
    a = _wgrad(ffi, case, entry, zp, twin)
    b = _wgrad(ffi, case, entry, zp, twin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ============================================================================================ sk_train_pack_weight
def _pack(ffi, twin, w, transposed, c_lo, c_n):
    """sk_train_pack_weight of w (Co, Ci, k, k, k) fp32 -> the packed bytes (uint8, on the device), tail checked"""
    Co, Ci, k = w.shape[0], w.shape[1], w.shape[2]
    co_eff, ci_eff = (c_n, Co) if transposed else (Co, Ci)
    n = k ** 3 * (ci_eff // 16) * (co_eff // 32) * 1024
    big, buf = _tailed((n,), torch.uint8, 0x5A)
    wd = w.to(DEV).contiguous()
    ffi.check(_fn(ffi, "sk_train_pack_weight", twin)(ffi.ptr(wd), Co, Ci, k, transposed, c_lo, c_n, ffi.ptr(buf),
                                                     ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert _tail_intact(big, 0x5A), "sk_train_pack_weight wrote behind dst"
    return buf


def _conv(ffi, twin, x16, packed, cout, k):
    """sk_conv3d of one plain source x16 (B, ox, oy, oz, cin) with a packed operator and a zero bias -> (B, ox, oy, oz, cout)
    float64 on the CPU, the tail behind the output checked"""
    B, ox, oy, oz, _ = x16.shape
    big, out = _tailed((B, ox, oy, oz, cout), x16.dtype, 7.0)
    zero_bias = torch.zeros(128, device=DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ffi.check(_fn(ffi, "sk_conv3d", twin)(_srcs(ffi, [x16], [0]), 1, ffi.ptr(packed), ffi.ptr(zero_bias), ffi.ptr(out), B, ox, oy, oz,
                                          cout, k, None, ffi.ptr(zeros), ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert _tail_intact(big, 7.0), "sk_conv3d wrote behind out"
    return out.cpu().double(), out


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("shape", T.PACK_FORWARD, ids=lambda s: "x".join(map(str, s)))
def test_pack_weight_forward_equals_the_host_packer(ffi, shape, twin):
    """transposed = 0 on a weight the 16-bit type holds: the bytes of sk_conv3d_pack_weight_host (the bf16 twin against the
    twin's own host packer), for ksize 3 with cout 32 (the 16x16x32 fragment order), cout 64 and 128, ksize 2 and ksize 1"""
    Co, Ci, k = shape
    w = T.pack_forward_weight(Co, Ci, k).contiguous()
    host = _fn(ffi, "sk_conv3d_pack_weight_host", twin)
    fpt = w.numpy().ctypes.data_as(C.POINTER(C.c_float))
    n = host(fpt, Co, Ci, k, None)
    want = np.full(n, 0xA5, dtype=np.uint8)
    assert host(fpt, Co, Ci, k, want.ctypes.data_as(C.c_void_p)) == n
    got = _pack(ffi, twin, w, 0, 0, Ci).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("idx", range(len(T.DGRAD_CASES)))
def test_pack_weight_transposed_gives_the_data_gradient(ffi, idx, twin):
    """transposed = 1 for the whole input, each half of a two-source layer and ranges that do not start at 0: sk_conv3d of
    the integer dy with the packed operator and a zero bias equals the float64 conv_transpose3d, sliced to the range, bit for
    bit (ksize 3: taps flipped; ksize 1)"""
    B, osp, Co, Ci, k, ranges = T.DGRAD_CASES[idx]
    dy, w, dx64 = T.dgrad_expected(idx)
    dy16 = _to16(_cl(dy), _dt(twin))
    for lo, n in ranges:
        got, _ = _conv(ffi, twin, dy16, _pack(ffi, twin, w, 1, lo, n), n, k)
        _same(_cf(got), dx64[:, lo:lo + n], f"data gradient of channels [{lo}, {lo + n})")


def _np_interleave(t):
    """t (8, B, cx, cy, cz, C) -> (B, 2cx, 2cy, 2cz, C): fine voxel (2x + px, 2y + py, 2z + pz) takes parity p = 4 px + 2 py + pz"""
    _, B, cx, cy, cz, Cc = t.shape
    out = np.zeros((B, 2 * cx, 2 * cy, 2 * cz, Cc), dtype=np.float64)
    for p in range(8):
        out[:, (p >> 2) & 1::2, (p >> 1) & 1::2, p & 1::2] = t[p]
    return out


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("idx", range(len(T.DGRAD2_CASES)))
def test_pack_weight_parity_blocks_give_the_stride2_data_gradient(ffi, idx, twin):
    """transposed = 2 as the training step uses it: the eight fragment blocks, each run with sk_conv3d(ksize 1) on the scaled
    integer dy into t16[p], assembled by sk_train_interleave2 with the dy's scale.  Each parity tensor equals the float64
    conv_transpose3d (stride 2) at its fine voxels, and so does the assembled fp32 gradient."""
    B, (cx, cy, cz), Co, Ci = T.DGRAD2_CASES[idx]
    dy, w, dx64 = T.dgrad2_expected(idx)
    dt = _dt(twin)
    dy16 = _to16(_cl(dy) * 2.0 ** K, dt)
    packed = _pack(ffi, twin, w, 2, 0, Ci)
    per = packed.numel() // 8
    assert per == (Co // 16) * (Ci // 32) * 1024
    big_t, t16 = _tailed((8, B, cx, cy, cz, Ci), dt, 7.0)
    want = _cl(dx64)                                                # (B, 2cx, 2cy, 2cz, Ci)
    for p in range(8):
        got, dev = _conv(ffi, twin, dy16, packed[p * per:(p + 1) * per], Ci, 1)
        _same(got * 2.0 ** -K, want[:, (p >> 2) & 1::2, (p >> 1) & 1::2, p & 1::2], f"parity {p}")
        t16[p].copy_(dev)
    big_x, dx = _tailed((B, 2 * cx, 2 * cy, 2 * cz, Ci))
    sc = _scale(K)
    ffi.check(_fn(ffi, "sk_train_interleave2", twin)(ffi.ptr(t16), ffi.ptr(dx), B, cx, cy, cz, Ci, ffi.ptr(sc), 0,
                                                     ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert _tail_intact(big_x) and _tail_intact(big_t, 7.0)
    _same(dx.cpu().double(), want.contiguous(), "the assembled data gradient")


# ============================================================================================ the 16-bit gradient chain
CHAIN_SHAPE = (2, 3, 5, 3)     # B, coarse extents: odd on every axis


def _ints(gen, shape, lo, hi, step=1):
    return (torch.randint(lo, hi + 1, shape, generator=gen) * step).float()


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("Cc", [8, 32, 128])
def test_interleave2_equals_its_restatement(ffi, Cc, twin):
    """sk_train_interleave2 (accumulate 0, accumulate 1 onto a known fp32 tensor, scale = NULL) and sk_train_interleave2_add16
    against _np_interleave: dx[2c + p] (+)= t16[p][c] scale[1] (+ add16 add_scale[1])"""
    B, cx, cy, cz = CHAIN_SHAPE
    gen = torch.Generator().manual_seed(100 + Cc)
    dt, st = _dt(twin), ffi.stream_ptr(torch.device(DEV))
    t = _ints(gen, (8, B, cx, cy, cz, Cc), -100, 100)
    add = _ints(gen, (B, 2 * cx, 2 * cy, 2 * cz, Cc), -100, 100)
    base = _ints(gen, add.shape, -50, 50) / 8
    t16, add16 = _to16(t, dt), _to16(add, dt)
    kT, kA = 5, 3
    sT, sA = _scale(kT), _scale(kA)
    want = _np_interleave(t.double().numpy())
    f = _fn(ffi, "sk_train_interleave2", twin)

    def run(scale, accumulate, start):
        big, dx = _tailed(add.shape)
        if start is not None:
            dx.copy_(start.to(DEV))
        ffi.check(f(ffi.ptr(t16), ffi.ptr(dx), B, cx, cy, cz, Cc, ffi.ptr(scale), accumulate, st))
        torch.cuda.synchronize()
        assert _tail_intact(big)
        return dx.cpu().double().numpy()

    assert np.array_equal(run(sT, 0, None), want * 2.0 ** -kT)
    assert np.array_equal(run(sT, 1, base), base.double().numpy() + want * 2.0 ** -kT)
    assert np.array_equal(run(None, 0, None), want)
    assert np.array_equal(run(None, 1, base), base.double().numpy() + want)
    big, dx = _tailed(add.shape)
    ffi.check(_fn(ffi, "sk_train_interleave2_add16", twin)(ffi.ptr(t16), ffi.ptr(add16), ffi.ptr(sA), ffi.ptr(dx), B, cx, cy, cz, Cc,
                                                           ffi.ptr(sT), st))
    torch.cuda.synchronize()
    assert _tail_intact(big)
    assert np.array_equal(dx.cpu().double().numpy(), want * 2.0 ** -kT + add.double().numpy() * 2.0 ** -kA)


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("kT,kA", [(5, 3), (3, 5), (4, 4)])
@pytest.mark.parametrize("Cc", [8, 32, 128])
def test_interleave2_h_equals_its_restatement(ffi, Cc, kT, kA, twin):
    """sk_train_interleave2_h: with add16 the 16-bit result is (T / s_T + add / s_add) s with s = min(s_T, s_add) / 2, and
    out_scale[0:2] = [s, 1 / s]; without, the parity tensor passes through and s = s_T.  Payloads are multiples of 8, so both
    rescalings (by 1/2 and at most 1/8) stay integers the type holds."""
    B, cx, cy, cz = CHAIN_SHAPE
    gen = torch.Generator().manual_seed(200 + Cc + kT)
    dt, st = _dt(twin), ffi.stream_ptr(torch.device(DEV))
    t = _ints(gen, (8, B, cx, cy, cz, Cc), -12, 12, 8)
    add = _ints(gen, (B, 2 * cx, 2 * cy, 2 * cz, Cc), -12, 12, 8)
    t16, add16 = _to16(t, dt), _to16(add, dt)
    sT, sA = _scale(kT), _scale(kA)
    inter = _np_interleave(t.double().numpy())
    for with_add in (True, False):
        big, out = _tailed(add.shape, dt, 7.0)
        big_s, osc = _tailed((3,))
        ffi.check(_fn(ffi, "sk_train_interleave2_h", twin)(ffi.ptr(t16), ffi.ptr(add16) if with_add else None,
                                                           ffi.ptr(sA) if with_add else None, ffi.ptr(out), ffi.ptr(osc), B, cx, cy,
                                                           cz, Cc, ffi.ptr(sT), st))
        torch.cuda.synchronize()
        assert _tail_intact(big, 7.0) and _tail_intact(big_s)
        s = min(2.0 ** kT, 2.0 ** kA) / 2 if with_add else 2.0 ** kT
        o = osc.cpu().double().numpy()
        assert o[0] == s and o[1] == 1 / s
        true = inter * 2.0 ** -kT + (add.double().numpy() * 2.0 ** -kA if with_add else 0.0)
        got = out.cpu().double().numpy()
        assert np.abs(got).max() < 2.0 ** 15                        # as test_16bit_gradient_handoffs: inside the type's range
        assert np.array_equal(got, true * s)
        assert np.array_equal(got * o[1], true)


def _pool(a):
    """a (B, 2cx, 2cy, 2cz, C) -> the sums over the 2 x 2 x 2 blocks (B, cx, cy, cz, C)"""
    B, X, Y, Z, Cc = a.shape
    return a.reshape(B, X // 2, 2, Y // 2, 2, Z // 2, 2, Cc).sum(axis=(2, 4, 6))


@pytest.mark.parametrize("Cc", [8, 32, 128])
def test_sumpool2_f32_equals_its_restatement(ffi, Cc):
    """sk_train_sumpool2 (fp32 in and out; one build) against a numpy block sum of integers"""
    B, cx, cy, cz = CHAIN_SHAPE
    gen = torch.Generator().manual_seed(350 + Cc)
    fine = _ints(gen, (B, 2 * cx, 2 * cy, 2 * cz, Cc), -1000, 1000)
    big, coarse = _tailed((B, cx, cy, cz, Cc))
    fd = fine.to(DEV)
    ffi.check(ffi.lib.sk_train_sumpool2(ffi.ptr(fd), ffi.ptr(coarse), B, cx, cy, cz, Cc, ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert _tail_intact(big)
    assert np.array_equal(coarse.cpu().double().numpy(), _pool(fine.double().numpy()))


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("Cc", [8, 32, 128])
def test_sumpool2_16bit_equals_its_restatement(ffi, Cc, twin):
    """sk_train_sumpool2_f16 (coarse = scale[1] x the sum of the eight children) and sk_train_sumpool2_hh (16-bit result =
    sum / 8, out_scale[0:2] = [s / 8, 8 / s]) against a numpy block sum.  The payload is multiples of 8, so sum / 8 is an
    integer the type holds."""
    B, cx, cy, cz = CHAIN_SHAPE
    gen = torch.Generator().manual_seed(300 + Cc)
    dt, st = _dt(twin), ffi.stream_ptr(torch.device(DEV))
    fshape = (B, 2 * cx, 2 * cy, 2 * cz, Cc)
    pool = _pool
    fine = _ints(gen, fshape, -3, 3, 8)
    f16 = _to16(fine, dt)
    k = 6
    sc = _scale(k)
    big, coarse = _tailed((B, cx, cy, cz, Cc))
    ffi.check(_fn(ffi, "sk_train_sumpool2_f16", twin)(ffi.ptr(f16), ffi.ptr(sc), ffi.ptr(coarse), B, cx, cy, cz, Cc, st))
    torch.cuda.synchronize()
    assert _tail_intact(big)
    want = pool(fine.double().numpy())
    assert np.abs(want).max() > 0
    assert np.array_equal(coarse.cpu().double().numpy(), want * 2.0 ** -k)

    big, c16 = _tailed((B, cx, cy, cz, Cc), dt, 7.0)
    big_s, osc = _tailed((3,))
    ffi.check(_fn(ffi, "sk_train_sumpool2_hh", twin)(ffi.ptr(f16), ffi.ptr(sc), ffi.ptr(c16), ffi.ptr(osc), B, cx, cy, cz, Cc, st))
    torch.cuda.synchronize()
    assert _tail_intact(big, 7.0) and _tail_intact(big_s)
    o = osc.cpu().double().numpy()
    assert o[0] == 2.0 ** k / 8 and o[1] == 8 / 2.0 ** k
    got = c16.cpu().double().numpy()
    assert np.abs(got).max() < 2.0 ** 15
    assert np.array_equal(got, want / 8) and np.array_equal(got * o[1], want * 2.0 ** -k)


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("n", [8 * 777, 8 * 777 + 3, 5])
def test_cast_f16_f32_equals_its_restatement(ffi, n, twin):
    """sk_train_cast_f16_f32: y (+)= float(x) scale[1] (scale NULL: 1), on the eight-a-lane path (n % 8 == 0) and on the scalar
    one, writing and accumulating onto a known fp32 tensor"""
    gen = torch.Generator().manual_seed(400 + n)
    dt, st = _dt(twin), ffi.stream_ptr(torch.device(DEV))
    x = _ints(gen, (n,), -200, 200)
    base = _ints(gen, (n,), -50, 50) / 8
    x16 = _to16(x, dt)
    k = 4
    for scale, factor in ((_scale(k), 2.0 ** -k), (None, 1.0)):
        for accumulate in (0, 1):
            big, y = _tailed((n,))
            if accumulate:
                y.copy_(base.to(DEV))
            ffi.check(_fn(ffi, "sk_train_cast_f16_f32", twin)(ffi.ptr(x16), ffi.ptr(y), n, ffi.ptr(scale), accumulate, st))
            torch.cuda.synchronize()
            assert _tail_intact(big)
            want = x.double().numpy() * factor + (base.double().numpy() if accumulate else 0.0)
            assert np.array_equal(y.cpu().double().numpy(), want)
