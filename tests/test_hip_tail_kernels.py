"""The three streaming kernels behind the 3x3x3 convs, through the C ABI: the LDS-staged 1x1x1 conv of sk_conv3d
(pointwise_lds_kernel: 64 -> 32 and 128 -> 64 channels), sk_heads with carried box coordinates, and the mask-word form
of sk_gate_dilate_scatter (tile depth <= 32).

Bounds.  1x1x1 conv: the bound of tests/test_hip_unet.py::test_conv_vs_torch (fp16 operands, fp32 accumulation, fp16
store: 2e-3 of max(1, |want|); partial sums rtol 1e-3 + 2e-2 sqrt(voxels), sums of squares rtol 2e-3), against a
float64 reference.  Heads: the bound of tests/test_hip_stem_heads.py::test_heads_vs_float64, whose helpers are used.
Scatter: integer / byte work, bit for bit against a NumPy restatement.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_stem_heads import SENT, U as EPS32, _act_check, _heads_weights, _run_heads, _silu_err, _split_err, _ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _st(ffi):
    return ffi.stream_ptr(torch.device(DEV))


# ============================================================================================ 1x1x1 conv
def _conv1(ffi, x, wp, bias, cout, affine=None):
    """sk_conv3d, ksize 1, on x (B, X, Y, Z, cin) fp16 -> (out (B, X, Y, Z, cout), partial (B, nblk, cout / 4, 2))."""
    B, X, Y, Z, cin = x.shape
    out = torch.full((B, X, Y, Z, cout), SENT, dtype=torch.float16, device=DEV)
    nblk = ffi.lib.sk_conv3d_num_blocks(B, X, Y, Z, cout, 1)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=DEV)
    arr = (ffi.ConvSrc * 1)()
    arr[0].data, arr[0].c, arr[0].upsample = x.data_ptr(), cin, 0
    arr[0].affine = None if affine is None else affine.data_ptr()
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ffi.check(ffi.lib.sk_conv3d(arr, 1, ffi.ptr(wp), ffi.ptr(bias), ffi.ptr(out), B, X, Y, Z, cout, 1, ffi.ptr(partial),
                                ffi.ptr(zeros), _st(ffi)))
    torch.cuda.synchronize()
    return out, partial


def _conv1_ref(z, w, b):
    """float64: z (B, n, cin) activated input as the kernel sees it, w (cout, cin) fp32 (used as fp16), b (cout)."""
    return z.double() @ w.half().double().t() + b.double()


def _check_conv1(out, partial, want):
    """out (B, X, Y, Z, cout), partial against want (B, n, cout) float64 at test_conv_vs_torch's bound."""
    B, n, cout = want.shape
    err = (out.reshape(B, n, cout).cpu().double() - want).abs().max().item()
    assert err <= 2e-3 * max(1.0, want.abs().max().item()), err
    p = partial.sum(dim=1).cpu().double()                      # (B, cout / 4, 2)
    wq = want.reshape(B, n, cout // 4, 4)
    assert torch.allclose(p[..., 0], wq.sum(dim=(1, 3)), rtol=1e-3, atol=2e-2 * n ** 0.5)
    assert torch.allclose(p[..., 1], (wq ** 2).sum(dim=(1, 3)), rtol=2e-3)


def _affine(B, cin, g):
    return torch.stack([torch.rand((B, cin), generator=g) + 0.5, torch.randn((B, cin), generator=g) * 0.3], dim=1).contiguous()


POINTWISE = [(64, 32), (128, 64)]
EXTENTS = [(6, 5, 4),     # 120 voxels: one ragged block
           (8, 8, 5),     # 320 voxels: one full block and one ragged block
           (16, 16, 2)]   # 512 voxels: exactly two blocks


@pytest.mark.parametrize("osp", EXTENTS)
@pytest.mark.parametrize("cin,cout", POINTWISE)
def test_pointwise_vs_float64(ffi, cin, cout, osp):
    """Activated and raw input, B = 2 with a different affine per sample, against float64; the raw form equals, BIT FOR
    BIT, sk_groupnorm_silu followed by the activated form (output and partial rows); B = 2 equals two B = 1 calls."""
    from skoots_amd import unet
    g = torch.Generator().manual_seed(cin + 3 * osp[0] + osp[2])
    B, n = 2, osp[0] * osp[1] * osp[2]
    x = torch.randn((B,) + osp + (cin,), generator=g).half()
    w = torch.randn((cout, cin), generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    aff = _affine(B, cin, g)
    aff[1, 0] *= 2.0
    wp = unet.pack_conv_weight(w.reshape(cout, cin, 1, 1, 1), DEV)
    xd, bd, affd = x.to(DEV), b.to(DEV), aff.to(DEV)

    out, partial = _conv1(ffi, xd, wp, bd, cout)
    _check_conv1(out, partial, _conv1_ref(x.reshape(B, n, cin), w, b))

    fused, pf = _conv1(ffi, xd, wp, bd, cout, affine=affd)
    t = aff[:, 0:1].double() * x.reshape(B, n, cin).double() + aff[:, 1:2].double()
    _check_conv1(fused, pf, _conv1_ref(F.silu(t).half(), w, b))
    act = xd.clone()
    ffi.check(ffi.lib.sk_groupnorm_silu(ffi.ptr(act), ffi.ptr(affd), B, n, cin, _st(ffi)))
    plain, pp = _conv1(ffi, act, wp, bd, cout)
    assert torch.equal(fused, plain) and torch.equal(pf, pp)

    for k in range(B):
        o1, p1 = _conv1(ffi, xd[k:k + 1].contiguous(), wp, bd, cout, affine=affd[k:k + 1].contiguous())
        assert torch.equal(o1[0], fused[k]) and torch.equal(p1[0], pf[k])
        o1, p1 = _conv1(ffi, xd[k:k + 1].contiguous(), wp, bd, cout)
        assert torch.equal(o1[0], out[k]) and torch.equal(p1[0], partial[k])


@pytest.mark.parametrize("osp", EXTENTS)
@pytest.mark.parametrize("cin,cout", POINTWISE)
def test_pointwise_exact_on_small_integers(ffi, cin, cout, osp):
    """|x| <= 8, weights in {-2 .. 2}, integer bias, activated input: every product and every partial sum is an integer
    below 2^24, so fp32 accumulation is exact in any order.  The output is the fp16 rounding of the exact integer and every
    partial row (block blk = voxels [256 blk, 256 blk + 256)) is the exact sum / sum of squares of its voxels."""
    from skoots_amd import unet
    g = torch.Generator().manual_seed(cin * 5 + osp[1])
    B, n = 2, osp[0] * osp[1] * osp[2]
    x = torch.randint(-8, 9, (B,) + osp + (cin,), generator=g)
    w = torch.randint(-2, 3, (cout, cin), generator=g)
    b = torch.randint(-3, 4, (cout,), generator=g)
    want = x.reshape(B, n, cin) @ w.t() + b                                  # int64, exact
    nblk = (n + 255) // 256
    padded = torch.zeros((B, nblk * 256, cout), dtype=torch.int64)
    padded[:, :n] = want
    rows = padded.reshape(B, nblk, 256, cout // 4, 4)
    want_sum, want_sq = rows.sum(dim=(2, 4)), (rows ** 2).sum(dim=(2, 4))
    assert int(want_sq.max()) < 2 ** 24 and int(want.abs().max()) < 2 ** 24      # the premise of exactness
    wp = unet.pack_conv_weight(w.float().reshape(cout, cin, 1, 1, 1), DEV)
    out, partial = _conv1(ffi, x.half().to(DEV), wp, b.float().to(DEV), cout)
    assert torch.equal(out.reshape(B, n, cout).cpu(), want.double().half())
    assert torch.equal(partial[..., 0].cpu().double(), want_sum.double())
    assert torch.equal(partial[..., 1].cpu().double(), want_sq.double())


def test_pointwise_other_widths_stay_on_the_gather_kernel(ffi):
    """Cin 32 is outside the LDS-staged kernel's shapes: gather_gemm_kernel still serves it."""
    from skoots_amd import unet
    g = torch.Generator().manual_seed(5)
    B, osp, cin, cout = 2, (8, 8, 5), 32, 32
    n = osp[0] * osp[1] * osp[2]
    x = torch.randn((B,) + osp + (cin,), generator=g).half()
    w = torch.randn((cout, cin), generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    out, partial = _conv1(ffi, x.to(DEV), unet.pack_conv_weight(w.reshape(cout, cin, 1, 1, 1), DEV), b.to(DEV), cout)
    _check_conv1(out, partial, _conv1_ref(x.reshape(B, n, cin), w, b))


# ============================================================================================ heads
HEAD_TILE = (7, 6, 8)
HEAD_BOXES = [((0, 0, 0), (7, 6, 8)),      # the whole tile
              ((1, 2, 1), (6, 5, 7)),      # bz = 6: z-runs cross the 32-voxel tiles; 90 voxels, not a multiple of 32
              ((3, 4, 5), (4, 5, 6))]      # one voxel


@pytest.mark.parametrize("box", HEAD_BOXES)
@pytest.mark.parametrize("with_affine", [False, True])
def test_heads_box_vs_float64(ffi, box, with_affine):
    """Inside the box: test_heads_vs_float64's reference and bound.  Outside: the sentinel written before the call.
    B = 2 equals two B = 1 calls bit for bit."""
    g = torch.Generator().manual_seed(11 + with_affine + sum(box[1]))
    B, n = 2, HEAD_TILE[0] * HEAD_TILE[1] * HEAD_TILE[2]
    W, b = _heads_weights(4)
    x = (torch.randn((B, n, 32), generator=g) * 1.5).half()
    aff = None
    if with_affine:
        aff = torch.stack([torch.rand((B, 32), generator=g) + 0.5, torch.randn((B, 32), generator=g) * 0.5], dim=1)
        aff[1, 0] *= 3.0
        t = aff[:, 0:1].double() * x.double() + aff[:, 1:2].double()
        z64 = F.silu(t)
        zr = z64.half().double()
        dz = _ulp16(z64.abs() + _silu_err(t, EPS32 * t.abs())) + _silu_err(t, EPS32 * t.abs())
    else:
        zr, dz = x.double(), torch.zeros((B, n, 32), dtype=torch.float64)
    xd, affd = x.to(DEV), None if aff is None else aff.to(DEV)
    out = _run_heads(ffi, xd, affd, W, b, HEAD_TILE, box=box)
    dW, _ = _split_err(W)
    W64 = W.double()
    L = zr @ W64.t() + b.double()
    S = zr.abs() @ W64.abs().t() + dz @ W64.abs().t() + b.double().abs()
    e_L = dz @ W64.abs().t() + zr.abs() @ dW.t() + 65 * EPS32 * S
    (x0, y0, z0), (x1, y1, z1) = box
    inside = torch.zeros(HEAD_TILE, dtype=torch.bool)
    inside[x0:x1, y0:y1, z0:z1] = True
    sel = inside.reshape(-1)
    o = out.cpu().reshape(B, 5, n)
    _act_check(o[:, :, sel].contiguous(), L[:, sel].contiguous(), e_L[:, sel].contiguous(), f"heads box {box} affine={with_affine}")
    assert bool((o[:, :, ~sel] == SENT).all())
    for k in range(B):
        o1 = _run_heads(ffi, xd[k:k + 1].contiguous(), None if affd is None else affd[k:k + 1].contiguous(), W, b, HEAD_TILE, box=box)
        assert torch.equal(o1[0], out[k])


# ============================================================================================ gate, dilate, scatter
PROB_THR, SKEL_THR = 0.75, 0.5        # both exact in fp16, so "exactly at the threshold" exists in either dtype
VEC_SENT, SKEL_SENT = 0x7BCD, 0xEE    # fill of the volumes before the call


def _around(thr, dtype):
    t = np.array(thr, dtype=dtype)
    return [np.nextafter(t, dtype(0)), t, np.nextafter(t, dtype(2))]


def _make_out5(rng, tile, dtype):
    """(5, w, h, d): vectors with negative values and -0.0; skeleton and probability drawn from values exactly at, just below
    and just above their thresholds plus clear misses and hits (about 0.6 % of the voxels pass both)."""
    w, h, d = tile
    out = np.empty((5, w, h, d), dtype=dtype)
    v = rng.standard_normal((3, w, h, d)).astype(dtype)
    v[rng.random((3, w, h, d)) < 0.1] = dtype(-0.0)
    v[rng.random((3, w, h, d)) < 0.05] = dtype(0.0)
    out[:3] = v
    out[3] = rng.choice(np.array(_around(SKEL_THR, dtype) + [dtype(0.05), dtype(0.9)]), size=(w, h, d), p=[0.1, 0.1, 0.005, 0.79, 0.005])
    out[4] = rng.choice(np.array(_around(PROB_THR, dtype) + [dtype(0.1), dtype(0.95)]), size=(w, h, d), p=[0.1, 0.1, 0.1, 0.2, 0.5])
    return out


def _restate(out5):
    """The kernel's result on a whole tile: (skeleton (w, h, d) uint8, vectors (3, w, h, d) fp16)."""
    _, w, h, d = out5.shape
    f = out5.astype(np.float32)
    gate = f[4] > np.float32(PROB_THR)
    m = gate & (f[3] > np.float32(SKEL_THR))
    pad = np.zeros((w + 6, h + 6, d + 2), dtype=bool)          # zero padding at the tile faces
    pad[3:-3, 3:-3, 1:-1] = m
    dil = np.zeros((w, h, d), dtype=bool)
    for dx in range(7):                                        # box OR of radius (3, 3, 1)
        for dy in range(7):
            for dz in range(3):
                dil |= pad[dx:dx + w, dy:dy + h, dz:dz + d]
    vec = np.where(gate[None], f[:3], np.copysign(np.float32(0.0), f[:3])).astype(np.float16)
    return dil.astype(np.uint8), vec


def _scatter(ffi, out5, origins, los, his, vol, planar=True):
    """sk_gate_dilate_scatter on out5 (n, 5, w, h, d) into fresh sentinel-filled volumes -> (vec4, vec_planar | None, skeleton)."""
    n, _, w, h, d = out5.shape
    X, Y, Z = vol
    vec4 = torch.full((X, Y, Z, 4), VEC_SENT, dtype=torch.int16, device=DEV)
    vecp = torch.full((3, X, Y, Z), VEC_SENT, dtype=torch.int16, device=DEV) if planar else None
    skel = torch.full((X, Y, Z), SKEL_SENT, dtype=torch.uint8, device=DEV)
    offs = (C.c_int64 * n)(*[k * out5.stride(0) for k in range(n)])
    flat = lambda rows: (C.c_int32 * (3 * n))(*[int(v) for r in rows for v in r])
    ffi.check(ffi.lib.sk_gate_dilate_scatter(ffi.ptr(out5), ffi.dtype_code(out5), n, offs, out5.stride(1), out5.stride(2), out5.stride(3),
                                             w, h, d, flat(origins), flat(los), flat(his), ffi.ptr(vec4), ffi.ptr(vecp), ffi.ptr(skel),
                                             X, Y, Z, PROB_THR, SKEL_THR, _st(ffi)))
    torch.cuda.synchronize()
    return vec4.cpu().numpy().view(np.uint16), None if vecp is None else vecp.cpu().numpy().view(np.uint16), skel.cpu().numpy()


def _expected(tiles, origins, los, his, vol):
    X, Y, Z = vol
    vec4 = np.full((X, Y, Z, 4), VEC_SENT, dtype=np.uint16)
    vecp = np.full((3, X, Y, Z), VEC_SENT, dtype=np.uint16)
    skel = np.full((X, Y, Z), SKEL_SENT, dtype=np.uint8)
    for t, org, lo, hi in zip(tiles, origins, los, his):
        s, v = _restate(t)
        src = tuple(slice(a, b) for a, b in zip(lo, hi))
        dst = tuple(slice(o + a, o + b) for o, a, b in zip(org, lo, hi))
        skel[dst] = s[src]
        bits = v.view(np.uint16)[(slice(None),) + src]
        vecp[(slice(None),) + dst] = bits
        vec4[dst + (slice(0, 3),)] = np.moveaxis(bits, 0, -1)
        vec4[dst + (3,)] = 0
    return vec4, vecp, skel


SCATTER_CASES = [
    # tile, two origins, two write boxes [lo, hi): one touches every face of its tile, one touches none it can avoid;
    # oz + lz is odd for the first tile and even for the second, so both alignments of the 16-byte vector stores occur
    ((12, 11, 2), [(1, 2, 1), (14, 3, 1)], [(0, 0, 0), (3, 3, 1)], [(12, 11, 2), (9, 8, 2)]),
    ((12, 11, 20), [(1, 2, 1), (14, 3, 1)], [(0, 0, 0), (3, 3, 5)], [(12, 11, 20), (9, 8, 15)]),
    ((12, 11, 32), [(1, 2, 1), (14, 3, 1)], [(0, 0, 0), (4, 3, 3)], [(12, 11, 32), (12, 7, 30)]),
    # several 16 x 16 patches per tile, a ragged last patch, an odd volume depth (column bases of either parity)
    ((37, 35, 20), [(0, 1, 0), (38, 0, 2)], [(0, 0, 0), (2, 1, 5)], [(37, 35, 20), (36, 34, 16)]),
]


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("tile,origins,los,his", SCATTER_CASES)
def test_scatter_equals_numpy_restatement(ffi, tile, origins, los, his, dtype):
    """vec4, vec_planar and skeleton equal, bit for bit, threshold + zero-padded box OR of radius (3, 3, 1) + interior write;
    every byte outside the two write boxes keeps its sentinel (the expected volumes start as sentinels).  Without
    vec_planar the other two volumes are the same."""
    w, h, d = tile
    rng = np.random.default_rng(w * 100 + d + (dtype == np.float32))
    tiles = [_make_out5(rng, tile, dtype) for _ in origins]
    vol = (max(o[0] for o in origins) + w + 1, max(o[1] for o in origins) + h + 2, d + 2 + (w > 16))
    out5 = torch.from_numpy(np.stack(tiles)).to(DEV)
    want4, wantp, wants = _expected(tiles, origins, los, his, vol)
    got4, gotp, gots = _scatter(ffi, out5, origins, los, his, vol)
    assert np.array_equal(gots, wants)
    assert np.array_equal(got4, want4)
    assert np.array_equal(gotp, wantp)
    got4, _, gots = _scatter(ffi, out5, origins, los, his, vol, planar=False)
    assert np.array_equal(gots, wants) and np.array_equal(got4, want4)
