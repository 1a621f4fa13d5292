"""GPU tests of the plain 16-bit slots conv3<64,4>, conv3<64,3> and conv3<128,2> of skoots_amd/csrc/conv3d.hip on the plane
geometries the forward runs them at, with a short x -- shapes the table of tests/conv16_cases.py does not hold: the
160-position level-1 planes (150 x 10: twelve linear patches, the last one ragged, x-chunks of 8 + 1 planes), the same with a
concatenated, upsampled second source, the level-2 plane (75 x 5, 128 channels) and the 4 x 32 rectangles with the five-plane
ring.  The slots run conv3_m16_kernel<COUT, XS> (v_mfma_f32_16x16x32_f16, A fragments gathered from the 32x32x16 weight image:
tests/test_conv3_wide16_weights_cpu.py) or conv3_kernel<COUT, XS>, whichever the dispatch table holds; the checks are the same.

In fp16 (sk_conv3d) and in the bf16 twin (sk_conv3d_bf16), operands and float64 references from tests/conv16_cases.py:

  * integer operands (activations in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]): every product and every partial sum
    is an exact integer in fp32 in ANY order, so `out` must be the float64 conv, rounded once to the 16-bit format, bit for
    bit (fp16 holds |y| <= 2048 exactly; bf16 rounds, to nearest even as torch does), and the GroupNorm totals -- sums and
    sums of squares of the values AS STORED -- must be exact: each test first shows on the reference that no 128-voxel
    column set of one x-chunk can pass 2^24, which bounds every workgroup's fp32 partial;
  * realistic operands (randn): a tile alone and as items 1 and 2 of a batch of 3 gives identical output bytes and identical
    partial rows -- the x-chunk cut, the chunk order and with them every summation order are functions of the tile alone.
"""
import functools

import pytest
import torch

from tests import conv16_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0
TAIL = 4096

CASES = [
    # (case, slot, what it exercises)
    ((2, (9, 150, 10), [(64, 0)], 64, 3), "conv3<64,4>"),            # 12 linear patches, ragged last (1500 = 11 * 128 + 92), x-chunks 8 + 1
    ((1, (6, 150, 10), [(64, 0), (64, 1)], 64, 3), "conv3<64,4>"),   # concat + upsampled source: four chunks, two sources
    ((2, (7, 75, 5), [(128, 0)], 128, 3), "conv3<128,2>"),           # level-2 plane: 375 voxels, three patches, x-chunks 4 + 3
    ((1, (5, 6, 72), [(64, 0)], 64, 3), "conv3<64,3>"),              # 4 x 32 rectangles, XS 3: y % 4, z % 32, x % 3 != 0
]
ONLY = [c for c, _ in CASES]
IDS = [K.case_id(c) for c in ONLY]
DTYPES = [torch.float16, torch.bfloat16]


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def _integer(idx):
    """(sources, weight, bias, float64 conv) of a case on the integer operands; computed once, not to be modified"""
    srcs, w, b = K.integer_operands(ONLY[idx])
    return srcs, w, b, K.conv64(ONLY[idx], srcs, w, b)


def _run(case, dt, srcs, w, b, B=None):
    """sk_conv3d (fp16) | sk_conv3d_bf16 on channels-first fp32 sources (values the 16-bit format holds) -> (out (B, x, y, z,
    cout) in dt, partial (B, rows, cout / 4, 2) fp32) on the CPU; the row count is the plan mirror's and the sentinel tails
    behind both buffers are intact"""
    from skoots_amd import _ffi as ffi, unet as U
    sfx = "_bf16" if dt == torch.bfloat16 else ""
    _, (ox, oy, oz), srcdef, cout, k = case
    B = srcs[0].shape[0] if B is None else B
    dev = [_cl(t).to(dt).to(DEV) for t in srcs]
    arr = (ffi.ConvSrc * len(dev))()
    for a, t, (c, up) in zip(arr, dev, srcdef):
        assert t.shape[-1] == c and t.shape[0] == B
        a.data, a.affine, a.c, a.upsample = t.data_ptr(), None, c, up
    wp = U._pack(getattr(ffi.lib, "sk_conv3d_pack_weight_host" + sfx), w, w.shape[:3], DEV)
    bd = b.float().to(DEV)
    zeros = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    rows = getattr(ffi.lib, "sk_conv3d_num_blocks" + sfx)(B, ox, oy, oz, cout, k)
    assert rows == K.num_blocks(case)
    n_out, n_par = B * ox * oy * oz * cout, B * rows * (cout // 4) * 2
    big_o = torch.full((n_out + TAIL,), SENT, dtype=dt, device=DEV)
    big_p = torch.full((n_par + TAIL,), SENT, dtype=torch.float32, device=DEV)
    out, partial = big_o[:n_out].view(B, ox, oy, oz, cout), big_p[:n_par].view(B, rows, cout // 4, 2)
    st = ffi.stream_ptr(torch.device(DEV))
    ffi.check(getattr(ffi.lib, "sk_conv3d" + sfx)(arr, len(dev), ffi.ptr(wp), ffi.ptr(bd), ffi.ptr(out), B, ox, oy, oz, cout, k,
                                                   ffi.ptr(partial), ffi.ptr(zeros), st))
    torch.cuda.synchronize()
    assert bool((big_o[-TAIL:] == SENT).all()), "the kernel wrote behind out"
    assert bool((big_p[-TAIL:] == SENT).all()), "the kernel wrote behind gn_partial"
    return out.cpu(), partial.cpu()


def _same(got, want, what):
    if torch.equal(got, want):
        return
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    pytest.fail(f"{len(bad)} of {want.numel()} {what} differ; first at {bad[0].tolist()}: "
                f"{got[tuple(bad[0])].item()!r} != {want[tuple(bad[0])].item()!r}")


def _workgroup_bound(case, stored):
    """The largest sum of squares (hence of absolute values: integers) a workgroup's fp32 partial of one quad can reach.  A
    workgroup owns one x-chunk of the plan and, of the plane, 128 voxels: on the linear plans (z <= 40) a run of 128 consecutive
    in-plane indices -> the largest sum over any such window, whatever its alignment; on the rectangle plans at most 128
    voxels -> the 128 largest per-column sums."""
    B, (ox, oy, oz), _, cout, _ = case
    plan = K.make_plan(ox, oy, oz, cout)
    XC = plan["XC"]
    sq = (stored.double() ** 2).reshape(B, cout // 4, 4, ox, oy * oz).sum(dim=2)          # (B, quad, x, voxel)
    worst = 0.0
    for x0 in range(0, ox, XC):
        col = sq[:, :, x0:x0 + XC].sum(dim=2)
        if plan["mode"] == 0:
            cs = torch.nn.functional.pad(col.cumsum(dim=-1), (1, 0))
            n = min(128, col.shape[-1])
            worst = max(worst, (cs[..., n:] - cs[..., :-n]).max().item())
        else:
            worst = max(worst, col.topk(min(128, col.shape[-1]), dim=-1).values.sum(dim=-1).max().item())
    return worst


@pytest.mark.parametrize("case,slot", CASES, ids=IDS)
def test_wide_cases_route_and_plan(case, slot):
    """Every case reaches the slot written next to it, in both builds, with the plan numbers of the mirror (the geometry the
    case was chosen for: 160 positions and twelve patches on the level-1 plane, the five-plane ring on the rectangles)."""
    _, (ox, oy, oz), _, cout, _ = case
    want = K.make_plan(ox, oy, oz, cout)
    for twin in (False, True):
        r = K.library_route(case, "fp16", twin=twin)
        assert r.name.decode() == slot
        assert (r.mode, r.tz, r.nposp, r.npatch, r.xs, r.plan_lds, r.xc, r.nxc) == tuple(
            want[k] for k in ("mode", "TZ", "nposp", "npatch", "xs", "lds", "XC", "nxc"))
        assert r.num_blocks == K.num_blocks(case)
    if case == ONLY[0]:
        assert (want["nposp"], want["npatch"], want["XC"], want["nxc"]) == (160, 12, 8, 2)
    if case == ONLY[3]:
        assert (want["mode"], want["TZ"], want["xs"]) == (1, 32, 3)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ONLY, ids=IDS)
def test_wide_exact_on_integer_operands(case, dt):
    """`out` equals the float64 conv rounded once to the 16-bit format, bit for bit; no row of gn_partial is left unwritten and
    the rows summed in float64 equal the float64 sums and sums of squares of the stored values exactly."""
    srcs, w, b, y = _integer(ONLY.index(case))
    stored = y.float().to(dt)                                  # integers below 2^24: exact in fp32, then ONE rounding
    if dt == torch.float16:
        assert torch.equal(stored.double(), y)                 # |y| <= 2048: the fp16 store is exact
    bound = _workgroup_bound(case, stored)
    assert bound < 2 ** 24, f"a workgroup's sum of squares may reach {bound}: the totals would not be exact in fp32"
    out, partial = _run(case, dt, srcs, w, b)
    _same(_cf(out).double(), stored.double(), "outputs (b, c, x, y, z)")
    assert not bool((partial == SENT).all(dim=(2, 3)).any()), "a row of gn_partial was left unwritten"
    _same(partial.double().sum(dim=1), K.gn_totals(stored), "totals (b, quad, sum | sumsq)")


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ONLY, ids=IDS)
def test_wide_tile_alone_and_in_a_batch_of_three(case, dt):
    """Realistic operands: sample 0 of the case alone, and as items 1 and 2 of a batch of 3 whose item 0 is another tile: the same
    output bytes and the same partial rows, and item 0 of the batch is not the tile's result (the comparison is no empty one)."""
    srcs, w, b = K.realistic_operands(case, "fp16")
    hold = lambda t: t.to(dt).float()
    tile = [hold(t[:1]) for t in srcs]
    g = torch.Generator().manual_seed(5)
    other = [hold(torch.randn(t.shape, generator=g)) for t in tile]
    one = (1,) + tuple(case[1:])
    alone_o, alone_p = _run(one, dt, tile, w, b)
    batch_o, batch_p = _run(one, dt, [torch.cat([o, t, t], dim=0) for o, t in zip(other, tile)], w, b)
    bits = torch.int16
    for item in (1, 2):
        _same(batch_o[item].view(bits), alone_o[0].view(bits), f"output halves of item {item}")
        _same(batch_p[item].view(torch.int32), alone_p[0].view(torch.int32), f"partial floats of item {item}")
    assert not torch.equal(batch_o[0].view(bits), alone_o[0].view(bits))
