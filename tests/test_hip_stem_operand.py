"""GPU tests of the stem kernels' patch operand and tile addressing (stem_kernel in skoots_amd/csrc/unet_misc.hip): the
operand is assembled from aligned two-dword LDS reads with a per-lane byte permute that depends on the parity of z and on
the lane half, and a wave carries (row, z) and its LDS address from tile to tile instead of dividing.  What can go wrong
there shows at tile shapes the other stem tests do not run: rows shorter than a 32-voxel MFMA tile (several row wraps
inside one tile), odd tile counts (the statistics pass pairs tiles), voxel counts that are no multiple of 32 or 64, and
the y-chunk threshold at 150 rows.

Operands are small integers (mean 0, std 1), so every product and every sum is exact in fp32: the raw conv and the
statistics partials are compared with torch.equal against F.conv3d in float64.  The apply modes run the same integers
through the identity affine, where silu is the only inexact step, and are held to the per-voxel bounds that
tests/test_hip_stem_heads.py derives (test_stem_apply_modes_vs_float64).  The delta test moves a single unit weight through
all 27 taps: the output is then the framed input shifted by that tap, bit for bit, for both parities of z.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_stem_heads import (DEV, SENT, _check_stem_sample, _block_sums, _norm_rule, _patches, _ptr, _st, _stem_apply,
                                       _stem_rows, _stem_stats, _tap_major)

pytestmark = pytest.mark.gpu

TILES = [
    (3, 5, 2),       # a 32-voxel tile spans 16 rows: the row wrap happens inside every tile; 1 tile per plane, odd count
    (2, 7, 6),       # 42 voxels per workgroup: two tiles, the second ragged
    (2, 9, 20),      # the production depth; 180 voxels: no multiple of 32 or 64
    (2, 3, 22),      # Zt % 4 == 2, 66 voxels: three tiles (the paired statistics loop has a lone tail)
    (1, 150, 20),    # exactly one y chunk of 150 rows
    (1, 151, 20),    # one row into the second chunk (76 + 75)
]
CASES = [(tile, B) for tile in TILES for B in (1, 3)]


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _origins(vol_shape, tile, B):
    """B distinct origins; the last overhangs the volume's far faces by 1, 2 and 3 voxels (x, y, z) where the tile allows."""
    X, Y, Z = vol_shape
    Xt, Yt, Zt = tile
    far = (min(X - 1, X - Xt + 1), min(Y - 1, Y - Yt + 2), min(Z - 1, Z - Zt + 3))
    out = [(0, 0, 0), (X - Xt, 1, 2)][:B - 1] + [far]
    assert len(set(out)) == B
    return out


_CACHE = {}


def _case(ffi, tile, B):
    """Everything one (tile, B) case needs, computed once: the kernels' outputs and the float64 reference."""
    key = (tile, B)
    if key in _CACHE:
        return _CACHE[key]
    Xt, Yt, Zt = tile
    g = torch.Generator().manual_seed(1000 * Yt + 10 * Zt + B)
    vol_shape = (Xt + 5, Yt + 4, Zt + 3)
    vol = torch.randint(-1, 2, vol_shape, generator=g).to(torch.float16)
    origins = _origins(vol_shape, tile, B)
    w = torch.randint(-1, 2, (32, 1, 3, 3, 3), generator=g).float()
    bias = torch.randint(-2, 3, (32,), generator=g).float()
    wt, bd = _tap_major(w).to(DEV), bias.to(DEV)
    vol_d = vol.to(DEV)
    ws, p0 = _stem_stats(ffi, vol_d, origins, tile, 0.0, 1.0, wt, bd)
    ws2, p2, raw = _stem_stats(ffi, vol_d, origins, tile, 0.0, 1.0, wt, bd, raw=True)
    framed16 = torch.stack([torch.from_numpy(_norm_rule(vol.numpy(), o, tile, 0.0, 1.0)) for o in origins])
    n = B * (Xt + 2) * (Yt + 2) * (Zt + 2)
    assert torch.equal(ws.cpu()[:n].reshape(framed16.shape), framed16) and torch.equal(ws2, ws)
    want = F.conv3d(framed16.double()[:, None], w.double(), bias.double()).permute(0, 2, 3, 4, 1)   # exact integers
    aff = torch.zeros((B, 2, 32))
    aff[:, 0] = 1.0                                                                                   # identity affine
    outs = {m: _stem_apply(ffi, m, ws, tile, B, wt, bd, aff.to(DEV)).cpu() for m in (1, 3, 4)}
    outs[2], outs["p0"], outs["p2"] = raw.cpu(), p0.cpu(), p2.cpu()
    _CACHE[key] = dict(origins=origins, w=w, bias=bias, wt=wt, bd=bd, framed16=framed16, want=want, aff=aff, outs=outs,
                       rows=_stem_rows(Yt, Zt))
    return _CACHE[key]


@pytest.mark.parametrize("tile,B", CASES)
def test_stem_operand_raw_exact(ffi, tile, B):
    """sk_conv3d_stem_raw (MODE 2) on integer operands equals F.conv3d in float64 exactly, every voxel of every tile."""
    c = _case(ffi, tile, B)
    assert torch.equal(c["outs"][2].double(), c["want"])


@pytest.mark.parametrize("tile,B", CASES)
def test_stem_operand_partials_exact(ffi, tile, B):
    """The statistics partials (B, nblk, 8, 2) of sk_conv3d_stem (MODE 0, two tiles per iteration) and of sk_conv3d_stem_raw
    (MODE 2) are the same bits, and equal the float64 sums and sums of squares per (workgroup, channel quad): integers
    below 2^24 (at most 3000 voxels x 4 channels x 29^2 per partial), so exact whatever the order."""
    c = _case(ffi, tile, B)
    p0, p2 = c["outs"]["p0"], c["outs"]["p2"]
    assert torch.equal(p0, p2)
    for b in range(B):
        ps = torch.stack([_block_sums(c["want"][b], c["rows"]), _block_sums(c["want"][b] ** 2, c["rows"])], dim=-1)
        assert float(ps.abs().max()) < 2.0 ** 24
        assert torch.equal(p0[b].double(), ps), f"tile {b}: partials"


@pytest.mark.parametrize("tile,B", CASES)
def test_stem_operand_apply_modes(ffi, tile, B):
    """sk_conv3d_stem_apply / _split / _mix8 (MODE 1, 3, 4) with the identity affine on the same integers: the conv result
    is exact, so silu and the store rounding are the only inexact steps; every voxel within the bounds of
    test_stem_apply_modes_vs_float64 (which also re-checks MODE 2 and both partial sets against them)."""
    c = _case(ffi, tile, B)
    for b in range(B):
        _check_stem_sample(b, c["framed16"][b], c["w"], c["bias"], c["aff"][b], c["outs"], c["rows"], f"{B}x{tile}")


@pytest.mark.parametrize("tile,B", CASES)
def test_stem_operand_train_fwd_exact(ffi, tile, B):
    """sk_train_stem_fwd_f16 and its bf16 twin (MODE 2 on the framed copy of an fp32 image) on the same integers: the raw
    tensor equals F.conv3d exactly and the partials are sk_conv3d_stem_raw's bits."""
    c = _case(ffi, tile, B)
    Xt, Yt, Zt = tile
    imgd = c["framed16"][:, 1:-1, 1:-1, 1:-1].float().contiguous().to(DEV)
    for sfx, dt in (("", torch.float16), ("_bf16", torch.bfloat16)):
        nblk = getattr(ffi.lib, "sk_conv3d_stem_num_blocks" + sfx)(Xt, Yt, Zt)
        ws_bytes = getattr(ffi.lib, "sk_conv3d_stem_workspace_bytes" + sfx)(B, Xt, Yt, Zt)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        y16 = torch.full((B, Xt, Yt, Zt, 32), SENT, dtype=dt, device=DEV)
        pt = torch.full((B, nblk, 8, 2), SENT, device=DEV)
        ffi.check(getattr(ffi.lib, "sk_train_stem_fwd_f16" + sfx)(_ptr(imgd), B, Xt, Yt, Zt, _ptr(c["wt"]), _ptr(c["bd"]),
                                                                   _ptr(y16), _ptr(pt), _ptr(ws), ws_bytes, _st()))
        torch.cuda.synchronize()
        assert torch.equal(y16.cpu().double(), c["want"]), sfx
        assert torch.equal(pt.cpu(), c["outs"]["p2"]), sfx


def test_stem_operand_delta_every_tap():
    """One tap = 1 (in all 32 channels), the other 26 = 0, bias 0, for each of the 27 taps at tile (2, 5, 6): the raw output
    of every channel is the framed normalised input shifted by that tap, bit for bit (products with 1.0 and 0.0, fp16 in
    and out).  A permute that picks the wrong half for one parity of z, or a read of the wrong (dx, dy) row in one lane
    half, moves exactly one tap's data.  The statistics of the two passes agree bit for bit as well."""
    from skoots_amd import _ffi as ffi
    tile, (Xt, Yt, Zt) = (2, 5, 6), (2, 5, 6)
    g = torch.Generator().manual_seed(256)
    vol_shape = (Xt + 5, Yt + 4, Zt + 3)
    vol = torch.randint(0, 256, vol_shape, generator=g).to(torch.float16)
    origins = _origins(vol_shape, tile, 2)
    vol_d, bd = vol.to(DEV), torch.zeros(32, device=DEV)
    framed = torch.stack([torch.from_numpy(_norm_rule(vol.numpy(), o, tile, 127.3, 73.91)) for o in origins])
    assert len(framed.unique()) > 40          # distinct values: a shift by the wrong tap cannot go unseen
    for tap in range(27):
        w = torch.zeros((27, 32))
        w[tap] = 1.0
        wd = w.to(DEV)
        _, p0 = _stem_stats(ffi, vol_d, origins, tile, 127.3, 73.91, wd, bd)
        _, p2, raw = _stem_stats(ffi, vol_d, origins, tile, 127.3, 73.91, wd, bd, raw=True)
        assert torch.equal(p0, p2), f"tap {tap}: partials"
        for b in range(2):
            shifted = _patches(framed[b])[..., tap]
            got = raw[b].cpu()
            for ch in (0, 13, 31):
                assert torch.equal(got[..., ch].view(torch.int16), shifted.view(torch.int16)), f"tap {tap} tile {b} channel {ch}"
            assert torch.equal(got, got[..., :1].expand_as(got)), f"tap {tap} tile {b}: channels differ"
