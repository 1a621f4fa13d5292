"""``lib.morphology``'s grey-value transforms on CPU tensors -- the numpy mirror of ``sk_tile_histograms`` and
``sk_apply_tile_luts`` and the table builders -- against the oracle of tests/equalize_cases.py, and the properties the
definitions promise.  Every comparison is exact.  No GPU."""
import numpy as np
import pytest
import torch

from tests import equalize_cases as EC

from skoots_amd import _ffi
from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import (apply_tile_luts, check_equalize, equalize, equalize_lut, histogram_shift, match_lut,
                                       stretch_bounds, stretch_lut, tile_histograms)

DTYPES = ("uint8", "uint16")


def _kinds(dtype):
    return ("noise", "ramp", "two") + (("noise12",) if dtype == "uint16" else ())


def test_abi_and_exports():
    assert _ffi.lib.sk_abi_version() >= 34
    for name in ("sk_tile_histograms", "sk_apply_tile_luts", "sk_equalize_path"):
        assert hasattr(_ffi.lib, name)


def test_histogram_shift():
    for bins in (256, 1024, 4096):
        for vmax in (0, 1, 255, 256, 1023, 1024, 4095, 4096, 32768, 65535):
            s = histogram_shift(vmax, bins)
            assert vmax >> s < bins and (s == 0 or vmax >> (s - 1) >= bins)
    assert histogram_shift(65535, 256) == 8 and histogram_shift(4095, 1024) == 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EC.CPU_SHAPES, ids=str)
def test_histograms_against_the_oracle(dtype, shape):
    for kind in _kinds(dtype):
        a = EC.source(kind, dtype, shape)
        for tile in EC.CPU_TILES:
            for bins in EC.BINS[dtype]:
                shift = 0 if dtype == "uint8" else EC.shift_of(int(a.max()), bins)
                got = tile_histograms(EC.to_torch(a), tile, bins).numpy()
                want = EC.expected_histograms(kind, dtype, shape, tile, bins, shift)
                assert got.dtype == np.int64 and got.shape == want.shape == EC.grid_of(shape, tile) + (bins,)
                assert np.array_equal(got, want), (kind, tile, bins)
                # the voxel count of every tile
                t = EC.sides_of(shape, tile)
                ext = [np.minimum((np.arange(c) + 1) * s, n) - np.arange(c) * s for c, s, n in zip(got.shape, t, shape)]
                assert np.array_equal(got.sum(-1), ext[0][:, None, None] * ext[1][None, :, None] * ext[2][None, None, :])
    if dtype == "uint16":       # an explicit shift, and the clamp of the last bin
        a = EC.source("noise", dtype, shape)
        got = tile_histograms(EC.to_torch(a), (4, 4, 4), 256, 4).numpy()
        assert np.array_equal(got, EC.oracle_histograms(a, (4, 4, 4), 256, 4))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EC.CPU_SHAPES, ids=str)
def test_apply_against_the_oracle_and_its_consequences(dtype, shape):
    a = EC.source("noise", dtype, shape)
    top = int(np.iinfo(dtype).max)
    for tile in EC.CPU_TILES:
        grid = EC.grid_of(shape, tile)
        for bins in EC.BINS[dtype]:
            shift = 0 if dtype == "uint8" else EC.shift_of(int(a.max()), bins)
            luts = EC.random_luts(dtype, grid, bins)
            out = {}
            for interpolate in (True, False):
                got = EC.to_numpy(apply_tile_luts(EC.to_torch(a), torch.from_numpy(luts.copy()), tile, shift, interpolate))
                assert got.dtype == a.dtype
                assert np.array_equal(got, EC.oracle_apply(a, luts, tile, shift, interpolate)), (tile, bins, interpolate)
                out[interpolate] = got
            if tile in (None, "slices") or max(grid) == 1:
                assert np.array_equal(out[True], out[False])      # one tile, or tz = 1: nothing to interpolate
            # identical tables in all tiles give luts[bin(v)], interpolated or not; the identity gives the input back
            same = np.broadcast_to(luts[:1, :1, :1], luts.shape).copy()
            ident = np.broadcast_to(np.minimum(np.arange(bins, dtype=np.int64) << shift, top).astype(np.int32), luts.shape).copy()
            for interpolate in (True, False):
                got = EC.to_numpy(apply_tile_luts(EC.to_torch(a), torch.from_numpy(same), tile, shift, interpolate))
                assert np.array_equal(got, same[0, 0, 0][EC.bin_of(a, bins, shift)].astype(a.dtype))
                got = EC.to_numpy(apply_tile_luts(EC.to_torch(a), torch.from_numpy(ident), tile, shift, interpolate))
                assert np.array_equal(got, ((a >> shift) << shift) if shift else a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_builders_against_the_oracle(dtype):
    top = int(np.iinfo(dtype).max)
    for kind in _kinds(dtype) + ("const",):
        a = EC.source(kind, dtype, (13, 10, 21))
        for bins in EC.BINS[dtype]:
            shift = 0 if dtype == "uint8" else EC.shift_of(int(a.max()), bins)
            for tile in ((4, 4, 4), "slices", None) if bins == 256 or kind == "ramp" else (None,):
                h = EC.oracle_histograms(a, tile, bins, shift)
                g = EC.oracle_histograms(EC.source("ramp", dtype, (13, 10, 21)), None, bins, shift)[0, 0, 0]
                for low, high in ((0.5, 99.5), (0, 100), (10, 60)):
                    assert np.array_equal(stretch_lut(h, low, high, top, shift), EC.per_tile(EC.stretch_lut_one, h, low, high, top, shift))
                for clip in (None, 3.0, 0.5, 40):
                    assert np.array_equal(equalize_lut(h, clip, top), EC.per_tile(EC.equalize_lut_one, h, clip, top))
                assert np.array_equal(match_lut(h, g, shift, top), EC.per_tile(EC.match_lut_one, h, g, shift, top))
                assert np.array_equal(match_lut(h, h, shift, top), np.array(
                    [EC.match_lut_one(r, r, shift, top) for r in h.reshape(-1, bins)], dtype=np.int32).reshape(h.shape))
                for lut in (stretch_lut(h), equalize_lut(h), match_lut(h, g)):
                    assert lut.dtype == np.int32 and lut.shape == h.shape


@pytest.mark.parametrize("dtype", DTYPES)
def test_builder_properties(dtype):
    top = int(np.iinfo(dtype).max)
    a = EC.source("ramp", dtype, (13, 10, 21))
    for bins in EC.BINS[dtype]:
        shift = 0 if dtype == "uint8" else EC.shift_of(int(a.max()), bins)
        b = EC.bin_of(a, bins, shift)
        h = EC.oracle_histograms(a, None, bins, shift)
        # nearest-rank percentiles of the bins
        for low, high in ((0.5, 99.5), (0, 100), (25, 75), (33.3, 33.4)):
            lo, hi = stretch_bounds(h, low, high)
            assert int(lo[0, 0, 0]) == int(np.percentile(b, low, method="inverted_cdf"))
            assert int(hi[0, 0, 0]) == int(np.percentile(b, high, method="inverted_cdf"))
        # plain equalisation: round-half-up of cdf * top
        n = a.size
        want = (np.cumsum(h[0, 0, 0]) * top + n // 2) // n
        assert np.array_equal(equalize_lut(h, None, top)[0, 0, 0], want)
        # a clipped histogram keeps its total, and the last entry is top
        ht = EC.oracle_histograms(a, (4, 4, 4), bins, shift)
        for clip in (3.0, 1.0, 0.25):
            for row in ht.reshape(-1, bins):
                assert sum(EC.clipped_one(row, clip)) == int(row.sum())
            assert (equalize_lut(ht, clip, top)[..., -1] == top).all()
        assert (equalize_lut(ht, None, top)[..., -1] == top).all()
        # matching a volume to itself is the identity on occupied bins
        lut = match_lut(h, h[0, 0, 0], 0, bins - 1)[0, 0, 0]
        occupied = np.nonzero(h[0, 0, 0])[0]
        assert np.array_equal(lut[occupied], occupied)


def test_match_recovers_a_strictly_increasing_map():
    """``a`` matched to ``c = f(a)`` with ``f`` strictly increasing on the occupied values gives ``c``"""
    a = EC.source("noise", "uint8", (13, 10, 21)) // 2          # 0 .. 127
    f = (np.arange(256) * 3 // 2 + 5).astype(np.uint8)           # strictly increasing on 0 .. 127
    c = f[a]
    got = EC.to_numpy(equalize(EC.to_torch(a), "match", target=EC.to_torch(c)))
    assert np.array_equal(got, c)
    h = np.bincount(c.ravel(), minlength=256).astype(np.int64)
    assert np.array_equal(EC.to_numpy(equalize(EC.to_torch(a), "match", target=torch.from_numpy(h))), c)
    a16 = (EC.source("noise12", "uint16", (13, 10, 21)) // 4).astype(np.uint16)          # 0 .. 1023: shift 0 at 1024 bins
    c16 = (a16 * 3 + 11).astype(np.uint16)                                                # below 4096: shift 2 at 1024 bins
    got = EC.to_numpy(equalize(EC.to_torch(a16), "match", target=EC.to_torch(c16), bins=4096))
    assert np.array_equal(got, c16)


def test_slice_matching_removes_flicker():
    """every plane's median within one bin of the stack's.  On this source it is the stack's exactly: a plane has 130
    samples in pairwise different bins, so its median bin b has H[b] / n = 1 / 2 and is sent to the first bin at which the
    stack's cumulative sum reaches m / 2 -- the stack's nearest-rank median; the tables never fall, so the median of the
    outputs is the output of the median."""
    for dtype in DTYPES:
        a = EC.source("flicker", dtype, (13, 10, 21))
        bins = 256 if dtype == "uint8" else 1024
        shift = 0 if dtype == "uint8" else EC.shift_of(int(a.max()), bins)
        before = [np.percentile(EC.bin_of(a[:, :, z], bins, shift), 50, method="inverted_cdf") for z in range(a.shape[2])]
        assert max(before) - min(before) > 8
        got = EC.to_numpy(equalize(EC.to_torch(a), "match", tile="slices"))
        assert np.array_equal(got, EC.oracle_equalize(a, "match", tile="slices"))
        stack = np.percentile(EC.bin_of(a, bins, shift), 50, method="inverted_cdf")
        for z in range(a.shape[2]):
            assert abs(np.percentile(EC.bin_of(got[:, :, z], bins, shift), 50, method="inverted_cdf") - stack) <= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("how", M.EQUALIZE_HOW)
def test_equalize_against_the_oracle(dtype, how):
    for shape in EC.CPU_SHAPES:
        for kind in ("ramp", "noise12" if dtype == "uint16" else "two"):
            a = EC.source(kind, dtype, shape)
            for tile in EC.CPU_TILES:
                # every tile at 256 bins; the larger tables where the oracle's loop per tile and bin stays short
                few = tile in ((5, 3, 8), "slices", None) and kind == "ramp"
                for bins in (EC.BINS[dtype] if few else EC.BINS[dtype][:1]):
                    for interpolate in (True, False):
                        got = EC.to_numpy(equalize(EC.to_torch(a), how, tile=tile, bins=bins, interpolate=interpolate))
                        want = EC.oracle_equalize(a, how, tile=tile, bins=bins, interpolate=interpolate)
                        assert got.dtype == a.dtype and np.array_equal(got, want), (shape, kind, tile, bins, interpolate)
    a = EC.source("ramp", dtype, (13, 10, 21))
    v4 = EC.to_torch(a).unsqueeze(0)
    assert tuple(equalize(v4, how).shape) == (1, 13, 10, 21)
    kw = {"stretch": dict(low=5, high=70, top=200), "equalize": dict(clip=None), "match": dict(
        target=EC.to_torch(EC.source("noise", dtype, (5, 6, 7))))}[how]
    want = EC.oracle_equalize(a, how, tile=(5, 3, 8), **{k: (EC.to_numpy(v) if k == "target" else v) for k, v in kw.items()})
    assert np.array_equal(EC.to_numpy(equalize(EC.to_torch(a), how, tile=(5, 3, 8), **kw)), want)


def test_refusals():
    v = torch.zeros((4, 5, 6), dtype=torch.uint8)
    w = torch.zeros((4, 5, 6), dtype=torch.uint16)
    for bad in (torch.float32, torch.float16, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool, torch.complex64):
        with pytest.raises(TypeError, match="take uint8 or uint16"):
            check_equalize(torch.zeros((4, 5, 6), dtype=bad), "stretch")
    with pytest.raises(TypeError, match="must be a tensor"):
        check_equalize(np.zeros((4, 5, 6), np.uint8), "stretch")
    with pytest.raises(ValueError, match="how = 'clahe', must be one of"):
        check_equalize(v, "clahe")
    with pytest.raises(ValueError, match="must be .X, Y, Z. or .1, X, Y, Z."):
        check_equalize(torch.zeros((2, 4, 5, 6), dtype=torch.uint8), "stretch")
    with pytest.raises(ValueError, match="must be .X, Y, Z. or .1, X, Y, Z."):
        check_equalize(torch.zeros((4, 5), dtype=torch.uint8), "stretch")
    with pytest.raises(ValueError, match="within 2.30"):
        check_equalize(torch.zeros((1, 1, 2 ** 30 + 1), dtype=torch.uint8, device="meta"), "stretch")
    with pytest.raises(ValueError, match="2.31 voxels or more"):
        check_equalize(torch.zeros((2 ** 11, 2 ** 10, 2 ** 10), dtype=torch.uint8, device="meta"), "stretch")
    check_equalize(torch.zeros((2 ** 11, 2 ** 10, 2 ** 10), dtype=torch.uint8, device="meta"), "stretch", tile="slices")
    for tile in ((1, 2), (1, 2, -1), (1.0, 2, 3), "planes", (1, 2, True)):
        with pytest.raises(ValueError, match="tile"):
            check_equalize(v, "stretch", tile=tile)
    with pytest.raises(ValueError, match="bins = 1024: volume is torch.uint8 and takes 256"):
        check_equalize(v, "stretch", bins=1024)
    with pytest.raises(ValueError, match="bins = 512, must be 256, 1024 or 4096"):
        check_equalize(w, "stretch", bins=512)
    for low, high in ((50, 50), (60, 40), (-1, 50), (0, 101)):
        with pytest.raises(ValueError, match="low = "):
            check_equalize(v, "stretch", low=low, high=high)
    for clip in (0, -1.0, float("inf"), "3"):
        with pytest.raises(ValueError, match="clip = "):
            check_equalize(v, "equalize", clip=clip)
    with pytest.raises(ValueError, match="how='stretch' takes low and high, not clip"):
        check_equalize(v, "stretch", clip=2.0)
    with pytest.raises(ValueError, match="how='equalize' takes clip, not low"):
        check_equalize(v, "equalize", low=1.0)
    with pytest.raises(ValueError, match="how='equalize' takes clip, not target"):
        check_equalize(v, "equalize", target=v)
    with pytest.raises(ValueError, match="how='match' takes target, not high"):
        check_equalize(v, "match", high=99.0)
    with pytest.raises(ValueError, match="top = 256 is beyond the maximum of torch.uint8"):
        check_equalize(v, "stretch", top=256)
    with pytest.raises(ValueError, match="top = 0"):
        check_equalize(v, "stretch", top=0)
    with pytest.raises(ValueError, match="interpolate = 1, must be True or False"):
        check_equalize(v, "stretch", interpolate=1)
    with pytest.raises(TypeError, match="target is torch.uint16 and volume is torch.uint8"):
        check_equalize(v, "match", target=w)
    with pytest.raises(ValueError, match="a target histogram must be int64 with bins = 256 entries"):
        check_equalize(v, "match", target=torch.zeros(1024, dtype=torch.int64))
    with pytest.raises(ValueError, match="a target histogram must be int64"):
        check_equalize(v, "match", target=torch.zeros(256, dtype=torch.int32))
    with pytest.raises(TypeError, match="target must be a volume, a 1-D int64 histogram or None"):
        check_equalize(v, "match", target="reference.tif")
    with pytest.raises(ValueError, match="target of shape .* has 2.31 voxels or more"):
        check_equalize(v, "match", target=torch.zeros((2 ** 11, 2 ** 10, 2 ** 10), dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match="total in 1 .. 2.31 - 1"):
        equalize(v, "match", target=torch.zeros(256, dtype=torch.int64))
    shape, plan = check_equalize(w.unsqueeze(0), "equalize", tile="slices")
    assert shape == (4, 5, 6) and plan["bins"] == 1024 and plan["top"] == 65535 and plan["tile"] == (0, 0, 1)
    # apply_tile_luts refuses tables that are not what it states
    luts = torch.zeros((1, 1, 1, 256), dtype=torch.int32)
    for bad in (luts.to(torch.int64), luts[0], torch.zeros((1, 1, 2, 256), dtype=torch.int32), torch.zeros((1, 1, 1, 100), dtype=torch.int32)):
        with pytest.raises(ValueError, match="luts must be an int32 tensor"):
            apply_tile_luts(v, bad)
    for value in (-1, 256):
        with pytest.raises(ValueError, match="luts holds values outside 0 .. 255"):
            apply_tile_luts(v, torch.full((1, 1, 1, 256), value, dtype=torch.int32))
    with pytest.raises(ValueError, match="shift = 9"):
        apply_tile_luts(w, torch.zeros((1, 1, 1, 256), dtype=torch.int32), shift=9)
    with pytest.raises(ValueError, match="uint8 takes shift 0"):
        tile_histograms(v, None, 256, 1)


def test_path_query_needs_no_device():
    assert M.equalize_path(torch.uint8, (64, 64, 130), None) == ("one", "lds/-+one/lookup")
    assert M.equalize_path(torch.uint8, (64, 64, 130), "slices") == ("planes", "lds/-+tile/lookup")
    assert M.equalize_path(torch.uint8, (9, 9, 9), (1, 1, 1)) == ("global", "gather/-+tile/lookup")
    assert M.equalize_path(torch.uint8, (9, 9, 70), (3, 5, 7)) == ("global", "gather/xy+interp/acc32")
    assert M.equalize_path(torch.uint16, (21, 21, 70), (8, 8, 16), 4096) == ("ztiles", "lds/xy+interp/acc32")
    assert M.equalize_path(torch.uint16, (21, 21, 130), (16, 16, 64), 256) == ("ztiles", "lds/xy+interp/acc64")
    assert M.equalize_path(torch.uint16, (21, 21, 70), (8, 8, 16), 4096, interpolate=False) == ("ztiles", "lds/-+tile/lookup")
    with pytest.raises(ValueError, match="sk_equalize_path: extents"):
        M.equalize_path(torch.uint8, (0, 1, 1), None)
