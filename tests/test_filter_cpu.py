"""The filters without a GPU: the oracle of tests/filter_cases.py against ``scipy.ndimage``, the CPU path of
``filter_volume`` against the oracle, ``gaussian_taps`` against its pinned lists, ``border_index`` against ``np.pad``,
every refusal of ``check_filter`` by name, the host query of the kernel path, and the reference's definition of
``median_filter`` / ``dilate`` / ``binary_erosion`` against the oracle.  Every comparison is exact."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from tests import filter_cases as FC

from skoots_amd import _ffi
from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import border_index, check_filter, filter_path, filter_volume, gaussian_taps

INT_DTYPES = ("uint8", "uint16")


def _ranks(radius):
    n = FC.window_size(radius)
    return sorted({0, n // 4, n // 2, n - 1})


@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("border", FC.BORDERS)
def test_rank_oracle_against_scipy(dtype, border):
    for shape in FC.CPU_SHAPES + ((9, 6, 130),):
        a = FC.source("noise", dtype, shape)
        for radius in FC.RANK_RADII:
            size = tuple(2 * r + 1 for r in radius)
            for rank in _ranks(radius):
                want = ndi.rank_filter(a, rank, size=size, mode=FC.SCIPY_MODE[border], cval=0)
                assert np.array_equal(FC.oracle_rank(a, radius, rank, border), want), (shape, radius, rank)


@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("border", FC.BORDERS)
def test_tap_oracle_against_scipy(dtype, border):
    for shape in FC.CPU_SHAPES:
        a = FC.source("noise", dtype, shape)
        for taps in FC.TAP_SETS:
            s, W = a.astype(np.int64), 1
            for axis, t in enumerate(taps):
                s = ndi.correlate1d(s, np.array(t, dtype=np.int64), axis=axis, output=np.int64, mode=FC.SCIPY_MODE[border],
                                    cval=0)
                W *= sum(t)
            want = ((s + W // 2) // W).astype(a.dtype)
            assert np.array_equal(FC.oracle_taps(a, taps, border), want), (shape, taps)


@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("border", FC.BORDERS)
def test_cpu_path_ranks(dtype, border):
    for shape in FC.CPU_SHAPES:
        for kind in ("noise", "two", "salt"):
            a = FC.source(kind, dtype, shape)
            t = FC.to_torch(a)
            for radius in FC.RANK_RADII:
                for rank in _ranks(radius):
                    got = filter_volume(t, "rank", radius=radius, rank=rank, border=border)
                    assert got.dtype == t.dtype and tuple(got.shape) == shape and got.device == t.device
                    assert np.array_equal(FC.to_numpy(got), FC.expected_rank(kind, dtype, shape, radius, rank, border))


def test_cpu_path_names_float_and_leading_axis():
    shape, radius = (5, 7, 70), (1, 1, 1)
    a = FC.source("noise", "uint16", shape)
    t = FC.to_torch(a)
    for how, rank in (("min", 0), ("median", 13), ("max", 26)):
        want = FC.expected_rank("noise", "uint16", shape, radius, rank, "mirror")
        assert np.array_equal(FC.to_numpy(filter_volume(t, how, radius=radius)), want)
        assert np.array_equal(FC.to_numpy(filter_volume(t, "rank", radius=radius, rank=how)), want)
    lead = filter_volume(t.unsqueeze(0), "median", radius=radius)
    assert tuple(lead.shape) == (1,) + shape
    assert np.array_equal(FC.to_numpy(lead[0]), FC.expected_rank("noise", "uint16", shape, radius, 13, "mirror"))
    f = FC.source("float", "float32", shape)
    for border in FC.BORDERS:
        for rank in (0, 13, 26):
            got = filter_volume(torch.from_numpy(f.copy()), "rank", radius=radius, rank=rank, border=border)
            assert got.dtype == torch.float32
            assert np.array_equal(got.numpy(), FC.expected_rank("float", "float32", shape, radius, rank, border))


@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("border", FC.BORDERS)
def test_cpu_path_taps(dtype, border):
    for shape in FC.CPU_SHAPES:
        t = FC.to_torch(FC.source("noise", dtype, shape))
        for taps in FC.TAP_SETS:
            got = filter_volume(t, "taps", taps=taps, border=border)
            assert got.dtype == t.dtype and tuple(got.shape) == shape
            assert np.array_equal(FC.to_numpy(got), FC.expected_taps("noise", dtype, shape, taps, border))
    shape = (5, 7, 70)
    t = FC.to_torch(FC.source("noise", dtype, shape))
    box = ((1,) * 3, (1,) * 5, (1,))
    assert np.array_equal(FC.to_numpy(filter_volume(t, "mean", radius=(1, 2, 0), border=border)),
                          FC.expected_taps("noise", dtype, shape, box, border))
    gauss = (FC.GAUSS_1, FC.GAUSS_HALF, (256,))
    assert np.array_equal(FC.to_numpy(filter_volume(t, "gauss", sigma=(1, 0.5, 0), border=border)),
                          FC.expected_taps("noise", dtype, shape, gauss, border))


def test_gaussian_taps():
    assert gaussian_taps(1) == list(FC.GAUSS_1)
    assert gaussian_taps(0.5) == list(FC.GAUSS_HALF)
    assert gaussian_taps(1 / 3) == list(FC.GAUSS_THIRD)
    two = gaussian_taps(2)
    assert len(two) == FC.GAUSS_2_LEN and tuple(two[5:8]) == FC.GAUSS_2_MIDDLE
    assert gaussian_taps(0) == [256] and gaussian_taps(0, total=7) == [7]
    for sigma in (0.2, 1 / 3, 0.5, 0.8, 1, 1.5, 2, 2.5, 2.7, 4, 8):
        for radius in (None, 0, 1, 4, 8):
            for total in (256, 16, 4096):
                w = gaussian_taps(sigma, radius, total)
                assert w == FC.gauss_definition(sigma, radius, total)
                assert sum(w) == total and w == w[::-1] and len(w) % 2 == 1 and len(w) <= 17
                assert (w[0] != 0 or len(w) == 1) and min(w) >= 0
    for bad in (dict(sigma=-1), dict(sigma=float("inf")), dict(sigma=float("nan")), dict(sigma=1, radius=9),
                dict(sigma=1, radius=1.5), dict(sigma=1, total=0), dict(sigma=1, total=4097)):
        with pytest.raises(ValueError):
            gaussian_taps(**bad)


def test_border_index_against_numpy_pad():
    for n in (1, 2, 5):
        line = np.arange(n)
        for border in FC.BORDERS:
            padded = np.pad(line, (20, 20), mode=FC.PAD_MODE[border], **({"constant_values": -1} if border == "zero" else {}))
            for i in range(-20, n + 20):
                assert border_index(i, n, border) == padded[i + 20], (i, n, border)
    with pytest.raises(ValueError, match="border"):
        border_index(0, 3, "wrap")
    with pytest.raises(ValueError, match="at least one"):
        border_index(0, 0, "edge")


def test_refusals_by_name():
    u8 = torch.zeros((4, 5, 6), dtype=torch.uint8)
    f32 = torch.zeros((4, 5, 6), dtype=torch.float32)
    ok = check_filter(u8, "median", radius=(1, 1, 0))
    assert ok == ((4, 5, 6), ("rank", (1, 1, 0), 4))
    assert check_filter(f32, "rank", radius=(2, 2, 2), rank="median")[1] == ("rank", (2, 2, 2), 62)
    assert check_filter(u8.unsqueeze(0), "mean", radius=(8, 0, 1))[1] == ("taps", ([1] * 17, [1], [1] * 3))
    value = ((u8, dict(how="mode", radius=(1, 1, 1)), "how = 'mode'"),
             (u8, dict(how="median", radius=(1, 1, 1), border="wrap"), "border = 'wrap'"),
             (u8, dict(how="median"), "radius is missing"),
             (u8, dict(how="median", radius=(1, 1, 1), rank=3), "not rank"),
             (u8, dict(how="median", radius=(1, 1, 1), sigma=(1, 1, 1)), "not sigma"),
             (u8, dict(how="rank", radius=(1, 1, 1)), "rank is missing"),
             (u8, dict(how="gauss", radius=(1, 1, 1)), "not radius"),
             (u8, dict(how="taps", sigma=(1, 1, 1)), "not sigma"),
             (u8, dict(how="median", radius=(1, 1)), "three"),
             (u8, dict(how="median", radius=(1, 1, 1.0)), "three integers"),
             (u8, dict(how="median", radius=(1, 3, 1)), "radii in 0 .. 2"),
             (u8, dict(how="max", radius=(-1, 0, 0)), "radii in 0 .. 2"),
             (u8, dict(how="mean", radius=(9, 0, 0)), "radii in 0 .. 8"),
             (u8, dict(how="rank", radius=(1, 1, 0), rank=9), "ranks 0 .. 8"),
             (u8, dict(how="rank", radius=(1, 1, 0), rank=-1), "ranks 0 .. 8"),
             (u8, dict(how="rank", radius=(1, 1, 0), rank="mode"), "ranks 0 .. 8"),
             (u8, dict(how="rank", radius=(1, 1, 0), rank=2.0), "ranks 0 .. 8"),
             (u8, dict(how="gauss", sigma=(1, -1, 1)), "sigma"),
             (u8, dict(how="gauss", sigma=(1, 1)), "three"),
             (u8, dict(how="taps", taps=([1], [1])), "three lists"),
             (u8, dict(how="taps", taps=([1], [1], [1, 1])), "count must be odd"),
             (u8, dict(how="taps", taps=([1] * 19, [1], [1])), "count must be odd"),
             (u8, dict(how="taps", taps=([1], [1], [])), "count must be odd"),
             (u8, dict(how="taps", taps=([1], [0], [1])), "tap sum of y is 0"),
             (u8, dict(how="taps", taps=([1], [1], [1, 4095, 1])), "tap sum of z is 4097"),
             (u8, dict(how="taps", taps=([1], [1, -1, 1], [1])), "non-negative integers"),
             (u8, dict(how="taps", taps=([1], [1], [0.5, 1, 0.5])), "non-negative integers"),
             (torch.zeros((4, 5), dtype=torch.uint8), dict(how="median", radius=(1, 1, 1)), "shape"),
             (torch.zeros((2, 4, 5, 6), dtype=torch.uint8), dict(how="median", radius=(1, 1, 1)), "shape"),
             (torch.zeros((4, 0, 6), dtype=torch.uint8), dict(how="median", radius=(1, 1, 1)), "shape"))
    for volume, kwargs, word in value:
        with pytest.raises(ValueError, match=word):
            check_filter(volume, **kwargs)
        with pytest.raises(ValueError, match=word):
            filter_volume(volume, **kwargs)
    kind = ((np.zeros((4, 5, 6), np.uint8), dict(how="median", radius=(1, 1, 1)), "must be a tensor"),
            (f32, dict(how="mean", radius=(1, 1, 1)), "float32.*no tap filter"),
            (f32, dict(how="gauss", sigma=(1, 1, 1)), "float32.*no tap filter"),
            (f32.double(), dict(how="median", radius=(1, 1, 1)), "float64.*uint8, uint16 or float32"),
            (u8.to(torch.int32), dict(how="median", radius=(1, 1, 1)), "int32.*uint8, uint16 or float32"),
            (u8.to(torch.int16), dict(how="mean", radius=(1, 1, 1)), "int16.*uint8 or uint16"),
            (u8.bool(), dict(how="taps", taps=([1], [1], [1])), "bool.*no tap filter"))
    for volume, kwargs, word in kind:
        with pytest.raises(TypeError, match=word):
            check_filter(volume, **kwargs)
        with pytest.raises(TypeError, match=word):
            filter_volume(volume, **kwargs)


def test_abi_and_the_host_query_of_the_path():
    assert _ffi.lib.sk_abi_version() >= 33
    for name in ("sk_filter_rank", "sk_filter_taps", "sk_filter_path", "sk_filter_tile"):
        assert name in _ffi.EXPORTS
    assert tuple(_ffi.lib.sk_filter_tile(k) for k in range(4)) == M.FILTER_TILE + (0,)
    assert filter_path(torch.uint8, (3, 4, 16), "median", radius=(1, 1, 1)) == ("network", "vector")
    assert filter_path(torch.float32, (3, 4, 16), "rank", radius=(1, 1, 0), rank=4) == ("network", "vector")
    assert filter_path(torch.uint8, (3, 4, 16), "rank", radius=(1, 1, 1), rank=12) == ("radix", "vector")
    assert filter_path(torch.uint8, (3, 4, 16), "median", radius=(2, 1, 1)) == ("radix", "vector")
    assert filter_path(torch.uint8, (3, 4, 16), "median", radius=(1, 0, 1)) == ("radix", "vector")
    assert filter_path(torch.uint8, (3, 4, 17), "median", radius=(1, 1, 2)) == ("radix", "scalar")
    assert filter_path(torch.uint8, (3, 4, 16), "median", radius=(2, 2, 1), aligned=False) == ("radix", "scalar")
    assert filter_path(torch.uint16, (3, 4, 6), "min", radius=(1, 1, 1)) == ("extreme", "vector")
    assert filter_path(torch.uint16, (3, 4, 7), "rank", radius=(2, 2, 2), rank=124) == ("extreme", "scalar")
    assert filter_path(torch.float32, (3, 4, 7), "rank", radius=(2, 2, 2), rank=123) == ("radix", "vector")
    # accumulator width: 32 bits where W vmax < 2^32.  uint16: W = 65536 is just below (65536 * 65535 = 2^32 - 65536),
    # 65537 does not factor into sums within 4096, so the next total, 16 * 16 * 257, is just above
    assert filter_path(torch.uint16, (3, 4, 8), "taps", taps=([16], [16], [256])) == ("acc32", "vector")
    assert filter_path(torch.uint16, (3, 4, 8), "taps", taps=([16], [16], [257])) == ("acc64", "vector")
    # uint8: 256^3 * 255 = 2^32 - 2^24 is below, 256 * 256 * 258 * 255 is above
    assert filter_path(torch.uint8, (3, 4, 8), "taps", taps=([256], [256], [256])) == ("acc32", "vector")
    assert filter_path(torch.uint8, (3, 4, 9), "taps", taps=([256], [256], [258])) == ("acc64", "scalar")
    with pytest.raises(ValueError, match="sk_filter_rank.*extents"):
        filter_path(torch.uint8, (3, 0, 8), "median", radius=(1, 1, 1))
    with pytest.raises(ValueError, match="sk_filter_taps.*dtype"):
        filter_path(torch.float32, (3, 4, 8), "mean", radius=(1, 1, 1))


def test_the_references_definition_is_the_oracles():
    """``median_filter`` / ``dilate`` / ``binary_erosion`` as skoots/lib/morphology.py means them -- ``F.conv3d`` with the
    one-hot 27-kernel and zero padding, then ``torch.median`` / ``max`` / ``min`` over the 27 channels -- stated afresh:
    rank 13 / 26 / 0 of the window at the ``"zero"`` border, radius (1, 1, 1)"""
    import torch.nn.functional as F
    shape = (6, 7, 8)
    a = FC.source("float", "float32", shape)
    a = np.where(np.isfinite(a), a, np.float32(3.0)).astype(np.float32)     # a convolution turns inf * 0 into NaN
    kernel = torch.zeros((27, 1, 3, 3, 3))
    for i in range(27):
        kernel.view(27, 27)[i, i] = 1.0
    features = F.conv3d(torch.from_numpy(a)[None, None], kernel, padding=1)          # (1, 27, X, Y, Z)
    for reduce, rank in ((lambda f: torch.median(f, dim=1)[0], 13), (lambda f: torch.max(f, dim=1)[0], 26),
                         (lambda f: torch.min(f, dim=1)[0], 0)):
        want = FC.oracle_rank(a, (1, 1, 1), rank, "zero")
        assert np.array_equal(reduce(features)[0].numpy(), want)
        assert np.array_equal(filter_volume(torch.from_numpy(a), "rank", radius=(1, 1, 1), rank=rank, border="zero").numpy(),
                              want)
