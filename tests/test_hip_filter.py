"""``sk_filter_rank`` and ``sk_filter_taps`` (skoots_amd/csrc/filter.hip) on the device against the integer oracle of
tests/filter_cases.py: z extents around a lane's 16-byte unit and around a wave, volumes smaller than the window, tile
edges and many workgroups, every rank of a window, ties, float32 keys, both accumulator widths and both row paths of the
tap kernel, non-contiguous and unaligned inputs, the C ABI on sentinel-filled buffers, the reference's names.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import filter_cases as FC

from skoots_amd import _ffi
from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import filter_path, filter_rank_device, filter_volume

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rank(kind, dtype, shape, radius, rank, border, method=None):
    """``method=None``: through ``filter_volume``, the selection ``filter_path`` names; else that selection forced"""
    src = FC.to_torch(FC.source(kind, dtype, shape)).to(DEV)
    if method is None:
        got = filter_volume(src, "rank", radius=radius, rank=rank, border=border)
    else:
        got = filter_rank_device(src, radius, rank, border, method)
    want = FC.expected_rank(kind, dtype, tuple(shape), tuple(radius), rank, border)
    assert got.dtype == src.dtype and got.device == src.device and tuple(got.shape) == want.shape
    assert np.array_equal(FC.to_numpy(got), want), (kind, dtype, shape, radius, rank, border)


def _taps(kind, dtype, shape, taps, border):
    src = FC.to_torch(FC.source(kind, dtype, shape)).to(DEV)
    got = filter_volume(src, "taps", taps=taps, border=border)
    want = FC.expected_taps(kind, dtype, tuple(shape), tuple(tuple(t) for t in taps), border)
    assert got.dtype == src.dtype and got.device == src.device and tuple(got.shape) == want.shape
    assert np.array_equal(FC.to_numpy(got), want), (kind, dtype, shape, taps, border)


Z_CASES = [("uint8", z) for z in (1, 15, 16, 17, 1023, 1024, 1025)] + [("uint16", z) for z in (1, 7, 8, 9, 511, 512, 513)]


@pytest.mark.parametrize("dtype,z", Z_CASES, ids=lambda v: str(v))
def test_z_around_a_lane_and_a_wave(dtype, z):
    paths = set()
    for radius in ((1, 1, 1), (0, 0, 2)):
        n = FC.window_size(radius)
        for border in FC.BORDERS:
            for rank in (0, n // 2, n - 1):
                _rank("noise", dtype, (3, 4, z), radius, rank, border)
                paths.add(filter_path(getattr(torch, dtype), (3, 4, z), "rank", radius=radius, rank=rank))
                _rank("noise", dtype, (3, 4, z), radius, rank, border, "radix")     # the ends by the descent too
    for border in FC.BORDERS:
        _rank("noise", dtype, (3, 4, z), (1, 1, 0), 4, border, "network")
    rows = "vector" if (z * np.dtype(dtype).itemsize) % 4 == 0 else "scalar"
    assert paths == {("extreme", rows), ("network", rows), ("radix", rows)}


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 3, 5), (1, 1, 40)), ids=str)
def test_volumes_smaller_than_the_window(shape):
    radius = (2, 2, 2)
    for border in FC.BORDERS:       # "mirror" reflects more than once here
        for dtype in ("uint8", "uint16"):
            for rank in (0, 31, 62, 124):
                _rank("noise", dtype, shape, radius, rank, border)
        _taps("noise", "uint8", shape, (FC.GAUSS_1, (1,) * 17, FC.SPARSE_Z), border)
        _taps("noise", "uint16", shape, ((1,) * 5, FC.GAUSS_1, (1,) * 17), border)


def test_one_row_more_than_the_tile():
    tx, ty, tz = M.FILTER_TILE
    assert (tx, ty, tz) == tuple(_ffi.lib.sk_filter_tile(k) for k in range(3))
    for dtype in ("uint8", "uint16"):
        shape = (tx + 1, ty + 1, tz // np.dtype(dtype).itemsize + 1)
        for border in FC.BORDERS:
            _rank("noise", dtype, shape, (2, 2, 2), 62, border)
            _rank("salt", dtype, shape, (1, 1, 1), 13, border)
            _rank("noise", dtype, shape, (2, 1, 0), 14, border)
            _taps("noise", dtype, shape, (FC.GAUSS_1, FC.GAUSS_HALF, FC.GAUSS_1), border)


@pytest.mark.parametrize("dtype", ("uint8", "uint16"))
@pytest.mark.parametrize("radius", ((1, 1, 1), (2, 2, 1)), ids=str)
def test_many_workgroups(dtype, radius):
    _rank("salt", dtype, (69, 71, 301), radius, FC.window_size(radius) // 2, "mirror")
    if radius == (1, 1, 1):
        _rank("salt", dtype, (69, 71, 301), radius, 13, "mirror", "radix")


def test_both_selection_methods_on_every_network_window():
    """the median of 3 x 3 x 1 and of 3 x 3 x 3 by the exchange network and by the radix descent, every dtype"""
    for dtype, kind in (("uint8", "noise"), ("uint8", "two"), ("uint16", "noise"), ("uint16", "salt"), ("float32", "float")):
        for radius in ((1, 1, 0), (1, 1, 1)):
            assert filter_path(getattr(torch, dtype), (6, 9, 37), "median", radius=radius)[0] == "network"
            for border in FC.BORDERS:
                for method in ("network", "radix", "auto"):
                    _rank(kind, dtype, (6, 9, 37), radius, FC.window_size(radius) // 2, border, method)
    src = FC.to_torch(FC.source("noise", "uint8", (6, 9, 37))).to(DEV)
    for radius, rank in (((1, 1, 1), 12), ((1, 1, 1), 0), ((2, 1, 1), 22), ((1, 0, 1), 4), ((1, 1, 2), 22)):
        with pytest.raises(ValueError, match="sk_filter_rank: method 2 .network. is built for the median"):
            filter_rank_device(src, radius, rank, "mirror", "network")


def test_every_rank_ties_and_a_constant():
    for dtype in ("uint8", "uint16"):
        for rank in range(9):
            _rank("two", dtype, (6, 9, 37), (1, 1, 0), rank, "mirror")
            _rank("two", dtype, (6, 9, 37), (1, 1, 0), rank, "zero")
        for rank in (0, 13, 26):
            _rank("const", dtype, (6, 9, 37), (1, 1, 1), rank, "edge")
            _rank("const", dtype, (6, 9, 37), (1, 1, 1), rank, "zero")
    _taps("const", "uint16", (6, 9, 37), (FC.GAUSS_1, FC.GAUSS_1, FC.GAUSS_1), "mirror")
    _taps("two", "uint8", (6, 9, 37), (FC.BOX3, FC.BOX3, FC.BOX3), "edge")


def test_float32_negatives_zeros_and_infinities():
    a = FC.source("float", "float32", (6, 9, 37))
    assert (a < 0).any() and np.isinf(a).any() and (np.signbit(a) & (a == 0)).any() and (~np.signbit(a) & (a == 0)).any()
    for border in FC.BORDERS:
        for rank in (0, 5, 13, 20, 26):
            _rank("float", "float32", (6, 9, 37), (1, 1, 1), rank, border)
    _rank("float", "float32", (5, 6, 7), (2, 0, 1), 7, "mirror")


def test_taps_both_accumulator_widths_and_both_row_paths():
    paths = set()

    def run(dtype, shape, taps, border="mirror"):
        _taps("noise", dtype, shape, taps, border)
        paths.add(filter_path(getattr(torch, dtype), shape, "taps", taps=taps))

    box = (FC.BOX3, FC.BOX3, FC.BOX3)
    gauss = tuple(tuple(M.gaussian_taps(s)) for s in (1, 2, 0.5))
    assert gauss[0] == FC.GAUSS_1 and len(gauss[1]) == FC.GAUSS_2_LEN and gauss[2] == FC.GAUSS_HALF
    for border in FC.BORDERS:
        run("uint16", (9, 10, 72), box, border)                    # W = 27
        run("uint8", (9, 10, 72), gauss, border)                   # W = 2^24: 2^24 * 255 < 2^32
        run("uint16", (9, 10, 72), gauss, border)                  # 2^24 * 65535 >= 2^32
        run("uint8", (9, 10, 73), gauss, border)                   # rows that are no dword multiple
        run("uint16", (9, 10, 71), gauss, border)
        run("uint8", (7, 6, 50), ((1,), (1,), FC.SPARSE_Z), border)
        run("uint16", (5, 6, 40), ((1,) * 17, (1,), (1,)), border)  # radius 8 on an axis of extent 5
    assert filter_path(torch.uint16, (9, 10, 72), "taps", taps=box) == ("acc32", "vector")
    assert filter_path(torch.uint8, (9, 10, 72), "taps", taps=gauss) == ("acc32", "vector")
    assert filter_path(torch.uint16, (9, 10, 72), "taps", taps=gauss) == ("acc64", "vector")
    assert paths == {("acc32", "vector"), ("acc64", "vector"), ("acc32", "scalar"), ("acc64", "scalar")}
    src = FC.to_torch(FC.source("noise", "uint8", (9, 10, 72))).to(DEV)
    assert np.array_equal(FC.to_numpy(filter_volume(src, "gauss", sigma=(1, 2, 0.5))),
                          FC.expected_taps("noise", "uint8", (9, 10, 72), gauss, "mirror"))
    assert np.array_equal(FC.to_numpy(filter_volume(src, "mean", radius=(1, 1, 1))),
                          FC.expected_taps("noise", "uint8", (9, 10, 72), box, "mirror"))


def test_a_large_tap_tile_of_many_workgroups():
    gauss = (FC.GAUSS_1, FC.GAUSS_HALF, FC.GAUSS_1)
    _taps("noise", "uint8", (33, 35, 301), gauss, "mirror")
    _taps("noise", "uint16", (33, 35, 301), gauss, "zero")
    _taps("salt", "uint16", (21, 19, 150), ((1,) * 17, (1,) * 17, (1,) * 17), "edge")


def test_non_contiguous_and_unaligned_inputs():
    dtype, shape, radius = "uint8", (5, 7, 24), (1, 1, 1)
    a = FC.source("noise", dtype, shape)
    want = FC.expected_rank("noise", dtype, shape, radius, 13, "mirror")
    want_taps = FC.expected_taps("noise", dtype, shape, (FC.BOX3, FC.GAUSS_1, FC.GAUSS_HALF), "mirror")
    t = FC.to_torch(np.ascontiguousarray(a.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)     # (X, Y, Z) with Z outermost
    assert not t.is_contiguous()
    assert np.array_equal(FC.to_numpy(filter_volume(t, "median", radius=radius)), want)
    # a volume that starts one element into its storage: rows are not dword aligned
    store = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    store[1:].copy_(FC.to_torch(a).to(DEV).reshape(-1))
    view = store[1:].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 4 != 0
    assert np.array_equal(FC.to_numpy(filter_volume(view, "median", radius=radius)), want)
    assert np.array_equal(FC.to_numpy(filter_volume(view, "taps", taps=(FC.BOX3, FC.GAUSS_1, FC.GAUSS_HALF))), want_taps)
    lead = FC.to_torch(a).to(DEV).unsqueeze(0)
    got = filter_volume(lead, "median", radius=radius)                                         # the leading 1 is kept
    assert tuple(got.shape) == (1,) + shape and np.array_equal(FC.to_numpy(got[0]), want)


def _ints(values):
    return (C.c_int32 * len(values))(*values)


def test_c_abi_writes_nothing_outside_out_and_refuses_by_name():
    dtype, shape, radius = "uint8", (5, 7, 37), (2, 1, 1)
    a = FC.source("noise", dtype, shape)
    n_out, pad = int(np.prod(shape)), 256
    stream = _ffi.stream_ptr(torch.device(DEV))
    src = FC.to_torch(a).to(DEV)
    store = torch.full((pad + n_out + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = store[pad:pad + n_out]
    rank_call = lambda s, d, code, ext, r, k, b, m=0: _ffi.lib.sk_filter_rank(  # noqa: E731
        _ffi.ptr(s), _ffi.ptr(d), code, *ext, *r, k, b, m, stream)

    def taps_call(s, d, code, ext, taps, b):
        arrays = [None if t is None else _ints(t) for t in taps]
        lists = [v for t, arr in zip(taps, arrays) for v in (arr, 0 if t is None else len(t))]
        return _ffi.lib.sk_filter_taps(_ffi.ptr(s), _ffi.ptr(d), code, *ext, *lists, b, stream)

    _ffi.check(rank_call(src, dst, 4, shape, radius, 22, 2))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(shape), FC.expected_rank("noise", dtype, shape, radius, 22, "mirror"))
    assert bool((store[:pad] == 0xA5).all()) and bool((store[pad + n_out:] == 0xA5).all())
    store.fill_(0xA5)
    taps = (FC.GAUSS_1, FC.BOX3, FC.GAUSS_HALF)
    _ffi.check(taps_call(src, dst, 4, shape, taps, 1))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(shape), FC.expected_taps("noise", dtype, shape, taps, "edge"))
    assert bool((store[:pad] == 0xA5).all()) and bool((store[pad + n_out:] == 0xA5).all())

    # every bad argument: SK_ERR_ARG with a message, nothing launched
    store.fill_(0xA5)
    torch.cuda.synchronize()
    bad_rank = ((src, src, 4, shape, radius, 22, 2, "in == out"),
                (None, dst, 4, shape, radius, 22, 2, "NULL"),
                (src, None, 4, shape, radius, 22, 2, "NULL"),
                (src, dst, 4, shape, radius, 45, 2, "rank = 45"),
                (src, dst, 4, shape, radius, -1, 2, "rank = -1"),
                (src, dst, 4, shape, (3, 1, 1), 0, 2, "radius"),
                (src, dst, 4, shape, (1, -1, 1), 0, 2, "radius"),
                (src, dst, 4, (5, 0, 37), radius, 22, 2, "extents"),
                (src, dst, 4, (5, 7, 2 ** 30 + 1), radius, 22, 2, "2\\^30"),
                (src, dst, 3, shape, radius, 22, 2, "dtype"),
                (src, dst, 4, shape, radius, 22, 3, "border"),
                (src, dst, 4, shape, radius, 22, 2, 3, "method = 3"),
                (src, dst, 4, shape, radius, 22, 2, -1, "method = -1"))
    for *args, word in bad_rank:
        rc = rank_call(*args)
        assert rc == -1, (args[2:], word)
        with pytest.raises(ValueError, match="sk_filter_rank.*" + word):
            _ffi.check(rc)
    bad_taps = ((src, src, 4, shape, taps, 1, "in == out"),
                (None, dst, 4, shape, taps, 1, "NULL"),
                (src, dst, 4, shape, (FC.GAUSS_1, None, FC.GAUSS_HALF), 1, "NULL tap list of y"),
                (src, dst, 4, shape, ((0, 0, 0), FC.BOX3, FC.BOX3), 1, "tap sum of x is 0"),
                (src, dst, 4, shape, (FC.BOX3, FC.BOX3, (1, 4095, 1)), 1, "tap sum of z is 4097"),
                (src, dst, 4, shape, (FC.BOX3, (1, 1), FC.BOX3), 1, "2 taps on y"),
                (src, dst, 4, shape, (FC.BOX3, (1,) * 19, FC.BOX3), 1, "19 taps on y"),
                (src, dst, 4, shape, (FC.BOX3, (1, -1, 1), FC.BOX3), 1, "tap 1 of y is -1"),
                (src, dst, 1, shape, taps, 1, "dtype"),
                (src, dst, 4, (0, 7, 37), taps, 1, "extents"),
                (src, dst, 4, shape, taps, -1, "border"))
    for *args, word in bad_taps:
        rc = taps_call(*args)
        assert rc == -1, (args[2:], word)
        with pytest.raises(ValueError, match="sk_filter_taps.*" + word):
            _ffi.check(rc)
    torch.cuda.synchronize()
    assert bool((store == 0xA5).all())


def test_reference_names():
    shape = (2, 1, 6, 7, 20)
    vols = [FC.source("float", "float32", (6, 7, 20 + i))[:, :, :20] for i in range(2)]
    x = torch.from_numpy(np.stack(vols)[:, None].copy()).to(DEV)
    assert tuple(x.shape) == shape
    for fn, rank in ((M.median_filter, 13), (M.dilate, 26)):
        got = fn(x)
        assert tuple(got.shape) == shape and got.dtype == torch.float32
        for i in range(2):
            assert np.array_equal(got[i, 0].cpu().numpy(), FC.oracle_rank(np.ascontiguousarray(vols[i]), (1, 1, 1), rank, "zero"))
    got = M.binary_erosion(x)
    assert tuple(got.shape) == (1, 2, 6, 7, 20)
    for i in range(2):
        assert np.array_equal(got[0, i].cpu().numpy(), FC.oracle_rank(np.ascontiguousarray(vols[i]), (1, 1, 1), 0, "zero"))
    assert torch.equal(M.dilate(x), M.binary_dilation(x))          # the existing max filter agrees
    with pytest.raises(TypeError, match="float32"):
        M.median_filter(x.half())
    with pytest.raises(ValueError, match="B, C, X, Y, Z"):
        M.median_filter(x[0])


def test_two_runs_and_a_side_stream_give_the_same_bits():
    src = FC.to_torch(FC.source("salt", "uint16", (33, 35, 301))).to(DEV)
    first = filter_volume(src, "median", radius=(1, 1, 1)), filter_volume(src, "gauss", sigma=(1, 1, 0.5))
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        again = filter_volume(src, "median", radius=(1, 1, 1)), filter_volume(src, "gauss", sigma=(1, 1, 0.5))
    stream.synchronize()
    assert torch.equal(first[0].view(torch.int16), again[0].view(torch.int16))
    assert torch.equal(first[1].view(torch.int16), again[1].view(torch.int16))
