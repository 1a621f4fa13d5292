"""``sk_tile_histograms`` and ``sk_apply_tile_luts`` (skoots_amd/csrc/equalize.hip) on the device against the integer
oracle of tests/equalize_cases.py: z extents around a lane's 16-byte window, bases one element off, every class of tile
(a few voxels, clipped blocks, planes, the whole volume, larger than the volume), every legal table size, tables of
arbitrary values, both sum widths, one counter far past 16 bits, the C ABI's refusals.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import equalize_cases as EC

from skoots_amd import _ffi
from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import apply_tile_luts, equalize, equalize_path, tile_histograms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILES = ((1, 1, 1), (3, 5, 7), (8, 8, 16), (4, 4, 128), "slices", None, (40, 40, 200), (6, 4, 5))
SHAPES = {1: (21, 13, 1), 15: (9, 6, 15), 16: (21, 5, 16), 17: (13, 10, 17), 70: (7, 21, 70), 130: (17, 9, 130)}
U16_BINS = ((256, 0), (256, 4), (1024, 4), (4096, 0), (4096, 4))          # (bins, shift)


def _unaligned(a):
    """the volume one element into its storage: a contiguous tensor whose rows start off any 16-byte boundary"""
    t = EC.to_torch(a).to(DEV)
    store = torch.zeros(a.size + 1, dtype=t.dtype, device=DEV)
    view = store[1:].view(*a.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == a.dtype.itemsize
    return view


def _combos(dtype, tile, shape):
    if dtype == "uint8":
        return ((256, 0),)
    tiles = int(np.prod(EC.grid_of(shape, tile)))
    return tuple(c for c in U16_BINS if tiles * c[0] <= 2 ** 23)       # the table of a (1, 1, 1) tiling stays small


def _kind(dtype, bins, shift):
    return "noise12" if dtype == "uint16" and shift == 0 else "noise"


@pytest.mark.parametrize("z", sorted(SHAPES))
@pytest.mark.parametrize("dtype", ("uint8", "uint16"))
def test_histograms(dtype, z):
    shape = SHAPES[z]
    for tile in TILES:
        for bins, shift in _combos(dtype, tile, shape):
            kind = _kind(dtype, bins, shift)
            a = EC.source(kind, dtype, shape)
            want = EC.expected_histograms(kind, dtype, shape, tile, bins, shift)
            for src in (EC.to_torch(a).to(DEV), _unaligned(a)):
                got = tile_histograms(src, tile, bins, shift)
                assert got.dtype == torch.int64 and got.device == src.device and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy(), want), (tile, bins, shift)


@pytest.mark.parametrize("z", sorted(SHAPES))
@pytest.mark.parametrize("dtype", ("uint8", "uint16"))
def test_apply_arbitrary_tables(dtype, z):
    shape = SHAPES[z]
    for tile in TILES:
        grid = EC.grid_of(shape, tile)
        for bins, shift in _combos(dtype, tile, shape):
            a = EC.source(_kind(dtype, bins, shift), dtype, shape)
            luts = EC.random_luts(dtype, grid, bins)
            dev_luts = torch.from_numpy(luts.copy()).to(DEV)
            for interpolate in (True, False):
                want = EC.oracle_apply(a, luts, tile, shift, interpolate)
                aligned = EC.to_torch(a).to(DEV)
                off = _unaligned(a)
                off_out = torch.zeros(a.size + 1, dtype=off.dtype, device=DEV)[1:].view(*shape)
                for src, out in ((aligned, None), (off, None), (off, off_out)):     # vector rows, scalar loads, both off
                    got = apply_tile_luts(src, dev_luts, tile, shift, interpolate, out=out)
                    assert got.dtype == src.dtype and tuple(got.shape) == shape
                    assert np.array_equal(EC.to_numpy(got), want), (tile, bins, shift, interpolate)


WIDE = (((21, 40, 130), (16, 16, 64), "lds/xy+interp/acc64"), ((7, 11, 1100), (3, 5, 550), "gather/xy+interp/acc64"),
        ((21, 40, 130), (16, 0, 0), "lds/xy+one/acc32"), ((21, 40, 130), (0, 0, 64), "lds/-+interp/acc32"),
        ((21, 40, 130), (16, 16, 1), "lds/xy+tile/acc32"))


def test_sums_in_64_bits_and_many_workgroups():
    """uint16 under tiles whose weights times 65535 pass 2^32, staged and gathered; several shares of rows per cell"""
    for shape, tile, path in WIDE:
        a = EC.source("noise", "uint16", shape)
        assert equalize_path(torch.uint16, shape, tile, 256, 8)[1] == path
        luts = EC.random_luts("uint16", EC.grid_of(shape, tile), 256)
        got = apply_tile_luts(EC.to_torch(a).to(DEV), torch.from_numpy(luts.copy()).to(DEV), tile, 8, True)
        assert np.array_equal(EC.to_numpy(got), EC.oracle_apply(a, luts, tile, 8, True)), tile
        got = tile_histograms(EC.to_torch(a).to(DEV), tile, 256, 8)
        assert np.array_equal(got.cpu().numpy(), EC.oracle_histograms(a, tile, 256, 8)), tile


def test_rounding_at_exact_halves():
    """voxels at which S + W // 2 is a multiple of W: the half goes up"""
    for shape, tile, at in (((4, 1, 1), (2, 0, 0), (1, 0, 0)),        # gathered: weights (3, 1) of 4
                            ((8, 8, 3), (4, 4, 0), (2, 0, 1))):       # staged: weights (7, 1) of 8 along x, y in the first cell
        a = np.zeros(shape, dtype=np.uint8)
        grid = EC.grid_of(shape, tile)
        luts = np.zeros(grid + (256,), dtype=np.int32)
        luts[1, 0, 0, :] = 2 if tile[0] == 2 else 4
        want = EC.oracle_apply(a, luts, tile, 0, True)
        W = 8 * int(np.prod(EC.sides_of(shape, tile)))
        S = (2 if tile[0] == 2 else 4) * W // (4 if tile[0] == 2 else 8)       # one part in 4 (or 8) of the second tile
        assert (S + W // 2) % W == 0 and want[at] == 1
        got = apply_tile_luts(torch.from_numpy(a).to(DEV), torch.from_numpy(luts).to(DEV), tile)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", ("uint8", "uint16"))
def test_one_counter_past_sixteen_bits(dtype):
    shape = (64, 64, 130)
    a = EC.source("const", dtype, shape)
    src = EC.to_torch(a).to(DEV)
    bins = 256 if dtype == "uint8" else 1024
    shift = 0 if dtype == "uint8" else 6
    b = int(a.flat[0]) >> shift
    one = tile_histograms(src, None, bins, shift).cpu().numpy()
    assert one.shape == (1, 1, 1, bins) and one[0, 0, 0, b] == 532480 and one.sum() == 532480
    planes = tile_histograms(src, "slices", bins, shift).cpu().numpy()
    assert planes.shape == (1, 1, 130, bins) and (planes[0, 0, :, b] == 4096).all() and planes.sum() == 532480
    blocks = tile_histograms(src, (32, 32, 16), bins, shift).cpu().numpy()
    assert np.array_equal(blocks, EC.oracle_histograms(a, (32, 32, 16), bins, shift))


@pytest.mark.parametrize("how", M.EQUALIZE_HOW)
def test_equalize_on_the_device_equals_the_cpu_path_and_the_oracle(how):
    for dtype, kind, shape in (("uint8", "ramp", (21, 13, 70)), ("uint16", "ramp", (13, 10, 21)), ("uint16", "noise12", (9, 6, 15))):
        a = EC.source(kind, dtype, shape)
        for tile in ((8, 8, 16), "slices", None, (3, 5, 7)):
            for interpolate in (True, False):
                dev = equalize(EC.to_torch(a).to(DEV), how, tile=tile, interpolate=interpolate)
                cpu = equalize(EC.to_torch(a), how, tile=tile, interpolate=interpolate)
                assert dev.device.type == "cuda" and dev.dtype == cpu.dtype
                assert np.array_equal(EC.to_numpy(dev), EC.to_numpy(cpu)), (dtype, tile, interpolate)
                assert np.array_equal(EC.to_numpy(dev), EC.oracle_equalize(a, how, tile=tile, interpolate=interpolate))
    a = EC.source("ramp", "uint16", (13, 10, 21))
    target = EC.source("noise", "uint16", (9, 6, 15))
    if how == "match":
        dev = equalize(EC.to_torch(a).to(DEV).unsqueeze(0), how, tile=(5, 3, 8), bins=4096, target=EC.to_torch(target).to(DEV))
        assert tuple(dev.shape) == (1, 13, 10, 21)
        assert np.array_equal(EC.to_numpy(dev[0]), EC.oracle_equalize(a, how, tile=(5, 3, 8), bins=4096, target=target))


def test_two_runs_give_the_same_bits():
    a = EC.source("two", "uint8", (64, 64, 130))
    src = EC.to_torch(a).to(DEV)
    for tile in (None, "slices", (8, 8, 16), (3, 5, 7)):
        first = tile_histograms(src, tile)
        assert torch.equal(first, tile_histograms(src, tile))
        assert np.array_equal(first.cpu().numpy(), EC.oracle_histograms(a, tile, 256, 0))
        assert torch.equal(equalize(src, "equalize", tile=tile), equalize(src, "equalize", tile=tile))


def test_paths_named_for_each_geometry():
    u8, u16 = torch.uint8, torch.uint16
    cases = ((u8, (17, 9, 130), None, 256, True, ("one", "lds/-+one/lookup")),
             (u8, (17, 9, 130), "slices", 256, True, ("planes", "lds/-+tile/lookup")),
             (u8, (17, 9, 130), (1, 1, 1), 256, True, ("global", "gather/-+tile/lookup")),
             (u8, (17, 9, 130), (3, 5, 7), 256, True, ("global", "gather/xy+interp/acc32")),
             (u8, (17, 9, 130), (3, 5, 7), 256, False, ("global", "gather/-+tile/lookup")),
             (u8, (17, 9, 130), (8, 8, 16), 256, True, ("ztiles", "lds/xy+interp/acc32")),
             (u8, (17, 9, 130), (8, 8, 16), 256, False, ("ztiles", "lds/-+tile/lookup")),
             (u8, (17, 9, 130), (4, 4, 128), 256, True, ("ztiles", "lds/xy+interp/acc32")),
             (u8, (21, 5, 16), (8, 8, 16), 256, True, ("one", "lds/xy+one/acc32")),
             (u8, (17, 9, 130), (40, 40, 200), 256, True, ("one", "lds/-+one/lookup")),
             (u8, (17, 9, 130), (6, 4, 5), 256, True, ("ztiles", "lds/xy+interp/acc32")),
             (u16, (17, 9, 130), (8, 8, 16), 4096, True, ("ztiles", "lds/xy+interp/acc32")),
             (u16, (17, 9, 130), "slices", 4096, True, ("planes", "lds/-+tile/lookup")),
             (u16, (21, 40, 130), (16, 16, 64), 256, True, ("ztiles", "lds/xy+interp/acc64")))
    for dtype, shape, tile, bins, interpolate, want in cases:
        assert equalize_path(dtype, shape, tile, bins, 0, interpolate) == want, (shape, tile, bins, interpolate)


def test_c_abi_refuses_by_name_and_launches_nothing():
    shape = (5, 7, 37)
    a = EC.source("noise", "uint8", shape)
    stream = _ffi.stream_ptr(torch.device(DEV))
    src = EC.to_torch(a).to(DEV)
    n_out, pad = a.size, 256
    store = torch.full((pad + n_out + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = store[pad:pad + n_out]
    luts = torch.from_numpy(EC.random_luts("uint8", (2, 2, 3), 256).copy()).to(DEV)
    counts = torch.full((2 * 2 * 3 * 256 + 2,), -7, dtype=torch.int64, device=DEV)
    table = counts[1:-1]
    tile = (3, 4, 16)

    def hist(s, code, ext, t, bins, shift, out):
        return _ffi.lib.sk_tile_histograms(_ffi.ptr(s), code, *ext, *t, bins, shift, _ffi.ptr(out), stream)

    def apply(s, d, code, ext, t, lut, bins, shift, interpolate):
        return _ffi.lib.sk_apply_tile_luts(_ffi.ptr(s), _ffi.ptr(d), code, *ext, *t, _ffi.ptr(lut), bins, shift, interpolate, stream)

    _ffi.check(hist(src, 4, shape, tile, 256, 0, table))
    _ffi.check(apply(src, dst, 4, shape, tile, luts, 256, 0, 1))
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().reshape(2, 2, 3, 256), EC.oracle_histograms(a, tile, 256, 0))
    assert int(counts[0]) == -7 and int(counts[-1]) == -7
    assert np.array_equal(dst.cpu().numpy().reshape(shape), EC.oracle_apply(a, luts.cpu().numpy(), tile, 0, True))
    assert bool((store[:pad] == 0xA5).all()) and bool((store[pad + n_out:] == 0xA5).all())

    store.fill_(0xA5)
    counts.fill_(-7)
    torch.cuda.synchronize()
    words = torch.zeros(64, dtype=torch.int16, device=DEV)
    bad_hist = ((None, 4, shape, tile, 256, 0, table, "NULL"),
                (src, 4, shape, tile, 256, 0, None, "NULL"),
                (src, 1, shape, tile, 256, 0, table, "dtype"),
                (src, 4, (5, 0, 37), tile, 256, 0, table, "extents"),
                (src, 4, (5, 7, 2 ** 30 + 1), tile, 256, 0, table, "2\\^30"),
                (src, 4, shape, (3, -1, 16), 256, 0, table, "tile"),
                (src, 4, shape, tile, 1024, 0, table, "uint8 takes bins = 256"),
                (src, 4, shape, tile, 256, 1, table, "uint8 takes bins = 256 and shift = 0"),
                (src, 5, shape, tile, 512, 0, table, "bins = 512"),
                (src, 5, shape, tile, 1024, 9, table, "shift = 9"),
                (words.view(torch.uint8)[1:], 5, (1, 1, 8), tile, 256, 0, table, "not aligned to its elements"),
                (src, 4, shape, tile, 256, 0, counts.view(torch.int32)[1:], "8-byte aligned"))
    for *args, word in bad_hist:
        rc = hist(*args)
        assert rc == -1, (args[1:6], word)
        with pytest.raises(ValueError, match="sk_tile_histograms.*" + word):
            _ffi.check(rc)
    bad_apply = ((src, src, 4, shape, tile, luts, 256, 0, 1, "in == out"),
                 (None, dst, 4, shape, tile, luts, 256, 0, 1, "NULL"),
                 (src, None, 4, shape, tile, luts, 256, 0, 1, "NULL"),
                 (src, dst, 4, shape, tile, None, 256, 0, 1, "NULL"),
                 (src, dst, 0, shape, tile, luts, 256, 0, 1, "dtype"),
                 (src, dst, 4, (0, 7, 37), tile, luts, 256, 0, 1, "extents"),
                 (src, dst, 4, shape, (-2, 4, 16), luts, 256, 0, 1, "tile"),
                 (src, dst, 4, shape, tile, luts, 4096, 0, 1, "uint8 takes bins = 256"),
                 (src, dst, 5, shape, tile, luts, 256, -1, 1, "shift = -1"),
                 (src, dst, 4, shape, tile, luts, 256, 0, 2, "interpolate = 2"),
                 (src, dst, 4, shape, tile, luts.view(torch.int16).reshape(-1)[1:], 256, 0, 1, "4-byte aligned"),
                 (src, words.view(torch.uint8)[1:], 5, (1, 1, 8), tile, luts, 256, 0, 1, "not aligned to its elements"))
    for *args, word in bad_apply:
        rc = apply(*args)
        assert rc == -1, (args[2:5], word)
        with pytest.raises(ValueError, match="sk_apply_tile_luts.*" + word):
            _ffi.check(rc)
    torch.cuda.synchronize()
    assert bool((store == 0xA5).all()) and bool((counts == -7).all())


def test_the_cases_reach_every_named_path():
    """the geometries test_histograms, test_apply_arbitrary_tables and test_sums_in_64_bits_and_many_workgroups run reach
    every histogram kernel, both apply kernels, every way z picks its table and every sum width"""
    hist, applied = set(), set()
    for dtype in ("uint8", "uint16"):
        for shape in SHAPES.values():
            for tile in TILES:
                for bins, shift in _combos(dtype, tile, shape):
                    for interpolate in (True, False):
                        h, a = equalize_path(getattr(torch, dtype), shape, tile, bins, shift, interpolate)
                        hist.add(h)
                        applied.add(a)
    applied.update(path for _, _, path in WIDE)
    assert hist == set(M.EQUALIZE_HIST_PATHS)
    kernels, modes, widths = (set(p.split("/")[k] for p in applied) for k in range(3))
    assert kernels == {"lds", "gather"}
    assert modes == {"-+one", "-+tile", "-+interp", "xy+one", "xy+tile", "xy+interp"}
    assert widths == {"lookup", "acc32", "acc64"}
