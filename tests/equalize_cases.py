"""Shared cases of the equalize tests (tests/test_equalize_cpu.py, tests/test_hip_equalize.py,
tests/test_hip_eval_equalize.py) and the oracle they are held against.  The oracle is written from the definitions of
``sk_tile_histograms`` and ``sk_apply_tile_luts`` (include/skoots_hip.h) and of the table builders, not from the kernels
or the library's mirror: ``np.add.at`` per tile for the histograms, the eight-corner sum with broadcast per-axis weights
in Python integers' range (int64, asserted) for the apply pass, a Python loop per tile and per bin for the builders."""
import functools
import math
import zlib

import numpy as np

from tests.filter_cases import to_numpy, to_torch  # noqa: F401  (uint16 through its bit pattern)

BINS = {"uint8": (256,), "uint16": (256, 1024, 4096)}


def sides_of(shape, tile):
    if tile is None:
        tile = (0, 0, 0)
    if tile == "slices":
        tile = (0, 0, 1)
    return tuple(n if t == 0 or t > n else t for t, n in zip(tile, shape))


def grid_of(shape, tile):
    return tuple(-(-n // t) for n, t in zip(shape, sides_of(shape, tile)))


def bin_of(a, bins, shift):
    return np.minimum(a.astype(np.int64) >> shift, bins - 1)


def shift_of(vmax, bins):
    s = 0
    while (vmax >> s) >= bins:
        s += 1
    return s


def oracle_histograms(a, tile, bins, shift):
    t, n = sides_of(a.shape, tile), grid_of(a.shape, tile)
    out = np.zeros(n + (bins,), dtype=np.int64)
    b = bin_of(a, bins, shift)
    for kx in range(n[0]):
        for ky in range(n[1]):
            for kz in range(n[2]):
                part = b[kx * t[0]:(kx + 1) * t[0], ky * t[1]:(ky + 1) * t[1], kz * t[2]:(kz + 1) * t[2]]
                np.add.at(out[kx, ky, kz], part.ravel(), 1)
    return out


def _axis(n, t, count):
    """the two tiles and the two weights of every index of an axis, from the definition, index by index"""
    k0, k1, w0, w1 = [], [], [], []
    for i in range(n):
        p = 2 * i + 1 - t
        k = p // (2 * t)                # Python's floor division
        b = p - 2 * t * k
        k0.append(min(max(k, 0), count - 1))
        k1.append(min(max(k + 1, 0), count - 1))
        w0.append(2 * t - b)
        w1.append(b)
    return [np.array(v, dtype=np.int64) for v in (k0, k1, w0, w1)]


def oracle_apply(a, luts, tile, shift, interpolate):
    t, n = sides_of(a.shape, tile), grid_of(a.shape, tile)
    bins = luts.shape[-1]
    assert luts.shape[:3] == n
    b = bin_of(a, bins, shift)
    luts = luts.astype(np.int64)
    X, Y, Z = a.shape
    if not interpolate:
        kx, ky, kz = (np.arange(m) // s for m, s in zip(a.shape, t))
        return luts[kx[:, None, None], ky[None, :, None], kz[None, None, :], b].astype(a.dtype)
    W = 8 * t[0] * t[1] * t[2]
    assert W * 65535 < 2 ** 62
    ax = [_axis(m, s, c) for m, s, c in zip(a.shape, t, n)]
    S = np.zeros(a.shape, dtype=np.int64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = ax[0][2 + cx].reshape(X, 1, 1) * ax[1][2 + cy].reshape(1, Y, 1) * ax[2][2 + cz].reshape(1, 1, Z)
                S += w * luts[ax[0][cx].reshape(X, 1, 1), ax[1][cy].reshape(1, Y, 1), ax[2][cz].reshape(1, 1, Z), b]
    return ((S + W // 2) // W).astype(a.dtype)


# ---- the builders, one histogram at a time in Python integers ----

def _first_reaching(H, k):
    for b, v in enumerate(H):
        if v >= k:
            return b
    raise AssertionError("the cumulative sum never reaches k")


def stretch_bounds_one(h, low, high):
    h = [int(v) for v in h]
    n = sum(h)
    H = np.cumsum(h).tolist()
    ks = [min(max(int(math.ceil(q / 100 * n)), 1), n) for q in (low, high)]
    return _first_reaching(H, ks[0]), _first_reaching(H, ks[1])


def stretch_lut_one(h, low, high, top, shift):
    lo, hi = stretch_bounds_one(h, low, high)
    if hi == lo:
        return [min(b << shift, top) for b in range(len(h))]
    return [min(max(((b - lo) * top + (hi - lo) // 2) // (hi - lo), 0), top) for b in range(len(h))]


def clipped_one(h, clip):
    h = [int(v) for v in h]
    n, bins = sum(h), len(h)
    if clip is None:
        return h
    c = max(1, int(math.ceil(clip * n / bins)))
    E = sum(max(v - c, 0) for v in h)
    q, r = divmod(E, bins)
    return [min(v, c) + q + (1 if b < r else 0) for b, v in enumerate(h)]


def equalize_lut_one(h, clip, top):
    n = int(sum(int(v) for v in h))
    H = np.cumsum(clipped_one(h, clip)).tolist()
    return [(v * top + n // 2) // n for v in H]


def match_lut_one(h, g, shift, top):
    h, g = [int(v) for v in h], [int(v) for v in g]
    n, m = sum(h), sum(g)
    H, G = np.cumsum(h).tolist(), np.cumsum(g).tolist()
    out, t = [], 0
    for b in range(len(h)):             # H never falls, so t never goes back
        while G[t] * n < H[b] * m:
            t += 1
        out.append(min(t << shift, top))
    return out


def per_tile(fn, h, *args):
    flat = h.reshape(-1, h.shape[-1])
    return np.array([fn(row, *args) for row in flat], dtype=np.int32).reshape(h.shape)


def oracle_equalize(a, how, tile=None, bins=None, low=0.5, high=99.5, clip=3.0, target=None, top=None, interpolate=True):
    """``equalize`` from the definitions: histograms, the builder per tile, the apply pass"""
    bins = bins or (256 if a.dtype == np.uint8 else 1024)
    top = top or int(np.iinfo(a.dtype).max)
    vmax = int(a.max())
    if how == "match" and isinstance(target, np.ndarray) and target.ndim == 3:
        vmax = max(vmax, int(target.max()))
    shift = 0 if a.dtype == np.uint8 else shift_of(vmax, bins)
    h = oracle_histograms(a, tile, bins, shift)
    if how == "stretch":
        luts = per_tile(stretch_lut_one, h, low, high, top, shift)
    elif how == "equalize":
        luts = per_tile(equalize_lut_one, h, clip, top)
    else:
        if target is None:
            g = oracle_histograms(a, None, bins, shift)[0, 0, 0]
        elif target.ndim == 3:
            g = oracle_histograms(target, None, bins, shift)[0, 0, 0]
        else:
            g = target
        luts = per_tile(match_lut_one, h, g, shift, top)
    return oracle_apply(a, luts, tile, shift, interpolate)


# ---- sources ----

def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))     # the same volume in every process


@functools.lru_cache(maxsize=None)
def source(kind, dtype, shape):
    """``noise``: seeded samples over the full range (uint16 reaches 32768 and above); ``noise12``: uint16 in 0 .. 4095;
    ``two``: two values; ``const``: one; ``ramp``: noise plus a gradient along z, so that tiles differ; ``flicker``: one
    pattern of pairwise different samples whose planes are multiplied and offset by a factor per plane"""
    r = _rng("equalize", kind, dtype, shape)
    top = int(np.iinfo(dtype).max)
    X, Y, Z = shape
    if kind == "noise":
        a = r.integers(0, top + 1, size=shape)
    elif kind == "noise12":
        assert dtype == "uint16"
        a = r.integers(0, 4096, size=shape)
    elif kind == "two":
        a = np.where(r.integers(0, 2, size=shape) == 1, top - 3, 7)
    elif kind == "const":
        a = np.full(shape, top - 1)
    elif kind == "ramp":
        a = r.integers(0, top // 4 + 1, size=shape) + (np.arange(Z) * (top // 2) // max(Z - 1, 1))[None, None, :]
    else:
        # every plane is the same pattern of pairwise different samples, multiplied and offset by its own factors: the
        # gain is at least 1 (times 256 for uint16, more than a bin at any shift), so the samples of a plane fall into
        # pairwise different bins; with an even number of them exactly half lie at or below the plane's median
        assert kind == "flicker" and X * Y <= 130 and X * Y % 2 == 0
        step = 1 if dtype == "uint8" else 256
        base = (r.permutation(X * Y).reshape(X, Y, 1) * step).astype(np.float64)
        gain = r.uniform(1.0, 1.75, size=Z)[None, None, :]
        offset = r.integers(0, 25 * step, size=Z)[None, None, :]
        a = np.floor(base * gain).astype(np.int64) + offset
        assert a.max() <= top
    a = a.astype(dtype)
    assert kind != "noise" or dtype != "uint16" or a.size < 64 or a.max() >= 32768
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_histograms(kind, dtype, shape, tile, bins, shift):
    out = oracle_histograms(source(kind, dtype, shape), tile, bins, shift)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_luts(dtype, grid, bins, seed=0):
    """tables of arbitrary values in 0 .. top: not monotone, nothing a builder would give"""
    top = int(np.iinfo(dtype).max)
    out = _rng("luts", dtype, grid, bins, seed).integers(0, top + 1, size=tuple(grid) + (bins,)).astype(np.int32)
    out.setflags(write=False)
    return out


CPU_SHAPES = ((1, 1, 1), (2, 3, 5), (13, 10, 21))
CPU_TILES = ((1, 1, 1), (4, 4, 4), (5, 3, 8), "slices", None, (20, 20, 40))
