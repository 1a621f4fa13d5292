"""Shared cases of the filter tests (tests/test_filter_cpu.py, tests/test_hip_filter.py,
tests/test_hip_eval_denoise.py) and the oracle they are held against.  The oracle is written from the definition of
``sk_filter_rank`` and ``sk_filter_taps`` (include/skoots_hip.h), not from the kernel or the library's mirror: ``np.pad``
with ``constant`` / ``edge`` / ``symmetric``, the ``n`` shifted views stacked, then ``sort(axis=0)[rank]`` for ranks or
the int64 triple sum with ``(S + W // 2) // W`` for taps."""
import functools
import zlib

import numpy as np

BORDERS = ("zero", "edge", "mirror")
PAD_MODE = {"zero": "constant", "edge": "edge", "mirror": "symmetric"}
SCIPY_MODE = {"zero": "constant", "edge": "nearest", "mirror": "reflect"}


def window_size(radius):
    return (2 * radius[0] + 1) * (2 * radius[1] + 1) * (2 * radius[2] + 1)


def _views(a, radius, border):
    p = np.pad(a, [(r, r) for r in radius], mode=PAD_MODE[border])
    X, Y, Z = a.shape
    return [p[dx:dx + X, dy:dy + Y, dz:dz + Z] for dx in range(2 * radius[0] + 1) for dy in range(2 * radius[1] + 1)
            for dz in range(2 * radius[2] + 1)]


def oracle_rank(a, radius, rank, border):
    return np.ascontiguousarray(np.sort(np.stack(_views(a, radius, border)), axis=0)[rank])


def oracle_taps(a, taps, border):
    radius = [len(t) // 2 for t in taps]
    weights = [int(wx) * int(wy) * int(wz) for wx in taps[0] for wy in taps[1] for wz in taps[2]]
    S = np.zeros(a.shape, dtype=np.int64)
    for w, v in zip(weights, _views(a.astype(np.int64), radius, border)):
        S += w * v
    W = sum(taps[0]) * sum(taps[1]) * sum(taps[2])
    assert W * int(np.iinfo(a.dtype).max) < 2 ** 62
    return ((S + W // 2) // W).astype(a.dtype)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))     # the same volume in every process


@functools.lru_cache(maxsize=None)
def source(kind, dtype, shape):
    """``noise``: seeded samples over the full range of the dtype (uint16 reaches 32768 and above); ``two``: two values;
    ``const``: one; ``salt``: noise with every second z sample divided by 64; ``float``: float32 with negative values,
    both zeros and both infinities"""
    r = _rng("filter", kind, dtype, shape)
    if kind == "float":
        assert dtype == "float32"
        a = r.normal(0, 100, size=shape).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5], dtype=np.float32)
        pick = r.integers(0, 3 * special.size, size=shape)
        a = np.where(pick < special.size, special[np.minimum(pick, special.size - 1)], a).astype(np.float32)
    else:
        top = int(np.iinfo(dtype).max)
        if kind == "noise":
            a = r.integers(0, top + 1, size=shape)
        elif kind == "two":
            a = np.where(r.integers(0, 2, size=shape) == 1, top - 3, 7)
        elif kind == "const":
            a = np.full(shape, top - 1)
        else:
            assert kind == "salt"
            a = r.integers(0, top + 1, size=shape)
            a[:, :, 1::2] //= 64
        a = a.astype(dtype)
        assert kind != "noise" or dtype != "uint16" or a.size < 64 or a.max() >= 32768
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_rank(kind, dtype, shape, radius, rank, border):
    out = oracle_rank(source(kind, dtype, shape), radius, rank, border)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_taps(kind, dtype, shape, taps, border):
    out = oracle_taps(source(kind, dtype, shape), taps, border)
    out.setflags(write=False)
    return out


# the pinned lists of the issue: gaussian_taps(sigma) at total 256
GAUSS_1 = (1, 14, 62, 102, 62, 14, 1)
GAUSS_HALF = (27, 202, 27)
GAUSS_THIRD = (3, 250, 3)
GAUSS_2_LEN, GAUSS_2_MIDDLE = 13, (45, 50, 45)     # sigma = 2: 13 taps, the three in the middle
BOX3 = (1, 1, 1)
SPARSE_Z = (3, 0, 250, 0, 3)

TAP_SETS = ((BOX3, BOX3, BOX3),
            (GAUSS_1, GAUSS_HALF, (256,)),
            ((1,), (1,), SPARSE_Z),
            ((1,) * 17, (1,), GAUSS_THIRD))
RANK_RADII = ((1, 1, 1), (1, 1, 0), (2, 2, 1), (2, 2, 2), (0, 0, 2))
CPU_SHAPES = ((1, 1, 1), (2, 3, 5), (5, 7, 70))


def gauss_definition(sigma, radius=None, total=256):
    """The statement of ``gaussian_taps`` in the issue, written out once more for the tests"""
    import math
    if sigma == 0:
        return [total]
    r = radius if radius is not None else min(8, math.ceil(3 * sigma))
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    s = math.fsum(g)
    w = [int(math.floor(total * (v / s) + 0.5)) for v in g]
    w[r] = total - (sum(w) - w[r])
    while len(w) > 1 and w[0] == 0 and w[-1] == 0:
        w = w[1:-1]
    return w


def to_torch(a):
    """numpy -> torch, uint16 through its bit pattern"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.uint16)
    return torch.from_numpy(a.copy())


def to_numpy(t):
    import torch
    t = t.cpu().contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()
