"""Shared cases of the pooling tests (tests/test_pool_cpu.py, tests/test_hip_pool.py) and the numpy oracle they are held
against.  The oracle is written from the definitions of ``sk_pool_volume`` (include/skoots_hip.h), block by block, not
from the kernel: ``np.unique`` counts for ``mode``, Python integers for ``mean``."""
import functools
import zlib

import numpy as np

FACTORS = ((2, 2, 2), (2, 2, 1), (1, 1, 2), (2, 1, 1))
# clipped edges; z around the 16-byte vector of a lane (4 int32, 8 int16, 16 uint8) and around a wave; many rows
SMALL_SHAPES = ((5, 7, 9), (1, 1, 2), (2, 1, 1), (3, 4, 15), (3, 4, 16), (3, 4, 17), (2, 3, 33), (2, 2, 130), (4, 6, 1023))
BIG_SHAPE = (70, 66, 300)        # many workgroups, odd x blocks none, z tail for int16 / uint8
PLANTED_SHAPE = (8, 8, 40)       # tests/pool_cases.py: mode_volume plants its blocks here
MODE_DTYPES = ("int32", "int16", "uint8")
IMAGE_DTYPES = ("uint8", "uint16")


def oracle_pool(a, factors, how, sparse=False):
    fx, fy, fz = factors
    X, Y, Z = a.shape
    out = np.zeros((-(-X // fx), -(-Y // fy), -(-Z // fz)), dtype=a.dtype)
    for i, j, k in np.ndindex(*out.shape):
        block = a[i * fx:(i + 1) * fx, j * fy:(j + 1) * fy, k * fz:(k + 1) * fz].ravel()
        if how == "mode":
            values, counts = np.unique(block, return_counts=True)        # ascending in the dtype's order
            if sparse and (values != 0).any():
                values, counts = values[values != 0], counts[values != 0]
            out[i, j, k] = values[np.argmax(counts)]                     # the first of the largest: the smallest value
        elif how == "mean":
            out[i, j, k] = (int(block.astype(np.int64).sum()) + block.size // 2) // block.size
        else:
            out[i, j, k] = block.max()
    return out


def block_census(a, factors):
    """How many blocks of ``a`` have a tie for the largest count, a tie with zero among the tied values, and only
    distinct values (of blocks with more than one voxel)"""
    fx, fy, fz = factors
    X, Y, Z = a.shape
    tied = zero_tied = distinct = 0
    for i in range(-(-X // fx)):
        for j in range(-(-Y // fy)):
            for k in range(-(-Z // fz)):
                block = a[i * fx:(i + 1) * fx, j * fy:(j + 1) * fy, k * fz:(k + 1) * fz].ravel()
                values, counts = np.unique(block, return_counts=True)
                top = values[counts == counts.max()]
                tied += top.size > 1
                zero_tied += top.size > 1 and (top == 0).any()
                distinct += block.size > 1 and values.size == block.size
    return int(tied), int(zero_tied), int(distinct)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))     # the same volume in every process


def _three_ids(dtype):
    """0 and two ids, one at the dtype's end: ties between three values are common"""
    return {"int32": (0, 5, 2 ** 31 - 1), "int16": (0, -7, 9), "uint8": (0, 5, 255)}[dtype]


@functools.lru_cache(maxsize=None)
def mode_volume(dtype, shape):
    """Labels drawn from three ids; at PLANTED_SHAPE also the blocks a (2, 2, 2) pooling must decide by its rules:
    4 + 4 (with and without zero), 2 + 2 + 2 + 2, 8 distinct values, ids at both ends of the dtype."""
    r = _rng("mode", dtype, shape)
    a = r.choice(np.array(_three_ids(dtype), dtype=np.int64), size=shape).astype(dtype)
    if shape == PLANTED_SHAPE:
        info = np.iinfo(dtype)
        x, y, z = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
        a[0, 0:2, 0:8], a[1, 0:2, 0:8] = 3, 4                       # 4 + 4: the smaller value wins
        a[0, 0:2, 8:16], a[1, 0:2, 8:16] = 0, 4                     # 4 + 4 with zero: 0, or 4 when sparse
        a[2:4, 0:2, :] = (20 + 2 * (y % 2) + z % 2)[2:4, 0:2, :]    # 2 + 2 + 2 + 2
        a[4:6, 0:2, :] = (40 + 4 * (x % 2) + 2 * (y % 2) + z % 2)[4:6, 0:2, :]    # 8 distinct values
        ends = np.array([info.min, info.max, info.max - 1, 0], dtype=np.int64)
        a[6:8, :, :] = r.choice(ends, size=(2,) + shape[1:]).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def image_volume(dtype, shape):
    """Per 2 x 2 x 2 cell one of: random samples over the whole range, the largest sample everywhere (the largest
    sum), and v / v + 1 in a checkerboard (every even block's mean ends in .5)"""
    r = _rng("image", dtype, shape)
    top = np.iinfo(dtype).max
    x, y, z = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    cells = r.integers(0, 3, size=tuple(-(-n // 2) for n in shape))
    kind = cells[x // 2, y // 2, z // 2]
    a = r.integers(0, top + 1, size=shape)
    a = np.where(kind == 1, top, a)
    a = np.where(kind == 2, 100 + ((x + y + z) & 1), a).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def binary_volume(dtype, shape):
    """A sparse skeleton-like volume: mostly 0, some 1, a few of the dtype's largest value"""
    r = _rng("binary", dtype, shape)
    a = r.choice(np.array([0, 0, 0, 0, 0, 1, np.iinfo(dtype).max], dtype=np.int64), size=shape).astype(dtype)
    a.setflags(write=False)
    return a


def source(how, dtype, shape):
    return {"mode": mode_volume, "mean": image_volume, "max": binary_volume}[how](dtype, tuple(shape))


@functools.lru_cache(maxsize=None)
def expected(how, dtype, shape, factors, sparse=False):
    """The oracle's result for ``source(how, dtype, shape)``, computed once and shared"""
    out = oracle_pool(source(how, dtype, shape), factors, how, sparse)
    out.setflags(write=False)
    return out


def small_cases():
    """(how, dtype, shape, factors, sparse) of every reduction, dtype, small extent and factor set"""
    out = []
    for shape in SMALL_SHAPES + (PLANTED_SHAPE,):
        for f in FACTORS:
            for dt in MODE_DTYPES:
                out += [("mode", dt, shape, f, False), ("mode", dt, shape, f, True)]
            for dt in IMAGE_DTYPES:
                out += [("mean", dt, shape, f, False), ("max", dt, shape, f, False)]
    return out


BIG_CASES = (("mode", "int32", BIG_SHAPE, (2, 2, 2), False), ("mean", "uint8", BIG_SHAPE, (2, 2, 2), False),
             ("max", "uint16", BIG_SHAPE, (2, 2, 1), False), ("mode", "uint8", BIG_SHAPE, (2, 2, 2), True))


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
