"""Shared cases of the resampling tests (tests/test_resample_cpu.py, tests/test_hip_resample.py,
tests/test_hip_eval_rescale.py) and the oracle they are held against.  The oracle is written from the definition of
``sk_resample_volume`` (include/skoots_hip.h), not from the kernel or the library's mirror: the tap list of every output
index in plain Python integers with the UNREDUCED weights, one weight matrix per axis, the three contractions in integers
(int64 where the largest sum fits, Python integers otherwise) and ``floor((2 S + W) / (2 W))``."""
import functools
import math
import zlib

import numpy as np

OPS = ("nearest", "linear", "area")


def taps(n, m, op, i):
    """[(k, w), ...] and W of output index i, as the definition states them"""
    if op == "nearest":
        return [(((2 * i + 1) * n) // (2 * m), 1)], 1
    if op == "linear":
        num, den = (2 * i + 1) * n - m, 2 * m
        k0 = num // den                                   # Python's // floors
        r = num - k0 * den
        clamp = lambda k: min(max(k, 0), n - 1)
        return [(clamp(k0), den - r), (clamp(k0 + 1), r)], den
    assert op == "area"
    out = []
    for k in range((i * n) // m, -(-((i + 1) * n) // m)):
        out.append((k, min((k + 1) * m, (i + 1) * n) - max(k * m, i * n)))
    return out, n


def axis_matrix(n, m, op, reduce=False):
    """(m, n) weights as Python integers in an object array, and W; ``reduce`` divides by the gcd of all weights"""
    M = np.zeros((m, n), dtype=object)
    W = 1
    for i in range(m):
        tl, W = taps(n, m, op, i)
        assert sum(w for _, w in tl) == W and all(0 <= k < n and w >= 0 for k, w in tl)
        for k, w in tl:
            M[i, k] += w
    if reduce:
        g = functools.reduce(math.gcd, [int(w) for w in M.ravel() if w] + [W])
        M, W = M // g, W // g
    return M, W


def operators(src_shape, dst_shape, how):
    if how == "auto":
        return tuple("linear" if m >= n else "area" for n, m in zip(src_shape, dst_shape))
    return (how,) * 3


def oracle_resample(a, shape, how="auto", reduce=False):
    ops = how if isinstance(how, tuple) else operators(a.shape, shape, how)
    top = max(abs(int(np.iinfo(a.dtype).max)), abs(int(np.iinfo(a.dtype).min)))
    mats = [axis_matrix(n, m, op, reduce) for n, m, op in zip(a.shape, shape, ops)]
    W = mats[0][1] * mats[1][1] * mats[2][1]
    wide = (2 * top + 1) * W >= 2 ** 63                     # the largest 2 S + W
    kind = object if wide else np.int64
    s = a.astype(kind)
    for axis, (M, _) in enumerate(mats):
        s = np.moveaxis(np.tensordot(M.astype(kind), s, axes=([1], [axis])), 0, axis)
    out = (2 * s + W) // (2 * W)                             # floors for negative sums too (labels: W = 1)
    return np.ascontiguousarray(out.astype(a.dtype))


def output_shape(shape, factors):
    return tuple(max(1, int(math.floor(n * f + 0.5))) for n, f in zip(shape, factors))


def centre_on_boundary(n, m):
    """the integer form of 'an output centre lies on a source voxel boundary'"""
    return any(((2 * i + 1) * n) % (2 * m) == 0 for i in range(m))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))     # the same volume in every process


@functools.lru_cache(maxsize=None)
def image_volume(dtype, shape):
    """Per 2 x 2 x 2 cell one of: random samples over the whole range, the largest sample everywhere (the largest
    sums), and v / v + 1 in a checkerboard (exact halves)"""
    r = _rng("resample-image", dtype, shape)
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
def label_volume(dtype, shape):
    """Ids from a small set that holds both ends of the dtype, in runs of a few voxels along z"""
    r = _rng("resample-label", dtype, shape)
    info = np.iinfo(dtype)
    ids = np.array([0, 1, 5, info.max, info.max - 1, info.min, 7, 0], dtype=np.int64)
    a = ids[r.integers(0, ids.size, size=shape)].astype(dtype)
    a.setflags(write=False)
    return a


def source(how, dtype, shape):
    return (label_volume if dtype in ("int32", "int16") else image_volume)(dtype, tuple(shape))


@functools.lru_cache(maxsize=None)
def expected(how, dtype, shape, out_shape):
    out = oracle_resample(source(how, dtype, shape), tuple(out_shape), how)
    out.setflags(write=False)
    return out


def z_targets(z):
    """m_z of a source extent z: the same, 2x, 3/2, 1/2, 2/3, 8x and 1/8"""
    return sorted({z, 2 * z, 3 * z // 2, z // 2, 2 * z // 3, 8 * z, -(-z // 8)})


Z_EXTENTS = (15, 16, 17, 33, 130, 1023)      # around a lane's 16 bytes (16 uint8, 8 uint16, 4 int32) and around a wave
IMAGE_DTYPES = ("uint8", "uint16")
LABEL_DTYPES = ("int32", "int16", "uint8", "uint16")


def z_cases():
    """(how, dtype, shape, out_shape): source (3, 4, z), x and y kept, every z target; dtypes and operators rotate so
    that every pair occurs at every z"""
    out = []
    for z in Z_EXTENTS:
        for j, mz in enumerate(z_targets(z)):
            dts = IMAGE_DTYPES if z != 1023 else (IMAGE_DTYPES[j % 2],)
            for dt in dts:
                out.append(("auto", dt, (3, 4, z), (3, 4, mz)))
            out.append((("linear", "area")[j % 2], IMAGE_DTYPES[(j + 1) % 2], (3, 4, z), (3, 4, mz)))
            out.append(("nearest", LABEL_DTYPES[j % 4], (3, 4, z), (3, 4, mz)))
    return out


# extents of 1 on every axis (n = 1 and m = 1), at both ends of the ratio limit
UNIT_CASES = tuple((how, dt, src, dst) for how, dt in (("auto", "uint8"), ("linear", "uint16"), ("area", "uint8"),
                                                       ("nearest", "int32"))
                   for src, dst in (((1, 5, 9), (8, 5, 9)), ((8, 5, 9), (1, 5, 9)), ((5, 1, 9), (5, 8, 9)),
                                    ((5, 8, 9), (5, 1, 9)), ((5, 6, 1), (5, 6, 8)), ((5, 6, 8), (5, 6, 1)),
                                    ((1, 1, 1), (8, 8, 8)), ((8, 8, 8), (1, 1, 1)), ((1, 1, 1), (1, 1, 1))))
MIXED_CASES = tuple(("auto", dt, (6, 9, 40), dst) for dt in IMAGE_DTYPES for dst in ((9, 6, 60), (3, 18, 13)))
DTYPE_CASES = tuple((how, dt, (5, 7, 24), (7, 5, 36)) for how in ("linear", "area", "auto") for dt in IMAGE_DTYPES) + \
    tuple(("nearest", dt, (5, 7, 24), (7, 5, 36)) for dt in LABEL_DTYPES)
ODD_ROW_CASES = (("auto", "uint8", (4, 5, 21), (6, 4, 31)), ("linear", "uint16", (4, 5, 21), (4, 5, 33)),
                 ("area", "uint8", (4, 5, 30), (4, 5, 13)), ("nearest", "int16", (4, 5, 21), (4, 5, 37)),
                 ("nearest", "uint8", (4, 5, 23), (4, 5, 23)))
BIG_SHAPE, BIG_OUT = (70, 66, 300), (105, 44, 450)
BIG_CASES = (("auto", "uint8", BIG_SHAPE, BIG_OUT), ("auto", "uint16", BIG_SHAPE, BIG_OUT),
             ("nearest", "int32", BIG_SHAPE, BIG_OUT))

# Accumulator width: 32 bits where the reduced W times the dtype's largest value stays below 2^32.  Linear n -> m has the
# reduced W = 2 m / gcd(2 m, 2 n, |n - m|): 31 -> 32 gives 64, 7 -> 8 gives 16, 15 -> 17 gives 17, 127 -> 128 gives 256,
# 128 -> 129 gives 258.
#   uint16: 64 * 64 * 16 = 65536,    65536 * 65535 = 2^32 - 65536       just below
#           64 * 64 * 17 = 69632,    69632 * 65535 = 1.06 * 2^32        just above
#   uint8:  256^3 = 16777216,        16777216 * 255 = 2^32 - 2^24       just below
#           256 * 256 * 258,         16908288 * 255 = 1.004 * 2^32      just above
ACC_CASES = (("linear", "uint16", (31, 31, 7), (32, 32, 8), "acc32"),
             ("linear", "uint16", (31, 31, 15), (32, 32, 17), "acc64"),
             ("linear", "uint8", (127, 127, 127), (128, 128, 128), "acc32"),
             ("linear", "uint8", (127, 127, 128), (128, 128, 129), "acc64"))


def reduced_total(src, dst, ops):
    """W after each axis' weights are divided by the closed-form factor the header states"""
    W = 1
    for n, m, op in zip(src, dst, ops):
        if op == "linear":
            W *= 2 * m // math.gcd(math.gcd(2 * m, 2 * n), abs(n - m))
        elif op == "area":
            W *= n // math.gcd(n, m)
    return W


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
