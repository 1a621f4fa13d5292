"""Writes tests/golden/blosc.npz: Blosc-1 frames from a real c-blosc encoder, each with the bytes it must expand to.

    python tests/golden/make_blosc_golden.py /path/to/libblosc.so

The library is loaded with ctypes (its directory may have to be on LD_LIBRARY_PATH for the codecs it links).  Never
imported by a test; the .npz holds arrays and bytes only.

  a_*   the chunk frames of a <f2 (3, 70, 64, 40) vector-like field in (1, 64, 64, 40) chunks, written as zarr writes
        them: Blosc(cname='lz4', clevel=5, shuffle=1, blocksize=0); edge chunks zero-padded; one chunk entirely zero
  b_*   the same for a |u1 (1, 70, 64, 40) sparse mask
  c_*   single frames: memcpyed, stored splits, shuffle 0, typesize 4 and 8, lz4hc, unsplit small, odd length, many blocks
  d_*   frames a reader of lz4 frames must refuse: blosclz, zlib, zstd, bitshuffle
"""
import ctypes
import itertools
import os
import sys

import numpy as np

CHUNKS = (1, 64, 64, 40)


def main() -> int:
    lib = ctypes.CDLL(sys.argv[1])
    lib.blosc_compress_ctx.restype = ctypes.c_int
    lib.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.blosc_decompress_ctx.restype = ctypes.c_int
    lib.blosc_decompress_ctx.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def compress(raw: bytes, typesize: int, cname: str = "lz4", clevel: int = 5, shuffle: int = 1, blocksize: int = 0) -> bytes:
        dest = ctypes.create_string_buffer(len(raw) + 16 + 4096)
        n = lib.blosc_compress_ctx(clevel, shuffle, typesize, len(raw), raw, dest, len(dest), cname.encode(), blocksize, 1)
        assert n > 0, (cname, n)
        frame = dest.raw[:n]
        back = ctypes.create_string_buffer(max(1, len(raw)))
        assert lib.blosc_decompress_ctx(frame, back, len(raw), 1) == len(raw) and back.raw[:len(raw)] == raw
        return frame

    rng = np.random.default_rng(2024)
    out = {}

    def u8(b: bytes) -> np.ndarray:
        return np.frombuffer(b, np.uint8).copy()

    def store(prefix: str, arr: np.ndarray) -> None:
        out[f"{prefix}_array"] = arr
        names = []
        grid = [range((s + c - 1) // c) for s, c in zip(arr.shape, CHUNKS)]
        for idx in itertools.product(*grid):
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, CHUNKS, arr.shape))
            block = np.zeros(CHUNKS, arr.dtype)
            part = arr[sl]
            if not part.any():
                continue                                     # zarr leaves fill-value chunks out
            block[tuple(slice(0, n) for n in part.shape)] = part
            name = ".".join(str(i) for i in idx)
            names.append(name)
            out[f"{prefix}_frame_{name}"] = u8(compress(block.tobytes(), arr.dtype.itemsize))
        out[f"{prefix}_names"] = np.array(names)

    # (a) vectors: a few smooth blobs of quantised offsets on a zero background; channel 1 beyond x = 64 is all zero
    x, y, z = np.meshgrid(np.arange(70), np.arange(64), np.arange(40), indexing="ij")
    vec = np.zeros((3, 70, 64, 40), np.float16)
    for c, (cx, cy, cz, r) in itertools.product(range(3), ((20, 20, 12, 9), (50, 40, 25, 11), (66, 12, 30, 5))):
        d2 = (x - cx) ** 2 + (y - cy) ** 2 + ((z - cz) * 2) ** 2
        comp = (x - cx, y - cy, z - cz)[c] / 16.0
        vec[c][d2 < r * r] = np.round(comp[d2 < r * r] * 8) / 8
    vec[1, 64:] = 0
    store("a", vec)
    # (b) a sparse mask
    mask = (rng.random((1, 70, 64, 40)) < 0.004).astype(np.uint8)
    store("b", mask)
    assert len(out["a_names"]) == 5 and len(out["b_names"]) == 2

    # (c) single frames
    text = (b"the quick brown fox jumps over the lazy dog. " * 4000)
    ramp32 = (np.arange(30000, dtype=np.uint32) // 7 * 3).tobytes()
    ramp64 = (np.arange(20000, dtype=np.uint64) // 5 * 11).tobytes()
    ramp16 = (np.arange(200001, dtype=np.uint16) // 9).tobytes()
    # random low bytes under zero high bytes: the low-byte split is incompressible (stored), the frame is not
    noisy = rng.integers(0, 256, 30000).astype(np.uint16).tobytes()
    singles = {
        "memcpy_clevel0": (compress(text[:5000], 1, clevel=0), text[:5000]),
        "memcpy_15_bytes": (compress(b"fifteen bytes !", 1), b"fifteen bytes !"),
        "incompressible": (compress(noisy, 2), noisy),
        "shuffle0": (compress(text, 2, shuffle=0), text),
        "typesize4": (compress(ramp32, 4), ramp32),
        "typesize8": (compress(ramp64, 8), ramp64),
        "lz4hc9": (compress(ramp32, 4, cname="lz4hc", clevel=9), ramp32),
        "small200": (compress(text[:200], 2), text[:200]),
        "odd_length": (compress(ramp16[:-1][:100001], 2), ramp16[:-1][:100001]),
        "many_blocks": (compress(ramp16[:400000], 2, blocksize=4096), ramp16[:400000]),
    }
    for name, (frame, raw) in singles.items():
        out[f"c_frame_{name}"] = u8(frame)
        out[f"c_raw_{name}"] = u8(raw)
    out["c_names"] = np.array(list(singles))

    # (d) to refuse
    small = text[:2000]
    refuse = {"blosclz": compress(small, 1, cname="blosclz"), "zlib": compress(small, 1, cname="zlib"),
              "zstd": compress(small, 1, cname="zstd"), "bitshuffle": compress(small, 4, shuffle=2)}
    for name, frame in refuse.items():
        out[f"d_frame_{name}"] = u8(frame)
    out["d_names"] = np.array(list(refuse))
    out["d_bytes"] = np.int64(len(small))

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blosc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        if "_frame_" in k:
            f = v.tobytes()
            print(f"  {k}: {len(f)} bytes, flags {f[2]:#04x}, typesize {f[3]}, nbytes {int.from_bytes(f[4:8], 'little')}, "
                  f"blocksize {int.from_bytes(f[8:12], 'little')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
