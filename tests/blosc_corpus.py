"""LZ4 raw blocks for the Blosc reader's tests (a helper, not a test): a pure-Python reference decoder that implements
exactly the acceptance rules of ``sk_lz4_streams`` (include/skoots_hip.h), hand-assembled streams at the edges where a
wave decoder can go wrong, every truncation and every single-bit flip of three short valid streams, and one named case
per status code.  Shared by tests/test_blosc_host.py, tests/test_hip_blosc.py and tools/blosc_host_check.py."""
from __future__ import annotations

import functools
import json
import os
import struct
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

E_RANGE, E_INPUT, E_OFFSET, E_LONG, E_SHORT = 1, 2, 3, 4, 5
E_HEADER, E_CODEC, E_FRAME = 6, 7, 8
KIND_LZ4, KIND_STORED = 0, 1
WINDOW = 4096           # bytes of the decoder's input window (kLz4Win dwords, skoots_amd/csrc/blosc_lz4.inc)
RING = 65536


class Case(NamedTuple):
    name: str
    stream: bytes
    size: int                   # bytes the stream must expand to
    expect: Optional[bytes]     # the bytes, or None: refused
    code: int = 0               # the status a refused stream must report; 0 = any non-zero status
    kind: int = KIND_LZ4


def decode(stream: bytes, size: int, kind: int = KIND_LZ4) -> Tuple[int, Optional[bytes]]:
    """(status, bytes): the reference.  Status 0 exactly when the stream parses, ends at its last byte after a literal
    run and has produced ``size`` bytes; the checks come in the order the header documents."""
    if kind == KIND_STORED:
        return (0, bytes(stream)) if len(stream) == size else (E_RANGE, None)
    if kind != KIND_LZ4:
        return E_RANGE, None
    n, ip, out = len(stream), 0, bytearray()
    while True:
        if ip >= n:
            return E_INPUT, None
        token = stream[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    return E_INPUT, None
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        if lit > n - ip:
            return E_INPUT, None
        if lit > size - len(out):
            return E_LONG, None
        out += stream[ip:ip + lit]
        ip += lit
        if ip == n:
            return (0, bytes(out)) if len(out) == size else (E_SHORT, None)
        if n - ip < 2:
            return E_INPUT, None
        off = stream[ip] | stream[ip + 1] << 8
        ip += 2
        if off == 0 or off > len(out):
            return E_OFFSET, None
        length = token & 15
        if length == 15:
            while True:
                if ip >= n:
                    return E_INPUT, None
                b = stream[ip]
                ip += 1
                length += b
                if b != 255:
                    break
        length += 4
        if length > size - len(out):
            return E_LONG, None
        period = bytes(out[-off:])
        out += (period * (length // off + 1))[:length]


def _ext(v: int) -> bytes:
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq(literals: bytes, offset: int, length: int) -> bytes:
    """One sequence: literals, then a match of ``length`` >= 4 bytes ``offset`` back."""
    ln, ml = len(literals), length - 4
    out = bytes([(min(ln, 15) << 4) | min(ml, 15)])
    if ln >= 15:
        out += _ext(ln - 15)
    out += literals + struct.pack("<H", offset)
    if ml >= 15:
        out += _ext(ml - 15)
    return out


def last(literals: bytes) -> bytes:
    """The closing sequence: literals only."""
    ln = len(literals)
    return bytes([min(ln, 15) << 4]) + (_ext(ln - 15) if ln >= 15 else b"") + literals


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _good(name: str, stream: bytes) -> Case:
    status, data = decode(stream, _size(stream))
    assert status == 0, (name, status)
    return Case(name, stream, len(data), data)


def _size(stream: bytes) -> int:
    """Bytes a well-formed stream expands to (parsed without a size limit)."""
    n, ip, total = len(stream), 0, 0
    while ip < n:
        token = stream[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        total += lit
        if ip >= n:
            break
        ip += 2
        length = token & 15
        if length == 15:
            while True:
                b = stream[ip]
                ip += 1
                length += b
                if b != 255:
                    break
        total += length + 4
    return total


@functools.lru_cache(maxsize=None)
def hand_assembled() -> List[Case]:
    cases = [_good("empty_output", b"\x00")]
    for n in (0, 14, 15, 16, 269, 270, 271):
        cases.append(_good(f"lit{n}_last", seq(_rand(20, n), 5, 7) + last(_rand(n, n + 1))))
        if n:
            cases.append(_good(f"lit{n}_first", seq(_rand(n, n + 2), 1, 4) + last(b"xyz")))
    for n in (4, 18, 19, 20, 273, 274):
        cases.append(_good(f"match{n}", seq(_rand(30, n), 7, n) + last(_rand(5, n))))
    for off in (1, 2, 3, 4, 7, 8, 63, 64, 65, 4095, 65534, 65535):
        cases.append(_good(f"offset{off}", seq(_rand(off, off), off, 200) + last(b"end")))
        cases.append(_good(f"offset{off}_behind", seq(_rand(off + 9, off), off, 131) + last(b"")))
    cases.append(_good("match_wraps_the_ring", seq(_rand(RING - 6, 1), 100, 300) + last(b"tail")))
    cases.append(_good("source_wraps_the_ring", seq(_rand(RING + 50, 2), 100, 150) + seq(b"ab", RING - 1, 70) + last(b"")))
    for total in (65535, 65536, 65537, 131072):
        cases.append(_good(f"out{total}", seq(_rand(16, total), 16, total - 20) + last(b"last")))
    cases.append(_good("out131072_offset7", seq(_rand(7, 7), 7, 131072 - 7 - 3) + last(b"end")))
    cases.append(_good("out131072_offset65535", seq(_rand(RING - 1, 8), RING - 1, 131072 - RING - 2) + last(b"end")))
    for target in (WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW, 2 * WINDOW + 1):
        k = (target - 10) // 6
        body = b"".join(seq(bytes([i & 255, (i * 7) & 255, (i * 13) & 255]), 2, 6) for i in range(k))
        stream = body + last(_rand(target - 6 * k - 1, target))
        assert len(stream) == target
        cases.append(_good(f"src{target}", stream))
    # a long literal run read across several windows, then a match
    cases.append(_good("literals_across_windows", seq(_rand(3 * WINDOW + 5, 3), 3 * WINDOW, 64) + last(b"")))
    cases.append(Case("stored", _rand(1000, 4), 1000, _rand(1000, 4), 0, KIND_STORED))
    cases.append(Case("stored_empty", b"", 0, b"", 0, KIND_STORED))
    return cases


@functools.lru_cache(maxsize=None)
def short_streams() -> List[bytes]:
    a = seq(_rand(20, 11), 3, 40) + seq(b"", 20, 19) + last(_rand(6, 12))
    b = seq(_rand(270, 13), 269, 274) + seq(_rand(5, 14), 1, 4) + last(_rand(16, 15))
    c = b"".join(seq(_rand(1 + i % 3, 20 + i), 1 + i % 2, 4 + i) for i in range(20)) + last(b"closing")
    assert all(len(s) <= 512 and decode(s, _size(s))[0] == 0 for s in (a, b, c))
    return [a, b, c]


def _judged(name: str, stream: bytes, size: int) -> Case:
    status, data = decode(stream, size)
    return Case(name, stream, size, data, 0 if data is not None else status)


@functools.lru_cache(maxsize=None)
def truncations() -> List[Case]:
    out = []
    for k, s in enumerate(short_streams()):
        size = _size(s)
        out += [_judged(f"trunc{k}:{n}", s[:n], size) for n in range(len(s))]
    return out


@functools.lru_cache(maxsize=None)
def bit_flips() -> List[Case]:
    out = []
    for k, s in enumerate(short_streams()):
        size = _size(s)
        for bit in range(8 * len(s)):
            t = bytearray(s)
            t[bit >> 3] ^= 1 << (bit & 7)
            out.append(_judged(f"flip{k}:{bit}", bytes(t), size))
    return out


@functools.lru_cache(maxsize=None)
def named_errors() -> List[Case]:
    good = seq(b"abcdefgh", 4, 8) + last(b"12345")            # 21 bytes
    cases = [
        Case("stored_lengths_differ", b"0123456789", 11, None, E_RANGE, KIND_STORED),
        Case("unknown_kind", good, 21, None, E_RANGE, 2),
        Case("no_input", b"", 0, None, E_INPUT),
        Case("ends_after_match", seq(b"abcdefgh", 4, 8), 16, None, E_INPUT),
        Case("literal_run_past_end", b"\x50abc", 5, None, E_INPUT),
        Case("literal_length_cut", b"\xf0\xff", 600, None, E_INPUT),
        Case("offset_cut", b"\x40abcd\x02", 12, None, E_INPUT),
        Case("match_length_cut", b"\x4fabcd\x02\x00\xff", 600, None, E_INPUT),
        Case("offset_zero", seq(b"abcd", 0, 4) + last(b"x"), 9, None, E_OFFSET),
        Case("offset_before_output", seq(b"abcd", 5, 4) + last(b"x"), 9, None, E_OFFSET),
        Case("expected_one_less", good, 20, None, E_LONG),
        Case("match_overflows", seq(b"abcdefgh", 4, 800) + last(b"1"), 100, None, E_LONG),
        Case("expected_one_more", good, 22, None, E_SHORT),
    ]
    for c in cases:
        assert decode(c.stream, c.size, c.kind) == (c.code, None), c.name
    return cases


def good_neighbours() -> List[Case]:
    """Valid streams to stand next to malformed ones in a launch: a failed stream never stops the others."""
    return [c for c in hand_assembled() if c.name in ("lit15_last", "match273", "offset63", "src4096")]


def range_rows(src_bytes: int, dst_bytes: int) -> List[Tuple[int, int, int, int, int]]:
    """Table rows that must report E_RANGE whatever the buffers hold."""
    big = 1 << 62
    return [(-1, 4, 0, 4, 0), (0, -1, 0, 4, 0), (0, 4, -1, 4, 0), (0, 4, 0, -1, 0), (src_bytes, 1, 0, 4, 0),
            (0, src_bytes + 1, 0, 4, 0), (0, 4, dst_bytes, 1, 0), (0, 4, 0, dst_bytes + 1, 0), (big, big, 0, 4, 0),
            (0, 4, big, big, 0), (0, 4, 0, 4, 7), (0, 4, 0, 5, 1), (src_bytes + 1, 0, 0, 0, 0), (0, 0, dst_bytes + 1, 0, 0)]


def all_cases() -> List[Case]:
    return hand_assembled() + truncations() + bit_flips() + named_errors()


def frame_of(stream: bytes, size: int, typesize: int = 1, shuffle: bool = False) -> Optional[bytes]:
    """The stream as the only split of a one-block Blosc-1 LZ4 frame (don't-split flag set), so that it can go through
    the frame decoders.  None where a frame cannot carry it: an empty output has no block, and a split as long as its
    output means "stored"."""
    if size == 0 or len(stream) == size:
        return None
    flags = 0x20 | 0x10 | (0x01 if shuffle else 0)
    body = struct.pack("<i", 20) + struct.pack("<i", len(stream)) + stream
    return struct.pack("<BBBBIII", 2, 1, flags, typesize, size, size, 16 + len(body)) + body


# ------------------------------------------------------------------------------------------ the golden frames
CHUNKS = (1, 64, 64, 40)
ZARR_BLOSC = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}     # what the reference's zarr writes


def _chunk(arr, name) -> bytes:
    idx = [int(v) for v in str(name).split(".")]
    block = np.zeros(CHUNKS, arr.dtype)
    part = arr[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, CHUNKS))]
    block[tuple(slice(0, n) for n in part.shape)] = part
    return block.tobytes()


def good_frames(d) -> List[Tuple[str, bytes, bytes]]:
    """(name, frame, expected bytes) of the parts (a), (b) and (c) of tests/golden/blosc.npz (``d``: the loaded file)."""
    out = []
    for prefix in "ab":
        out += [(f"{prefix}:{n}", d[f"{prefix}_frame_{n}"].tobytes(), _chunk(d[f"{prefix}_array"], n)) for n in d[f"{prefix}_names"]]
    return out + [(f"c:{n}", d[f"c_frame_{n}"].tobytes(), d[f"c_raw_{n}"].tobytes()) for n in d["c_names"]]


def damaged(frame: bytes) -> bytes:
    """The frame with the first three bytes of its first split set to zero: a token without literals and a match of
    offset 0 (E_OFFSET).  For frames with a block table whose first split is an LZ4 block."""
    p0 = int.from_bytes(frame[16:20], "little")
    return frame[:p0 + 4] + bytes(3) + frame[p0 + 7:]


def write_store(path: str, d, prefix: str, compressor=ZARR_BLOSC):
    """Part (a) or (b) as a zarr v2 store directory: the chunk frames as files, fill-value chunks absent."""
    arr = d[f"{prefix}_array"]
    os.makedirs(path)
    meta = {"zarr_format": 2, "shape": list(arr.shape), "chunks": list(CHUNKS), "dtype": "<f2" if prefix == "a" else "|u1",
            "compressor": compressor, "fill_value": 0, "order": "C", "filters": None}
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f)
    for n in d[f"{prefix}_names"]:
        with open(os.path.join(path, str(n)), "wb") as f:
            f.write(d[f"{prefix}_frame_{n}"].tobytes())
    return arr
