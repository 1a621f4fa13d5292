"""Blosc-1 frames with the LZ4 codec: what zarr's default compressor writes, hence every chunk file of the stores the
reference's ``eval()`` leaves behind (skoots/lib/eval.py:101-111).  ``numcodecs`` is not needed: a frame is a 16-byte
header, a table of block offsets, LZ4 raw blocks and a byte transpose.

``parse_header`` is pure Python (the store readers use it to refuse a store before they decode anything).  The frame
itself is walked in one place, ``sk_blosc_plan_host`` (skoots_amd/csrc/blosc.hip): ``plan`` turns frames into the stream
table and the block table, ``decode_host`` runs the host build of the decoder, ``decode_device`` uploads the frames as
they are, expands all their streams in one ``sk_lz4_streams`` launch (one wave per stream) and undoes the shuffle with
``sk_blosc_unshuffle``.  Written stores stay zlib: nothing here compresses."""
from __future__ import annotations

import ctypes as C
import struct
import time
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np

CODECS = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}

ERRORS = {
    1: "stream table row out of range",
    2: "input exhausted",
    3: "offset 0 or before the start of the output",
    4: "output longer than expected",
    5: "output shorter than expected",
    6: "bad frame header",
    7: "inner codec or shuffle this reader does not decode",
    8: "block table or split prefix outside the frame",
}


class Header(NamedTuple):
    """The 16 bytes in front of a Blosc-1 frame."""
    version: int
    codec_version: int
    flags: int
    typesize: int
    nbytes: int
    blocksize: int
    cbytes: int

    @property
    def shuffle(self) -> bool:
        return bool(self.flags & 0x01)

    @property
    def memcpyed(self) -> bool:
        return bool(self.flags & 0x02)

    @property
    def bitshuffle(self) -> bool:
        return bool(self.flags & 0x04)

    @property
    def dont_split(self) -> bool:
        return bool(self.flags & 0x10)

    @property
    def codec(self) -> str:
        return CODECS.get(self.flags >> 5, f"codec {self.flags >> 5}")

    @property
    def nblocks(self) -> int:
        if self.memcpyed or self.nbytes == 0 or self.blocksize == 0:
            return 0
        return (self.nbytes + self.blocksize - 1) // self.blocksize


def parse_header(first_16_bytes: bytes) -> Header:
    if len(first_16_bytes) < 16:
        raise ValueError(f"a Blosc frame starts with 16 bytes of header, got {len(first_16_bytes)}")
    return Header(*struct.unpack("<BBBBIII", bytes(first_16_bytes[:16])))


def refusal(first_16_bytes: bytes, file_bytes: int, expected_bytes: int) -> Optional[str]:
    """Why a chunk file with this start and this size is no Blosc-1 LZ4 frame of ``expected_bytes``; None if it is."""
    if file_bytes < 16 or len(first_16_bytes) < 16:
        return f"{file_bytes} bytes, shorter than the 16-byte header"
    h = parse_header(first_16_bytes)
    if h.version != 2:
        return f"format version {h.version}, not 2"
    if h.cbytes != file_bytes:
        return f"the header says {h.cbytes} bytes, the file has {file_bytes}"
    if h.nbytes != expected_bytes:
        return f"the frame holds {h.nbytes} bytes, a chunk has {expected_bytes}"
    if h.typesize == 0 or (h.nbytes > 0 and h.blocksize == 0):
        return "typesize or blocksize 0"
    if h.bitshuffle:
        return "bitshuffle is not decoded here"
    if not h.memcpyed and h.codec != "lz4":
        return f"inner codec '{h.codec}' is not decoded here (lz4 only)"
    if not h.memcpyed and h.shuffle and h.typesize > 16:
        return f"byte shuffle with typesize {h.typesize} is not decoded here"
    return None


class BloscError(ValueError):
    """A frame that does not decode: ``index`` is its place in the call, ``reason`` the text of the cause."""

    def __init__(self, index: int, n: int, reason: str):
        super().__init__(f"frame {index} of {n} does not decode: {reason}")
        self.index, self.reason = index, reason


def _reason(code: int) -> str:
    return f"{ERRORS.get(code, code)} (status {code})"


class Plan(NamedTuple):
    """``streams``: int64 (n, 5) rows of src_begin, src_len, dst_begin, dst_len, kind as ``sk_lz4_streams`` takes them,
    src offsets into the frames laid back to back, dst offsets into the outputs laid back to back; rows whose output is
    final come first (``n_direct`` of them), the rows of byte-shuffled frames after them.  ``frame``: the frame every
    row belongs to.  ``blocks``: int64 (m, 2) begin, bytes of every block to unshuffle, ``typesize`` its typesize."""
    streams: np.ndarray
    frame: np.ndarray
    n_direct: int
    blocks: np.ndarray
    typesize: np.ndarray


def plan(frames: Sequence[bytes], expected_bytes: int) -> Plan:
    """Walks every frame (``sk_blosc_plan_host``: header, block table and split prefixes, every offset checked against
    the frame's length) and returns the tables of the whole call.  Raises :class:`BloscError` for a frame that is not
    a well-formed Blosc-1 LZ4 frame of ``expected_bytes``."""
    from .. import _ffi
    n, expected = len(frames), int(expected_bytes)
    rows, owner, shuffled, blocks, sizes = [], [], [], [], []
    counts = np.zeros(4, np.int64)
    status = C.c_int32(0)
    at = 0
    for i, fr in enumerate(frames):
        fr = bytes(fr)
        cap_b = parse_header(fr).nblocks if len(fr) >= 16 else 0
        cap_b = min(cap_b, len(fr) // 4)                       # a table the frame cannot hold is refused by the walk
        cap_s = max(1, cap_b * 16)
        st = np.zeros((cap_s, 5), np.int64)
        bl = np.zeros((max(1, cap_b), 2), np.int64)
        _ffi.check(_ffi.lib.sk_blosc_plan_host(fr, len(fr), expected, st.ctypes.data, cap_s, bl.ctypes.data, cap_b,
                                               counts.ctypes.data, C.byref(status)))
        if status.value != 0:
            raise BloscError(i, n, _reason(status.value))
        ns, nb, ts = int(counts[0]), int(counts[1]), int(counts[2])
        assert ns <= cap_s and nb <= cap_b
        st, bl = st[:ns], bl[:nb]
        st[:, 0] += at
        st[:, 2] += i * expected
        bl[:, 0] += i * expected
        rows.append(st)
        owner.append(np.full(ns, i, np.int64))
        shuffled.append(np.full(ns, nb > 0, bool))
        blocks.append(bl)
        sizes.append(np.full(nb, ts, np.int64))
        at += len(fr)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)  # noqa: E731
    streams, frame, sh = cat(rows, (0, 5), np.int64), cat(owner, (0,), np.int64), cat(shuffled, (0,), bool)
    order = np.argsort(sh, kind="stable")
    return Plan(np.ascontiguousarray(streams[order]), frame[order], int((~sh).sum()), cat(blocks, (0, 2), np.int64),
                cat(sizes, (0,), np.int64))


def decode_host(frames: Sequence[bytes], expected_bytes: int) -> np.ndarray:
    """``(n, expected_bytes)`` uint8: every frame decoded by ``sk_blosc_decode_host``, the host build of the decoder."""
    from .. import _ffi
    n, expected = len(frames), int(expected_bytes)
    out = np.empty((n, expected), np.uint8)
    status = C.c_int32(0)
    for i, fr in enumerate(frames):
        fr = bytes(fr)
        _ffi.check(_ffi.lib.sk_blosc_decode_host(fr, len(fr), out[i].ctypes.data, expected, C.byref(status)))
        if status.value != 0:
            raise BloscError(i, n, _reason(status.value))
    return out


def decode_device(frames: Sequence[bytes], expected_bytes: int, device, timings: Optional[Dict[str, float]] = None):
    """``(n, expected_bytes)`` uint8 rows on ``device``, the shape ``deflate.inflate_streams`` returns.  On a device:
    one upload of the frames as they are, one upload of the tables, ``sk_lz4_streams`` over all streams (twice when
    the call mixes shuffled and unshuffled frames), ``sk_blosc_unshuffle`` per typesize, one read-back of the status
    words.  On ``"cpu"`` the host decoder.  ``timings`` accumulates ``h2d_s``, ``kernel_s`` and ``decoded_bytes``."""
    import torch

    from .. import _ffi
    dev = torch.device(device)
    n, expected = len(frames), int(expected_bytes)
    if dev.type != "cuda":
        return torch.from_numpy(decode_host(frames, expected))
    out = torch.empty((n, expected), dtype=torch.uint8, device=dev)
    p = plan(frames, expected)
    ns = int(p.streams.shape[0])
    if ns == 0:
        return out
    blob = bytearray(b"".join(bytes(f) for f in frames))
    t0 = time.perf_counter()
    src = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    table = torch.from_numpy(p.streams).to(dev)
    status = torch.empty(ns, dtype=torch.int32, device=dev)
    nb = int(p.blocks.shape[0])
    tmp = torch.empty_like(out) if nb else None
    blocks = torch.from_numpy(p.blocks).to(dev) if nb else None
    if timings is not None:
        torch.cuda.synchronize(dev)
        timings["h2d_s"] = timings.get("h2d_s", 0.0) + time.perf_counter() - t0
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(dev))
    stream = _ffi.stream_ptr(dev)
    for lo, hi, dst in ((0, p.n_direct, out), (p.n_direct, ns, tmp)):
        if hi > lo:
            _ffi.check(_ffi.lib.sk_lz4_streams(_ffi.ptr(src), len(blob), _ffi.ptr(table[lo:hi]), hi - lo, _ffi.ptr(dst),
                                               n * expected, _ffi.ptr(status[lo:hi]), stream))
    for ts in sorted(set(p.typesize.tolist())):
        sel = np.flatnonzero(p.typesize == ts)
        a, b = int(sel[0]), int(sel[-1]) + 1
        if b - a == len(sel):
            part = blocks[a:b]                     # the usual case: one typesize, or frames grouped by it
        else:
            part = blocks[torch.from_numpy(sel).to(dev)].contiguous()
        _ffi.check(_ffi.lib.sk_blosc_unshuffle(_ffi.ptr(tmp), _ffi.ptr(out), _ffi.ptr(part), len(sel), int(ts), stream))
    if timings is not None:
        ev1.record(torch.cuda.current_stream(dev))
    bad = status.cpu()   # the one synchronisation
    if timings is not None:
        timings["kernel_s"] = timings.get("kernel_s", 0.0) + ev0.elapsed_time(ev1) * 1e-3
        timings["decoded_bytes"] = timings.get("decoded_bytes", 0) + n * expected
    if bool(bad.any()):
        i = int(p.frame[np.flatnonzero(bad.numpy())].min())      # the first frame that holds a failed stream
        k = int(np.flatnonzero((bad.numpy() != 0) & (p.frame == i))[0])
        raise BloscError(i, n, _reason(int(bad[k])))
    return out
