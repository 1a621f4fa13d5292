"""zlib streams for the chunks and pages ``eval()`` writes, produced where the data lives.

A device tensor goes through ``sk_deflate_streams`` (skoots_amd/csrc/deflate.hip): one launch sequence for the whole batch,
one read-back of the offsets, one device-to-host copy of exactly the compressed bytes.  A CPU tensor goes through the
stdlib's ``zlib.compress(row, 1)``, which is what the host writers always did, so that everything above this module
(chunking, store layout, TIFF directories) runs and is tested without a GPU.  Both give complete RFC 1950 streams; the
bytes differ (the device encoder has its own match search and codes every 16 KiB piece with the fixed Huffman code, or
with ``huffman="dynamic"`` with the smaller of that and a code built for the piece), what they decode to does not.

``inflate_streams`` is the way back: streams from any deflate encoder go to the device compressed and are inflated there
by ``sk_inflate_streams`` (skoots_amd/csrc/inflate.hip), one wave per stream; for ``device="cpu"`` the stdlib's zlib does
the same with the same checks.
"""
from __future__ import annotations

import numbers
import time
import zlib
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _ffi


def bound(stream_bytes: int) -> int:
    """Worst-case bytes of one stream of the device encoder (host function: no GPU needed)."""
    return int(_ffi.lib.sk_deflate_bound(int(stream_bytes)))


def device_bytes_per_stream(stream_bytes: int) -> int:
    """Device memory ``deflate_streams`` takes per row besides the row itself: output buffer + workspace."""
    return bound(stream_bytes) + int(_ffi.lib.sk_deflate_workspace_bytes(1, int(stream_bytes)))


HUFFMAN_MODES = {"fixed": 0, "dynamic": 1}


def huffman_mode(huffman: str) -> int:
    """``"fixed" | "dynamic"`` -> the ``huffman`` argument of ``sk_deflate_streams_coded``; anything else raises."""
    if not isinstance(huffman, str) or huffman not in HUFFMAN_MODES:
        raise ValueError(f"huffman = {huffman!r}, must be 'fixed' or 'dynamic'")
    return HUFFMAN_MODES[huffman]


def deflate_streams(t: torch.Tensor, elem_bytes: int = 1, skip_zero: bool = False,
                    timings: Optional[Dict[str, float]] = None, huffman: str = "fixed") -> List[Optional[bytes]]:
    """One zlib stream per row of the ``(n, L)`` uint8 tensor ``t``.

    ``elem_bytes`` (1, 2 or 4) tells the device encoder which match distances are worth trying; it never changes the
    format.  With ``skip_zero`` a row of zero bytes gives ``None`` (on the device its stream is neither compacted nor
    copied).  ``timings`` (optional) accumulates ``kernel_s`` (device events), ``d2h_s`` and ``compressed_bytes``.
    ``huffman``: ``"fixed"`` codes every piece with the fixed code of RFC 1951 (or stores it); ``"dynamic"`` also builds
    a code for every piece and writes the smallest form, so no stream gets longer.  A CPU tensor is compressed by zlib
    either way.
    """
    mode = huffman_mode(huffman)
    if t.ndim != 2 or t.dtype != torch.uint8:
        raise ValueError(f"deflate_streams takes a (n, L) uint8 tensor, got {tuple(t.shape)} {t.dtype}")
    if elem_bytes not in (1, 2, 4):
        raise ValueError(f"elem_bytes = {elem_bytes}, must be 1, 2 or 4")
    n, length = int(t.shape[0]), int(t.shape[1])
    if n == 0:
        return []
    t = t.contiguous()
    if not t.is_cuda:
        rows = t.numpy()
        out: List[Optional[bytes]] = []
        for r in rows:
            out.append(None if skip_zero and not r.any() else zlib.compress(r.tobytes(), 1))
        return out

    dev = t.device
    cap = bound(length)
    ws_bytes = int(_ffi.lib.sk_deflate_workspace_bytes(n, length))
    dst = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    zero = torch.empty(n, dtype=torch.uint8, device=dev) if skip_zero else None
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if timings is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(dev))
    if mode == 0:
        _ffi.check(_ffi.lib.sk_deflate_streams(_ffi.ptr(t), n, length, elem_bytes, _ffi.ptr(dst), _ffi.ptr(offsets),
                                               _ffi.ptr(zero), _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(dev)))
    else:
        _ffi.check(_ffi.lib.sk_deflate_streams_coded(_ffi.ptr(t), n, length, elem_bytes, mode, _ffi.ptr(dst),
                                                     _ffi.ptr(offsets), _ffi.ptr(zero), _ffi.ptr(ws), ws_bytes,
                                                     _ffi.stream_ptr(dev)))
    if timings is not None:
        ev1.record(torch.cuda.current_stream(dev))
    off = offsets.cpu().tolist()   # the one synchronisation
    t0 = time.perf_counter()
    blob = dst[:off[-1]].cpu().numpy().tobytes()
    if timings is not None:
        timings["d2h_s"] = timings.get("d2h_s", 0.0) + time.perf_counter() - t0
        timings["kernel_s"] = timings.get("kernel_s", 0.0) + ev0.elapsed_time(ev1) * 1e-3
        timings["compressed_bytes"] = timings.get("compressed_bytes", 0) + off[-1]
    # a real stream has at least 8 bytes: an empty slice is a row the encoder left out
    return [blob[a:b] if b > a else None for a, b in zip(off[:-1], off[1:])]


class InflateError(ValueError):
    """A stream that does not inflate: ``index`` is its place in the call, ``reason`` the text of the cause."""

    def __init__(self, index: int, n: int, reason: str):
        super().__init__(f"stream {index} of {n} does not inflate: {reason}")
        self.index, self.reason = index, reason


INFLATE_ERRORS = {
    1: "bad or unsupported zlib header",
    2: "reserved block type",
    3: "stored block whose LEN and NLEN do not match",
    4: "bad code-length set",
    5: "invalid symbol",
    6: "distance before the start of the output",
    7: "input exhausted",
    8: "output longer than expected",
    9: "output shorter than expected",
    10: "Adler-32 mismatch",
    11: "offsets out of range",
}


def _inflate_host(stream: bytes, size: int, wbits: int) -> Optional[bytes]:
    """The stream's bytes if zlib inflates it without error, to its end and to ``size`` bytes; else the reason."""
    d = zlib.decompressobj(wbits)
    try:
        out = d.decompress(stream, size + 1)
    except zlib.error as e:
        return str(e)
    if len(out) > size:
        return INFLATE_ERRORS[8]
    if not d.eof:
        return INFLATE_ERRORS[7]
    if len(out) < size:
        return INFLATE_ERRORS[9]
    return out


def inflate_streams(streams: Sequence[bytes], sizes: Union[int, Sequence[int]], device, wrapper: str = "zlib",
                    timings: Optional[Dict[str, float]] = None, out: Optional[torch.Tensor] = None
                    ) -> Union[torch.Tensor, Tuple[torch.Tensor, List[int]]]:
    """Inflates ``streams`` (a sequence of ``bytes``: zlib streams, or raw deflate with ``wrapper="raw"``) on ``device``.

    ``sizes`` is what every stream must inflate to, exactly: one int for all, or one per stream.  Returns a ``(n, L)``
    uint8 tensor when all sizes are the same ``L``, otherwise ``(flat, offsets)``: the outputs back to back in one uint8
    tensor and the ``n + 1`` offsets into it.  ``out`` (optional, a contiguous uint8 tensor on ``device`` with exactly
    the total number of bytes) receives the outputs instead of a new tensor.  On a device this is one upload of the
    concatenated streams, one launch (one wave per stream) and one read-back of the status words; on ``"cpu"`` the
    stdlib's zlib.  A stream that does not inflate to its end and its size raises ``ValueError`` naming its index and
    the reason (:class:`InflateError`, a ``ValueError`` that also carries ``index``).  ``timings`` (optional) accumulates ``h2d_s``, ``kernel_s`` (device events) and ``inflated_bytes``."""
    if wrapper not in ("zlib", "raw"):
        raise ValueError(f"wrapper = {wrapper!r}, must be 'zlib' or 'raw'")
    n = len(streams)
    size_list = [int(sizes)] * n if isinstance(sizes, numbers.Integral) else [int(v) for v in sizes]
    if len(size_list) != n or any(v < 0 for v in size_list):
        raise ValueError(f"{n} streams but sizes = {sizes!r}")
    dst_off = [0]
    for v in size_list:
        dst_off.append(dst_off[-1] + v)
    total = dst_off[-1]
    dev = torch.device(device)
    if out is not None:
        if out.dtype != torch.uint8 or out.numel() != total or not out.is_contiguous() or out.device.type != dev.type:
            raise ValueError(f"out must be a contiguous uint8 tensor of {total} bytes on {dev}")
        flat = out.view(-1)
    else:
        flat = torch.empty(total, dtype=torch.uint8, device=dev)
    equal = n > 0 and all(v == size_list[0] for v in size_list)

    if dev.type != "cuda":
        parts = []
        for i, (st, v) in enumerate(zip(streams, size_list)):
            got = _inflate_host(bytes(st), v, 15 if wrapper == "zlib" else -15)
            if isinstance(got, str):
                raise InflateError(i, n, got)
            parts.append(got)
        if total:
            flat.copy_(torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8))
    elif n:
        src_off = [0]
        for st in streams:
            src_off.append(src_off[-1] + len(st))
        blob = bytearray(b"".join(bytes(st) for st in streams)) or bytearray(1)
        t0 = time.perf_counter()
        src = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        offs = torch.tensor([src_off, dst_off], dtype=torch.int64).to(dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        dst = flat if total else torch.empty(1, dtype=torch.uint8, device=dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["h2d_s"] = timings.get("h2d_s", 0.0) + time.perf_counter() - t0
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(torch.cuda.current_stream(dev))
        _ffi.check(_ffi.lib.sk_inflate_streams(_ffi.ptr(src), _ffi.ptr(offs[0]), n, _ffi.ptr(dst), _ffi.ptr(offs[1]),
                                               1 if wrapper == "zlib" else 0, _ffi.ptr(status), _ffi.stream_ptr(dev)))
        if timings is not None:
            ev1.record(torch.cuda.current_stream(dev))
        bad = status.cpu()   # the one synchronisation
        if timings is not None:
            timings["kernel_s"] = timings.get("kernel_s", 0.0) + ev0.elapsed_time(ev1) * 1e-3
            timings["inflated_bytes"] = timings.get("inflated_bytes", 0) + total
        if bool(bad.any()):
            i = int(bad.ne(0).nonzero()[0])
            code = int(bad[i])
            raise InflateError(i, n, f"{INFLATE_ERRORS.get(code, code)} (status {code})")
    if equal:
        return flat.view(n, size_list[0])
    return flat, dst_off
