"""zlib streams for the chunks and pages ``eval()`` writes, produced where the data lives.

A device tensor goes through ``sk_deflate_streams`` (skoots_amd/csrc/deflate.hip): one launch sequence for the whole batch,
one read-back of the offsets, one device-to-host copy of exactly the compressed bytes.  A CPU tensor goes through the
stdlib's ``zlib.compress(row, 1)``, which is what the host writers always did, so that everything above this module
(chunking, store layout, TIFF directories) runs and is tested without a GPU.  Both give complete RFC 1950 streams; the
bytes differ (the device encoder uses the fixed Huffman code and its own match search), what they decode to does not.
"""
from __future__ import annotations

import time
import zlib
from typing import Dict, List, Optional

import torch

from .. import _ffi


def bound(stream_bytes: int) -> int:
    """Worst-case bytes of one stream of the device encoder (host function: no GPU needed)."""
    return int(_ffi.lib.sk_deflate_bound(int(stream_bytes)))


def device_bytes_per_stream(stream_bytes: int) -> int:
    """Device memory ``deflate_streams`` takes per row besides the row itself: output buffer + workspace."""
    return bound(stream_bytes) + int(_ffi.lib.sk_deflate_workspace_bytes(1, int(stream_bytes)))


def deflate_streams(t: torch.Tensor, elem_bytes: int = 1, skip_zero: bool = False,
                    timings: Optional[Dict[str, float]] = None) -> List[Optional[bytes]]:
    """One zlib stream per row of the ``(n, L)`` uint8 tensor ``t``.

    ``elem_bytes`` (1, 2 or 4) tells the device encoder which match distances are worth trying; it never changes the
    format.  With ``skip_zero`` a row of zero bytes gives ``None`` (on the device its stream is neither compacted nor
    copied).  ``timings`` (optional) accumulates ``kernel_s`` (device events), ``d2h_s`` and ``compressed_bytes``.
    """
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
    _ffi.check(_ffi.lib.sk_deflate_streams(_ffi.ptr(t), n, length, elem_bytes, _ffi.ptr(dst), _ffi.ptr(offsets),
                                           _ffi.ptr(zero), _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(dev)))
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
