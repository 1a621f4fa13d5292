"""Multi-page TIFF input shared by ``eval()`` and the training dataset (the reference reads both with skimage.io), and
the multi-page TIFF ``eval()`` writes its instance mask to."""
from __future__ import annotations

import struct

import numpy as np


def read_image(path: str) -> np.ndarray:
    """[Z, X, Y(, C)] array from a multi-page TIFF (Pillow) or a .npy file (eval.py:61)."""
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    pages = []
    with Image.open(path) as im:
        for i in range(getattr(im, "n_frames", 1)):
            im.seek(i)
            pages.append(np.array(im))
    return np.stack(pages, axis=0)


# ----------------------------------------------------------------------------------------
# Multi-page TIFF output: classic little-endian TIFF written by hand, one deflate strip per page
# ----------------------------------------------------------------------------------------
WRITE_STACK_BUDGET = 256 << 20  # bytes of page data + encoder buffers per batch of pages
_TIFF_MAX = 2 ** 32 - 1
_IFD_TAGS = 10
_IFD_BYTES = 2 + 12 * _IFD_TAGS + 4


def _page_rows(pages):
    """(Z, H, W) array or tensor of uint8 / uint16 / int32 -> ((Z, H * W * itemsize) uint8 tensor, bits, sample format)."""
    import torch
    if isinstance(pages, np.ndarray):
        if pages.dtype not in (np.uint8, np.uint16, np.int32) or pages.ndim != 3:
            raise ValueError(f"write_stack takes (Z, H, W) uint8 / uint16 / int32, got {pages.shape} {pages.dtype}")
        fmt = 2 if pages.dtype == np.int32 else 1
        arr = np.ascontiguousarray(pages)
        raw = torch.from_numpy(arr.view(np.uint8).reshape(arr.shape[0], -1) if arr.size else
                               np.zeros((arr.shape[0], 0), np.uint8))
        return raw, 8 * arr.dtype.itemsize, fmt
    if pages.ndim != 3 or pages.dtype not in (torch.uint8, torch.uint16, torch.int32):
        raise ValueError(f"write_stack takes (Z, H, W) uint8 / uint16 / int32, got {tuple(pages.shape)} {pages.dtype}")
    t = pages.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1), 8 * t.element_size(), 2 if t.dtype == torch.int32 else 1


def _write_pages(path: str, rows, height: int, width: int, bits: int, sample_format: int,
                 budget_bytes: int = WRITE_STACK_BUDGET, timings=None) -> None:
    """``rows``: (Z, page_bytes) uint8 tensor on either device, page z = row z in C order, little-endian samples."""
    import time

    from . import deflate
    n_pages, page_bytes = int(rows.shape[0]), int(rows.shape[1])
    if n_pages < 1 or height * width * (bits // 8) != page_bytes:
        raise ValueError(f"{n_pages} pages of {page_bytes} bytes do not make {height} x {width} x {bits} bit pages")
    batch = max(1, int(budget_bytes) // (page_bytes + deflate.device_bytes_per_stream(page_bytes)))
    strips = []
    for lo in range(0, n_pages, batch):
        strips += deflate.deflate_streams(rows[lo:lo + batch], elem_bytes=bits // 8, timings=timings)
    # layout: header, the strips (each on an even offset), then one directory per page
    offsets, at = [], 8
    for s in strips:
        offsets.append(at)
        at += len(s) + (len(s) & 1)
    total = at + n_pages * _IFD_BYTES
    if total > _TIFF_MAX:
        raise ValueError(f"{path}: {total} bytes do not fit a classic TIFF (32-bit offsets); BigTIFF is not supported")
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, at))
        for s in strips:
            f.write(s)
            if len(s) & 1:
                f.write(b"\0")
        for z, s in enumerate(strips):
            ifd = at + z * _IFD_BYTES
            tags = ((256, 4, width), (257, 4, height), (258, 3, bits), (259, 3, 8), (262, 3, 1), (273, 4, offsets[z]),
                    (277, 3, 1), (278, 4, height), (279, 4, len(s)), (339, 3, sample_format))
            f.write(struct.pack("<H", len(tags)))
            for tag, typ, val in tags:   # a SHORT value sits in the low half of the 4-byte value field
                f.write(struct.pack("<HHII", tag, typ, 1, val))
            f.write(struct.pack("<I", ifd + _IFD_BYTES if z + 1 < n_pages else 0))
    if timings is not None:
        timings["file_s"] = timings.get("file_s", 0.0) + time.perf_counter() - t0


def write_stack(path: str, pages, budget_bytes: int = WRITE_STACK_BUDGET, timings=None) -> None:
    """(Z, H, W) uint8 / uint16 / int32 tensor (either device) or array -> multi-page TIFF with Adobe-deflate strips.

    One directory and one strip per page; tags 256, 257, 258, 259 (= 8), 262 (= 1), 273, 277, 278, 279, 339.  Every
    strip is one zlib stream from :func:`skoots_amd.lib.deflate.deflate_streams`, made on the tensor's device in batches
    of pages that keep page data + encoder buffers under ``budget_bytes``; the compressed strips are held on the host
    until the layout is known.  A file past 2**32 - 1 bytes raises ``ValueError`` before anything is written."""
    rows, bits, fmt = _page_rows(pages)
    _write_pages(path, rows, int(pages.shape[1]), int(pages.shape[2]), bits, fmt, budget_bytes, timings)


def write_label_stack(path: str, labels_zxy, timings=None) -> None:
    """(Z, X, Y) int32 label tensor -> TIFF, uint16 pages while every label is below 65536, int32 otherwise (the
    narrowing ``eval._write_mask_tif`` applies on the host), without leaving the tensor's device."""
    import torch
    t = labels_zxy.contiguous()
    if t.dtype != torch.int32 or t.ndim != 3:
        raise ValueError(f"write_label_stack takes a (Z, X, Y) int32 tensor, got {tuple(t.shape)} {t.dtype}")
    if t.numel() == 0 or int(t.max()) < 65536:
        # the low two bytes of every label: int16 storage holds the uint16 bit patterns
        rows = t.to(torch.int16).view(torch.uint8).reshape(t.shape[0], -1)
        _write_pages(path, rows, int(t.shape[1]), int(t.shape[2]), 16, 1, timings=timings)
    else:
        write_stack(path, t, timings=timings)
