"""Multi-page TIFF input shared by ``eval()`` and the training dataset (the reference reads both with skimage.io), and
the multi-page TIFF ``eval()`` writes its instance mask to.  ``read_stack`` reads the common kind of such files --
stripped, uncompressed or deflate, integer samples -- straight to a device: the strips are uploaded as they are in the
file and inflated there (``lib/deflate.py: inflate_streams``); everything else goes through ``read_image``."""
from __future__ import annotations

import struct
from typing import NamedTuple, Optional, Tuple

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
# Multi-page TIFF input on a device: a directory scan on the host, the strips inflated where the stack is wanted
# ----------------------------------------------------------------------------------------
class TiffPage(NamedTuple):
    strip_offsets: Tuple[int, ...]
    strip_byte_counts: Tuple[int, ...]
    rows_per_strip: int
    width: int
    height: int
    bits: int
    sample_format: int
    samples_per_pixel: int
    predictor: int
    compression: int


class TiffPlan(NamedTuple):
    pages: Tuple[TiffPage, ...]
    dtype: np.dtype            # of the array read_image gives for such a file
    shape: Tuple[int, ...]     # (Z, H, W) or (Z, H, W, C)


_TIFF_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8}
_TIFF_TYPE_FMT = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 16: "Q"}
_DEFLATE = (8, 32946)


def _ifd_values(buf: bytes, typ: int, count: int, field: int):
    """Integer values of one directory entry (``field`` = offset of its 4-byte value field), or None."""
    if typ not in _TIFF_TYPE_FMT or count < 1:
        return None
    nbytes = _TIFF_TYPE_SIZE[typ] * count
    at = field if nbytes <= 4 else struct.unpack_from("<I", buf, field)[0]
    if at + nbytes > len(buf):
        return None
    return struct.unpack_from(f"<{count}{_TIFF_TYPE_FMT[typ]}", buf, at)


def _scan_bytes(buf: bytes) -> Optional[TiffPlan]:
    if len(buf) < 8 or buf[:4] != b"II*\0":
        return None                      # big-endian, BigTIFF (version 43) or no TIFF at all
    pages, seen = [], set()
    ifd = struct.unpack_from("<I", buf, 4)[0]
    while ifd:
        if ifd in seen or ifd + 2 > len(buf):
            return None
        seen.add(ifd)
        n = struct.unpack_from("<H", buf, ifd)[0]
        if ifd + 2 + 12 * n + 4 > len(buf):
            return None
        tags = {}
        for k in range(n):
            tag, typ, count = struct.unpack_from("<HHI", buf, ifd + 2 + 12 * k)
            tags[tag] = (typ, count, ifd + 2 + 12 * k + 8)

        def get(tag, default=None, many=False):
            if tag not in tags:
                return default
            v = _ifd_values(buf, *tags[tag])
            if v is None:
                return None
            return v if many else v[0]

        if any(t in tags for t in (322, 323, 324, 325)):          # tiled
            return None
        if get(274, 1) != 1:              # Pillow applies the Orientation tag when it loads a page: left to read_image
            return None
        width, height = get(256), get(257)
        spp = get(277, 1)
        bits = get(258, (1,), many=True)
        fmt = get(339, (1,), many=True)
        comp, photo, fill, planar = get(259, 1), get(262), get(266, 1), get(284, 1)
        pred, rps = get(317, 1), get(278, 2 ** 32 - 1)
        offs, counts = get(273, many=True), get(279, many=True)
        if None in (width, height, spp, bits, fmt, comp, photo, fill, planar, pred, rps, offs, counts):
            return None
        if width < 1 or height < 1 or rps < 1 or len(set(bits)) != 1 or len(set(fmt)) != 1 or len(bits) not in (1, spp):
            return None
        bits, fmt = bits[0], fmt[0]
        # what Pillow turns into the same array: 8- and 16-bit unsigned and 32-bit integer grey, 8-bit RGB(A)
        grey = spp == 1 and photo == 1 and ((bits in (8, 16) and fmt == 1) or (bits == 32 and fmt in (1, 2)))
        colour = spp in (3, 4) and photo == 2 and bits == 8 and fmt == 1 and (spp == 3 or 338 in tags)
        if not (grey or colour) or fill != 1 or (spp > 1 and planar != 1):
            return None
        if comp not in (1,) + _DEFLATE or pred not in (1, 2) or (comp == 1 and pred != 1):
            return None
        rps = min(rps, height)
        n_strips = (height + rps - 1) // rps
        if len(offs) != n_strips or len(counts) != n_strips:
            return None
        row_bytes = width * spp * (bits // 8)
        for k, (o, c) in enumerate(zip(offs, counts)):
            want = min(rps, height - k * rps) * row_bytes
            if o + c > len(buf) or c < 1 or (comp == 1 and c != want):
                return None
        pages.append(TiffPage(tuple(offs), tuple(counts), rps, width, height, bits, fmt, spp, pred, comp))
        ifd = struct.unpack_from("<I", buf, ifd + 2 + 12 * n)[0]
    if not pages:
        return None
    p0 = pages[0]
    for p in pages[1:]:   # one geometry and one sample type for the whole stack (the strips may be cut differently)
        if (p.width, p.height, p.bits, p.sample_format, p.samples_per_pixel) != \
                (p0.width, p0.height, p0.bits, p0.sample_format, p0.samples_per_pixel):
            return None
    dtype = np.dtype({8: np.uint8, 16: np.uint16, 32: np.int32}[p0.bits])
    shape = (len(pages), p0.height, p0.width) + ((p0.samples_per_pixel,) if p0.samples_per_pixel > 1 else ())
    return TiffPlan(tuple(pages), dtype, shape)


def scan(path: str) -> Optional[TiffPlan]:
    """Directory scan of a classic little-endian TIFF, on the host and by hand: per page the strip offsets and byte
    counts, rows per strip, width, height, bits, sample format, samples per pixel, predictor and compression.  ``None``
    for everything ``read_stack``'s device path does not cover: big-endian, BigTIFF, tiles, a compression other than
    none (1) or deflate (8, 32946), a predictor other than 1 or 2, samples other than 8- / 16-bit unsigned and 32-bit
    integers (grey) or 8-bit RGB(A), planar configuration 2, an Orientation other than 1, pages of different sizes, ``.npy``, a damaged directory."""
    if path.endswith(".npy"):
        return None
    try:
        with open(path, "rb") as f:
            buf = f.read()
        return _scan_bytes(buf)
    except (struct.error, OSError):
        return None


def read_stack(path: str, device, timings=None):
    """``torch.from_numpy(read_image(path)).to(device)`` -- the (Z, H, W[, C]) stack with the dtype ``read_image`` gives --
    with the strips inflated on ``device``: for a file ``scan`` covers, the strips are uploaded as they are in the file,
    inflated by ``inflate_streams`` (one wave per strip) and predictor 2 is undone by ``sk_tiff_undo_predictor``; on
    ``"cpu"`` the same plan runs with the stdlib's zlib and numpy.  Every other file goes through ``read_image``."""
    import torch

    from . import deflate
    plan = scan(path)
    if plan is None:
        return torch.from_numpy(read_image(path)).to(device)
    dev = torch.device(device)
    with open(path, "rb") as f:
        buf = f.read()
    p0 = plan.pages[0]
    row_bytes = p0.width * p0.samples_per_pixel * (p0.bits // 8)
    flat = torch.empty(len(plan.pages) * p0.height * row_bytes, dtype=torch.uint8, device=dev)
    # pages with the same compression are read together; they lie back to back in `flat` in page and row order
    at, k = 0, 0
    while k < len(plan.pages):
        j = k
        while j < len(plan.pages) and plan.pages[j].compression == plan.pages[k].compression:
            j += 1
        strips, sizes = [], []
        for p in plan.pages[k:j]:
            for i, (o, c) in enumerate(zip(p.strip_offsets, p.strip_byte_counts)):
                strips.append(buf[o:o + c])
                sizes.append(min(p.rows_per_strip, p.height - i * p.rows_per_strip) * row_bytes)
        total = sum(sizes)
        if plan.pages[k].compression == 1:
            flat[at:at + total].copy_(torch.frombuffer(bytearray(b"".join(strips)), dtype=torch.uint8))
        else:
            try:
                deflate.inflate_streams(strips, sizes, dev, timings=timings, out=flat[at:at + total])
            except ValueError as e:
                raise ValueError(f"{path}: strip {e}") from None
        at += total
        k = j
    tdt = torch.from_numpy(np.empty(0, dtype=plan.dtype)).dtype
    stack = flat.view(tdt).view(plan.shape)
    z = 0
    while z < len(plan.pages):      # runs of pages with predictor 2
        if plan.pages[z].predictor != 2:
            z += 1
            continue
        j = z
        while j < len(plan.pages) and plan.pages[j].predictor == 2:
            j += 1
        _undo_predictor(stack[z:j], p0)
        z = j
    return stack


def _undo_predictor(pages, p0: TiffPage) -> None:
    """In place, on the tensor's device: (n, H, W[, C]) differences along W -> samples."""
    import torch
    if pages.is_cuda:
        from .. import _ffi
        _ffi.check(_ffi.lib.sk_tiff_undo_predictor(_ffi.ptr(pages), int(pages.shape[0]) * p0.height, p0.width,
                                                   p0.samples_per_pixel, p0.bits // 8, _ffi.stream_ptr(pages.device)))
    else:
        arr = pages.numpy()     # shares the tensor's memory
        np.cumsum(arr, axis=2, dtype=arr.dtype, out=arr)


# ----------------------------------------------------------------------------------------
# Multi-page TIFF output: classic little-endian TIFF written by hand, one deflate strip per page
# ----------------------------------------------------------------------------------------
WRITE_STACK_BUDGET = 256 << 20  # bytes of page data + encoder buffers per batch of pages
_TIFF_MAX = 2 ** 32 - 1
_IFD_TAGS = 10


def _page_rows(pages):
    """(Z, H, W) array or tensor of uint8 / uint16 / int32, or (Z, H, W, C) uint8 with C in {1, 3, 4} ->
    ((Z, page bytes) uint8 tensor, bits, sample format, samples per pixel)."""
    import torch
    is_np = isinstance(pages, np.ndarray)
    ok = (np.uint8, np.uint16, np.int32) if is_np else (torch.uint8, torch.uint16, torch.int32)
    grey = pages.ndim == 3 and pages.dtype in ok
    colour = pages.ndim == 4 and pages.dtype == ok[0] and pages.shape[3] in (1, 3, 4)
    if not (grey or colour):
        raise ValueError("write_stack takes (Z, H, W) uint8 / uint16 / int32 or (Z, H, W, C) uint8 with C in {1, 3, 4}, "
                         f"got {tuple(pages.shape)} {pages.dtype}")
    spp = int(pages.shape[3]) if colour else 1
    if is_np:
        fmt = 2 if pages.dtype == np.int32 else 1
        arr = np.ascontiguousarray(pages)
        raw = torch.from_numpy(arr.view(np.uint8).reshape(arr.shape[0], -1) if arr.size else
                               np.zeros((arr.shape[0], 0), np.uint8))
        return raw, 8 * arr.dtype.itemsize, fmt, spp
    t = pages.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1), 8 * t.element_size(), 2 if t.dtype == torch.int32 else 1, spp


def _write_pages(path: str, rows, height: int, width: int, bits: int, sample_format: int,
                 budget_bytes: int = WRITE_STACK_BUDGET, timings=None, samples: int = 1, huffman: str = "fixed") -> None:
    """``rows``: (Z, page_bytes) uint8 tensor on either device, page z = row z in C order, little-endian samples;
    ``samples`` = 3 / 4: chunky RGB / RGBA pixels of 8-bit samples; ``huffman``: see ``deflate.deflate_streams``."""
    import time

    from . import deflate
    n_pages, page_bytes = int(rows.shape[0]), int(rows.shape[1])
    # the keyword goes down only when it is not the default: the call is then the one it always was
    coded = {"huffman": huffman} if deflate.huffman_mode(huffman) else {}
    if samples not in (1, 3, 4) or (samples > 1 and (bits, sample_format) != (8, 1)):
        raise ValueError(f"{samples} samples of {bits} bits per pixel: pages are grey, or 8-bit RGB / RGBA")
    if n_pages < 1 or height * width * samples * (bits // 8) != page_bytes:
        raise ValueError(f"{n_pages} pages of {page_bytes} bytes do not make {height} x {width} x {bits} bit pages"
                         + (f" of {samples} samples" if samples > 1 else ""))
    batch = max(1, int(budget_bytes) // (page_bytes + deflate.device_bytes_per_stream(page_bytes)))
    strips = []
    for lo in range(0, n_pages, batch):
        strips += deflate.deflate_streams(rows[lo:lo + batch], elem_bytes=bits // 8, timings=timings, **coded)
    # layout: header, the strips (each on an even offset), then one directory per page
    offsets, at = [], 8
    for s in strips:
        offsets.append(at)
        at += len(s) + (len(s) & 1)
    # RGB(A): BitsPerSample holds `samples` shorts, more than the 4-byte value field takes; every directory points at
    # one copy of them behind the strips
    bits_at, n_tags = at, _IFD_TAGS
    if samples > 1:
        at += 2 * samples
        n_tags = _IFD_TAGS + (samples == 4)   # PlanarConfiguration in SampleFormat's place; RGBA: + ExtraSamples
    ifd_bytes = 2 + 12 * n_tags + 4
    total = at + n_pages * ifd_bytes
    if total > _TIFF_MAX:
        raise ValueError(f"{path}: {total} bytes do not fit a classic TIFF (32-bit offsets); BigTIFF is not supported")
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, at))
        for s in strips:
            f.write(s)
            if len(s) & 1:
                f.write(b"\0")
        if samples > 1:
            f.write(struct.pack(f"<{samples}H", *([bits] * samples)))
        for z, s in enumerate(strips):
            ifd = at + z * ifd_bytes
            if samples == 1:
                tags = ((256, 4, 1, width), (257, 4, 1, height), (258, 3, 1, bits), (259, 3, 1, 8), (262, 3, 1, 1),
                        (273, 4, 1, offsets[z]), (277, 3, 1, 1), (278, 4, 1, height), (279, 4, 1, len(s)),
                        (339, 3, 1, sample_format))
            else:   # unsigned samples are SampleFormat's default; ExtraSamples 2 = unassociated alpha
                tags = ((256, 4, 1, width), (257, 4, 1, height), (258, 3, samples, bits_at), (259, 3, 1, 8),
                        (262, 3, 1, 2), (273, 4, 1, offsets[z]), (277, 3, 1, samples), (278, 4, 1, height),
                        (279, 4, 1, len(s)), (284, 3, 1, 1)) + (((338, 3, 1, 2),) if samples == 4 else ())
            f.write(struct.pack("<H", len(tags)))
            for tag, typ, count, val in tags:   # a SHORT value sits in the low half of the 4-byte value field
                f.write(struct.pack("<HHII", tag, typ, count, val))
            f.write(struct.pack("<I", ifd + ifd_bytes if z + 1 < n_pages else 0))
    if timings is not None:
        timings["file_s"] = timings.get("file_s", 0.0) + time.perf_counter() - t0


def write_stack(path: str, pages, budget_bytes: int = WRITE_STACK_BUDGET, timings=None, huffman: str = "fixed") -> None:
    """(Z, H, W) uint8 / uint16 / int32 tensor (either device) or array -> multi-page TIFF with Adobe-deflate strips;
    (Z, H, W, C) uint8 with C = 3 / 4 -> RGB / RGBA pages (PhotometricInterpretation 2, SamplesPerPixel C, chunky, C
    BitsPerSample shorts out of line, ExtraSamples 2 for C = 4), and (Z, H, W, 1) is written as grey.

    One directory and one strip per page; tags 256, 257, 258, 259 (= 8), 262 (= 1), 273, 277, 278, 279, 339.  Every
    strip is one zlib stream from :func:`skoots_amd.lib.deflate.deflate_streams`, made on the tensor's device in batches
    of pages that keep page data + encoder buffers under ``budget_bytes``; the compressed strips are held on the host
    until the layout is known.  A file past 2**32 - 1 bytes raises ``ValueError`` before anything is written.
    ``huffman`` (``"fixed" | "dynamic"``) is the code of the strips made on a device, as in ``deflate_streams``."""
    rows, bits, fmt, spp = _page_rows(pages)
    _write_pages(path, rows, int(pages.shape[1]), int(pages.shape[2]), bits, fmt, budget_bytes, timings, samples=spp,
                 huffman=huffman)


def write_float_stack(path: str, pages, budget_bytes: int = WRITE_STACK_BUDGET, timings=None,
                      huffman: str = "fixed") -> None:
    """(Z, H, W) float32 tensor (either device) or array -> multi-page TIFF of 32-bit IEEE samples (SampleFormat 3),
    laid out like ``write_stack``'s pages: one Adobe-deflate strip and one directory per page.  ``write_stack`` and the
    readers of this module keep to integer samples; ImageJ / Fiji and tifffile open these pages as 32-bit float."""
    import torch
    is_np = isinstance(pages, np.ndarray)
    if pages.ndim != 3 or pages.dtype != (np.float32 if is_np else torch.float32):
        raise ValueError(f"write_float_stack takes (Z, H, W) float32, got {tuple(pages.shape)} {pages.dtype}")
    t = torch.from_numpy(np.ascontiguousarray(pages)) if is_np else pages.contiguous()
    rows = t.view(torch.uint8).reshape(t.shape[0], -1) if t.numel() else torch.zeros((t.shape[0], 0), dtype=torch.uint8)
    _write_pages(path, rows, int(t.shape[1]), int(t.shape[2]), 32, 3, budget_bytes, timings, huffman=huffman)


def write_label_stack(path: str, labels_zxy, timings=None, huffman: str = "fixed") -> None:
    """(Z, X, Y) int32 label tensor -> TIFF, uint16 pages while every label is below 65536, int32 otherwise (the
    narrowing ``eval._write_mask_tif`` applies on the host), without leaving the tensor's device."""
    import torch
    t = labels_zxy.contiguous()
    if t.dtype != torch.int32 or t.ndim != 3:
        raise ValueError(f"write_label_stack takes a (Z, X, Y) int32 tensor, got {tuple(t.shape)} {t.dtype}")
    if t.numel() == 0 or int(t.max()) < 65536:
        # the low two bytes of every label: int16 storage holds the uint16 bit patterns
        rows = t.to(torch.int16).view(torch.uint8).reshape(t.shape[0], -1)
        _write_pages(path, rows, int(t.shape[1]), int(t.shape[2]), 16, 1, timings=timings, huffman=huffman)
    else:
        write_stack(path, t, timings=timings, huffman=huffman)
