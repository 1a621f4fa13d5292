"""``python -m skoots_amd --convert PATH``: ``eval()``'s zarr stores and ``.trch`` tensors -> multi-page TIFF stacks any
image viewer opens (skoots/utils/convert_trch_to_tif.py:11-76): the vector field as an RGB stack, the skeleton as a
0 / 255 mask.

The array is read to a device, transformed and transposed there (one pass of ``sk_convert_pages_u8`` for the 4-D
uint8 / fp16 / fp32 arrays ``eval()`` writes, the reference's own chain of torch operations for everything else) and
deflated there by ``tiff.write_stack``: only compressed bytes leave the device.

Deliberate differences from the reference:
  1. a directory is searched for ``*.zarr`` stores as well as ``*.trch`` files (``discover``);
  2. a ``.trch`` file that holds no tensor is skipped with a log line (``convert``);
  3. every output is deflate-compressed (``tiff.write_stack`` writes nothing else);
  4. ``(Z, X, Y, 1)`` pages are written as grey pages (``tiff.write_stack``).
"""
from __future__ import annotations

import glob
import logging
import os
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

MODE_CAST, MODE_TRUNC, MODE_ROUND = 0, 1, 2   # SK_CONVERT_CAST / _TRUNC / _ROUND of include/skoots_hip.h
_KERNEL_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}   # SK_CONVERT_U8 / _F16 / _F32
_PAGE_DTYPES = ("uint8", "uint16", "int32")   # what tiff.write_stack takes


class ConversionPlan(NamedTuple):
    mode: Optional[int]        # value transform (MODE_*), or None: the values are kept as they are
    perm: Tuple[int, ...]      # pages = x.permute(perm)
    out_dtype: str             # dtype of the pages: "uint8" after a transform, the array's own otherwise


def _dtype_name(dtype) -> str:
    if isinstance(dtype, torch.dtype):
        return str(dtype).replace("torch.", "")
    return dtype if isinstance(dtype, str) else np.dtype(dtype).name


def plan_conversion(kind: str, ndim: int, dtype, vmin, vmax) -> Optional[ConversionPlan]:
    """What the reference does to an array of file kind ``kind`` (``"zarr"`` / ``"trch"``), rank ``ndim``, ``dtype``
    (torch or numpy dtype, or its name) and minimum / maximum ``vmin`` / ``vmax``; ``None`` where it writes no file
    (a rank other than 3 and 4).  A store looks at ``vmax`` only and only in 4-D, a tensor at ``vmin`` only: the other
    one may be ``None``.

      store, 3-D             transpose(2, 0, 1), dtype kept                              (:43-45)
      store, 4-D, max < 2    mode 1, transpose(3, 1, 2, 0), uint8                        (:48-55)
      store, 4-D, max >= 2   mode 0 = astype(np.uint8), transpose(3, 1, 2, 0)            (:55)
      tensor, min < 0        mode 2, uint8, permute(2, 0, 1) / permute(3, 1, 2, 0)       (:59-65)
      tensor, min >= 0       permute only, dtype kept                                    (:68-74)
    """
    if kind not in ("zarr", "trch"):
        raise ValueError(f"kind = {kind!r}, must be 'zarr' or 'trch'")
    if ndim not in (3, 4):
        return None
    perm = (2, 0, 1) if ndim == 3 else (3, 1, 2, 0)
    name = _dtype_name(dtype)
    if kind == "zarr":
        if ndim == 3:
            return ConversionPlan(None, perm, name)
        return ConversionPlan(MODE_TRUNC if vmax < 2 else MODE_CAST, perm, "uint8")
    if vmin < 0:
        return ConversionPlan(MODE_ROUND, perm, "uint8")
    return ConversionPlan(None, perm, name)


def _low8(t: torch.Tensor) -> torch.Tensor:
    """numpy's ``astype(np.uint8)``: truncate toward zero, keep the low 8 bits.  Outside [0, 256) the reference's
    result is not defined (a C cast); this is what x86 gives for everything an int32 holds."""
    if t.dtype == torch.uint8:
        return t
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if t.is_floating_point():
        t = t.to(torch.int32)
    elif t.dtype in (torch.uint16, torch.uint32, torch.uint64):
        t = t.to(torch.int64)
    return (t & 255).to(torch.uint8)


def values_torch(x: torch.Tensor, mode: int) -> torch.Tensor:
    """The value transform of ``mode`` as the reference's own torch operations, on ``x``'s device: uint8, ``x``'s shape."""
    if mode == MODE_CAST:
        return _low8(x)
    t = x.add(1).div(2).mul(255)             # :51 / :63; every operation rounds in the array's own float type
    if mode == MODE_ROUND:
        t = t.float().round()
    return _low8(t).masked_fill(x == 0, 0)   # :50-52 / :61-65


def pages_torch(x: torch.Tensor, mode: Optional[int]) -> torch.Tensor:
    """Pages of a 3-D / 4-D array by torch operations: transform (``mode`` not None), then the reference's permute."""
    perm = (2, 0, 1) if x.ndim == 3 else (3, 1, 2, 0)
    return (x if mode is None else values_torch(x, mode)).permute(perm).contiguous()


def pages_kernel(x: torch.Tensor, mode: int) -> torch.Tensor:
    """(C, X, Y, Z) uint8 / fp16 / fp32 on a GPU -> (Z, X, Y, C) uint8 pages, one pass of ``sk_convert_pages_u8``."""
    from .. import _ffi
    _ffi.require_gpu(x, "pages_kernel: x")
    if x.ndim != 4 or x.dtype not in _KERNEL_DTYPES:
        raise ValueError(f"pages_kernel takes a (C, X, Y, Z) uint8 / fp16 / fp32 tensor, got {tuple(x.shape)} {x.dtype}")
    C, X, Y, Z = (int(s) for s in x.shape)
    out = torch.empty((Z, X, Y, C), dtype=torch.uint8, device=x.device)
    _ffi.check(_ffi.lib.sk_convert_pages_u8(_ffi.ptr(x), _KERNEL_DTYPES[x.dtype], int(mode), C, X, Y, Z, _ffi.ptr(out),
                                            _ffi.stream_ptr(x.device)))
    return out


def make_pages(x: torch.Tensor, plan: ConversionPlan) -> torch.Tensor:
    """Pages of ``x`` under ``plan`` on ``x``'s device.  On a GPU the kernel takes every 4-D uint8 / fp16 / fp32 array
    with a transform, the 4-D uint8 tensor without one (mode 0 on uint8 is a pure transpose) and the 3-D tensor with
    negatives (C = 1: its (Z, X, Y, 1) pages are the (Z, X, Y) ones); both routes give the same bytes."""
    kernel = x.is_cuda and x.dtype in _KERNEL_DTYPES and x.numel() > 0
    if kernel and x.ndim == 4 and (plan.mode is not None or x.dtype == torch.uint8):
        return pages_kernel(x.contiguous(), MODE_CAST if plan.mode is None else plan.mode)
    if kernel and x.ndim == 3 and plan.mode is not None:
        return pages_kernel(x.contiguous().unsqueeze(0), plan.mode).squeeze(3)
    return pages_torch(x, plan.mode)


def discover(base_dir: str) -> List[str]:
    """Files to convert (:12-18): a path ending in ``.zarr`` or a plain file is itself, a path containing ``*`` is the
    glob, any other directory is its ``*.zarr`` stores and ``*.trch`` files, sorted.

    Difference 1: the reference globs a directory for ``*.trch`` only, which predates ``eval()`` writing zarr stores, so
    its help text ("all skoots eval outputs in directory") no longer holds there."""
    if os.path.isdir(base_dir) and not base_dir.rstrip("/\\").endswith(".zarr"):
        return sorted(glob.glob(os.path.join(base_dir, "*.zarr")) + glob.glob(os.path.join(base_dir, "*.trch")))
    if "*" in base_dir:
        return sorted(glob.glob(base_dir))
    return [base_dir]


def _check_pages(f: str, shape, plan: ConversionPlan) -> None:
    if len(shape) == 4 and shape[0] not in (1, 3, 4):
        raise ValueError(f"{f}: {shape[0]} channels cannot be written as TIFF pages (1 = grey, 3 = RGB, 4 = RGBA)")
    if plan.out_dtype not in _PAGE_DTYPES or (len(shape) == 4 and shape[0] > 1 and plan.out_dtype != "uint8"):
        raise ValueError(f"{f}: pages of dtype {plan.out_dtype} and shape {tuple(shape[i] for i in plan.perm)} cannot be "
                         "written (grey pages are uint8 / uint16 / int32, RGB(A) pages uint8)")


def convert(base_dir: str, device=None, read_on_device: Optional[bool] = None,
            huffman: Optional[str] = None) -> List[str]:
    """Converts every store / tensor ``discover(base_dir)`` finds to ``os.path.splitext(f)[0] + ".tif"``; returns the
    files written.  ``device``: where the work happens (default: the current GPU if there is one, else ``"cpu"``).
    ``read_on_device``: stores are read with ``zarr_store.load_device`` (chunks inflated on the device) instead of
    ``zarr_store.load`` + upload; ``None`` = ``skoots_amd.lib.eval.READ_ON_DEVICE`` at the time of the call.
    ``huffman``: the code of the strips ``tiff.write_stack`` makes on a device (``"fixed" | "dynamic"``); ``None`` =
    ``skoots_amd.lib.eval.OUTPUT_HUFFMAN`` at the time of the call."""
    from ..lib import deflate, tiff, zarr_store
    if huffman is None:
        from ..lib import eval as E
        huffman = E.OUTPUT_HUFFMAN
    deflate.huffman_mode(huffman)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    if read_on_device is None:
        from ..lib import eval as E
        read_on_device = E.READ_ON_DEVICE
    files = [f for f in discover(base_dir) if os.path.exists(f)]
    print(f"Found {len(files)} files to convert:")
    for f in files:
        print(f"-->  {f}")
    print("------")
    written = []
    for f in files:
        is_store = f.rstrip("/\\").endswith(".zarr")
        if is_store:
            x = zarr_store.load_device(f, device) if read_on_device else torch.from_numpy(zarr_store.load(f)).to(device)
        else:
            obj = torch.load(f, map_location="cpu", weights_only=True)
            if not isinstance(obj, torch.Tensor):
                # difference 2: the reference raises AttributeError at print(x.shape) (:36) for a checkpoint or a
                # *.skeletons.trch dict, before it reaches its own isinstance check (:38)
                logging.info(f"convert: {f} holds a {type(obj).__name__}, no tensor: skipped")
                print(f"Skipping {f} (no tensor)")
                continue
            x = obj.to(device)
        if x.ndim not in (3, 4) or x.numel() == 0:
            logging.info(f"convert: {f} has shape {tuple(x.shape)}: nothing to write")   # as the reference: no file
            continue
        # min / max are reductions on the device; a store needs its maximum only in 4-D, a tensor its minimum
        vmax = x.max().item() if is_store and x.ndim == 4 else None
        vmin = x.min().item() if not is_store else None
        plan = plan_conversion("zarr" if is_store else "trch", x.ndim, x.dtype, vmin, vmax)
        _check_pages(f, tuple(x.shape), plan)
        new_file = os.path.splitext(f.rstrip("/\\"))[0] + ".tif"
        print(f"Converting {f} {tuple(x.shape)} {_dtype_name(x.dtype)} -> {new_file}")
        pages = make_pages(x, plan)
        del x
        if pages.ndim == 4 and pages.shape[3] == 1:
            # difference 4: (Z, X, Y, 1) is written as grey pages; what tifffile makes of that shape is not pinned
            pages = pages.squeeze(3)
        tiff.write_stack(new_file, pages, huffman=huffman)    # difference 3: deflate strips; the reference leaves 4-D outputs uncompressed
        written.append(new_file)
    return written
