"""``skoots.lib.eval.eval`` on the MI355X (reference: skoots/lib/eval.py:33-320).

The reference streams 300x300x20 tiles host->GPU->host through zarr arrays and runs
flood fill, offset following and assignment on the CPU.  Here the whole volume stays
resident in HBM (a 2048x2048x512 volume needs ~35 GB of the 288 GB): the image, the
vectors (interleaved fp16x4), the skeleton mask, the labels and the instance mask
never leave the device between stages, tiles are read in place, clamped duplicate
tiles are skipped and stage 3 evaluates every voxel exactly once.

Stage boundaries (and the timed region of ``<image>_skoots_benchmark.txt``) are the
reference's: stage 1 = tiles -> network -> gate/dilate/scatter (eval.py:126-176),
stage 2 = skeleton labelling (:223), stage 3 = follow + assign (:245-284), then
renumber (:304-306).
"""
from __future__ import annotations

import ctypes as C
import logging
import os
import time
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _ffi
from ..profile import ASSIGN_BYTES_PER_VOXEL, GATE_BYTES_PER_VOXEL, maybe_span
from . import cropper
from .flood_fill import label_skeleton
from .tiff import read_image as _read_image  # noqa: F401  (shared with skoots_amd.train.dataloader)
from .vector_to_embedding import step_scales

TILE = (300, 300, 20)          # eval.py:126
TILE_OVERLAP = (50, 50, 5)     # eval.py:127
ASSIGN_CROP = (500, 500, 50)   # eval.py:248
ASSIGN_OVERLAP = (50, 50, 5)   # eval.py:249
PROB_THR = 0.8                 # eval.py:149-150
SKEL_THR = 0.8                 # eval.py:176
FOLLOW_N = 10                  # eval.py:272


def thresholds_for(dtype: torch.dtype) -> Tuple[float, float]:
    """``tensor.gt(0.8)`` compares in the tensor's dtype: the python scalar is cast to
    fp16 for an fp16 network output (autocast path, eval.py:142-150) and to fp32
    otherwise; ``skeleton_map`` is always fp32 (eval.py:146)."""
    prob = float(torch.tensor(PROB_THR, dtype=dtype).float())
    skel = float(torch.tensor(SKEL_THR, dtype=torch.float32))
    return prob, skel


class VolumeState:
    """HBM-resident arrays of one volume, or of one rank's z-window of it (slab + halo).

    ``shape`` is the GLOBAL (X, Y, Z); ``window`` = (w_lo, w_hi) are the planes the local
    arrays cover (the whole volume on one GPU)."""

    def __init__(self, shape: Sequence[int], device, window: Optional[Tuple[int, int]] = None,
                 keep_planar_vectors: bool = False):
        X, Y, Z = (int(s) for s in shape)
        self.shape = (X, Y, Z)
        self.window = (0, Z) if window is None else (int(window[0]), int(window[1]))
        zl = self.window[1] - self.window[0]
        self.local_shape = (X, Y, zl)
        self.device = torch.device(device)
        # vectors: interleaved (X,Y,Zl,4) fp16 -- zero = the never-written frame (eval.py:103)
        self.vec4 = torch.zeros((X, Y, zl, 4), dtype=torch.float16, device=device)
        self.skeleton = torch.zeros((X, Y, zl), dtype=torch.uint8, device=device)  # eval.py:102
        self.vec_planar = (torch.zeros((3, X, Y, zl), dtype=torch.float16, device=device)
                           if keep_planar_vectors else None)
        self.labels: Optional[Tensor] = None
        self.instance: Optional[Tensor] = None
        self.profile = None   # optional skoots_amd.profile.KernelProfile (bench.py: per-stage HBM rooflines)

    # -- stage 1 tail ------------------------------------------------------------------
    def scatter_tile(self, out5: Tensor, origin: Sequence[int], overlap=TILE_OVERLAP,
                     owners: Optional[Sequence[np.ndarray]] = None) -> None:
        """One-tile form of :meth:`scatter_tiles`; ``out5`` is (5, w, h, d)."""
        self.scatter_tiles([out5], [origin], overlap, owners)

    def scatter_tiles(self, tiles: Sequence[Tensor], origins: Sequence[Sequence[int]], overlap=TILE_OVERLAP,
                      owners: Optional[Sequence[np.ndarray]] = None) -> None:
        """Gate + dilate + threshold + interior scatter (eval.py:145-176) of a batch of tile outputs in
        one launch.  ``tiles``: (5, w, h, d) fp16/fp32 tensors that are views of ONE storage with
        identical strides and a contiguous z axis (e.g. ``out5[b]`` of a (B,5,w,h,d) batch, or windows
        of a (5,X,Y,Z) array); ``origins`` in GLOBAL coordinates.

        ``owners`` (per-axis ``cropper.owner_table``): restrict each write to the part of the interior
        the tile writes LAST in the reference's order, so that tiles may be scattered in any order
        (or concurrently on several streams) with the same result."""
        t0 = tiles[0]
        _ffi.require_gpu(t0, "out5") if t0.is_contiguous() else None
        if not t0.is_cuda:
            raise RuntimeError("out5 must live on the MI355X; skoots_amd has no CPU fallback")
        assert t0.ndim == 4 and t0.shape[0] == 5 and t0.stride(3) == 1
        _, w, h, d = t0.shape
        X, Y, zl = self.local_shape
        esz = t0.element_size()
        base = min(t.data_ptr() for t in tiles)
        offs, orgs, los, his = [], [], [], []
        for t, origin in zip(tiles, origins):
            assert t.shape == t0.shape and t.stride() == t0.stride() and t.dtype == t0.dtype
            lo = [int(o) for o in overlap]
            hi = [int(s - o) for s, o in zip((w, h, d), overlap)]
            if owners is not None:
                skip = False
                for ax in range(3):
                    own = np.nonzero(owners[ax] == origin[ax])[0]
                    if own.size == 0:
                        skip = True  # every voxel of this tile's interior is overwritten by later tiles
                        break
                    lo[ax], hi[ax] = int(own[0]) - origin[ax], int(own[-1]) + 1 - origin[ax]
                if skip:
                    continue
            offs.append((t.data_ptr() - base) // esz)
            orgs += [int(origin[0]), int(origin[1]), int(origin[2]) - self.window[0]]
            los += lo
            his += hi
        n = len(offs)
        if n == 0:
            return
        pthr, sthr = thresholds_for(t0.dtype)
        for k in range(0, n, 16):
            m = min(16, n - k)
            written = sum((his[3 * j] - los[3 * j]) * (his[3 * j + 1] - los[3 * j + 1]) * (his[3 * j + 2] - los[3 * j + 2])
                          for j in range(k, k + m))
            with maybe_span(self.profile, "gate_dilate_scatter", self.device, GATE_BYTES_PER_VOXEL * written):
                _ffi.check(_ffi.lib.sk_gate_dilate_scatter(
                    C.c_void_p(base), _ffi.dtype_code(t0), m, (C.c_int64 * m)(*offs[k:k + m]),
                    t0.stride(0), t0.stride(1), t0.stride(2), w, h, d,
                    (C.c_int32 * (3 * m))(*orgs[3 * k:3 * (k + m)]), (C.c_int32 * (3 * m))(*los[3 * k:3 * (k + m)]),
                    (C.c_int32 * (3 * m))(*his[3 * k:3 * (k + m)]), _ffi.ptr(self.vec4), _ffi.ptr(self.vec_planar),
                    _ffi.ptr(self.skeleton), X, Y, zl, pthr, sthr, _ffi.stream_ptr(self.device)))
        self._keep = tiles  # the views must outlive the launch

    # -- stage 2 -----------------------------------------------------------------------
    def label(self) -> Tensor:
        assert self.window == (0, self.shape[2]), "label() is the single-GPU path"
        self.labels = label_skeleton(self.skeleton)
        return self.labels

    # -- stage 3 -----------------------------------------------------------------------
    def assign(self, scale, n: int = FOLLOW_N, decay: float = 1.0, crop=ASSIGN_CROP,
               overlap=ASSIGN_OVERLAP, labels: Optional[Tensor] = None,
               z_range: Optional[Tuple[int, int]] = None) -> Tensor:
        """Follow + assign for the planes ``z_range`` (eval.py:245-284) against the FULL
        (X, Y, Z) label volume; returns ``instance`` int32 (X, Y, planes)."""
        labels = self.labels if labels is None else labels
        assert labels is not None, "run label() first"
        X, Y, Z = self.shape
        assert tuple(labels.shape) == (X, Y, Z), "labels must be the full-volume label array"
        eff = cropper.clamp_crop_(list(crop), (X, Y, Z))
        tables = [cropper.owner_table(dm, c, o) for dm, c, o in zip((X, Y, Z), eff, overlap)]
        z_lo, z_hi = (0, Z) if z_range is None else z_range
        oz = tables[2][z_lo:z_hi]
        oz = oz[oz >= 0]
        if oz.size:
            assert self.window[0] <= oz.min() and oz.max() + eff[2] <= self.window[1], (
                "a stage-3 crop reaches outside the rank's window: increase the halo")
        own = [torch.from_numpy(t).to(self.device) for t in tables]
        self.instance = torch.zeros((X, Y, z_hi - z_lo), dtype=torch.int32, device=self.device)
        sc = step_scales(scale, n, decay)
        with maybe_span(self.profile, "follow_assign", self.device, ASSIGN_BYTES_PER_VOXEL * X * Y * (z_hi - z_lo)):
            _ffi.check(_ffi.lib.sk_follow_assign(
                _ffi.ptr(self.vec4), _ffi.ptr(labels), _ffi.dtype_code(labels), _ffi.ptr(self.instance),
                X, Y, Z, self.window[0], self.window[1], _ffi.ptr(own[0]), _ffi.ptr(own[1]), _ffi.ptr(own[2]),
                eff[0], eff[1], eff[2], _ffi.float_array(sc), n, z_lo, z_hi, _ffi.stream_ptr(self.device)))
        self._own = own  # keep the tables alive until the stream has consumed them
        return self.instance

    # -- renumber ----------------------------------------------------------------------
    def renumber(self, max_label: Optional[int] = None) -> int:
        """In-place relabel of ``instance`` to 1..K by first appearance (eval.py:304-306)."""
        inst = self.instance
        assert inst is not None
        if max_label is None:
            max_label = int(inst.max().item())
        n = inst.numel()
        ws_bytes = _ffi.lib.sk_renumber_workspace_bytes(n, max_label)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        k = torch.zeros(1, dtype=torch.int32, device=self.device)
        _ffi.check(_ffi.lib.sk_renumber(_ffi.ptr(inst), n, max_label, _ffi.ptr(ws), ws_bytes,
                                        _ffi.ptr(k), _ffi.stream_ptr(self.device)))
        return int(k.item())

    def vectors_planar(self) -> Tensor:
        """(3, X, Y, Zl) fp16, the layout of the reference's ``vectors`` array."""
        X, Y, Z = self.local_shape
        out = torch.empty((3, X, Y, Z), dtype=torch.float16, device=self.device)
        _ffi.check(_ffi.lib.sk_vec_deinterleave(_ffi.ptr(self.vec4), _ffi.ptr(out), X * Y * Z,
                                                _ffi.stream_ptr(self.device)))
        return out


def tile_grid(shape: Sequence[int], tile=TILE, overlap=TILE_OVERLAP):
    """Distinct stage-1 tile origins in reference order + the effective tile size."""
    eff = list(tile)
    origins = cropper.distinct_origins(shape, eff, overlap)
    return origins, eff


def eval_volume(image: Tensor, model, scale, mean=None, std=None, n: int = FOLLOW_N,
                tile=TILE, tile_overlap=TILE_OVERLAP, tile_batch: Optional[int] = None,
                inject: Optional[Callable] = None, keep_planar_vectors: bool = False,
                timings: Optional[Dict[str, float]] = None) -> Dict[str, Tensor]:
    """In-memory variant of :func:`eval` on one GPU: (1, X, Y, Z) or (X, Y, Z) image on the
    device -> instance mask, vectors, skeleton, labels (all HBM-resident tensors).

    ``model`` is a :class:`skoots_amd.unet.HipUNet`; ``inject(out5, origin, eff) -> out5``
    may replace a tile's network output (parity tests and bench.py's assignment workload
    use it).  The multi-GPU form is :class:`skoots_amd.parallel.ShardedVolume`.
    ``tile_batch``: tiles per network launch; None = as many as the tile count and the free device memory allow,
    at most 64 (:func:`skoots_amd.parallel.pick_tile_batch`; a tile's output does not depend on its batch).
    """
    from ..parallel import ShardedVolume
    img = image.squeeze(0) if image.ndim == 4 else image
    _ffi.require_gpu(img, "image")
    img16 = img if img.dtype == torch.float16 else img.to(torch.float16)  # eval.py:80
    if mean is None or std is None:
        # eval.py:87-88 fallback: statistics of the fp16 image, evaluated by the same torch
        # CPU reduction the reference uses (outside the timed region).
        cpu = img16.cpu()
        mean = float(cpu.mean()) if mean is None else mean
        std = float(cpu.std()) if std is None else std
    sv = ShardedVolume(tuple(img16.shape), 0, 1, img16.device)
    res = sv.run(img16.contiguous(), model, scale, float(mean), float(std), n=n, tile=tile,
                 tile_overlap=tile_overlap, tile_batch=tile_batch, inject=inject,
                 keep_planar_vectors=keep_planar_vectors)
    if timings is not None:
        timings.update(sv.timings)
    return res


# ----------------------------------------------------------------------------------------
# File-level entry point: same signature and side effects as skoots.lib.eval.eval
# ----------------------------------------------------------------------------------------
def _write_mask_tif(path: str, mask_zxy: np.ndarray) -> None:
    """(Z, X, Y) integer stack -> multi-page TIFF, zlib/deflate compressed (eval.py:309-310)."""
    from PIL import Image
    arr = mask_zxy.astype(np.uint16) if mask_zxy.max() < 65536 else mask_zxy.astype(np.int32)
    pages = [Image.fromarray(p) for p in arr]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression="tiff_adobe_deflate")


# Whether eval() reads its files -- the image and, with used_cached_data, the two zarr stores -- through the device
# readers (tiff.read_stack, zarr_store.load_device: compressed bytes are uploaded and inflated by csrc/inflate.hip) or
# through the host readers and an upload.  The results are the same; DESIGN.md section 16 has the timings behind the default.
READ_ON_DEVICE = False

# The Huffman code of the chunks and pages eval() writes: "fixed" (RFC 1951's fixed code) or "dynamic" (per 16 KiB piece
# the smaller of that and a code built for the piece).  The files inflate to the same arrays; DESIGN.md section 15 has the
# sizes and timings behind the default.
OUTPUT_HUFFMAN = "fixed"


def _to_f32(t: torch.Tensor) -> torch.Tensor:
    """Integer samples as float32, what ``ndarray.astype(np.float32)`` gives; uint16 goes through its bit pattern."""
    if t.dtype == torch.uint16:
        return (t.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)
    return t.to(torch.float32)


def _cfg_get(cfg, section: str, key: str, default=None):
    sec = cfg[section] if isinstance(cfg, dict) else getattr(cfg, section)
    return sec.get(key, default) if isinstance(sec, dict) else getattr(sec, key, default)


DENOISE_HOW = ("median", "mean", "min", "max", "gauss")


def denoise_arguments(denoise) -> dict:
    """``eval``'s ``denoise=(how, (a, b, c))`` as the keywords of ``lib.morphology.filter_volume``: ``how`` one of
    ``DENOISE_HOW``, the three numbers integer radii, or sigmas for ``"gauss"``; checked by ``filter_plan``."""
    from .morphology import filter_plan
    try:
        how, numbers = denoise
        numbers = tuple(numbers)
    except (TypeError, ValueError):
        raise ValueError(f"denoise must be (how, (a, b, c)), got {denoise!r}") from None
    if how not in DENOISE_HOW:
        raise ValueError(f"denoise how = {how!r}, must be one of {DENOISE_HOW}")
    if how == "gauss":
        kwargs = dict(how=how, sigma=numbers)
    else:
        if len(numbers) == 3 and all(isinstance(v, float) and float(v).is_integer() for v in numbers):
            numbers = tuple(int(v) for v in numbers)
        kwargs = dict(how=how, radius=numbers)
    filter_plan(**kwargs)
    return kwargs


EQUALIZE_KEYS = ("how", "tile", "bins", "low", "high", "clip", "target", "top", "interpolate")


def equalize_arguments(equalize) -> dict:
    """``eval``'s ``equalize={"how": ..., ...}`` as the keywords of ``lib.morphology.equalize``, checked by
    ``equalize_plan`` as far as that goes without the image: ``how`` and the keywords that belong to it.  A ``target``
    given as a path must exist; it is read when the image is."""
    from .morphology import equalize_plan
    if not isinstance(equalize, dict) or "how" not in equalize:
        raise ValueError(f"equalize must be a dict of lib.morphology.equalize's keywords with 'how' among them, got {equalize!r}")
    unknown = [k for k in equalize if k not in EQUALIZE_KEYS]
    if unknown:
        raise ValueError(f"equalize takes {EQUALIZE_KEYS}, not {unknown}")
    kwargs = dict(equalize)
    if isinstance(kwargs.get("tile"), list):
        kwargs["tile"] = tuple(kwargs["tile"])
    target = kwargs.get("target")
    if isinstance(target, (str, os.PathLike)):
        if kwargs["how"] != "match":
            raise ValueError(f"how={kwargs['how']!r} takes no target")
        if not os.path.exists(target):
            raise FileNotFoundError(f"equalize target {target} does not exist")
        equalize_plan(**{k: v for k, v in kwargs.items() if k != "target"})
    else:
        equalize_plan(**kwargs)
    return kwargs


def _image_volume(path: str) -> Tensor:
    """The (X, Y, Z) samples of an image file, the channel ``eval`` evaluates: uint16 through its bit pattern"""
    image = _read_image(path)  # [Z, X, Y(, C)]
    image = image[..., np.newaxis] if image.ndim == 3 else image
    image = image.transpose(-1, 1, 2, 0)
    image = image[[2], ...] if image.shape[0] > 3 else image
    raw = np.ascontiguousarray(image[0])
    return torch.from_numpy(raw.view(np.int16)).view(torch.uint16) if raw.dtype == np.uint16 else torch.from_numpy(raw)


@torch.inference_mode()
def eval(image_path: str, checkpoint_path: str, used_cached_data: bool = False, precision: str = "fp16",
         read_on_device: Optional[bool] = None, output_huffman: Optional[str] = None, pyramid: bool = False,
         rescale=None, denoise=None, equalize=None) -> None:
    """Evaluates SKOOTS on an arbitrary image (drop-in for ``skoots.lib.eval.eval``).

    ``precision`` (not in the reference's signature; keyword with the reference's behaviour as default): "fp16" = what the
    reference's fp16 autocast does (eval.py:142); "split" = fp16 hi + lo operand pairs, network outputs within 1e-3 of an
    fp32 forward at about a third of the speed; "mix8" = "split" with the 3x3x3 convs' correction products on the block-scaled fp8
    matrix instruction (same tolerance, ~20 % faster); "fp32" = exact-fp32 matrix instructions (:class:`skoots_amd.unet.HipUNet`).

    Writes next to the image, with the reference's names: ``<base>_skoots_skeleton`` (1,X,Y,Z) u1
    and ``<base>_skoots_vectors`` (3,X,Y,Z) f2 as ``.zarr`` directory stores (zarr v2 layout, zlib codec,
    written by ``zarr_store.save_device``: the zarr package itself is not in this image; chunks and TIFF pages are
    deflated on the device, ``lib/deflate.py``),
    ``<base>_skoots_benchmark.txt`` and ``<base>_instance_mask.tif`` (Z,X,Y), and prints DONE.

    ``read_on_device`` (keyword, not in the reference's signature; ``None`` = the module's ``READ_ON_DEVICE``, which is
    ``False`` until the device readers have been timed against the host ones): with ``True`` the image and, with ``used_cached_data``, the two
    stores are read by ``tiff.read_stack`` / ``zarr_store.load_device`` (compressed bytes go to the device and are inflated
    there) instead of the host readers + an upload; the results do not depend on it.

    ``output_huffman`` (keyword, not in the reference's signature; ``None`` = the module's ``OUTPUT_HUFFMAN``):
    ``"fixed"`` or ``"dynamic"``, the code of the device deflate encoder that writes the two stores and the TIFF.  The
    files differ in size only: they inflate to the same arrays, and the ``.zarray`` text is the same.

    ``pyramid`` (keyword, not in the reference's signature; off by default, and without it every output is byte for
    byte what it was): after the mask is written, also writes ``<base>_skoots.ome.zarr``, one OME-Zarr (NGFF 0.4) group
    of multiscale pyramids made from the tensors still on the device (``utils.pyramid.write_ome_zarr``): the input
    image (integer samples as read, pooled by the rounded mean), ``labels/instances`` (the instance mask, by the most
    frequent id, sparse off) and ``labels/skeleton`` (by the maximum).  The voxel spacing is the checkpoint's
    ``SKOOTS.ANISOTROPY``, (1, 1, 3) without one; ``output_huffman`` applies.  An image that is not uint8 / uint16 (or
    signed with values in 0 .. 65535) is refused before the model runs.

    ``rescale`` (keyword, not in the reference's signature; ``None`` by default, and without it every output is byte
    for byte what it was): ``(fx, fy, fz)``, output voxels per input voxel in this function's (X, Y, Z) order, for an
    image whose voxel size is not the one the model was trained at.  The integer samples as read (uint8 or uint16, or
    signed with values in 0 .. 65535; anything else is refused by name before the model is built) are resampled on the
    device to ``resample_shape((X, Y, Z), rescale)`` with ``lib.morphology.resample(how="auto")`` before the fp16
    conversion, and the statistics fallback is taken from that fp16 image.  The network, labelling, following, the two
    zarr stores (their ``.zarray`` shapes say so: they are intermediates), ``used_cached_data`` and the benchmark file
    all live on the resampled grid.  The instance mask is mapped back with ``how="nearest"`` to exactly the input's
    (X, Y, Z) before it is written.  Its ids are those of the network's grid and are not renumbered, so an instance
    smaller than an input voxel can be missing from the file.  ``rescale=(1, 1, 1)`` takes this path and gives the same
    files.  Together with ``pyramid`` it is refused by name: run ``utils.pyramid`` on the outputs.

    ``denoise`` (keyword, not in the reference's signature; ``None`` by default, and without it every output is byte
    for byte what it was): ``(how, (a, b, c))`` with ``how`` one of ``"median"``, ``"mean"``, ``"min"``, ``"max"`` --
    ``(a, b, c)`` the integer radii along x, y, z -- or ``"gauss"`` -- the three sigmas in voxels.  The integer samples as
    read (uint8 or uint16, or signed with values in 0 .. 65535) are filtered on the device in their own dtype with
    ``lib.morphology.filter_volume(..., border="mirror")``, before ``rescale`` if both are given and before the fp16
    conversion: ``("median", (1, 1, 0))`` is the 3x3x1 median that removes shot noise and hot pixels.  A float image is
    refused by name before the model is built.  ``pyramid=True`` still writes the image as read.

    ``equalize`` (keyword, not in the reference's signature; ``None`` by default, and without it every output is byte
    for byte what it was): a dict of the keywords of ``lib.morphology.equalize`` -- ``{"how": "stretch", "low": 0.5,
    "high": 99.5}``, ``{"how": "equalize", "tile": (64, 64, 16), "clip": 3.0}``, ``{"how": "match", "tile": "slices"}``,
    ``{"how": "match", "target": "train_volume.tif"}`` (a path is read as the image is) -- that brings the grey values of
    the integer image to what ``dataset_mean`` / ``dataset_std`` expect.  It runs on the device in the image's own dtype,
    after ``denoise`` and before ``rescale`` and the fp16 conversion.  A float image is refused by name before the model is
    built.  ``pyramid=True`` still writes the image as read.

    ``checkpoint_path``: ``torch.save``d dict with ``cfg`` (dict/attribute config holding
    ``SKOOTS.VECTOR_SCALING`` and ``MODEL.*``), ``model_state_dict`` and optionally
    ``dataset_mean`` / ``dataset_std`` (eval.py:51-55, 87-88, 99, 117-118).
    """
    from .. import unet
    from . import deflate
    if output_huffman is None:
        output_huffman = OUTPUT_HUFFMAN   # looked up now, so that setting the module's switch takes effect
    deflate.huffman_mode(output_huffman)
    if rescale is not None:
        if pyramid:
            raise ValueError("pyramid=True together with rescale is not built: run skoots_amd.utils.pyramid on the outputs")
        from .morphology import resample_shape
        resample_shape((1, 1, 1), rescale)   # three positive finite numbers, or a ValueError that says so
    if denoise is not None:
        denoise = denoise_arguments(denoise)   # how and its three numbers, or a ValueError that says so
    if equalize is not None:
        equalize = equalize_arguments(equalize)   # how and its keywords, or a ValueError that says so
    before = denoise is not None or equalize is not None   # the integer image is worked on before the network sees it
    start = time.time()
    logging.info(f"Loading model file: {checkpoint_path}")
    checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    if "cfg" not in checkpoint:
        raise RuntimeError("Attempting to evaluate skoots on a legacy model file.")  # eval.py:55
    cfg = checkpoint["cfg"]
    if not torch.cuda.is_available():
        raise RuntimeError("skoots_amd.eval needs an MI355X: there is no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())
    base = os.path.splitext(image_path)[0]

    logging.info(f"Loading image from file: {image_path}")
    from . import tiff, zarr_store
    if read_on_device is None:
        read_on_device = READ_ON_DEVICE   # looked up now, so that setting the module's switch takes effect
    if read_on_device:
        stack = tiff.read_stack(image_path, device)  # [Z, X, Y(, C)], strips inflated on the device
        stack = stack.unsqueeze(-1) if stack.ndim == 3 else stack
        stack = stack.permute(3, 1, 2, 0)
        stack = stack[[2], ...] if stack.shape[0] > 3 else stack  # eval.py:64 -> [C=1, X, Y, Z]
        c, x, y, z = stack.shape
        logging.info(f"Loaded an image with shape: {(c, x, y, z)}, dtype: {stack.dtype}")
        raw_img = stack[0] if pyramid or rescale is not None or before else None
        dev_img = _to_f32(stack[0]).to(torch.float16).contiguous() if rescale is None and not before \
            else None  # eval.py:80
        # the statistics fallback stays the CPU reduction over the same fp16 values: the image comes back for it only
        img16 = dev_img.cpu() if not ("dataset_mean" in checkpoint and "dataset_std" in checkpoint) and \
            rescale is None and not before else None
    else:
        image = _read_image(image_path)  # [Z, X, Y(, C)]
        image = image[..., np.newaxis] if image.ndim == 3 else image
        image = image.transpose(-1, 1, 2, 0)
        image = image[[2], ...] if image.shape[0] > 3 else image  # eval.py:64 -> [C=1, X, Y, Z]
        c, x, y, z = image.shape
        logging.info(f"Loaded an image with shape: {(c, x, y, z)}, dtype: {image.dtype}")
        img16 = torch.from_numpy(np.ascontiguousarray(image[0]).astype(np.float32)).to(torch.float16) \
            if rescale is None and not before else None  # eval.py:80
        dev_img = None
        raw_img = None
        if pyramid or rescale is not None or before:     # the samples as read: uint16 through its bit pattern
            raw = np.ascontiguousarray(image[0])
            raw_img = (torch.from_numpy(raw.view(np.int16)).view(torch.uint16) if raw.dtype == np.uint16
                       else torch.from_numpy(raw))
    if pyramid:
        from ..utils.pyramid import check_spacing
        from .morphology import check_pool_volume
        check_pool_volume(raw_img, "mean", "image")   # refused by name before the model runs
        try:
            aniso = _cfg_get(cfg, "SKOOTS", "ANISOTROPY", None)
        except (KeyError, AttributeError):
            aniso = None
        spacing = check_spacing(aniso if aniso is not None else (1.0, 1.0, 3.0))
    input_shape = (x, y, z)
    denoised = None
    if before:
        # the raw samples go up and are worked on there, in their own dtype; raw_img stays the image as read
        from .morphology import check_pool_volume, pool_source
        if raw_img.dtype.is_floating_point:
            if denoise is not None:
                raise TypeError(f"image is {raw_img.dtype}: denoise filters the integer samples as read (uint8 / uint16), a float "
                                "image is not denoised")
            raise TypeError(f"image is {raw_img.dtype}: equalize transforms the integer samples as read (uint8 / uint16), a "
                            "float image is not equalized")
        check_pool_volume(raw_img, "mean", "image")
        denoised = pool_source(raw_img.to(device), "mean", "image")   # signed samples: 0 .. 65535 or a ValueError
        if denoise is not None:
            from .morphology import check_filter, filter_volume
            check_filter(denoised, border="mirror", name="image", **denoise)
            logging.info(f"Denoising the image: {denoise}")
            denoised = filter_volume(denoised, border="mirror", **denoise)
        if equalize is not None:
            from .morphology import check_equalize, equalize as equalize_volume
            if isinstance(equalize.get("target"), (str, os.PathLike)):
                target = _image_volume(equalize["target"])
                check_pool_volume(target, "mean", "equalize target")
                equalize = dict(equalize, target=pool_source(target.to(device), "mean", "equalize target"))
            check_equalize(denoised, name="image", **equalize)
            logging.info("Equalizing the image: " + ", ".join(f"{k}={v!r}" for k, v in equalize.items() if k != "target"))
            denoised = equalize_volume(denoised, **equalize)
        if rescale is None:
            dev_img = _to_f32(denoised).to(torch.float16).contiguous()
            img16 = dev_img.cpu() if not ("dataset_mean" in checkpoint and "dataset_std" in checkpoint) else None
            denoised = None
    if rescale is not None:
        # the raw samples go up and are resampled there; everything below lives on the resampled grid
        from .morphology import check_pool_volume, check_resample, pool_source, resample
        x, y, z = resample_shape(input_shape, rescale)
        check_pool_volume(raw_img, "mean", "image")                  # float images are refused by name, as pool refuses them
        raw_dev = denoised if denoised is not None else \
            pool_source(raw_img.to(device), "mean", "image")         # signed samples: 0 .. 65535 or a ValueError
        check_resample(raw_dev, (x, y, z), "auto", "image")
        logging.info(f"Rescaling the image from {input_shape} to {(x, y, z)}")
        dev_img = _to_f32(resample(raw_dev, shape=(x, y, z), how="auto")).to(torch.float16).contiguous()
        del raw_dev, denoised
        img16 = dev_img.cpu() if not ("dataset_mean" in checkpoint and "dataset_std" in checkpoint) else None
    mean = checkpoint["dataset_mean"] if "dataset_mean" in checkpoint else img16.mean()  # eval.py:87
    std = checkpoint["dataset_std"] if "dataset_std" in checkpoint else img16.std()  # eval.py:88
    scale = [int(v) for v in _cfg_get(cfg, "SKOOTS", "VECTOR_SCALING")]  # eval.py:99

    logging.info("Constructing SKOOTS model")
    model = unet.cfg_to_model(cfg, device, checkpoint["model_state_dict"], precision=precision)
    skel_path, vec_path = base + "_skoots_skeleton.zarr", base + "_skoots_vectors.zarr"  # eval.py:102-103

    benchmark_start = time.time()
    if dev_img is None:
        dev_img = img16.to(device)
    if used_cached_data and os.path.exists(skel_path) and os.path.exists(vec_path):  # eval.py:105 (os.exists bug fixed)
        from ..parallel import ShardedVolume  # noqa: F401
        state = VolumeState((x, y, z), device)
        if read_on_device:   # chunk files go up as they are and are inflated on the device
            state.skeleton.copy_(zarr_store.load_device(skel_path, device)[0])
            vp = zarr_store.load_device(vec_path, device)
        else:
            state.skeleton.copy_(torch.from_numpy(zarr_store.load(skel_path)[0]).to(device))
            vp = torch.from_numpy(zarr_store.load(vec_path)).to(device)
        _ffi.check(_ffi.lib.sk_vec_interleave(_ffi.ptr(vp), _ffi.ptr(state.vec4), x * y * z,
                                              _ffi.stream_ptr(device)))
        state.label()
        state.assign(scale)
        state.renumber()
        inst, vectors, skeleton = state.instance, vp, state.skeleton
    else:
        res = eval_volume(dev_img, model, scale, mean=float(mean), std=float(std))
        inst, skeleton = res["instance_mask"], res["skeleton"]
        vectors = res["state"].vectors_planar()
    torch.cuda.synchronize(device)
    dt = time.time() - benchmark_start

    # deflated on the device: only compressed bytes leave it
    zarr_store.save_device(skel_path, skeleton.unsqueeze(0), huffman=output_huffman)
    zarr_store.save_device(vec_path, vectors, huffman=output_huffman)
    logging.info("writing benchmark information")
    with open(base + "_skoots_benchmark.txt", "w") as f:  # eval.py:286-295
        f.write("SKOOTS Segmentation Benchmark:\n")
        f.write("------------------------------\n")
        f.write(f"Time: {dt} seconds\n")
        f.write(f"Memory (current/max): ({torch.cuda.memory_allocated(device)}, "
                f"{torch.cuda.max_memory_allocated(device)})\n\n")
    print("DONE")
    logging.info(f"saving to tif file at {base}_instance_mask.tif")
    if rescale is not None:   # back onto the input's grid: the ids of the network's grid, not renumbered
        inst = resample(inst, shape=input_shape, how="nearest")
    tiff.write_label_stack(base + "_instance_mask.tif", inst.permute(2, 0, 1), huffman=output_huffman)
    if pyramid:
        from ..utils.pyramid import write_ome_zarr
        logging.info(f"saving multiscale pyramids to {base}_skoots.ome.zarr")
        write_ome_zarr(base + "_skoots.ome.zarr", spacing, image=raw_img.to(device),
                       labels={"instances": inst, "skeleton": (skeleton, "max")}, huffman=output_huffman)
    elapsed = time.time() - start
    logging.info(f"DONE: Process took {elapsed} seconds, {elapsed / 60} minutes, {elapsed / (60 ** 2)}, hours")
