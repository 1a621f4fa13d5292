"""``python -m skoots_amd.utils.flood_and_stitch image.tif [-d DIM]``: a one-label semantic mask -> a 3-D instance mask
(skoots/utils/flood_and_stitch.py).  Every 2-D slice along ``DIM`` is flood-filled on its own, then two greedy passes
(forwards, backwards) stitch the slices' components into objects by their largest overlap.

Three stages, each callable on its own:

  ``label_planes``     all slices at once: ``sk_label_planes`` on a GPU, ``scipy.ndimage.label`` per slice on ``"cpu"``
  ``plane_overlaps``   voxel counts of every pair of components of adjacent slices: ``sk_plane_overlaps`` / ``numpy.unique``
  ``stitch_tables``    the reference's two passes played on those tables (``sk_stitch_walk_host``, plain C++, either route)

and the result is one ``sk_relabel_lut`` pass plus ``renumber_first_seen``.  The reference's quirks are kept: the numbering
restarts in every slice, the first new id of a pass equals the largest id present, and a component of the next slice that
happens to carry the same number as ``u`` counts as "already the same object".
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np
import torch

from .renumber import narrow, renumber_first_seen

MAX_VOXELS = 2 ** 31 - 1 - 4096   # int32 voxel indices and ids inside sk_label_planes


def _check_mask(mask, dim) -> torch.Tensor:
    if isinstance(mask, np.ndarray):
        if mask.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"mask dtype must be uint8 or bool, not {mask.dtype}")
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a torch tensor or a numpy array, not {type(mask).__name__}")
    if mask.ndim != 3:
        raise ValueError(f"mask must have 3 axes, not shape {tuple(mask.shape)}")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask dtype must be uint8 or bool, not {mask.dtype}")
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 0 <= dim <= 2:
        raise ValueError(f"dim must be 0, 1 or 2, not {dim!r}")
    if mask.numel() > MAX_VOXELS:
        raise ValueError(f"a volume of shape {tuple(mask.shape)} has more than {MAX_VOXELS} voxels: the plane ids and "
                         "the relabel table are int32")
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _planes_first(t: torch.Tensor, dim: int) -> torch.Tensor:
    """(A0, A1, A2) -> the (P, H, W) view whose planes are the slices along ``dim``, rows / columns in the slice's own
    C order (what ``scipy.ndimage.label`` sees)."""
    return t.permute((0, 1, 2) if dim == 0 else (1, 0, 2) if dim == 1 else (2, 0, 1))


def _planes_back(t: torch.Tensor, dim: int) -> torch.Tensor:
    return t.permute((0, 1, 2) if dim == 0 else (1, 0, 2) if dim == 1 else (1, 2, 0))


def _strides(t: torch.Tensor):
    """Element strides for the kernels: an axis of extent 1 may carry any stride (0 after ``array[None]``), and is never
    stepped along."""
    return tuple(int(s) if n > 1 else 1 for s, n in zip(t.stride(), t.shape))


def _label_view_device(m: torch.Tensor, out: torch.Tensor):
    """``sk_label_planes`` on the (P, H, W) views ``m`` (uint8) and ``out`` (int32), whatever their strides."""
    from .. import _ffi
    P, H, W = (int(s) for s in m.shape)
    ws_bytes = _ffi.lib.sk_label_planes_workspace_bytes(P, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=m.device)
    offsets = torch.empty(P + 1, dtype=torch.int32, device=m.device)
    total = torch.empty(1, dtype=torch.int32, device=m.device)
    _ffi.check(_ffi.lib.sk_label_planes(_ffi.ptr(m), P, H, W, *_strides(m), _ffi.ptr(out), *_strides(out), _ffi.ptr(offsets),
                                        _ffi.ptr(total), _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(m.device)))
    return offsets


def _label_view_cpu(m: torch.Tensor, out: torch.Tensor):
    from scipy import ndimage
    P = int(m.shape[0])
    offsets = np.zeros(P + 1, dtype=np.int32)
    mv, ov = m.numpy(), out.numpy()
    for p in range(P):
        lab, k = ndimage.label(mv[p] > 0)
        ov[p] = np.where(lab > 0, lab + offsets[p], 0)
        offsets[p + 1] = offsets[p] + k
    return torch.from_numpy(offsets)


def _label_view(m: torch.Tensor, out: torch.Tensor):
    if m.numel() == 0:
        return torch.zeros(int(m.shape[0]) + 1, dtype=torch.int32, device=m.device)
    return _label_view_device(m, out) if m.is_cuda else _label_view_cpu(m, out)


def label_planes(mask, dim: int, strided: bool = False):
    """Labels every slice of ``mask`` along ``dim`` on its own (4-connected).  Returns ``(labels, offsets)``: int32
    labels of the mask's shape with GLOBAL ids -- slice ``p`` owns ``offsets[p] + 1 .. offsets[p + 1]``, numbered inside
    the slice as scipy numbers them -- and the ``shape[dim] + 1`` int32 offsets, both on the mask's device.

    On a GPU the kernels run on the volume in place through strides; for ``dim == 2`` (lanes would stride by the row
    length) a permuted contiguous copy is labelled and permuted back, unless ``strided`` asks for the in-place route."""
    mask = _check_mask(mask, dim).contiguous()
    if mask.is_cuda and dim == 2 and not strided:
        m = _planes_first(mask, dim).contiguous()
        out = torch.empty(m.shape, dtype=torch.int32, device=m.device)
        offsets = _label_view(m, out)
        return _planes_back(out, dim).contiguous(), offsets
    labels = torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
    offsets = _label_view(_planes_first(mask, dim), _planes_first(labels, dim))
    return labels, offsets


def _overlaps_once(lab: torch.Tensor, capacity: int):
    """One run of ``sk_plane_overlaps`` on the (P, H, W) int32 view ``lab`` with a table of ``capacity`` slots.  Returns
    ``(rows, needed, complete)``: the (R, 3) rows found (unsorted), the number of pairs the kernel counted -- exact when
    ``complete``, otherwise not less than the number there is -- and whether every pair found a slot."""
    from .. import _ffi
    P, H, W = (int(s) for s in lab.shape)
    ws_bytes = _ffi.lib.sk_plane_overlaps_workspace_bytes(capacity)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=lab.device)
    rows = torch.empty((capacity, 3), dtype=torch.int32, device=lab.device)
    counts = torch.zeros(4, dtype=torch.int32, device=lab.device)
    _ffi.check(_ffi.lib.sk_plane_overlaps(_ffi.ptr(lab), P, H, W, *_strides(lab), _ffi.ptr(rows), capacity, _ffi.ptr(counts),
                                          _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(lab.device)))
    stored, refused, written = (int(v) for v in counts[:3].tolist())
    assert written == stored
    return rows[:written], stored + refused, refused == 0


def _sort_rows(rows: torch.Tensor) -> torch.Tensor:
    if rows.shape[0] == 0:
        return rows.reshape(0, 3)
    key = rows[:, 0].to(torch.int64) * (1 << 32) + rows[:, 1].to(torch.int64)
    return rows[torch.argsort(key)].contiguous()


def _overlaps_view(lab: torch.Tensor, total: int, capacity=None) -> torch.Tensor:
    P = int(lab.shape[0])
    if P < 2 or total == 0 or lab.numel() == 0:
        return torch.zeros((0, 3), dtype=torch.int32, device=lab.device)
    if lab.is_cuda:
        # sizing rule: a component usually overlaps one or two of the next slice, so 3 slots per component keep the
        # table under half full; a table that turns out too small is counted, not guessed, and run once more
        capacity = int(capacity) if capacity else max(1024, 3 * total)
        while True:
            rows, needed, complete = _overlaps_once(lab, capacity)
            if complete:
                return _sort_rows(rows)
            # `needed` counts a refused pair once per corner of its overlap region, far too many on a noisy volume:
            # a rerun grows the table by at most 64 x, so its memory follows the pairs there are, not that count
            capacity = min(max(2 * needed, 2 * capacity), 64 * capacity)
    a = lab[:-1].numpy().reshape(-1).astype(np.int64)
    b = lab[1:].numpy().reshape(-1).astype(np.int64)
    both = (a > 0) & (b > 0)
    keys, n = np.unique(a[both] << 32 | b[both], return_counts=True)
    rows = np.stack([keys >> 32, keys & 0xFFFFFFFF, n], axis=1).astype(np.int32).reshape(-1, 3)
    return torch.from_numpy(rows)


def plane_overlaps(labels: torch.Tensor, offsets: torch.Tensor, dim: int, capacity=None) -> torch.Tensor:
    """(R, 3) int32 rows ``(id_a, id_b, n)``, sorted by ``(id_a, id_b)``: component ``id_a`` of slice ``p`` and ``id_b`` of
    slice ``p + 1`` (ids of ``label_planes``) share ``n`` voxel positions.  On the labels' device.  ``capacity``: slots of
    the first table on a GPU (default: three per component); a table that is too small is run again larger."""
    if labels.ndim != 3 or labels.dtype != torch.int32 or not 0 <= dim <= 2:
        raise ValueError("plane_overlaps takes the int32 labels of label_planes and their dim")
    lab = _planes_first(labels.contiguous(), dim)
    if labels.is_cuda and dim == 2:
        lab = lab.contiguous()
    return _overlaps_view(lab, int(offsets[-1]), capacity)


def stitch_tables(offsets, rows):
    """The reference's two stitching passes on tables (``sk_stitch_walk_host``).  ``offsets``: P + 1 ints, ``rows``:
    (R, 3) sorted by the first two columns.  Returns ``(lut, max_label)``: the int32 CPU tensor that maps a global
    component id (0 kept) to the label it carries after both passes, and the largest of them."""
    from .. import _ffi
    off = np.ascontiguousarray(torch.as_tensor(offsets).cpu().numpy(), dtype=np.int32)
    r = np.ascontiguousarray(torch.as_tensor(rows).cpu().numpy(), dtype=np.int32).reshape(-1, 3)
    if off.ndim != 1 or off.size < 2:
        raise ValueError("offsets must hold P + 1 entries")
    lut = np.zeros(int(off[-1]) + 1 if off[-1] >= 0 else 1, dtype=np.int32)
    mx = C.c_int32(0)
    rc = _ffi.lib.sk_stitch_walk_host(off.ctypes.data_as(_ffi.ip), off.size - 1, r.ctypes.data_as(_ffi.ip), r.shape[0],
                                      lut.ctypes.data_as(_ffi.ip), C.byref(mx))
    _ffi.check(rc)
    return torch.from_numpy(lut), int(mx.value)


def _apply_lut(labels: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """labels[i] = lut[labels[i]] on the contiguous int32 ``labels`` (in place on a GPU)."""
    if labels.is_cuda:
        from .. import _ffi
        lut_d = lut.to(labels.device)
        _ffi.check(_ffi.lib.sk_relabel_lut(_ffi.ptr(labels), labels.numel(), _ffi.ptr(lut_d), lut_d.numel(),
                                           _ffi.stream_ptr(labels.device)))
        return labels
    return lut[labels.long()]


def watershed_and_stitch(mask, dim: int) -> torch.Tensor:
    """skoots/utils/flood_and_stitch.py:38-133.  ``mask``: 3-axis uint8 / bool tensor or array, foreground = nonzero;
    the work runs where the tensor lives.  Returns int32 labels of the same shape, 1..K in order of first appearance."""
    mask = _check_mask(mask, dim).contiguous()
    if mask.numel() == 0:
        return torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
    permuted = mask.is_cuda and dim == 2
    m = _planes_first(mask, dim)
    if permuted:
        m = m.contiguous()    # lanes along the slice's columns: one copy in, one copy out
        lab = torch.empty(m.shape, dtype=torch.int32, device=m.device)
        store = lab
    else:
        store = torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
        lab = _planes_first(store, dim)
    offsets = _label_view(m, lab)
    total = int(offsets[-1])
    if total > 0 and mask.shape[dim] > 1:
        rows = _overlaps_view(lab, total)
        lut, _ = stitch_tables(offsets, rows)
        # the stitched ids run up to components + renames: their ranks (1..K) keep sk_renumber's table at K entries
        uniq, inverse = torch.unique(lut[1:], return_inverse=True)
        lut[1:] = inverse.to(torch.int32) + 1
        store = _apply_lut(store, lut)
        k = int(uniq.numel())
    else:
        k = total   # :71  one slice: the flood fill is the answer, and its numbering is already by first appearance
    out = _planes_back(store, dim).contiguous() if permuted else store
    return renumber_first_seen(out, k)


def flood_stitch_save(path: str, dim: int = 0, device=None) -> str:
    """Reads the TIFF ``path`` as (Z, X, Y), thresholds ``> 0``, stitches along ``dim`` and writes the labels, in the
    narrowest of uint8 / uint16 / int32 that holds them, to ``path`` with ``.tif`` replaced by ``_replaced.tif``.
    ``device``: the current GPU if there is one, else ``"cpu"``.  Returns the path written."""
    from ..lib import tiff
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} does not exist")
    out_path = path.replace(".tif", "_replaced.tif")
    if out_path == path:
        raise ValueError(f"{path}: the output name replaces '.tif' in the input's name, which has none")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    im = tiff.read_stack(path, device)
    if im.ndim != 3:
        raise ValueError(f"{path}: expected a (Z, X, Y) stack, got shape {tuple(im.shape)}")
    logging.info("loaded %s with shape %s and dtype %s", path, tuple(im.shape), im.dtype)
    if im.dtype in (torch.uint16, torch.uint32):
        im = im.to(torch.int64)   # torch compares no wider unsigned types
    try:
        labels = watershed_and_stitch((im > 0).to(torch.uint8), dim)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    k = int(labels.max()) if labels.numel() else 0
    logging.info("found %d objects", k)
    tiff.write_stack(out_path, narrow(labels, k))
    return out_path


def main(argv=None) -> str:
    import argparse

    parser = argparse.ArgumentParser(
        prog="skoots_amd.utils.flood_and_stitch",
        description="Takes a 3D image of a semantic mask with one label (0 is background, anything else foreground), flood "
                    "fills each slice along one dimension, then stitches the slices into a 3D instance mask.")
    parser.add_argument("image_path", type=str, help="input image tif")
    parser.add_argument("-d", "--dimension", type=int, default=0, help="spatial dimension to slice over. default=0")
    parser.add_argument("--distance", action="store_true", help="accepted and ignored, as the reference ignores it")
    parser.add_argument("--log", type=int, default=3, help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    args = parser.parse_args(argv)
    levels = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]
    if not 0 <= args.log < len(levels):
        parser.error(f"--log must be 0..{len(levels) - 1}")
    logging.basicConfig(level=levels[args.log], force=True,
                        format="[%(asctime)s] skoots_amd/utils/flood_and_stitch.py [%(levelname)s]: %(message)s")
    if args.distance:
        import warnings
        warnings.warn("--distance has no effect: the reference parses it and never applies a distance transform, and "
                      "neither does this tool", stacklevel=1)
    out = flood_stitch_save(args.image_path, args.dimension)
    print(f"Saved to path: {out}", flush=True)
    return out


if __name__ == "__main__":
    main()
