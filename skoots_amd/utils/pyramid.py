"""``python -m skoots_amd.utils.pyramid [--image I.tif] [--labels M.tif ...] [--skeleton S.zarr] --spacing SX SY SZ
[--levels N] [--until N] [--sparse] [--output-huffman fixed|dynamic] [-o OUT.ome.zarr]``: multiscale pyramids of an
image, its instance masks and its skeleton, written as one OME-Zarr (NGFF 0.4) group that napari, neuroglancer and the
Fiji / MoBIE plug-ins open interactively at the sizes ``eval()`` works at.

    python -m skoots_amd.utils.pyramid --image I.tif --labels I_instance_mask.tif --spacing 1 1 3
    python -m skoots_amd.utils.pyramid --labels I_instance_mask.tif --sparse --spacing 1 1 3 -o I_masks.ome.zarr
    python -m skoots_amd.utils.pyramid --image I.tif --skeleton I_skoots_skeleton.zarr --spacing 1 1 3 --levels 4

Every level is one launch of ``lib.morphology.pool`` on the level before it: images by the
rounded mean, label volumes by the most frequent id (``--sparse``: zeros do not vote, thin instances survive), the
skeleton by the maximum.  ``plan_pyramid`` decides the factors of every level from the voxel spacing alone, so an
anisotropic volume is halved in x and y until its voxels are about cubic, then in all three.  The reference has no
counterpart."""
from __future__ import annotations

import math
import os
import shutil
import time
from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor


class Level(NamedTuple):
    """One level of a plan: the factors that made it from the level before (``(1, 1, 1)`` for level 0), its (X, Y, Z)
    shape and its (sx, sy, sz) spacing"""
    factors: Tuple[int, int, int]
    shape: Tuple[int, int, int]
    spacing: Tuple[float, float, float]


def check_spacing(spacing) -> Tuple[float, float, float]:
    try:
        s = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be three positive finite numbers (x, y, z), got {spacing!r}") from None
    if len(s) != 3 or not all(0 < v < math.inf for v in s):
        raise ValueError(f"spacing must be three positive finite numbers (x, y, z), got {spacing!r}")
    return s


def _check_count(value, name: str, low: int) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or value < low:
        raise ValueError(f"{name} must be an integer of at least {low}, got {value!r}")
    return value


def plan_pyramid(shape, spacing, levels: Optional[int] = None, until: int = 64) -> List[Level]:
    """The levels of a pyramid over an (X, Y, Z) volume at the voxel spacing (sx, sy, sz), level 0 -- the volume itself,
    factors (1, 1, 1) -- first.  A pure function of its arguments: it touches no tensor.

    Rule per level: an axis is halved iff its extent is above 1 and its current spacing is below twice the smallest
    current spacing (the smallest among the axes that can still be halved).  A halved axis takes the extent
    ``ceil(n / 2)`` and twice the spacing.  Spacing (1, 1, 3) therefore gives (2, 2, 1) first and (2, 2, 2) from
    (2, 2, 3) on; an isotropic volume gives (2, 2, 2) throughout.

    ``levels`` is the number of levels of the result, level 0 included (so ``levels=1`` plans no pooling); with
    ``levels=None`` levels are added until the largest extent is at most ``until``.  Either way the plan ends when every
    extent is 1."""
    try:
        shp = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be three positive integers (X, Y, Z), got {shape!r}") from None
    if len(shp) != 3 or min(shp) < 1:
        raise ValueError(f"shape must be three positive integers (X, Y, Z), got {shape!r}")
    sp = check_spacing(spacing)
    if levels is not None:
        _check_count(levels, "levels", 1)
    _check_count(until, "until", 1)
    plan = [Level((1, 1, 1), shp, sp)]
    while (len(plan) < levels) if levels is not None else (max(shp) > until):
        live = [s for n, s in zip(shp, sp) if n > 1]
        if not live:
            break
        finest = min(live)
        f = tuple(2 if n > 1 and s < 2 * finest else 1 for n, s in zip(shp, sp))
        shp = tuple(-(-n // k) for n, k in zip(shp, f))
        sp = tuple(s * k for s, k in zip(sp, f))
        plan.append(Level(f, shp, sp))
    return plan


def pyramid(volume: Tensor, spacing, how: str, levels: Optional[int] = None, until: int = 64, sparse: bool = False,
            plan: Optional[List[Level]] = None) -> Tuple[List[Tensor], List[Level]]:
    """``(tensors, plan)``: the levels of ``plan_pyramid(volume's shape, spacing, levels, until)`` as (X, Y, Z) tensors
    on the volume's device, level k + 1 pooled from level k by ``lib.morphology.pool(.., how, sparse)``.  Level 0 is the
    input itself (without a leading 1; a signed image under ``how="mean"`` as ``pool`` converts it).  ``plan`` is a plan
    the caller already has for this shape."""
    from ..lib.morphology import check_pool_volume, pool, pool_source
    shape = check_pool_volume(volume, how)
    if sparse and how != "mode":
        raise ValueError(f"sparse leaves zeros out of the vote of how='mode' and has no meaning for how={how!r}")
    if plan is None:
        plan = plan_pyramid(shape, spacing, levels, until)
    elif tuple(plan[0].shape) != tuple(shape):
        raise ValueError(f"the plan is for a volume of shape {tuple(plan[0].shape)}, the volume has {tuple(shape)}")
    out = [pool_source(volume, how)]
    for level in plan[1:]:
        out.append(pool(out[-1], level.factors, how, sparse))
    return out, plan


def _label_entry(name, entry):
    """(volume, how) of one ``labels`` entry: a tensor means ``"mode"``, ``(tensor, how)`` names the reduction"""
    if not isinstance(name, str) or not name or "/" in name or "\\" in name or name.startswith("."):
        raise ValueError(f"labels: {name!r} cannot name a label group")
    if isinstance(entry, (tuple, list)):
        if len(entry) != 2:
            raise ValueError(f"labels[{name!r}] must be a tensor or (tensor, how)")
        vol, how = entry
    else:
        vol, how = entry, "mode"
    if how not in ("mode", "max"):
        raise ValueError(f"labels[{name!r}]: how = {how!r}, a label volume is pooled by 'mode' or 'max'")
    return vol, how


def write_ome_zarr(path: str, spacing, image: Optional[Tensor] = None, labels=None, huffman: str = "fixed",
                   levels: Optional[int] = None, until: int = 64, sparse: bool = False, unit: Optional[str] = None,
                   timings=None) -> dict:
    """Writes the OME-Zarr group ``path`` (layout: ``lib/ome_zarr.py``): the pyramid of ``image`` -- an (X, Y, Z) or
    (1, X, Y, Z) uint8 / uint16 tensor or ``None``, pooled by ``"mean"`` -- in the group itself and the pyramid of every
    entry of ``labels`` under ``path/labels/<name>``.  ``labels`` maps a name to an integer tensor of the same shape,
    pooled by ``"mode"`` (``sparse`` applies), or to ``(tensor, "max")``: ``{"instances": mask, "skeleton": (skel,
    "max")}``.  All volumes share one plan (``plan_pyramid(shape, spacing, levels, until)``) and so have the same
    levels; they may live on any device, each is pooled and deflated where it lives.  ``spacing`` is the project's
    (sx, sy, sz); ``unit`` (e.g. ``"micrometer"``) is added to every axis when given; ``huffman`` goes to the device
    deflate encoder.

    Everything is checked before anything is written: dtypes (float volumes are refused by name), shapes that differ
    between image and labels, ``huffman``, ``spacing``, and a ``path`` that exists without being a zarr group.  An
    existing group at ``path`` is replaced.  Returns a report: ``plan``, ``bytes_written`` and ``levels``; ``timings``
    (optional dict) accumulates ``pool_s`` beside the keys of ``zarr_store.save_device``."""
    from ..lib import deflate, ome_zarr
    from ..lib.morphology import check_pool_volume
    if not isinstance(path, (str, os.PathLike)):
        raise TypeError(f"path must be a path, got {type(path).__name__}")
    path = os.fspath(path)
    deflate.huffman_mode(huffman)
    sp = check_spacing(spacing)
    if unit is not None and not isinstance(unit, str):
        raise ValueError(f"unit must be a string or None, got {unit!r}")
    labels = {} if labels is None else labels
    if not isinstance(labels, dict):
        raise TypeError("labels must be a dict name -> tensor or (tensor, how)")
    if image is None and not labels:
        raise ValueError("nothing to write: give an image, labels or both")
    todo = []   # (group path relative to the root, volume, how, sparse, name)
    if image is not None:
        todo.append(("", image, "mean", False, "image"))
    for name, entry in labels.items():
        vol, how = _label_entry(name, entry)
        todo.append((os.path.join("labels", name), vol, how, bool(sparse) and how == "mode", f"labels[{name!r}]"))
    shape = None
    for _, vol, how, _, what in todo:
        s = check_pool_volume(vol, how, what)
        if shape is None:
            shape, first = s, what
        elif s != shape:
            raise ValueError(f"{what} has the shape {s}, {first} has {shape}: image and labels must share one shape")
    plan = plan_pyramid(shape, sp, levels, until)
    if os.path.exists(path):
        if not os.path.isdir(path) or (os.listdir(path) and not os.path.exists(os.path.join(path, ".zgroup"))):
            raise FileExistsError(f"{path} exists and is not a zarr group: it is not replaced")
        shutil.rmtree(path)

    base = os.path.basename(os.path.normpath(path))
    for ext in (".zarr", ".ome"):
        base = base[:-len(ext)] if base.endswith(ext) else base
    spacings = [lv.spacing for lv in plan]
    written = 0
    ome_zarr.write_group(path, {"multiscales": [ome_zarr.multiscales(base, spacings, "mean", unit)]}
                         if image is not None else None)
    if labels:
        ome_zarr.write_group(os.path.join(path, "labels"), {"labels": list(labels)})
    for rel, vol, how, sp_flag, _ in todo:
        t0 = time.perf_counter()
        tensors, _ = pyramid(vol, sp, how, sparse=sp_flag, plan=plan)
        if timings is not None:
            if tensors[-1].is_cuda:
                torch.cuda.synchronize(tensors[-1].device)
            timings["pool_s"] = timings.get("pool_s", 0.0) + time.perf_counter() - t0
        group = os.path.join(path, rel) if rel else path
        if rel:
            attrs = {"multiscales": [ome_zarr.multiscales(os.path.basename(rel), spacings, how, unit)],
                     "image-label": dict({"version": ome_zarr.NGFF_VERSION},
                                         **({"source": {"image": "../../"}} if image is not None else {}))}
            ome_zarr.write_group(group, attrs)
        written += ome_zarr.write_levels(group, tensors, huffman, timings)
        del tensors
    return {"plan": plan, "levels": len(plan), "bytes_written": written}


def read_multiscales(path: str):
    """``[(array_path, scale), ...]`` of the group at ``path`` (``lib.ome_zarr.read_multiscales``): pair it with
    ``zarr_store.load`` / ``load_device``, which give the (Z, X, Y) array of a level."""
    from ..lib import ome_zarr
    return ome_zarr.read_multiscales(path)


# ---- the command ----

def _base_name(path: str) -> str:
    name = os.path.basename(os.path.normpath(path))
    for ext in (".tiff", ".tif", ".npy", ".zarr"):
        if name.lower().endswith(ext):
            return name[:-len(ext)]
    return os.path.splitext(name)[0]


def load_volume(path: str, device) -> Tensor:
    """(X, Y, Z) tensor of a file stored [Z, X, Y(, C)] (.tif, .npy: ``tiff.read_image``; channel 2 of a colour stack, as
    ``eval()`` takes it) or of an (X, Y, Z) / (1, X, Y, Z) ``.zarr`` store (``zarr_store.load``), in the file's dtype"""
    import numpy as np
    if path.rstrip("/\\").endswith(".zarr"):
        from ..lib import zarr_store
        a = zarr_store.load(path.rstrip("/\\"))
        a = a[0] if a.ndim == 4 and a.shape[0] == 1 else a
        if a.ndim != 3:
            raise ValueError(f"{path}: expected an (X, Y, Z) or (1, X, Y, Z) store, got shape {a.shape}")
    else:
        from ..lib import tiff
        a = tiff.read_image(path)
        a = a[..., np.newaxis] if a.ndim == 3 else a
        a = a.transpose(-1, 1, 2, 0)
        a = (a[2] if a.shape[0] > 3 else a[0])
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:     # through the bit pattern: int16 storage holds the uint16 values
        return torch.from_numpy(a.view(np.int16)).to(device).view(torch.uint16)
    return torch.from_numpy(a).to(device)


def _as_labels(t: Tensor, path: str) -> Tensor:
    """A mask file's values as the narrowest dtype ``pool(how="mode")`` takes"""
    if t.dtype in (torch.uint8, torch.int16, torch.int32):
        return t
    if t.dtype == torch.uint16:
        return t.view(torch.int16).to(torch.int32) & 0xFFFF
    if t.dtype in (torch.int8, torch.int64, torch.bool) or t.dtype == getattr(torch, "uint32", None):
        wide = t.to(torch.int64)
        if t.numel() and (int(wide.min()) < -2 ** 31 or int(wide.max()) > 2 ** 31 - 1):
            raise ValueError(f"{path}: ids beyond int32 cannot be pooled")
        return wide.to(torch.int32)
    raise TypeError(f"{path}: a mask of dtype {t.dtype} cannot be pooled: integer ids only")


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.utils.pyramid",
                                     description="SKOOTS: write an image, its masks and its skeleton as one multiscale "
                                                 "OME-Zarr (NGFF 0.4) group")
    parser.add_argument("--image", type=str, default=None, metavar="I.tif",
                        help="Path to an image (.tif, stored [Z, X, Y]), uint8 or uint16: pooled by the rounded mean")
    parser.add_argument("--labels", type=str, nargs="+", default=[], metavar="M.tif",
                        help="Paths to instance masks (.tif, stored [Z, X, Y]): pooled by the most frequent id; a "
                             "label's name is its file's base name")
    parser.add_argument("--skeleton", type=str, default=None, metavar="S.zarr",
                        help="Path to a *_skoots_skeleton.zarr store of eval(): pooled by the maximum, as labels/skeleton")
    parser.add_argument("--spacing", type=float, nargs=3, required=True, metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--levels", type=int, default=None, metavar="N", help="Levels to write, the input included")
    parser.add_argument("--until", type=int, default=64, metavar="N",
                        help="Without --levels: add levels until the largest extent is at most N")
    parser.add_argument("--sparse", action="store_true",
                        help="Zeros do not vote when masks are pooled, so thin instances survive")
    parser.add_argument("--unit", type=str, default=None, help="Unit of the spacing, e.g. micrometer")
    parser.add_argument("--output-huffman", choices=("fixed", "dynamic"), default="fixed",
                        help="Code of the device deflate encoder that writes the chunks")
    parser.add_argument("--device", type=str, default=None,
                        help="Where the volumes are pooled and deflated: cuda (default when there is one) or cpu")
    parser.add_argument("-o", "--output", type=str, default=None, metavar="OUT.ome.zarr",
                        help="The group to write; default <first input without extension>.ome.zarr")
    args = parser.parse_args(argv)
    if args.image is None and not args.labels and args.skeleton is None:
        parser.error("give at least one of --image, --labels, --skeleton")
    if not all(0 < v < float("inf") for v in args.spacing):
        parser.error("--spacing must be three positive finite numbers")
    if args.levels is not None and args.levels < 1:
        parser.error("--levels must be at least 1")
    if args.until < 1:
        parser.error("--until must be at least 1")
    names = [_base_name(p) for p in args.labels] + (["skeleton"] if args.skeleton is not None else [])
    if len(set(names)) != len(names):
        parser.error(f"two label inputs share a name: {names}")
    args.spacing = tuple(args.spacing)
    return args


def main(argv=None) -> str:
    """Runs the command; returns the path written."""
    args = parse_args(argv)
    inputs = ([args.image] if args.image is not None else []) + list(args.labels) + \
             ([args.skeleton] if args.skeleton is not None else [])
    for p in inputs:
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} does not exist")
    device = torch.device(args.device if args.device is not None else
                          ("cuda" if torch.cuda.is_available() else "cpu"))
    first = os.path.normpath(inputs[0])
    out = args.output if args.output is not None else \
        os.path.join(os.path.dirname(first), _base_name(first) + ".ome.zarr")
    start = time.time()
    image = load_volume(args.image, device) if args.image is not None else None
    labels = {_base_name(p): _as_labels(load_volume(p, device), p) for p in args.labels}
    if args.skeleton is not None:
        labels["skeleton"] = (load_volume(args.skeleton, device), "max")
    timings = {}
    report = write_ome_zarr(out, args.spacing, image=image, labels=labels, huffman=args.output_huffman,
                            levels=args.levels, until=args.until, sparse=args.sparse, unit=args.unit, timings=timings)
    from ..lib import ome_zarr
    for k, lv in enumerate(report["plan"]):
        print(f"level {k}: factors {lv.factors} shape (X, Y, Z) {lv.shape} scale (z, y, x) {ome_zarr.level_scale(lv.spacing)}")
    print(f"arrays: {'image ' if image is not None else ''}{' '.join('labels/' + n for n in labels)}".rstrip())
    print(f"bytes written: {report['bytes_written']}")
    print(f"seconds: {time.time() - start:.3f} (pooling {timings.get('pool_s', 0.0):.3f}, "
          f"deflate {timings.get('kernel_s', 0.0):.3f}, files {timings.get('file_s', 0.0):.3f})")
    print(f"File Written: {out}", flush=True)
    return out


if __name__ == "__main__":
    main()
