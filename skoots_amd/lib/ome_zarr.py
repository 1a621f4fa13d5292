"""The group and metadata layer of an OME-Zarr (NGFF 0.4) multiscale image on the zarr v2 directory stores of
``zarr_store``: what napari, neuroglancer and the Fiji / MoBIE plug-ins open as a pyramid.

    path/.zgroup                     {"zarr_format": 2}
    path/.zattrs                     {"multiscales": [{"version": "0.4", "name", "axes", "datasets", "type"}]}
    path/0, path/1, ...              the levels, each a ``zarr_store.save_device`` array
    path/labels/.zgroup, .zattrs     {"labels": [name, ...]}
    path/labels/<name>/.zgroup, .zattrs   its own "multiscales" and "image-label"; its levels 0, 1, ... beside them

Arrays are stored in the order of the mask TIFF -- planes, rows, columns: the project's (X, Y, Z) tensor permuted
(2, 0, 1) -- and their axes are named z, y, x, so a level's scale is ``(spacing_z, spacing_x, spacing_y)`` of the
project's (x, y, z) spacing.  Chunks are (32, 256, 256) clipped to the level; chunk keys are ``.``-separated, which
zarr v2 reads by default (NGFF only recommends ``/``).  The ``zarr`` and ``ome-zarr`` packages are not in this image: the
layout follows the published specification, and no third-party reader has opened these files.

Out of scope: ``omero`` rendering metadata, label ``colors``, time and channel axes, zarr v3 / sharded stores, and
reading groups other writers made beyond what ``read_multiscales`` does on ours."""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple

NGFF_VERSION = "0.4"
CHUNKS = (32, 256, 256)      # (z, y, x) of the stored arrays, clipped to each level


def axes(unit: Optional[str] = None) -> List[dict]:
    return [dict({"name": n, "type": "space"}, **({"unit": unit} if unit is not None else {})) for n in ("z", "y", "x")]


def level_scale(spacing: Sequence[float]) -> List[float]:
    """The scale of a stored (Z, X, Y) array from the project's (sx, sy, sz) spacing of its level"""
    sx, sy, sz = (float(v) for v in spacing)
    return [sz, sx, sy]


def multiscales(name: str, spacings: Sequence[Sequence[float]], how: str, unit: Optional[str] = None) -> dict:
    """One entry of a group's ``multiscales`` list: level k is the array ``str(k)`` at ``spacings[k]`` (sx, sy, sz)."""
    return {"version": NGFF_VERSION, "name": name, "axes": axes(unit),
            "datasets": [{"path": str(k), "coordinateTransformations": [{"type": "scale", "scale": level_scale(s)}]}
                         for k, s in enumerate(spacings)],
            "type": how}


def write_group(path: str, attrs: Optional[dict] = None) -> None:
    """``path/.zgroup`` and, with ``attrs``, ``path/.zattrs``"""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f, indent=2)
    if attrs is not None:
        with open(os.path.join(path, ".zattrs"), "w") as f:
            json.dump(attrs, f, indent=2)


def level_chunks(shape_zxy: Sequence[int]) -> List[int]:
    return [max(1, min(int(s), c)) for s, c in zip(shape_zxy, CHUNKS)]


def write_levels(group: str, levels, huffman: str = "fixed", timings=None) -> int:
    """The levels of one pyramid, (X, Y, Z) tensors of either device, as the arrays ``group/0``, ``group/1``, ...: the
    permuted view goes to ``zarr_store.save_device`` (its chunk gather handles the strides), with explicit chunks.
    Returns the bytes of the chunk files."""
    from . import zarr_store
    written = 0
    for k, t in enumerate(levels):
        view = t.permute(2, 0, 1)
        dest = os.path.join(group, str(k))
        zarr_store.save_device(dest, view, chunks=level_chunks(view.shape), timings=timings, huffman=huffman)
        written += sum(os.path.getsize(os.path.join(dest, fn)) for fn in os.listdir(dest) if not fn.startswith("."))
    return written


def read_multiscales(path: str) -> List[Tuple[str, List[float]]]:
    """``[(array_path, scale), ...]`` of the first ``multiscales`` entry of the group at ``path``, finest level first:
    ``array_path`` opens with ``zarr_store.load`` / ``load_device`` and holds a (Z, X, Y) array, ``scale`` is its
    (z, y, x) scale.  A group without ``multiscales`` (the root of a labels-only store) raises ``ValueError``."""
    with open(os.path.join(path, ".zgroup")) as f:
        if json.load(f).get("zarr_format") != 2:
            raise ValueError(f"{path}: not a zarr v2 group")
    attrs_path = os.path.join(path, ".zattrs")
    attrs = {}
    if os.path.exists(attrs_path):
        with open(attrs_path) as f:
            attrs = json.load(f)
    if not attrs.get("multiscales"):
        raise ValueError(f"{path}: the group has no multiscales entry")
    out = []
    for d in attrs["multiscales"][0]["datasets"]:
        scale = [t["scale"] for t in d["coordinateTransformations"] if t.get("type") == "scale"]
        if len(scale) != 1:
            raise ValueError(f"{path}: dataset {d.get('path')!r} must carry exactly one scale transformation")
        out.append((os.path.join(path, d["path"]), [float(v) for v in scale[0]]))
    return out


def read_labels(path: str) -> List[str]:
    """The names under ``path/labels``, or [] when the group has none"""
    attrs_path = os.path.join(path, "labels", ".zattrs")
    if not os.path.exists(attrs_path):
        return []
    with open(attrs_path) as f:
        return list(json.load(f).get("labels", []))
