"""Training data: ``dataset``, ``MultiDataset`` and ``skeleton_colate`` (reference: skoots/train/dataloader.py:21-310,
500-649).

A ``dataset`` holds the volumes of one source folder: for every ``<base>.labels.tif`` its image ``<base>.tif`` and its
skeletons ``<base>.skeletons.trch`` (or ``<base>.labels.tif.skeletons.trch``, the name ``--skeletonize-train-data``
writes), on the host or on the device.  ``__getitem__`` runs the transform on one volume.

The statistics keep the reference's arithmetic, quirks included, because mean and standard deviation go into the
checkpoint and into every later ``eval()``.  Each volume contributes through a 256-bin
histogram, computed once and cached: ``numpy.bincount`` for a volume on the host, the ``sk_u8_histogram`` kernel for a
volume on the device (which is never copied to the host).
"""
from __future__ import annotations

import glob
import logging
import math
import os
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch
from torch import Tensor
from torch.utils.data import Dataset

from .. import _ffi
from ..lib.tiff import read_image
from .transforms import skeleton_colate  # noqa: F401  (re-exported: the reference defines it in this module)

log = logging.getLogger(__name__)

_LABELS = ".labels.tif"
_BINS = np.arange(256, dtype=np.float64)


def u8_histogram(x: Tensor) -> np.ndarray:
    """The 256-bin histogram of a uint8 tensor as int64: ``numpy.bincount`` on the host, ``sk_u8_histogram`` on the
    device (only the 256 counters travel to the host)."""
    if x.dtype != torch.uint8:
        raise ValueError(f"dataset statistics need uint8 volumes, got {x.dtype}")
    if not x.is_cuda:
        return np.bincount(x.contiguous().numpy().reshape(-1), minlength=256).astype(np.int64)
    x = x.contiguous()
    hist = torch.zeros(256, dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib.sk_u8_histogram(_ffi.ptr(x), x.numel(), _ffi.ptr(hist), _ffi.stream_ptr(x.device)))
    return hist.cpu().numpy()


def _int64_over_int(total: int, n: int) -> float:
    """``torch.tensor(total) / n`` as the reference evaluates it: an int64 tensor over a Python int is a true division
    in the default dtype, fp32."""
    return float((torch.tensor(int(total), dtype=torch.int64) / int(n)).item())


class dataset(Dataset):
    """``dataset(path, transforms, pad_size, device, sample_per_image)`` (dataloader.py:41-157).

    ``path``: a folder or a list of folders.  ``device``: where ``__getitem__`` puts its outputs; ``to(device)`` moves
    the stored volumes.  Images must be uint8 ``[Z, X, Y(, C)]`` and are kept as ``(1, X, Y, Z)`` (channel 2 when
    C > 3); masks ``[Z, X, Y]`` are kept as ``(1, X, Y, Z)`` uint8 / int16 / int32, the narrowest that holds the ids."""

    def __init__(self, path: Union[List[str], str], transforms: Optional[Callable] = lambda x: x,
                 pad_size: Optional[int] = 100, device: Optional[str] = "cpu", sample_per_image: Optional[int] = 1):
        super().__init__()
        self.path = path
        self.files: List[str] = []
        self.image: List[Tensor] = []
        self.centroids: List[Tensor] = []
        self.masks: List[Tensor] = []
        self.skeletons: List[Dict[int, Tensor]] = []
        self.baked_skeleton: List[Optional[Tensor]] = []
        self.transforms = transforms
        self.device = device
        self.pad_size: List[int] = [pad_size, pad_size]
        self.sample_per_image: int = sample_per_image
        self._hist: Dict[int, np.ndarray] = {}
        self._reset_caches()

        for p in ([path] if isinstance(path, str) else path):
            self.files.extend(sorted(glob.glob(os.path.join(p, "*" + _LABELS))))
        for f in self.files:
            base = f[:-len(_LABELS)]
            image_path = base + ".tif"
            if not os.path.exists(image_path):
                raise FileNotFoundError(f"Could not find the image {image_path} that belongs to {f}")
            skel_path = next((s for s in (base + ".skeletons.trch", f + ".skeletons.trch") if os.path.exists(s)), None)
            if skel_path is None:
                raise FileNotFoundError(f"cannot find skeleton file for: {f} (expected {base}.skeletons.trch; "
                                        "python -m skoots_amd --skeletonize-train-data writes it)")
            skeleton = torch.load(skel_path, map_location="cpu", weights_only=True)
            for k, v in skeleton.items():
                if v.numel() == 0:
                    raise ValueError(f"{f} instance label {k} has an empty skeleton ({skel_path})")

            log.info("Loading Image: %s", image_path)
            image = read_image(image_path)
            masks = read_image(f)                         # [Z, X, Y]
            if image.dtype != np.uint8:
                raise ValueError(f"{image_path}: image must be 8bit, not {image.dtype}")
            if masks.ndim != 3:
                raise ValueError(f"{f}: masks must be [Z, X, Y], got shape {masks.shape}")
            image = image[..., np.newaxis] if image.ndim == 3 else image
            image = image.transpose(-1, 1, 2, 0)
            image = image[[2], ...] if image.shape[0] > 3 else image
            masks = masks.transpose(1, 2, 0)
            top = masks.max() if masks.size else 0
            dtype = np.uint8 if top < 256 else np.int16 if top < (2 ** 16 // 2) - 1 else np.int32
            log.info("saving mask at %s as dtype: %s", f, np.dtype(dtype).name)
            self.image.append(torch.from_numpy(np.ascontiguousarray(image)))
            self.masks.append(torch.from_numpy(np.ascontiguousarray(masks.astype(dtype))).unsqueeze(0))
            self.skeletons.append(skeleton)
            self.baked_skeleton.append(None)
        log.info("done loading from source: %s", path)

    def _reset_caches(self) -> None:
        self._sum: Optional[Dict[str, Any]] = None
        self._numel: Optional[Dict[str, Any]] = None
        self._mean: Optional[Dict[str, Any]] = None
        self._std: Optional[Dict[str, Any]] = None

    def __len__(self) -> int:
        return len(self.image) * self.sample_per_image

    def __getitem__(self, item: int) -> Dict[str, Any]:
        item = item // self.sample_per_image   # an image may be sampled several times per pass
        with torch.no_grad():
            data_dict = self.transforms({"image": self.image[item], "masks": self.masks[item],
                                         "skeletons": self.skeletons[item],
                                         "baked_skeleton": self.baked_skeleton[item]})
        for k, v in data_dict.items():
            if isinstance(v, Tensor):
                data_dict[k] = v.to(self.device)
            elif isinstance(v, dict):
                data_dict[k] = {key: value.to(self.device) for key, value in v.items()}
        return data_dict

    def to(self, device) -> "dataset":
        """Move the stored images, masks and skeletons."""
        self.image = [x.to(device) for x in self.image]
        self.masks = [x.to(device) for x in self.masks]
        self.skeletons = [{k: v.to(device) for k, v in x.items()} for x in self.skeletons]
        return self

    def cuda(self) -> "dataset":
        return self.to("cuda:0")

    def cpu(self) -> "dataset":
        return self.to("cpu")

    def pin_memory(self) -> "dataset":
        self.image = [x.pin_memory() for x in self.image]
        self.masks = [x.pin_memory() for x in self.masks]
        self.skeletons = [{k: v.pin_memory() for k, v in x.items()} for x in self.skeletons]
        return self

    def map(self, fn, key: Union[List[str], str]) -> "dataset":
        """Apply ``fn`` to every stored item of ``key`` ('image', 'masks' or 'skeletons', or a list of them; the
        reference compares the list it has just built with a string, so its map never applies anything)."""
        valid = ["image", "masks", "skeletons"]
        keys = [key] if isinstance(key, str) else list(key)
        for k in keys:
            if k not in valid:
                raise ValueError(f"key: {k} is invalid. Valid keys are: {valid}")
            setattr(self, k, [fn(v) for v in getattr(self, k)])
        if "image" in keys:
            self._hist = {}
            self._reset_caches()
        return self

    # -- statistics (dataloader.py:246-310) ----------------------------------------------------------------
    def histogram(self, i: int) -> np.ndarray:
        """Cached int64 histogram of image ``i``."""
        if i not in self._hist:
            self._hist[i] = u8_histogram(self.image[i])
        return self._hist[i]

    def _image_sum(self, i: int) -> int:
        return sum(v * int(c) for v, c in enumerate(self.histogram(i).tolist()))

    def sum(self, with_invert: bool = False) -> int:
        """Sum of every voxel; ``with_invert`` adds the inverted sum (255 - x) of the LAST image only (the reference's
        ``if`` sits outside its loop)."""
        if self._sum is None or self._sum["with_invert"] != with_invert:
            total = 0
            for i in range(len(self.image)):
                total += self._image_sum(i)
            if with_invert and self.image:
                last = len(self.image) - 1
                total += 255 * int(self.image[last].numel()) - self._image_sum(last)
            self._sum = {"sum": total, "with_invert": with_invert}
        return self._sum["sum"]

    def numel(self, with_invert: bool = False) -> int:
        """Voxels of all images, doubled by ``with_invert`` (for ALL images, unlike ``sum``)."""
        if self._numel is None or self._numel["with_invert"] != with_invert:
            n = sum(int(x.numel()) for x in self.image)
            self._numel = {"numel": n * 2 if with_invert else n, "with_invert": with_invert}
        return self._numel["numel"]

    def mean(self, with_invert: bool = False) -> Optional[float]:
        if self._mean is None or self._mean["with_invert"] != with_invert:
            n = self.numel(with_invert)
            self._mean = {"mean": _int64_over_int(self.sum(with_invert), n) if n else None, "with_invert": with_invert}
        return self._mean["mean"]

    def std(self, with_invert: bool = False) -> Optional[float]:
        """As written in the reference: the numerator is the SQUARE of ``subtract_square_sum(mean)``.  The engine does
        not call it (``MultiDataset.std`` is the one that reaches the checkpoint)."""
        if self._std is None or self._std["with_invert"] != with_invert:
            mean, n = self.mean(with_invert), self.numel(with_invert)
            self._std = {"std": math.sqrt(self.subtract_square_sum(mean) ** 2 / n) if n else None,
                         "with_invert": with_invert}
        return self._std["std"]

    def subtract_square_sum(self, other) -> float:
        """sum over every voxel of (x - other)^2 in float64: sum_v h[v] (v - other)^2 from the cached histograms."""
        other = float(other)
        total = 0.0
        for i in range(len(self.image)):
            total += float(np.sum(self.histogram(i).astype(np.float64) * (_BINS - other) ** 2))
        return total


class MultiDataset(Dataset):
    """Several datasets behind one index (dataloader.py:500-623)."""

    def __init__(self, *args):
        self.datasets: List[dataset] = [ds for ds in args if isinstance(ds, Dataset)]
        self._dataset_lengths = [len(ds) for ds in self.datasets]
        self.num_datasets = len(self.datasets)
        self._mapped_indicies: List[int] = []
        for i, n in enumerate(self._dataset_lengths):
            self._mapped_indicies.extend([i] * n)

    def __len__(self) -> int:
        return len(self._mapped_indicies)

    def __getitem__(self, item: int):
        i = self._mapped_indicies[item]
        return self.datasets[i][item - sum(self._dataset_lengths[:i])]

    def to(self, device) -> "MultiDataset":
        for ds in self.datasets:
            ds.to(device)
        return self

    def cuda(self) -> "MultiDataset":
        return self.to("cuda:0")

    def cpu(self) -> "MultiDataset":
        return self.to("cpu")

    def map(self, fn, key) -> "MultiDataset":
        for ds in self.datasets:
            ds.map(fn, key)
        return self

    def sum(self, with_invert: bool = False) -> Optional[int]:
        total = 0
        for ds in self.datasets:
            total += ds.sum(with_invert=with_invert)
        return total if total else None

    def numel(self, with_invert: bool = False) -> Optional[int]:
        total = 0
        for ds in self.datasets:
            total += ds.numel(with_invert=with_invert)
        return total if total else None

    def mean(self, with_invert: bool = False) -> Optional[float]:
        """The fp32 value the reference's ``int64 tensor / int`` gives, as a Python float."""
        s, n = self.sum(with_invert), self.numel(with_invert)
        return _int64_over_int(s, n) if s and n else None

    def std(self, with_invert: bool = False) -> Optional[float]:
        """sqrt(sum_datasets subtract_square_sum(mean) / n): ``mean`` the fp32 value above, the sum over the images as
        they are (no inverted copy), ``n`` the doubled count under ``with_invert``."""
        mean = self.mean(with_invert)
        if mean is None:
            return None
        n = self.numel(with_invert)
        return math.sqrt(sum(ds.subtract_square_sum(mean) for ds in self.datasets) / n)
