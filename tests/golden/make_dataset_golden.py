#!/usr/bin/env python3
"""Generate tests/golden/dataset_stats.npz from the REFERENCE's own ``dataset`` / ``MultiDataset`` statistics
(skoots/train/dataloader.py:246-310, 580-623).

Run where the reference checkout is available (the tests read only the committed .npz):

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dataset_golden.py

numba is stubbed to the identity (``_sub_sq_sum`` then runs as plain Python: a serial float64 sum), ``skimage.io`` is a
placeholder (nothing here reads a file).  ``dataset`` objects are built with ``object.__new__`` -- no folder is read --
with ``image`` set to the volumes of ``volumes()`` below and the name-mangled caches set to ``None``.  A fresh set of
objects is used per ``with_invert`` value: the per-dataset caches are keyed by the flag.

  dataset_stats.npz
    v{d}_{i}            the uint8 volumes, (1, X, Y, Z): dataset d, image i  (3 datasets: 2, 1 and 3 images, so that
                        "the inverted sum of the last image only" shows)
    layout              images per dataset
    sum_{0,1} numel_{0,1}   MultiDataset.sum / numel, int64, with_invert False / True
    mean_{0,1}          MultiDataset.mean as the reference returns it (an fp32 tensor), stored as float32
    std_{0,1}           MultiDataset.std, float64
    ds_sum_{0,1} ds_numel_{0,1}   the same per dataset, int64 arrays
    others, sss         subtract_square_sum(other) summed over the datasets for two values of ``other``, float64
    ds_sss              per dataset and ``other``, float64 (n_datasets, 2)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT = (2, 1, 3)
OTHERS = (88.80663299560547, 127.5)


def volumes():
    """Seeded uint8 volumes, skewed like micrographs (a dark background, a few bright structures)."""
    g = np.random.default_rng(20240611)
    shapes = [[(1, 13, 11, 5), (1, 9, 17, 4)], [(1, 16, 16, 6)], [(1, 7, 5, 3), (1, 21, 8, 5), (1, 10, 10, 10)]]
    out = []
    for d, group in enumerate(shapes):
        vols = []
        for i, s in enumerate(group):
            base = g.normal(40 + 25 * d, 12 + 3 * i, size=s)
            bright = g.random(s) < 0.08 + 0.03 * i
            v = np.where(bright, g.normal(200, 30, size=s), base)
            vols.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
        out.append(vols)
    return out


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main():
    ident = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))  # noqa: E731
    _stub("numba", njit=ident, prange=range)
    sk = _stub("skimage")
    sk.io = _stub("skimage.io")
    from skoots.train.dataloader import MultiDataset, dataset

    vols = volumes()

    def build():
        sets = []
        for d, group in enumerate(vols):
            ds = object.__new__(dataset)
            ds.path = f"dataset{d}"
            ds.image = [torch.from_numpy(v.copy()) for v in group]
            ds.sample_per_image = 1
            for cache in ("sum", "numel", "mean", "std"):
                setattr(ds, f"_dataset__{cache}", None)
            sets.append(ds)
        return MultiDataset(*sets), sets

    out = {"layout": np.array(LAYOUT), "others": np.array(OTHERS, dtype=np.float64)}
    for d, group in enumerate(vols):
        for i, v in enumerate(group):
            out[f"v{d}_{i}"] = v
    for flag in (False, True):
        multi, sets = build()
        t = int(flag)
        out[f"sum_{t}"] = np.int64(int(multi.sum(with_invert=flag)))
        out[f"numel_{t}"] = np.int64(int(multi.numel(with_invert=flag)))
        mean = multi.mean(with_invert=flag)
        assert isinstance(mean, torch.Tensor) and mean.dtype == torch.float32, (type(mean), getattr(mean, "dtype", None))
        out[f"mean_{t}"] = np.float32(mean.item())
        out[f"std_{t}"] = np.float64(multi.std(with_invert=flag))
        out[f"ds_sum_{t}"] = np.array([int(s.sum(with_invert=flag)) for s in sets], dtype=np.int64)
        out[f"ds_numel_{t}"] = np.array([int(s.numel(with_invert=flag)) for s in sets], dtype=np.int64)
    multi, sets = build()
    ds_sss = np.array([[float(np.asarray(s.subtract_square_sum(o)).reshape(-1)[0]) for o in OTHERS] for s in sets],
                      dtype=np.float64)
    out["ds_sss"] = ds_sss
    out["sss"] = ds_sss.sum(0)
    path = os.path.join(HERE, "dataset_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in ("sum_0", "sum_1", "numel_0", "numel_1", "mean_0", "mean_1", "std_0", "std_1", "sss"):
        print(k, repr(out[k]))


if __name__ == "__main__":
    main()
