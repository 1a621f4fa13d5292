#!/usr/bin/env python3
"""Generate tests/golden/surface_area.npz from the REFERENCE's own ``get_surface_area`` (skoots/validate/stats.py:30-48).

Run where the reference checkout and scikit-image (written with 0.18.3) are available; the tests read only the
committed .npz.  The interpreter needs numpy and scikit-image, and no torch:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_surface_area_golden.py

``skoots/validate/stats.py`` is loaded by its path (the package's ``__init__`` wants far more) behind stand-ins for
``torch`` and ``fvcore``: the tensor stand-in wraps a numpy array and offers what the function calls -- ``gt``, ``mul``,
``cpu``, ``numpy`` -- and ``torch.from_numpy`` hands the result through.  The function itself is the reference's.

Inputs: the mask of instance_stats.npz (ids 3 and 7 share a face, 300 is ragged, 1000 is one voxel in the corner), a
12 x 14 x 16 volume of 50 % noise as one label, and two touching ellipsoids.  Stored, arrays only: the two new masks,
and per input ``<name>_ids`` and ``<name>_area`` (ids, spacings, 2) float64 -- the reference's area of ``mask == id``
(open: index 0) and of the same mask padded with one layer of zeros (closed: index 1) at each of ``spacings``.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPACINGS = ((1.0, 1.0, 1.0), (1.0, 1.0, 3.0), (0.5, 2.0, 3.0))


class Tensor:
    """what get_surface_area touches of a torch.Tensor, on a numpy array"""

    def __init__(self, a):
        self.a = np.asarray(a)

    def gt(self, v):
        return Tensor(self.a > v)

    def mul(self, v):
        return Tensor(self.a * v)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_torch = _stub("torch", Tensor=Tensor, from_numpy=lambda a: a)
_torch.nn = _stub("torch.nn", Module=object)
_fv = _stub("fvcore")
_fv.nn = _stub("fvcore.nn", FlopCountAnalysis=None)
_fv.nn.parameter_count = _stub("fvcore.nn.parameter_count", parameter_count=None)


def reference_function():
    for root in sys.path:
        path = os.path.join(root, "skoots", "validate", "stats.py")
        if os.path.exists(path):
            spec = importlib.util.spec_from_file_location("reference_validate_stats", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            return mod.get_surface_area
    raise SystemExit("skoots/validate/stats.py not found: put the reference checkout on PYTHONPATH")


def ellipsoids(shape=(14, 18, 20)):
    """two labels: ellipsoids whose voxels touch along x"""
    g = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1).astype(np.float64)
    lab = np.zeros(shape, np.int32)
    lab[(((g - (4.0, 8.5, 9.0)) / (3.6, 6.2, 7.4)) ** 2).sum(-1) <= 1] = 5
    lab[(((g - (10.0, 9.0, 11.0)) / (3.2, 5.0, 6.0)) ** 2).sum(-1) <= 1] = 9
    assert ((lab[:-1] == 5) & (lab[1:] == 9)).any(), "the ellipsoids do not touch"
    return lab


def main():
    get_surface_area = reference_function()
    masks = {
        "instance_stats": np.load(os.path.join(HERE, "instance_stats.npz"))["mask"][0],
        "noise": (np.random.default_rng(2121).random((12, 14, 16)) < 0.5).astype(np.int32) * 4,
        "ellipsoids": ellipsoids(),
    }
    out = {"names": np.array(list(masks)), "spacings": np.array(SPACINGS, np.float64),
           "noise_mask": masks["noise"], "ellipsoids_mask": masks["ellipsoids"]}
    for name, lab in masks.items():
        ids = np.unique(lab)
        ids = ids[ids > 0]
        area = np.zeros((len(ids), len(SPACINGS), 2), np.float64)
        for i, u in enumerate(ids):
            one = (lab == u).astype(np.uint8)
            for s, spacing in enumerate(SPACINGS):
                area[i, s, 0] = float(get_surface_area(Tensor(one), list(spacing)))
                area[i, s, 1] = float(get_surface_area(Tensor(np.pad(one, 1)), list(spacing)))
        out[name + "_ids"], out[name + "_area"] = ids.astype(np.int64), area
        print(name, lab.shape, ids.tolist(), area[:, 0].tolist())
    path = os.path.join(HERE, "surface_area.npz")
    np.savez_compressed(path, **out)
    print(f"surface_area.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
