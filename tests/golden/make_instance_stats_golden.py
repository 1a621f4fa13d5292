#!/usr/bin/env python3
"""Generate tests/golden/instance_stats.npz from the REFERENCE's own ``mask_to_bbox`` (skoots/validate/lib.py:12-54).

Run where the reference checkout is available (the tests read only the committed .npz), like make_validate_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_instance_stats_golden.py

The same stand-in modules as make_validate_golden.py let ``skoots.validate.lib`` import without its optional
dependencies.  The fixture holds arrays only: one (1, 23, 31, 40) int32 mask with sparse ids (3, 7, 300, 1000) -- 3 and
7 share a face, 1000 is a single voxel -- and the ids and (6, N) int16 boxes the reference returns for it.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _ident(*a, **k):
    return a[0] if a and callable(a[0]) else (lambda f: f)


_stub("numba", njit=_ident, prange=range)
_sk = _stub("skimage")
_sk.morphology = _stub("skimage.morphology")
_sk.io = _stub("skimage.io", imread=lambda path: None)
_stub("bism")
for _s in ("backends", "modules", "models", "models.spatial_embedding"):
    _stub("bism." + _s)
sys.modules["bism.models.spatial_embedding"].SpatialEmbedding = object
_y = _stub("yacs")
_y.config = _stub("yacs.config", CfgNode=dict)
torch.compile = lambda m, *a, **k: m

from skoots.validate.lib import mask_to_bbox  # noqa: E402


def main():
    gen = torch.Generator().manual_seed(1818)
    mask = torch.zeros((1, 23, 31, 40), dtype=torch.int32)
    mask[0, 2:9, 4:15, 5:21] = 3
    mask[0, 9:14, 6:12, 8:30] = 7                      # shares the x = 8 | 9 face with 3
    blob = torch.rand((9, 12, 11), generator=gen) < 0.6
    mask[0, 14:23, 19:31, 29:40][blob] = 300           # ragged, reaches the far corner region
    mask[0, 22, 30, 39] = 300
    mask[0, 0, 0, 0] = 1000                            # a single voxel
    ids, boxes = mask_to_bbox(mask)
    path = os.path.join(HERE, "instance_stats.npz")
    np.savez_compressed(path, mask=mask.numpy(), ids=ids.numpy(), boxes=boxes.numpy())
    print(f"instance_stats.npz: {os.path.getsize(path) / 1024:.1f} KiB, ids {ids.tolist()}")


if __name__ == "__main__":
    main()
