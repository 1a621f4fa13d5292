#!/usr/bin/env python3
"""Generate tests/golden/skeleton.npz from the REFERENCE's calculate_skeletons and scikit-image 0.18.3.

Run where the reference checkout is available (the tests read only the committed .npz), like make_golden.py, and
name a second interpreter that imports scikit-image 0.18.3 (its environment has no torch):

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 SKIMAGE_PYTHON=<python with skimage 0.18.3> \\
        python tests/golden/make_skeleton_golden.py

The reference module imports kimimaro, skimage.io and skimage.morphology.skeletonize.  kimimaro and skimage.io are
placeholders (calculate_skeletons does not reach them); skeletonize is a shim that hands the crops to
``skimage.morphology.skeletonize(crop, method="lee")`` in the other interpreter, all crops of one call in one
subprocess: calculate_skeletons runs once recording its crops, the crops are thinned, and it runs again replaying the
results in the same order.

  skeleton.npz
    (a) a_*: raw skeletonize of small random volumes (unions of 1-3 boxes, 0 / 5 / 20 % of voxels knocked out) and of
        shapes that stress the rules (thin planes and lines, a hollow box, a torus, two tubes along z whose rows span
        three 32-voxel words, one voxel, a full box touching the crop border): shapes, the inputs and outputs as
        concatenated flat uint8;
    (b) b_*: calculate_skeletons of one label volume (~40 instances: touching ones, a diagonal two-voxel object, one
        that thins away, ids above 65535) under four scales; for each scale its keys, row counts and concatenated fp32 points, or
        raises = 1 when the reference raised "Downscaled too much!";
    (c) c_points: the skeleton of large_object() (defined in tests/test_skeletonize.py, too large for the LDS path).
"""
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_skeletonize import SCALES, large_object, label_volume  # noqa: E402

_THIN = r"""
import sys
import numpy as np
from skimage.morphology import skeletonize
d = np.load(sys.argv[1])
out = {}
for i in range(int(d["n"])):
    out["o%d" % i] = skeletonize(d["c%d" % i], method="lee") != 0
np.savez(sys.argv[2], **out)
"""


def skimage_thin(crops):
    """skeletonize(crop, method="lee") != 0 of every crop, in one subprocess of the scikit-image interpreter."""
    if not crops:
        return []
    py = os.environ.get("SKIMAGE_PYTHON")
    if not py:
        raise SystemExit("set SKIMAGE_PYTHON to an interpreter that imports scikit-image 0.18.3")
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, script = (os.path.join(tmp, n) for n in ("in.npz", "out.npz", "thin.py"))
        np.savez(src, n=len(crops), **{"c%d" % i: c for i, c in enumerate(crops)})
        with open(script, "w") as f:
            f.write(_THIN)
        subprocess.check_call([py, script, src, dst], env={"PATH": os.environ.get("PATH", "")})
        d = np.load(dst)
        return [d["o%d" % i] for i in range(len(crops))]


class _Shim:
    """skimage.morphology.skeletonize: records crops, or replays thinned ones in the same order."""

    def __init__(self):
        self.record, self.replay = [], None

    def __call__(self, image, method=None):
        assert method == "lee"
        if self.replay is None:
            self.record.append(np.array(image))
            return np.zeros(image.shape, np.uint8)
        return self.replay.pop(0).astype(np.uint8)


SHIM = _Shim()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("kimimaro")
_stub("skimage")
_stub("skimage.io")
_stub("skimage.morphology", skeletonize=SHIM)


def reference_calculate_skeletons(mask, scale):
    from skoots.train.generate_skeletons import calculate_skeletons
    SHIM.record, SHIM.replay = [], None
    calculate_skeletons(mask, scale)
    SHIM.replay = skimage_thin(SHIM.record)
    out = calculate_skeletons(mask, scale)
    assert not SHIM.replay
    return out


def random_volumes(rng, n):
    vols = []
    for _ in range(n):
        shape = tuple(int(s) for s in rng.integers(3, 12, size=3))
        v = np.zeros(shape, np.uint8)
        for _ in range(int(rng.integers(1, 4))):
            lo = [int(rng.integers(0, s)) for s in shape]
            hi = [int(rng.integers(l + 1, s + 1)) for l, s in zip(lo, shape)]
            v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        knock = [0.0, 0.05, 0.2][int(rng.integers(0, 3))]
        v[rng.random(shape) < knock] = 0
        vols.append(v)
    return vols


def stress_volumes():
    vols = []
    v = np.zeros((9, 10, 11), np.uint8); v[4, 1:9, 1:10] = 1; vols.append(v)          # one-voxel-thin plane (x)
    v = np.zeros((9, 10, 11), np.uint8); v[1:8, 1:9, 5] = 1; vols.append(v)           # thin plane (z)
    v = np.zeros((9, 10, 11), np.uint8); v[1:8, 5, 2:9] = 1; vols.append(v)           # thin plane (y)
    v = np.zeros((5, 6, 14), np.uint8); v[2, 3, 1:13] = 1; vols.append(v)             # line along z
    v = np.zeros((12, 5, 5), np.uint8); v[1:11, 2, 2] = 1; vols.append(v)             # line along x
    v = np.zeros((10, 10, 10), np.uint8)
    for i in range(1, 9):
        v[i, i, min(i, 8)] = 1
    vols.append(v)                                                                     # diagonal line
    v = np.zeros((10, 11, 12), np.uint8); v[1:9, 1:10, 1:11] = 1; v[3:6, 3:7, 3:8] = 0; vols.append(v)  # hollow box
    x, y, z = np.meshgrid(np.arange(24) - 11.5, np.arange(24) - 11.5, np.arange(9) - 4, indexing="ij")
    vols.append(((np.sqrt(x ** 2 + y ** 2) - 7.0) ** 2 + z ** 2 <= 9.0).astype(np.uint8))  # torus
    v = np.zeros((8, 8, 72), np.uint8); v[1:7, 1:7, 1:71] = 1; vols.append(v)         # tube along z: 3 words a row
    x, y, z = np.meshgrid(np.arange(12), np.arange(12), np.arange(80), indexing="ij")
    cx, cy = 5.5 + 3.0 * np.sin(z / 8.0), 5.5 + 3.0 * np.cos(z / 8.0)
    v = ((x - cx) ** 2 + (y - cy) ** 2 <= 6.5) & ((x * 7 + y * 3 + z * 5) % 11 != 0)
    vols.append(v.astype(np.uint8))                                                    # winding tube with holes
    v = np.zeros((5, 5, 5), np.uint8); v[2, 2, 2] = 1; vols.append(v)                 # single voxel
    vols.append(np.ones((1, 1, 1), np.uint8))                                          # single voxel, no margin
    vols.append(np.ones((7, 6, 9), np.uint8))                                          # full box touching the border
    vols.append(np.ones((1, 8, 8), np.uint8))                                          # flat full crop
    vols.append(np.zeros((4, 4, 4), np.uint8))                                         # empty
    return vols


def main():
    out = {}
    rng = np.random.default_rng(20261016)
    vols = random_volumes(rng, 100) + stress_volumes()
    thin = skimage_thin(vols)
    out["a_shapes"] = np.array([v.shape for v in vols], np.int32)
    out["a_in"] = np.concatenate([v.reshape(-1) for v in vols]).astype(np.uint8)
    out["a_out"] = np.concatenate([t.reshape(-1) for t in thin]).astype(np.uint8)

    mask = torch.from_numpy(label_volume())
    for si, scale in enumerate(SCALES):
        try:
            sk = reference_calculate_skeletons(mask.clone(), torch.tensor(scale))
        except AssertionError as e:
            assert "Downscaled too much" in str(e)
            out[f"b{si}_raises"] = np.array(1)
            continue
        out[f"b{si}_raises"] = np.array(0)
        out[f"b{si}_keys"] = np.array(list(sk.keys()), np.int64)
        out[f"b{si}_counts"] = np.array([v.shape[0] for v in sk.values()], np.int64)
        out[f"b{si}_points"] = torch.cat([v.reshape(-1, 3).float() for v in sk.values()]).numpy()
        assert all(v.dtype == torch.float32 for v in sk.values())

    big = large_object()
    (c_out,) = skimage_thin([big])
    out["c_points"] = np.argwhere(c_out).astype(np.int16)
    path = os.path.join(HERE, "skeleton.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(vols), "volumes,", out["c_points"].shape[0],
          "large-object points")


if __name__ == "__main__":
    main()
