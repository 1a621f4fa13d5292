"""Lee thinning and calculate_skeletons on the MI355X against scikit-image 0.18.3 and the reference
(tests/golden/skeleton.npz, tests/golden/make_skeleton_golden.py), bit for bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_skeletonize import SCALES, fixture_a, fixture_b, label_volume, large_object

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got: dict, want: dict):
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, k
        assert np.array_equal(g, w, equal_nan=True), k


def test_skeletonize_fixture_a():
    from skoots_amd.lib.morphology import skeletonize
    for i, (src, want) in enumerate(fixture_a()):
        got = skeletonize(torch.from_numpy(src).to(DEV))
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), f"volume {i} {src.shape}"


def test_skeletonize_large_object_global_path():
    from skoots_amd.lib.morphology import skeletonize, thin_objects
    from tests.test_skeletonize import golden
    big = large_object()
    got = skeletonize(torch.from_numpy(big).to(DEV))
    assert np.array_equal(np.argwhere(got.cpu().numpy()), golden()["c_points"].astype(np.int64))
    # the same object next to small ones in one launch: LDS and workspace objects side by side
    lab = torch.from_numpy(big.astype(np.int32)).to(DEV)
    lab[:4, :4, :4] = 2
    pts, counts, stats = thin_objects(lab, [1, 2], [(0, 0, 0) + big.shape, (0, 0, 0, 4, 4, 4)])
    assert counts[0] == golden()["c_points"].shape[0] and stats[0, 0] > 1


@pytest.mark.parametrize("si", range(len(SCALES)))
def test_calculate_skeletons_fixture_b(si):
    from skoots_amd.train import calculate_skeletons
    mask = torch.from_numpy(label_volume()).to(DEV)
    want = fixture_b(si)
    if want is None:
        with pytest.raises(ValueError, match="Downscaled too much!"):
            calculate_skeletons(mask, torch.tensor(SCALES[si]))
        return
    got = calculate_skeletons(mask, torch.tensor(SCALES[si]))
    assert all(v.device.type == "cuda" for v in got.values())
    _same(got, want)


def test_device_resample_equals_cpu_on_odd_ratios():
    v = torch.from_numpy(label_volume()).float()
    for size in [(40, 36, 42), (13, 11, 5), (53, 47, 19), (80, 72, 28), (40, 36, 13)]:
        cpu = F.interpolate(v[None, None], size=size, mode="nearest")[0, 0]
        gpu = F.interpolate(v.to(DEV)[None, None], size=size, mode="nearest")[0, 0]
        assert torch.equal(gpu.cpu(), cpu), size


def _many_instances(seed=11, shape=(256, 256, 64), n=1000):
    rng = np.random.default_rng(seed)
    v = torch.zeros(shape, dtype=torch.int32)
    cx = rng.integers(0, shape[0], n)
    cy = rng.integers(0, shape[1], n)
    cz = rng.integers(0, shape[2], n)
    r = rng.integers(2, 7, (n, 3))
    for i in range(n):
        xs = slice(max(cx[i] - r[i, 0], 0), cx[i] + r[i, 0])
        ys = slice(max(cy[i] - r[i, 1], 0), cy[i] + r[i, 1])
        zs = slice(max(cz[i] - r[i, 2] // 2, 0), cz[i] + r[i, 2] // 2 + 1)
        v[xs, ys, zs] = i + 1
    return v


def test_one_launch_equals_per_object_launches():
    from skoots_amd.lib.morphology import thin_objects
    from skoots_amd.train.generate_skeletons import _object_boxes
    lab = _many_instances().to(DEV)
    ids, lower, upper = _object_boxes(lab)
    assert ids.numel() > 900
    boxes = np.concatenate([lower, lower + np.maximum(upper - lower, 1)], 1)
    ids_np = ids.cpu().numpy()
    pts, counts, _ = thin_objects(lab, ids_np, boxes)
    pts = pts.cpu().numpy()
    start = 0
    for i in range(len(ids_np)):
        one, c1, _ = thin_objects(lab, ids_np[i:i + 1], boxes[i:i + 1])
        assert c1[0] == counts[i]
        assert np.array_equal(one.cpu().numpy(), pts[start:start + counts[i]]), int(ids_np[i])
        start += counts[i]


def test_cli_writes_reference_skeletons():
    from skoots_amd.lib.eval import _write_mask_tif
    want = fixture_b(SCALES.index((1.0, 1.0, 3.0)))
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "vol.labels.tif")
        _write_mask_tif(f, label_volume().transpose(2, 0, 1))
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, "-m", "skoots_amd", "--skeletonize-train-data", tmp, "--anisotropyZ", "3"],
                       cwd=ROOT, env=env, check=True, timeout=300, capture_output=True)
        got = torch.load(f + ".skeletons.trch")
    assert all(v.device.type == "cpu" for v in got.values())
    _same(got, want)


def test_skeletons_bake_and_mask_smoke():
    from skoots_amd.lib.skeleton import bake_skeleton, skeleton_to_mask
    from skoots_amd.train import calculate_skeletons
    mask = torch.from_numpy(label_volume()).to(DEV)
    sk = calculate_skeletons(mask, torch.tensor((1.0, 1.0, 1.0)))
    sk = {k: v for k, v in sk.items() if not torch.isnan(v).any()}
    baked = bake_skeleton(mask, sk, anisotropy=(1.0, 1.0, 3.0))
    assert baked.shape == (3,) + tuple(mask.shape) and torch.isfinite(baked).all()
    skm = skeleton_to_mask(sk, tuple(mask.shape))
    assert skm.shape == (1,) + tuple(mask.shape) and skm.sum() > 0
