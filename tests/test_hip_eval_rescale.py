"""``eval(..., rescale=)``: the network runs on the resampled grid -- the stores equal those of a plain ``eval`` on the
image the oracle of tests/resample_cases.py resamples -- and the mask comes back on the input's own grid as that run's
mask under the oracle's ``nearest``; ``rescale=(1, 1, 1)`` and no keyword give the same bytes; what is not built is refused
before the model runs."""
import os

import numpy as np
import pytest
import torch

from tests import resample_cases as RC

pytestmark = pytest.mark.gpu

CFG = {"SKOOTS": {"VECTOR_SCALING": (60, 60, 12)},
       "MODEL": {"DIMS": [32, 64, 128, 64, 32], "DEPTHS": [2, 2, 2, 2, 2], "IN_CHANNELS": 1}}


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            if not p.endswith(("_benchmark.txt", ".trch", ".npy")):
                with open(p, "rb") as f:
                    out[os.path.relpath(p, root)] = f.read()
    return out


def _reference_model():
    from oracle import unet_spec
    ref = unet_spec.build()
    with torch.no_grad():  # open both gates everywhere, as tests/test_hip_eval_pyramid.py does
        ref.heads.weight[3:5].mul_(0.05)
        ref.heads.weight[0:3].mul_(1e-5)
        ref.heads.bias[0:3] = 1e-5
        ref.heads.bias[3] = 2.2
        ref.heads.bias[4] = 3.0
    return ref


def _run(root, img_zxy, state, **extra):
    from skoots_amd.lib.eval import eval as sk_eval
    os.makedirs(root)
    np.save(os.path.join(root, "vol.npy"), img_zxy)
    torch.save({"cfg": CFG, "model_state_dict": state, "dataset_mean": 127.0, "dataset_std": 70.0},
               os.path.join(root, "model.trch"))
    sk_eval(os.path.join(root, "vol.npy"), os.path.join(root, "model.trch"), **extra)
    return _files(root)


def _mask(root):
    from skoots_amd.validate.__main__ import load_mask
    return load_mask(os.path.join(root, "vol_instance_mask.tif"))[0].numpy().astype(np.int32)       # (X, Y, Z)


def test_eval_rescale(tmp_path):
    state = _reference_model().state_dict()
    Z, X, Y = 24, 88, 64
    img = torch.randint(0, 256, (Z, X, Y), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).numpy()
    factors, grid = (1.5, 2.0, 1.0), (132, 128, 24)
    assert RC.output_shape((X, Y, Z), factors) == grid
    resampled = RC.oracle_resample(np.ascontiguousarray(img.transpose(1, 2, 0)), grid, "auto")     # (X, Y, Z)
    a = _run(str(tmp_path / "rescaled"), img, state, rescale=factors)
    b = _run(str(tmp_path / "plain"), np.ascontiguousarray(resampled.transpose(2, 0, 1)), state)
    # the vector store is compared by its file list alone: two forwards need not agree in the last bit of an fp16 value
    assert sorted(a) == sorted(b) and len(a) > 3
    skeleton = [k for k in a if "_skoots_skeleton.zarr" in k]
    assert len(skeleton) > 1 and all(a[k] == b[k] for k in skeleton)
    plain = _mask(str(tmp_path / "plain"))
    got = _mask(str(tmp_path / "rescaled"))
    assert plain.shape == grid and got.shape == (X, Y, Z) and plain.any()
    assert np.array_equal(got, RC.oracle_resample(plain, (X, Y, Z), "nearest"))


def test_rescale_of_one_gives_the_same_bytes(tmp_path):
    state = _reference_model().state_dict()
    img = torch.randint(0, 256, (24, 132, 128), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).numpy()
    a = _run(str(tmp_path / "one"), img, state, rescale=(1, 1, 1))
    b = _run(str(tmp_path / "none"), img, state)
    assert sorted(a) == sorted(b) and len(a) > 3 and all(a[k] == b[k] for k in a if "_vectors.zarr" not in k)


def test_refused_before_the_model_runs(tmp_path, monkeypatch):
    from skoots_amd import unet
    from skoots_amd.lib.eval import eval as sk_eval

    def no_model(*args, **kwargs):
        raise AssertionError("the model was built")
    monkeypatch.setattr(unet, "cfg_to_model", no_model)
    root = str(tmp_path)
    torch.save({"cfg": CFG, "model_state_dict": {}, "dataset_mean": 127.0, "dataset_std": 70.0},
               os.path.join(root, "model.trch"))
    np.save(os.path.join(root, "vol.npy"), np.zeros((4, 16, 16), np.uint8))
    np.save(os.path.join(root, "float.npy"), np.zeros((4, 16, 16), np.float32))
    np.save(os.path.join(root, "negative.npy"), np.full((4, 16, 16), -3, np.int16))
    model = os.path.join(root, "model.trch")
    with pytest.raises(ValueError, match="pyramid.*rescale"):
        sk_eval(os.path.join(root, "vol.npy"), model, pyramid=True, rescale=(1.5, 1.5, 1))
    with pytest.raises(TypeError, match="image is torch.float32"):
        sk_eval(os.path.join(root, "float.npy"), model, rescale=(1.5, 1.5, 1))
    with pytest.raises(ValueError, match="0 .. 65535"):
        sk_eval(os.path.join(root, "negative.npy"), model, rescale=(1.5, 1.5, 1))
    with pytest.raises(ValueError, match="ratio of X"):
        sk_eval(os.path.join(root, "vol.npy"), model, rescale=(9, 1, 1))
    with pytest.raises(ValueError, match="factors"):
        sk_eval(os.path.join(root, "vol.npy"), model, rescale=(1, 0, 1))
    assert sorted(os.listdir(root)) == ["float.npy", "model.trch", "negative.npy", "vol.npy"]
