"""``eval(..., equalize=)``: the network sees the transformed image -- every output equals that of a plain ``eval`` on a
file that holds the image the oracle of tests/equalize_cases.py equalizes -- also with ``denoise`` in front and
``rescale`` behind; a float image and a bad ``how`` are refused by name before the model is built; ``python -m
skoots_amd.utils.equalize`` writes the samples of the library call."""
import os

import numpy as np
import pytest
import torch

from tests import equalize_cases as EC
from tests import filter_cases as FC
from tests.test_hip_eval_denoise import CFG, _reference_model, _run, _same_outputs

pytestmark = pytest.mark.gpu

STRETCH = {"how": "stretch", "low": 2.0, "high": 90.0}
SLICES = {"how": "match", "tile": "slices"}


def _image(seed, shape_zxy):
    """[Z, X, Y] uint8: noise in a narrow range whose planes carry their own gain and offset"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(40, 140, shape_zxy, generator=g, dtype=torch.int32)
    gain = torch.linspace(0.6, 1.4, shape_zxy[0]).view(-1, 1, 1)
    return (img * gain + torch.arange(shape_zxy[0]).view(-1, 1, 1) % 7 * 5).clamp(0, 255).to(torch.uint8).numpy()


def _equalized(img_zxy, **kwargs):
    """[Z, X, Y] -> the oracle's transform of the (X, Y, Z) volume -> [Z, X, Y]"""
    vol = np.ascontiguousarray(img_zxy.transpose(1, 2, 0))
    return np.ascontiguousarray(EC.oracle_equalize(vol, **kwargs).transpose(2, 0, 1))


@pytest.mark.parametrize("option", (STRETCH, SLICES), ids=("stretch", "slices"))
def test_eval_equalize(tmp_path, option):
    state = _reference_model().state_dict()
    img = _image(0, (24, 132, 128))
    want = _equalized(img, **option)
    assert not np.array_equal(want, img)
    a = _run(str(tmp_path / "equalized"), img, state, equalize=option)
    b = _run(str(tmp_path / "plain"), want, state)
    _same_outputs(a, b)


def test_eval_denoise_then_equalize_then_rescale(tmp_path):
    state = _reference_model().state_dict()
    img = _image(1, (24, 88, 64))
    factors = (1.5, 2.0, 1.0)
    vol = np.ascontiguousarray(img.transpose(1, 2, 0))
    filtered = FC.oracle_rank(vol, (1, 1, 0), 4, "mirror")
    want = np.ascontiguousarray(EC.oracle_equalize(filtered, **SLICES).transpose(2, 0, 1))
    a = _run(str(tmp_path / "all"), img, state, denoise=("median", (1, 1, 0)), equalize=SLICES, rescale=factors)
    b = _run(str(tmp_path / "rescaled"), want, state, rescale=factors)
    _same_outputs(a, b)


def test_refused_before_the_model_is_built(tmp_path, monkeypatch):
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
    model = os.path.join(root, "model.trch")
    vol = os.path.join(root, "vol.npy")
    with pytest.raises(TypeError, match="image is torch.float32.*equalize"):
        sk_eval(os.path.join(root, "float.npy"), model, equalize=STRETCH)
    with pytest.raises(ValueError, match="how = 'clahe', must be one of"):
        sk_eval(vol, model, equalize={"how": "clahe"})
    with pytest.raises(ValueError, match="equalize must be a dict"):
        sk_eval(vol, model, equalize="stretch")
    with pytest.raises(ValueError, match="not \\['radius'\\]"):
        sk_eval(vol, model, equalize={"how": "stretch", "radius": 1})
    with pytest.raises(ValueError, match="how='stretch' takes low and high, not clip"):
        sk_eval(vol, model, equalize={"how": "stretch", "clip": 2.0})
    with pytest.raises(FileNotFoundError, match="missing.tif does not exist"):
        sk_eval(vol, model, equalize={"how": "match", "target": os.path.join(root, "missing.tif")})
    with pytest.raises(ValueError, match="bins = 1024: image is torch.uint8"):
        sk_eval(vol, model, equalize={"how": "equalize", "bins": 1024})
    assert sorted(os.listdir(root)) == ["float.npy", "model.trch", "vol.npy"]


def test_the_main_command_parses_every_form(tmp_path):
    from skoots_amd.__main__ import parse_args
    ref = str(tmp_path / "ref.tif")
    open(ref, "wb").close()
    base = ["--image", "I.tif", "--pretrained-checkpoint", "m.trch", "--equalize"]
    assert parse_args(base + ["stretch", "0.5", "99.5"]).equalize == {"how": "stretch", "low": 0.5, "high": 99.5}
    assert parse_args(base + ["clahe", "64", "64", "16", "3"]).equalize == {"how": "equalize", "tile": (64, 64, 16), "clip": 3.0}
    assert parse_args(base + ["match", ref]).equalize == {"how": "match", "target": ref}
    assert parse_args(base + ["slices"]).equalize == {"how": "match", "tile": "slices"}
    for bad in (["stretch", "5"], ["clahe", "8", "8", "8"], ["median", "1", "1", "0"], ["stretch", "60", "40"],
                ["match", str(tmp_path / "none.tif")]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_the_equalize_command(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.lib.morphology import equalize
    from skoots_amd.utils import equalize as command
    vol = EC.source("ramp", "uint16", (21, 19, 30))                              # (X, Y, Z)
    ref = EC.source("noise12", "uint16", (9, 6, 15))
    path, ref_path = str(tmp_path / "I.tif"), str(tmp_path / "R.tif")
    tiff.write_stack(path, EC.to_torch(np.ascontiguousarray(vol.transpose(2, 0, 1))))
    tiff.write_stack(ref_path, EC.to_torch(np.ascontiguousarray(ref.transpose(2, 0, 1))))
    written = command.main([path, "--stretch", "1", "99"])
    assert written == [str(tmp_path / "I_equalized.tif")]
    got = np.ascontiguousarray(tiff.read_image(written[0]).transpose(1, 2, 0))
    want = equalize(EC.to_torch(vol).to("cuda:0"), "stretch", low=1.0, high=99.0)
    assert got.dtype == np.uint16 and np.array_equal(got, EC.to_numpy(want))
    assert np.array_equal(got, EC.oracle_equalize(vol, "stretch", low=1.0, high=99.0))
    shift = EC.shift_of(int(vol.max()), 1024)
    lo, hi = EC.stretch_bounds_one(EC.oracle_histograms(vol, None, 1024, shift)[0, 0, 0], 1.0, 99.0)
    report = capsys.readouterr().out
    for line in ("shape (X, Y, Z) (21, 19, 30), dtype uint16", "operator: stretch", "tile grid: 1 x 1 x 1 tiles of 21 x 19 x 30",
                 f"bins: 1024, shift {shift}", "kernel paths: histograms one, apply lds/-+one/lookup", f"lo: {lo}", f"hi: {hi}",
                 "File Written: " + written[0]):
        assert line in report, line
    written = command.main([path, "--clahe", "8", "8", "16", "--clip", "2", "--bins", "256", "--no-interpolate"])
    got = np.ascontiguousarray(tiff.read_image(written[0]).transpose(1, 2, 0))
    assert np.array_equal(got, EC.oracle_equalize(vol, "equalize", tile=(8, 8, 16), clip=2.0, bins=256, interpolate=False))
    report = capsys.readouterr().out
    assert "tile grid: 3 x 3 x 2 tiles of 8 x 8 x 16" in report and "bins: 256, shift" in report
    assert "kernel paths: histograms ztiles, apply lds/-+tile/lookup" in report
    written = command.main([path, "--match", ref_path, "-o"])
    assert written == [path]
    got = np.ascontiguousarray(tiff.read_image(path).transpose(1, 2, 0))
    assert np.array_equal(got, EC.oracle_equalize(vol, "match", target=ref))
    assert "tiles matched: 1" in capsys.readouterr().out
    tiff.write_stack(path, EC.to_torch(np.ascontiguousarray(vol.transpose(2, 0, 1))))
    written = command.main([path, "--slices"])
    got = np.ascontiguousarray(tiff.read_image(written[0]).transpose(1, 2, 0))
    assert np.array_equal(got, EC.oracle_equalize(vol, "match", tile="slices"))
    report = capsys.readouterr().out
    assert "tiles matched: 30" in report and "kernel paths: histograms planes, apply lds/-+tile/lookup" in report
    written = command.main([path, "--equalize", "--device", "cpu"])
    got = np.ascontiguousarray(tiff.read_image(written[0]).transpose(1, 2, 0))
    assert np.array_equal(got, EC.oracle_equalize(vol, "equalize", clip=None))
