"""The validate command's host side (skoots_amd/validate/__main__.py) on the CPU: the CSV text from the reference
fixture's matrices (G13, tests/golden/make_validate_golden.py), argument parsing, reading and cropping."""
import numpy as np
import pytest
import torch


def test_reports_reproduce_the_reference_text(golden):
    from skoots_amd.validate.__main__ import format_reports
    d = golden("validate_cldice.npz")
    acc, tab = format_reports("gt.tif", "pred.tif", torch.from_numpy(d["csv_iou_matrix"]),
                              torch.from_numpy(d["csv_dice"]), torch.from_numpy(d["csv_cldice"]),
                              d["csv_gt_ids"].tolist())
    assert acc == str(d["csv_accuracy"])
    assert tab == str(d["csv_iou"])


def test_reports_refuse_empty_matrices():
    from skoots_amd.validate.__main__ import format_reports
    e = torch.zeros((0, 3))
    with pytest.raises(ValueError, match="no ground-truth instances"):
        format_reports("g", "p", e, e, e, [])
    e = torch.zeros((2, 0))
    with pytest.raises(ValueError, match="no predicted instances"):
        format_reports("g", "p", e, e, e, [1, 2])


def test_parse_args():
    from skoots_amd.validate.__main__ import parse_args
    a = parse_args(["--ground_truth", "a.tif", "--predicted", "b.tif"])
    assert (a.ground_truth, a.predicted, a.log) == ("a.tif", "b.tif", 3)
    assert parse_args(["--ground_truth", "a", "--predicted", "b", "--log", "0"]).log == 0
    for bad in (["--predicted", "b"], ["--ground_truth", "a", "--predicted", "b", "--log", "7"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_load_and_crop(tmp_path):
    from skoots_amd.validate.__main__ import crop, load_mask
    zxy = np.arange(12 * 103 * 104, dtype=np.int32).reshape(12, 103, 104)
    np.save(tmp_path / "m.npy", zxy)
    m = load_mask(str(tmp_path / "m.npy"))
    assert m.dtype == torch.int32 and m.shape == (1, 103, 104, 12)
    assert m[0, 4, 7, 9].item() == zxy[9, 4, 7]
    c = crop(m)
    assert c.shape == (1, 3, 4, 2) and c[0, 0, 0, 0].item() == zxy[5, 50, 50]
    with pytest.raises(ValueError, match="leaves nothing"):
        crop(m[:, :100])
    rgb = np.stack([zxy, zxy + 1, zxy + 2, zxy + 3], axis=-1)   # more than 3 channels: channel 2 is kept
    np.save(tmp_path / "c.npy", rgb)
    assert torch.equal(load_mask(str(tmp_path / "c.npy")), m + 2)
