"""``resample`` without a device: the integer oracle of tests/resample_cases.py against scipy, the library's CPU path
against the oracle on every shared case, ``resample_shape``, every refusal by name, and the command end to end on CPU
tensors."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import pool_cases as PC
from tests import resample_cases as RC

from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import check_resample, resample, resample_shape
from skoots_amd.utils import resample as tool


# ---- the oracle against scipy ----

def _zoom(a, shape, order):
    return ndimage.zoom(a.astype(np.float64), [m / n for n, m in zip(a.shape, shape)], order=order, mode="nearest",
                        grid_mode=True)


LINEAR_1D = [(n, m) for n in (1, 2, 3, 7, 16, 33) for m in (n, n + 1, 2 * n, 3 * n, 5 * n + 1, 8 * n) if m >= n]
LINEAR_3D = (((5, 7, 9), (7, 9, 20)), ((4, 6, 8), (32, 6, 9)), ((3, 3, 3), (5, 24, 4)))


@pytest.mark.parametrize("dtype", RC.IMAGE_DTYPES)
def test_linear_upsampling_is_within_half_a_unit_of_scipy(dtype):
    top = int(np.iinfo(dtype).max)
    worst = 0.0
    for src, dst in [((1, 1, n), (1, 1, m)) for n, m in LINEAR_1D] + list(LINEAR_3D):
        a = RC.image_volume(dtype, src)
        got = RC.oracle_resample(a, dst, "linear")
        want = _zoom(a, dst, 1)
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"{dtype}: largest |oracle - scipy| = {worst}")
    assert worst <= 0.5 + 1e-6 * top


NEAREST_1D = [(n, m) for n in range(1, 41) for m in range(max(1, -(-n // 8)), min(8 * n, 64) + 1)
              if not RC.centre_on_boundary(n, m)]


def test_nearest_equals_scipy_where_no_centre_lies_on_a_boundary():
    assert len(NEAREST_1D) > 500
    assert all(not any(((2 * i + 1) * n) % (2 * m) == 0 for i in range(m)) for n, m in NEAREST_1D)
    for n, m in NEAREST_1D:
        a = RC.image_volume("uint16", (1, 1, n))
        got = RC.oracle_resample(a, (1, 1, m), "nearest")
        assert np.array_equal(got, _zoom(a, (1, 1, m), 0).astype(np.uint16)), (n, m)


def test_area_equals_block_means_and_oracle_pool():
    for dtype in RC.IMAGE_DTYPES:
        a = RC.image_volume(dtype, (6, 8, 12))
        for f in ((2, 2, 2), (2, 2, 1), (1, 1, 2)):
            shape = tuple(n // k for n, k in zip(a.shape, f))
            assert np.array_equal(RC.oracle_resample(a, shape, "area"), PC.oracle_pool(a, f, "mean"))
        for f in ((3, 4, 6), (6, 1, 3), (1, 8, 4)):
            shape = tuple(n // k for n, k in zip(a.shape, f))
            blocks = a.astype(np.int64).reshape(shape[0], f[0], shape[1], f[1], shape[2], f[2]).sum(axis=(1, 3, 5))
            count = f[0] * f[1] * f[2]
            assert np.array_equal(RC.oracle_resample(a, shape, "area"), ((blocks + count // 2) // count).astype(dtype))


def test_identity_gcd_reduction_and_the_way_back():
    for dtype in RC.IMAGE_DTYPES:
        a = RC.image_volume(dtype, (5, 7, 24))
        for how in ("linear", "area", "auto", "nearest"):
            assert np.array_equal(RC.oracle_resample(a, a.shape, how), a)
        for how, shape in (("linear", (10, 9, 36)), ("area", (3, 4, 9)), ("auto", (7, 5, 36)), ("auto", (40, 1, 16))):
            assert np.array_equal(RC.oracle_resample(a, shape, how), RC.oracle_resample(a, shape, how, reduce=True))
    assert RC.axis_matrix(4, 8, "linear", reduce=True)[1] == 4           # 2x up: weights 1 and 3 of 4
    assert sorted(set(RC.axis_matrix(4, 8, "linear", reduce=True)[0].ravel().tolist())) == [0, 1, 3, 4]
    for dtype in RC.LABEL_DTYPES:
        a = RC.source("nearest", dtype, (5, 7, 24))
        up = RC.oracle_resample(a, (10, 21, 96), "nearest")
        assert np.array_equal(RC.oracle_resample(up, a.shape, "nearest"), a)


def test_halves_round_up_and_saturated_blocks_stay():
    a = np.array([100, 101], np.uint8).reshape(1, 1, 2)
    assert RC.oracle_resample(a, (1, 1, 1), "area").item() == 101                 # 100.5
    assert RC.oracle_resample(a, (1, 1, 4), "linear").ravel().tolist() == [100, 100, 101, 101]   # 100.25 and 100.75
    full = np.full((8, 8, 8), 65535, np.uint16)
    for how, shape in (("area", (1, 1, 1)), ("linear", (9, 64, 13)), ("auto", (3, 11, 5))):
        assert (RC.oracle_resample(full, shape, how) == 65535).all()


# ---- the library's CPU path against the oracle ----

ALL_CASES = RC.z_cases() + list(RC.UNIT_CASES) + list(RC.MIXED_CASES) + list(RC.DTYPE_CASES) + list(RC.ODD_ROW_CASES) + \
    [c[:4] for c in RC.ACC_CASES[:2]] + list(RC.BIG_CASES[:1])


def test_cpu_path_equals_the_oracle_on_every_case():
    for how, dtype, shape, out_shape in ALL_CASES:
        src = RC.to_torch(RC.source(how, dtype, shape))
        got = resample(src, shape=out_shape, how=how)
        assert got.dtype == src.dtype and not got.is_cuda
        assert np.array_equal(RC.to_numpy(got), RC.expected(how, dtype, tuple(shape), tuple(out_shape))), (how, dtype, shape)


def test_cpu_path_keeps_a_leading_one_and_takes_views():
    a = RC.source("auto", "uint16", (5, 7, 24))
    want = RC.expected("auto", "uint16", (5, 7, 24), (7, 5, 36))
    got = resample(RC.to_torch(a).unsqueeze(0), factors=(1.4, 0.7, 1.5))
    assert tuple(got.shape) == (1, 7, 5, 36) and np.array_equal(RC.to_numpy(got[0]), want)
    view = RC.to_torch(np.ascontiguousarray(a.transpose(2, 0, 1))).permute(1, 2, 0)
    assert not view.is_contiguous() and np.array_equal(RC.to_numpy(resample(view, shape=(7, 5, 36))), want)


def test_tap_tables_are_the_oracle_taps_divided_by_one_factor():
    for n, m in ((4, 8), (7, 7), (31, 32), (9, 6), (40, 13), (1, 8), (8, 1), (5, 3)):
        for op in RC.OPS:
            start, count, w, W = M.resample_taps(n, m, op)
            for i in range(m):
                want, total = RC.taps(n, m, op, i)
                dense = {}
                for k, wt in want:
                    dense[k] = dense.get(k, 0) + wt
                dense = {k: wt for k, wt in dense.items() if wt}
                got = {int(start[i]) + t: int(w[i, t]) for t in range(int(count[i])) if int(w[i, t])}
                assert total % W == 0 and {k: wt * (total // W) for k, wt in got.items()} == dense, (n, m, op, i)
                assert all(int(w[i, t]) == 0 for t in range(int(count[i]), w.shape[1]))


# ---- shapes and refusals ----

def test_resample_shape():
    assert resample_shape((88, 64, 24), (1.5, 2.0, 1.0)) == (132, 128, 24)
    assert resample_shape((5, 5, 5), (0.5, 0.1, 0.3)) == (3, 1, 2)            # 2.5 rounds up; never below 1
    assert resample_shape((300, 300, 20), (1, 1, 3)) == (300, 300, 60)
    for bad in ((1, 1), (1, 0, 1), (1, -2, 1), (1, float("nan"), 1), (1, float("inf"), 1), "abc", None):
        with pytest.raises(ValueError, match="factors"):
            resample_shape((4, 4, 4), bad)
    with pytest.raises(ValueError, match="shape"):
        resample_shape((4, 0, 4), (1, 1, 1))


def test_refusals_by_name():
    u8 = torch.zeros((8, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="exactly one of shape and factors"):
        resample(u8)
    with pytest.raises(ValueError, match="exactly one of shape and factors"):
        resample(u8, shape=(4, 4, 4), factors=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="how = 'cubic'"):
        resample(u8, shape=(4, 4, 4), how="cubic")
    for dt in (torch.float16, torch.float32, torch.float64, torch.bool):
        with pytest.raises(TypeError, match="float, complex and bool volumes are not resampled"):
            resample(torch.zeros((8, 8, 8), dtype=dt), shape=(4, 4, 4))
    for how in ("auto", "linear", "area"):
        for dt in (torch.int32, torch.int16):
            with pytest.raises(TypeError, match="takes uint8 or uint16"):
                resample(torch.zeros((8, 8, 8), dtype=dt), shape=(4, 4, 4), how=how)
    for dt in (torch.int8, torch.int64):
        with pytest.raises(TypeError, match="takes int32, int16, uint8 or uint16"):
            resample(torch.zeros((8, 8, 8), dtype=dt), shape=(4, 4, 4), how="nearest")
    with pytest.raises(TypeError, match="must be a tensor"):
        resample(np.zeros((8, 8, 8), np.uint8), shape=(4, 4, 4))
    with pytest.raises(ValueError, match=r"\(X, Y, Z\) or \(1, X, Y, Z\)"):
        resample(torch.zeros((2, 8, 8, 8), dtype=torch.uint8), shape=(4, 4, 4))
    with pytest.raises(ValueError, match="shape must be three integers"):
        resample(u8, shape=(4, 4))
    with pytest.raises(ValueError, match="shape must be three integers"):
        resample(u8, shape=(4, 4.5, 4))
    with pytest.raises(ValueError, match="shape must be three integers"):
        resample(u8, shape=(4, 0, 4))
    with pytest.raises(ValueError, match="ratio of X, 8 -> 65"):
        resample(u8, shape=(65, 8, 8))
    with pytest.raises(ValueError, match="ratio of Z, 17 -> 2"):
        resample(torch.zeros((8, 8, 17), dtype=torch.uint8), shape=(8, 8, 2))
    assert tuple(resample(u8, shape=(64, 1, 8)).shape) == (64, 1, 8)           # both ends of the limit are inside
    # descriptions only: an expanded tensor has the extents without the memory
    huge = torch.zeros((1, 1, 1), dtype=torch.uint16).expand(2 ** 15, 2 ** 15, 2 ** 30)
    with pytest.raises(ValueError, match="2\\^63"):
        check_resample(huge, (2 ** 15, 2 ** 15, 2 ** 30), "linear")     # 2^16 * 2^16 * 2^31 * 65535
    assert check_resample(huge, (2 ** 15, 2 ** 15, 2 ** 30), "nearest")[1] == ("nearest",) * 3
    with pytest.raises(ValueError, match="too large"):
        check_resample(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2 ** 30 + 8, 1, 1), (2 ** 30 + 8, 1, 1), "nearest")
    with pytest.raises(ValueError, match="too large"):
        check_resample(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2 ** 16, 2 ** 16, 1), (2 ** 16, 2 ** 16, 1), "nearest")
    s, ops = check_resample(torch.zeros((1, 6, 9, 40), dtype=torch.uint8), (9, 6, 60))
    assert s == (6, 9, 40) and ops == ("linear", "area", "linear")


# ---- the command ----

def _write_pair(root):
    from skoots_amd.lib import tiff
    image = RC.image_volume("uint16", (12, 10, 6))
    labels = np.zeros((12, 10, 6), np.int32)
    labels[0:6, 0:5, :] = 3
    labels[6:12, 5:10, :] = 70000
    labels[4, 7, 2] = 9                     # one voxel at an even x: halving x by nearest keeps the odd ones, so it is lost
    tiff.write_stack(os.path.join(root, "a.tif"), np.ascontiguousarray(image.transpose(2, 0, 1)))
    tiff.write_stack(os.path.join(root, "a.labels.tif"), np.ascontiguousarray(labels.transpose(2, 0, 1)))
    return image, labels


def _read(path):
    from skoots_amd.utils.pyramid import load_volume
    return RC.to_numpy(load_volume(path, "cpu"))


def test_tool_end_to_end_on_cpu(tmp_path, capsys):
    root = str(tmp_path)
    image, labels = _write_pair(root)
    written = tool.main([os.path.join(root, "a.tif"), "--spacing", "1", "1", "3", "--to-spacing", "2", "2", "1.5",
                         "--device", "cpu"])
    assert written == [os.path.join(root, "a_resampled.tif")]
    want = RC.oracle_resample(image, (6, 5, 12), "auto")
    assert np.array_equal(_read(written[0]), want)
    out = capsys.readouterr().out
    assert "shape (X, Y, Z) (12, 10, 6) -> (6, 5, 12)" in out and "factors: 0.5 0.5 2" in out
    assert "operators: area area linear" in out and f"File Written: {written[0]}" in out and "ids_lost" not in out

    reports = []
    masks = tool.resample_file([os.path.join(root, "a.labels.tif")], like=written[0], labels=True, device="cpu",
                               reports=reports)
    assert masks == [os.path.join(root, "a.labels_resampled.tif")]
    want_labels = RC.oracle_resample(labels, (6, 5, 12), "nearest")
    assert np.array_equal(_read(masks[0]).astype(np.int32), want_labels) and 70000 in want_labels
    rep = reports[0]
    assert (rep.ids_in, rep.ids_out, rep.ids_lost) == (3, 2, 1) and rep.operators == ("nearest",) * 3
    assert rep.shape_in == (12, 10, 6) and rep.shape_out == (6, 5, 12) and rep.factors == (0.5, 0.5, 2.0)

    tool.main([os.path.join(root, "a.labels.tif"), "--labels", "--factors", "1", "1", "3", "--device", "cpu", "-o"])
    out = capsys.readouterr().out
    assert "ids_in: 3" in out and "ids_out: 3" in out and "ids_lost: 0" in out and "operators: nearest nearest nearest" in out
    assert np.array_equal(_read(os.path.join(root, "a.labels.tif")).astype(np.int32),
                          RC.oracle_resample(labels, (12, 10, 18), "nearest"))


def test_tool_refusals(tmp_path):
    root = str(tmp_path)
    _write_pair(root)
    a = os.path.join(root, "a.tif")
    for argv in ([a], [a, "--factors", "1", "1", "2", "--like", a], [a, "--spacing", "1", "1", "1"],
                 [a, "--factors", "1", "0", "1"], [a, "--labels", "--how", "linear", "--factors", "1", "1", "2"]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
    with pytest.raises(FileNotFoundError):
        tool.resample_file([os.path.join(root, "missing.tif")], factors=(1, 1, 2), device="cpu")
    with pytest.raises(ValueError, match="ratio of Z"):
        tool.resample_file([a], factors=(1, 1, 9), device="cpu")
    with pytest.raises(ValueError, match="exactly one of"):
        tool.resample_file([a], factors=(1, 1, 2), like=a, device="cpu")
    np.save(os.path.join(root, "f.npy"), np.zeros((4, 5, 6), np.float32))
    with pytest.raises(TypeError, match="not resampled"):
        tool.resample_file([os.path.join(root, "f.npy")], factors=(1, 1, 2), device="cpu")
    with pytest.raises(TypeError, match="not resampled"):
        tool.resample_file([os.path.join(root, "f.npy")], factors=(1, 1, 2), labels=True, device="cpu")
    assert not [n for n in os.listdir(root) if "_resampled" in n]


# ---- ABI and signatures ----

def test_abi_and_eval_signature():
    import inspect

    from skoots_amd import _ffi
    from skoots_amd.__main__ import parse_args
    from skoots_amd.lib.eval import eval as sk_eval
    assert _ffi.lib.sk_abi_version() >= 32
    assert {"sk_resample_volume", "sk_resample_workspace_bytes", "sk_resample_path"} <= set(_ffi.EXPORTS)
    p = inspect.signature(sk_eval).parameters["rescale"]
    assert p.default is None
    args = parse_args(["--image", "I.tif", "--pretrained-checkpoint", "M.trch", "--rescale", "1.5", "1.5", "1"])
    assert args.rescale == [1.5, 1.5, 1.0]
    assert parse_args(["--image", "I.tif", "--pretrained-checkpoint", "M.trch"]).rescale is None
    for bad in (["--rescale", "1", "0", "1"], ["--rescale", "1", "1", "1", "--pyramid"]):
        with pytest.raises(SystemExit):
            parse_args(["--image", "I.tif", "--pretrained-checkpoint", "M.trch"] + bad)
    # the host query answers without a device, and refuses what the launch refuses
    assert M.resample_path(torch.int32, (4, 4, 4), (8, 8, 8), ("nearest",) * 3) == "gather"
    with pytest.raises(ValueError, match="sk_resample_volume.*ratio"):
        M.resample_path(torch.uint8, (4, 4, 4), (33, 4, 4), ("linear",) * 3)
