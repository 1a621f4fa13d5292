"""The host side of the intensity measurement, no GPU: the numpy restatement of
tests/intensity_cases.py against scipy.ndimage and against a plain loop, ``intensity_columns`` / ``ring_columns`` on
hand-made tables, the CSV texts, the command's flags and the refusals of the image that come before any device call."""
import numpy as np
import pytest
import torch

from tests import intensity_cases as K

ndi = pytest.importorskip("scipy.ndimage")

# scipy sums n float64 terms: its own error is bounded by n 2^-53 ~ 1e-11 relative at n <= 1e5 voxels
RTOL = 1e-9

SMALL = [((7, 9, 11), 1, "u8"), ((5, 17, 70), 2, "u8"), ((12, 13, 9), 3, "u16"), ((3, 5, 40), 4, "u16")]


def _case(shape, seed, kind):
    mask = K.boxes(shape, 6, seed)
    image = K.noise_u8(shape, seed + 100) if kind == "u8" else K.noise_u16(shape, seed + 100)
    assert mask.size <= 10 ** 5
    return mask, image


@pytest.mark.parametrize("shape,seed,kind", SMALL)
def test_restatement_against_scipy_mean_extrema_histogram_centroid(shape, seed, kind):
    mask, image = _case(shape, seed, kind)
    shift = 0 if kind == "u8" else 8
    m, e, h = K.ref_intensity(mask, image, shift)
    rows, ids = K.rows_of(mask)
    index = np.arange(1, ids.size + 1)
    f = image.astype(np.float64)
    assert np.array_equal(m[:, 0], np.bincount(rows.reshape(-1), minlength=ids.size + 1)[1:])
    np.testing.assert_allclose(m[:, 1] / m[:, 0], ndi.mean(f, rows, index), rtol=RTOL, atol=0)
    assert np.array_equal(e[:, 0], ndi.minimum(image, rows, index).astype(np.int64))
    assert np.array_equal(e[:, 1], ndi.maximum(image, rows, index).astype(np.int64))
    width = 1 << shift
    want_h = ndi.histogram(image, 0, 256 * width, 256, rows, index)
    assert np.array_equal(h, np.stack(list(want_h)).astype(np.int64))
    com = np.array(ndi.center_of_mass(f, rows, index))
    np.testing.assert_allclose(m[:, 3:6] / m[:, 1:2], com, rtol=RTOL, atol=0)


@pytest.mark.parametrize("shape,seed,kind", SMALL)
def test_restatement_against_scipy_variance(shape, seed, kind):
    from skoots_amd.validate.compare import intensity_columns
    mask, image = _case(shape, seed, kind)
    m, e, h = K.ref_intensity(mask, image, 0 if kind == "u8" else 8)
    rows, ids = K.rows_of(mask)
    want = ndi.variance(image.astype(np.float64), rows, np.arange(1, ids.size + 1))
    n, sv, svv = (m[:, k].astype(object) for k in range(3))
    got = np.array([float(a) for a in (n * svv - sv * sv)]) / np.array([float(a) for a in n * n])
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-9)
    std = intensity_columns(m, e, h, 0 if kind == "u8" else 8)["intensity_std"].numpy()
    np.testing.assert_allclose(std * std, want, rtol=RTOL, atol=1e-9)


def test_restatement_against_a_plain_loop():
    mask = K.boxes((4, 6, 9), 4, 11, ids=(3, 7, 300, 1000))
    for image, shift in ((K.noise_u8(mask.shape, 5), 0), (K.noise_u16(mask.shape, 6), 8), (K.noise_u16(mask.shape, 6), 3)):
        for a, b in zip(K.ref_intensity(mask, image, shift), K.loop_intensity(mask, image, shift)):
            assert np.array_equal(a, b)


def _tables(rows):
    """(moments, extrema, hist) at shift 0 of hand-written rows: a list of lists of (value, x, y, z)"""
    m, e, h = np.zeros((len(rows), 6), np.int64), np.zeros((len(rows), 2), np.int64), np.zeros((len(rows), 256), np.int64)
    for i, vox in enumerate(rows):
        for v, x, y, z in vox:
            m[i] += (1, v, v * v, v * x, v * y, v * z)
            h[i, v] += 1
        e[i] = (min(v[0] for v in vox), max(v[0] for v in vox))
    return m, e, h


def test_intensity_columns_one_voxel_and_zero_sum():
    from skoots_amd.validate.compare import intensity_columns
    m, e, h = _tables([[(37, 2, 3, 4)], [(0, 1, 1, 1), (0, 5, 5, 5)]])
    c = intensity_columns(torch.from_numpy(m), torch.from_numpy(e), torch.from_numpy(h), 0, (1.0, 0.5, 2.0))
    assert c["intensity_mean"].tolist() == [37.0, 0.0] and c["intensity_std"].tolist() == [0.0, 0.0]
    for k in ("intensity_min", "intensity_max", "intensity_median", "intensity_p05", "intensity_p95"):
        assert c[k].dtype == torch.int64 and c[k].tolist() == [37, 0]
    assert c["weighted_centroid"][0].tolist() == [2.0, 1.5, 8.0]
    assert torch.isnan(c["weighted_centroid"][1]).all()
    assert all(c[k].dtype == torch.float64 for k in ("intensity_mean", "intensity_std", "weighted_centroid"))


@pytest.mark.parametrize("n", [1, 2, 19, 20, 21])
def test_quantile_ranks(n):
    from skoots_amd.validate.compare import intensity_columns
    from skoots_amd.validate.lib import nearest_rank
    values = [(7 * k) % 251 + 2 for k in range(n)]
    m, e, h = _tables([[(v, 0, 0, 0) for v in values]])
    c = intensity_columns(m, e, h, 0)
    s = np.sort(values)
    for name, p in (("intensity_median", 50), ("intensity_p05", 5), ("intensity_p95", 95)):
        assert c[name].tolist() == [int(s[nearest_rank(n, p)])], (name, n)
    # the ranks themselves, 1-based: ceil(p n / 100)
    assert [nearest_rank(n, p) + 1 for p in (5, 50, 95)] == [-(-5 * n // 100), -(-50 * n // 100), -(-95 * n // 100)]
    mean = sum(values) / n
    assert c["intensity_mean"].tolist() == [mean]
    assert abs(c["intensity_std"].item() - float(np.std(values))) <= 1e-12 * max(1.0, float(np.std(values)))


def test_shift_reports_bin_lower_edges():
    from skoots_amd.validate.compare import intensity_columns
    values = [1000, 1001, 1007, 1008, 2047]
    m = np.array([[5, sum(values), sum(v * v for v in values), 0, 0, 0]], np.int64)
    e = np.array([[1000, 2047]], np.int64)
    h = np.zeros((1, 256), np.int64)
    for v in values:
        h[0, v >> 3] += 1
    c = intensity_columns(m, e, h, 3)
    assert c["intensity_median"].tolist() == [1000] and (1007 >> 3) << 3 == 1000      # the sample is 1007, its bin [1000, 1008)
    assert c["intensity_p05"].tolist() == [1000] and c["intensity_p95"].tolist() == [2040]
    assert c["intensity_min"].tolist() == [1000] and c["intensity_max"].tolist() == [2047]      # these stay exact


def test_ring_columns_empty_ring_and_contrast():
    from skoots_amd.validate.compare import ring_columns
    m = np.array([[4, 40, 500, 0, 0, 0], [2, 0, 0, 0, 0, 0], [1, 9, 81, 0, 0, 0]], np.int64)
    r = np.array([[0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [2, 6, 20, 0, 0, 0]], np.int64)
    c = ring_columns(torch.from_numpy(r), torch.from_numpy(m))
    assert c["ring_voxels"].dtype == torch.int64 and c["ring_voxels"].tolist() == [0, 3, 2]
    c = {k: v.numpy() for k, v in c.items()}
    assert np.isnan(c["ring_mean"][0]) and np.isnan(c["ring_std"][0]) and np.isnan(c["contrast"][0])       # empty ring
    assert c["ring_mean"][1] == 0.0 and np.isnan(c["contrast"][1])                                        # 0 / 0
    assert c["ring_mean"][2] == 3.0 and c["ring_std"][2] == 1.0 and c["contrast"][2] == (9.0 - 3.0) / (9.0 + 3.0)


def _csv_inputs():
    ids = [3, 9]
    sums = torch.zeros((2, 13), dtype=torch.int64)
    sums[0, :10] = torch.tensor([2, 2, 4, 7, 2, 8, 25, 4, 7, 14])      # voxels (1, 2, 3), (1, 2, 4)
    sums[0, 10:] = torch.tensor([4, 4, 2])
    sums[1, :10] = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0, 0, 0])        # voxel (0, 0, 0)
    sums[1, 10:] = torch.tensor([2, 2, 2])
    boxes = torch.tensor([[1, 2, 3, 1, 2, 4], [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    m, e, h = _tables([[(10, 1, 2, 3), (30, 1, 2, 4)], [(0, 0, 0, 0)]])
    ring = np.array([[3, 12, 72, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.int64)
    return ids, sums, boxes, (m, e, h, 0), ring


def test_format_csv_appends_the_two_groups_and_leaves_the_rest():
    from skoots_amd.validate import compare as CMP
    ids, sums, boxes, intensity, ring = _csv_inputs()
    spacing = (1.0, 1.0, 3.0)
    plain = CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing)
    again = CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing, intensity=None, ring=None)
    assert plain == again and "intensity" not in plain and "ring" not in plain
    assert plain.splitlines()[2] == CMP.CSV_COLUMNS
    with_i = CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing, intensity=intensity)
    both = CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing, intensity=intensity, ring=ring)
    a, b, c = plain.splitlines(), with_i.splitlines(), both.splitlines()
    assert a[:2] == b[:2] == c[:2]
    assert b[2] == a[2] + "," + CMP.INTENSITY_COLUMNS and c[2] == b[2] + "," + CMP.RING_COLUMNS
    assert CMP.INTENSITY_COLUMNS == ("intensity_mean,intensity_std,intensity_min,intensity_max,intensity_median,"
                                     "intensity_p05,intensity_p95,wcx,wcy,wcz")
    assert CMP.RING_COLUMNS == "ring_voxels,ring_mean,ring_std,contrast"
    for la, lb, lc in zip(a[3:], b[3:], c[3:]):
        assert lb.startswith(la + ",") and lc.startswith(lb + ",")
    # the worked row: samples 10 at z = 3 and 30 at z = 4; weighted z = (30 + 120) / 40 = 3.75, times the spacing 3
    assert b[3][len(a[3]) + 1:] == "20.0,10.0,10,30,10,10,30,1.0,2.0,11.25"
    # its ring: three voxels 2, 2, 8 -> mean 4, variance 72 / 3 - 16 = 8; contrast (20 - 4) / (20 + 4)
    assert c[3][len(b[3]) + 1:] == ",".join(["3", "4.0", repr(float(np.sqrt(np.float64(8.0)))), repr(16.0 / 24.0)])
    assert b[4][len(a[4]) + 1:] == "0.0,0.0,0,0,0,0,0,nan,nan,nan" and c[4][len(b[4]) + 1:] == "0,nan,nan,nan"
    with pytest.raises(ValueError):
        CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing, ring=ring)
    # with contacts in front, the new groups still come last
    table = np.zeros((0, 9), np.int64)
    mixed = CMP.format_csv("m.tif", ids, sums, boxes, (4, 5, 6), spacing, contact_table=table, intensity=intensity)
    assert mixed.splitlines()[2] == a[2] + "," + CMP.CONTACT_COLUMNS + "," + CMP.INTENSITY_COLUMNS


def test_format_histograms_csv():
    from skoots_amd.validate import compare as CMP
    ids, _, _, (m, e, h, shift), _ = _csv_inputs()
    text = CMP.format_histograms_csv("m.tif", ids, torch.from_numpy(h), 4).splitlines()
    assert text[0] == "Mask File: m.tif" and text[1] == "Bin width: 2^4"
    assert text[2] == "id," + ",".join(f"b{k}" for k in range(256)) and len(text) == 5
    row = text[3].split(",")
    assert len(row) == 257 and row[0] == "3" and row[11] == "1" and row[31] == "1" and sum(int(v) for v in row[1:]) == 2
    assert text[4].split(",")[:2] == ["9", "1"]
    with pytest.raises(ValueError):
        CMP.format_histograms_csv("m.tif", [1], h, 0)


def test_parse_args_flag_dependencies():
    from skoots_amd.validate.compare import parse_args
    a = parse_args(["m.tif"])
    assert a.image is None and a.intensity_ring is None and a.save_histograms is False
    a = parse_args(["m.tif", "--image", "i.tif", "--intensity-ring", "3", "--save-histograms"])
    assert a.image == "i.tif" and a.intensity_ring == 3.0 and a.save_histograms is True
    for bad in (["--intensity-ring", "3"], ["--save-histograms"], ["--image", "i.tif", "--intensity-ring", "0"],
                ["--image", "i.tif", "--intensity-ring", "-1"], ["--image", "i.tif", "--intensity-ring", "inf"]):
        with pytest.raises(SystemExit):
            parse_args(["m.tif", *bad])


def test_image_refusals_come_before_the_device():
    from skoots_amd.validate import lib as L
    shape = (3, 4, 5)
    for dtype in (torch.float32, torch.float16, torch.float64, torch.bool, torch.complex64):
        with pytest.raises(TypeError, match=str(dtype).replace(".", r"\.")):
            L.check_image(torch.zeros(shape, dtype=dtype), shape)
    with pytest.raises(TypeError):
        L.check_image(np.zeros(shape, np.uint8), shape)
    for bad in ((3, 4, 6), (1, 3, 5, 4), (2, 3, 4, 5), (60,), (3, 4, 5, 1)):
        with pytest.raises(ValueError, match="shape"):
            L.check_image(torch.zeros(bad, dtype=torch.uint8), shape)
    for dtype in (torch.uint8, torch.uint16, torch.int8, torch.int16, torch.int32, torch.int64):
        L.check_image(torch.zeros(shape, dtype=dtype), shape)
        L.check_image(torch.zeros((1,) + shape, dtype=dtype), shape)
    # the public functions refuse the image before they ask for a device tensor: host tensors get this far
    mask = torch.ones(shape, dtype=torch.int32)
    with pytest.raises(TypeError, match="float32"):
        L.instance_intensity(mask, torch.zeros(shape))
    with pytest.raises(ValueError, match="shape"):
        L.instance_intensity(mask, torch.zeros((3, 4, 6), dtype=torch.uint8))
    with pytest.raises(TypeError, match="float32"):
        L.intensity_ring(mask, torch.zeros(shape), 3.0)
    with pytest.raises(ValueError, match="MI355X"):
        L.instance_intensity(mask, torch.zeros(shape, dtype=torch.uint8))
    for bad in (0, -1.0, float("inf"), float("nan"), None, "x", True):
        with pytest.raises(ValueError, match="distance"):
            L.intensity_ring(mask, torch.zeros(shape, dtype=torch.uint8), bad)


def test_overflow_guard_matches_the_library():
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as L
    for shape, eb in (((2 ** 10, 2 ** 10, 2 ** 10), 1), ((2 ** 10, 2 ** 10, 2 ** 10), 2), ((2 ** 14, 2 ** 14, 2 ** 10), 2),
                      ((2 ** 14, 2 ** 14, 2 ** 3), 2), ((2 ** 20, 2 ** 20, 2 ** 8), 1), ((2 ** 21, 2 ** 20, 2 ** 5), 1),
                      ((2 ** 31 - 1, 1, 1), 2), ((2 ** 31 - 1, 2 ** 16, 1), 1), ((0, 5, 5), 2)):
        V = 255 if eb == 1 else 65535
        fits = shape[0] * shape[1] * shape[2] * V * max(V, *shape) < 2 ** 63
        rc = _ffi.lib.sk_instance_intensity(None, *shape, None, 1, 0, None, eb, 0, None, None, None, None)   # N = 0
        assert (rc == 0) == fits, (shape, eb, _ffi.last_error())
        if fits:
            L.check_intensity_shape(shape, eb)
        else:
            with pytest.raises(ValueError, match=r"2\^63"):
                L.check_intensity_shape(shape, eb)
    assert _ffi.lib.sk_abi_version() >= 25
    assert [_ffi.lib.sk_instance_intensity_row_values(k) for k in range(4)] == [6, 2, 256, 0]
    # the argument refusals need no device either: nothing is launched for them
    L_ = _ffi.lib
    assert L_.sk_instance_intensity(None, 4, 4, 4, None, 1, 1, None, 3, 0, None, None, None, None) == -1
    assert "elem_bytes" in _ffi.last_error()
    assert L_.sk_instance_intensity(None, 4, 4, 4, None, 1, 1, None, 2, 9, None, None, None, None) == -1
    assert L_.sk_instance_intensity(None, 4, 4, 4, None, 1, 1, None, 1, 1, None, None, None, None) == -1
    assert "shift" in _ffi.last_error()
    assert L_.sk_instance_intensity(None, 2 ** 21, 2 ** 21, 2 ** 21, None, 1, 1, None, 1, 0, None, None, None, None) == -1
    assert "2^63" in _ffi.last_error()
    assert L_.sk_instance_intensity(None, 4, 4, 4, None, 1, 1, None, 1, 0, None, None, None, None) == -1      # NULL outputs
