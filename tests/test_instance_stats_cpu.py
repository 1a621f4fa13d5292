"""Host side of the per-instance measurements (skoots_amd/validate/compare.py): ``derive`` on
sums built with numpy from voxel coordinates, the CSV text, and the overflow guard.  No GPU is used here; the kernel
that produces the sums is tested in tests/test_hip_instance_stats.py."""
import math

import numpy as np
import pytest
import torch

from skoots_amd.validate import compare as CMP
from skoots_amd.validate import lib as VL

SPACINGS = [(1.0, 1.0, 1.0), (0.5, 0.5, 3.0)]
SHAPE = (40, 41, 42)


def _box(origin, size):
    g = np.stack(np.meshgrid(*(np.arange(o, o + k) for o, k in zip(origin, size)), indexing="ij"), -1)
    return g.reshape(-1, 3)


def _objects():
    ell = np.concatenate([_box((5, 6, 7), (9, 3, 2)), _box((5, 9, 7), (3, 8, 2))])     # an L, two voxels thick
    return {
        "box": _box((3, 4, 5), (4, 7, 11)),
        "ell": ell,
        "voxel": np.array([[17, 0, 41]]),
        "diagonal": np.stack([np.arange(2, 21)] * 3, -1),
    }


def _sums_and_box(c):
    """the kernel's 13 sums and its box, from (n, 3) integer coordinates"""
    c = c.astype(np.int64)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    occupied = {tuple(v) for v in c.tolist()}
    faces = [0, 0, 0]
    for v in c.tolist():
        for axis in range(3):
            for step in (-1, 1):
                nb = list(v)
                nb[axis] += step
                outside = not (0 <= nb[axis] < SHAPE[axis])
                faces[axis] += outside or tuple(nb) not in occupied
    sums = [len(c), x.sum(), y.sum(), z.sum(), (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(),
            (x * z).sum(), (y * z).sum(), *faces]
    return np.array(sums, np.int64), np.concatenate([c.min(0), c.max(0)]).astype(np.int32)


def _direct(c, spacing):
    """two-pass float64 on the coordinates themselves"""
    s = np.array(spacing)
    p = c.astype(np.float64) * s
    centroid = p.mean(0)
    d = p - centroid
    lam = np.linalg.eigvalsh(d.T @ d / len(c))[::-1]
    # an exactly flat object (a line, a single voxel) has exactly zero eigenvalues; LAPACK leaves round-off of either
    # sign there, which the square root would amplify: the rule of compare.FLAT_EIGENVALUE
    lam = np.where(lam > CMP.FLAT_EIGENVALUE * lam[0], lam, 0.0)
    return centroid, len(c) * s.prod(), 2.0 * np.sqrt(5.0 * lam)


@pytest.fixture(scope="module")
def measured():
    objs = _objects()
    sb = [_sums_and_box(c) for c in objs.values()]
    return objs, torch.from_numpy(np.stack([a for a, _ in sb])), torch.from_numpy(np.stack([b for _, b in sb]))


@pytest.mark.parametrize("spacing", SPACINGS)
def test_derive_against_two_pass(measured, spacing):
    objs, sums, boxes = measured
    d = CMP.derive(sums, boxes, SHAPE, spacing)
    sx, sy, sz = spacing
    for i, (name, c) in enumerate(objs.items()):
        centroid, volume, axes = _direct(c, spacing)
        f = sums[i, 10:13].numpy()
        area = f[0] * sy * sz + f[1] * sx * sz + f[2] * sx * sy
        print(name, d["centroid"][i].tolist(), centroid.tolist(), d["axis_lengths"][i].tolist(), axes.tolist())
        np.testing.assert_allclose(d["centroid"][i].numpy(), centroid, rtol=1e-9, atol=0, err_msg=name)
        np.testing.assert_allclose(d["volume"][i].item(), volume, rtol=1e-9, atol=0, err_msg=name)
        np.testing.assert_allclose(d["face_area"][i].item(), area, rtol=1e-9, atol=0, err_msg=name)
        np.testing.assert_allclose(d["axis_lengths"][i].numpy(), axes, rtol=1e-9, atol=0, err_msg=name)
        assert d["voxels"][i].item() == len(c)
    assert d["bbox"].dtype == torch.int32 and torch.equal(d["bbox"], boxes)
    assert d["touches_border"].tolist() == [False, False, True, False]
    assert d["axis_lengths"][2].tolist() == [0.0, 0.0, 0.0]                  # a single voxel
    assert d["axis_lengths"][3, 1:].tolist() == [0.0, 0.0]                  # a line has one axis
    for k in ("volume", "centroid", "face_area", "axis_lengths"):
        assert d[k].dtype == torch.float64


@pytest.mark.parametrize("spacing", SPACINGS)
def test_box_axes_closed_form(measured, spacing):
    """The variance of k equally spaced points at distance s is s^2 (k^2 - 1) / 12."""
    _, sums, boxes = measured
    d = CMP.derive(sums, boxes, SHAPE, spacing)
    want = sorted((2.0 * math.sqrt(5.0 * (k * k - 1) / 12.0 * s * s) for k, s in zip((4, 7, 11), spacing)),
                  reverse=True)
    np.testing.assert_allclose(d["axis_lengths"][0].numpy(), want, rtol=1e-9, atol=0)
    # the faces of an a x b x c box: two walls per axis
    assert sums[0, 10:13].tolist() == [2 * 7 * 11, 2 * 4 * 11, 2 * 4 * 7]


def test_derive_empty():
    d = CMP.derive(torch.zeros((0, 13), dtype=torch.int64), torch.zeros((0, 6), dtype=torch.int32), SHAPE)
    assert d["axis_lengths"].shape == (0, 3) and d["centroid"].shape == (0, 3) and d["volume"].shape == (0,)
    assert d["touches_border"].dtype == torch.bool and d["touches_border"].shape == (0,)


# a 2 x 2 x 2 cube at the origin and the single voxel (3, 4, 5) of a (4, 5, 6) mask
_CSV_SUMS = torch.tensor([[8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 8, 8, 8],
                          [1, 3, 4, 5, 9, 16, 25, 12, 15, 20, 2, 2, 2]], dtype=torch.int64)
_CSV_BOXES = torch.tensor([[0, 0, 0, 1, 1, 1], [3, 4, 5, 3, 4, 5]], dtype=torch.int32)
_CSV_HEAD = ("Mask File: dir/mask.tif\n"
             "Spacing: 0.5 0.5 3.0\n"
             "id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,axis_minor\n")
_CSV_ROW_5 = "5,8,6.0,0,0,0,1,1,1,1,0.25,0.25,1.5,26.0,6.708203932499369,1.118033988749895,1.118033988749895\n"
_CSV_ROW_9 = "9,1,0.75,3,4,5,3,4,5,1,1.5,2.0,15.0,6.5,0.0,0.0,0.0\n"


def test_csv_text():
    text = CMP.format_csv("dir/mask.tif", [5, 9], _CSV_SUMS, _CSV_BOXES, (4, 5, 6), (0.5, 0.5, 3.0))
    assert text == _CSV_HEAD + _CSV_ROW_5 + _CSV_ROW_9


def test_csv_min_voxels():
    args = ("dir/mask.tif", torch.tensor([5, 9]), _CSV_SUMS, _CSV_BOXES, (4, 5, 6), (0.5, 0.5, 3.0))
    assert CMP.format_csv(*args, min_voxels=2) == _CSV_HEAD + _CSV_ROW_5
    assert CMP.format_csv(*args, min_voxels=8) == _CSV_HEAD + _CSV_ROW_5
    assert CMP.format_csv(*args, min_voxels=9) == _CSV_HEAD


def test_overflow_guard_on_the_host():
    """X Y Z max(X, Y, Z)^2 < 2^63, checked in Python before the library is called."""
    VL.check_shape((2048, 2048, 512))
    VL.check_shape((1, 1, 2097151))                      # 2097151^3 < 2^63
    VL.check_shape((0, 5, 5))
    for bad in [(1, 1, 2097152), (2 ** 21, 2 ** 21, 2 ** 21), (2 ** 31, 1, 1), (100000, 100000, 100000)]:
        with pytest.raises(ValueError, match="2\\^63"):
            VL.check_shape(bad)


def test_guard_runs_before_the_library(monkeypatch):
    """instance_sums refuses the shape itself: the library function is not reached."""
    called = []
    monkeypatch.setattr(VL, "_as_volume", lambda x, name: x)
    monkeypatch.setattr(VL._ffi, "check", lambda rc: called.append(rc))

    class Huge:
        shape = (1, 1, 2097152)

    with pytest.raises(ValueError, match="2\\^63"):
        VL.instance_sums(Huge())
    assert not called


def test_host_tensor_is_refused():
    x = torch.zeros((3, 4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        CMP.stats_per_instance(x)
    from skoots_amd.validate import stats as ST
    with pytest.raises(ValueError, match="no CPU fallback"):
        ST.get_volume(x)


def test_spacing_is_checked():
    with pytest.raises(ValueError):
        CMP.derive(_CSV_SUMS, _CSV_BOXES, (4, 5, 6), (1.0, 1.0))
    with pytest.raises(ValueError):
        CMP.derive(_CSV_SUMS, _CSV_BOXES, (4, 5, 6), (1.0, 0.0, 1.0))
