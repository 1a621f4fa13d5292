"""``sk_label_planes`` and ``sk_plane_overlaps`` (skoots_amd/csrc/stitch.hip) and ``watershed_and_stitch`` on the device:
the labelling against ``scipy.ndimage.label`` per plane, the overlap rows against ``numpy.unique`` counts, the whole tool
against the reference's own results (tests/golden/flood_and_stitch.npz) and against the CPU route.  Every comparison is
exact."""
import os

import numpy as np
import pytest
import torch

from tests import stitch_reference as R

from skoots_amd.lib import tiff
from skoots_amd.utils import flood_and_stitch as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_G = np.load(os.path.join(os.path.dirname(__file__), "golden", "flood_and_stitch.npz"))
NAMES = [str(n) for n in _G["names"]]


def spiral(H, W):
    """A one-voxel-wide path winding inwards with one background voxel between its turns: one component."""
    g = np.zeros((H, W), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not g[ny, nx] and not (0 <= ny2 < H and 0 <= nx2 < W and g[ny2, nx2]):
                y, x = ny, nx
                g[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return g


def u_shape():
    """The first raster voxel is the top of the RIGHT arm, tiles away from the left arm; the lone voxel between the
    arms comes later in raster order and must be number 2."""
    g = np.zeros((40, 150), dtype=np.uint8)
    g[5:, 3] = 1
    g[0:, 140] = 1
    g[39, 3:141] = 1
    g[2, 70] = 1
    return g


def _volumes():
    rng = np.random.default_rng(59)
    stripes = np.zeros((2, 47, 47), dtype=np.uint8)     # m = 16 stripes of two rows / columns, one apart
    stripes[0, np.arange(47) % 3 != 2, :] = 1
    stripes[1, :, np.arange(47) % 3 != 2] = 1
    return {
        "spiral": spiral(67, 131)[None],
        "checkerboard": (np.add.outer(np.arange(33), np.arange(65)) % 2 == 0).astype(np.uint8)[None],
        "ones_zeros": np.stack([np.ones((64, 64), np.uint8), np.zeros((64, 64), np.uint8), np.ones((64, 64), np.uint8),
                                np.ones((64, 64), np.uint8)]),
        "height_one": (rng.random((3, 1, 200)) < 0.6).astype(np.uint8),
        "width_one": (rng.random((3, 200, 1)) < 0.6).astype(np.uint8),
        "one_plane": (rng.random((1, 40, 70)) < 0.55).astype(np.uint8),
        "percolation": (rng.random((5, 130, 257)) < 0.59).astype(np.uint8),
        "u_shape": np.stack([u_shape(), u_shape()[::-1].copy()]),
        "two_full_planes": np.ones((2, 50, 70), dtype=np.uint8),
        "stripes": stripes,
    }


VOLUMES = _volumes()
_REF = {}


def reference(name, dim):
    """(labels, offsets, rows) by scipy / numpy, computed once per volume and axis."""
    key = (name, dim)
    if key not in _REF:
        mask = VOLUMES[name] if name in VOLUMES else _G[f"mask_{name}"]
        _REF[key] = R.plane_tables(mask, dim)
    return _REF[key]


def _mask(name):
    return VOLUMES[name] if name in VOLUMES else _G[f"mask_{name}"]


def _check_labelling(name, dim, strided):
    want_labels, want_offsets, _ = reference(name, dim)
    labels, offsets = F.label_planes(torch.from_numpy(_mask(name)).to(DEV), dim, strided=strided)
    assert labels.dtype == torch.int32 and labels.is_contiguous()
    assert np.array_equal(offsets.cpu().numpy(), want_offsets), (name, dim)
    assert np.array_equal(labels.cpu().numpy(), want_labels), (name, dim)
    return labels, offsets


def test_shapes_are_what_they_claim():
    import scipy.ndimage
    assert scipy.ndimage.label(VOLUMES["spiral"][0])[1] == 1 and VOLUMES["spiral"].sum() > 67 * 131 // 3
    assert reference("checkerboard", 0)[1][-1] == (33 * 65 + 1) // 2
    u = reference("u_shape", 0)[0][0]
    assert u[0, 140] == 1 and u[5, 3] == 1 and u[2, 70] == 2
    assert len(reference("stripes", 0)[2]) == 16 * 16


@pytest.mark.parametrize("name", NAMES)
def test_label_planes_fixture_masks_every_axis_in_place(name):
    for dim in range(3):
        _check_labelling(name, dim, strided=True)
    _check_labelling(name, 2, strided=False)     # the permuted copy the wrapper makes for dim 2


@pytest.mark.parametrize("name", [n for n in VOLUMES])
def test_label_planes_shapes(name):
    _check_labelling(name, 0, strided=True)


def test_label_planes_refuses_bad_arguments():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_label_planes_workspace_bytes(0, 4, 4) == 0
    assert _ffi.lib.sk_label_planes_workspace_bytes(2048, 1024, 1024) == 0
    assert _ffi.lib.sk_label_planes_workspace_bytes(1 << 23, 1, 1) == 0       # a workgroup per tile: too many tiny planes
    assert _ffi.lib.sk_label_planes_workspace_bytes(1 << 22, 1, 1) > 0
    with pytest.raises(ValueError, match="tiles"):
        F.label_planes(torch.zeros((1 << 23, 1, 1), dtype=torch.uint8, device=DEV), 0)
    m = torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros((2, 4, 4), dtype=torch.int32, device=DEV)
    off = torch.zeros(3, dtype=torch.int32, device=DEV)
    ws = torch.zeros(16, dtype=torch.uint8, device=DEV)     # too small
    rc = _ffi.lib.sk_label_planes(_ffi.ptr(m), 2, 4, 4, 16, 4, 1, _ffi.ptr(out), 16, 4, 1, _ffi.ptr(off), _ffi.ptr(off),
                                  _ffi.ptr(ws), 16, _ffi.stream_ptr(torch.device(DEV)))
    assert rc == -1 and "workspace" in _ffi.last_error()


@pytest.mark.parametrize("name", NAMES + [n for n in VOLUMES])
def test_plane_overlaps(name):
    dims = range(3) if name in NAMES else (0,)
    for dim in dims:
        want_labels, want_offsets, want_rows = reference(name, dim)
        labels = torch.from_numpy(want_labels).to(DEV)
        rows = F.plane_overlaps(labels, torch.from_numpy(want_offsets), dim)
        assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), want_rows), (name, dim)


def test_plane_overlaps_one_key_for_two_full_planes():
    labels, offsets, want_rows = reference("two_full_planes", 0)
    assert want_rows.tolist() == [[1, 2, 50 * 70]]
    rows, needed, complete = F._overlaps_once(torch.from_numpy(labels).to(DEV), 4)
    assert complete and needed == 1 and rows.cpu().tolist() == [[1, 2, 50 * 70]]


def test_plane_overlaps_counts_past_a_small_table():
    want_labels, want_offsets, want_rows = reference("stripes", 0)
    labels = torch.from_numpy(want_labels).to(DEV)
    rows, needed, complete = F._overlaps_once(labels, 8)
    assert not complete and needed == 16 * 16 and rows.shape[0] <= 8
    stored = {tuple(r) for r in rows.cpu().tolist()}
    assert stored <= {tuple(r) for r in want_rows.tolist()}          # what fitted is right, counts included
    again = F.plane_overlaps(labels, torch.from_numpy(want_offsets), 0, capacity=8)
    assert np.array_equal(again.cpu().numpy(), want_rows)


@pytest.mark.parametrize("name", NAMES)
def test_watershed_and_stitch_equals_reference(name):
    for dim in range(3):
        got = F.watershed_and_stitch(torch.from_numpy(_G[f"mask_{name}"]).to(DEV), dim)
        assert got.dtype == torch.int32 and got.device.type == "cuda"
        assert np.array_equal(got.cpu().numpy(), R.first_seen(_G[f"labels_{name}_d{dim}"])), (name, dim)


@pytest.fixture(scope="module")
def field():
    import scipy.ndimage
    rng = np.random.default_rng(4096)
    return (scipy.ndimage.gaussian_filter(rng.standard_normal((40, 96, 80)), (0.8, 2, 2)) > 0.02).astype(np.uint8)


@pytest.mark.parametrize("dim", [0, 1, 2])
def test_device_route_equals_cpu_route(field, dim):
    want = F.watershed_and_stitch(torch.from_numpy(field), dim)
    got = F.watershed_and_stitch(torch.from_numpy(field).to(DEV), dim)
    assert int(want.max()) > 10 and torch.equal(got.cpu(), want)


def test_command_on_the_device_equals_cpu_run(field, tmp_path):
    (tmp_path / "gpu").mkdir()
    (tmp_path / "cpu").mkdir()
    pages = torch.from_numpy(field * 255)
    outs = []
    for sub in ("gpu", "cpu"):
        path = str(tmp_path / sub / "mask.tif")
        tiff.write_stack(path, pages)
        outs.append(F.main([path, "-d", "0"]) if sub == "gpu" else F.flood_stitch_save(path, 0, device="cpu"))
    assert outs[0].endswith("mask_replaced.tif")
    a, b = tiff.read_stack(outs[0], "cpu"), tiff.read_stack(outs[1], "cpu")
    assert a.dtype == b.dtype and torch.equal(a, b) and int(a.to(torch.int32).max()) > 10
