"""``sk_instance_stats`` (skoots_amd/csrc/instance_stats.hip) and everything on top of it -- ``stats_per_instance``,
``mask_to_bbox``, ``get_volume`` / ``get_face_area`` and ``python -m skoots_amd.validate.compare`` -- against a numpy
oracle in this file.  Every output of the kernel is an integer, so every comparison of it is exact equality.

The kernel works on tiles of 4 x 16 x 64 voxels (z along the 64 lanes of a wave) and keeps 32 rows per tile in LDS;
the shapes below are no multiples of any of these, exceed the table, and degenerate in every axis."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def oracle(lab):
    """(ids, sums (N, 13) int64, boxes (N, 6) int32) of an (X, Y, Z) integer array: np.add.at over the coordinates,
    faces by shifted comparisons with a -1 pad (outside the volume equals no row)."""
    lab = np.asarray(lab).astype(np.int64)
    ids = np.unique(lab)
    ids = ids[ids > 0]
    N = len(ids)
    row = np.where(lab > 0, np.searchsorted(ids, lab) + 1, 0)
    sums = np.zeros((N, 13), np.int64)
    boxes = np.zeros((N, 6), np.int32)
    x, y, z = (c.astype(np.int64) for c in np.nonzero(row))
    r = row[x, y, z] - 1
    for k, v in enumerate([np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z]):
        np.add.at(sums[:, k], r, v)
    pad = np.pad(row, 1, constant_values=-1)
    core = (slice(1, -1),) * 3
    for axis in range(3):
        for step in (-1, 1):
            nb = np.roll(pad, -step, axis=axis)[core]
            exposed = (row > 0) & (nb != row)
            sums[:, 10 + axis] += np.bincount(row[exposed] - 1, minlength=N)
    for k, c in enumerate((x, y, z)):
        lo = np.full(N, np.iinfo(np.int32).max, np.int64)
        hi = np.full(N, -1, np.int64)
        np.minimum.at(lo, r, c)
        np.maximum.at(hi, r, c)
        boxes[:, k], boxes[:, 3 + k] = lo, hi
    return ids, sums, boxes


def check(lab, dtype=torch.int32, out=None):
    """stats_per_instance on the device against the oracle; returns the device result"""
    from skoots_amd.validate.compare import stats_per_instance
    ids, sums, boxes = oracle(lab)
    got = out if out is not None else stats_per_instance(torch.from_numpy(np.asarray(lab)).to(dtype).to(DEV))
    assert got["id"].dtype == torch.int64 and got["voxels"].dtype == torch.int64
    assert got["sums"].dtype == torch.int64 and got["sums"].shape == (len(ids), 13)
    assert got["bbox"].dtype == torch.int32 and got["bbox"].shape == (len(ids), 6)
    assert got["faces"].dtype == torch.int64 and got["faces"].shape == (len(ids), 3)
    assert np.array_equal(got["id"].cpu().numpy(), ids)
    g = got["sums"].cpu().numpy()
    bad = np.argwhere(g != sums)
    assert bad.size == 0, f"{len(bad)} sums differ, first (row, column) {bad[0]}: {g[tuple(bad[0])]} != " \
                          f"{sums[tuple(bad[0])]}"
    assert np.array_equal(got["bbox"].cpu().numpy(), boxes)
    assert np.array_equal(got["voxels"].cpu().numpy(), sums[:, 0])
    assert np.array_equal(got["faces"].cpu().numpy(), sums[:, 10:13])
    return got


def blobs(shape, n, seed, id_max=100000, rmax=9):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32)
    g = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1)
    for i in rng.choice(np.arange(1, id_max), n, replace=False):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        rad = rng.uniform(1.5, rmax, 3)
        lab[(((g - c) / rad) ** 2).sum(-1) <= 1] = i
    return lab


@pytest.fixture(scope="module")
def volume1():
    """(19, 45, 130): Z is two wave rows and a bit, X and Y are no multiples of the tile"""
    lab = blobs((19, 45, 130), 30, seed=18)
    lab[2:9, 3:12, 60:70] = 41000                     # two boxes sharing the y = 11 | 12 face,
    lab[2:9, 12:20, 60:70] = 41001                    # across the z = 63 | 64 tile seam
    lab[:, 22, 64] = 77777                            # one object touching all six faces of the volume
    lab[9, :, 64] = 77777
    lab[9, 22, :] = 77777
    lab[0, 0, 0] = 90001                              # single voxels in two opposite corners
    lab[18, 44, 129] = 90002
    return lab


def test_blobs_sparse_ids(volume1):
    got = check(volume1)
    ids = got["id"].tolist()
    assert {41000, 41001, 77777, 90001, 90002} <= set(ids)
    box = got["bbox"][ids.index(77777)].tolist()
    assert box == [0, 0, 0, 18, 44, 129]
    assert got["touches_border"][ids.index(77777)].item() and got["touches_border"][ids.index(90002)].item()
    assert got["sums"][ids.index(90001)].tolist() == [1] + [0] * 9 + [2, 2, 2]
    assert not got["touches_border"][ids.index(41000)].item()


def test_every_voxel_its_own_label():
    """16 384 rows in four tiles: far more than the LDS table holds, the direct-to-global path carries the result."""
    rng = np.random.default_rng(5)
    lab = (rng.permutation(16 * 16 * 64) + 1).astype(np.int32).reshape(16, 16, 64)
    got = check(lab)
    assert bool((got["voxels"] == 1).all()) and bool((got["faces"] == 2).all())


def test_checkerboard():
    """Two labels in a 3-D checkerboard: every face of every voxel is exposed, every run has length 1."""
    g = np.indices((6, 18, 70)).sum(0) % 2
    got = check((g + 1).astype(np.int32))
    assert got["faces"].sum().item() == 6 * 6 * 18 * 70


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 1, 1), (1, 1, 70), (3, 70, 1)])
def test_degenerate_extents(shape):
    rng = np.random.default_rng(sum(shape))
    lab = rng.integers(0, 4, shape).astype(np.int32) * 7
    lab.flat[0] = 7
    check(lab)
    check(np.full(shape, 3, np.int32))


def test_all_background_and_one_label():
    from skoots_amd.validate.compare import stats_per_instance
    got = check(np.zeros((8, 9, 10), np.int32))
    want = {"id": ((0,), torch.int64), "voxels": ((0,), torch.int64), "volume": ((0,), torch.float64),
            "bbox": ((0, 6), torch.int32), "touches_border": ((0,), torch.bool), "centroid": ((0, 3), torch.float64),
            "face_area": ((0,), torch.float64), "faces": ((0, 3), torch.int64), "axis_lengths": ((0, 3), torch.float64),
            "sums": ((0, 13), torch.int64)}
    assert set(got) == set(want)
    for k, (shape, dtype) in want.items():
        assert tuple(got[k].shape) == shape and got[k].dtype == dtype and got[k].is_cuda, k
    assert stats_per_instance(torch.full((3, 3, 3), -5, dtype=torch.int32, device=DEV))["id"].numel() == 0
    assert stats_per_instance(torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV))["id"].numel() == 0

    got = check(np.full((8, 9, 10), 12, np.int32))
    assert got["faces"].tolist() == [[2 * 9 * 10, 2 * 8 * 10, 2 * 8 * 9]]      # the six walls
    assert got["bbox"].tolist() == [[0, 0, 0, 7, 8, 9]] and got["voxels"].tolist() == [720]


def test_huge_ids_take_the_relabel_route(monkeypatch):
    from skoots_amd.validate import lib as VL
    lab = np.zeros((4, 4, 4), np.int32)
    lab[0, 0, :3] = 2 ** 31 - 1
    lab[1:3, 1:3, 1:3] = 2 ** 30
    lab[3, 3, 3] = 5
    lab[3, 0, 0] = -9
    monkeypatch.setattr(VL, "_lut", lambda m: pytest.fail("the max id + 1 table was built for a 2^31 - 1 id"))
    got = check(lab)
    assert got["id"].tolist() == [5, 2 ** 30, 2 ** 31 - 1]
    big = lab.astype(np.int64)
    big[0, 0, :3] = 2 ** 40                           # beyond int32 altogether
    assert check(big, dtype=torch.int64)["id"].tolist() == [5, 2 ** 30, 2 ** 40]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int64])
def test_integer_dtypes_and_4d(dtype, volume1):
    from skoots_amd.validate.compare import stats_per_instance
    lab = (volume1[:7, :20, :66] % 120).astype(np.int32)
    x = torch.from_numpy(lab).to(dtype).to(DEV)
    check(lab, out=stats_per_instance(x[None]))
    with pytest.raises(TypeError):
        stats_per_instance(x.float())


def test_mask_to_bbox_against_reference(golden):
    from skoots_amd.validate.lib import mask_to_bbox
    g = golden("instance_stats.npz")
    ids, boxes = mask_to_bbox(torch.from_numpy(g["mask"]).to(DEV))
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == g["boxes"].shape
    assert np.array_equal(ids.cpu().numpy().astype(np.int64), g["ids"].astype(np.int64))
    assert np.array_equal(boxes.cpu().numpy().astype(np.int64), g["boxes"].astype(np.int64))
    check(g["mask"][0])


def test_single_mask_functions(volume1):
    from skoots_amd.validate.compare import stats_per_instance
    from skoots_amd.validate.stats import get_face_area, get_volume
    spacing = (0.5, 0.5, 3.0)
    x = torch.from_numpy(volume1).to(DEV)
    st = stats_per_instance(x, spacing)
    i = st["id"].tolist().index(77777)
    one = x == 77777
    assert get_volume(one).item() == st["voxels"][i].item() and get_volume(one).dtype == torch.int64
    assert get_volume(one, list(spacing)).item() == st["volume"][i].item()
    assert get_volume(one, torch.tensor(spacing)).item() == st["volume"][i].item()
    assert get_face_area(one, spacing).item() == st["face_area"][i].item()
    assert get_volume(torch.zeros_like(one)).item() == 0
    # the derived columns are the pure function of the sums
    from skoots_amd.validate.compare import derive
    for k, v in derive(st["sums"].cpu(), st["bbox"].cpu(), volume1.shape, spacing).items():
        assert st[k].is_cuda and torch.equal(st[k].cpu(), v), k


def test_two_runs_are_bit_identical(volume1):
    from skoots_amd.validate.lib import instance_sums
    x = torch.from_numpy(volume1).to(DEV)
    a, b = instance_sums(x), instance_sums(x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_non_default_stream(volume1):
    from skoots_amd.validate.compare import stats_per_instance
    x = torch.from_numpy(volume1).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = stats_per_instance(x)
    s.synchronize()
    check(volume1, out=got)


def test_overflow_guard_launches_nothing():
    from skoots_amd import _ffi
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    lut = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    sums = torch.full((1, 13), -7, dtype=torch.int64, device=DEV)
    boxes = torch.full((1, 6), -7, dtype=torch.int32, device=DEV)

    def call(X, Y, Z, N=1, lab_p=_ffi.ptr(lab)):
        rc = _ffi.lib.sk_instance_stats(lab_p, X, Y, Z, _ffi.ptr(lut), 1, N, _ffi.ptr(sums), _ffi.ptr(boxes),
                                        _ffi.stream_ptr(lab.device))
        torch.cuda.synchronize()
        return rc

    for shape in [(3000000, 3000000, 3000000), (1, 1, 2097152), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert call(*shape) == -1
        assert "2^63" in _ffi.last_error()
    assert call(4, 4, 4, N=-1) == -1
    assert call(-1, 4, 4) == -1
    assert call(4, 4, 4, lab_p=None) == -1 and "NULL" in _ffi.last_error()
    assert call(0, 4, 4) == 0 and call(4, 4, 4, N=0) == 0          # nothing to do: success, nothing written
    assert bool((sums == -7).all()) and bool((boxes == -7).all())
    assert call(4, 4, 4) == 0                                      # the same buffers, now measured
    assert sums[0, 0].item() == 64 and boxes[0].tolist() == [0, 0, 0, 3, 3, 3]
    assert _ffi.lib.sk_abi_version() >= 12


def test_command_end_to_end(tmp_path, volume1):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import main, stats_per_instance
    lab = volume1[:, :, :40].copy()
    x = torch.from_numpy(lab).to(DEV)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    spacing = (0.5, 0.25, 3.0)
    out = main([path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"])
    assert out == os.path.join(tmp_path, "mito_instance_stats.csv")
    lines = open(out).read().splitlines()
    assert lines[0] == f"Mask File: {path}" and lines[1] == "Spacing: 0.5 0.25 3.0"
    assert lines[2].split(",")[:3] == ["id", "voxels", "volume"] and len(lines[2].split(",")) == 17
    st = stats_per_instance(x, spacing)
    keep = (st["voxels"] >= 2).cpu().numpy()
    assert not keep.all() and keep.any()
    rows = [ln.split(",") for ln in lines[3:]]
    assert [int(r[0]) for r in rows] == st["id"].cpu().numpy()[keep].tolist()
    assert [int(r[1]) for r in rows] == st["voxels"].cpu().numpy()[keep].tolist()
    assert [[int(v) for v in r[3:9]] for r in rows] == st["bbox"].cpu().numpy()[keep].tolist()
    assert [bool(int(r[9])) for r in rows] == st["touches_border"].cpu().numpy()[keep].tolist()
    assert [float(r[2]) for r in rows] == st["volume"].cpu().numpy()[keep].tolist()
    assert [[float(v) for v in r[10:13]] for r in rows] == st["centroid"].cpu().numpy()[keep].tolist()
    assert [float(r[13]) for r in rows] == st["face_area"].cpu().numpy()[keep].tolist()
    assert [[float(v) for v in r[14:17]] for r in rows] == st["axis_lengths"].cpu().numpy()[keep].tolist()
    other = main([path, "--out", os.path.join(tmp_path, "all.csv")])
    assert other == os.path.join(tmp_path, "all.csv")
    assert len(open(other).read().splitlines()) == 3 + st["id"].numel()
