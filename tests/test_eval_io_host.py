"""Host side of eval()'s output writers (lib/deflate.py, zarr_store.save_device, tiff.write_stack) on CPU tensors: the
chunking, the store layout and the TIFF directories are the same code for both devices, only the encoder differs."""
import filecmp
import os
import zlib

import numpy as np
import pytest
import torch

from skoots_amd import _ffi
from skoots_amd.lib import deflate, tiff, zarr_store


def _same_tree(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    return names


def _one_voxel():
    arr = np.zeros((1, 300, 100, 70), np.uint8)
    arr[0, 299, 3, 69] = 7
    return arr


@pytest.mark.parametrize("make, chunks, n_files", [
    (lambda: np.random.default_rng(0).standard_normal((3, 300, 270, 70)).astype(np.float16), None, 3 * 2 * 2 * 2 + 1),
    (lambda: np.zeros((1, 256, 256, 64), np.uint8), None, 1),
    (lambda: np.random.default_rng(1).integers(-5, 5, (100, 37)).astype(np.int32), (32, 16), 4 * 3 + 1),
    (_one_voxel, None, 2),
], ids=["f16_edges", "all_zero", "int32_2d", "one_voxel"])
def test_save_device_on_cpu_equals_save(tmp_path, make, chunks, n_files):
    arr = make()
    a, b = str(tmp_path / "a.zarr"), str(tmp_path / "b.zarr")
    zarr_store.save(a, arr, chunks, compressor="zlib")
    zarr_store.save_device(b, torch.from_numpy(arr), chunks)
    names = _same_tree(a, b)
    assert len(names) == n_files
    assert open(os.path.join(a, ".zarray")).read() == open(os.path.join(b, ".zarray")).read()
    assert np.array_equal(zarr_store.load(b), arr)


def test_save_device_negative_zero_chunk_is_fill_value(tmp_path):
    arr = np.zeros((1, 8, 8, 8), np.float16)
    arr[0, :4] = -0.0
    a, b = str(tmp_path / "a.zarr"), str(tmp_path / "b.zarr")
    zarr_store.save(a, arr, (1, 4, 8, 8))
    zarr_store.save_device(b, torch.from_numpy(arr), (1, 4, 8, 8))
    assert _same_tree(a, b) == [".zarray"]


def test_save_device_small_budget_batches(tmp_path):
    arr = np.random.default_rng(2).integers(0, 3, (2, 40, 40, 8)).astype(np.uint8)
    a, b = str(tmp_path / "a.zarr"), str(tmp_path / "b.zarr")
    zarr_store.save(a, arr, (1, 16, 16, 8))
    zarr_store.save_device(b, torch.from_numpy(arr), (1, 16, 16, 8), budget_bytes=1)   # one chunk per batch
    _same_tree(a, b)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("shape", [(1, 5, 7), (4, 33, 21), (3, 64, 64)])
def test_write_stack_reads_back(tmp_path, dtype, shape):
    from PIL import Image
    rng = np.random.default_rng(3)
    hi = {np.uint8: 255, np.uint16: 65535, np.int32: 2 ** 31 - 1}[dtype]
    arr = rng.integers(0, hi, shape, endpoint=True).astype(dtype)
    arr[0, 0, :3] = (0, hi, 1)
    if dtype == np.int32:
        arr[-1, -1, -1] = -5
    for k, pages in enumerate((arr, torch.from_numpy(arr))):
        path = str(tmp_path / f"s{k}.tif")
        tiff.write_stack(path, pages)
        with Image.open(path) as im:
            assert im.n_frames == shape[0]
            got = []
            for z in range(shape[0]):
                im.seek(z)
                assert im.tag_v2[259] == 8 and len(im.tag_v2[273]) == 1 and im.tag_v2[273][0] % 2 == 0
                got.append(np.array(im))
        got = np.stack(got)
        assert got.shape == shape and np.array_equal(got.astype(np.int64), arr.astype(np.int64))
        back = tiff.read_image(path)
        assert back.shape == shape and back.dtype == dtype and np.array_equal(back, arr)


def test_write_label_stack_narrows_like_the_host_writer(tmp_path):
    lab = torch.zeros((2, 6, 5), dtype=torch.int32)
    lab[1, 2, 3] = 65535
    tiff.write_label_stack(str(tmp_path / "a.tif"), lab)
    a = tiff.read_image(str(tmp_path / "a.tif"))
    assert a.dtype == np.uint16 and np.array_equal(a, lab.numpy())
    lab[0, 0, 0] = 65536
    tiff.write_label_stack(str(tmp_path / "b.tif"), lab)
    b = tiff.read_image(str(tmp_path / "b.tif"))
    assert b.dtype == np.int32 and np.array_equal(b, lab.numpy())


def test_write_stack_refuses_what_needs_bigtiff(tmp_path, monkeypatch):
    class Sized:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    def fake(rows, elem_bytes=1, skip_zero=False, timings=None):
        return [Sized(2 ** 30) for _ in range(rows.shape[0])]

    monkeypatch.setattr(deflate, "deflate_streams", fake)
    path = str(tmp_path / "big.tif")
    with pytest.raises(ValueError, match="BigTIFF"):
        tiff.write_stack(path, np.zeros((4, 2, 2), np.uint8))
    assert not os.path.exists(path)


def test_write_stack_rejects_other_dtypes(tmp_path):
    with pytest.raises(ValueError):
        tiff.write_stack(str(tmp_path / "x.tif"), np.zeros((2, 3, 3), np.float32))
    with pytest.raises(ValueError):
        tiff.write_stack(str(tmp_path / "x.tif"), np.zeros((3, 3), np.uint8))


def test_deflate_bound_contract():
    prev = -1
    for n in (0, 1, 65535, 65536, 8 << 20):
        b = int(_ffi.lib.sk_deflate_bound(n))
        assert n + 8 <= b <= n + n // 1024 + 64, (n, b)
        assert b == deflate.bound(n)
        assert b >= prev
        prev = b
    sizes = [int(_ffi.lib.sk_deflate_bound(n)) for n in range(0, 200000, 977)]
    assert sizes == sorted(sizes)
    assert int(_ffi.lib.sk_deflate_workspace_bytes(3, 1 << 20)) >= 3 * (1 << 20)


def test_deflate_streams_argument_checks_need_no_gpu():
    # every argument is checked before anything is launched or written
    with pytest.raises(ValueError, match="elem_bytes"):
        _ffi.check(_ffi.lib.sk_deflate_streams(None, 1, 16, 3, None, None, None, None, 0, None))
    with pytest.raises(ValueError, match="stream_bytes"):
        _ffi.check(_ffi.lib.sk_deflate_streams(None, 1, -1, 1, None, None, None, None, 0, None))
    with pytest.raises(ValueError, match="dst_offsets"):
        _ffi.check(_ffi.lib.sk_deflate_streams(None, 1, 16, 1, None, None, None, None, 0, None))


def test_deflate_streams_cpu_rows():
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 4, (5, 1000)).astype(np.uint8)
    rows[1] = 0
    rows[3] = 0
    t = torch.from_numpy(rows)
    out = deflate.deflate_streams(t, elem_bytes=2)
    assert [zlib.decompress(s) for s in out] == [r.tobytes() for r in rows]
    out = deflate.deflate_streams(t, skip_zero=True)
    assert [s is None for s in out] == [False, True, False, True, False]
    assert all(zlib.decompress(s) == rows[i].tobytes() for i, s in enumerate(out) if s is not None)
    assert deflate.deflate_streams(torch.zeros((0, 16), dtype=torch.uint8)) == []
    empty = deflate.deflate_streams(torch.zeros((3, 0), dtype=torch.uint8))
    assert len(empty) == 3 and all(zlib.decompress(s) == b"" for s in empty)
    with pytest.raises(ValueError):
        deflate.deflate_streams(torch.zeros((3, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        deflate.deflate_streams(t, elem_bytes=3)
