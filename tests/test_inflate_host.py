"""Host side of the device readers (lib/deflate.py: inflate_streams, zarr_store.load_device, tiff.scan / read_stack) on
the CPU device, where the stdlib's zlib stands in for csrc/inflate.hip: everything above the kernel -- batching, chunk
scatter, the TIFF directory scan, predictor, fallbacks, error reporting -- runs here without a GPU."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from skoots_amd import _ffi
from skoots_amd.lib import deflate, tiff, zarr_store
from tests import inflate_corpus as C


# ------------------------------------------------------------------------------------------ inflate_streams
def test_inflate_streams_cpu_good_streams():
    pays = [C.pattern(p, n) for p in C.PATTERNS for n in (0, 1, 259, 40000)]
    out, offs = deflate.inflate_streams([zlib.compress(p, 6) for p in pays], [len(p) for p in pays], "cpu")
    assert out.dtype == torch.uint8 and out.ndim == 1 and offs[-1] == sum(len(p) for p in pays)
    for p, a, b in zip(pays, offs[:-1], offs[1:]):
        assert out[a:b].numpy().tobytes() == p
    same = [C.pattern(p, 1000) for p in C.PATTERNS]
    rows = deflate.inflate_streams([zlib.compress(p) for p in same], 1000, "cpu")
    assert tuple(rows.shape) == (len(same), 1000)
    assert [r.numpy().tobytes() for r in rows] == same
    raw = deflate.inflate_streams([C.ENCODERS["raw"][1](p) for p in same], 1000, "cpu", wrapper="raw")
    assert torch.equal(raw, rows)
    buf = torch.zeros(len(same) * 1000, dtype=torch.uint8)
    deflate.inflate_streams([zlib.compress(p) for p in same], 1000, "cpu", out=buf)
    assert torch.equal(buf.view(len(same), 1000), rows)
    rows = deflate.inflate_streams([zlib.compress(p) for p in same], np.prod([10, 100]), "cpu")   # a numpy integer
    assert tuple(rows.shape) == (len(same), 1000)
    empty, offs = deflate.inflate_streams([], [], "cpu")
    assert empty.numel() == 0 and offs == [0]


@pytest.mark.parametrize("case", C.named_errors()[:-2], ids=lambda c: c.name)
def test_inflate_streams_cpu_bad_stream_names_its_index(case):
    good = zlib.compress(b"abc" * 50)
    with pytest.raises(ValueError, match=r"stream 1 of 3 does not inflate"):
        deflate.inflate_streams([good, case.stream, good], [150, case.size, 150], "cpu")


def test_inflate_error_carries_the_index():
    good = zlib.compress(b"abc" * 50)
    with pytest.raises(deflate.InflateError) as e:
        deflate.inflate_streams([good, good, good[:-3]], 150, "cpu")
    assert e.value.index == 2 and isinstance(e.value, ValueError) and e.value.reason in str(e.value)


def test_inflate_streams_cpu_hand_assembled_and_arguments():
    for c in C.hand_assembled():
        out = deflate.inflate_streams([c.stream], c.size, "cpu", wrapper="raw")
        assert out[0].numpy().tobytes() == c.expect, c.name
    with pytest.raises(ValueError, match="wrapper"):
        deflate.inflate_streams([b""], 0, "cpu", wrapper="gzip")
    with pytest.raises(ValueError, match="sizes"):
        deflate.inflate_streams([b"", b""], [1], "cpu")
    with pytest.raises(ValueError, match="out must be"):
        deflate.inflate_streams([zlib.compress(b"ab")], 2, "cpu", out=torch.zeros(3, dtype=torch.uint8))


def test_inflate_streams_argument_checks_need_no_gpu():
    """sk_inflate_streams / sk_tiff_undo_predictor refuse bad arguments before any launch, so this runs without a device."""
    lib = _ffi.lib
    with pytest.raises(ValueError, match="n_streams"):
        _ffi.check(lib.sk_inflate_streams(None, None, -1, None, None, 1, None, None))
    with pytest.raises(ValueError, match="wrapper"):
        _ffi.check(lib.sk_inflate_streams(None, None, 1, None, None, 2, None, None))
    with pytest.raises(ValueError, match="src or dst"):
        _ffi.check(lib.sk_inflate_streams(None, None, 1, None, None, 1, None, None))
    with pytest.raises(ValueError, match="src_offsets"):
        _ffi.check(lib.sk_inflate_streams(16, 4, 1, 16, 8, 1, 8, None))
    with pytest.raises(ValueError, match="dst_offsets"):
        _ffi.check(lib.sk_inflate_streams(16, 8, 1, 16, 12, 1, 8, None))
    with pytest.raises(ValueError, match="status"):
        _ffi.check(lib.sk_inflate_streams(16, 8, 1, 16, 8, 1, 2, None))
    _ffi.check(lib.sk_inflate_streams(None, None, 0, None, None, 1, None, None))   # nothing to do
    with pytest.raises(ValueError, match="bytes_per_sample"):
        _ffi.check(lib.sk_tiff_undo_predictor(16, 1, 1, 1, 3, None))
    with pytest.raises(ValueError, match="samples_per_pixel"):
        _ffi.check(lib.sk_tiff_undo_predictor(16, 1, 1, 0, 1, None))
    with pytest.raises(ValueError, match="n_rows"):
        _ffi.check(lib.sk_tiff_undo_predictor(16, -1, 1, 1, 1, None))
    with pytest.raises(ValueError, match="row_pixels"):
        _ffi.check(lib.sk_tiff_undo_predictor(16, 1, -1, 1, 1, None))
    with pytest.raises(ValueError, match="aligned"):
        _ffi.check(lib.sk_tiff_undo_predictor(18, 1, 1, 1, 4, None))
    _ffi.check(lib.sk_tiff_undo_predictor(None, 0, 5, 1, 2, None))
    assert _ffi.lib.sk_abi_version() >= 10


# ------------------------------------------------------------------------------------------ load_device
def _field(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 7, shape)
    a = np.where(rng.random(shape) < 0.7, 0, a)
    return a.astype(dtype)


def _same(t, arr):
    assert tuple(t.shape) == arr.shape
    assert t.numpy().dtype == arr.dtype
    assert t.numpy().tobytes() == arr.tobytes()


def test_load_device_cpu_equals_load(tmp_path):
    a = _field((3, 70, 33, 21), np.float16, 1)
    a[a == 3] = -0.0
    p = str(tmp_path / "f16.zarr")
    zarr_store.save(p, a, chunks=(2, 32, 16, 8))       # edge chunks on every axis: 3 = 2 + 1, 70 = 64 + 6, 33, 21
    _same(zarr_store.load_device(p, "cpu"), zarr_store.load(p))
    _same(zarr_store.load_device(p, "cpu", budget_bytes=1), a)    # one chunk per batch

    b = _field((2, 40, 40, 10), np.uint8, 2)
    b[:, :16, :16, :] = 0                               # chunks that hold only the fill value are not written
    p = str(tmp_path / "missing.zarr")
    zarr_store.save(p, b, chunks=(1, 16, 16, 10))
    assert not os.path.exists(os.path.join(p, "0.0.0.0"))
    _same(zarr_store.load_device(p, "cpu"), b)

    c = _field((37, 53), np.int32, 3) * 100000
    p = str(tmp_path / "i32.zarr")
    zarr_store.save(p, c, chunks=(16, 16))
    _same(zarr_store.load_device(p, "cpu"), c)

    p = str(tmp_path / "raw.zarr")
    zarr_store.save(p, c, chunks=(16, 20), compressor=None)
    _same(zarr_store.load_device(p, "cpu"), c)


def test_load_device_cpu_gzip_and_refusals(tmp_path):
    c = _field((20, 30), np.uint16, 4)
    p = str(tmp_path / "gz.zarr")
    zarr_store.save(p, c, chunks=(8, 16))
    import json
    meta = json.load(open(os.path.join(p, ".zarray")))
    meta["compressor"] = {"id": "gzip", "level": 1}
    json.dump(meta, open(os.path.join(p, ".zarray"), "w"))
    for fn in os.listdir(p):
        if fn != ".zarray":
            raw = zlib.decompress(open(os.path.join(p, fn), "rb").read())
            open(os.path.join(p, fn), "wb").write(gzip.compress(raw))
    _same(zarr_store.load_device(p, "cpu"), c)
    _same(zarr_store.load_device(p, "cpu"), zarr_store.load(p))

    meta["compressor"] = {"id": "blosc"}
    json.dump(meta, open(os.path.join(p, ".zarray"), "w"))
    with pytest.raises(RuntimeError) as e_dev:
        zarr_store.load_device(p, "cpu")
    with pytest.raises(RuntimeError) as e_host:
        zarr_store.load(p)
    assert str(e_dev.value) == str(e_host.value)

    p = str(tmp_path / "bad.zarr")
    zarr_store.save(p, c, chunks=(8, 16))
    with open(os.path.join(p, "1.1"), "r+b") as f:
        f.seek(5)
        f.write(b"\xff\xff\xff")
    with pytest.raises(ValueError, match=r"1\.1"):
        zarr_store.load_device(p, "cpu")


# ------------------------------------------------------------------------------------------ tiff.scan / read_stack
def _pil_save(path, arr, **kw):
    from PIL import Image
    pages = [Image.fromarray(p) for p in arr]
    pages[0].save(path, save_all=True, append_images=pages[1:], **kw)


def _stack(dtype, z, h, w, seed=0):
    rng = np.random.default_rng(seed)
    hi = {np.uint8: 200, np.uint16: 60000, np.int32: 100000}[dtype]
    a = rng.integers(0, hi, (z, h, w))
    a[:, : h // 2] = a[:, :1]          # something for the encoder to find
    return a.astype(dtype)


PIL_CASES = [(dt, comp, pred, z, h, w)
             for dt in (np.uint8, np.uint16, np.int32)
             for comp, pred in (("tiff_adobe_deflate", 1), ("tiff_adobe_deflate", 2), ("raw", 1))
             for z, h, w in ((3, 300, 301), (1, 17, 5))]


@pytest.mark.parametrize("dt,comp,pred,z,h,w", PIL_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}-p{c[2]}-z{c[3]}w{c[5]}" for c in PIL_CASES])
def test_scan_and_read_stack_on_pillow_files(tmp_path, dt, comp, pred, z, h, w):
    arr = _stack(dt, z, h, w, seed=h)
    path = str(tmp_path / "a.tif")
    _pil_save(path, arr, compression=comp, **({"tiffinfo": {317: 2}} if pred == 2 else {}))
    ref = tiff.read_image(path)
    assert np.array_equal(ref, arr)
    plan = tiff.scan(path)
    assert plan is not None and plan.shape == arr.shape and plan.dtype == ref.dtype and len(plan.pages) == z
    for p in plan.pages:
        assert (p.width, p.height, p.bits, p.samples_per_pixel) == (w, h, 8 * arr.dtype.itemsize, 1)
        assert p.predictor == pred and p.compression == (1 if comp == "raw" else 8)
        assert len(p.strip_offsets) == len(p.strip_byte_counts) == -(-h // p.rows_per_strip)
    if (h, w) == (300, 301) and dt == np.uint16 and comp != "raw":
        assert len(plan.pages[0].strip_offsets) == 3 and plan.pages[0].rows_per_strip == 108   # several strips per page
    got = tiff.read_stack(path, "cpu")
    _same(got, ref)


def test_read_stack_cpu_rgb_and_write_stack_files(tmp_path):
    rgb = np.random.default_rng(1).integers(0, 255, (2, 40, 31, 3)).astype(np.uint8)
    rgb[:, :, 10:] = rgb[:, :, 9:10]
    for k, kw in enumerate(({"compression": "tiff_adobe_deflate"}, {"compression": "tiff_adobe_deflate", "tiffinfo": {317: 2}},
                            {"compression": "raw"})):
        path = str(tmp_path / f"rgb{k}.tif")
        _pil_save(path, rgb, **kw)
        assert tiff.scan(path) is not None and tiff.scan(path).shape == rgb.shape
        _same(tiff.read_stack(path, "cpu"), tiff.read_image(path))
    for dt in (np.uint8, np.uint16, np.int32):
        arr = _stack(dt, 4, 33, 65, seed=2)
        path = str(tmp_path / f"w_{np.dtype(dt).name}.tif")
        tiff.write_stack(path, arr)
        plan = tiff.scan(path)
        assert plan is not None and all(len(p.strip_offsets) == 1 for p in plan.pages)
        _same(tiff.read_stack(path, "cpu"), tiff.read_image(path))


def _tiled_tiff() -> bytes:
    """One 16 x 16 uint8 page stored as one 16 x 16 tile, uncompressed."""
    data = bytes(range(256))
    tags = ((256, 4, 16), (257, 4, 16), (258, 3, 8), (259, 3, 1), (262, 3, 1), (277, 3, 1), (322, 4, 16), (323, 4, 16),
            (324, 4, 8), (325, 4, 256))
    ifd = 8 + len(data)
    out = struct.pack("<2sHI", b"II", 42, ifd) + data + struct.pack("<H", len(tags))
    for tag, typ, val in tags:
        out += struct.pack("<HHII", tag, typ, 1, val)
    return out + struct.pack("<I", 0)


def test_scan_refuses_what_the_device_path_does_not_cover(tmp_path):
    arr = _stack(np.uint8, 2, 40, 31)
    lzw = str(tmp_path / "lzw.tif")
    _pil_save(lzw, arr, compression="tiff_lzw")
    assert tiff.scan(lzw) is None

    good = str(tmp_path / "good.tif")
    _pil_save(good, arr, compression="tiff_adobe_deflate")
    assert tiff.scan(good) is not None
    big = str(tmp_path / "big_endian.tif")
    with open(big, "wb") as f:
        f.write(b"MM\0*" + open(good, "rb").read()[4:])
    assert tiff.scan(big) is None
    bigtiff = str(tmp_path / "bigtiff.tif")
    with open(bigtiff, "wb") as f:
        f.write(b"II+\0" + open(good, "rb").read()[4:])
    assert tiff.scan(bigtiff) is None

    tiled = str(tmp_path / "tiled.tif")
    with open(tiled, "wb") as f:
        f.write(_tiled_tiff())
    assert tiff.scan(tiled) is None

    from PIL import Image
    mixed = str(tmp_path / "mixed.tif")
    pages = [Image.fromarray(arr[0]), Image.fromarray(arr[1][:20])]
    pages[0].save(mixed, save_all=True, append_images=pages[1:], compression="tiff_adobe_deflate")
    assert tiff.scan(mixed) is None

    flt = str(tmp_path / "float.tif")
    _pil_save(flt, arr.astype(np.float32), compression="tiff_adobe_deflate")
    assert tiff.scan(flt) is None
    npy = str(tmp_path / "a.npy")
    np.save(npy, arr)
    assert tiff.scan(npy) is None
    assert tiff.scan(str(tmp_path / "absent.tif")) is None

    # the fallbacks read_image can read give read_image's array
    for path in (lzw, flt, npy, tiled):
        _same(tiff.read_stack(path, "cpu"), tiff.read_image(path))


def test_read_stack_names_the_file_of_a_damaged_strip(tmp_path):
    arr = _stack(np.uint16, 2, 40, 31)
    path = str(tmp_path / "a.tif")
    tiff.write_stack(path, arr)
    plan = tiff.scan(path)
    with open(path, "r+b") as f:
        f.seek(plan.pages[1].strip_offsets[0] + 4)
        f.write(b"\xff\xff\xff\xff")
    with pytest.raises(ValueError, match="a.tif"):
        tiff.read_stack(path, "cpu")


def test_validate_load_mask_on_a_device_equals_the_host_reader(tmp_path):
    from skoots_amd.validate.__main__ import load_mask
    for dt in (np.uint8, np.uint16, np.int32):
        arr = _stack(dt, 5, 20, 31, seed=3)
        path = str(tmp_path / f"m_{np.dtype(dt).name}.tif")
        tiff.write_stack(path, arr)
        host, dev = load_mask(path), load_mask(path, "cpu")
        assert dev.dtype == torch.int32 and dev.is_contiguous() and torch.equal(host, dev)


@pytest.mark.parametrize("orientation", [2, 6])
@pytest.mark.parametrize("comp", ["tiff_adobe_deflate", "raw"])
def test_orientation_is_left_to_read_image(tmp_path, orientation, comp):
    """Pillow applies the Orientation tag when it loads a page (mirrors for 2, rotates for 6): no plan, and read_stack
    gives read_image's array, shape included."""
    arr = _stack(np.uint8, 2, 20, 31, seed=6)
    plain, path = str(tmp_path / "plain.tif"), str(tmp_path / "oriented.tif")
    _pil_save(plain, arr, compression=comp, tiffinfo={274: 1})
    _pil_save(path, arr, compression=comp, tiffinfo={274: orientation})
    assert tiff.scan(plain) is not None
    assert tiff.scan(path) is None
    ref = tiff.read_image(path)
    _same(tiff.read_stack(path, "cpu"), ref)
    _same(tiff.read_stack(plain, "cpu"), arr)
