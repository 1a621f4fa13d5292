"""The HIP deflate encoder (skoots_amd/csrc/deflate.hip) and the writers on top of it, on the device.  The check of
every stream is the stdlib's inflater: it must give the input back, end exactly at the stream's last byte (so header,
block structure and Adler-32 are right), and the stream must be within sk_deflate_bound."""
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(stream, raw):
    from skoots_amd.lib import deflate
    assert stream[:2] == b"\x78\x01"
    d = zlib.decompressobj()
    out = d.decompress(stream)
    assert out == raw and d.eof and d.unused_data == b"", (len(raw), len(stream))
    assert len(stream) <= deflate.bound(len(raw)), (len(raw), len(stream))


def _encode(rows, elem_bytes=1, skip_zero=False):
    """rows: list of equal-length bytes objects -> list of streams from one call."""
    from skoots_amd.lib import deflate
    n = len(rows)
    length = len(rows[0]) if n else 0
    arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, length) if length else np.zeros((n, 0), np.uint8)
    return deflate.deflate_streams(torch.from_numpy(arr.copy()).to(DEV), elem_bytes=elem_bytes, skip_zero=skip_zero)


def _runs(dtype):
    """Runs of every length 1..300 of alternating values."""
    vals = (np.arange(300) * 2654435761 % np.iinfo(dtype).max).astype(dtype)
    return np.repeat(vals, np.arange(1, 301)).tobytes()


LENGTHS = (0, 1, 2, 3, 257, 258, 259, 65535, 65536, 65537, 8 << 20)


@pytest.mark.parametrize("length", LENGTHS)
def test_edge_lengths(length):
    rng = np.random.default_rng(length)
    last = bytearray(length)
    if length:
        last[-1] = 9
    rows = [bytes(length), b"\xff" * length, rng.integers(0, 256, length, dtype=np.uint8).tobytes(), bytes(last),
            (b"abc" * (length // 3 + 1))[:length], (b"\x00\x01\x02\x03\x04" * (length // 5 + 1))[:length]]
    together = _encode(rows)
    assert len(together) == len(rows)
    for raw, s in zip(rows, together):
        _check(s, raw)
    for e in (1, 2, 4):   # each as its own stream; the distance hint changes the bytes, never the content
        for raw, s in zip(rows, together):
            alone = _encode([raw], elem_bytes=e)[0]
            _check(alone, raw)
            if e == 1:
                assert alone == s, "a stream's bytes must not depend on the batch it is in"
    if length == 0:
        assert all(len(s) == 8 for s in together)


@pytest.mark.parametrize("dtype, e", [(np.uint8, 1), (np.uint16, 2), (np.int32, 4)])
def test_runs_of_every_length(dtype, e):
    raw = _runs(dtype)
    for hint in (e, 1):
        s = _encode([raw], elem_bytes=hint)[0]
        _check(s, raw)
    assert len(_encode([raw], elem_bytes=e)[0]) < len(raw) // 4   # runs are found at the element's distance


def test_far_repeats_and_sparse_streams():
    rng = np.random.default_rng(7)
    block = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    raw = block * 3   # the repeat lies beyond 32768: it must not be coded as a match
    _check(_encode([raw])[0], raw)
    last = bytearray(100000)
    last[-1] = 1
    s = _encode([bytes(last)], skip_zero=True)[0]
    assert s is not None
    _check(s, bytes(last))
    for period in (3, 5):
        raw = bytes(rng.integers(0, 256, period, dtype=np.uint8)) * 20000
        for e in (1, 2, 4):
            _check(_encode([raw], elem_bytes=e)[0], raw)


def test_skip_zero_leaves_zero_rows_out():
    rows = [bytes(70000), b"\x00" * 69999 + b"\x01", bytes(70000), b"\x02" + bytes(69999)]
    got = _encode(rows, skip_zero=True)
    assert [g is None for g in got] == [True, False, True, False]
    _check(got[1], rows[1])
    _check(got[3], rows[3])
    kept = _encode(rows, skip_zero=False)
    for raw, s in zip(rows, kept):
        _check(s, raw)
    assert kept[1] == got[1] and kept[3] == got[3]


def test_argument_checks():
    from skoots_amd import _ffi
    from skoots_amd.lib import deflate
    t = torch.zeros((2, 64), dtype=torch.uint8, device=DEV)
    offs = torch.empty(3, dtype=torch.int64, device=DEV)
    dst = torch.empty(2 * deflate.bound(64), dtype=torch.uint8, device=DEV)
    ws = torch.empty(16, dtype=torch.uint8, device=DEV)   # too small
    with pytest.raises(ValueError, match="workspace"):
        _ffi.check(_ffi.lib.sk_deflate_streams(_ffi.ptr(t), 2, 64, 1, _ffi.ptr(dst), _ffi.ptr(offs), None, _ffi.ptr(ws),
                                               16, _ffi.stream_ptr(DEV)))


def _blob_outputs():
    """The three arrays eval() would write for the 512 x 512 x 64 blob field: planar vectors and skeleton as the
    gate of the pipeline leaves them (oracle.pipeline.gate_dilate), the label mask as (Z, X, Y) uint16 pages."""
    import scipy.ndimage as ndi

    from oracle import pipeline as O
    from tests.workload import blob_field
    out, _ = blob_field((512, 512, 64), seed=3, n_blobs=300)
    vec, skel = O.gate_dilate(out.unsqueeze(0))
    vectors = vec[0].half().contiguous()
    skeleton = skel[0].gt(O.SKEL_THR).to(torch.uint8).contiguous()
    mask = ndi.label(out[4].float().numpy() > 0.8)[0].astype(np.uint16).transpose(2, 0, 1)
    return vectors, skeleton, torch.from_numpy(np.ascontiguousarray(mask))


def _chunk_rows(t):
    """(C, 512, 512, 64) tensor -> list of the (1, 256, 256, 64) chunks' bytes, the stores' default chunking."""
    rows = []
    for c in range(t.shape[0]):
        for i in range(2):
            for j in range(2):
                rows.append(t[c, i * 256:(i + 1) * 256, j * 256:(j + 1) * 256].contiguous().numpy().tobytes())
    return rows


def test_blob_field_outputs_round_trip_and_size():
    """Size condition of the encoder: at most 2x what zlib level 1 writes for the same chunks / pages."""
    vectors, skeleton, mask = _blob_outputs()
    ratios = {}
    for name, rows, e in (("vectors", _chunk_rows(vectors), 2), ("skeleton", _chunk_rows(skeleton), 1),
                          ("mask", [p.numpy().tobytes() for p in mask], 2)):
        ours = host = 0
        step = 4 if name == "vectors" else len(rows)   # 32 MiB of chunks per call
        for lo in range(0, len(rows), step):
            part = rows[lo:lo + step]
            for raw, s in zip(part, _encode(part, elem_bytes=e)):
                _check(s, raw)
                ours += len(s)
                host += len(zlib.compress(raw, 1))
        ratios[name] = ours / host
        print(f"{name}: device {ours} bytes, zlib level 1 {host} bytes, ratio {ours / host:.3f}")
    assert all(r <= 2.0 for r in ratios.values()), ratios


def test_deterministic_across_calls_and_batching():
    rng = np.random.default_rng(11)
    rows = []
    for k in range(6):
        a = rng.integers(0, 3, 200000, dtype=np.uint8) * (rng.random(200000) < 0.2)
        rows.append(a.astype(np.uint8).tobytes())
    for e in (1, 2):
        first, second = _encode(rows, elem_bytes=e), _encode(rows, elem_bytes=e)
        assert first == second
        assert [_encode([r], elem_bytes=e)[0] for r in rows] == first
        for raw, s in zip(rows, first):
            _check(s, raw)


def test_save_device_and_write_stack_on_device(tmp_path):
    from PIL import Image

    from skoots_amd.lib import tiff, zarr_store
    rng = np.random.default_rng(5)
    vec = np.zeros((3, 300, 270, 70), np.float16)
    vec[:, 40:200, 30:90, 5:60] = rng.standard_normal((3, 160, 60, 55)).astype(np.float16)
    vec[1] = 0   # a whole channel of fill value: its chunks are left out
    skel = (rng.random((1, 130, 257, 64)) < 0.01).astype(np.uint8)
    for k, (arr, chunks) in enumerate(((vec, None), (skel, None), (skel, (1, 64, 64, 64)))):
        a, b = str(tmp_path / f"a{k}.zarr"), str(tmp_path / f"b{k}.zarr")
        zarr_store.save(a, arr, chunks)
        zarr_store.save_device(b, torch.from_numpy(arr).to(DEV), chunks, budget_bytes=40 << 20)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b))
        assert open(os.path.join(a, ".zarray")).read() == open(os.path.join(b, ".zarray")).read()
        assert np.array_equal(zarr_store.load(b), arr)
    for dtype in (np.uint8, np.uint16, np.int32):
        pages = rng.integers(0, 200, (5, 61, 47)).astype(dtype) * (rng.random((5, 61, 47)) < 0.3)
        pages = pages.astype(dtype)
        path = str(tmp_path / f"p_{np.dtype(dtype).name}.tif")
        tiff.write_stack(path, torch.from_numpy(pages).to(DEV))
        with Image.open(path) as im:
            assert im.n_frames == 5
            got = []
            for z in range(5):
                im.seek(z)
                got.append(np.array(im))
        assert np.array_equal(np.stack(got), pages)
        back = tiff.read_image(path)
        assert back.dtype == dtype and np.array_equal(back, pages)
    lab = torch.from_numpy(rng.integers(0, 70000, (3, 20, 30)).astype(np.int32)).to(DEV)
    tiff.write_label_stack(str(tmp_path / "wide.tif"), lab)
    assert np.array_equal(tiff.read_image(str(tmp_path / "wide.tif")), lab.cpu().numpy())
    tiff.write_label_stack(str(tmp_path / "narrow.tif"), lab % 65536)
    narrow = tiff.read_image(str(tmp_path / "narrow.tif"))
    assert narrow.dtype == np.uint16 and np.array_equal(narrow, (lab % 65536).cpu().numpy())


def test_eval_writes_device_deflated_files(tmp_path):
    """The files eval() leaves on the small volume of test_hip_eval_file: every chunk file is a stream of the device
    encoder that inflates to the chunk load() returns, every TIFF page is one Adobe-deflate strip."""
    import json

    from PIL import Image

    from oracle import unet_spec
    from skoots_amd.lib import zarr_store
    from skoots_amd.lib.eval import eval as sk_eval
    ref = unet_spec.build()
    with torch.no_grad():
        ref.heads.weight[3:5].mul_(0.05)
        ref.heads.weight[0:3].mul_(1e-5)
        ref.heads.bias[0:3] = 1e-5
        ref.heads.bias[3] = 2.2
        ref.heads.bias[4] = 3.0
    Z, X, Y = 24, 132, 128
    img = torch.randint(0, 256, (Z, X, Y), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).numpy()
    ipath, cpath = str(tmp_path / "vol.npy"), str(tmp_path / "model.trch")
    np.save(ipath, img)
    cfg = {"SKOOTS": {"VECTOR_SCALING": (60, 60, 12)},
           "MODEL": {"DIMS": [32, 64, 128, 64, 32], "DEPTHS": [2, 2, 2, 2, 2], "IN_CHANNELS": 1}}
    torch.save({"cfg": cfg, "model_state_dict": ref.state_dict(), "dataset_mean": 127.0, "dataset_std": 70.0}, cpath)
    sk_eval(ipath, cpath)
    base = str(tmp_path / "vol")
    for suffix in ("_skoots_skeleton.zarr", "_skoots_vectors.zarr"):
        path = base + suffix
        arr = zarr_store.load(path)
        meta = json.load(open(os.path.join(path, ".zarray")))
        assert meta["compressor"] == {"id": "zlib", "level": 1}
        chunks = meta["chunks"]
        files = [f for f in os.listdir(path) if f != ".zarray"]
        assert files
        for fn in files:
            idx = [int(v) for v in fn.split(".")]
            block = np.zeros(chunks, arr.dtype)
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, arr.shape))
            part = arr[sl]
            block[tuple(slice(0, n) for n in part.shape)] = part
            _check(open(os.path.join(path, fn), "rb").read(), block.tobytes())
    with Image.open(base + "_instance_mask.tif") as im:
        assert im.n_frames == Z
        for z in range(Z):
            im.seek(z)
            assert im.tag_v2[259] == 8 and len(im.tag_v2[273]) == 1 and len(im.tag_v2[279]) == 1
