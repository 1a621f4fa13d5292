"""The HIP inflate decoder (skoots_amd/csrc/inflate.hip) and the readers on top of it, on the device.  The oracle is the
stdlib's zlib: a stream's status is 0 exactly when zlib inflates it without error, to its end and to the expected size,
and then the bytes are zlib's.  Every launch goes through ``_run``, which lays guard bytes before and after every
stream's dst range and checks that they are intact, whatever the stream was.

The malformed streams of this file (tests/inflate_corpus.py) ran on the CPU build of the same kernel text under
AddressSanitizer and UBSan (tools/inflate_host_check.py) before they ran here; DESIGN.md section 16 has the result."""
import os
import shutil
import zlib

import numpy as np
import pytest
import torch

from tests import inflate_corpus as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL = 0xA5


def _run(cases, leads=None):
    """One launch for ``cases`` (all of one wrapper).  Between the streams, in src and in dst, lie gap streams: their
    src is `lead` bytes of FF (no header, and block type 3 when read raw: refused before anything is written), their
    dst range is the guard.  Returns (status per case, output bytes per case)."""
    from skoots_amd import _ffi
    wrapper = cases[0].wrapper
    assert all(c.wrapper == wrapper for c in cases)
    n = len(cases)
    src, src_off, dst_off = bytearray(), [0], [0]
    for k, c in enumerate(cases):
        lead = 0 if leads is None else leads[k]
        pad = (lead - len(src)) % 8 if leads is not None else 0
        src += b"\xff" * pad                     # the gap stream's bytes
        src_off.append(len(src))
        dst_off.append(dst_off[-1] + GUARD)
        src += c.stream
        src_off.append(len(src))
        dst_off.append(dst_off[-1] + c.size)
        if leads is not None:
            assert src_off[-2] % 8 == lead
    src_off.append(len(src))                     # the last gap: empty
    dst_off.append(dst_off[-1] + GUARD)
    ns = 2 * n + 1
    s = torch.frombuffer(src or bytearray(1), dtype=torch.uint8).to(DEV)
    assert s.data_ptr() % 8 == 0
    offs = torch.tensor([src_off, dst_off], dtype=torch.int64, device=DEV)
    dst = torch.full((dst_off[-1],), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((ns,), -1, dtype=torch.int32, device=DEV)
    _ffi.check(_ffi.lib.sk_inflate_streams(_ffi.ptr(s), _ffi.ptr(offs[0]), ns, _ffi.ptr(dst), _ffi.ptr(offs[1]), wrapper,
                                           _ffi.ptr(status), _ffi.stream_ptr(torch.device(DEV))))
    st = status.cpu().tolist()
    out = dst.cpu().numpy()
    for g in range(0, ns, 2):
        assert st[g] != 0, "a gap stream was accepted"
        assert (out[dst_off[g]:dst_off[g + 1]] == FILL).all(), f"guard bytes around stream {g // 2} were written"
    return [st[2 * k + 1] for k in range(n)], [out[dst_off[2 * k + 1]:dst_off[2 * k + 2]].tobytes() for k in range(n)]


def _check(cases, leads=None):
    """Status and bytes of every case against what the case expects (the payload, or refusal); guards by ``_run``."""
    status, data = _run(cases, leads)
    for c, st, d in zip(cases, status, data):
        if c.expect is None:
            assert st != 0, f"{c.name}: accepted, zlib refuses it"
            if c.code:
                assert st == c.code, f"{c.name}: status {st}, wanted {c.code}"
        else:
            assert st == 0, f"{c.name}: status {st}, zlib accepts it"
            assert d == c.expect, f"{c.name}: wrong bytes"
    return status, data


def _check_batch_and_alone(cases):
    status, data = _check(cases)
    for c, st, d in zip(cases, status, data):
        st1, d1 = _check([c])
        assert (st1[0], d1[0]) == (st, d), f"{c.name}: the output depends on the batch"


# ------------------------------------------------------------------------------------------ payloads x encoders
@pytest.mark.parametrize("encoder", list(C.ENCODERS))
def test_payloads(encoder):
    _check_batch_and_alone(C.encoded(encoder))


def test_chunk_of_8_mib():
    chunk = C.chunk_payload()
    assert len(chunk) == 8 << 20
    _check_batch_and_alone([C.Case("level6:chunk", zlib.compress(chunk, 6), 1, len(chunk), chunk),
                            C.Case("level1:chunk", zlib.compress(chunk, 1), 1, len(chunk), chunk)])


@pytest.mark.parametrize("elem_bytes", [1, 2, 4])
def test_round_trip_of_the_device_encoder(elem_bytes):
    from skoots_amd.lib import deflate
    by_len = {}
    for name, data in C.payloads():
        by_len.setdefault(len(data), []).append((name, data))
    cases = []
    for length, group in by_len.items():
        arr = np.frombuffer(b"".join(d for _, d in group), dtype=np.uint8).reshape(len(group), length) if length else \
            np.zeros((len(group), 0), np.uint8)
        streams = deflate.deflate_streams(torch.from_numpy(arr.copy()).to(DEV), elem_bytes=elem_bytes)
        cases += [C.Case(f"own{elem_bytes}:{name}", s, 1, length, d) for (name, d), s in zip(group, streams)]
    _check_batch_and_alone(cases)
    # and through the public function: one call, (flat, offsets)
    flat, offs = deflate.inflate_streams([c.stream for c in cases], [c.size for c in cases], DEV)
    host = flat.cpu().numpy()
    for c, a, b in zip(cases, offs[:-1], offs[1:]):
        assert host[a:b].tobytes() == c.expect, c.name


# ------------------------------------------------------------------------------------------ hand-assembled streams
def test_hand_assembled_streams():
    cases = C.hand_assembled()
    assert {c.name for c in cases} >= {"dist32768_len258", "dist1_len258", "all_length_and_distance_codes",
                                       "repeat16_across_boundary", "repeat17_across_boundary", "repeat18_across_boundary",
                                       "codes_of_15_bits", "single_distance_code", "literals_only"}
    _check_batch_and_alone(cases)


@pytest.mark.parametrize("lead", range(1, 8))
def test_unaligned_stream_starts(lead):
    cases = C.hand_assembled() + [c._replace(wrapper=0, stream=c.stream[2:-4]) for c in C.good_neighbours()]
    _check(cases, leads=[lead] * len(cases))
    _check(cases, leads=[(lead + k) % 8 for k in range(len(cases))])


# ------------------------------------------------------------------------------------------ malformed input
def test_every_truncation_is_refused():
    cases = C.truncations()
    assert len(cases) == 300
    status, _ = _check(cases + C.good_neighbours())
    assert all(st != 0 for st in status[:300])


def test_every_single_bit_flip_follows_zlib():
    cases = C.bit_flips()
    assert len(cases) == 2400
    accepted = sum(c.expect is not None for c in cases)
    status, _ = _check(cases + C.good_neighbours())
    assert sum(st == 0 for st in status[:2400]) == accepted


def test_named_errors_report_their_codes():
    cases = C.named_errors()
    names = {c.name: c.code for c in cases}
    assert names["reserved_block_type"] == C.E_BLOCK_TYPE and names["len_nlen"] == C.E_STORED
    assert names["oversubscribed_set"] == names["incomplete_set"] == C.E_CODES
    assert names["symbol_286"] == names["distance_code_30"] == C.E_SYMBOL
    assert names["distance_before_output"] == C.E_DISTANCE
    assert names["expected_one_less"] == C.E_LONG and names["expected_one_more"] == C.E_SHORT
    assert names["adler_off_by_one"] == C.E_ADLER and names["fdict"] == names["bad_cmf"] == C.E_HEADER
    assert names["input_ends_in_trailer"] == C.E_INPUT
    assert len({C.E_HEADER, C.E_BLOCK_TYPE, C.E_STORED, C.E_CODES, C.E_SYMBOL, C.E_DISTANCE, C.E_INPUT, C.E_LONG,
                C.E_SHORT, C.E_ADLER}) == 10
    _check_batch_and_alone(cases + C.good_neighbours())


def test_inflate_streams_raises_with_index_and_reason():
    from skoots_amd.lib import deflate
    good = zlib.compress(b"abc" * 50)
    bad = {c.name: c for c in C.named_errors()}["adler_off_by_one"]
    with pytest.raises(ValueError, match=r"stream 1 of 3 does not inflate: Adler-32 mismatch"):
        deflate.inflate_streams([good, bad.stream, good], [150, bad.size, 150], DEV)
    rows = deflate.inflate_streams([good, good], 150, DEV)
    assert tuple(rows.shape) == (2, 150) and rows.cpu().numpy().tobytes() == b"abc" * 100


def test_deterministic():
    cases = C.encoded("level6", big=False) + C.named_errors()[:-2]
    first, second = _run(cases), _run(cases)
    assert first[0] == second[0]
    for c, a, b in zip(cases, first[1], second[1]):
        if c.expect is not None:
            assert a == b


# ------------------------------------------------------------------------------------------ predictor
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("spp", [1, 3])
def test_undo_predictor(dtype, spp):
    from skoots_amd import _ffi
    rng = np.random.default_rng(spp)
    for width in (1, 63, 64, 65, 301):
        rows = 7
        info = np.iinfo(dtype)
        diff = rng.integers(info.min, info.max, (rows, width, spp), endpoint=True).astype(dtype)
        want = np.cumsum(diff, axis=1, dtype=dtype)          # wraps modulo 2^bits
        t = torch.from_numpy(diff.view(np.int16) if dtype == np.uint16 else diff).to(DEV)
        _ffi.check(_ffi.lib.sk_tiff_undo_predictor(_ffi.ptr(t), rows, width, spp, diff.dtype.itemsize,
                                                   _ffi.stream_ptr(torch.device(DEV))))
        got = t.cpu().numpy().view(dtype)
        assert np.array_equal(got, want), (width, spp)


# ------------------------------------------------------------------------------------------ files
def test_load_device_equals_load(tmp_path):
    from skoots_amd.lib import zarr_store
    rng = np.random.default_rng(5)
    vec = np.zeros((3, 300, 270, 70), np.float16)
    vec[:, 40:200, 30:90, 5:60] = rng.standard_normal((3, 160, 60, 55)).astype(np.float16)
    vec[1] = 0   # a whole channel of fill value: its chunks are missing
    skel = (rng.random((1, 130, 257, 64)) < 0.01).astype(np.uint8)
    lab = rng.integers(0, 1 << 20, (37, 53)).astype(np.int32)
    for k, (arr, chunks) in enumerate(((vec, None), (skel, None), (skel, (1, 64, 64, 64)), (lab, (16, 16)))):
        a, b, r = (str(tmp_path / f"{n}{k}.zarr") for n in "abr")
        zarr_store.save(a, arr, chunks)
        zarr_store.save_device(b, torch.from_numpy(arr).to(DEV), chunks)
        zarr_store.save(r, arr, chunks, compressor=None)
        for path in (a, b, r):
            want = zarr_store.load(path)
            for budget in (zarr_store.LOAD_DEVICE_BUDGET, 1):
                got = zarr_store.load_device(path, DEV, budget_bytes=budget)
                assert got.is_cuda and tuple(got.shape) == want.shape
                assert got.cpu().numpy().dtype == want.dtype and got.cpu().numpy().tobytes() == want.tobytes()


def _pil_save(path, arr, **kw):
    from PIL import Image
    pages = [Image.fromarray(p) for p in arr]
    pages[0].save(path, save_all=True, append_images=pages[1:], **kw)


def test_read_stack_equals_read_image(tmp_path):
    from skoots_amd.lib import tiff
    rng = np.random.default_rng(9)
    paths = []
    for dtype in (np.uint8, np.uint16, np.int32):
        pages = (rng.integers(0, 200, (5, 300, 301)) * (rng.random((5, 300, 301)) < 0.3)).astype(dtype)
        name = np.dtype(dtype).name
        paths.append(str(tmp_path / f"ws_{name}.tif"))
        tiff.write_stack(paths[-1], torch.from_numpy(pages).to(DEV))
        for tag, kw in (("deflate", {"compression": "tiff_adobe_deflate"}),
                        ("pred2", {"compression": "tiff_adobe_deflate", "tiffinfo": {317: 2}}), ("raw", {"compression": "raw"})):
            paths.append(str(tmp_path / f"pil_{tag}_{name}.tif"))
            _pil_save(paths[-1], pages, **kw)
            assert tiff.scan(paths[-1]) is not None
    rgb = rng.integers(0, 255, (2, 40, 31, 3)).astype(np.uint8)
    paths.append(str(tmp_path / "rgb_pred2.tif"))
    _pil_save(paths[-1], rgb, compression="tiff_adobe_deflate", tiffinfo={317: 2})
    assert tiff.scan(paths[-1]) is not None
    paths.append(str(tmp_path / "lzw.tif"))        # a fallback
    _pil_save(paths[-1], rgb[..., 0], compression="tiff_lzw")
    assert tiff.scan(paths[-1]) is None
    for path in paths:
        want = tiff.read_image(path)
        got = tiff.read_stack(path, DEV)
        assert got.is_cuda and tuple(got.shape) == want.shape, path
        host = got.cpu().numpy()
        assert host.dtype == want.dtype and host.tobytes() == want.tobytes(), path


def test_eval_from_cached_stores_gives_the_same_mask(tmp_path, monkeypatch):
    """eval() on a blob-field volume, then again with used_cached_data=True (the stores are read by load_device, the image
    by read_stack), then once more through the host readers: three identical instance masks."""
    from oracle import unet_spec
    from skoots_amd.lib import eval as E
    from skoots_amd.lib import tiff
    from tests.workload import blob_field
    shape = (140, 132, 34)
    out_vol, k = blob_field(shape, seed=3, n_blobs=12, rmax=(8, 8, 3))
    out_dev = out_vol.to(DEV)

    def inject(_, origin, eff):
        x, y, z = origin
        return out_dev[:, x:x + eff[0], y:y + eff[1], z:z + eff[2]].contiguous()

    real = E.eval_volume
    monkeypatch.setattr(E, "eval_volume", lambda img, model, scale, mean, std: real(img, model, scale, mean=mean, std=std,
                                                                                    inject=inject))
    img = torch.randint(0, 256, (shape[2], shape[0], shape[1]), generator=torch.Generator().manual_seed(0),
                        dtype=torch.uint8).numpy()
    ipath, cpath = str(tmp_path / "vol.tif"), str(tmp_path / "model.trch")
    _pil_save(ipath, img, compression="tiff_adobe_deflate")
    assert tiff.scan(ipath) is not None
    cfg = {"SKOOTS": {"VECTOR_SCALING": (60, 60, 12)},
           "MODEL": {"DIMS": [32, 64, 128, 64, 32], "DEPTHS": [2, 2, 2, 2, 2], "IN_CHANNELS": 1}}
    torch.save({"cfg": cfg, "model_state_dict": unet_spec.build().state_dict(), "dataset_mean": 127.0,
                "dataset_std": 70.0}, cpath)
    mask = str(tmp_path / "vol_instance_mask.tif")
    E.eval(ipath, cpath, read_on_device=True)
    first = tiff.read_image(mask)
    assert first.max() == k
    os.remove(mask)
    E.eval(ipath, cpath, used_cached_data=True, read_on_device=True)
    second = tiff.read_image(mask)
    os.remove(mask)
    E.eval(ipath, cpath, used_cached_data=True, read_on_device=False)
    third = tiff.read_image(mask)
    assert first.dtype == second.dtype == third.dtype
    assert np.array_equal(first, second) and np.array_equal(first, third)
    # and the mask eval() wrote, read on the device
    got = tiff.read_stack(mask, DEV)
    assert np.array_equal(got.cpu().numpy().view(first.dtype), first)


def test_validate_command_on_device_read_masks(golden, tmp_path, monkeypatch):
    """The two CSV files of the validate command with the masks read on the device and on the host: the same text."""
    from skoots_amd.lib import tiff
    from skoots_amd.validate import __main__ as V
    d = golden("validate_cldice.npz")
    for name in ("gt", "pred"):
        tiff.write_label_stack(str(tmp_path / f"{name}.tif"),
                               torch.from_numpy(np.ascontiguousarray(d[f"csv_{name}_zxy"]).astype(np.int32)).to(DEV))
        assert tiff.scan(str(tmp_path / f"{name}.tif")) is not None
    monkeypatch.chdir(tmp_path)
    texts = []
    for on_device in (True, False):
        monkeypatch.setattr(V, "READ_ON_DEVICE", on_device)
        acc_path, iou_path = V.main(["--ground_truth", "gt.tif", "--predicted", "pred.tif"])
        texts.append((open(acc_path).read(), open(iou_path).read()))
        shutil.move(acc_path, f"acc_{on_device}.csv")
    assert texts[0] == texts[1]
    assert texts[0] == (str(d["csv_accuracy"]), str(d["csv_iou"]))
    host, dev = V.load_mask("gt.tif"), V.load_mask("gt.tif", DEV)
    assert dev.is_cuda and dev.dtype == torch.int32 and torch.equal(dev.cpu(), host)
