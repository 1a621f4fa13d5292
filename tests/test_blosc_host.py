"""The Blosc reader without a GPU: ``parse_header`` and ``plan`` on frames a real c-blosc wrote (tests/golden/blosc.npz,
made by tests/golden/make_blosc_golden.py), the host build of the decoder (``sk_blosc_decode_host``) against their
expected bytes and against the pure-Python reference of tests/blosc_corpus.py, and the two store readers on store
directories assembled from the frames, with the ``.zarray`` the reference's zarr writes."""
import json
import os

import numpy as np
import pytest

from tests import blosc_corpus as C

good_frames, write_store = C.good_frames, C.write_store


def test_golden_file_is_small():
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "blosc.npz")) < 400 << 10


def test_abi():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 13


def test_parse_header(golden):
    from skoots_amd.lib import blosc
    d = golden("blosc.npz")
    h = blosc.parse_header(d["a_frame_0.0.0.0"].tobytes()[:16])
    assert (h.version, h.typesize, h.nbytes, h.blocksize, h.nblocks) == (2, 2, 327680, 262144, 2)
    assert h.cbytes == len(d["a_frame_0.0.0.0"]) and h.shuffle and not h.memcpyed and not h.bitshuffle and h.codec == "lz4"
    h = blosc.parse_header(d["b_frame_0.0.0.0"].tobytes()[:16])
    assert (h.typesize, h.nbytes, h.blocksize, h.nblocks, h.shuffle) == (1, 163840, 131072, 2, True)
    h = blosc.parse_header(d["c_frame_memcpy_15_bytes"].tobytes())
    assert h.memcpyed and h.nbytes == 15 and h.cbytes == 31 and h.nblocks == 0
    assert blosc.parse_header(d["c_frame_shuffle0"].tobytes()).shuffle is False
    assert blosc.parse_header(d["c_frame_lz4hc9"].tobytes()).codec == "lz4"
    assert [blosc.parse_header(d[f"d_frame_{n}"].tobytes()).codec for n in ("blosclz", "zlib", "zstd")] == ["blosclz", "zlib", "zstd"]
    assert blosc.parse_header(d["d_frame_bitshuffle"].tobytes()).bitshuffle
    with pytest.raises(ValueError):
        blosc.parse_header(b"\x02\x01\x21")
    # the store-level refusals, one per condition
    f = d["b_frame_0.1.0.0"].tobytes()
    assert blosc.refusal(f[:16], len(f), 163840) is None
    assert "shorter" in blosc.refusal(f[:10], 10, 163840)
    assert "version" in blosc.refusal(b"\x03" + f[1:16], len(f), 163840)
    assert "file has" in blosc.refusal(f[:16], len(f) + 1, 163840)
    assert "a chunk has" in blosc.refusal(f[:16], len(f), 163841)
    assert "blocksize 0" in blosc.refusal(f[:8] + bytes(4) + f[12:16], len(f), 163840)
    assert "'zstd'" in blosc.refusal(d["d_frame_zstd"].tobytes()[:16], len(d["d_frame_zstd"]), 2000)
    assert "bitshuffle" in blosc.refusal(d["d_frame_bitshuffle"].tobytes()[:16], len(d["d_frame_bitshuffle"]), 2000)


def test_plan_split_leftover_and_stored_rules(golden):
    from skoots_amd.lib import blosc
    d = golden("blosc.npz")
    # (a): block 0 is split in two byte planes, block 1 is the leftover: one stream; both are unshuffled afterwards
    f = d["a_frame_0.0.0.0"].tobytes()
    p = blosc.plan([f], 327680)
    assert p.streams[:, 2:4].tolist() == [[0, 131072], [131072, 131072], [262144, 65536]]
    assert p.n_direct == 0 and p.blocks.tolist() == [[0, 262144], [262144, 65536]] and p.typesize.tolist() == [2, 2]
    bstarts = np.frombuffer(f[16:24], "<i4")
    assert p.streams[0, 0] == bstarts[0] + 4 and p.streams[2, 0] == bstarts[1] + 4
    assert p.streams[1, 0] == p.streams[0, 0] + p.streams[0, 1] + 4          # a split follows the one before it
    assert (p.streams[:, 0] + p.streams[:, 1] <= len(f)).all() and (p.streams[:, 4] == C.KIND_LZ4).all()
    # (b): typesize 1: two blocks, no splits, nothing to unshuffle although the flag is set
    p = blosc.plan([d["b_frame_0.0.0.0"].tobytes()], 163840)
    assert p.streams[:, 2:4].tolist() == [[0, 131072], [131072, 32768]] and p.n_direct == 2 and len(p.blocks) == 0
    # two frames in one call: offsets are into the frames and the outputs laid back to back
    f0, f1 = d["b_frame_0.0.0.0"].tobytes(), d["b_frame_0.1.0.0"].tobytes()
    p = blosc.plan([f0, f1], 163840)
    assert p.frame.tolist() == [0, 0, 1, 1] and p.streams[2, 2] == 163840 and p.streams[2, 0] == len(f0) + 16 + 8 + 4
    # stored split: the incompressible low-byte plane is kept as it is, the zero high bytes are LZ4
    p = blosc.plan([d["c_frame_incompressible"].tobytes()], 60000)
    assert p.streams[:, 4].tolist() == [C.KIND_STORED, C.KIND_LZ4] and p.streams[0, 1] == 30000 == p.streams[0, 3]
    # memcpyed: one stored stream behind the header, no block table
    p = blosc.plan([d["c_frame_memcpy_clevel0"].tobytes()], 5000)
    assert p.streams.tolist() == [[16, 5000, 0, 5000, C.KIND_STORED]] and len(p.blocks) == 0
    # blocksize / typesize < 128: not split; typesize 4 and 8: that many splits; odd length: a 1-byte leftover block
    assert len(blosc.plan([d["c_frame_small200"].tobytes()], 200).streams) == 1
    assert len(blosc.plan([d["c_frame_typesize4"].tobytes()], 120000).streams) == 4
    assert len(blosc.plan([d["c_frame_typesize8"].tobytes()], 160000).streams) == 8
    p = blosc.plan([d["c_frame_odd_length"].tobytes()], 100001)
    assert p.streams[:, 3].tolist() == [50000, 50000, 1] and p.blocks.tolist() == [[0, 100000], [100000, 1]]
    p = blosc.plan([d["c_frame_many_blocks"].tobytes()], 400000)
    assert len(p.blocks) == 7 and len(p.streams) == 6 * 2 + 1
    assert len(blosc.plan([d["c_frame_shuffle0"].tobytes()], 180000).blocks) == 0
    for n in d["d_names"]:
        with pytest.raises(blosc.BloscError, match="status 7"):
            blosc.plan([d[f"d_frame_{n}"].tobytes()], int(d["d_bytes"]))
    # every offset is checked against the frame: a block start and a split prefix that point outside it
    f = bytearray(d["a_frame_0.0.0.0"].tobytes())
    for at, value in ((16, len(f) + 1), (20, -5), (int(bstarts[1]), len(f))):
        g = bytearray(f)
        g[at:at + 4] = int(value).to_bytes(4, "little", signed=True)
        with pytest.raises(blosc.BloscError, match="status 8") as e:
            blosc.plan([f, g], 327680)
        assert e.value.index == 1


def test_decode_host_on_the_golden_frames(golden):
    from skoots_amd.lib import blosc
    for name, frame, raw in good_frames(golden("blosc.npz")):
        got = blosc.decode_host([frame], len(raw))
        assert got.shape == (1, len(raw)) and got.tobytes() == raw, name


def test_corpus_through_the_host_entry_point():
    """Every LZ4 stream of the corpus as the one split of a frame: status and bytes of sk_blosc_decode_host against the
    pure-Python reference decoder."""
    import ctypes
    from skoots_amd import _ffi
    cases = [c for c in C.all_cases() if c.kind == C.KIND_LZ4]
    ran = accepted = 0
    status = ctypes.c_int32(0)
    for c in cases:
        want_status, want = C.decode(c.stream, c.size)
        assert want == c.expect and (want is not None or not c.code or c.code == want_status), c.name
        frame = C.frame_of(c.stream, c.size)
        if frame is None:
            continue
        out = np.full(c.size, 0xA5, np.uint8)
        _ffi.check(_ffi.lib.sk_blosc_decode_host(frame, len(frame), out.ctypes.data, c.size, ctypes.byref(status)))
        assert status.value == want_status, f"{c.name}: status {status.value}, the reference says {want_status}"
        if want is not None:
            assert out.tobytes() == want, c.name
            accepted += 1
        ran += 1
    assert ran > 4000 and accepted > 60
    # a shuffled frame around a hand-made stream: the transpose of the host decoder, with a tail byte
    raw = bytes(range(200)) + b"\x07"
    planes = np.frombuffer(raw[:200], np.uint8).reshape(50, 4).T.tobytes() + raw[200:]
    frame = C.frame_of(C.last(planes), len(raw), typesize=4, shuffle=True)
    out = np.zeros(len(raw), np.uint8)
    _ffi.check(_ffi.lib.sk_blosc_decode_host(frame, len(frame), out.ctypes.data, len(raw), ctypes.byref(status)))
    assert status.value == 0 and out.tobytes() == raw


def _same(t, arr):
    got = t.cpu().numpy()
    assert got.dtype == arr.dtype and got.shape == arr.shape and got.tobytes() == arr.tobytes()


def test_stores_the_reference_wrote_read_back(golden, tmp_path):
    """(a) and (b) as store directories with the reference's .zarray: both readers give the arrays; the all-zero chunk's
    file is absent.  Fails without the Blosc reader: such stores were refused by name."""
    from skoots_amd.lib import zarr_store
    d = golden("blosc.npz")
    assert "1.1.0.0" not in d["a_names"].tolist() and len(d["a_names"]) == 5
    for prefix in "ab":
        path = str(tmp_path / f"{prefix}.zarr")
        arr = write_store(path, d, prefix)
        got = zarr_store.load(path)
        assert got.dtype == arr.dtype and np.array_equal(got.view(np.uint8), arr.view(np.uint8))
        _same(zarr_store.load_device(path, "cpu"), arr)
        _same(zarr_store.load_device(path, "cpu", budget_bytes=1), arr)
        # {"id": "blosc"} alone: the frame carries everything
        bare = str(tmp_path / f"{prefix}_bare.zarr")
        write_store(bare, d, prefix, {"id": "blosc"})
        assert zarr_store.load(bare).tobytes() == arr.tobytes()
        _same(zarr_store.load_device(bare, "cpu"), arr)


def _both(path, exc):
    from skoots_amd.lib import zarr_store
    with pytest.raises(exc) as e_host:
        zarr_store.load(path)
    with pytest.raises(exc) as e_dev:
        zarr_store.load_device(path, "cpu")
    assert str(e_host.value) == str(e_dev.value)
    return str(e_host.value)


def test_stores_with_other_inner_codecs_are_refused_by_name(golden, tmp_path):
    d = golden("blosc.npz")
    for n in d["d_names"]:
        path = str(tmp_path / f"{n}.zarr")
        os.makedirs(path)
        json.dump({"zarr_format": 2, "shape": [2000], "chunks": [2000], "dtype": "|u1", "compressor": {"id": "blosc"},
                   "fill_value": 0, "order": "C", "filters": None}, open(os.path.join(path, ".zarray"), "w"))
        open(os.path.join(path, "0"), "wb").write(d[f"d_frame_{n}"].tobytes())
        text = _both(path, RuntimeError)
        assert "'blosc'" in text and os.path.join(path, "0") in text
        assert (f"'{n}'" in text) if n != "bitshuffle" else ("bitshuffle" in text)
    # one bad file refuses the whole store before anything is decoded: a good store with one chunk of another size
    path = str(tmp_path / "mixed.zarr")
    write_store(path, d, "b")
    open(os.path.join(path, "0.1.0.0"), "wb").write(d["c_frame_small200"].tobytes())
    assert "0.1.0.0" in _both(path, RuntimeError)
    open(os.path.join(path, "0.1.0.0"), "wb").write(b"\x02\x01\x21")
    assert "shorter" in _both(path, RuntimeError)


def test_a_damaged_chunk_raises_value_error_naming_the_file(golden, tmp_path):
    d = golden("blosc.npz")
    path = str(tmp_path / "a.zarr")
    write_store(path, d, "a")
    fn = os.path.join(path, "2.0.0.0")
    good = open(fn, "rb").read()
    p0 = int.from_bytes(good[16:20], "little")
    # a payload byte (the first token now asks for more literals than the stream has), a block start outside the
    # frame, a split prefix longer than the frame
    for at, patch in ((p0 + 4, b"\xf0\xff\xff\xff\xff"), (16, (len(good) + 7).to_bytes(4, "little")), (p0, b"\xff\xff\xff\x7f")):
        bad = bytearray(good)
        bad[at:at + len(patch)] = patch
        open(fn, "wb").write(bytes(bad))
        text = _both(path, ValueError)
        assert fn in text and "status" in text
