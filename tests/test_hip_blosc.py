"""The HIP LZ4 block decoder and the Blosc unshuffle (skoots_amd/csrc/blosc.hip) and the readers on top of them, on the
device.  The oracle for a stream is the pure-Python reference of tests/blosc_corpus.py: a stream's status is 0 exactly
when the reference accepts it, and then the bytes are the reference's; the host build of the same decoder text
(``sk_blosc_decode_host``) must agree on every case a frame can carry.  Every LZ4 launch goes through ``_run``, which
lays guard bytes before and after every stream's dst range and checks that they are intact, whatever the stream was.

No malformed input runs here that has not run before on the CPU build of the same decoder text under AddressSanitizer
and UBSan (tools/blosc_host_check.py: this corpus, the out-of-range rows and the golden frames, in allocations of exactly
their sizes); DESIGN.md section 19 has the result."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import blosc_corpus as C

pytestmark = pytest.mark.gpu

CHUNKS, good_frames, write_store = C.CHUNKS, C.good_frames, C.write_store
DEV = "cuda:0"
GUARD = 64
FILL = 0xA5


def _launch(src: bytes, rows, dst_bytes):
    from skoots_amd import _ffi
    s = torch.frombuffer(bytearray(src) or bytearray(1), dtype=torch.uint8).to(DEV)
    assert s.data_ptr() % 8 == 0
    table = torch.tensor(rows, dtype=torch.int64, device=DEV).view(-1, 5)
    dst = torch.full((max(1, dst_bytes),), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((len(rows),), -1, dtype=torch.int32, device=DEV)
    _ffi.check(_ffi.lib.sk_lz4_streams(_ffi.ptr(s), len(src), _ffi.ptr(table), len(rows), _ffi.ptr(dst), dst_bytes,
                                       _ffi.ptr(status), _ffi.stream_ptr(torch.device(DEV))))
    return status.cpu().tolist(), dst.cpu().numpy()[:dst_bytes]


def _run(cases, src_leads=None, dst_leads=None):
    """One launch for ``cases``.  Between the streams lie gap rows: no input at all (refused before anything is
    written), their dst range is the guard.  Stream k starts ``src_leads[k]`` / ``dst_leads[k]`` bytes past a multiple
    of 8 in src / dst.  Returns (status per case, output bytes per case)."""
    n = len(cases)
    src, rows, at = bytearray(), [], 0
    for k, c in enumerate(cases):
        sl = 0 if src_leads is None else src_leads[k]
        dl = 0 if dst_leads is None else dst_leads[k]
        src += b"\xff" * ((sl - len(src)) % 8)
        guard = GUARD + (dl - (at + GUARD)) % 8
        rows.append((len(src), 0, at, guard, C.KIND_LZ4))
        at += guard
        assert len(src) % 8 == sl and at % 8 == dl
        rows.append((len(src), len(c.stream), at, c.size, c.kind))
        src += c.stream
        at += c.size
    rows.append((len(src), 0, at, GUARD, C.KIND_LZ4))
    at += GUARD
    st, out = _launch(bytes(src), rows, at)
    for g in range(0, 2 * n + 1, 2):
        assert st[g] == C.E_INPUT, "a gap row was not refused for its empty input"
        assert (out[rows[g][2]:rows[g][2] + rows[g][3]] == FILL).all(), f"guard bytes around stream {g // 2} were written"
    return [st[2 * k + 1] for k in range(n)], [out[rows[2 * k + 1][2]:rows[2 * k + 1][2] + cases[k].size].tobytes() for k in range(n)]


@functools.lru_cache(maxsize=None)
def _host(case):
    """(status, bytes) of sk_blosc_decode_host for the case as the one split of a frame; None where no frame carries it."""
    from skoots_amd import _ffi
    frame = C.frame_of(case.stream, case.size) if case.kind == C.KIND_LZ4 else None
    if frame is None:
        return None
    out = np.zeros(case.size, np.uint8)
    status = ctypes.c_int32(0)
    _ffi.check(_ffi.lib.sk_blosc_decode_host(frame, len(frame), out.ctypes.data, case.size, ctypes.byref(status)))
    return status.value, out.tobytes()


def _check(cases, src_leads=None, dst_leads=None):
    """Status and bytes of every case against the reference and against the host decoder; guards by ``_run``."""
    status, data = _run(cases, src_leads, dst_leads)
    for c, st, d in zip(cases, status, data):
        want_status, want = C.decode(c.stream, c.size, c.kind)
        assert want == c.expect, c.name
        assert st == want_status, f"{c.name}: status {st}, the reference says {want_status}"
        if c.code:
            assert st == c.code, f"{c.name}: status {st}, wanted {c.code}"
        if want is not None:
            assert d == want, f"{c.name}: wrong bytes"
        host = _host(c)
        if host is not None:
            assert host[0] == st and (st != 0 or host[1] == d), f"{c.name}: device and host decoder differ"
    return status, data


def _check_batch_and_alone(cases):
    status, data = _check(cases)
    for c, st, d in zip(cases, status, data):
        st1, d1 = _run([c])
        assert st1[0] == st and (st != 0 or d1[0] == d), f"{c.name}: the output depends on the batch"


@functools.lru_cache(maxsize=None)
def _golden_cases():
    """Every stream of every golden frame that must decode, cut out of its frame by ``plan``."""
    from skoots_amd.lib import blosc
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "blosc.npz"))
    cases = []
    for name, frame, raw in good_frames(d):
        p = blosc.plan([frame], len(raw))
        for k, (sb, sl, _, dl, kind) in enumerate(p.streams.tolist()):
            stream = frame[sb:sb + sl]
            status, want = C.decode(stream, dl, kind)
            assert status == 0, name
            cases.append(C.Case(f"{name}#{k}", stream, dl, want, 0, kind))
    return cases


# ------------------------------------------------------------------------------------------ streams
def test_hand_assembled_streams():
    cases = C.hand_assembled()
    names = {c.name for c in cases}
    assert names >= {"empty_output", "lit0_last", "lit271_first", "match274", "offset1", "offset65535", "out131072_offset7",
                     "match_wraps_the_ring", "source_wraps_the_ring", f"src{C.WINDOW - 1}", f"src{C.WINDOW + 1}", "out65537"}
    _check_batch_and_alone(cases)


def test_golden_streams():
    cases = _golden_cases()
    assert len(cases) > 50 and any(c.kind == C.KIND_STORED for c in cases)
    _check_batch_and_alone(cases)


@pytest.mark.parametrize("lead", range(1, 8))
def test_unaligned_stream_starts(lead):
    cases = C.hand_assembled() + C.named_errors() + _golden_cases()[:12]
    n = len(cases)
    _check(cases, [lead] * n, [0] * n)
    _check(cases, [0] * n, [lead] * n)
    _check(cases, [(lead + k) % 8 for k in range(n)], [(3 * lead + 5 * k) % 8 for k in range(n)])


def test_every_truncation_follows_the_reference():
    cases = C.truncations()
    assert len(cases) == sum(len(s) for s in C.short_streams())
    status, _ = _check(cases + C.good_neighbours())
    assert all(st != 0 for st in status[:len(cases)])


def test_every_single_bit_flip_follows_the_reference():
    cases = C.bit_flips()
    assert len(cases) == 8 * sum(len(s) for s in C.short_streams())
    accepted = sum(c.expect is not None for c in cases)
    assert 0 < accepted < len(cases)
    status, _ = _check(cases + C.good_neighbours())
    assert sum(st == 0 for st in status[:len(cases)]) == accepted


def test_named_errors_report_their_codes():
    cases = C.named_errors()
    names = {c.name: c.code for c in cases}
    assert names["stored_lengths_differ"] == C.E_RANGE and names["ends_after_match"] == names["offset_cut"] == C.E_INPUT
    assert names["offset_zero"] == names["offset_before_output"] == C.E_OFFSET
    assert names["expected_one_less"] == names["match_overflows"] == C.E_LONG and names["expected_one_more"] == C.E_SHORT
    assert {c.code for c in cases} == {C.E_RANGE, C.E_INPUT, C.E_OFFSET, C.E_LONG, C.E_SHORT}
    _check_batch_and_alone(cases + C.good_neighbours())


def test_rows_out_of_range_are_refused_and_write_nothing():
    stream = C.seq(b"abcdefgh", 4, 8) + C.last(b"12345")
    good = C.Case("good", stream, 21, C.decode(stream, 21)[1])
    rows = C.range_rows(40, 48)
    src = good.stream + bytes(40 - len(good.stream))
    st, out = _launch(src, [(0, len(good.stream), 8, good.size, 0)] + rows, 48)
    assert st[0] == 0 and out[8:8 + good.size].tobytes() == good.expect
    assert st[1:] == [C.E_RANGE] * len(rows)
    assert (out[:8] == FILL).all() and (out[8 + good.size:] == FILL).all()


def test_arguments_are_checked_before_the_launch():
    from skoots_amd import _ffi
    t = torch.zeros(64, dtype=torch.uint8, device=DEV)
    stream = _ffi.stream_ptr(torch.device(DEV))
    assert _ffi.lib.sk_lz4_streams(_ffi.ptr(t), 64, _ffi.ptr(t), -1, _ffi.ptr(t), 64, _ffi.ptr(t), stream) == -1
    assert _ffi.lib.sk_lz4_streams(_ffi.ptr(t), -1, _ffi.ptr(t), 1, _ffi.ptr(t), 64, _ffi.ptr(t), stream) == -1
    assert _ffi.lib.sk_lz4_streams(_ffi.ptr(t), 64, _ffi.ptr(t[4:]), 1, _ffi.ptr(t), 64, _ffi.ptr(t), stream) == -1
    assert _ffi.lib.sk_lz4_streams(None, 64, _ffi.ptr(t), 1, _ffi.ptr(t), 64, _ffi.ptr(t), stream) == -1
    for ts in (0, 1, 17):
        assert _ffi.lib.sk_blosc_unshuffle(_ffi.ptr(t), _ffi.ptr(t[32:]), _ffi.ptr(t), 1, ts, stream) == -1
    assert _ffi.lib.sk_blosc_unshuffle(_ffi.ptr(t), _ffi.ptr(t), _ffi.ptr(t), 1, 2, stream) == -1
    assert _ffi.lib.sk_lz4_streams(None, 0, None, 0, None, 0, None, stream) == 0


# ------------------------------------------------------------------------------------------ unshuffle
@pytest.mark.parametrize("ts", [2, 3, 4, 8, 16])
def test_unshuffle(ts):
    """Blocks with 0 to 15 tail bytes at unaligned begins, from a block smaller than one element up to one of more tiles
    than the grid has rows (a workgroup then takes more than one), guard bytes between them."""
    from skoots_amd import _ffi
    rng = np.random.default_rng(ts)
    nes = (0, 1, 5, 63, 64, 65, 255, 256, 257, 1000, 1365, 2048, 4095, 4097, 9000, 3)
    sizes = [ts * ne + k % ts for k, ne in enumerate(nes)] + [ts * (150000 // ts) + ts - 1, 4096 * 3, 1]
    begins, at = [], 0
    for k, s in enumerate(sizes):
        at += GUARD
        at += (k * 7 + 3 - at) % 16              # block k begins 7 k + 3 past a multiple of 16: every phase occurs
        begins.append(at)
        at += s
    total = at + GUARD
    src = rng.integers(0, 256, total, dtype=np.uint8)
    want = np.full(total, FILL, np.uint8)
    for b, s in zip(begins, sizes):
        ne = s // ts
        want[b:b + ne * ts] = src[b:b + ne * ts].reshape(ts, ne).T.reshape(-1)
        want[b + ne * ts:b + s] = src[b + ne * ts:b + s]
    assert {s % ts for s in sizes} == set(range(ts)) and {b % 16 for b in begins} == set(range(16))
    for shift in (0, 3):                      # the whole buffer moved: other 16-byte phases of the same blocks
        s = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), src])).to(DEV)[shift:]
        d = torch.full((total + shift,), FILL, dtype=torch.uint8, device=DEV)[shift:]
        blocks = torch.tensor([[b, n] for b, n in zip(begins, sizes)] + [[-1, 5], [0, 0], [3, -2]], dtype=torch.int64, device=DEV)
        _ffi.check(_ffi.lib.sk_blosc_unshuffle(_ffi.ptr(s), _ffi.ptr(d), _ffi.ptr(blocks), int(blocks.shape[0]), ts,
                                               _ffi.stream_ptr(torch.device(DEV))))
        got = d.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"typesize {ts}, shift {shift}: first wrong byte at {bad[:1]}"


# ------------------------------------------------------------------------------------------ frames and stores
def test_decode_device_on_the_golden_frames(golden):
    from skoots_amd.lib import blosc
    d = golden("blosc.npz")
    frames = good_frames(d)
    for name, frame, raw in frames:
        got = blosc.decode_device([frame], len(raw), DEV)
        assert got.is_cuda and tuple(got.shape) == (1, len(raw)) and got.cpu().numpy().tobytes() == raw, name
        assert blosc.decode_host([frame], len(raw)).tobytes() == raw
    # all chunks of a store in one call, and a call that mixes shuffled and unshuffled frames of one size
    a = [(f, r) for n, f, r in frames if n.startswith("a:")]
    got = blosc.decode_device([f for f, _ in a], 327680, DEV)
    assert got.cpu().numpy().tobytes() == b"".join(r for _, r in a)
    raw = a[0][1]
    plain = C.frame_of(C.last(raw), len(raw))
    got = blosc.decode_device([a[0][0], plain, a[1][0]], 327680, DEV)
    assert got.cpu().numpy().tobytes() == raw + raw + a[1][1]
    # a damaged frame in the middle of a call is named by its index
    with pytest.raises(blosc.BloscError, match=r"frame 1 of 3 does not decode: offset 0") as e:
        blosc.decode_device([a[0][0], C.damaged(a[1][0]), a[2][0]], 327680, DEV)
    assert e.value.index == 1
    for n in d["d_names"]:
        with pytest.raises(blosc.BloscError, match="status 7"):
            blosc.decode_device([d[f"d_frame_{n}"].tobytes()], int(d["d_bytes"]), DEV)


def test_load_device_equals_load(golden, tmp_path):
    from skoots_amd.lib import zarr_store
    d = golden("blosc.npz")
    for prefix in "ab":
        path = str(tmp_path / f"{prefix}.zarr")
        arr = write_store(path, d, prefix)
        want = zarr_store.load(path)
        assert want.tobytes() == arr.tobytes()
        for budget in (zarr_store.LOAD_DEVICE_BUDGET, 1):        # 1: one chunk per batch
            got = zarr_store.load_device(path, DEV, budget_bytes=budget)
            assert got.is_cuda and tuple(got.shape) == want.shape
            assert got.cpu().numpy().dtype == want.dtype and got.cpu().numpy().tobytes() == want.tobytes()


def test_convert_of_a_blosc_store_gives_the_bytes_of_the_zlib_store(golden, tmp_path):
    from skoots_amd.lib import zarr_store
    from skoots_amd.utils.convert_trch_to_tif import convert
    d = golden("blosc.npz")
    outs = []
    for name, on_device in (("blosc_dev", True), ("blosc_host", False), ("zlib", True)):
        os.makedirs(tmp_path / name)
        store = str(tmp_path / name / "vol_skoots_vectors.zarr")
        if name == "zlib":
            zarr_store.save(store, d["a_array"], CHUNKS)
        else:
            write_store(store, d, "a")
        written = convert(str(tmp_path / name), DEV, read_on_device=on_device)
        assert [os.path.basename(w) for w in written] == ["vol_skoots_vectors.tif"]
        outs.append(open(written[0], "rb").read())
    assert outs[0] == outs[2] and outs[1] == outs[2] and len(outs[2]) > 1000
