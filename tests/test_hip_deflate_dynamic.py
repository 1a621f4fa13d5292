"""Dynamic Huffman codes in the HIP deflate encoder (deflate_piece_kernel<true>, sk_deflate_streams_coded), on the
device.  Beyond "zlib can read it" the streams are walked by tests/deflate_reader.py, so that the tests see every
piece's block type, code lengths and tokens: the parse must be that of the fixed mode, the block type the smallest of
the three forms, the code optimal for the block's own histogram and equal to what the host text gives."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import deflate_reader as R
from tests.test_deflate_code_cpu import code_host, huffman_optimum
from tests.test_hip_deflate import _blob_outputs, _check, _chunk_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PIECE = 16384


def _encode(rows, elem_bytes=1, skip_zero=False, huffman="dynamic"):
    from skoots_amd.lib import deflate
    n = len(rows)
    length = len(rows[0]) if n else 0
    arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, length) if length else np.zeros((n, 0), np.uint8)
    return deflate.deflate_streams(torch.from_numpy(arr.copy()).to(DEV), elem_bytes=elem_bytes, skip_zero=skip_zero,
                                   huffman=huffman)


def _pieces(stream, raw):
    """The stream's blocks grouped by 16 KiB piece: [(data block, aligning block or None)]; checks the framing: every
    coded piece but the last is followed by an empty stored block that ends on a byte, a stored piece ends on one."""
    s = R.read_zlib(stream)
    assert s.output == raw
    n_pieces = max(1, -(-len(raw) // PIECE))
    out, blocks = [], list(s.blocks)
    for p in range(n_pieces):
        data = blocks.pop(0)
        align = None
        if p < n_pieces - 1:
            if data.type == "stored":
                assert data.end_bit % 8 == 0 and not data.final
                out.append((data, None))
                continue
            align = blocks.pop(0)
            assert align.type == "stored" and align.stored == b"" and not align.final and align.end_bit % 8 == 0
            assert not data.final
        else:
            assert data.final
        out.append((data, align))
    assert not blocks
    return out


def _block_bytes(bits, last):
    """Bytes of a piece whose data block has ``bits`` bits: the last one is padded to a byte, any other is followed
    by the 3 header bits of the empty stored block, padding, and its LEN / NLEN."""
    return (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4


def _token_bytes(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def _dynamic_bits(tokens):
    """Bits of the dynamic form of these tokens as the encoder defines it: host code builder + host header."""
    from tests.test_deflate_code_cpu import header_host
    lit, dist, extra = R.histogram(tokens)
    ll, dl = code_host(lit, 15)[0], code_host(dist, 15)[0]
    _, hbits = header_host(ll, dl)
    return hbits + sum(c * n for c, n in zip(lit, ll)) + sum(c * n for c, n in zip(dist, dl)) + extra, ll, dl


def _fixed_bits(tokens):
    lit, dist, extra = R.histogram(tokens)
    return 3 + sum(c * n for c, n in zip(lit, R.FIXED_LIT)) + 5 * sum(dist) + extra


def _compare_modes(raw, elem_bytes, fixed, dynamic):
    """Same parse, right choice, right code for one input and its two streams."""
    pf, pd = _pieces(fixed, raw), _pieces(dynamic, raw)
    assert len(pf) == len(pd)
    kinds = []
    for k, ((bf, af), (bd, ad)) in enumerate(zip(pf, pd)):
        last = k == len(pf) - 1
        n = len(raw[k * PIECE:(k + 1) * PIECE])
        assert (af is None) == (last or bf.type == "stored") and (ad is None) == (last or bd.type == "stored")
        # the parse: a coded block shows its tokens; a stored one has none to show, its bytes are the piece's
        tokens = bf.tokens if bf.type != "stored" else (bd.tokens if bd.type != "stored" else None)
        if bf.type != "stored" and bd.type != "stored":
            assert bf.tokens == bd.tokens, f"piece {k}: the parse differs between the modes"
        for b in (bf, bd):
            if b.type == "stored":
                assert b.stored == raw[k * PIECE:(k + 1) * PIECE]
        assert bf.type in ("stored", "fixed")
        if tokens is None:
            # stored in both modes: no block shows the parse, so there are no tokens to recompute the choice from; what
            # holds is that the bytes are the piece's (above) and that the dynamic stream is no longer (the caller)
            kinds.append("stored")
            continue
        assert _token_bytes(tokens) == raw[k * PIECE:(k + 1) * PIECE]
        # the choice: argmin of the three byte counts, on equal bytes stored, then fixed, then dynamic
        dbits, ll, dl = _dynamic_bits(tokens)
        sizes = [("stored", 5 + n), ("fixed", _block_bytes(_fixed_bits(tokens), last)),
                 ("dynamic", _block_bytes(dbits, last))]
        want = min(sizes, key=lambda kv: kv[1])[0]   # min() keeps the first of equal values
        assert bd.type == want, (k, sizes, bd.type)
        kinds.append(bd.type)
        got_bytes = (bd if ad is None else ad).byte_range[1] - bd.byte_range[0]
        assert got_bytes == dict(sizes)[want]
        if bd.type == "dynamic":
            # the code: the header's lengths are the host text's, and the payload costs the heapq optimum
            assert bd.lit_lengths == ll and bd.dist_lengths == dl, f"piece {k}: device and host code differ"
            assert bd.header_bits + bd.payload_bits == dbits
            lit, dist, extra = R.histogram(tokens)
            cost = sum(c * n for c, n in zip(lit, bd.lit_lengths)) + sum(c * n for c, n in zip(dist, bd.dist_lengths))
            assert cost + extra == bd.payload_bits
            best = 0
            for freq in (lit, dist):
                used = sum(1 for f in freq if f)
                opt, depth = huffman_optimum(freq) if used else (0, 0)
                if depth > 15:
                    best = None
                    break
                best += opt
            if best is not None:
                assert cost == best, f"piece {k}: payload {cost} bits, optimum {best}"
    return kinds


LENGTHS = (0, 1, 2, 3, 257, 258, 259, 16383, 16384, 16385, 40000, 65537)


def _edge_rows(length):
    rng = np.random.default_rng(length)
    last = bytearray(length)
    if length:
        last[-1] = 9
    return [bytes(length), b"\xff" * length, rng.integers(0, 256, length, dtype=np.uint8).tobytes(), bytes(last),
            (b"abc" * (length // 3 + 1))[:length], (b"\x00\x01\x02\x03\x04" * (length // 5 + 1))[:length]]


@pytest.mark.parametrize("length", LENGTHS)
def test_edge_lengths(length):
    rows = _edge_rows(length)
    for e in (1, 2, 4):
        together = _encode(rows, elem_bytes=e)
        fixed = _encode(rows, elem_bytes=e, huffman="fixed")
        assert len(together) == len(rows)
        for raw, s, f in zip(rows, together, fixed):
            _check(s, raw)
            _check(f, raw)
            assert len(s) <= len(f)
            alone = _encode([raw], elem_bytes=e)[0]
            assert alone == s, "a stream's bytes must not depend on the batch it is in"
            if e == 1 or length <= 16385:
                _compare_modes(raw, e, f, s)
    if length == 0:
        assert all(len(s) == 8 for s in together)


def test_fixed_mode_is_the_old_entry_point():
    """huffman = 0 of the new entry point writes the bytes of sk_deflate_streams; other values are refused by name."""
    from skoots_amd import _ffi
    from skoots_amd.lib import deflate
    rows = _edge_rows(40000)
    t = torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 40000).copy()).to(DEV)
    n, length = t.shape
    ws_bytes = int(_ffi.lib.sk_deflate_workspace_bytes(n, length))
    outs = []
    for mode in (None, 0):
        dst = torch.zeros(n * deflate.bound(length), dtype=torch.uint8, device=DEV)
        offs = torch.empty(n + 1, dtype=torch.int64, device=DEV)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        if mode is None:
            _ffi.check(_ffi.lib.sk_deflate_streams(_ffi.ptr(t), n, length, 1, _ffi.ptr(dst), _ffi.ptr(offs), None,
                                                   _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(DEV)))
        else:
            _ffi.check(_ffi.lib.sk_deflate_streams_coded(_ffi.ptr(t), n, length, 1, mode, _ffi.ptr(dst), _ffi.ptr(offs),
                                                         None, _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(DEV)))
        o = offs.cpu().tolist()
        outs.append((o, dst[:o[-1]].cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="sk_deflate_streams_coded: huffman"):
            _ffi.check(_ffi.lib.sk_deflate_streams_coded(_ffi.ptr(t), n, length, 1, bad, _ffi.ptr(dst), _ffi.ptr(offs),
                                                         None, _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr(DEV)))
    with pytest.raises(ValueError, match="workspace"):
        _ffi.check(_ffi.lib.sk_deflate_streams_coded(_ffi.ptr(t), n, length, 1, 1, _ffi.ptr(dst), _ffi.ptr(offs), None,
                                                     _ffi.ptr(ws), 16, _ffi.stream_ptr(DEV)))
    for bad in ("Fixed", "", None, 1):
        with pytest.raises(ValueError, match="huffman"):
            deflate.deflate_streams(t, huffman=bad)
    cpu = deflate.deflate_streams(t.cpu()[:1], huffman="dynamic")
    assert cpu == [zlib.compress(rows[0], 1)]


def _mixed_rows():
    """Rows whose pieces take every form: two-literal noise, few-symbol noise, text, runs, random bytes, sparse fields."""
    rng = np.random.default_rng(21)
    n = 3 * PIECE + 1234
    coin = (rng.integers(0, 2, n, dtype=np.uint8) * 128).astype(np.uint8).tobytes()
    few = rng.choice(np.array([0, 1, 2, 3, 7, 200], np.uint8), n, p=[0.5, 0.2, 0.1, 0.1, 0.05, 0.05]).tobytes()
    text = (b"the quick brown fox jumps over the lazy dog. " * (n // 45 + 1))[:n]
    sparse = (rng.integers(1, 255, n, dtype=np.uint8) * (rng.random(n) < 0.03)).astype(np.uint8).tobytes()
    rand = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    half = (rng.integers(0, 256, n, dtype=np.uint8) >> 1).astype(np.uint8).tobytes()   # 128 values: 7 bits beat 8
    f16 = (rng.standard_normal(n // 2) * (rng.random(n // 2) < 0.3)).astype(np.float16).tobytes()
    return [coin, few, text, sparse, rand, half, f16]


def test_same_parse_right_choice_right_code():
    rows = _mixed_rows()
    seen = set()
    for e in (1, 2):
        fixed, dyn = _encode(rows, elem_bytes=e, huffman="fixed"), _encode(rows, elem_bytes=e)
        for raw, f, d in zip(rows, fixed, dyn):
            _check(d, raw)
            assert len(d) <= len(f)
            seen.update(_compare_modes(raw, e, f, d))
    assert seen == {"stored", "fixed", "dynamic"}, seen


def _geometric_piece(seed):
    """One piece of 16 KiB, all literals, whose counts fall geometrically (ratio 1.618) over 18 byte values: 1, 2, 3, 5,
    8, ... 2584 and the rest for the most common one.  With the end-of-block symbol's count of 1 that is the Fibonacci
    histogram, whose optimal tree is a comb.  The 18 values fill two of every three positions in an order drawn from the
    seed; every third position cycles through 22 other values, so that with ``elem_bytes`` = 1 (distances 1 ... 64) no
    three bytes in a row repeat at any candidate distance: the parse is 16 384 literals and the histogram is exact."""
    rng = np.random.default_rng(seed)
    blockers = (PIECE + 2) // 3
    fib = [1, 2]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += PIECE - blockers - sum(fib)
    skew = np.repeat(np.arange(70, 88, dtype=np.uint8), fib)
    rng.shuffle(skew)
    x = np.empty(PIECE, np.uint8)
    free = np.ones(PIECE, bool)
    free[0::3] = False
    x[0::3] = np.arange(blockers) % 22
    x[free] = skew
    return x.tobytes()


LIMIT_SEED = 4


def test_limit_on_the_device():
    raw = _geometric_piece(LIMIT_SEED)
    fixed, dyn = _encode([raw], huffman="fixed")[0], _encode([raw])[0]
    (bf, _), = _pieces(fixed, raw)
    assert bf.type == "fixed"
    lit, dist, _ = R.histogram(bf.tokens)
    depth = huffman_optimum(lit)[1]
    assert depth > 15, f"seed {LIMIT_SEED}: the optimal literal/length code is only {depth} deep, the limit is not met"
    _check(dyn, raw)
    (bd, _), = _pieces(dyn, raw)
    assert bd.type == "dynamic" and bd.tokens == bf.tokens and max(bd.lit_lengths) == 15
    assert bd.lit_lengths == code_host(lit, 15)[0] and bd.dist_lengths == code_host(dist, 15)[0]
    assert len(dyn) < len(fixed)


def _de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) (Lyndon words), unrolled: every n-gram over k values once."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq + seq[:n - 1]


def test_no_distance_code():
    seq = _de_bruijn(8, 3)
    assert len(seq) == 514
    grams = [tuple(seq[i:i + 3]) for i in range(512)]
    assert len(set(grams)) == 512                      # no trigram repeats: no match of length 3 anywhere
    raw = bytes(np.array([3, 17, 40, 90, 128, 200, 251, 255], np.uint8)[seq])
    s = _encode([raw])[0]
    _check(s, raw)
    (b, _), = _pieces(s, raw)
    assert b.type == "dynamic"
    assert b.tokens == list(raw)
    assert b.hdist == 1 and b.dist_lengths == [0] * 30
    assert sum(1 for n in b.lit_lengths[:256] if n) == 8 and sum(1 for n in b.lit_lengths[257:] if n) == 0


def test_one_distance_code():
    raw = b"\x5a" * PIECE
    s = _encode([raw])[0]
    _check(s, raw)
    (b, _), = _pieces(s, raw)
    assert b.type == "dynamic"
    assert all(isinstance(t, tuple) and t[1] == 1 for t in b.tokens[1:]) and b.tokens[0] == 0x5a
    assert b.hdist == 1 and b.dist_lengths == [1] + [0] * 29
    assert len(s) < len(_encode([raw], huffman="fixed")[0])


def test_skip_zero_behaves_as_in_the_fixed_mode():
    rows = [bytes(70000), b"\x00" * 69999 + b"\x01", bytes(70000), b"\x02" + bytes(69999)]
    got = _encode(rows, skip_zero=True)
    assert [g is None for g in got] == [True, False, True, False]
    assert [g is None for g in _encode(rows, skip_zero=True, huffman="fixed")] == [True, False, True, False]
    _check(got[1], rows[1])
    _check(got[3], rows[3])
    kept = _encode(rows, skip_zero=False)
    for raw, s in zip(rows, kept):
        _check(s, raw)
    assert kept[1] == got[1] and kept[3] == got[3]


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
    fixed = _encode(rows, elem_bytes=1, huffman="fixed")
    assert sum(map(len, _encode(rows))) < sum(map(len, fixed))


def test_device_inflater_reads_the_dynamic_blocks():
    from skoots_amd.lib import deflate
    rows = _mixed_rows()
    streams = _encode(rows, elem_bytes=2)
    assert any(b.type == "dynamic" for s in streams for b in R.read_zlib(s).blocks)
    back = deflate.inflate_streams(streams, len(rows[0]), DEV)
    assert [bytes(r) for r in back.cpu().numpy()] == [bytes(r) for r in rows]
    edge = [r for length in (1, 259, 16385) for r in _edge_rows(length)]
    streams = [_encode([r])[0] for r in edge]
    flat, offs = deflate.inflate_streams(streams, [len(r) for r in edge], DEV)
    flat = flat.cpu().numpy().tobytes()
    assert [flat[a:b] for a, b in zip(offs[:-1], offs[1:])] == edge


def test_writers_with_dynamic_codes(tmp_path):
    from PIL import Image

    from skoots_amd.lib import tiff, zarr_store
    rng = np.random.default_rng(5)
    vec = np.zeros((3, 300, 270, 70), np.float16)
    vec[:, 40:200, 30:90, 5:60] = rng.standard_normal((3, 160, 60, 55)).astype(np.float16)
    vec[1] = 0   # a whole channel of fill value: its chunks are left out
    skel = (rng.random((1, 130, 257, 64)) < 0.01).astype(np.uint8)
    for k, (arr, chunks) in enumerate(((vec, None), (skel, None), (skel, (1, 64, 64, 64)))):
        a, b = str(tmp_path / f"a{k}.zarr"), str(tmp_path / f"b{k}.zarr")
        zarr_store.save_device(a, torch.from_numpy(arr).to(DEV), chunks, budget_bytes=40 << 20)
        zarr_store.save_device(b, torch.from_numpy(arr).to(DEV), chunks, budget_bytes=40 << 20, huffman="dynamic")
        assert sorted(os.listdir(a)) == sorted(os.listdir(b))
        assert open(os.path.join(a, ".zarray")).read() == open(os.path.join(b, ".zarray")).read()
        assert np.array_equal(zarr_store.load(b), arr)
        size = {p: sum(os.path.getsize(os.path.join(p, f)) for f in os.listdir(p)) for p in (a, b)}
        assert size[b] < size[a]
    with pytest.raises(ValueError, match="huffman"):
        zarr_store.save_device(str(tmp_path / "c.zarr"), torch.from_numpy(skel).to(DEV), huffman="best")
    for dtype in (np.uint8, np.uint16, np.int32):
        pages = rng.integers(0, 200, (5, 61, 47)).astype(dtype) * (rng.random((5, 61, 47)) < 0.3)
        pages = pages.astype(dtype)
        path = str(tmp_path / f"p_{np.dtype(dtype).name}.tif")
        tiff.write_stack(path, torch.from_numpy(pages).to(DEV), huffman="dynamic")
        with Image.open(path) as im:
            assert im.n_frames == 5
            got = []
            for z in range(5):
                im.seek(z)
                got.append(np.array(im))
        assert np.array_equal(np.stack(got), pages)
        back = tiff.read_image(path)
        assert back.dtype == dtype and np.array_equal(back, pages)
        fixed = str(tmp_path / f"f_{np.dtype(dtype).name}.tif")
        tiff.write_stack(fixed, torch.from_numpy(pages).to(DEV))
        assert os.path.getsize(path) <= os.path.getsize(fixed)
    lab = torch.from_numpy(rng.integers(0, 70000, (3, 20, 30)).astype(np.int32)).to(DEV)
    tiff.write_label_stack(str(tmp_path / "wide.tif"), lab, huffman="dynamic")
    assert np.array_equal(tiff.read_image(str(tmp_path / "wide.tif")), lab.cpu().numpy())
    tiff.write_label_stack(str(tmp_path / "narrow.tif"), lab % 65536, huffman="dynamic")
    narrow = tiff.read_image(str(tmp_path / "narrow.tif"))
    assert narrow.dtype == np.uint16 and np.array_equal(narrow, (lab % 65536).cpu().numpy())
    flt = (rng.standard_normal((4, 33, 29)) * (rng.random((4, 33, 29)) < 0.4)).astype(np.float32)
    tiff.write_float_stack(str(tmp_path / "float.tif"), torch.from_numpy(flt).to(DEV), huffman="dynamic")
    with Image.open(str(tmp_path / "float.tif")) as im:
        assert im.n_frames == 4
        for z in range(4):
            im.seek(z)
            assert np.array_equal(np.array(im), flt[z])


def test_blob_field_outputs_are_smaller():
    """The first four chunks of the vectors, all skeleton chunks and all mask pages of the 512 x 512 x 64 blob field:
    the dynamic total is strictly below the fixed total for each.  The ratios and the header share are printed (and
    stand in DESIGN.md section 15); no ratio is asserted."""
    vectors, skeleton, mask = _blob_outputs()
    for name, rows, e in (("vectors", _chunk_rows(vectors)[:4], 2), ("skeleton", _chunk_rows(skeleton), 1),
                          ("mask", [p.numpy().tobytes() for p in mask], 2)):
        fixed, dyn = _encode(rows, elem_bytes=e, huffman="fixed"), _encode(rows, elem_bytes=e)
        for raw, f, d in zip(rows, fixed, dyn):
            _check(d, raw)
            assert len(d) <= len(f)
        tf, td = sum(map(len, fixed)), sum(map(len, dyn))
        # header share: the blocks of a sample, the first 256 KiB of up to four rows (pieces are coded independently,
        # so these are the blocks the whole rows begin with)
        sample = [r[:16 * PIECE] for r in rows[::max(1, len(rows) // 4)][:4]]
        hdr = tot = 0
        kinds = {"stored": 0, "fixed": 0, "dynamic": 0}
        for raw, s in zip(sample, _encode(sample, elem_bytes=e)):
            for b, _ in _pieces(s, raw):
                kinds[b.type] += 1
                if b.type == "dynamic":
                    hdr += b.header_bits
                    tot += b.header_bits + b.payload_bits
        print(f"{name}: fixed {tf} bytes, dynamic {td} bytes, ratio {td / tf:.3f}; sample pieces {kinds}, "
              f"header share of the dynamic blocks' bits {hdr / max(tot, 1):.3f}")
        assert td < tf, (name, td, tf)
