"""Pins tests/deflate_reader.py against zlib: streams made by zlib.compressobj at level 0 and 1 and with Z_FIXED,
Z_HUFFMAN_ONLY and Z_RLE must be walked to their last bit, the tokens must expand to the input, and the bit counts of
the blocks must add up to the stream's length."""
import zlib

import numpy as np
import pytest

from tests import deflate_reader as R


def _inputs():
    rng = np.random.default_rng(2)
    sparse = (rng.integers(0, 3, 70000, dtype=np.uint8) * (rng.random(70000) < 0.2)).astype(np.uint8).tobytes()
    return {
        "empty": b"",
        "one": b"\x07",
        "text": b"the quick brown fox jumps over the lazy dog, " * 300,
        "random": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(),
        "sparse": sparse,
        "runs": np.repeat(np.arange(200, dtype=np.uint8), np.arange(1, 201)).tobytes(),
        "zeros": bytes(100000),
    }


CONFIGS = {
    "level0": dict(level=0, strategy=zlib.Z_DEFAULT_STRATEGY),
    "level1": dict(level=1, strategy=zlib.Z_DEFAULT_STRATEGY),
    "fixed": dict(level=1, strategy=zlib.Z_FIXED),
    "huffman_only": dict(level=1, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(level=1, strategy=zlib.Z_RLE),
    "level9": dict(level=9, strategy=zlib.Z_DEFAULT_STRATEGY),
}


def _expand(blocks):
    out = bytearray()
    for b in blocks:
        if b.type == "stored":
            out += b.stored
        for t in b.tokens:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    out.append(out[-t[1]])
            else:
                out.append(t)
    return bytes(out)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(_inputs()))
def test_reader_walks_zlib_streams(name, config):
    raw = _inputs()[name]
    c = zlib.compressobj(CONFIGS[config]["level"], zlib.DEFLATED, 15, 8, CONFIGS[config]["strategy"])
    stream = c.compress(raw) + c.flush()
    s = R.read_zlib(stream)
    assert s.output == raw
    assert _expand(s.blocks) == raw
    assert 16 + sum(b.header_bits + b.payload_bits for b in s.blocks) + s.pad_bits + 32 == 8 * len(stream)
    assert [b.final for b in s.blocks] == [False] * (len(s.blocks) - 1) + [True]
    at = 16
    for b in s.blocks:
        assert b.start_bit == at and b.end_bit == at + b.header_bits + b.payload_bits
        assert b.byte_range == (at // 8, (b.end_bit + 7) // 8)
        at = b.end_bit
    types = {b.type for b in s.blocks}
    if config == "level0":
        assert types == {"stored"}
    if config == "fixed":
        assert types <= {"fixed", "stored"}
    if config == "huffman_only":
        assert all(not isinstance(t, tuple) for b in s.blocks for t in b.tokens)
    if config == "rle":
        assert all(t[1] == 1 for b in s.blocks for t in b.tokens if isinstance(t, tuple))
    for b in s.blocks:
        if b.type == "dynamic":
            assert len(b.lit_lengths) == 286 and len(b.dist_lengths) == 30 and b.lit_lengths[256] > 0
            # the payload is the tokens under the block's own lengths
            lit, dist, extra = R.histogram(b.tokens)
            bits = sum(c * n for c, n in zip(lit, b.lit_lengths)) + sum(c * n for c, n in zip(dist, b.dist_lengths))
            assert bits + extra == b.payload_bits
        if b.type == "fixed":
            lit, dist, extra = R.histogram(b.tokens)
            assert sum(c * n for c, n in zip(lit, R.FIXED_LIT)) + 5 * sum(dist) + extra == b.payload_bits


def test_reader_sees_a_sync_flush_and_refuses_damage():
    c = zlib.compressobj(1)
    stream = c.compress(b"abc" * 100) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(b"xyz" * 100) + c.flush()
    s = R.read_zlib(stream)
    assert s.output == b"abc" * 100 + b"xyz" * 100
    empty = [b for b in s.blocks if b.type == "stored" and b.stored == b""]
    assert len(empty) == 1 and empty[0].end_bit % 8 == 0
    with pytest.raises(ValueError):
        R.read_zlib(stream[:-1])
    with pytest.raises(ValueError):
        R.read_zlib(stream + b"\x00")
    bad = bytearray(stream)
    bad[-1] ^= 1
    with pytest.raises(ValueError, match="Adler"):
        R.read_zlib(bytes(bad))


def test_canonical_codes_are_rfc_1951():
    # the example of RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    assert R.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
