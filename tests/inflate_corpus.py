"""Streams for the inflate decoder's tests (tests/test_hip_inflate.py on the device, tools/inflate_host_check.py on the
sanitized CPU build): payloads x encoders of the stdlib's zlib, hand-assembled RFC 1951 blocks, malformed input.  A case
is ``Case(name, stream, wrapper, size, expect)``: the bytes, 0 = raw / 1 = zlib, the number of bytes the caller expects,
and ``expect`` = the payload when the stream must inflate, or None when it must be refused.  What a stream must do is
decided by ``oracle`` -- the stdlib's zlib -- never by the decoder under test; hand-assembled streams are confirmed
with it when they are made."""
from __future__ import annotations

import zlib
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

E_HEADER, E_BLOCK_TYPE, E_STORED, E_CODES, E_SYMBOL, E_DISTANCE, E_INPUT, E_LONG, E_SHORT, E_ADLER, E_RANGE = range(1, 12)


class Case(NamedTuple):
    name: str
    stream: bytes
    wrapper: int
    size: int
    expect: Optional[bytes]
    code: int = 0      # the status a named malformed case must report (0 = any non-zero / not checked)


def oracle(stream: bytes, wrapper: int, size: int) -> Optional[bytes]:
    """What zlib makes of it: the bytes if it inflates without error, reaches eof and gives ``size`` bytes, else None."""
    d = zlib.decompressobj(15 if wrapper else -15)
    try:
        out = d.decompress(stream, size + 1)
        if len(out) <= size and not d.eof:
            out += d.decompress(d.unconsumed_tail, size + 1 - len(out))
    except zlib.error:
        return None
    if not d.eof or len(out) != size:
        return None
    return out


# ------------------------------------------------------------------------------------------ payloads
LENGTHS = (0, 1, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65535, 65536, 65537, 1 << 20)
PATTERNS = ("zero", "ff", "random", "last", "period3", "period5")


def pattern(kind: str, n: int, seed: int = 0) -> bytes:
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind == "random":
        return np.random.default_rng(seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "last":
        return bytes(n - 1) + b"\x01" if n else b""
    if kind == "period3":
        return (b"\x01\x02\x03" * (n // 3 + 1))[:n]
    if kind == "period5":
        return (b"abcde" * (n // 5 + 1))[:n]
    raise ValueError(kind)


def run_table(dtype) -> bytes:
    """Runs of every length 1...300 of a value that changes from run to run."""
    parts = [np.full(k, (k * 2654435761) % 65521 + 1, dtype=np.uint32).astype(dtype) for k in range(1, 301)]
    return np.concatenate(parts).tobytes()


def payloads(big: bool = True) -> List[Tuple[str, bytes]]:
    out = [(f"{p}{n}", pattern(p, n)) for n in LENGTHS for p in PATTERNS if big or n < (1 << 20)]
    out += [(f"runs_{np.dtype(t).name}", run_table(t)) for t in (np.uint8, np.uint16, np.int32)]
    out.append(("block40000x3", pattern("random", 40000, seed=7) * 3))
    return out


def chunk_payload() -> bytes:
    """8 MiB, the stores' chunk size: a label-like field (runs), so that every encoder has matches to make."""
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 300, 1 << 16, dtype=np.uint16)
    reps = rng.integers(1, 128, 1 << 16)
    arr = np.repeat(vals, reps)
    arr = np.resize(arr, (8 << 20) // 2)
    return arr.tobytes()


def _deflate(data: bytes, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if flush is None:
        return c.compress(data) + c.flush()
    cut = len(data) // 3
    out = c.compress(data[:cut]) + c.flush(flush) + c.flush(flush)   # the second flush adds one more empty stored block
    return out + c.compress(data[cut:]) + c.flush()


ENCODERS = {
    "level0": (1, lambda d: _deflate(d, 0)),
    "level1": (1, lambda d: _deflate(d, 1)),
    "level6": (1, lambda d: _deflate(d, 6)),
    "level9": (1, lambda d: _deflate(d, 9)),
    "fixed": (1, lambda d: _deflate(d, 6, strategy=zlib.Z_FIXED)),
    "huffman_only": (1, lambda d: _deflate(d, 6, strategy=zlib.Z_HUFFMAN_ONLY)),
    "rle": (1, lambda d: _deflate(d, 6, strategy=zlib.Z_RLE)),
    "wbits9": (1, lambda d: _deflate(d, 6, wbits=9)),
    "raw": (0, lambda d: _deflate(d, 6, wbits=-15)),
    "sync_flush": (1, lambda d: _deflate(d, 6, flush=zlib.Z_SYNC_FLUSH)),
    "full_flush": (1, lambda d: _deflate(d, 6, flush=zlib.Z_FULL_FLUSH)),
}


def encoded(encoder: str, big: bool = True) -> List[Case]:
    wrapper, fn = ENCODERS[encoder]
    return [Case(f"{encoder}:{name}", fn(data), wrapper, len(data), data) for name, data in payloads(big)]


# ------------------------------------------------------------------------------------------ bit writer
class BitWriter:
    """RFC 1951 bit order: values least-significant bit first, Huffman codes most-significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, count: int) -> "BitWriter":
        assert 0 <= value < (1 << count) or count == 0
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code: int, length: int) -> "BitWriter":
        rev = int(format(code, f"0{length}b")[::-1], 2) if length else 0
        return self.bits(rev, length)

    def align(self) -> "BitWriter":
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data: bytes) -> "BitWriter":
        assert self.n == 0
        self.out += data
        return self

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def fixed_lit(sym: int) -> Tuple[int, int]:
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def len_token(length: int) -> Tuple[int, int, int]:
    """(symbol, extra bits, extra value); 258 as code 285."""
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_token(dist: int) -> Tuple[int, int, int]:
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def canonical(lengths: Sequence[int]) -> dict:
    """symbol -> (code, length) of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def complete_lengths(k: int) -> List[int]:
    """Lengths of a complete prefix code of k >= 2 symbols, the longer codes first."""
    m = k.bit_length() - 1
    r = k - (1 << m)
    return [m + 1] * (2 * r) + [m] * (k - 2 * r)


def lz_apply(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def fixed_block(w: BitWriter, tokens, final: bool = True) -> BitWriter:
    """tokens: int = literal, (length, dist) or (length, dist, (symbol, extra bits, extra value)) for a chosen length code."""
    w.bits(1 if final else 0, 1).bits(1, 2)
    for t in tokens:
        if isinstance(t, int):
            w.code(*fixed_lit(t))
        else:
            sym, eb, ev = t[2] if len(t) > 2 else len_token(t[0])
            w.code(*fixed_lit(sym)).bits(ev, eb)
            dc, deb, dev = dist_token(t[1])
            w.code(dc, 5).bits(dev, deb)
    return w.code(*fixed_lit(256))


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def rle_lengths(seq: Sequence[int]) -> List[Tuple[int, int]]:
    """Greedy code-length-code symbols (symbol, extra value) for the joined literal/length + distance lengths: runs do
    not stop at the boundary between the two, as RFC 1951 allows."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((17, take - 3) if take <= 10 else (18, take - 11))
            i += take
        elif v != 0 and run >= 4:
            out.append((v, 0))
            take = min(run - 1, 6)
            out.append((16, take - 3))
            i += 1 + take
        else:
            out.append((v, 0))
            i += 1
    return out


def dynamic_block(w: BitWriter, lit_lengths: Sequence[int], dist_lengths: Sequence[int], tokens, final: bool = True,
                  cl_symbols=None) -> BitWriter:
    """One dynamic block with exactly these code lengths (len(lit_lengths) >= 257, symbol 256 must have a code)."""
    seq = list(lit_lengths) + list(dist_lengths)
    cls = cl_symbols if cl_symbols is not None else rle_lengths(seq)
    used = sorted({s for s, _ in cls})
    cl_len = [0] * 19
    if len(used) == 1:
        used.append(next(s for s in range(19) if s not in used))   # a complete code needs two symbols
    for s, l in zip(used, sorted(complete_lengths(len(used)))):
        cl_len[s] = l
    assert max(cl_len) <= 7
    cl_code = canonical(cl_len)
    hclen = max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    w.bits(1 if final else 0, 1).bits(2, 2)
    w.bits(len(lit_lengths) - 257, 5).bits(len(dist_lengths) - 1, 5).bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_len[CL_ORDER[i]], 3)
    for s, ev in cls:
        w.code(*cl_code[s])
        if s >= 16:
            w.bits(ev, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lengths), canonical(dist_lengths)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            sym, eb, ev = len_token(t[0])
            w.code(*lit[sym]).bits(ev, eb)
            dc, deb, dev = dist_token(t[1])
            w.code(*dist[dc]).bits(dev, deb)
    return w.code(*lit[256])


def _confirmed(name: str, raw: bytes, payload: bytes) -> Case:
    got = zlib.decompressobj(-15).decompress(raw)
    assert got == payload, f"{name}: the construction is wrong (zlib gives {len(got)} bytes, wanted {len(payload)})"
    return Case(name, raw, 0, len(payload), payload)


def hand_assembled() -> List[Case]:
    cases = []
    rng = np.random.default_rng(5)
    lits = rng.integers(0, 256, 32768, dtype=np.uint8).tolist()

    toks = lits + [(258, 32768)]
    cases.append(_confirmed("dist32768_len258", fixed_block(BitWriter(), toks).done(), lz_apply(toks)))
    toks = [97, (258, 1)]
    cases.append(_confirmed("dist1_len258", fixed_block(BitWriter(), toks).done(), lz_apply(toks)))

    # every length code and every distance code, extra bits all zeros and all ones
    lens = [(LEN_BASE[i] + ev, (257 + i, LEN_EXTRA[i], ev)) for i in range(29) for ev in {0, (1 << LEN_EXTRA[i]) - 1}]
    dists = [DIST_BASE[i] + ev for i in range(30) for ev in {0, (1 << DIST_EXTRA[i]) - 1}]
    toks = list(lits)
    for k, (length, tok) in enumerate(lens):
        toks.append((length, dists[k % len(dists)], tok))
    for k, d in enumerate(dists):
        toks.append((lens[k % len(lens)][0], d, lens[k % len(lens)][1]))
    assert {t[2][0] for t in toks if not isinstance(t, int)} == set(range(257, 286))
    assert {dist_token(t[1])[0] for t in toks if not isinstance(t, int)} == set(range(30))
    cases.append(_confirmed("all_length_and_distance_codes", fixed_block(BitWriter(), toks).done(), lz_apply(toks)))

    # code-length codes 16 / 17 / 18 that run across the literal / distance boundary
    lit16 = [8] * 192 + [0] * 64 + [4] * 4            # 192/256 + 4/16 = 1
    dist16 = [4] * 16
    cls = rle_lengths(lit16 + dist16)
    at, crossing = 0, False
    for s, ev in cls:
        n = {16: 3 + ev, 17: 3 + ev, 18: 11 + ev}.get(s, 1)
        crossing |= s == 16 and at < len(lit16) < at + n
        at += n
    assert crossing
    toks = list(range(192)) + [(3, 1), (4, 16), (5, 100), (3, 150)]
    cases.append(_confirmed("repeat16_across_boundary", dynamic_block(BitWriter(), lit16, dist16, toks).done(), lz_apply(toks)))
    for name, zeros_lit, zeros_dist in (("repeat17_across_boundary", 2, 2), ("repeat18_across_boundary", 26, 4)):
        n_lit = 286
        used = n_lit - zeros_lit
        lit_l = complete_lengths(used) + [0] * zeros_lit
        assert lit_l[256] != 0
        dist_l = [0] * zeros_dist + [2] * 4
        cls = rle_lengths(lit_l + dist_l)
        assert any(s == (17 if zeros_lit + zeros_dist <= 10 else 18) and ev + (3 if s == 17 else 11) == zeros_lit + zeros_dist
                   for s, ev in cls)
        toks = list(range(200)) + [(3, DIST_BASE[zeros_dist]), (5, DIST_BASE[zeros_dist + 3] + 1)]
        cases.append(_confirmed(name, dynamic_block(BitWriter(), lit_l, dist_l, toks).done(), lz_apply(toks)))

    # 15-bit codes in both alphabets: lengths 1, 2, ..., 14, 15, 15
    lit15 = [0] * 258
    for s, l in zip(list(range(14)) + [256, 257], list(range(1, 15)) + [15, 15]):
        lit15[s] = l
    dist15 = list(range(1, 15)) + [15, 15]
    toks = [s for s in range(14)] * 15 + [(3, DIST_BASE[k]) for k in range(16)] + [13, 12, 13]
    cases.append(_confirmed("codes_of_15_bits", dynamic_block(BitWriter(), lit15, dist15, toks).done(), lz_apply(toks)))

    # one distance code (zlib accepts this incomplete set), and no distance code at all
    lit_s = complete_lengths(260)
    toks = [1, 2, 3, (3, 1), 7, (4, 1)]
    cases.append(_confirmed("single_distance_code", dynamic_block(BitWriter(), lit_s, [1], toks).done(), lz_apply(toks)))
    toks = list(range(256)) * 2
    cases.append(_confirmed("literals_only", dynamic_block(BitWriter(), complete_lengths(257), [0], toks).done(), bytes(toks)))

    # several blocks of all three types, empty stored blocks between them
    w = BitWriter()
    fixed_block(w, [65, 66, 67, (6, 3)], final=False)
    w.bits(0, 3).align().raw(b"\x00\x00\xff\xff")
    w.bits(0, 3).align().raw(b"\x05\x00\xfa\xffhello")
    dynamic_block(w, lit_s, [1], [(5, 1), 9], final=False)
    w.bits(0, 3).align().raw(b"\x00\x00\xff\xff")
    fixed_block(w, [(20, 14)], final=True)
    pay = lz_apply([65, 66, 67, (6, 3)]) + b"hello"
    pay = lz_apply(list(pay) + [(5, 1), 9, (20, 14)])
    cases.append(_confirmed("mixed_blocks", w.done(), pay))
    return cases


# ------------------------------------------------------------------------------------------ malformed input
def text_payload(n: int) -> bytes:
    rng = np.random.default_rng(3)
    words = [b"skeleton", b"vector", b"mask", b"chunk", b"strip", b"zarr", b"tiff", b"wave", b"lane", b"block"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + bytes([32 + int(rng.integers(0, 8))])
    return bytes(out[:n])


def stream300() -> Tuple[bytes, bytes]:
    """A level-6 zlib stream of exactly 300 bytes and its payload."""
    for n in range(400, 4000):
        pay = text_payload(n)
        z = zlib.compress(pay, 6)
        if len(z) == 300:
            return z, pay
    raise AssertionError("no payload gives a 300-byte stream")


def truncations() -> List[Case]:
    z, pay = stream300()
    return [Case(f"cut{k}", z[:k], 1, len(pay), None) for k in range(len(z))]


def bit_flips() -> List[Case]:
    z, pay = stream300()
    out = []
    for bit in range(8 * len(z)):
        m = bytearray(z)
        m[bit >> 3] ^= 1 << (bit & 7)
        m = bytes(m)
        out.append(Case(f"flip{bit}", m, 1, len(pay), oracle(m, 1, len(pay))))
    return out


def _zwrap(raw: bytes, payload: bytes = b"", cmf_flg: bytes = b"\x78\x01", adler: Optional[int] = None) -> bytes:
    a = zlib.adler32(payload) if adler is None else adler
    return cmf_flg + raw + a.to_bytes(4, "big")


def named_errors() -> List[Case]:
    good_pay = text_payload(500)
    good = zlib.compress(good_pay, 6)
    cases = [
        Case("reserved_block_type", _zwrap(BitWriter().bits(1, 1).bits(3, 2).done()), 1, 0, None, E_BLOCK_TYPE),
        Case("len_nlen", _zwrap(BitWriter().bits(1, 3).align().raw(b"\x03\x00\xfc\xfeabc").done(), b"abc"), 1, 3, None, E_STORED),
    ]
    # over-subscribed: three code-length codes of one bit
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for v in (1, 1, 1, 0):
        w.bits(v, 3)
    cases.append(Case("oversubscribed_set", _zwrap(w.bits(0, 32).done()), 1, 0, None, E_CODES))
    # incomplete: one code-length code of two bits
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for v in (2, 0, 0, 0):
        w.bits(v, 3)
    cases.append(Case("incomplete_set", _zwrap(w.bits(0, 32).done()), 1, 0, None, E_CODES))
    w = BitWriter().bits(1, 1).bits(1, 2).code(*fixed_lit(65)).code(*fixed_lit(286)).code(*fixed_lit(256))
    cases.append(Case("symbol_286", _zwrap(w.done(), b"A"), 1, 1, None, E_SYMBOL))
    w = BitWriter().bits(1, 1).bits(1, 2).code(*fixed_lit(65)).code(*fixed_lit(257)).code(30, 5).code(*fixed_lit(256))
    cases.append(Case("distance_code_30", _zwrap(w.done(), b"AAAA"), 1, 4, None, E_SYMBOL))
    w = BitWriter().bits(1, 1).bits(1, 2).code(*fixed_lit(65)).code(*fixed_lit(257)).code(1, 5).code(*fixed_lit(256))
    cases.append(Case("distance_before_output", _zwrap(w.done(), b"AAAA"), 1, 4, None, E_DISTANCE))
    cases.append(Case("expected_one_less", good, 1, len(good_pay) - 1, None, E_LONG))
    cases.append(Case("expected_one_more", good, 1, len(good_pay) + 1, None, E_SHORT))
    bad = good[:-4] + ((int.from_bytes(good[-4:], "big") + 1) & 0xFFFFFFFF).to_bytes(4, "big")
    cases.append(Case("adler_off_by_one", bad, 1, len(good_pay), None, E_ADLER))
    flg = 0x20
    flg += 31 - (0x78 * 256 + flg) % 31
    cases.append(Case("fdict", bytes([0x78, flg]) + good[2:], 1, len(good_pay), None, E_HEADER))
    flg = 31 - (0x77 * 256) % 31
    cases.append(Case("bad_cmf", bytes([0x77, flg]) + good[2:], 1, len(good_pay), None, E_HEADER))
    cases.append(Case("window_too_large", bytes([0x88, 31 - (0x88 * 256) % 31]) + good[2:], 1, len(good_pay), None, E_HEADER))
    cases.append(Case("input_ends_in_trailer", good[:-1], 1, len(good_pay), None, E_INPUT))
    for c in cases:
        assert oracle(c.stream, c.wrapper, c.size) is None, f"{c.name}: zlib accepts it"
    cases.append(Case("good_neighbour", good, 1, len(good_pay), good_pay))
    cases.append(Case("trailing_bytes", good + b"\0\0\0", 1, len(good_pay), good_pay))
    return cases


def good_neighbours() -> List[Case]:
    out = []
    for n, p in ((1000, "period5"), (70000, "random"), (40000, "zero")):
        d = pattern(p, n)
        out.append(Case(f"neighbour_{p}{n}", zlib.compress(d, 6), 1, n, d))
    return out
