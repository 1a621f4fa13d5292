"""A deflate reader for the tests: walks a zlib stream (RFC 1950 / 1951) block by block and keeps what an inflater
throws away -- every block's type, its two code-length arrays, its tokens, its header and payload bits, its byte range
-- next to the re-expanded output.  Pure Python, no dependency; pinned against zlib by tests/test_deflate_reader_cpu.py.

    s = read_zlib(stream)
    s.output                 the inflated bytes
    s.blocks[i].type         "stored" | "fixed" | "dynamic"
    s.blocks[i].final        BFINAL
    s.blocks[i].lit_lengths  286 / 30 code lengths of a dynamic block (as sent, padded with zeros), else None
    s.blocks[i].dist_lengths
    s.blocks[i].hlit, .hdist, .hclen   the counts a dynamic block's header states (HLIT + 257, HDIST + 1, HCLEN + 4)
    s.blocks[i].tokens       literals as int, matches as (length, distance); a stored block has none (see .stored)
    s.blocks[i].stored       the bytes of a stored block, else None
    s.blocks[i].header_bits  BFINAL + BTYPE + (stored: padding to a byte, LEN, NLEN; dynamic: the code lengths)
    s.blocks[i].payload_bits the tokens and the end-of-block symbol, or 8 * len(stored)
    s.blocks[i].start_bit, .end_bit    in bits from the start of the stream (the zlib header is bits 0..15)
    s.blocks[i].byte_range   (first byte, one past the last byte) the block's bits touch
    s.pad_bits               bits between the last block and the Adler-32
    16 + sum(header_bits + payload_bits) + pad_bits + 32 == 8 * len(stream)
"""
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class Block:
    def __init__(self):
        self.type = None
        self.final = False
        self.lit_lengths = self.dist_lengths = self.stored = None
        self.hlit = self.hdist = self.hclen = None
        self.tokens = []
        self.header_bits = self.payload_bits = 0
        self.start_bit = self.end_bit = 0

    @property
    def byte_range(self):
        return self.start_bit // 8, (self.end_bit + 7) // 8


class Stream:
    def __init__(self):
        self.blocks = []
        self.output = b""
        self.pad_bits = 0


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol (most significant bit first), 0 for an unused one."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def _table(lengths, what):
    """{(length, code): symbol}; refuses an over-subscribed set, and an incomplete one unless it is one code of 1 bit
    (what zlib accepts for the literal / length and the distance alphabet) or has no code at all (distance only)."""
    kraft = sum(1 << (15 - n) for n in lengths if n)
    used = sum(1 for n in lengths if n)
    if kraft > 1 << 15:
        raise ValueError(f"over-subscribed {what} code")
    if kraft < 1 << 15 and not (what != "code-length" and (used == 0 or (used == 1 and max(lengths) == 1))):
        raise ValueError(f"incomplete {what} code")
    # keyed by (length, code as it stands in the stream: first bit read = lowest bit); None -> the lengths in use
    table = {(n, int(format(c, f"0{n}b")[::-1], 2)): s
             for s, (n, c) in enumerate(zip(lengths, canonical_codes(lengths))) if n}
    table[None] = sorted({n for n in lengths if n})
    return table


_FIXED = None


class _Bits:
    def __init__(self, data, pos):
        self.data, self.pos = data, pos   # pos in bits
        self.end = 8 * len(data)

    def take(self, n):
        if self.pos + n > self.end:
            raise ValueError("input exhausted")
        p, v = self.pos, 0
        first = p >> 3
        chunk = int.from_bytes(self.data[first:first + 4], "little")
        v = (chunk >> (p & 7)) & ((1 << n) - 1)
        self.pos = p + n
        return v

    def symbol(self, table):
        p = self.pos
        first = p >> 3
        v = int.from_bytes(self.data[first:first + 3], "little") >> (p & 7)   # the next 15 bits at least, zeros past the end
        for n in table[None]:
            s = table.get((n, v & ((1 << n) - 1)))
            if s is not None:
                if p + n > self.end:
                    raise ValueError("input exhausted")
                self.pos = p + n
                return s
        raise ValueError("invalid code" if p + 15 <= self.end else "input exhausted")


def read_deflate(data, bit_pos=0):
    """The blocks of the raw deflate data that starts at bit ``bit_pos`` of ``data`` -> (blocks, output, end bit)."""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table(FIXED_LIT, "literal"), _table(FIXED_DIST + [5, 5], "distance"))   # 288 / 32 codes, the last unused
    b = _Bits(data, bit_pos)
    out = bytearray()
    blocks = []
    while True:
        blk = Block()
        blk.start_bit = b.pos
        blk.final = bool(b.take(1))
        btype = b.take(2)
        if btype == 3:
            raise ValueError("reserved block type")
        if btype == 0:
            blk.type = "stored"
            b.pos = (b.pos + 7) & ~7
            n, nn = b.take(16), b.take(16)
            if n != (~nn & 0xFFFF):
                raise ValueError("stored block whose LEN and NLEN do not match")
            blk.header_bits = b.pos - blk.start_bit
            first = b.pos >> 3
            if first + n > len(data):
                raise ValueError("input exhausted")
            blk.stored = bytes(data[first:first + n])
            out += blk.stored
            b.pos += 8 * n
            blk.payload_bits = 8 * n
        else:
            if btype == 1:
                blk.type = "fixed"
                lit, dist = _FIXED
            else:
                blk.type = "dynamic"
                blk.hlit, blk.hdist, blk.hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                if blk.hlit > 286 or blk.hdist > 30:
                    raise ValueError("too many length or distance symbols")
                cl = [0] * 19
                for j in range(blk.hclen):
                    cl[CL_ORDER[j]] = b.take(3)
                cl_table = _table(cl, "code-length")
                seq = []
                while len(seq) < blk.hlit + blk.hdist:
                    s = b.symbol(cl_table)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        if not seq:
                            raise ValueError("repeat with no previous length")
                        seq += [seq[-1]] * (3 + b.take(2))
                    elif s == 17:
                        seq += [0] * (3 + b.take(3))
                    else:
                        seq += [0] * (11 + b.take(7))
                if len(seq) > blk.hlit + blk.hdist:
                    raise ValueError("repeat past the last length")
                blk.lit_lengths = seq[:blk.hlit] + [0] * (286 - blk.hlit)
                blk.dist_lengths = seq[blk.hlit:] + [0] * (30 - blk.hdist)
                if blk.lit_lengths[256] == 0:
                    raise ValueError("no end-of-block code")
                lit, dist = _table(blk.lit_lengths, "literal"), _table(blk.dist_lengths, "distance")
            blk.header_bits = b.pos - blk.start_bit
            tokens = blk.tokens
            while True:
                s = b.symbol(lit)
                if s < 256:
                    tokens.append(s)
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("invalid length symbol")
                    length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    d = b.symbol(dist)
                    if d > 29:
                        raise ValueError("invalid distance symbol")
                    distance = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                    if distance > len(out):
                        raise ValueError("distance before the start of the output")
                    tokens.append((length, distance))
                    if distance >= length:
                        out += out[len(out) - distance:len(out) - distance + length]
                    else:
                        for _ in range(length):
                            out.append(out[-distance])
            blk.payload_bits = b.pos - blk.start_bit - blk.header_bits
        blk.end_bit = b.pos
        blocks.append(blk)
        if blk.final:
            return blocks, bytes(out), b.pos


def read_zlib(stream):
    """A whole zlib stream -> Stream; ValueError if it is malformed, has bytes left over or a wrong Adler-32."""
    stream = bytes(stream)
    if len(stream) < 6 or (stream[0] & 15) != 8 or (stream[0] >> 4) > 7 or ((stream[0] << 8) | stream[1]) % 31 or \
            stream[1] & 32:
        raise ValueError("bad or unsupported zlib header")
    s = Stream()
    s.blocks, s.output, end = read_deflate(stream, 16)
    tail = (end + 7) // 8
    s.pad_bits = 8 * tail - end
    if len(stream) != tail + 4:
        raise ValueError(f"{len(stream) - tail - 4} bytes beyond the Adler-32")
    if int.from_bytes(stream[tail:], "big") != zlib.adler32(s.output):
        raise ValueError("Adler-32 mismatch")
    return s


def symbol_of_length(length):
    """(literal/length symbol, extra bits) of a match length 3..258."""
    for k in range(28, -1, -1):
        if length >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k]
    raise ValueError(length)


def symbol_of_distance(distance):
    """(distance symbol, extra bits) of a distance 1..32768."""
    for k in range(29, -1, -1):
        if distance >= DIST_BASE[k]:
            return k, DIST_EXTRA[k]
    raise ValueError(distance)


def histogram(tokens):
    """(286 literal / length counts with the end-of-block symbol counted once, 30 distance counts, extra bits)."""
    lit, dist, extra = [0] * 286, [0] * 30, 0
    lit[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            s, e = symbol_of_length(t[0])
            d, f = symbol_of_distance(t[1])
            lit[s] += 1
            dist[d] += 1
            extra += e + f
        else:
            lit[t] += 1
    return lit, dist, extra
