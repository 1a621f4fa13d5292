"""The code builder of the dynamic Huffman blocks (skoots_amd/csrc/deflate_code.inc), run on the CPU through
sk_deflate_code_host and sk_deflate_header_host: the same text the piece kernel runs on its LDS tables.  The reference
is a heapq Huffman in this file: the optimal cost is unique even where the lengths are not."""
import heapq
import math

import numpy as np
import pytest

from tests import deflate_reader as R


def code_host(freq, limit):
    from skoots_amd import _ffi
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lengths = np.full(len(f), 255, np.uint8)
    codes = np.full(len(f), 65535, np.uint16)
    _ffi.check(_ffi.lib.sk_deflate_code_host(f.ctypes.data, len(f), limit, lengths.ctypes.data, codes.ctypes.data))
    return lengths.tolist(), codes.tolist()


def header_host(lit, dist, bfinal=0):
    from skoots_amd import _ffi
    a, b = np.ascontiguousarray(lit, dtype=np.uint8), np.ascontiguousarray(dist, dtype=np.uint8)
    assert len(a) == 286 and len(b) == 30
    out = np.full(576, 255, np.uint8)
    bits = np.zeros(1, np.int64)
    _ffi.check(_ffi.lib.sk_deflate_header_host(a.ctypes.data, b.ctypes.data, bfinal, out.ctypes.data, 576,
                                               bits.ctypes.data))
    return out.tobytes(), int(bits[0])


def huffman_optimum(freq):
    """(cost, depth) of an optimal prefix code of the used symbols: sum of count * length, and the smallest possible
    longest length among optimal codes (ties: the shallower subtree first)."""
    heap = [(f, 0) for f in freq if f]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def kraft(lengths, limit):
    return sum(1 << (limit - n) for n in lengths if n), 1 << limit


def _check(freq, limit):
    lengths, codes = code_host(freq, limit)
    used = [s for s, f in enumerate(freq) if f]
    assert all((lengths[s] > 0) == (freq[s] > 0) for s in range(len(freq)))
    assert max(lengths) <= limit
    assert codes == R.canonical_codes(lengths)   # RFC 1951 3.2.2, computed from the lengths in Python
    cost = sum(f * n for f, n in zip(freq, lengths))
    if len(used) >= 2:
        k, one = kraft(lengths, limit)
        assert k == one
        best, depth = huffman_optimum(freq)
        if depth <= limit:
            assert cost == best
        else:
            assert cost > best
    return lengths, cost


def test_abi():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 30


@pytest.mark.parametrize("seed", range(40))
def test_random_histograms_are_coded_optimally(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 287))
    kind = seed % 4
    if kind == 0:
        freq = rng.integers(0, 50, n)
    elif kind == 1:
        freq = rng.integers(1, 16384 // n + 2, n)
    elif kind == 2:
        freq = (rng.pareto(1.0, n) * 3).astype(np.int64) % 5000
    else:
        freq = rng.integers(0, 3, n) * rng.integers(1, 400, n)
    freq = [int(v) for v in freq]
    if sum(1 for v in freq if v) < 2:
        freq[0], freq[-1] = 3, 1
    _check(freq, 15)
    if n <= 19:
        _check(freq, 7)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@pytest.mark.parametrize("n, limit", [(17, 15), (20, 15), (24, 15), (19, 7), (12, 7)])
def test_depth_beyond_the_limit_is_repaired(n, limit):
    """Fibonacci counts 1, 1, 2, 3, ... make the deepest optimal tree: n symbols give depth n - 1.  17 symbols add up to
    4180, so a 16 KiB piece can hold such a histogram; 19 symbols under the limit 7 are the code-length alphabet's case."""
    freq = _fib(n)
    if n == 17:
        assert sum(freq) < 16384
    assert huffman_optimum(freq)[1] > limit
    for order in (freq, freq[::-1]):
        lengths, cost = _check(order, limit)
        flat = math.ceil(math.log2(n))
        assert cost <= sum(order) * flat


def test_edge_histograms():
    # one used symbol: the one incomplete code the format allows
    lengths, codes = code_host([0, 0, 7, 0], 15)
    assert lengths == [0, 0, 1, 0] and codes == [0, 0, 0, 0]
    # none: no length (the distance alphabet of a piece without a match)
    assert code_host([0] * 30, 15)[0] == [0] * 30
    # one distance symbol: one length of 1
    assert code_host([0] * 4 + [9] + [0] * 25, 15)[0] == [0] * 4 + [1] + [0] * 25
    # two used symbols
    lengths, codes = code_host([5, 0, 0, 1], 15)
    assert lengths == [1, 0, 0, 1] and codes == [0, 0, 0, 1]
    # all 286 used with equal counts: 226 codes of 8 bits and 60 of 9 would not be canonical by symbol alone; the order
    # (count, symbol) gives the longer lengths to the lower symbols
    lengths, _ = _check([3] * 286, 15)
    assert sorted(set(lengths)) == [8, 9] and lengths.count(9) == 2 * (286 - 256)
    assert lengths[:60] == [9] * 60
    # ties are broken by symbol: the same counts permuted give the permuted lengths' multiset and the same cost
    a, ca = _check([4, 4, 4, 1, 1, 2], 15)
    b, cb = _check([1, 2, 4, 4, 1, 4], 15)
    assert sorted(a) == sorted(b) and ca == cb


def test_refusals():
    from skoots_amd import _ffi
    f = np.ones(300, np.uint32)
    lengths, codes = np.zeros(300, np.uint8), np.zeros(300, np.uint16)
    for n, limit, what in ((0, 15, "n_symbols"), (287, 15, "n_symbols"), (10, 16, "limit"), (10, 0, "limit"),
                           (19, 4, "do not fit")):
        with pytest.raises(ValueError, match=what):
            _ffi.check(_ffi.lib.sk_deflate_code_host(f.ctypes.data, n, limit, lengths.ctypes.data, codes.ctypes.data))
    big = np.full(4, 2 ** 31, np.uint32)
    with pytest.raises(ValueError, match="add up"):
        _ffi.check(_ffi.lib.sk_deflate_code_host(big.ctypes.data, 4, 15, lengths.ctypes.data, codes.ctypes.data))
    bad = np.zeros(286, np.uint8)
    bad[3] = 16
    out, bits = np.zeros(576, np.uint8), np.zeros(1, np.int64)
    with pytest.raises(ValueError, match="above 15"):
        _ffi.check(_ffi.lib.sk_deflate_header_host(bad.ctypes.data, np.zeros(30, np.uint8).ctypes.data, 0,
                                                   out.ctypes.data, 576, bits.ctypes.data))


def _header_cases():
    rng = np.random.default_rng(5)
    cases = []
    for seed in range(12):
        n = int(rng.integers(2, 257))
        lit = [0] * 286
        for s in rng.choice(256, n, replace=False):
            lit[int(s)] = int(rng.integers(1, 3000))
        lit[256] = 1
        for s in range(257, 257 + int(rng.integers(0, 30))):
            lit[s] = int(rng.integers(0, 200))
        dist = [int(v) for v in rng.integers(0, 100, 30) * (rng.random(30) < 0.4)]
        cases.append((lit, dist))
    two = [0] * 286
    two[0], two[128], two[256] = 9000, 7000, 1
    cases.append((two, [0] * 30))                 # two literals, no match: about 280 zero lengths, HDIST = 1
    cases.append((two, [0] * 3 + [40] + [0] * 26))   # one distance symbol
    cases.append(([1] * 286, [1] * 30))           # everything used
    return cases


@pytest.mark.parametrize("case", range(15))
def test_header_gives_both_length_arrays_back(case):
    lit_freq, dist_freq = _header_cases()[case]
    lit, dist = code_host(lit_freq, 15)[0], code_host(dist_freq, 15)[0]
    for bfinal in (0, 1):
        head, bits = header_host(lit, dist, bfinal)
        assert all(v == 0 for v in head[(bits + 7) // 8:]) and (bits % 8 == 0 or head[bits // 8] >> (bits % 8) == 0)
        # the reader needs a whole block: the end-of-block code follows the header, and BFINAL ends the walk
        eob = R.canonical_codes(lit)[256]
        stream = bytearray(head[:(bits + lit[256] + 7) // 8 + 1])
        for k in range(lit[256]):
            bit = (eob >> (lit[256] - 1 - k)) & 1
            stream[(bits + k) // 8] |= bit << ((bits + k) % 8)
        if not bfinal:
            stream[0] |= 1
        blocks, out, end = R.read_deflate(bytes(stream))
        assert out == b"" and len(blocks) == 1 and end == bits + lit[256]
        b = blocks[0]
        assert b.type == "dynamic" and b.header_bits == bits
        assert b.lit_lengths == lit and b.dist_lengths == dist
        used = [s for s, n in enumerate(dist) if n]
        assert b.hdist == (used[-1] + 1 if used else 1)
        assert b.hlit == max(257, max(s for s, n in enumerate(lit) if n) + 1)
    if case == 12:
        assert dist == [0] * 30 and bits < 200      # 17 / 18 runs: the zero lengths cost a few symbols, not 280
    if case == 13:
        assert dist == [0, 0, 0, 1] + [0] * 26
