// The serial parts of the dynamic Huffman blocks of deflate.hip (RFC 1951 3.2.7), written once and compiled for the
// device (one lane of the piece kernel runs them on tables in LDS) and for the host (sk_deflate_code_host,
// sk_deflate_header_host, and tools/deflate_code_check.cpp under AddressSanitizer / UBSan): code lengths of one
// alphabet under a limit, canonical codes, the run-length coded length sequence, the code-length code and the header's
// bits.  The includer defines SK_DFC_NS (namespace) and SK_DFC_FN (function qualifiers).
//
// Everything here is a function of its inputs alone.  Every array that is indexed by a run-time value lives in a struct
// the caller passes in (DfcWork, DfcHdr), never on the stack: on the device these sit in LDS and nothing goes to scratch.
//
// Code lengths (dfc_lengths).  The used symbols stand in the total order (count, then symbol), ascending
// (dfc_sort here; the device ranks by counting in parallel and gets the same order).  The tree is built with the
// two-queue method: the sorted leaves are one queue, the internal nodes, made in non-decreasing weight, the other; on
// equal weights the leaf is taken first, which gives the flattest of the optimal trees.  Only the NUMBER of leaves at
// each depth is kept.  Depths past the limit are counted at the limit and the counts repaired: while the Kraft sum
// (in units of 2^-limit) exceeds 1, one leaf leaves the limit depth and the deepest leaf above the limit depth is
// replaced by two leaves one level down; every step lowers the sum by one unit, so it ends at exactly 1.  Lengths are
// then dealt out along the order: the rarest symbol gets the longest length.  Without a repair that is an optimal
// code (the multiset of depths is the tree's, and depth is monotone in the order); with one it is complete and within
// the limit.  One used symbol gets the length 1 (the one incomplete code the format allows), none gets no length.
//
// The length sequence (dfc_header_plan): the HLIT literal/length lengths and the HDIST distance lengths as one
// sequence, cut into runs of equal values.  A run of zeros is coded 18 (11..138) while at least 11 remain, then 17
// (3..10), then single zeros; a run of a non-zero length is the length once, then 16 (repeat 3..6) while at least 3
// remain, then the length itself.  16 is used: a block with many literals has long runs of 8s and 9s.
namespace SK_DFC_NS {

constexpr int kDfcLit = 286, kDfcDist = 30, kDfcCl = 19;
constexpr int kDfcSeq = kDfcLit + kDfcDist;
constexpr int kDfcHeaderBytes = 576;            // 17 + 3 * 19 + 316 * (7 + 7) bits at the very most

struct DfcWork {
    uint32_t iw[kDfcLit];                       // weights of the internal nodes, in the order they are made
    uint16_t order[kDfcLit];                    // used symbols by (count, symbol)
    uint16_t lp[kDfcLit], ip[kDfcLit];          // parent (an internal node) of leaf i of the order / of internal node k
    uint16_t bl[16], next[16];                  // leaves per depth; first code per length
};

struct DfcHdr {
    uint32_t cl_freq[kDfcCl];
    uint16_t cl_code[kDfcCl];
    uint8_t cl_len[kDfcCl];
    uint8_t sym[kDfcSeq], extra[kDfcSeq];       // the run-length coded sequence: symbol 0..18 and its extra bits' value
    int nseq, hlit, hdist, hclen;
    unsigned bits;                              // of the whole header, the 3 bits of BFINAL and BTYPE included
};

SK_DFC_FN inline unsigned dfc_rev(unsigned code, int len) {
    unsigned r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// place j of the order in which the code-length code's own lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
SK_DFC_FN inline int dfc_cl_place(int j) {
    if (j < 3) return 16 + j;
    const int k = j - 3;
    return k == 0 ? 0 : ((k & 1) ? 8 + (k - 1) / 2 : 8 - k / 2);
}

// order[0 .. m) = the symbols with freq > 0 by (count, symbol) ascending; returns m
SK_DFC_FN inline int dfc_sort(const uint32_t* freq, int n, uint16_t* order) {
    int m = 0;
    for (int s = 0; s < n; ++s) {
        if (freq[s] == 0) continue;
        int at = m++;
        while (at > 0 && freq[order[at - 1]] > freq[s]) {   // equal counts: the lower symbol stays in front
            order[at] = order[at - 1];
            --at;
        }
        order[at] = (uint16_t)s;
    }
    return m;
}

// len[0 .. n) from freq and w.order[0 .. m); m <= 2^limit, limit <= 15, the counts add up to less than 2^32
SK_DFC_FN inline void dfc_lengths(const uint32_t* freq, int n, int m, int limit, DfcWork& w, uint8_t* len) {
    for (int s = 0; s < n; ++s) len[s] = 0;
    if (m == 0) return;
    if (m == 1) {
        len[w.order[0]] = 1;
        return;
    }
    int li = 0, ii = 0;                          // heads of the two queues
    for (int k = 0; k < m - 1; ++k) {
        uint32_t sum = 0;
        for (int side = 0; side < 2; ++side) {
            const bool leaf = li < m && (ii >= k || freq[w.order[li]] <= w.iw[ii]);
            if (leaf) {
                sum += freq[w.order[li]];
                w.lp[li++] = (uint16_t)k;
            } else {
                sum += w.iw[ii];
                w.ip[ii++] = (uint16_t)k;
            }
        }
        w.iw[k] = sum;
    }
    // depth of every internal node in place of its parent (a parent is made later, so it is turned first)
    w.ip[m - 2] = 0;
    for (int k = m - 3; k >= 0; --k) w.ip[k] = (uint16_t)(w.ip[w.ip[k]] + 1);
    for (int d = 0; d < 16; ++d) w.bl[d] = 0;
    for (int i = 0; i < m; ++i) {
        const int d = w.ip[w.lp[i]] + 1;
        w.bl[d < limit ? d : limit] += 1;
    }
    unsigned total = 0;
    for (int d = 1; d <= limit; ++d) total += (unsigned)w.bl[d] << (limit - d);
    while (total > (1u << limit) && w.bl[limit] > 0) {   // counts of a tree never run out of leaves at the limit
        w.bl[limit] -= 1;
        for (int d = limit - 1; d > 0; --d) {
            if (w.bl[d]) {
                w.bl[d] -= 1;
                w.bl[d + 1] += 2;
                break;
            }
        }
        total -= 1;
    }
    int i = 0;
    for (int d = limit; d >= 1; --d)
        for (int c = w.bl[d]; c > 0 && i < m; --c) len[w.order[i++]] = (uint8_t)d;
}

// canonical codes of RFC 1951 3.2.2, most significant bit first
SK_DFC_FN inline void dfc_codes(const uint8_t* len, int n, DfcWork& w, uint16_t* code) {
    for (int d = 0; d < 16; ++d) w.bl[d] = 0;
    for (int s = 0; s < n; ++s) w.bl[len[s]] += 1;
    w.bl[0] = 0;
    unsigned c = 0;
    w.next[0] = 0;
    for (int d = 1; d < 16; ++d) {
        c = (c + w.bl[d - 1]) << 1;
        w.next[d] = (uint16_t)c;
    }
    for (int s = 0; s < n; ++s) code[s] = len[s] ? w.next[len[s]]++ : (uint16_t)0;
}

SK_DFC_FN inline void dfc_seq_put(DfcHdr& h, int sym, int extra) {
    h.sym[h.nseq] = (uint8_t)sym;
    h.extra[h.nseq] = (uint8_t)extra;
    h.nseq += 1;
    h.cl_freq[sym] += 1;
}
SK_DFC_FN inline int dfc_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }

// the header of a dynamic block for the lengths ll[286] and dl[30] (each 0..15); returns its bits
SK_DFC_FN inline unsigned dfc_header_plan(const uint8_t* ll, const uint8_t* dl, DfcWork& w, DfcHdr& h) {
    int hlit = kDfcLit, hdist = kDfcDist;
    while (hlit > 257 && ll[hlit - 1] == 0) --hlit;
    while (hdist > 1 && dl[hdist - 1] == 0) --hdist;   // no distance code at all: one length of zero
    h.hlit = hlit;
    h.hdist = hdist;
    h.nseq = 0;
    for (int s = 0; s < kDfcCl; ++s) h.cl_freq[s] = 0;
    const int total = hlit + hdist;
    int j = 0;
    while (j < total) {
        const int v = j < hlit ? ll[j] : dl[j - hlit];
        int run = 1;
        while (j + run < total && (j + run < hlit ? ll[j + run] : dl[j + run - hlit]) == v) ++run;
        j += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                dfc_seq_put(h, 18, r - 11);
                run -= r;
            }
            if (run >= 3) {
                dfc_seq_put(h, 17, run - 3);
                run = 0;
            }
        } else {
            dfc_seq_put(h, v, 0);
            run -= 1;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                dfc_seq_put(h, 16, r - 3);
                run -= r;
            }
        }
        for (; run > 0; --run) dfc_seq_put(h, v, 0);
    }
    const int m = dfc_sort(h.cl_freq, kDfcCl, w.order);
    dfc_lengths(h.cl_freq, kDfcCl, m, 7, w, h.cl_len);
    // the code-length code must be complete: next to a single used symbol, one that is never sent takes the other half
    if (m == 1) h.cl_len[w.order[0] == 0 ? 18 : 0] = 1;
    dfc_codes(h.cl_len, kDfcCl, w, h.cl_code);
    int hclen = kDfcCl;
    while (hclen > 4 && h.cl_len[dfc_cl_place(hclen - 1)] == 0) --hclen;
    h.hclen = hclen;
    unsigned bits = 3u + 5u + 5u + 4u + 3u * (unsigned)hclen;
    for (int s = 0; s < kDfcCl; ++s) bits += h.cl_freq[s] * (unsigned)(h.cl_len[s] + dfc_extra_bits(s));
    h.bits = bits;
    return bits;
}

// put(value, bits): the header's bits in stream order, least significant bit of value first
template <class Put>
SK_DFC_FN inline void dfc_header_emit(const DfcHdr& h, int bfinal, Put put) {
    put((bfinal ? 1u : 0u) | (2u << 1), 3);
    put((unsigned)(h.hlit - 257), 5);
    put((unsigned)(h.hdist - 1), 5);
    put((unsigned)(h.hclen - 4), 4);
    for (int j = 0; j < h.hclen; ++j) put((unsigned)h.cl_len[dfc_cl_place(j)], 3);
    for (int i = 0; i < h.nseq; ++i) {
        const int s = h.sym[i], nl = h.cl_len[s];
        put(dfc_rev(h.cl_code[s], nl) | ((unsigned)h.extra[i] << nl), nl + dfc_extra_bits(s));
    }
}

}  // namespace SK_DFC_NS
