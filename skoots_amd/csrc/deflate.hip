// Deflate encoder for the arrays eval() writes: every output is one complete zlib stream (RFC 1950: 78 01, RFC 1951
// blocks, Adler-32 big-endian) that any zarr / TIFF reader inflates.  Replaces the host's zlib.compress(raw, 1) per
// chunk (skoots_amd/lib/zarr_store.py) and Pillow's tiff_adobe_deflate per page for data that already sits in HBM.
// No reference counterpart (the reference hands its arrays to zarr / skimage on the host, eval.py:101-111, 309-310).
//
// Parallelism inside one stream is the pigz construction: the input is cut into pieces of kDfPiece bytes that are
// encoded independently, every piece but the last ends with an empty stored block (00 00 FF FF after padding to a
// byte), so that pieces are byte-aligned and a stream is the concatenation of its pieces; Adler-32 is computed per
// piece and combined.  Four launches, all stream-ordered:
//   deflate_piece_kernel    one workgroup per piece: match search, parse, Huffman bits -> the piece's slot
//   deflate_stream_kernel   one workgroup per stream: prefix sum of its pieces' sizes, Adler-32 combine, all-zero flag
//   deflate_offsets_kernel  one workgroup: prefix sum of the stream sizes -> dst_offsets
//   deflate_compact_kernel  one workgroup per piece: slot -> its place in dst, stream header and trailer
//
// The piece kernel, thread t owning bytes [64 t, 64 t + 64) of the piece:
//   (a) match search.  Candidate distances are 1 and k * elem_bytes for k = 1..64: on these arrays a repeat is the
//       previous element or the previous Z row (64 elements in the stores' chunks), not something a hash of the last
//       32 KiB finds better.  Per distance every thread builds the 64-bit word "byte i equals byte i - d" for its own
//       bytes (16 word compares against the shifted LDS image), the words go to LDS, and the run of ones from bit i --
//       the match length at i -- comes from one walk down the thread's own word plus the run that continues in the
//       following words.  The best (length, nearer distance) per position is a max over packed integers.
//   (b) greedy parse without a serial walk: next[i] = i + max(1, len[i]); the positions reachable from 0 are marked by
//       pointer jumping (mark what the marked reach in 2^k hops, square the jump table), log2(tokens) rounds.
//   (c) bits per token -> block scan -> every token ORs its bits into the LDS image of the output (atomicOr: the
//       result does not depend on the order).  Huffman codes most-significant bit first, extra bits least first.
//   (d) end of block, the aligning stored block; a piece whose encoding would be longer than storing it is stored.
// Nothing depends on the order in which atomics land (OR into words, monotone marks, integer counters), so the bytes
// are the same on every run and for every batching.
//
// Dynamic codes (deflate_piece_kernel<true>, sk_deflate_streams_coded with huffman = 1).  Parse, (a), (b), the Adler sums
// and the all-zero flag are the same text.  After (b): (i) the tokens are counted into 286 + 30 LDS counters; (ii) the
// used symbols are ranked by (count, symbol) by counting, and one lane runs the serial text of deflate_code.inc on the
// tables in LDS: two-queue merge, limit 15 with its repair, canonical codes, the run-length coded length sequence, the
// code-length code; (iii) one walk gives every token's bits under both codes; (iv) the piece is written in the form
// with the fewest bytes -- stored, fixed, dynamic in that order on equal bytes -- by the same phase (c), the codes
// read from an LDS table.  A minimum over forms that include "stored" keeps sk_deflate_bound as it is.
#include "common.h"

#define SK_DFC_NS sk_dfc
#define SK_DFC_FN __host__ __device__
#include "deflate_code.inc"
#undef SK_DFC_NS
#undef SK_DFC_FN

namespace sk {

constexpr int kDfPiece = 16384;                 // bytes of input per workgroup
constexpr int kDfBlock = 256;
constexpr int kDfPer = kDfPiece / kDfBlock;     // 64 bytes = one 64-bit mask word per thread
constexpr int kDfWords = kDfPiece / 4;
constexpr int kDfCand = 64;                     // multiples of elem_bytes tried as distances (plus distance 1)
constexpr int kDfGroup = 4;                     // distances per round (LDS for the mask words)
constexpr int kDfRounds = (kDfCand + 1 + kDfGroup - 1) / kDfGroup;
constexpr int kDfMaxLen = 258;
constexpr int kDfSlot = kDfPiece + 32;          // workspace bytes per piece
constexpr int kDfStoredOff = 11;                // a stored piece's 5 header bytes end where its 16-byte aligned data begin
constexpr int kDfMeta = 8;                      // uint32 per piece: bytes, offset in slot, sum, weighted sum, nonzero
constexpr unsigned kAdlerMod = 65521u;
constexpr int kDfSyms = sk_dfc::kDfcSeq;         // 286 literal / length symbols, then the 30 distance symbols
static_assert(kDfPer == 64, "one mask word per thread");

static inline int64_t df_pieces(int64_t stream_bytes) {
    return stream_bytes <= 0 ? 1 : (stream_bytes + kDfPiece - 1) / kDfPiece;
}

// tables of a piece's dynamic code; they live where eq[] was, which is dead after the match search
struct DfDyn {
    unsigned freq[kDfSyms];                                  // token histogram
    unsigned tab[kDfSyms];                                   // bit-reversed code | length << 16
    unsigned short code[kDfSyms];
    uint8_t len[kDfSyms];
    unsigned short dorder[sk_dfc::kDfcDist];                 // used distance symbols by (count, symbol)
    int used[2];
    sk_dfc::DfcWork work;
    sk_dfc::DfcHdr hdr;
};

struct DfLds {
    unsigned data[kDfWords + kDfWords / 16];                 // word w at w + (w >> 4): a thread's 16 words, stride 17
    union {
        unsigned long long eq[kDfGroup][kDfBlock + 8];       // words past the piece stay zero
        DfDyn dyn;
    };
    unsigned long long marks[kDfBlock];
    unsigned red[32];
    union {
        unsigned short jump[kDfPiece];                       // position 64 t + k at k * 256 + t
        unsigned out[(kDfPiece + 64) / 4];
    };
};

__device__ inline int df_sw(int w) { return w + (w >> 4); }
__device__ inline int df_dist(int c, int e) { return c == 0 ? 1 : (c <= kDfCand ? c * e : 0); }
__device__ inline unsigned df_rev(unsigned code, int len) { return __brev(code) >> (32 - len); }

// literal / length symbol of the fixed code (RFC 1951 3.2.6), bit-reversed for an LSB-first stream
__device__ inline void df_sym(int sym, unsigned& code, int& nb) {
    if (sym < 144) { code = 0x30u + sym; nb = 8; }
    else if (sym < 256) { code = 0x190u + (sym - 144); nb = 9; }
    else if (sym < 280) { code = sym - 256; nb = 7; }
    else { code = 0xC0u + (sym - 280); nb = 8; }
    code = df_rev(code, nb);
}
// length 3..258 -> symbol 257..285, its extra bits and their value
__device__ inline void df_len_sym(int len, int& sym, int& eb, unsigned& extra) {
    const int l = len - 3;
    eb = 0;
    extra = 0;
    if (len == kDfMaxLen) sym = 285;
    else if (l < 8) sym = 257 + l;
    else {
        eb = (31 - __clz(l)) - 2;
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        extra = l & ((1u << eb) - 1);
    }
}
// distance 1..32768 -> symbol 0..29, its extra bits and their value
__device__ inline void df_dist_sym(int d, int& code, int& eb, unsigned& extra) {
    const int dd = d - 1;
    code = dd;
    eb = 0;
    extra = 0;
    if (dd >= 4) {
        eb = (31 - __clz(dd)) - 1;
        code = 2 * eb + 2 + ((dd >> eb) & 1);
        extra = dd & ((1u << eb) - 1);
    }
}
__device__ inline void df_len_bits(int len, unsigned& bits, int& nb) {
    int sym, eb;
    unsigned extra;
    df_len_sym(len, sym, eb, extra);
    unsigned code;
    df_sym(sym, code, nb);
    bits = code | (extra << nb);
    nb += eb;
}
__device__ inline void df_dist_bits(int d, unsigned& bits, int& nb) {
    int code, eb;
    unsigned extra;
    df_dist_sym(d, code, eb, extra);
    bits = df_rev(code, 5) | (extra << 5);
    nb = 5 + eb;
}
// 4 bits: byte j of x is zero
__device__ inline unsigned df_zero_bytes(unsigned x) {
    const unsigned nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    const unsigned y = (nz ^ 0x80808080u) >> 7;
    return (y | (y >> 7) | (y >> 14) | (y >> 21)) & 15u;
}
__device__ inline void df_put(unsigned* out, unsigned off, unsigned val, int nb) {
    const unsigned long long v = (unsigned long long)val << (off & 31);
    atomicOr(&out[off >> 5], (unsigned)v);
    if (v >> 32) atomicOr(&out[(off >> 5) + 1], (unsigned)(v >> 32));
}
// bits of the token that starts at a marked position: packed best = (len << 7) | (127 - candidate)
__device__ inline void df_token(unsigned best, unsigned byte, int e, unsigned& b0, int& n0, unsigned& b1, int& n1) {
    const int len = (int)(best >> 7);
    if (len >= 3) {
        df_len_bits(len, b0, n0);
        df_dist_bits(df_dist(127 - (int)(best & 127u), e), b1, n1);
    } else {
        df_sym((int)byte, b0, n0);
        b1 = 0;
        n1 = 0;
    }
}
// the same token under the piece's own code: codes and lengths come from tab[]
__device__ inline void df_token_dyn(unsigned best, unsigned byte, int e, const unsigned* tab, unsigned& b0, int& n0,
                                    unsigned& b1, int& n1) {
    const int len = (int)(best >> 7);
    if (len >= 3) {
        int sym, eb;
        unsigned extra;
        df_len_sym(len, sym, eb, extra);
        unsigned ent = tab[sym];
        int nl = (int)(ent >> 16);
        b0 = (ent & 0xffffu) | (extra << nl);
        n0 = nl + eb;
        df_dist_sym(df_dist(127 - (int)(best & 127u), e), sym, eb, extra);
        ent = tab[sk_dfc::kDfcLit + sym];
        nl = (int)(ent >> 16);
        b1 = (ent & 0xffffu) | (extra << nl);
        n1 = nl + eb;
    } else {
        const unsigned ent = tab[byte];
        b0 = ent & 0xffffu;
        n0 = (int)(ent >> 16);
        b1 = 0;
        n1 = 0;
    }
}

// kDyn = false: every piece is coded with the fixed code or stored.  kDyn = true: the piece's own code is built as
// well and the smallest of stored, fixed and dynamic is written.
template <bool kDyn>
__global__ __launch_bounds__(kDfBlock, 2) void deflate_piece_kernel(const uint8_t* __restrict__ src, const int64_t L,
                                                                    const int64_t pps, const int e,
                                                                    uint8_t* __restrict__ slots,
                                                                    unsigned* __restrict__ meta) {
    __shared__ DfLds s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t piece = blockIdx.x;
    const int64_t strm = piece / pps, p = piece - strm * pps;
    const int64_t start = p * kDfPiece;
    const int n = (int)(L - start < kDfPiece ? L - start : kDfPiece);
    const bool last = p == pps - 1;
    const uint8_t* x = src + strm * L + start;
    const int base = t * kDfPer;

    // ---- load: 64 bytes per thread, zero past the piece
    unsigned own[16];
    if ((((uintptr_t)x) & 15) == 0 && base + kDfPer <= n) {
        const uint4* xv = (const uint4*)(x + base);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 v = xv[j];
            own[4 * j] = v.x; own[4 * j + 1] = v.y; own[4 * j + 2] = v.z; own[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            unsigned w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int pos = base + 4 * j + b;
                if (pos < n) w |= (unsigned)x[pos] << (8 * b);
            }
            own[j] = w;
        }
    }
    unsigned sa = 0, sb = 0, nz = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        s.data[df_sw(16 * t + j)] = own[j];
        nz |= own[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned v = (own[j] >> (8 * b)) & 255u;
            sa += v;
            sb += v * (unsigned)(n - (base + 4 * j + b));   // v is 0 past n; at most 64 * 255 * 16384 < 2^32
        }
    }
    sb %= kAdlerMod;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o);
        sb += __shfl_xor(sb, o);
        nz |= __shfl_xor(nz, o);
    }
    if (lane == 0) {
        s.red[wave] = sa;          // at most 16384 * 255
        s.red[4 + wave] = sb;      // at most 64 * 65520
        s.red[8 + wave] = nz;
    }
    if (t < kDfGroup * 8) s.eq[t >> 3][kDfBlock + (t & 7)] = 0;
    const int left = n - base;
    const unsigned long long vn = left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1));
    unsigned best[kDfPer];
#pragma unroll
    for (int k = 0; k < kDfPer; ++k) best[k] = 0;
    __syncthreads();

    // ---- (a) match search
    for (int r = 0; r < kDfRounds; ++r) {
        unsigned long long my[kDfGroup];
#pragma unroll
        for (int gi = 0; gi < kDfGroup; ++gi) {
            const int d = df_dist(r * kDfGroup + gi, e);
            unsigned long long m = 0;
            if (d > 0) {
                const int sh = base - d;            // first byte of the shifted window; negative before the piece
                const int q0 = sh >> 2, rb = (sh & 3) * 8;
                unsigned lo = s.data[df_sw(q0 < 0 ? 0 : q0)];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    int q = q0 + j + 1;
                    q = q < 0 ? 0 : (q > kDfWords - 1 ? kDfWords - 1 : q);
                    const unsigned hi = s.data[df_sw(q)];
                    const unsigned shifted = (unsigned)(((((unsigned long long)hi) << 32) | lo) >> rb);
                    m |= (unsigned long long)df_zero_bytes(own[j] ^ shifted) << (4 * j);
                    lo = hi;
                }
                const int before = d - base;        // positions whose partner lies before the piece
                if (before > 0) m &= before >= 64 ? 0ull : ~((1ull << before) - 1);
                m &= vn;
            }
            my[gi] = m;
            s.eq[gi][t] = m;
        }
        __syncthreads();
#pragma unroll
        for (int gi = 0; gi < kDfGroup; ++gi) {
            // run of ones that continues past this thread's word; exact below 258, a lower bound >= 258 otherwise
            int run = 0;
            for (int idx = t + 1; run < kDfMaxLen; ++idx) {
                const unsigned long long w = ~s.eq[gi][idx];
                if (w != 0) {
                    run += __builtin_ctzll(w);
                    break;
                }
                run += 64;
            }
            const unsigned tag = 127u - (unsigned)(r * kDfGroup + gi);
            const unsigned long long m = my[gi];
#pragma unroll
            for (int k = kDfPer - 1; k >= 0; --k) {
                run = ((m >> k) & 1ull) ? run + 1 : 0;
                const unsigned len = (unsigned)(run < kDfMaxLen ? run : kDfMaxLen);
                const unsigned cand = (len << 7) | tag;
                best[k] = best[k] > cand ? best[k] : cand;
            }
        }
        __syncthreads();
    }

    // ---- (b) greedy parse: next[], then the positions reachable from 0
#pragma unroll
    for (int k = 0; k < kDfPer; ++k) {
        const int pos = base + k;
        const int len = (int)(best[k] >> 7);
        int nx = pos + (len >= 3 ? len : 1);
        if (pos >= n || nx > n) nx = n;
        s.jump[k * kDfBlock + t] = (unsigned short)nx;
    }
    s.marks[t] = (t == 0 && n > 0) ? 1ull : 0ull;
    if constexpr (kDyn) {   // eq[] is behind the last barrier of (a)
        for (int i = t; i < kDfSyms; i += kDfBlock) s.dyn.freq[i] = i == 256 ? 1u : 0u;   // end of block counts once
        if (t < 2) s.dyn.used[t] = 0;
    }
    __syncthreads();
    while ((int)s.jump[0] < n) {   // level k: everything within 2^k - 1 hops of 0 is marked, jump = next^(2^k)
        const unsigned long long m = s.marks[t];
        unsigned short nxt[kDfPer];
#pragma unroll
        for (int k = 0; k < kDfPer; ++k) {
            const int J = s.jump[k * kDfBlock + t];
            int JJ = n;
            if (J < n) {
                JJ = s.jump[(J & 63) * kDfBlock + (J >> 6)];
                if ((m >> k) & 1ull) atomicOr((unsigned*)s.marks + (J >> 5), 1u << (J & 31));
            }
            nxt[k] = (unsigned short)JJ;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kDfPer; ++k) s.jump[k * kDfBlock + t] = nxt[k];
        __syncthreads();
    }

    // ---- (c) bits per token, block scan
    const unsigned long long marked = s.marks[t];
    if constexpr (kDyn) {
        DfDyn& y = s.dyn;
        // (i) histogram of the tokens.  A thread keeps the two symbols it saw last in registers, so that a piece made of
        // two literals costs two adds per thread; integer adds, so the counts do not depend on the order.
        int ca = -1, cb = -1;
        unsigned na = 0, nb = 0;
#pragma unroll
        for (int k = 0; k < kDfPer; ++k) {
            if ((marked >> k) & 1ull) {
                const int len = (int)(best[k] >> 7);
                int sym = (int)((own[k >> 2] >> (8 * (k & 3))) & 255u);
                if (len >= 3) {
                    int dsym, eb;
                    unsigned extra;
                    df_len_sym(len, sym, eb, extra);
                    df_dist_sym(df_dist(127 - (int)(best[k] & 127u), e), dsym, eb, extra);
                    atomicAdd(&y.freq[sk_dfc::kDfcLit + dsym], 1u);
                }
                if (sym == cb) ++nb;
                else if (sym == ca) ++na;
                else {
                    if (na) atomicAdd(&y.freq[ca], na);
                    ca = cb;
                    na = nb;
                    cb = sym;
                    nb = 1;
                }
            }
        }
        if (na) atomicAdd(&y.freq[ca], na);
        if (nb) atomicAdd(&y.freq[cb], nb);
        __syncthreads();
        // (ii) the used symbols of either alphabet in the order (count, symbol): rank by counting
        for (int i = t; i < kDfSyms; i += kDfBlock) {
            const unsigned f = y.freq[i];
            if (f) {
                const bool dist = i >= sk_dfc::kDfcLit;
                const int lo = dist ? sk_dfc::kDfcLit : 0, hi = dist ? kDfSyms : sk_dfc::kDfcLit;
                int r = 0;
                for (int j = lo; j < hi; ++j) {
                    const unsigned g = y.freq[j];
                    r += (g != 0 && (g < f || (g == f && j < i))) ? 1 : 0;
                }
                if (dist) y.dorder[r] = (unsigned short)(i - sk_dfc::kDfcLit);
                else y.work.order[r] = (unsigned short)i;
                atomicAdd(&y.used[dist ? 1 : 0], 1);
            }
        }
        __syncthreads();
        if (t == 0) {   // the serial parts: deflate_code.inc
            sk_dfc::dfc_lengths(y.freq, sk_dfc::kDfcLit, y.used[0], 15, y.work, y.len);
            sk_dfc::dfc_codes(y.len, sk_dfc::kDfcLit, y.work, y.code);
            const int md = y.used[1];
            for (int i = 0; i < md; ++i) y.work.order[i] = y.dorder[i];
            sk_dfc::dfc_lengths(y.freq + sk_dfc::kDfcLit, sk_dfc::kDfcDist, md, 15, y.work, y.len + sk_dfc::kDfcLit);
            sk_dfc::dfc_codes(y.len + sk_dfc::kDfcLit, sk_dfc::kDfcDist, y.work, y.code + sk_dfc::kDfcLit);
            sk_dfc::dfc_header_plan(y.len, y.len + sk_dfc::kDfcLit, y.work, y.hdr);
        }
        __syncthreads();
        for (int i = t; i < kDfSyms; i += kDfBlock) {
            const int nl = y.len[i];
            y.tab[i] = (nl ? df_rev(y.code[i], nl) : 0u) | ((unsigned)nl << 16);
        }
        __syncthreads();
    }
    // bits per token under both codes in one walk
    unsigned tb = 0, tbd = 0;
#pragma unroll
    for (int k = 0; k < kDfPer; ++k) {
        if ((marked >> k) & 1ull) {
            unsigned b0, b1;
            int n0, n1;
            df_token(best[k], (own[k >> 2] >> (8 * (k & 3))) & 255u, e, b0, n0, b1, n1);
            tb += (unsigned)(n0 + n1);
            if constexpr (kDyn) {
                df_token_dyn(best[k], (own[k >> 2] >> (8 * (k & 3))) & 255u, e, s.dyn.tab, b0, n0, b1, n1);
                tbd += (unsigned)(n0 + n1);
            }
        }
    }
    unsigned inc = tb, incd = tbd;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
        if constexpr (kDyn) {
            const unsigned vd = __shfl_up(incd, o);
            if (lane >= o) incd += vd;
        }
    }
    if (lane == 63) {
        s.red[16 + wave] = inc;
        if constexpr (kDyn) s.red[20 + wave] = incd;
    }
    __syncthreads();   // also: every read of jump[] is behind us, out[] may take its place
    unsigned woff = 0, total = 0, woffd = 0, totald = 0;
#pragma unroll
    for (int w = 0; w < kDfBlock / 64; ++w) {
        const unsigned v = s.red[16 + w];
        if (w < wave) woff += v;
        total += v;
        if constexpr (kDyn) {
            const unsigned vd = s.red[20 + w];
            if (w < wave) woffd += vd;
            totald += vd;
        }
    }
    unsigned T = 3u + total + 7u;                             // block header, tokens, end of block
    unsigned sync_at = (T + 3u + 7u) / 8u;                    // first byte after the empty stored block's header
    unsigned cbytes = last ? (T + 7u) / 8u : sync_at + 4u;
    bool stored = cbytes > 5u + (unsigned)n;
    bool dyn = false;
    unsigned hbits = 3u;                                      // bits in front of the first token
    if constexpr (kDyn) {
        // the smallest of the three wins; on equal bytes stored, then fixed, then dynamic
        stored = cbytes >= 5u + (unsigned)n;
        hbits = s.dyn.hdr.bits;
        const unsigned Td = hbits + totald + (s.dyn.tab[256] >> 16);
        const unsigned sync_d = (Td + 3u + 7u) / 8u;
        const unsigned cbytes_d = last ? (Td + 7u) / 8u : sync_d + 4u;
        if (cbytes_d < (stored ? 5u + (unsigned)n : cbytes)) {
            dyn = true;
            stored = false;
            T = Td;
            sync_at = sync_d;
            cbytes = cbytes_d;
            woff = woffd;
            inc = incd;
            tb = tbd;
        } else {
            hbits = 3u;
        }
    }
    uint8_t* slot = slots + piece * kDfSlot;

    if (!stored) {
        const unsigned nwords = (cbytes + 3u) / 4u;
        for (unsigned i = t; i < nwords; i += kDfBlock) s.out[i] = 0;
        __syncthreads();
        if (t == 0) {
            if (!dyn) atomicOr(&s.out[0], (last ? 1u : 0u) | 2u);   // BFINAL, BTYPE = 01; its end of block is 7 zero bits
            if (!last) {                                      // 00 00 FF FF
                atomicOr(&s.out[(sync_at + 2) >> 2], 0xFFu << (8 * ((sync_at + 2) & 3)));
                atomicOr(&s.out[(sync_at + 3) >> 2], 0xFFu << (8 * ((sync_at + 3) & 3)));
            }
        }
        if constexpr (kDyn) {
            if (dyn && t == 0) {                              // BFINAL, BTYPE = 10, the code lengths; end of block
                unsigned at = 0;
                unsigned* out = s.out;
                sk_dfc::dfc_header_emit(s.dyn.hdr, last ? 1 : 0, [&](unsigned val, int nb) {
                    df_put(out, at, val, nb);
                    at += (unsigned)nb;
                });
                const unsigned eob = s.dyn.tab[256];
                df_put(out, hbits + totald, eob & 0xffffu, (int)(eob >> 16));
            }
        }
        unsigned off = hbits + woff + inc - tb;
#pragma unroll
        for (int k = 0; k < kDfPer; ++k) {
            if ((marked >> k) & 1ull) {
                unsigned b0, b1;
                int n0, n1;
                if (kDyn && dyn) df_token_dyn(best[k], (own[k >> 2] >> (8 * (k & 3))) & 255u, e, s.dyn.tab, b0, n0, b1, n1);
                else df_token(best[k], (own[k >> 2] >> (8 * (k & 3))) & 255u, e, b0, n0, b1, n1);
                df_put(s.out, off, b0, n0);
                off += n0;
                if (n1) df_put(s.out, off, b1, n1);
                off += n1;
            }
        }
        __syncthreads();
        unsigned* g = (unsigned*)slot;
        for (unsigned i = t; i < nwords; i += kDfBlock) g[i] = s.out[i];
    } else {
        if (t == 0) {
            slot[kDfStoredOff] = last ? 1 : 0;
            slot[kDfStoredOff + 1] = (uint8_t)(n & 255);
            slot[kDfStoredOff + 2] = (uint8_t)(n >> 8);
            slot[kDfStoredOff + 3] = (uint8_t)(~n & 255);
            slot[kDfStoredOff + 4] = (uint8_t)((~n >> 8) & 255);
        }
        if (base < n) {
            uint4* g = (uint4*)(slot + kDfStoredOff + 5) + 4 * t;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = make_uint4(own[4 * j], own[4 * j + 1], own[4 * j + 2], own[4 * j + 3]);
        }
    }
    if (t == 0) {
        unsigned* mt = meta + piece * kDfMeta;
        mt[0] = stored ? 5u + (unsigned)n : cbytes;
        mt[1] = stored ? (unsigned)kDfStoredOff : 0u;
        mt[2] = (s.red[0] + s.red[1] + s.red[2] + s.red[3]) % kAdlerMod;
        mt[3] = (s.red[4] + s.red[5] + s.red[6] + s.red[7]) % kAdlerMod;
        mt[4] = s.red[8] | s.red[9] | s.red[10] | s.red[11];
    }
}

// exclusive prefix sums over the 256 per-thread partials in LDS (thread 0 walks them: 256 steps, not on any hot path)
__device__ inline void df_scan256(unsigned long long* v, unsigned long long* total) {
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < kDfBlock; ++i) {
            const unsigned long long c = v[i];
            v[i] = run;
            run += c;
        }
        *total = run;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kDfBlock) void deflate_stream_kernel(const unsigned* __restrict__ meta, const int64_t L,
                                                                  const int64_t pps, const int skip_zero,
                                                                  int64_t* __restrict__ prefix,
                                                                  int64_t* __restrict__ stream_size,
                                                                  unsigned* __restrict__ stream_adler,
                                                                  unsigned* __restrict__ stream_zero) {
    __shared__ unsigned long long ssz[kDfBlock], ssa[kDfBlock], tot[2];
    __shared__ unsigned ssb[kDfBlock], snz[kDfBlock];
    const int t = threadIdx.x;
    const int64_t strm = blockIdx.x;
    const int64_t per = (pps + kDfBlock - 1) / kDfBlock;
    const int64_t lo = t * per < pps ? t * per : pps, hi = lo + per < pps ? lo + per : pps;
    const unsigned* mt = meta + strm * pps * kDfMeta;
    unsigned long long sz = 0, a = 0;
    unsigned nz = 0;
    for (int64_t p = lo; p < hi; ++p) {
        sz += mt[p * kDfMeta];
        a += mt[p * kDfMeta + 2];
        nz |= mt[p * kDfMeta + 4];
    }
    ssz[t] = sz;
    ssa[t] = a;
    snz[t] = nz;
    df_scan256(ssz, &tot[0]);
    df_scan256(ssa, &tot[1]);
    unsigned long long at = ssz[t];
    unsigned s1 = (unsigned)((1ull + ssa[t]) % kAdlerMod), s2 = 0;   // Adler-32 state in front of piece lo
    for (int64_t p = lo; p < hi; ++p) {
        prefix[strm * pps + p] = (int64_t)at;
        at += mt[p * kDfMeta];
        const int64_t left = L - p * kDfPiece;
        const unsigned np = (unsigned)(left < kDfPiece ? left : kDfPiece);
        s2 = (unsigned)((s2 + (unsigned long long)np * s1 + mt[p * kDfMeta + 3]) % kAdlerMod);
        s1 = (s1 + mt[p * kDfMeta + 2]) % kAdlerMod;
    }
    ssb[t] = s2;
    __syncthreads();
    if (t == 0) {
        unsigned long long b = 0;
        unsigned any = 0;
        for (int i = 0; i < kDfBlock; ++i) {
            b += ssb[i];
            any |= snz[i];
        }
        const unsigned zero = any == 0 ? 1u : 0u;
        stream_adler[strm] = ((unsigned)(b % kAdlerMod) << 16) | (unsigned)((1ull + tot[1]) % kAdlerMod);
        stream_zero[strm] = zero;
        stream_size[strm] = (skip_zero && zero) ? 0 : (int64_t)(2 + tot[0] + 4);
    }
}

__global__ __launch_bounds__(kDfBlock) void deflate_offsets_kernel(const int64_t* __restrict__ stream_size,
                                                                   const unsigned* __restrict__ stream_zero,
                                                                   const int n_streams, int64_t* __restrict__ dst_offsets,
                                                                   uint8_t* __restrict__ all_zero) {
    __shared__ unsigned long long ssz[kDfBlock], tot;
    const int t = threadIdx.x;
    const int per = (n_streams + kDfBlock - 1) / kDfBlock;
    const int lo = t * per < n_streams ? t * per : n_streams, hi = lo + per < n_streams ? lo + per : n_streams;
    unsigned long long sz = 0;
    for (int i = lo; i < hi; ++i) sz += (unsigned long long)stream_size[i];
    ssz[t] = sz;
    df_scan256(ssz, &tot);
    unsigned long long at = ssz[t];
    for (int i = lo; i < hi; ++i) {
        dst_offsets[i] = (int64_t)at;
        at += (unsigned long long)stream_size[i];
        if (all_zero) all_zero[i] = (uint8_t)stream_zero[i];
    }
    if (t == 0) dst_offsets[n_streams] = (int64_t)tot;
}

__global__ __launch_bounds__(kDfBlock) void deflate_compact_kernel(const uint8_t* __restrict__ slots,
                                                                   const unsigned* __restrict__ meta, const int64_t pps,
                                                                   const int64_t* __restrict__ prefix,
                                                                   const int64_t* __restrict__ stream_size,
                                                                   const unsigned* __restrict__ stream_adler,
                                                                   const int64_t* __restrict__ dst_offsets,
                                                                   uint8_t* __restrict__ dst) {
    const int t = threadIdx.x;
    const int64_t piece = blockIdx.x;
    const int64_t strm = piece / pps, p = piece - strm * pps;
    if (stream_size[strm] == 0) return;   // an all-zero stream the caller asked to leave out
    const unsigned nb = meta[piece * kDfMeta];
    const uint8_t* from = slots + piece * kDfSlot + meta[piece * kDfMeta + 1];
    uint8_t* out = dst + dst_offsets[strm];
    uint8_t* to = out + 2 + prefix[piece];
    for (unsigned i = t; i < nb; i += kDfBlock) to[i] = from[i];
    if (t == 0 && p == 0) {
        out[0] = 0x78;
        out[1] = 0x01;
    }
    if (t == 0 && p == pps - 1) {
        const unsigned ad = stream_adler[strm];
        uint8_t* tail = out + stream_size[strm] - 4;
        tail[0] = (uint8_t)(ad >> 24);
        tail[1] = (uint8_t)(ad >> 16);
        tail[2] = (uint8_t)(ad >> 8);
        tail[3] = (uint8_t)ad;
    }
}

static_assert(sizeof(DfDyn) <= sizeof(unsigned long long) * kDfGroup * (kDfBlock + 8), "the dynamic tables take eq[]'s place");
static inline size_t df_align(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace sk

extern "C" size_t sk_deflate_bound(int64_t stream_bytes) {
    if (stream_bytes < 0) stream_bytes = 0;
    // 2 header + 4 trailer bytes; a stored piece is its bytes + 5, and no piece is written larger than that
    return (size_t)stream_bytes + 6 + 5 * (size_t)sk::df_pieces(stream_bytes);
}

extern "C" size_t sk_deflate_workspace_bytes(int n_streams, int64_t stream_bytes) {
    if (n_streams < 0 || stream_bytes < 0) return 0;
    const size_t pieces = (size_t)n_streams * (size_t)sk::df_pieces(stream_bytes);
    return sk::df_align(pieces * sk::kDfSlot) + sk::df_align(pieces * sk::kDfMeta * 4) + sk::df_align(pieces * 8) +
           sk::df_align((size_t)n_streams * 8) + 2 * sk::df_align((size_t)n_streams * 4) + 16;
}

// both entry points: fn is the name the refusals carry
static int df_streams(const char* fn, const uint8_t* src, int n_streams, int64_t stream_bytes, int elem_bytes, int huffman,
                      uint8_t* dst, int64_t* dst_offsets, uint8_t* all_zero, void* workspace, size_t workspace_bytes,
                      void* stream) {
    SK_CHECK_ARG(n_streams >= 0, "%s: n_streams = %d is negative", fn, n_streams);
    SK_CHECK_ARG(stream_bytes >= 0 && stream_bytes <= ((int64_t)1 << 40), "%s: stream_bytes = %lld outside [0, 2^40]", fn,
                 (long long)stream_bytes);
    SK_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, "%s: elem_bytes = %d, must be 1, 2 or 4", fn,
                 elem_bytes);
    SK_CHECK_ARG(huffman == 0 || huffman == 1, "%s: huffman = %d, must be 0 (fixed code) or 1 (best of fixed and dynamic)",
                 fn, huffman);
    SK_CHECK_ARG(dst_offsets != nullptr && ((uintptr_t)dst_offsets & 7) == 0,
                 "%s: dst_offsets is NULL or not 8-byte aligned", fn);
    const int64_t pps = sk::df_pieces(stream_bytes);
    const int64_t pieces = (int64_t)n_streams * pps;
    SK_CHECK_ARG(pieces <= 0x7fffffffLL, "%s: %lld pieces of 16 KiB in one call, at most 2^31 - 1", fn,
                 (long long)pieces);
    SK_CHECK_ARG(n_streams == 0 || stream_bytes == 0 || src != nullptr, "%s: src is NULL", fn);
    SK_CHECK_ARG(n_streams == 0 || dst != nullptr, "%s: dst is NULL", fn);
    const size_t need = sk_deflate_workspace_bytes(n_streams, stream_bytes);
    SK_CHECK_ARG(workspace != nullptr && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                 "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu at %p", fn, need, workspace_bytes,
                 workspace);
    uint8_t* w = (uint8_t*)workspace;
    uint8_t* slots = w;
    w += sk::df_align((size_t)pieces * sk::kDfSlot);
    unsigned* meta = (unsigned*)w;
    w += sk::df_align((size_t)pieces * sk::kDfMeta * 4);
    int64_t* prefix = (int64_t*)w;
    w += sk::df_align((size_t)pieces * 8);
    int64_t* stream_size = (int64_t*)w;
    w += sk::df_align((size_t)n_streams * 8);
    unsigned* stream_adler = (unsigned*)w;
    w += sk::df_align((size_t)n_streams * 4);
    unsigned* stream_zero = (unsigned*)w;
    hipStream_t st = (hipStream_t)stream;
    if (n_streams > 0) {
        if (huffman)
            hipLaunchKernelGGL(sk::deflate_piece_kernel<true>, dim3((unsigned)pieces), dim3(sk::kDfBlock), 0, st, src,
                               stream_bytes, pps, elem_bytes, slots, meta);
        else
            hipLaunchKernelGGL(sk::deflate_piece_kernel<false>, dim3((unsigned)pieces), dim3(sk::kDfBlock), 0, st, src,
                               stream_bytes, pps, elem_bytes, slots, meta);
        SK_CHECK_LAUNCH();
        hipLaunchKernelGGL(sk::deflate_stream_kernel, dim3((unsigned)n_streams), dim3(sk::kDfBlock), 0, st, meta,
                           stream_bytes, pps, all_zero != nullptr ? 1 : 0, prefix, stream_size, stream_adler, stream_zero);
        SK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sk::deflate_offsets_kernel, dim3(1), dim3(sk::kDfBlock), 0, st, stream_size, stream_zero, n_streams,
                       dst_offsets, all_zero);
    SK_CHECK_LAUNCH();
    if (n_streams > 0) {
        hipLaunchKernelGGL(sk::deflate_compact_kernel, dim3((unsigned)pieces), dim3(sk::kDfBlock), 0, st, slots, meta, pps,
                           prefix, stream_size, stream_adler, dst_offsets, dst);
        SK_CHECK_LAUNCH();
    }
    return SK_OK;
}

extern "C" int sk_deflate_streams(const uint8_t* src, int n_streams, int64_t stream_bytes, int elem_bytes, uint8_t* dst,
                                  int64_t* dst_offsets, uint8_t* all_zero, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return df_streams("sk_deflate_streams", src, n_streams, stream_bytes, elem_bytes, 0, dst, dst_offsets, all_zero,
                      workspace, workspace_bytes, stream);
}

extern "C" int sk_deflate_streams_coded(const uint8_t* src, int n_streams, int64_t stream_bytes, int elem_bytes,
                                        int huffman, uint8_t* dst, int64_t* dst_offsets, uint8_t* all_zero,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return df_streams("sk_deflate_streams_coded", src, n_streams, stream_bytes, elem_bytes, huffman, dst, dst_offsets,
                      all_zero, workspace, workspace_bytes, stream);
}

extern "C" int sk_deflate_code_host(const uint32_t* freq, int n_symbols, int limit, uint8_t* lengths, uint16_t* codes) {
    SK_CHECK_ARG(freq != nullptr && lengths != nullptr && codes != nullptr, "sk_deflate_code_host: NULL argument");
    SK_CHECK_ARG(n_symbols >= 1 && n_symbols <= sk_dfc::kDfcLit, "sk_deflate_code_host: n_symbols = %d outside [1, 286]",
                 n_symbols);
    SK_CHECK_ARG(limit >= 1 && limit <= 15, "sk_deflate_code_host: limit = %d outside [1, 15]", limit);
    unsigned long long sum = 0;
    int used = 0;
    for (int s = 0; s < n_symbols; ++s) {
        sum += freq[s];
        used += freq[s] != 0;
    }
    SK_CHECK_ARG(sum <= 0xffffffffull, "sk_deflate_code_host: the counts add up to %llu, at most 2^32 - 1", sum);
    SK_CHECK_ARG(used <= (1 << limit), "sk_deflate_code_host: %d used symbols do not fit a code of at most %d bits", used,
                 limit);
    sk_dfc::DfcWork w;
    const int m = sk_dfc::dfc_sort(freq, n_symbols, w.order);
    sk_dfc::dfc_lengths(freq, n_symbols, m, limit, w, lengths);
    sk_dfc::dfc_codes(lengths, n_symbols, w, codes);
    return SK_OK;
}

extern "C" int sk_deflate_header_host(const uint8_t* lit_lengths, const uint8_t* dist_lengths, int bfinal, uint8_t* out,
                                      size_t out_bytes, int64_t* n_bits) {
    SK_CHECK_ARG(lit_lengths != nullptr && dist_lengths != nullptr && out != nullptr && n_bits != nullptr,
                 "sk_deflate_header_host: NULL argument");
    SK_CHECK_ARG(bfinal == 0 || bfinal == 1, "sk_deflate_header_host: bfinal = %d, must be 0 or 1", bfinal);
    SK_CHECK_ARG(out_bytes >= (size_t)sk_dfc::kDfcHeaderBytes, "sk_deflate_header_host: out of %zu bytes, need %d", out_bytes,
                 sk_dfc::kDfcHeaderBytes);
    for (int s = 0; s < sk_dfc::kDfcLit; ++s)
        SK_CHECK_ARG(lit_lengths[s] <= 15, "sk_deflate_header_host: lit_lengths[%d] = %d above 15", s, lit_lengths[s]);
    for (int s = 0; s < sk_dfc::kDfcDist; ++s)
        SK_CHECK_ARG(dist_lengths[s] <= 15, "sk_deflate_header_host: dist_lengths[%d] = %d above 15", s, dist_lengths[s]);
    sk_dfc::DfcWork w;
    sk_dfc::DfcHdr h;
    sk_dfc::dfc_header_plan(lit_lengths, dist_lengths, w, h);
    for (int i = 0; i < sk_dfc::kDfcHeaderBytes; ++i) out[i] = 0;
    unsigned at = 0;
    sk_dfc::dfc_header_emit(h, bfinal, [&](unsigned val, int nb) {
        for (int b = 0; b < nb; ++b, ++at) out[at >> 3] |= (uint8_t)(((val >> b) & 1u) << (at & 7));
    });
    *n_bits = (int64_t)at;
    return SK_OK;
}
