// Inflate decoder for the files eval() reads back: zarr chunks with the zlib codec and Adobe-deflate TIFF strips, each
// one RFC 1950 stream (or raw RFC 1951), inflated where the array is wanted.  The mirror of deflate.hip; replaces
// zlib.decompress per chunk (skoots_amd/lib/zarr_store.py: load) and Pillow's page-by-page read (lib/tiff.py:
// read_image) for readers that want the array on the device.  No reference counterpart (the reference leaves reading
// to zarr / skimage on the host, eval.py:61, 160-176).
//
// One wave64 workgroup per stream.  Decoding a Huffman stream is serial, so the wave decodes with wave-uniform state --
// bit buffer, positions and error code are the same in every lane, table entries come out of LDS through
// readfirstlane -- and uses its lanes where there is something to do side by side:
//   input     a 2 KiB window of the stream in LDS, loaded by all lanes with every byte checked against the stream's
//             range (bytes past the end are zeros and never loaded); the bit buffer refills 32 bits at a time from it
//   tables    per dynamic block: code lengths -> counts per length (lane l counts length l), canonical order (lane l
//             places the symbols of length l), a 10-bit primary table filled by all lanes; longer codes are decoded by
//             the canonical walk over the counts (at most 15 steps).  The fixed code goes through the same builder, once
//   tokens    up to 64 (literal | length + distance) are decoded into LDS, every bound checked while decoding
//             (distance <= bytes produced, output <= expected), so that emitting cannot leave the stream's dst range
//   emit      in token order: a run of literals is stored by as many lanes at once; a match is copied by all lanes,
//             64 bytes a step, lane k reading base + k % dist when the match overlaps itself
//   output    every byte goes to dst (byte stores of consecutive lanes) and into a 32 KiB ring in LDS, which is what
//             matches read: no byte is ever read back from dst.  Steps are strictly in output order and the ring is as
//             long as the largest distance, so a slot is overwritten only by the byte 32768 after it, which no later
//             source can be (source >= position - 32768).  All lanes of a step read before any of them writes
//   Adler-32  per batch over the bytes just written to the ring: (sum b, sum j b_j) per lane, one wave reduction
// A data error is a status code; the kernel has no assert and no trap.  Every loop consumes input bits or ends on an
// error, and running out of input is an error, so every loop ends.
//
// The wave is written as "uniform code + lane sections" (SK_LANES).  On the device a lane section runs once with
// lane = threadIdx.x; with -DSK_INFLATE_HOST the same text compiles as host C++ in which a lane section is a loop over
// the 64 lanes, which is how the decoder is run under AddressSanitizer / UBSan on the CPU (tools/inflate_host_check.cpp).
#ifndef SK_INFLATE_HOST
#include "common.h"
#define SK_LANES for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define SK_LI 0                 // index of a lane's slot in a per-lane temporary
#define SK_NL 1
#define SK_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#define SK_SYNC() __syncthreads()
#define SK_BREV(x) __brev(x)
#define SK_CTZ64(x) __builtin_ctzll(x)
__device__ inline unsigned long long inf_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
#define SK_WAVE_SUM(x) inf_wave_sum(x)
#else
#define SK_LANES for (int lane = 0; lane < 64; ++lane)
#define SK_LI lane
#define SK_NL 64
#define SK_UNI(x) ((int)(x))
#define SK_SYNC()
static inline unsigned inf_brev(unsigned x) {
    unsigned r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
#define SK_BREV(x) inf_brev(x)
#define SK_CTZ64(x) __builtin_ctzll(x)
#define SK_WAVE_SUM(x) (x)
#endif

namespace sk {

constexpr int kInfRing = 32768;                 // bytes of output kept in LDS = the largest distance
constexpr int kInfWin = 512;                    // dwords of input in LDS
constexpr int kInfPrim = 10;                    // bits of the primary tables
constexpr int kInfSyms = 288;                   // symbols of the largest alphabet
constexpr int kInfBatch = 64;                   // tokens per batch
constexpr int kInfStoredStep = 16384;           // bytes of a stored block copied between two Adler updates
constexpr unsigned kInfAdlerMod = 65521u;

struct InfCode {
    unsigned short prim[1 << kInfPrim];         // (symbol << 4) | bits; 0 = no code of <= 10 bits starts like this
    unsigned short sym[kInfSyms];                  // symbols in canonical order
    unsigned short count[16], offs[16], first[16];   // per length: codes, index of the first in sym, first code
};

struct InfLds {
    unsigned ring[kInfRing / 4];
    unsigned win[kInfWin];
    InfCode lit, dist;
    unsigned tok[kInfBatch];                    // literal: byte << 9; match: length | distance << 9
    unsigned char lens[320 + 32];               // code lengths: literal/length + distance; the code-length code at 320
};

// wave-uniform decoder state
struct InfState {
    unsigned long long bb;                      // bit buffer, next bit = bit 0
    int bc;                                     // valid bits in bb
    long long bits_left;                        // stream bits not yet consumed; negative = read past the end
    long long d;                                // next dword of the stream to enter bb (dword 0 starts at a0)
    long long wbase;                            // first dword in the window; -1 = nothing loaded
    unsigned long long a0, lo, hi;              // addresses: a0 = lo rounded down to 4, stream = [lo, hi)
    int err;
};

__device__ inline void inf_load_window(InfLds& s, InfState& st) {
    SK_SYNC();
    SK_LANES {
        for (int j = lane; j < kInfWin; j += 64) {
            const unsigned long long a = st.a0 + 4ull * (unsigned long long)(st.wbase + j);
            unsigned v = 0;
            if (a >= st.lo && a + 4 <= st.hi) {
                v = *(const unsigned*)(uintptr_t)a;
            } else if (a < st.hi) {
                for (int b = 0; b < 4; ++b)
                    if (a + b >= st.lo && a + b < st.hi) v |= (unsigned)(*(const uint8_t*)(uintptr_t)(a + b)) << (8 * b);
            }
            s.win[j] = v;
        }
    }
    SK_SYNC();
}

// after this at least 32 bits are in the buffer (exactly 32 when it was empty): enough for a code (15) + its extra
// bits (13), or for 32 plain bits
__device__ inline void inf_refill(InfLds& s, InfState& st) {
    if (st.bc <= 32) {
        if (st.wbase < 0 || st.d < st.wbase || st.d - st.wbase >= kInfWin) {
            st.wbase = st.d;
            inf_load_window(s, st);
        }
        const unsigned w = (unsigned)SK_UNI(s.win[(int)(st.d - st.wbase)]);
        st.bb |= (unsigned long long)w << st.bc;
        st.bc += 32;
        st.d += 1;
    }
}

__device__ inline unsigned inf_take(InfState& st, int n) {   // n <= 32 and <= bc
    const unsigned v = (unsigned)(st.bb & ((1ull << n) - 1ull));
    st.bb >>= n;
    st.bc -= n;
    st.bits_left -= n;
    return v;
}

// the bit reader at byte `pos` of the stream (0 <= pos <= length)
__device__ inline void inf_seek(InfLds& s, InfState& st, long long pos) {
    const unsigned long long a = st.lo + (unsigned long long)pos;
    st.d = (long long)((a - st.a0) >> 2);
    const int skip = (int)((a - st.a0) & 3u) * 8;
    st.bb = 0;
    st.bc = 0;
    st.bits_left = 8 * ((long long)(st.hi - st.lo) - pos);
    inf_refill(s, st);
    st.bb >>= skip;
    st.bc -= skip;
    inf_refill(s, st);
}

// One symbol of `c`, or -1 if the next bits are no code of it.  Needs 15 bits in the buffer.
__device__ inline int inf_decode(const InfCode& c, InfState& st) {
    const unsigned peek = (unsigned)st.bb;
    const unsigned e = (unsigned)SK_UNI(c.prim[peek & ((1u << kInfPrim) - 1u)]);
    if (e != 0) {
        inf_take(st, (int)(e & 15u));
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((peek >> (l - 1)) & 1u);
        const int cnt = SK_UNI(c.count[l]);
        if (code - cnt < first) {
            const int at = index + (code - first);
            if (at < 0 || at >= kInfSyms) return -1;
            inf_take(st, l);
            return SK_UNI(c.sym[at]);
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

enum { kInfKindCodeLen = 0, kInfKindLit = 1, kInfKindDist = 2 };

// Tables of one code from n code lengths (0..15) at `lens`.  zlib's rules (inftrees.c): an over-subscribed set is
// refused; an incomplete one too, unless it is a literal/length or distance set whose longest code has one bit; a set
// without any code is an empty table (every symbol invalid).  Returns 0 or SK_INFLATE_E_CODES.
__device__ inline int inf_build(InfCode& c, const unsigned char* lens, int n, int kind) {
    SK_SYNC();
    SK_LANES {
        for (int j = lane; j < (1 << kInfPrim); j += 64) c.prim[j] = 0;
        if (lane < 16) {
            int k = 0;
            for (int i = 0; i < n; ++i) k += lens[i] == lane ? 1 : 0;
            c.count[lane] = (unsigned short)(lane == 0 ? 0 : k);
        }
    }
    SK_SYNC();
    int left = 1, total = 0, maxlen = 0;
    bool over = false;
    for (int l = 1; l <= 15; ++l) {
        const int cnt = SK_UNI(c.count[l]);
        total += cnt;
        left = (left << 1) - cnt;
        if (left < 0) {
            over = true;
            left = 0;                 // keeps the shifts defined; `over` is what counts
        }
        if (cnt) maxlen = l;
    }
    if (over) return SK_INFLATE_E_CODES;
    if (total > 0 && left > 0 && (kind == kInfKindCodeLen || maxlen != 1)) return SK_INFLATE_E_CODES;
    SK_LANES {
        if (lane < 16) {              // canonical code: first code and first index of length `lane`
            int code = 0, at = 0;
            for (int l = 1; l <= lane; ++l) {
                code = (code + c.count[l - 1]) << 1;
                at += c.count[l - 1];
            }
            c.offs[lane] = (unsigned short)at;
            c.first[lane] = (unsigned short)code;
        }
    }
    SK_SYNC();
    SK_LANES {
        if (lane >= 1 && lane < 16) {
            int k = c.offs[lane];
            for (int i = 0; i < n; ++i)
                if (lens[i] == lane && k < kInfSyms) c.sym[k++] = (unsigned short)i;
        }
    }
    SK_SYNC();
    SK_LANES {
        for (int i = lane; i < total; i += 64) {
            const int sy = c.sym[i];
            const int l = sy < n ? lens[sy] : 0;
            if (l >= 1 && l <= kInfPrim) {
                const unsigned cd = (unsigned)c.first[l] + (unsigned)(i - c.offs[l]);
                const unsigned r = SK_BREV(cd) >> (32 - l);
                for (unsigned j = r; j < (1u << kInfPrim); j += 1u << l) c.prim[j] = (unsigned short)((sy << 4) | l);
            }
        }
    }
    SK_SYNC();
    return 0;
}

// Adler-32 over the n <= 16512 bytes at output position `start`, which are still in the ring
__device__ inline void inf_adler(const InfLds& s, long long start, int n, unsigned& s1, unsigned& s2) {
    if (n <= 0) return;
    SK_SYNC();
    const unsigned char* ring = (const unsigned char*)s.ring;
    unsigned long long a = 0, c = 0;
    SK_LANES {
        unsigned la = 0, lc = 0;                     // per lane at most 258 bytes: 258 * 255 * 16512 < 2^32
        for (int j = lane; j < n; j += 64) {
            const unsigned b = ring[(unsigned)(start + j) & (kInfRing - 1)];
            la += b;
            lc += b * (unsigned)j;
        }
        a += la;
        c += lc;
    }
    a = SK_WAVE_SUM(a);
    c = SK_WAVE_SUM(c);
    // s2 += n s1 + sum (n - j) b_j
    s2 = (unsigned)((s2 + (unsigned long long)n * s1 + (unsigned long long)n * a - c) % kInfAdlerMod);
    s1 = (unsigned)((s1 + a) % kInfAdlerMod);
}

// The tokens s.tok[0..n) to the ring and to out[pos ..]; bit i of litmask = token i is a literal.  Every token was
// checked while decoding: all of the output lies inside the stream's range, every source at or after its start.
__device__ inline void inf_emit(InfLds& s, uint8_t* out, long long pos, int n, unsigned long long litmask) {
    SK_SYNC();
    unsigned char* ring = (unsigned char*)s.ring;
    int i = 0;
    while (i < n) {
        if ((litmask >> i) & 1ull) {
            const unsigned long long rest = ~(litmask >> i);
            int r = rest == 0 ? 64 : (int)SK_CTZ64(rest);
            if (r > n - i) r = n - i;
            SK_LANES {
                if (lane < r) {
                    const unsigned char b = (unsigned char)(s.tok[i + lane] >> 9);
                    ring[(unsigned)(pos + lane) & (kInfRing - 1)] = b;
                    out[pos + lane] = b;
                }
            }
            SK_SYNC();            // the next step may be a match whose lanes read these bytes from the ring
            pos += r;
            i += r;
        } else {
            const unsigned t = (unsigned)SK_UNI(s.tok[i]);
            const int len = (int)(t & 511u), dist = (int)(t >> 9);
            const long long base = pos - dist;
            for (int c0 = 0; c0 < len; c0 += 64) {
                unsigned char v[SK_NL];
                SK_LANES {
                    const int k = c0 + lane;
                    if (k < len) v[SK_LI] = ring[(unsigned)(base + (k < dist ? k : k % dist)) & (kInfRing - 1)];
                }
                SK_SYNC();
                SK_LANES {
                    const int k = c0 + lane;
                    if (k < len) {
                        ring[(unsigned)(pos + k) & (kInfRing - 1)] = v[SK_LI];
                        out[pos + k] = v[SK_LI];
                    }
                }
                SK_SYNC();
            }
            pos += len;
            i += 1;
        }
    }
    SK_SYNC();
}

__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t* __restrict__ src,
                                                     const int64_t* __restrict__ src_offsets,
                                                     uint8_t* __restrict__ dst, const int64_t* __restrict__ dst_offsets,
                                                     const int wrapper, int32_t* __restrict__ status) {
    __shared__ InfLds s;
    const int strm = (int)blockIdx.x;
    const long long so = src_offsets[strm], se = src_offsets[strm + 1];
    const long long dofs = dst_offsets[strm], de = dst_offsets[strm + 1];
    InfState st;
    st.err = 0;
    if (so < 0 || se < so || dofs < 0 || de < dofs) {
        SK_LANES { if (lane == 0) status[strm] = SK_INFLATE_E_RANGE; }
        return;
    }
    const long long out_len = de - dofs;
    uint8_t* out = dst + dofs;
    st.lo = (unsigned long long)(uintptr_t)src + (unsigned long long)so;
    st.hi = st.lo + (unsigned long long)(se - so);
    st.a0 = st.lo & ~3ull;
    st.wbase = -1;
    inf_seek(s, st, 0);

    long long produced = 0;
    unsigned s1 = 1, s2 = 0;
    bool fixed_built = false;

    if (wrapper) {
        const unsigned cmf = inf_take(st, 8), flg = inf_take(st, 8);
        if (st.bits_left < 0) st.err = SK_INFLATE_E_INPUT;
        else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0 || (flg & 0x20u))
            st.err = SK_INFLATE_E_HEADER;
    }

    bool last = false;
    while (!last && st.err == 0) {
        inf_refill(s, st);
        last = inf_take(st, 1) != 0;
        const unsigned type = inf_take(st, 2);
        if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
        if (type == 3) { st.err = SK_INFLATE_E_BLOCK_TYPE; break; }
        if (type == 0) {
            inf_take(st, (int)(st.bits_left & 7));
            inf_refill(s, st);
            const unsigned len = inf_take(st, 16);
            inf_refill(s, st);
            const unsigned nlen = inf_take(st, 16);
            if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
            if (len != ((~nlen) & 0xFFFFu)) { st.err = SK_INFLATE_E_STORED; break; }
            if (produced + (long long)len > out_len) { st.err = SK_INFLATE_E_OUTPUT_LONG; break; }
            if (8ll * (long long)len > st.bits_left) { st.err = SK_INFLATE_E_INPUT; break; }
            const long long at = (long long)(st.hi - st.lo) - st.bits_left / 8;   // byte of the stream the data start at
            const uint8_t* from = (const uint8_t*)(uintptr_t)st.lo + at;
            unsigned char* ring = (unsigned char*)s.ring;
            for (int c0 = 0; c0 < (int)len; c0 += kInfStoredStep) {
                const int m = (int)len - c0 < kInfStoredStep ? (int)len - c0 : kInfStoredStep;
                SK_SYNC();
                SK_LANES {
#pragma unroll 4
                    for (int k = lane; k < m; k += 64) {
                        const unsigned char b = from[c0 + k];
                        ring[(unsigned)(produced + k) & (kInfRing - 1)] = b;
                        out[produced + k] = b;
                    }
                }
                if (wrapper) inf_adler(s, produced, m, s1, s2);
                produced += m;
            }
            inf_seek(s, st, at + (long long)len);
            continue;
        }
        if (type == 1) {
            if (!fixed_built) {
                SK_SYNC();
                SK_LANES {
                    for (int i = lane; i < 288; i += 64) s.lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                    if (lane < 32) s.lens[288 + lane] = 5;
                }
                SK_SYNC();
                inf_build(s.lit, s.lens, 288, kInfKindLit);
                inf_build(s.dist, s.lens + 288, 32, kInfKindDist);
                fixed_built = true;
            }
        } else {
            fixed_built = false;
            inf_refill(s, st);
            const int hlit = (int)inf_take(st, 5) + 257, hdist = (int)inf_take(st, 5) + 1, hclen = (int)inf_take(st, 4) + 4;
            if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
            if (hlit > 286 || hdist > 30) { st.err = SK_INFLATE_E_CODES; break; }
            unsigned long long cl = 0;                       // 19 code lengths of 3 bits, in symbol order
            for (int i = 0; i < hclen; ++i) {
                // the order the code-length code's lengths are sent in (RFC 1951 3.2.7), 5 bits each
                const unsigned long long order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 |
                                                    9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
                const unsigned long long order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 |
                                                    15ull << 30;
                const int sy = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31ull);
                inf_refill(s, st);
                cl |= (unsigned long long)inf_take(st, 3) << (3 * sy);
            }
            if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
            SK_SYNC();
            SK_LANES { if (lane < 19) s.lens[320 + lane] = (unsigned char)((cl >> (3 * lane)) & 7ull); }
            if (cl == 0 || inf_build(s.dist, s.lens + 320, 19, kInfKindCodeLen) != 0) { st.err = SK_INFLATE_E_CODES; break; }
            const int total = hlit + hdist;
            int i = 0, prev = 0;
            while (i < total && st.err == 0) {
                inf_refill(s, st);
                const int sy = inf_decode(s.dist, st);
                int rep = 1, val = sy;
                if (sy == 16) { rep = 3 + (int)inf_take(st, 2); val = prev; }
                else if (sy == 17) { rep = 3 + (int)inf_take(st, 3); val = 0; }
                else if (sy == 18) { rep = 11 + (int)inf_take(st, 7); val = 0; }
                if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
                if (sy < 0 || sy > 18 || (sy == 16 && i == 0) || i + rep > total) { st.err = SK_INFLATE_E_CODES; break; }
                SK_LANES {
                    for (int k = lane; k < rep; k += 64) s.lens[i + k] = (unsigned char)val;
                }
                prev = val;
                i += rep;
            }
            if (st.err) break;
            SK_SYNC();
            if (SK_UNI(s.lens[256]) == 0) { st.err = SK_INFLATE_E_CODES; break; }
            // the distance lengths follow the literal/length ones directly; the second build reads them before it
            // overwrites nothing of lens
            if (inf_build(s.lit, s.lens, hlit, kInfKindLit) != 0 || inf_build(s.dist, s.lens + hlit, hdist, kInfKindDist) != 0) {
                st.err = SK_INFLATE_E_CODES;
                break;
            }
        }

        bool eob = false;
        while (!eob && st.err == 0) {
            int n = 0;
            unsigned long long litmask = 0;
            const long long batch_start = produced;
            SK_SYNC();
            while (n < kInfBatch) {
                inf_refill(s, st);
                const int sy = inf_decode(s.lit, st);
                if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
                if (sy < 0 || sy > 285) { st.err = SK_INFLATE_E_SYMBOL; break; }
                if (sy == 256) { eob = true; break; }
                unsigned tok;
                if (sy < 256) {
                    if (produced >= out_len) { st.err = SK_INFLATE_E_OUTPUT_LONG; break; }
                    tok = (unsigned)sy << 9;
                    litmask |= 1ull << n;
                    produced += 1;
                } else {
                    int len;
                    if (sy < 265) len = sy - 254;
                    else if (sy == 285) len = 258;
                    else {
                        const int q = sy - 261, eb = q >> 2;
                        len = ((4 + (q & 3)) << eb) + 3 + (int)inf_take(st, eb);
                    }
                    inf_refill(s, st);
                    const int dc = inf_decode(s.dist, st);
                    int dist = dc + 1;
                    if (dc >= 4 && dc < 30) {
                        const int eb = (dc >> 1) - 1;
                        dist = ((2 + (dc & 1)) << eb) + 1 + (int)inf_take(st, eb);
                    }
                    if (st.bits_left < 0) { st.err = SK_INFLATE_E_INPUT; break; }
                    if (dc < 0 || dc >= 30) { st.err = SK_INFLATE_E_SYMBOL; break; }
                    if ((long long)dist > produced) { st.err = SK_INFLATE_E_DISTANCE; break; }
                    if (produced + len > out_len) { st.err = SK_INFLATE_E_OUTPUT_LONG; break; }
                    tok = (unsigned)len | (unsigned)dist << 9;
                    produced += len;
                }
                SK_LANES { if (lane == 0) s.tok[n] = tok; }
                n += 1;
            }
            inf_emit(s, out, batch_start, n, litmask);
            if (wrapper) inf_adler(s, batch_start, (int)(produced - batch_start), s1, s2);
        }
    }

    if (st.err == 0 && produced != out_len) st.err = SK_INFLATE_E_OUTPUT_SHORT;
    if (st.err == 0 && wrapper) {
        inf_take(st, (int)(st.bits_left & 7));
        inf_refill(s, st);
        const unsigned t = inf_take(st, 32);
        const unsigned want = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);   // big-endian
        if (st.bits_left < 0) st.err = SK_INFLATE_E_INPUT;
        else if (want != ((s2 << 16) | s1)) st.err = SK_INFLATE_E_ADLER;
    }
    SK_LANES { if (lane == 0) status[strm] = st.err; }
}

#ifndef SK_INFLATE_HOST
// TIFF predictor 2: every sample is stored as the difference to the same sample of the pixel before it, modulo 2^bits.
// One wave per row: lane l owns a run of consecutive pixels, sums it, the wave scans the sums, the lane adds up again.
template <typename T>
__global__ __launch_bounds__(64) void undo_predictor_kernel(T* __restrict__ rows, const int64_t n_rows, const int width,
                                                            const int spp) {
    const int lane = (int)threadIdx.x;
    const int per = (width + 63) / 64;
    const int p0 = lane * per < width ? lane * per : width;
    const int p1 = p0 + per < width ? p0 + per : width;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        T* x = rows + r * (int64_t)width * spp;
        for (int c = 0; c < spp; ++c) {
            T sum = 0;
            for (int p = p0; p < p1; ++p) sum = (T)(sum + x[(int64_t)p * spp + c]);
            T inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const T v = (T)__shfl_up((unsigned)inc, o);
                if (lane >= o) inc = (T)(inc + v);
            }
            T run = (T)(inc - sum);
            for (int p = p0; p < p1; ++p) {
                run = (T)(run + x[(int64_t)p * spp + c]);
                x[(int64_t)p * spp + c] = run;
            }
        }
    }
}
#endif

}  // namespace sk

#ifndef SK_INFLATE_HOST
extern "C" int sk_inflate_streams(const uint8_t* src, const int64_t* src_offsets, int n_streams, uint8_t* dst,
                                  const int64_t* dst_offsets, int wrapper, int32_t* status, void* stream) {
    SK_CHECK_ARG(n_streams >= 0, "sk_inflate_streams: n_streams = %d is negative", n_streams);
    SK_CHECK_ARG(wrapper == 0 || wrapper == 1, "sk_inflate_streams: wrapper = %d, must be 0 (raw) or 1 (zlib)", wrapper);
    if (n_streams == 0) return SK_OK;
    SK_CHECK_ARG(src != nullptr && dst != nullptr, "sk_inflate_streams: src or dst is NULL");
    SK_CHECK_ARG(src_offsets != nullptr && ((uintptr_t)src_offsets & 7) == 0,
                 "sk_inflate_streams: src_offsets is NULL or not 8-byte aligned");
    SK_CHECK_ARG(dst_offsets != nullptr && ((uintptr_t)dst_offsets & 7) == 0,
                 "sk_inflate_streams: dst_offsets is NULL or not 8-byte aligned");
    SK_CHECK_ARG(status != nullptr && ((uintptr_t)status & 3) == 0, "sk_inflate_streams: status is NULL or not 4-byte aligned");
    hipLaunchKernelGGL(sk::inflate_kernel, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, src, src_offsets, dst,
                       dst_offsets, wrapper, status);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

extern "C" int sk_tiff_undo_predictor(void* rows, int64_t n_rows, int row_pixels, int samples_per_pixel,
                                      int bytes_per_sample, void* stream) {
    SK_CHECK_ARG(n_rows >= 0 && n_rows <= ((int64_t)1 << 40), "sk_tiff_undo_predictor: n_rows = %lld outside [0, 2^40]",
                 (long long)n_rows);
    SK_CHECK_ARG(row_pixels >= 0 && row_pixels <= (1 << 24), "sk_tiff_undo_predictor: row_pixels = %d outside [0, 2^24]",
                 row_pixels);
    SK_CHECK_ARG(samples_per_pixel >= 1 && samples_per_pixel <= 16,
                 "sk_tiff_undo_predictor: samples_per_pixel = %d outside [1, 16]", samples_per_pixel);
    SK_CHECK_ARG(bytes_per_sample == 1 || bytes_per_sample == 2 || bytes_per_sample == 4,
                 "sk_tiff_undo_predictor: bytes_per_sample = %d, must be 1, 2 or 4", bytes_per_sample);
    if (n_rows == 0 || row_pixels == 0) return SK_OK;
    SK_CHECK_ARG(rows != nullptr && ((uintptr_t)rows & (uintptr_t)(bytes_per_sample - 1)) == 0,
                 "sk_tiff_undo_predictor: rows is NULL or not aligned to its samples");
    const unsigned grid = (unsigned)(n_rows < 65536 ? n_rows : 65536);
    hipStream_t st = (hipStream_t)stream;
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(sk::undo_predictor_kernel<uint8_t>, dim3(grid), dim3(64), 0, st, (uint8_t*)rows, n_rows, row_pixels,
                           samples_per_pixel);
    else if (bytes_per_sample == 2)
        hipLaunchKernelGGL(sk::undo_predictor_kernel<uint16_t>, dim3(grid), dim3(64), 0, st, (uint16_t*)rows, n_rows,
                           row_pixels, samples_per_pixel);
    else
        hipLaunchKernelGGL(sk::undo_predictor_kernel<uint32_t>, dim3(grid), dim3(64), 0, st, (uint32_t*)rows, n_rows,
                           row_pixels, samples_per_pixel);
    SK_CHECK_LAUNCH();
    return SK_OK;
}
#endif
