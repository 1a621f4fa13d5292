// The LZ4 raw-block decoder of blosc.hip, written once as "uniform code + lane sections" (the SK_LANES scheme of
// inflate.hip) and included twice by blosc.hip: as the device code of lz4_kernel (a lane section runs once with
// lane = threadIdx.x) and as host C++ (a lane section is a loop over the 64 lanes), which is what
// sk_blosc_decode_host runs and what tools/blosc_host_check.cpp puts under AddressSanitizer / UBSan.
//
// The includer defines: SK_LZ4_NS (namespace), SK_LZ4_FN (function qualifiers), SK_LANES, SK_LI, SK_NL, SK_UNI, SK_SYNC.
//
// One wave decodes one stream.  The parse state (input position, output position, error) is the same in every lane;
// the bytes it looks at come out of a 4 KiB window of the stream in LDS, loaded by all lanes with every byte checked
// against the stream's range.  A literal run is copied by all lanes from the stream to dst and into the ring; a match
// is copied by all lanes, 64 bytes a step, from the ring to dst and the ring.  Nothing is read back from dst.
//
// The ring: 64 KiB of output in LDS, position p in slot p & 65535.  A match of offset `off` at output position `pos`
// is copied in steps of 64 bytes; in the step that writes [pos + c0, pos + c0 + 64) lane l reads position
// pos + c0 - off + l % off.  For c0 = 0 that is base + l % off, the overlapping-match rule; for the later steps it is
// the same byte value (the output is periodic in off from pos - off on) taken from the copy that lies nearest before
// the step, so every read lies in [pos + c0 - off, pos + c0): at most 65 535 bytes back however long the match is.
// A slot is overwritten only by the position 65 536 after it, and everything written so far lies before pos + c0, so
// no slot a step reads has been overwritten.  All lanes of a step read before any of them writes.
//
// Every bound is checked before the copy it guards: a literal run against the end of the stream and of dst, an offset
// against the bytes produced, a match against the end of dst.  A data error is a status code; there is no assert and no
// trap.  Every turn of every loop consumes at least one input byte or ends on an error, and running out of input is an
// error, so every loop ends.

namespace SK_LZ4_NS {

constexpr int kLz4Ring = 65536;                 // bytes of output kept in LDS: the largest offset is 65 535
constexpr int kLz4Win = 1024;                   // dwords of input in LDS

struct Lz4Lds {
    unsigned ring[kLz4Ring / 4];
    unsigned win[kLz4Win];
};

// wave-uniform reader state
struct Lz4In {
    unsigned long long a0, lo, hi;              // addresses: stream = [lo, hi), a0 = lo rounded down to 4
    long long wbase;                            // first dword (counted from a0) in the window; -1 = nothing loaded
};

SK_LZ4_FN inline void lz4_load_window(Lz4Lds& s, const Lz4In& in) {
    SK_SYNC();
    SK_LANES {
        for (int j = lane; j < kLz4Win; j += 64) {
            const unsigned long long a = in.a0 + 4ull * (unsigned long long)(in.wbase + j);
            unsigned v = 0;
            if (a >= in.lo && a + 4 <= in.hi) {
                v = *(const unsigned*)(uintptr_t)a;
            } else if (a < in.hi) {
                for (int b = 0; b < 4; ++b)
                    if (a + b >= in.lo && a + b < in.hi) v |= (unsigned)(*(const uint8_t*)(uintptr_t)(a + b)) << (8 * b);
            }
            s.win[j] = v;
        }
    }
    SK_SYNC();
}

// byte `pos` of the stream; the caller has checked 0 <= pos < length
SK_LZ4_FN inline unsigned lz4_byte(Lz4Lds& s, Lz4In& in, long long pos) {
    const unsigned long long r = (in.lo - in.a0) + (unsigned long long)pos;
    const long long d = (long long)(r >> 2);
    if (in.wbase < 0 || d < in.wbase || d - in.wbase >= kLz4Win) {
        in.wbase = d;
        lz4_load_window(s, in);
    }
    const unsigned w = (unsigned)SK_UNI(s.win[(int)(d - in.wbase)]);
    return (w >> (8 * (unsigned)(r & 3u))) & 255u;
}

// One row of the stream table: src[row[0] .. + row[1]) -> dst[row[2] .. + row[3]), row[4] = kind.  Returns 0 or an
// SK_LZ4_E_* code.  Reads nothing outside the row's src range and writes nothing outside its dst range.
SK_LZ4_FN inline int lz4_stream(Lz4Lds& s, const uint8_t* src, const long long src_bytes, const long long sb,
                                const long long sl, const long long db, const long long dl, const long long kind,
                                uint8_t* dst, const long long dst_bytes) {
    if (sb < 0 || sl < 0 || sb > src_bytes || sl > src_bytes - sb) return SK_LZ4_E_RANGE;
    if (db < 0 || dl < 0 || db > dst_bytes || dl > dst_bytes - db) return SK_LZ4_E_RANGE;
    if (kind != SK_LZ4_KIND_LZ4 && kind != SK_LZ4_KIND_STORED) return SK_LZ4_E_RANGE;
    const uint8_t* from = src + sb;
    uint8_t* out = dst + db;
    if (kind == SK_LZ4_KIND_STORED) {
        if (sl != dl) return SK_LZ4_E_RANGE;
        SK_LANES {
#pragma unroll 4
            for (long long k = lane; k < dl; k += 64) out[k] = from[k];
        }
        return 0;
    }
    unsigned char* ring = (unsigned char*)s.ring;
    Lz4In in;
    in.lo = (unsigned long long)(uintptr_t)from;
    in.hi = in.lo + (unsigned long long)sl;
    in.a0 = in.lo & ~3ull;
    in.wbase = -1;
    long long ip = 0, op = 0;
    for (;;) {
        if (ip >= sl) return SK_LZ4_E_INPUT;                 // no token: empty, or the stream ended right after a match
        const unsigned token = lz4_byte(s, in, ip++);
        long long lit = (long long)(token >> 4);
        if (lit == 15) {
            unsigned b;
            do {
                if (ip >= sl) return SK_LZ4_E_INPUT;
                b = lz4_byte(s, in, ip++);
                lit += (long long)b;
            } while (b == 255u);
        }
        if (lit > sl - ip) return SK_LZ4_E_INPUT;
        if (lit > dl - op) return SK_LZ4_E_OUTPUT_LONG;
        if (lit > 0) {
            SK_LANES {
#pragma unroll 4
                for (long long k = lane; k < lit; k += 64) {
                    const unsigned char b = from[ip + k];
                    ring[(unsigned)(op + k) & (kLz4Ring - 1)] = b;
                    out[op + k] = b;
                }
            }
            SK_SYNC();            // the next step may be a match whose lanes read these bytes from the ring
            ip += lit;
            op += lit;
        }
        if (ip == sl) return op == dl ? 0 : SK_LZ4_E_OUTPUT_SHORT;   // the last sequence ends after its literals
        if (sl - ip < 2) return SK_LZ4_E_INPUT;
        const unsigned o0 = lz4_byte(s, in, ip), o1 = lz4_byte(s, in, ip + 1);
        ip += 2;
        const long long off = (long long)(o0 | (o1 << 8));
        if (off == 0 || off > op) return SK_LZ4_E_OFFSET;
        long long len = (long long)(token & 15u);
        if (len == 15) {
            unsigned b;
            do {
                if (ip >= sl) return SK_LZ4_E_INPUT;
                b = lz4_byte(s, in, ip++);
                len += (long long)b;
            } while (b == 255u);
        }
        len += 4;
        if (len > dl - op) return SK_LZ4_E_OUTPUT_LONG;
        const int ioff = (int)off;
        for (long long c0 = 0; c0 < len; c0 += 64) {
            unsigned char v[SK_NL];
            SK_LANES {
                if (c0 + lane < len) {
                    const int back = lane < ioff ? lane : lane % ioff;
                    v[SK_LI] = ring[(unsigned)(op + c0 - off + back) & (kLz4Ring - 1)];
                }
            }
            SK_SYNC();
            SK_LANES {
                if (c0 + lane < len) {
                    ring[(unsigned)(op + c0 + lane) & (kLz4Ring - 1)] = v[SK_LI];
                    out[op + c0 + lane] = v[SK_LI];
                }
            }
            SK_SYNC();
        }
        op += len;
    }
}

}  // namespace SK_LZ4_NS
