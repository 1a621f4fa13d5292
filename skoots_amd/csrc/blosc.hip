// Blosc-1 frames with the LZ4 codec: the chunks of the stores the reference's eval() writes (zarr's default compressor,
// Blosc(cname='lz4', clevel=5, shuffle=SHUFFLE), skoots/lib/eval.py:101-111), decoded where the array is wanted.  The
// reference leaves reading to zarr / numcodecs on the host; here the chunk files go to the device as they are.
//
// A frame is a 16-byte header, a table of block offsets, per block 1 or typesize "splits" (an int32 length + one LZ4
// raw block, or the bytes as they are when the length equals the expanded size), and a byte transpose per block.
//   blosc_walk          host: header and block-table checks and the walk over the split prefixes, every offset checked
//                       against the frame's length before it is used; gives the stream table and the block table
//   lz4_kernel          one wave64 workgroup per stream of the table (blosc_lz4.inc); every row is checked again
//   unshuffle_kernel    out[e * typesize + j] = in[j * ne + e] per block, 16-byte stores, 4-byte loads through LDS
//   sk_blosc_decode_host the same walk, the same decoder text compiled as host C++, a plain loop for the transpose
//
// With -DSK_BLOSC_HOST this file compiles as plain host C++ without the device half (tools/blosc_host_check.cpp).
#include <stdint.h>
#include <string.h>

#include <new>

#ifndef SK_BLOSC_HOST
#include "common.h"

#define SK_LZ4_NS sk_lz4_dev
#define SK_LZ4_FN __device__
#define SK_LANES for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define SK_LI 0                 // index of a lane's slot in a per-lane temporary
#define SK_NL 1
#define SK_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#define SK_SYNC() __syncthreads()
#include "blosc_lz4.inc"
#undef SK_LZ4_NS
#undef SK_LZ4_FN
#undef SK_LANES
#undef SK_LI
#undef SK_NL
#undef SK_UNI
#undef SK_SYNC
#else
#include "../../include/skoots_hip.h"
#endif

#define SK_LZ4_NS sk_lz4_host
#define SK_LZ4_FN static
#define SK_LANES for (int lane = 0; lane < 64; ++lane)
#define SK_LI lane
#define SK_NL 64
#define SK_UNI(x) ((int)(x))
#define SK_SYNC()
#include "blosc_lz4.inc"
#undef SK_LZ4_NS
#undef SK_LZ4_FN
#undef SK_LANES
#undef SK_LI
#undef SK_NL
#undef SK_UNI
#undef SK_SYNC

namespace sk {

// ------------------------------------------------------------------------------------------------ the frame walk
struct BloscFrame {
    int typesize;
    bool shuffle, memcpyed;
    long long nbytes, blocksize, nblocks;
};

static inline long long blosc_le32(const uint8_t* p) {
    return (long long)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

// The header of a frame that must expand to dst_bytes.  0 or SK_BLOSC_E_HEADER / SK_BLOSC_E_CODEC.
static int blosc_header(const uint8_t* frame, long long frame_bytes, long long dst_bytes, BloscFrame& f) {
    if (frame_bytes < 16 || frame[0] != 2) return SK_BLOSC_E_HEADER;
    const unsigned flags = frame[2];
    f.typesize = frame[3];
    f.nbytes = blosc_le32(frame + 4);
    f.blocksize = blosc_le32(frame + 8);
    const long long cbytes = blosc_le32(frame + 12);
    if (cbytes != frame_bytes || f.nbytes != dst_bytes || f.typesize == 0) return SK_BLOSC_E_HEADER;
    if (f.nbytes > 0 && f.blocksize == 0) return SK_BLOSC_E_HEADER;
    f.memcpyed = (flags & 0x02u) != 0;
    f.shuffle = (flags & 0x01u) != 0 && f.typesize > 1;
    if (flags & 0x04u) return SK_BLOSC_E_CODEC;                        // bitshuffle
    if (!f.memcpyed && (flags >> 5) != 1u) return SK_BLOSC_E_CODEC;    // blosclz, snappy, zlib, zstd
    if (!f.memcpyed && f.shuffle && f.typesize > 16) return SK_BLOSC_E_CODEC;
    f.nblocks = f.nbytes == 0 ? 0 : (f.nbytes + f.blocksize - 1) / f.blocksize;
    if (f.memcpyed) {
        if (frame_bytes - 16 < f.nbytes) return SK_BLOSC_E_FRAME;
        f.nblocks = 0;
        return 0;
    }
    if ((frame_bytes - 16) / 4 < f.nblocks) return SK_BLOSC_E_FRAME;   // the block table itself
    return 0;
}

// Walks a frame.  streams (cap_streams rows of 5) and blocks (cap_blocks rows of 2: begin, bytes of every block that
// is byte-shuffled) are filled as far as the capacities reach; counts = rows wanted of each, typesize, 1 if the
// streams' output still has to be unshuffled.  All offsets are relative to the frame / to its output.
static int blosc_walk(const uint8_t* frame, long long frame_bytes, long long dst_bytes, int64_t* streams,
                      long long cap_streams, int64_t* blocks, long long cap_blocks, int64_t* counts) {
    BloscFrame f;
    const int rc = blosc_header(frame, frame_bytes, dst_bytes, f);
    if (rc != 0) return rc;
    long long ns = 0, nb = 0;
    auto put = [&](long long sb, long long sl, long long db, long long dl, long long kind) {
        if (ns < cap_streams) {
            int64_t* r = streams + 5 * ns;
            r[0] = sb, r[1] = sl, r[2] = db, r[3] = dl, r[4] = kind;
        }
        ns += 1;
    };
    if (f.memcpyed) {
        if (f.nbytes > 0) put(16, f.nbytes, 0, f.nbytes, SK_LZ4_KIND_STORED);
    } else {
        const bool dont_split = (frame[2] & 0x10u) != 0;
        for (long long b = 0; b < f.nblocks; ++b) {
            const long long begin = b * f.blocksize;
            const long long bytes = f.nbytes - begin < f.blocksize ? f.nbytes - begin : f.blocksize;
            const bool split = !dont_split && f.typesize <= 16 && f.blocksize / f.typesize >= 128 && bytes == f.blocksize;
            const long long nsplits = split ? f.typesize : 1;
            if (bytes % nsplits != 0) return SK_BLOSC_E_FRAME;
            const long long each = bytes / nsplits;
            long long at = (long long)(int32_t)(uint32_t)blosc_le32(frame + 16 + 4 * b);
            if (at < 16 + 4 * f.nblocks || at > frame_bytes) return SK_BLOSC_E_FRAME;
            for (long long j = 0; j < nsplits; ++j) {
                if (frame_bytes - at < 4) return SK_BLOSC_E_FRAME;
                const long long csize = (long long)(int32_t)(uint32_t)blosc_le32(frame + at);
                at += 4;
                if (csize < 0 || csize > frame_bytes - at) return SK_BLOSC_E_FRAME;
                put(at, csize, begin + j * each, each, csize == each ? SK_LZ4_KIND_STORED : SK_LZ4_KIND_LZ4);
                at += csize;
            }
            if (f.shuffle) {
                if (nb < cap_blocks) blocks[2 * nb] = begin, blocks[2 * nb + 1] = bytes;
                nb += 1;
            }
        }
    }
    counts[0] = ns, counts[1] = nb, counts[2] = f.typesize, counts[3] = nb > 0 ? 1 : 0;
    return 0;
}

#ifndef SK_BLOSC_HOST
// ------------------------------------------------------------------------------------------------ device
__global__ __launch_bounds__(64) void lz4_kernel(const uint8_t* __restrict__ src, const long long src_bytes,
                                                 const int64_t* __restrict__ table, uint8_t* __restrict__ dst,
                                                 const long long dst_bytes, int32_t* __restrict__ status) {
    __shared__ sk_lz4_dev::Lz4Lds s;
    const int64_t* row = table + 5 * (int64_t)blockIdx.x;
    const int rc = sk_lz4_dev::lz4_stream(s, src, src_bytes, row[0], row[1], row[2], row[3], row[4], dst, dst_bytes);
    if (threadIdx.x == 0) status[blockIdx.x] = rc;
}

constexpr int kUnshThreads = 256;
constexpr int kUnshTile = kUnshThreads * 16;            // output bytes per step of a workgroup
constexpr int kUnshLds = (kUnshTile + 8 * 16) / 4;     // dwords: typesize planes of kUnshTile / typesize + 8 bytes at most
constexpr int kUnshGridY = 32;

// Byte un-transpose of every block: out[e * ts + j] = in[j * ne + e], ne = bytes / ts; the bytes % ts tail bytes are
// copied.  The write side is the coalesced one: the block's output is cut at the 16-byte boundaries of its address, a
// thread owns one such 16-byte line and stores it with one instruction (bytewise where a line reaches past either
// end of the block).  The ts byte planes a step needs are loaded into LDS with aligned 4-byte loads (bytewise where
// a dword reaches past either end of the block), so nothing outside the block is read in src or written in dst.
__global__ __launch_bounds__(kUnshThreads) void unshuffle_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                const int64_t* __restrict__ blocks, const int ts) {
    __shared__ unsigned lds[kUnshLds];
    const long long begin = blocks[2 * (int64_t)blockIdx.x], bytes = blocks[2 * (int64_t)blockIdx.x + 1];
    if (begin < 0 || bytes <= 0) return;
    const long long ne = bytes / ts, body = ne * ts;
    const int pl = ((kUnshTile / ts + 2 + 3) + 3) & ~3;        // bytes of one plane in LDS
    const unsigned char* l8 = (const unsigned char*)lds;
    const unsigned long long in0 = (unsigned long long)(uintptr_t)src + (unsigned long long)begin, in1 = in0 + (unsigned long long)bytes;
    const unsigned long long out0 = (unsigned long long)(uintptr_t)dst + (unsigned long long)begin;
    const long long first = -(long long)(out0 & 15ull);         // output offset of the first 16-byte line (<= 0)
    const long long tiles = (bytes - first + kUnshTile - 1) / kUnshTile;
    for (long long t = blockIdx.y; t < tiles; t += gridDim.y) {
        const long long o_lo = first + t * kUnshTile;
        long long o0 = o_lo < 0 ? 0 : o_lo, o1 = o_lo + kUnshTile < body ? o_lo + kUnshTile : body;
        __syncthreads();
        if (o0 < o1) {
            const long long e_lo = o0 / ts, e_hi = (o1 - 1) / ts + 1;
            for (int j = 0; j < ts; ++j) {
                const unsigned long long a = in0 + (unsigned long long)(j * ne + e_lo);      // first byte wanted of plane j
                const unsigned long long a4 = a & ~3ull;
                const int nd = (int)(((a - a4) + (unsigned long long)(e_hi - e_lo) + 3) >> 2);
                for (int d = (int)threadIdx.x; d < nd; d += kUnshThreads) {
                    const unsigned long long q = a4 + 4ull * (unsigned)d;
                    unsigned v = 0;
                    if (q >= in0 && q + 4 <= in1) {
                        v = *(const unsigned*)(uintptr_t)q;
                    } else {
                        for (int b = 0; b < 4; ++b)
                            if (q + b >= in0 && q + b < in1) v |= (unsigned)(*(const uint8_t*)(uintptr_t)(q + b)) << (8 * b);
                    }
                    lds[(j * pl >> 2) + d] = v;
                }
            }
        }
        __syncthreads();
        const long long o = o_lo + 16 * (long long)threadIdx.x;
        if (o + 16 <= 0 || o >= bytes) continue;
        const long long e_lo = o0 / ts;
        const unsigned base3 = (unsigned)((in0 + (unsigned long long)e_lo) & 3ull), ne3 = (unsigned)(ne & 3);
        unsigned char v[16];
        int er = -1, j = 0;                  // element (counted from e_lo) and plane of the byte at hand; one division
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const long long p = o + b;
            unsigned char x = 0;
            if (p >= 0 && p < body) {
                if (er < 0) {
                    const unsigned r = (unsigned)(p - e_lo * ts);
                    er = (int)(r / (unsigned)ts);
                    j = (int)(r - (unsigned)er * (unsigned)ts);
                }
                x = l8[j * pl + (int)((base3 + (unsigned)j * ne3) & 3u) + er];
                if (++j == ts) j = 0, ++er;
            } else if (p >= body && p < bytes) {
                x = *(const uint8_t*)(uintptr_t)(in0 + (unsigned long long)p);
            }
            v[b] = x;
        }
        uint8_t* to = (uint8_t*)(uintptr_t)(out0 + (unsigned long long)o);   // o may be negative: wraps to before out0
        if (o >= 0 && o + 16 <= bytes) {
            uint4 w;
            w.x = v[0] | v[1] << 8 | v[2] << 16 | (unsigned)v[3] << 24;
            w.y = v[4] | v[5] << 8 | v[6] << 16 | (unsigned)v[7] << 24;
            w.z = v[8] | v[9] << 8 | v[10] << 16 | (unsigned)v[11] << 24;
            w.w = v[12] | v[13] << 8 | v[14] << 16 | (unsigned)v[15] << 24;
            *(uint4*)to = w;
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (o + b >= 0 && o + b < bytes) to[b] = v[b];
        }
    }
}
#endif

}  // namespace sk

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int sk_blosc_plan_host(const uint8_t* frame, int64_t frame_bytes, int64_t dst_bytes, int64_t* streams,
                                  int64_t cap_streams, int64_t* blocks, int64_t cap_blocks, int64_t* counts,
                                  int32_t* status) {
    if (frame == nullptr || frame_bytes < 0 || dst_bytes < 0 || cap_streams < 0 || cap_blocks < 0 || counts == nullptr ||
        status == nullptr || (cap_streams > 0 && streams == nullptr) || (cap_blocks > 0 && blocks == nullptr))
        return SK_ERR_ARG;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    *status = sk::blosc_walk(frame, frame_bytes, dst_bytes, streams, cap_streams, blocks, cap_blocks, counts);
    return SK_OK;
}

extern "C" int sk_blosc_decode_host(const uint8_t* frame, int64_t frame_bytes, uint8_t* dst, int64_t dst_bytes,
                                    int32_t* status) {
    if (frame == nullptr || frame_bytes < 0 || dst_bytes < 0 || status == nullptr || (dst_bytes > 0 && dst == nullptr))
        return SK_ERR_ARG;
    int64_t counts[4] = {0, 0, 0, 0};
    *status = sk::blosc_walk(frame, frame_bytes, dst_bytes, nullptr, 0, nullptr, 0, counts);
    if (*status != 0) return SK_OK;
    const int64_t ns = counts[0], nb = counts[1];
    const int ts = (int)counts[2];
    int64_t* streams = new (std::nothrow) int64_t[5 * ns + 2 * nb + 1];
    sk_lz4_host::Lz4Lds* lds = new (std::nothrow) sk_lz4_host::Lz4Lds;
    uint8_t* tmp = nb > 0 ? new (std::nothrow) uint8_t[dst_bytes] : nullptr;
    int rc = SK_OK;
    if (streams == nullptr || lds == nullptr || (nb > 0 && tmp == nullptr)) {
        rc = SK_ERR_CAPACITY;
    } else {
        int64_t* blocks = streams + 5 * ns;
        sk::blosc_walk(frame, frame_bytes, dst_bytes, streams, ns, blocks, nb, counts);
        uint8_t* to = nb > 0 ? tmp : dst;            // shuffled frames expand next to dst and are transposed into it
        for (int64_t i = 0; i < ns && *status == 0; ++i) {
            const int64_t* r = streams + 5 * i;
            *status = sk_lz4_host::lz4_stream(*lds, frame, frame_bytes, r[0], r[1], r[2], r[3], r[4], to, dst_bytes);
        }
        for (int64_t b = 0; b < nb && *status == 0; ++b) {
            const int64_t begin = blocks[2 * b], bytes = blocks[2 * b + 1], ne = bytes / ts;
            const uint8_t* in = tmp + begin;
            uint8_t* out = dst + begin;
            for (int j = 0; j < ts; ++j)
                for (int64_t e = 0; e < ne; ++e) out[e * ts + j] = in[j * ne + e];
            for (int64_t p = ne * ts; p < bytes; ++p) out[p] = in[p];
        }
    }
    delete[] streams;
    delete lds;
    delete[] tmp;
    return rc;
}

#ifndef SK_BLOSC_HOST
extern "C" int sk_lz4_streams(const uint8_t* src, int64_t src_bytes, const int64_t* table, int n_streams, uint8_t* dst,
                              int64_t dst_bytes, int32_t* status, void* stream) {
    SK_CHECK_ARG(n_streams >= 0, "sk_lz4_streams: n_streams = %d is negative", n_streams);
    SK_CHECK_ARG(src_bytes >= 0 && dst_bytes >= 0, "sk_lz4_streams: src_bytes = %lld or dst_bytes = %lld is negative",
                 (long long)src_bytes, (long long)dst_bytes);
    if (n_streams == 0) return SK_OK;
    SK_CHECK_ARG(src != nullptr && dst != nullptr, "sk_lz4_streams: src or dst is NULL");
    SK_CHECK_ARG(table != nullptr && ((uintptr_t)table & 7) == 0, "sk_lz4_streams: table is NULL or not 8-byte aligned");
    SK_CHECK_ARG(status != nullptr && ((uintptr_t)status & 3) == 0, "sk_lz4_streams: status is NULL or not 4-byte aligned");
    hipLaunchKernelGGL(sk::lz4_kernel, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, src, (long long)src_bytes,
                       table, dst, (long long)dst_bytes, status);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

extern "C" int sk_blosc_unshuffle(const uint8_t* src, uint8_t* dst, const int64_t* blocks, int n_blocks, int typesize,
                                  void* stream) {
    SK_CHECK_ARG(n_blocks >= 0, "sk_blosc_unshuffle: n_blocks = %d is negative", n_blocks);
    SK_CHECK_ARG(typesize >= 2 && typesize <= 16, "sk_blosc_unshuffle: typesize = %d outside [2, 16]", typesize);
    if (n_blocks == 0) return SK_OK;
    SK_CHECK_ARG(src != nullptr && dst != nullptr && src != dst, "sk_blosc_unshuffle: src or dst is NULL, or they are the same");
    SK_CHECK_ARG(blocks != nullptr && ((uintptr_t)blocks & 7) == 0, "sk_blosc_unshuffle: blocks is NULL or not 8-byte aligned");
    hipLaunchKernelGGL(sk::unshuffle_kernel, dim3((unsigned)n_blocks, sk::kUnshGridY), dim3(sk::kUnshThreads), 0,
                       (hipStream_t)stream, src, dst, blocks, typesize);
    SK_CHECK_LAUNCH();
    return SK_OK;
}
#endif
