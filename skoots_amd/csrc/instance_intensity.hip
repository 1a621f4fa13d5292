// The image under every instance in one pass: voxel count, the sums of v, v^2, v x, v y, v z, the
// smallest and largest sample and a 256-bin histogram of the image samples v under every instance of a mask.  The
// reference has no such step; like contacts() this is ground the project defines for itself.
//
// Shape of the kernel
//   * A workgroup takes a tile of kTX x kTY x kTZ voxels (the tile of instance_stats.hip, no halo) and strides over the
//     tiles.  A wave owns 16 of the tile's 64 z rows, lanes = consecutive z.  It loads the labels of all 16 rows into
//     registers first, coalesced 256-byte lines with the lut applied once per voxel, so 16 loads and 16 look-ups are in
//     flight per lane.  The image tile is staged in LDS by the whole workgroup with 32-bit loads (four 8-bit or two
//     16-bit samples per lane and instruction) whenever rows start on 4-byte boundaries, by single samples otherwise.
//   * A maximal run of one row along the lanes is reduced by segmented inclusive wave scans (__shfl_up) of v, v^2,
//     v z_local, min and max.  The sums of an 8-bit image travel packed in one 64-bit word, those of a 16-bit image in
//     two; min and max share one 32-bit word.  The steps stop at the longest run of the wave row (at most 6; a row of
//     specks takes none).  The run's LAST lane holds the totals and adds
//     n, S v, S v^2, x S v, y S v, z_tile S v + S v z_local to a small table in LDS keyed by row (kSlots slots, open
//     addressing, at most kProbes probes; the run's first lane claims the slot and the run shares it).  A run whose row
//     finds no slot adds to global memory directly.
//   * Histogram: kSlots x 256 16-bit counters in LDS, two to a 32-bit word (a tile holds 4096 voxels, so no counter
//     carries into its neighbour): 16 KiB, which leaves room for five to seven workgroups on a compute unit where
//     32-bit counters left three or four.  Every instance voxel does one LDS atomic add; when all instance voxels of a
//     wave row fall into one counter -- a constant image under one run -- one lane adds their number instead of 64
//     lanes queueing on one address.  A voxel whose row has no slot adds to the global histogram directly.  Compiled
//     out when the caller passes no histogram (the ring pass).
//   * Flush once per tile, only the slots in use: non-zero entries go out with 64-bit global atomic adds and 32-bit
//     atomic min / max, and the flush leaves the counters zero for the next tile.
//   * Integer atomics only: every result is exact and independent of the order of arrival.
//
// gfx950 build (hipcc -O3, ROCm 7.0), VGPRs / LDS bytes / scratch bytes per kernel:
//   8-bit  with histogram  80 / 22400 / 0     without  70 /  6016 / 0
//   16-bit with histogram  80 / 26496 / 0     without  72 / 10112 / 0
#include "instance_rows.h"

#include <limits.h>

namespace {

constexpr int kTX = 4, kTY = 16, kTZ = 64;            // tile; kTZ is the wave width: one lane per z
constexpr int kRows = kTX * kTY;                      // z rows of a tile
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPerWave = kRows / kWaves;              // z rows a wave owns: 16
constexpr int kSlotBits = 5, kSlots = 1 << kSlotBits;  // rows the LDS tables hold per tile
constexpr int kProbes = 8;                            // linear probes before a run goes to global memory
constexpr int kMom = 6, kExt = 2, kBins = 256;
constexpr int kHistWords = kBins / 2;                 // a 32-bit word of the LDS histogram holds two bins

static_assert(kTZ == 64, "one lane per z of the tile");
static_assert(kTY == 16 && kWaves == 4, "row k of wave w is (k / 4, w + 4 (k % 4))");
static_assert(kHistWords <= kThreads, "the flush gives one word of two bins to a thread");
static_assert(kTX * kTY * kTZ < (1 << 16), "a 16-bit counter holds a tile's voxels");
static_assert(kSlots * kMom <= kThreads, "the reset gives one accumulator to each thread");

typedef unsigned long long u64;

// the larger of each 16-bit half (v_pk_max_u16)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ inline unsigned pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

template <typename T, bool kHist>
__global__ void __launch_bounds__(kThreads) instance_intensity_kernel(
    const int* __restrict__ lab, int X, int Y, int Z, const int* __restrict__ lut, int max_id, int N, long long ntiles,
    int tiles_y, int tiles_z, const T* __restrict__ img, int wide, int shift, u64* __restrict__ moments,
    int* __restrict__ extrema, u64* __restrict__ hist) {
    constexpr int kE = (int)sizeof(T), kPer = 4 / kE;      // samples per 32-bit word
    constexpr int kW = kTZ / kPer;                        // words per z row of the tile
    __shared__ unsigned s_img[kRows * kW];                // the image tile, row-major: 4 KiB (8-bit) or 8 KiB (16-bit)
    __shared__ unsigned s_hist[kHist ? kSlots * kHistWords : 1];   // two 16-bit counters per word: a tile has 4096 voxels
    __shared__ u64 s_mom[kSlots * kMom];
    __shared__ int s_ext[kSlots * kExt];
    __shared__ int s_key[kSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (kHist)
        for (int i = tid; i < kSlots * kHistWords; i += kThreads) s_hist[i] = 0;
    if (tid < kSlots * kMom) s_mom[tid] = 0;
    if (tid < kSlots * kExt) s_ext[tid] = (tid & 1) ? -1 : INT_MAX;
    if (tid < kSlots) s_key[tid] = 0;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tz0 = (int)(t % tiles_z) * kTZ, y0 = (int)(t / tiles_z % tiles_y) * kTY;
        const int x0 = (int)(t / ((long long)tiles_z * tiles_y)) * kTX;
        int a[kPerWave];                                   // the rows of this wave's 16 z rows, 0 for background
#pragma unroll
        for (int k = 0; k < kPerWave; ++k) {
            const int x = x0 + (k >> 2), y = y0 + wave + 4 * (k & 3), z = tz0 + lane;
            a[k] = (x < X && y < Y && z < Z) ? sk::row_of(lab[((long long)x * Y + y) * Z + z], lut, max_id, N) : 0;
        }
        // the previous tile's readers of s_img passed the barrier before its flush
        if (wide) {                                        // rows start on 4-byte boundaries: whole words
            for (int i = tid; i < kRows * kW; i += kThreads) {
                const int row = i / kW, w = i % kW;
                const int x = x0 + (row >> 4), y = y0 + (row & 15), z = tz0 + w * kPer;
                unsigned word = 0;
                if (x < X && y < Y && z < Z)               // Z is a multiple of kPer here: the word lies inside the row
                    word = *(const unsigned*)(img + (((long long)x * Y + y) * Z + z));
                s_img[i] = word;
            }
        } else {
            T* si = (T*)s_img;
            for (int i = tid; i < kRows * kTZ; i += kThreads) {
                const int row = i >> 6;
                const int x = x0 + (row >> 4), y = y0 + (row & 15), z = tz0 + (i & 63);
                si[i] = (x < X && y < Y && z < Z) ? img[((long long)x * Y + y) * Z + z] : (T)0;
            }
        }
        __syncthreads();

#pragma unroll
        for (int k = 0; k < kPerWave; ++k) {               // wave-uniform: every lane reaches the shuffles
            const int av = a[k];
            const bool valid = av > 0;
            const u64 vmask = __ballot(valid);
            if (vmask == 0) continue;                      // wave-uniform
            const int ix = k >> 2, iy = wave + 4 * (k & 3);
            const unsigned v = valid ? (unsigned)((const T*)s_img)[(ix * kTY + iy) * kTZ + lane] : 0u;
            const int prev = __shfl_up(av, 1);
            const bool cont = valid && lane > 0 && prev == av;
            const u64 cmask = __ballot(cont);
            const u64 starts = vmask & ~cmask;             // the first lane of every run
            const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
            const int head = 63 - __builtin_clzll((starts & upto) | 1ull);     // of this lane's run, if it is in one
            const bool last = valid && (lane == 63 || !((cmask >> (lane + 1)) & 1ull));
            int s = -1;
            if (valid && !cont) s = sk::claim_slot<kSlotBits, kProbes>(s_key, av);
            s = __shfl(s, head);                           // the run shares its first lane's slot
            // Segmented inclusive scans.  Bit L of `reach` says that lane L - d lies in lane L's run: cmask at d = 1, and
            // reach & (reach << d) at 2 d.  It is wave-uniform, so the steps end with the longest run of the row.  The
            // sums travel packed (no field can carry into the next: the bounds are those of a whole wave row), min and
            // max as one word of two 16-bit maxima, 65535 - min in the low half.
            u64 reach = cmask;
            unsigned ext = valid ? (v << 16 | (0xFFFFu - v)) : 0u;
            unsigned sv, svz;
            u64 svv;
            if constexpr (kE == 1) {
                // S v <= 64 * 255 at bit 44, S v z_local <= 2016 * 255 < 2^20 at bit 24, S v^2 <= 64 * 255^2 < 2^24 at bit 0
                u64 p = (u64)v << 44 | (u64)(v * (unsigned)lane) << 24 | (u64)(v * v);
#pragma unroll
                for (int d = 1; d < 64 && reach; d <<= 1) {
                    const u64 up = __shfl_up(p, d);
                    const unsigned ue = __shfl_up(ext, d);
                    if ((reach >> lane) & 1ull) {
                        p += up;
                        ext = pk_max_u16(ext, ue);
                    }
                    reach &= reach << d;
                }
                sv = (unsigned)(p >> 44), svz = (unsigned)(p >> 24) & 0xFFFFFu, svv = p & 0xFFFFFFull;
            } else {
                // S v <= 64 * 65535 < 2^22 in the high word, S v z_local <= 2016 * 65535 < 2^27 in the low word
                u64 p = (u64)v << 32 | (u64)(v * (unsigned)lane);
                svv = (u64)v * v;
#pragma unroll
                for (int d = 1; d < 64 && reach; d <<= 1) {
                    const u64 up = __shfl_up(p, d), uq = __shfl_up(svv, d);
                    const unsigned ue = __shfl_up(ext, d);
                    if ((reach >> lane) & 1ull) {
                        p += up;
                        svv += uq;
                        ext = pk_max_u16(ext, ue);
                    }
                    reach &= reach << d;
                }
                sv = (unsigned)(p >> 32), svz = (unsigned)p;
            }
            const int mn = 0xFFFF - (int)(ext & 0xFFFFu), mx = (int)(ext >> 16);
            if (kHist) {
                const unsigned b = v >> shift;
                const int bin = (int)(b < (unsigned)kBins ? b : (unsigned)(kBins - 1));
                const int key = (s << 8) | bin;
                const bool local = valid && s >= 0;
                const int lead = __ffsll((unsigned long long)vmask) - 1;
                const int key0 = __shfl(key, lead);
                if (__ballot(local && key == key0) == vmask) {      // wave-uniform: one counter takes them all
                    if (lane == lead) atomicAdd(&s_hist[key0 >> 1], (unsigned)__popcll(vmask) << 16 * (key0 & 1));
                } else if (local) {
                    atomicAdd(&s_hist[key >> 1], 1u << 16 * (key & 1));
                } else if (valid) {                        // the table is full for this row: global memory directly
                    atomicAdd(&hist[(long long)(av - 1) * kBins + bin], 1ull);
                }
            }
            if (!last) continue;
            const u64 usv = sv;
            const u64 m[kMom] = {(u64)(lane - head + 1), usv, svv, (u64)(x0 + ix) * usv, (u64)(y0 + iy) * usv,
                                 (u64)tz0 * usv + svz};
            if (s >= 0) {
#pragma unroll
                for (int j = 0; j < kMom; ++j)
                    if (m[j]) atomicAdd(&s_mom[s * kMom + j], m[j]);
                atomicMin(&s_ext[s * kExt + 0], mn);
                atomicMax(&s_ext[s * kExt + 1], mx);
            } else {                                       // the table is full for this row: global memory directly
#pragma unroll
                for (int j = 0; j < kMom; ++j)
                    if (m[j]) atomicAdd(&moments[(long long)(av - 1) * kMom + j], m[j]);
                atomicMin(&extrema[(long long)(av - 1) * kExt + 0], mn);
                atomicMax(&extrema[(long long)(av - 1) * kExt + 1], mx);
            }
        }
        __syncthreads();
        for (int s = 0; s < kSlots; ++s) {                 // flush: only the slots in use; block-uniform
            const int key = s_key[s];
            if (key == 0) continue;
            if (kHist && tid < kHistWords) {
                const unsigned c = s_hist[s * kHistWords + tid];
                if (c) {
                    u64* g = hist + (long long)(key - 1) * kBins + 2 * tid;
                    if (c & 0xFFFFu) atomicAdd(&g[0], (u64)(c & 0xFFFFu));
                    if (c >> 16) atomicAdd(&g[1], (u64)(c >> 16));
                    s_hist[s * kHistWords + tid] = 0;      // zero again for the next tile
                }
            }
            if (tid < kMom) {
                const u64 v = s_mom[s * kMom + tid];
                if (v) atomicAdd(&moments[(long long)(key - 1) * kMom + tid], v);
            } else if (tid == kMom) {
                atomicMin(&extrema[(long long)(key - 1) * kExt + 0], s_ext[s * kExt + 0]);
            } else if (tid == kMom + 1) {
                atomicMax(&extrema[(long long)(key - 1) * kExt + 1], s_ext[s * kExt + 1]);
            }
        }
        __syncthreads();                                   // every thread has read the keys
        if (tid < kSlots * kMom) s_mom[tid] = 0;
        if (tid < kSlots * kExt) s_ext[tid] = (tid & 1) ? -1 : INT_MAX;
        if (tid < kSlots) s_key[tid] = 0;                  // visible to the next tile behind its staging barrier
    }
}

__global__ void __launch_bounds__(kThreads) instance_intensity_init_kernel(int* __restrict__ extrema, long long n) {
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        extrema[i] = (i & 1) ? -1 : INT_MAX;
}

}  // namespace

extern "C" {

int sk_instance_intensity_row_values(int which) { return which == 0 ? kMom : which == 1 ? kExt : which == 2 ? kBins : 0; }

int sk_instance_intensity(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                          const void* image, int elem_bytes, int shift, int64_t* moments, int32_t* extrema,
                          int64_t* hist, void* stream) {
    const char* who = "sk_instance_intensity";
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 0);    // the guard below covers X Y Z itself
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2, "sk_instance_intensity: elem_bytes = %d must be 1 or 2", elem_bytes);
    SK_CHECK_ARG(shift >= 0 && shift <= 8 && (elem_bytes == 2 || shift == 0),
                 "sk_instance_intensity: shift = %d must lie in 0 .. 8, and be 0 for 1-byte samples", shift);
    const int m = X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z);
    const unsigned __int128 V = elem_bytes == 1 ? 255 : 65535, lim = (unsigned __int128)1 << 63;
    const unsigned __int128 voxels = (unsigned __int128)X * Y * Z;                       // below 2^93
    SK_CHECK_ARG(voxels < lim && voxels * V < lim && voxels * V * (V > (unsigned)m ? V : (unsigned __int128)m) < lim,
                 "sk_instance_intensity: extents %d x %d x %d with %d-byte samples: X Y Z V max(V, X, Y, Z) must stay "
                 "below 2^63, V = %d (int64 sums)", X, Y, Z, elem_bytes, elem_bytes == 1 ? 255 : 65535);
    if (N == 0) return SK_OK;
    SK_CHECK_ARG(moments && extrema, "sk_instance_intensity: NULL output pointer");
    SK_CHECK_ARG(((uintptr_t)moments & 7) == 0 && ((uintptr_t)extrema & 3) == 0 && ((uintptr_t)hist & 7) == 0,
                 "sk_instance_intensity: an output pointer is not aligned to its elements");
    const bool empty = (long long)X * Y * Z == 0;
    if (!empty) {
        rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}, {image, (unsigned)elem_bytes}});
        if (rc != SK_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(moments, 0, (size_t)N * kMom * sizeof(int64_t), st));
    if (hist) SK_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)N * kBins * sizeof(int64_t), st));
    instance_intensity_init_kernel<<<sk::stream_grid((long long)N * kExt, kThreads), kThreads, 0, st>>>(
        extrema, (long long)N * kExt);
    SK_CHECK_LAUNCH();
    if (empty) return SK_OK;
    const sk::TileGrid tg = sk::tile_grid(X, Y, Z, kTX, kTY, kTZ);
    // whole 32-bit words of image when every z row starts on a 4-byte boundary
    const int wide = ((uintptr_t)image & 3) == 0 && ((long long)Z * elem_bytes) % 4 == 0;
#define SK_II_LAUNCH(T, H)                                                                                           \
    instance_intensity_kernel<T, H><<<tg.blocks, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, tg.ntiles,      \
                                                                    tg.tiles_y, tg.tiles_z, (const T*)image, wide,   \
                                                                    shift, (u64*)moments, extrema, (u64*)hist)
    if (elem_bytes == 1) {
        if (hist) SK_II_LAUNCH(uint8_t, true);
        else SK_II_LAUNCH(uint8_t, false);
    } else {
        if (hist) SK_II_LAUNCH(uint16_t, true);
        else SK_II_LAUNCH(uint16_t, false);
    }
#undef SK_II_LAUNCH
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
