// Exact change of grid: an (X, Y, Z) volume, Z innermost, resampled to (Xo, Yo, Zo) by any ratio n/8 <= m <= 8n per axis.
//
// Definition (include/skoots_hip.h: sk_resample_volume).  Every axis has one operator, a list of
// integer taps (k, w) per output index i and a total W: nearest (one tap), linear (two taps, W = 2m) or area (the source
// voxels an output cell covers, W = n).  The output voxel is S / W rounded to nearest, halves up, with S the sum of
// wx wy wz v over the product of the three tap lists and W = Wx Wy Wz.  Integers only: the same bits on every run.
//
// The taps of an axis are always consecutive source indices, so a table row is (start, count, weights).  The weights of
// an axis are divided by a common factor the host knows in closed form -- linear: gcd(2m, 2n, |n - m|), area: gcd(n, m)
// -- which leaves every rounded quotient as it was (2x up is weights 1 and 3 of 4, the identity one tap of weight 1).
//
// Memory-bound.  Two kernels after a prologue that fills the three tap tables (m threads per axis; the only place with
// 64-bit divisions):
//   weighted   uint8 / uint16.  A wave owns `rows` consecutive output rows times one z chunk; `lanes` = 64 / rows lanes
//              work on a row, each on one unit of 16 output bytes.  Phase 1: the x/y taps of the row are summed into
//              the source's z resolution -- one 16-byte load per tap row and 16 source bytes, weight wx wy, accumulated
//              in registers -- and the sums of the chunk's source span go to the wave's part of LDS.  Phase 2: every
//              lane forms its outputs from LDS with the z taps of the table, divides by W (an estimate in floating
//              point, corrected exactly in integers: the quotient has at most 16 bits) and stores 16 bytes.  So the z
//              taps cost LDS reads, not memory reads, and the x/y sum is formed once per source voxel and output row.
//              The tap rows that neighbouring output rows share are left to L2.  Where the z axis
//              keeps its extent there is no phase 2 and no LDS: the sums are divided and stored as they are.  Where no
//              output has more than two z taps (nearest, linear) phase 2 reads both without a loop.
//              Accumulators are 32-bit where W vmax < 2^32 after the reduction and 64-bit otherwise; both are exact.
//   nearest    every dtype: out[x, y, z] = src[kx[x], ky[y], kz[z]], a lane on one unit of 16 output bytes; where the z
//              axis keeps its extent the unit is one 16-byte load.
//   scalar     rows that are not dword multiples, misaligned pointers, the tail of a row and the source units that
//              reach past a row's end go voxel by voxel.
// All stores are ordinary vector stores.  Nothing is allocated: the tables live in the caller's workspace.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kMaxExtent = 1LL << 30;       // weights (at most 2 m) and table offsets stay in 32 bits
constexpr size_t kLdsLimit = 64 * 1024;

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct Axis {
    int n, m, op;
    int taps;              // table columns: the largest tap count of an output index
    unsigned g;            // the common factor the weights are divided by
    unsigned long long W;  // the reduced total
    const int* start;      // device: [m]
    const int* count;      // device: [m]
    const unsigned* w;     // device: [m][taps]
};

long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int axis_taps(int n, int m, int op) {
    if (op == SK_RESAMPLE_NEAREST) return 1;
    if (op == SK_RESAMPLE_LINEAR) return 2;
    return (n + m - 1) / m + 1;
}

size_t axis_bytes(int m, int taps) { return (size_t)m * (2 + taps) * 4; }

// ---- prologue: the tap table of one axis ----

__global__ void __launch_bounds__(kThreads) taps_kernel(int n, int m, int op, int taps, unsigned g, int* __restrict__ start,
                                                        int* __restrict__ count, unsigned* __restrict__ w) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    unsigned* wi = w + (size_t)i * taps;
    const long long N = n, M = m;
    if (op == SK_RESAMPLE_NEAREST) {
        start[i] = (int)(((2LL * i + 1) * N) / (2 * M));
        count[i] = 1;
        wi[0] = 1u;
    } else if (op == SK_RESAMPLE_LINEAR) {
        const long long den = 2 * M, num = (2LL * i + 1) * N - M;    // num >= n - m > -den
        const long long k0 = num >= 0 ? num / den : -1;
        const long long r = num - k0 * den;
        if (k0 < 0 || k0 + 1 > N - 1 || r == 0) {   // both taps on one voxel after clamping, or the second has weight 0
            start[i] = (int)(k0 < 0 ? 0 : k0);
            count[i] = 1;
            wi[0] = (unsigned)(den / g);
            wi[1] = 0u;
        } else {
            start[i] = (int)k0;
            count[i] = 2;
            wi[0] = (unsigned)((den - r) / g);
            wi[1] = (unsigned)(r / g);
        }
    } else {
        const long long lo = (long long)i * N, hi = lo + N;
        const long long kb = lo / M, ke = (hi + M - 1) / M - 1;
        start[i] = (int)kb;
        count[i] = (int)(ke - kb + 1);
        for (int t = 0; t < taps; ++t) {
            const long long k = kb + t;
            const long long a = k * M > lo ? k * M : lo, b = (k + 1) * M < hi ? (k + 1) * M : hi;
            wi[t] = k <= ke ? (unsigned)((b - a) / g) : 0u;
        }
    }
}

// ---- helpers ----

template <typename T>
__device__ __forceinline__ T elem(const u32x4_a4& w, int k) {
    constexpr int per = 4 / (int)sizeof(T);
    if constexpr (per == 1) return (T)w[k];
    else return (T)(w[k / per] >> (8 * (int)sizeof(T) * (k % per)));
}

template <typename T, int kO>
__device__ __forceinline__ void store_unit(T* out, const T (&o)[kO]) {
    unsigned p[4] = {0u, 0u, 0u, 0u};
    constexpr int per = 4 / (int)sizeof(T);
    constexpr unsigned kMask = sizeof(T) == 4 ? 0xFFFFFFFFu : (1u << (8 * (sizeof(T) & 3))) - 1u;
#pragma unroll
    for (int k = 0; k < kO; ++k) p[k / per] |= ((unsigned)o[k] & kMask) << (8 * (int)sizeof(T) * (k % per));
    const u32x4_a4 s = {p[0], p[1], p[2], p[3]};
    *(u32x4_a4*)out = s;
}

// floor((2 S + W) / (2 W)) for S <= W vmax, vmax < 2^16: the quotient from a floating-point estimate that is off by less
// than one, put right with the exact remainder
__device__ __forceinline__ unsigned round_div(unsigned S, unsigned W, float inv, double) {
    unsigned q = (unsigned)((float)S * inv);
    int r = (int)(S - q * W);   // -W < S - q W < 2 W and W < 2^25: right in wrapping 32-bit arithmetic
    if (r < 0) { --q; r += (int)W; }
    if (r >= (int)W) { ++q; r -= (int)W; }
    return q + (2 * r >= (int)W ? 1u : 0u);
}
__device__ __forceinline__ unsigned round_div(unsigned long long S, unsigned long long W, float, double inv) {
    unsigned long long q = (unsigned long long)((double)S * inv);
    long long r = (long long)(S - q * W);   // |S - q W| < 2 W < 2^63
    if (r < 0) { --q; r += (long long)W; }
    if (r >= (long long)W) { ++q; r -= (long long)W; }
    return (unsigned)q + (2 * r >= (long long)W ? 1u : 0u);
}

struct Geometry {
    int lanes_log2;   // lanes of a wave on one output row; 64 >> lanes_log2 rows a wave
    int unit;         // output voxels of a lane: 16 bytes of them, fewer where z shrinks so much that the spans would not fit LDS
    int chunk;        // output voxels of a row one wave covers: unit << lanes_log2
    int span;         // LDS entries of one row: at least the source voxels a chunk reads
};

// ---- weighted: uint8 / uint16 ----

// The x/y taps of output row (xo, yo) summed over the 16 source bytes that start at voxel zb of the tap rows
template <typename T, typename ACC>
__device__ __forceinline__ void xy_sum(ACC (&acc)[16 / sizeof(T)], const T* __restrict__ src, int Y, int Z, const Axis& ax,
                                       const Axis& ay, int xo, int yo, int zb, bool whole) {
    constexpr int kV = 16 / (int)sizeof(T);
    const int sx = ax.start[xo], cx = ax.count[xo], sy = ay.start[yo], cy = ay.count[yo];
    const unsigned* wx = ax.w + (size_t)xo * ax.taps;
    const unsigned* wy = ay.w + (size_t)yo * ay.taps;
#pragma unroll
    for (int e = 0; e < kV; ++e) acc[e] = 0;
    for (int tx = 0; tx < cx; ++tx) {
        const ACC wxv = wx[tx];
        for (int ty = 0; ty < cy; ++ty) {
            const ACC wxy = wxv * (ACC)wy[ty];
            const T* row = src + ((size_t)(sx + tx) * Y + (sy + ty)) * Z;
            if (whole) {
                const u32x4_a4 v = *(const u32x4_a4*)(row + zb);
#pragma unroll
                for (int e = 0; e < kV; ++e) acc[e] += wxy * (ACC)elem<T>(v, e);
            } else {
#pragma unroll
                for (int e = 0; e < kV; ++e) acc[e] += zb + e < Z ? wxy * (ACC)row[zb + e] : (ACC)0;
            }
        }
    }
}

// The z axis keeps its extent (one tap of weight 1 whatever its operator): no LDS, the sums are the outputs' own
template <typename T, typename ACC>
__global__ void __launch_bounds__(kThreads) weighted_xy_kernel(const T* __restrict__ src, T* __restrict__ dst, int Y, int Z,
                                                               long long rows_total, int Yo, Axis ax, Axis ay, int lanes_log2,
                                                               int vec_src, int vec_dst, ACC W, float inv_f, double inv_d) {
    constexpr int kV = 16 / (int)sizeof(T);
    const int lanes = 1 << lanes_log2;
    const int li = threadIdx.x & (lanes - 1);
    const long long at = ((long long)blockIdx.x * kThreads + threadIdx.x) >> lanes_log2;
    if (at >= rows_total) return;
    const unsigned orow = (unsigned)at;
    const int xo = (int)(orow / (unsigned)Yo), yo = (int)(orow - (unsigned)xo * (unsigned)Yo);
    const int z0 = (blockIdx.y * lanes + li) * kV;
    if (z0 >= Z) return;
    const bool whole = z0 + kV <= Z;
    ACC acc[kV];
    xy_sum<T, ACC>(acc, src, Y, Z, ax, ay, xo, yo, z0, vec_src && whole);
    T o[kV];
#pragma unroll
    for (int e = 0; e < kV; ++e) o[e] = (T)round_div(acc[e], W, inv_f, inv_d);
    T* out = dst + (size_t)orow * Z + z0;
    if (vec_dst && whole) {
        store_unit<T, kV>(out, o);
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e)
            if (z0 + e < Z) out[e] = o[e];
    }
}

// TWO: no output index has more than two z taps (nearest, linear, area that does not shrink): both are read without a
// loop, the second with its table weight, 0 where there is one tap
template <typename T, typename ACC, bool TWO>
__global__ void __launch_bounds__(kThreads) weighted_kernel(const T* __restrict__ src, T* __restrict__ dst, int Y, int Z,
                                                            long long rows_total, int Yo, int Zo, Axis ax, Axis ay, Axis az,
                                                            Geometry geo, int vec_src, int vec_dst, ACC W, float inv_f,
                                                            double inv_d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int kV = 16 / (int)sizeof(T);    // voxels of 16 bytes
    constexpr int kD = 4 / (int)sizeof(T);     // voxels of a dword
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lanes = 1 << geo.lanes_log2, rows = 64 >> geo.lanes_log2;
    const int li = lane & (lanes - 1), g = lane >> geo.lanes_log2;
    ACC* lds = (ACC*)lds_raw + ((size_t)wave * rows + g) * geo.span;
    const long long at = ((long long)blockIdx.x * kWaves + wave) * rows + g;
    const bool live = at < rows_total;
    const unsigned orow = live ? (unsigned)at : 0u;
    const int xo = (int)(orow / (unsigned)Yo), yo = (int)(orow - (unsigned)xo * (unsigned)Yo);
    // the chunk's source span: starts and ends of the z taps do not decrease with the output index
    const int zo_first = blockIdx.y * geo.chunk, zo_last = min(Zo, zo_first + geo.chunk) - 1;
    const int s0 = az.start[zo_first];
    const int span = min(az.start[zo_last] + az.count[zo_last] - s0, geo.span);
    if (live) {
        const int e0 = s0 & ~(kD - 1);                       // dword-aligned start of the units
        const int n_units = (s0 + span - e0 + kV - 1) / kV;
        for (int j = li; j < n_units; j += lanes) {
            const int zb = e0 + j * kV;
            ACC acc[kV];
            xy_sum<T, ACC>(acc, src, Y, Z, ax, ay, xo, yo, zb, vec_src && zb + kV <= Z);
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                const int idx = zb + e - s0;
                if (idx >= 0 && idx < span) lds[idx] = acc[e];
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const int zo0 = zo_first + li * geo.unit;
    if (zo0 >= Zo) return;
    T* out = dst + (size_t)orow * Zo + zo0;
    T o[kV];
    if (TWO && az.taps == 2 && geo.unit == kV && zo0 + kV <= Zo) {
        // a whole unit: the table rows of its outputs are consecutive, 4 starts or 2 weight pairs a 16-byte load
        int st[kV];
        unsigned wz[2 * kV];
#pragma unroll
        for (int q = 0; q < kV / 4; ++q) {
            const u32x4_a4 v = *(const u32x4_a4*)(az.start + zo0 + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) st[4 * q + i] = (int)v[i] - s0;
        }
#pragma unroll
        for (int q = 0; q < kV / 2; ++q) {
            const u32x4_a4 v = *(const u32x4_a4*)(az.w + 2 * (size_t)zo0 + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) wz[4 * q + i] = v[i];
        }
#pragma unroll
        for (int e = 0; e < kV; ++e) {
            const ACC S = (ACC)wz[2 * e] * lds[min(st[e], span - 1)] + (ACC)wz[2 * e + 1] * lds[min(st[e] + 1, span - 1)];
            o[e] = (T)round_div(S, W, inv_f, inv_d);
        }
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e) {
            const int zo = min(zo0 + e, Zo - 1);
            const int st = az.start[zo] - s0;
            const unsigned* wz = az.w + (size_t)zo * az.taps;
            ACC S;
            if (TWO) {
                const ACC w1 = az.taps == 2 ? (ACC)wz[1] : (ACC)0;
                S = (ACC)wz[0] * lds[min(st, span - 1)] + w1 * lds[min(st + 1, span - 1)];
            } else {
                const int cn = e < geo.unit ? az.count[zo] : 0;
                S = 0;
                for (int t = 0; t < cn; ++t) S += (ACC)wz[t] * lds[min(st + t, span - 1)];
            }
            o[e] = (T)round_div(S, W, inv_f, inv_d);
        }
    }
    if (vec_dst && geo.unit == kV && zo0 + kV <= Zo) {
        store_unit<T, kV>(out, o);
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e)
            if (e < geo.unit && zo0 + e < Zo) out[e] = o[e];
    }
}

// ---- nearest: every dtype ----

template <typename T>
__global__ void __launch_bounds__(kThreads) nearest_kernel(const T* __restrict__ src, T* __restrict__ dst, int Y, int Z,
                                                           long long rows_total, int Yo, int Zo, const int* __restrict__ kx,
                                                           const int* __restrict__ ky, const int* __restrict__ kz,
                                                           int lanes_log2, int vec_src, int vec_dst) {
    constexpr int kV = 16 / (int)sizeof(T);
    const int lanes = 1 << lanes_log2;
    const int li = threadIdx.x & (lanes - 1);
    const long long at = ((long long)blockIdx.x * kThreads + threadIdx.x) >> lanes_log2;
    if (at >= rows_total) return;
    const unsigned orow = (unsigned)at;
    const int xo = (int)(orow / (unsigned)Yo), yo = (int)(orow - (unsigned)xo * (unsigned)Yo);
    const int zo0 = (blockIdx.y * lanes + li) * kV;
    if (zo0 >= Zo) return;
    const T* row = src + ((size_t)kx[xo] * Y + ky[yo]) * Z;
    T* out = dst + (size_t)orow * Zo + zo0;
    const bool whole = zo0 + kV <= Zo;
    if (Z == Zo && vec_src && vec_dst && whole) {     // the z axis keeps its extent: nearest is the identity on it
        *(u32x4_a4*)out = *(const u32x4_a4*)(row + zo0);
        return;
    }
    T o[kV];
#pragma unroll
    for (int e = 0; e < kV; ++e) o[e] = row[kz[min(zo0 + e, Zo - 1)]];
    if (vec_dst && whole) {
        store_unit<T, kV>(out, o);
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e)
            if (zo0 + e < Zo) out[e] = o[e];
    }
}

// ---- host ----

struct Plan {
    Axis ax[3];
    size_t workspace_bytes;
    bool all_nearest;
    bool wide;               // 64-bit accumulators
    unsigned long long W;    // reduced total
};

int make_plan(int dtype, const int n[3], const int m[3], const int op[3], Plan* p) {
    const char* names = "xyz";
    SK_CHECK_ARG(dtype == SK_I32 || dtype == SK_I16 || dtype == SK_U8 || dtype == SK_U16,
                 "sk_resample_volume: dtype = %d, must be int32 (3), int16 (2), uint8 (4) or uint16 (5)", dtype);
    p->all_nearest = true;
    for (int a = 0; a < 3; ++a) {
        SK_CHECK_ARG(n[a] > 0 && m[a] > 0, "sk_resample_volume: extents (%d, %d, %d) -> (%d, %d, %d) must be positive", n[0],
                     n[1], n[2], m[0], m[1], m[2]);
        SK_CHECK_ARG(n[a] <= kMaxExtent && m[a] <= kMaxExtent,
                     "sk_resample_volume: extents (%d, %d, %d) -> (%d, %d, %d): the limit of an extent is 2^30", n[0], n[1], n[2],
                     m[0], m[1], m[2]);
        SK_CHECK_ARG(op[a] >= SK_RESAMPLE_NEAREST && op[a] <= SK_RESAMPLE_AREA,
                     "sk_resample_volume: operator of %c = %d, must be 0 (nearest), 1 (linear) or 2 (area)", names[a], op[a]);
        SK_CHECK_ARG(8LL * m[a] >= n[a] && m[a] <= 8LL * n[a],
                     "sk_resample_volume: ratio of %c, %d -> %d, is outside n / 8 <= m <= 8 n (halve with sk_pool_volume first)",
                     names[a], n[a], m[a]);
        p->all_nearest = p->all_nearest && op[a] == SK_RESAMPLE_NEAREST;
    }
    SK_CHECK_ARG(p->all_nearest || dtype == SK_U8 || dtype == SK_U16,
                 "sk_resample_volume: dtype = %d, linear and area take uint8 (4) or uint16 (5); label volumes take nearest on "
                 "every axis", dtype);
    const unsigned long long vmax = dtype == SK_U8 ? 255ull : dtype == SK_U16 ? 65535ull : dtype == SK_I16 ? 32767ull : 2147483647ull;
    unsigned __int128 full = vmax, reduced = vmax;
    p->W = 1;
    size_t bytes = 0;
    for (int a = 0; a < 3; ++a) {
        Axis& A = p->ax[a];
        A.n = n[a];
        A.m = m[a];
        A.op = op[a];
        A.taps = axis_taps(n[a], m[a], op[a]);
        long long total = 1, g = 1;
        if (op[a] == SK_RESAMPLE_LINEAR) {
            total = 2LL * m[a];
            g = gcd_ll(gcd_ll(2LL * m[a], 2LL * n[a]), n[a] > m[a] ? n[a] - m[a] : m[a] - n[a]);
        } else if (op[a] == SK_RESAMPLE_AREA) {
            total = n[a];
            g = gcd_ll(n[a], m[a]);
        }
        A.g = (unsigned)g;
        A.W = (unsigned long long)(total / g);
        full *= (unsigned long long)total;
        reduced *= A.W;
        p->W *= A.W;
        bytes += axis_bytes(m[a], A.taps);
    }
    SK_CHECK_ARG(full < ((unsigned __int128)1 << 63),
                 "sk_resample_volume: the weight total Wx Wy Wz times the dtype's largest value reaches 2^63: (%d, %d, %d) -> "
                 "(%d, %d, %d) cannot be summed exactly", n[0], n[1], n[2], m[0], m[1], m[2]);
    p->wide = reduced >= ((unsigned __int128)1 << 32);
    p->workspace_bytes = bytes;
    SK_CHECK_ARG((long long)m[0] * m[1] <= 0x7FFFFFFFLL, "sk_resample_volume: %lld output rows, the limit is 2^31 - 1",
                 (long long)m[0] * m[1]);
    return SK_OK;
}

void place_tables(Plan& p, void* workspace) {
    char* at = (char*)workspace;
    for (int a = 0; a < 3; ++a) {
        Axis& A = p.ax[a];
        A.start = (const int*)at;
        A.count = (const int*)(at + (size_t)A.m * 4);
        A.w = (const unsigned*)(at + (size_t)A.m * 8);
        at += axis_bytes(A.m, A.taps);
    }
}

template <typename T>
int launch_nearest(const Plan& p, const void* src, void* dst, int vec_src, int vec_dst, hipStream_t stream) {
    constexpr int kV = 16 / (int)sizeof(T);
    const int Zo = p.ax[2].m, units = (Zo + kV - 1) / kV;
    int lanes_log2 = 0;
    while (lanes_log2 < 6 && (1 << lanes_log2) < units) ++lanes_log2;
    const long long rows = (long long)p.ax[0].m * p.ax[1].m;
    const long long gx = ((rows << lanes_log2) + kThreads - 1) / kThreads, gy = (units + (1 << lanes_log2) - 1) >> lanes_log2;
    SK_CHECK_ARG(gx <= 0x7FFFFFFFLL && gy <= 65535, "sk_resample_volume: %lld x %lld workgroups do not fit one grid", gx, gy);
    nearest_kernel<T><<<dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, stream>>>(
        (const T*)src, (T*)dst, p.ax[1].n, p.ax[2].n, rows, p.ax[1].m, Zo, p.ax[0].start, p.ax[1].start, p.ax[2].start,
        lanes_log2, vec_src, vec_dst);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

// The source voxels the z taps of `chunk` consecutive outputs can reach: the taps of an output lie within one voxel of
// its cell, so chunk n / m rounded up and three more bound it for all three operators.
long long span_bound(long long chunk, int n, int m) { return (chunk * n + m - 1) / m + 3; }

template <typename T, typename ACC>
int launch_weighted(const Plan& p, const void* src, void* dst, int vec_src, int vec_dst, hipStream_t stream) {
    constexpr int kV = 16 / (int)sizeof(T);
    const int Z = p.ax[2].n, Zo = p.ax[2].m;
    const long long rows = (long long)p.ax[0].m * p.ax[1].m;
    const float inv_f = 1.0f / (float)p.W;
    const double inv_d = 1.0 / (double)p.W;
    if (Z == Zo) {
        const int units = (Z + kV - 1) / kV;
        int lanes_log2 = 0;
        while (lanes_log2 < 6 && (1 << lanes_log2) < units) ++lanes_log2;
        const long long gx = ((rows << lanes_log2) + kThreads - 1) / kThreads, gy = (units + (1 << lanes_log2) - 1) >> lanes_log2;
        SK_CHECK_ARG(gx <= 0x7FFFFFFFLL && gy <= 65535, "sk_resample_volume: %lld x %lld workgroups do not fit one grid", gx, gy);
        weighted_xy_kernel<T, ACC><<<dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, stream>>>(
            (const T*)src, (T*)dst, p.ax[1].n, Z, rows, p.ax[1].m, p.ax[0], p.ax[1], lanes_log2, vec_src, vec_dst, (ACC)p.W, inv_f,
            inv_d);
        SK_CHECK_LAUNCH();
        return SK_OK;
    }
    Geometry geo;
    // fewer outputs a lane until the workgroup's staged spans fit LDS: one output a lane needs at most 11 entries
    for (geo.unit = kV;; geo.unit /= 2) {
        const int units = (Zo + geo.unit - 1) / geo.unit;
        geo.lanes_log2 = 0;
        while (geo.lanes_log2 < 6 && (1 << geo.lanes_log2) < units) ++geo.lanes_log2;
        geo.chunk = geo.unit << geo.lanes_log2;
        geo.span = (int)span_bound(geo.chunk, Z, Zo);
        const size_t need = (size_t)kWaves * (64 >> geo.lanes_log2) * geo.span * sizeof(ACC);
        if (need <= kLdsLimit || geo.unit == 1) break;
    }
    const size_t lds_bytes = (size_t)kWaves * (64 >> geo.lanes_log2) * geo.span * sizeof(ACC);
    SK_CHECK_ARG(lds_bytes <= kLdsLimit, "sk_resample_volume: %zu bytes of LDS for z %d -> %d, the limit is %zu", lds_bytes, Z, Zo,
                 kLdsLimit);
    const int rows_per_block = kWaves * (64 >> geo.lanes_log2);
    const long long gx = (rows + rows_per_block - 1) / rows_per_block, gy = (Zo + geo.chunk - 1) / geo.chunk;
    SK_CHECK_ARG(gx <= 0x7FFFFFFFLL && gy <= 65535, "sk_resample_volume: %lld x %lld workgroups do not fit one grid", gx, gy);
    if (p.ax[2].taps <= 2)
        weighted_kernel<T, ACC, true><<<dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), lds_bytes, stream>>>(
            (const T*)src, (T*)dst, p.ax[1].n, Z, rows, p.ax[1].m, Zo, p.ax[0], p.ax[1], p.ax[2], geo, vec_src, vec_dst, (ACC)p.W,
            inv_f, inv_d);
    else
        weighted_kernel<T, ACC, false><<<dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), lds_bytes, stream>>>(
            (const T*)src, (T*)dst, p.ax[1].n, Z, rows, p.ax[1].m, Zo, p.ax[0], p.ax[1], p.ax[2], geo, vec_src, vec_dst, (ACC)p.W,
            inv_f, inv_d);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // namespace

extern "C" size_t sk_resample_workspace_bytes(int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x, int op_y,
                                              int op_z) {
    const int n[3] = {X, Y, Z}, m[3] = {Xo, Yo, Zo}, op[3] = {op_x, op_y, op_z};
    Plan p;
    if (make_plan(dtype, n, m, op, &p) != SK_OK) return 0;
    return p.workspace_bytes;
}

extern "C" int sk_resample_path(int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x, int op_y, int op_z) {
    const int n[3] = {X, Y, Z}, m[3] = {Xo, Yo, Zo}, op[3] = {op_x, op_y, op_z};
    Plan p;
    const int rc = make_plan(dtype, n, m, op, &p);
    if (rc != SK_OK) return rc;
    return p.all_nearest ? SK_RESAMPLE_PATH_GATHER : p.wide ? SK_RESAMPLE_PATH_ACC64 : SK_RESAMPLE_PATH_ACC32;
}

extern "C" int sk_resample_volume(const void* src, void* dst, int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x,
                                  int op_y, int op_z, void* workspace, size_t workspace_bytes, void* stream) {
    SK_CHECK_ARG(src && dst && workspace, "sk_resample_volume: NULL pointer");
    const int n[3] = {X, Y, Z}, m[3] = {Xo, Yo, Zo}, op[3] = {op_x, op_y, op_z};
    Plan p;
    const int rc = make_plan(dtype, n, m, op, &p);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= p.workspace_bytes, "sk_resample_volume: workspace of %zu bytes, need %zu", workspace_bytes,
                 p.workspace_bytes);
    const int elem_bytes = dtype == SK_I32 ? 4 : dtype == SK_U8 ? 1 : 2;
    SK_CHECK_ARG(((uintptr_t)src & (elem_bytes - 1)) == 0 && ((uintptr_t)dst & (elem_bytes - 1)) == 0,
                 "sk_resample_volume: src or dst is not aligned to its elements");
    SK_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "sk_resample_volume: the workspace is not aligned to 4 bytes");
    place_tables(p, workspace);
    hipStream_t st = (hipStream_t)stream;
    for (int a = 0; a < 3; ++a) {
        const Axis& A = p.ax[a];
        taps_kernel<<<dim3((A.m + kThreads - 1) / kThreads), dim3(kThreads), 0, st>>>(
            A.n, A.m, A.op, A.taps, A.g, (int*)A.start, (int*)A.count, (unsigned*)A.w);
        SK_CHECK_LAUNCH();
    }
    const int vec_src = ((size_t)Z * elem_bytes) % 4 == 0 && ((uintptr_t)src & 3) == 0;
    const int vec_dst = ((size_t)Zo * elem_bytes) % 4 == 0 && ((uintptr_t)dst & 3) == 0;
    if (p.all_nearest) {
        if (dtype == SK_I32) return launch_nearest<uint32_t>(p, src, dst, vec_src, vec_dst, st);
        if (dtype == SK_U8) return launch_nearest<uint8_t>(p, src, dst, vec_src, vec_dst, st);
        return launch_nearest<uint16_t>(p, src, dst, vec_src, vec_dst, st);
    }
    if (dtype == SK_U8)
        return p.wide ? launch_weighted<uint8_t, unsigned long long>(p, src, dst, vec_src, vec_dst, st)
                      : launch_weighted<uint8_t, unsigned>(p, src, dst, vec_src, vec_dst, st);
    return p.wide ? launch_weighted<uint16_t, unsigned long long>(p, src, dst, vec_src, vec_dst, st)
                  : launch_weighted<uint16_t, unsigned>(p, src, dst, vec_src, vec_dst, st);
}
