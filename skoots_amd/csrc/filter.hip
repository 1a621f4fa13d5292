// Exact neighbourhood filters of an (X, Y, Z) volume, Z innermost: rank filters (median, min, max, any rank) on windows
// of up to 5 x 5 x 5 and separable integer tap filters (box mean, Gaussian) of up to 17 taps per axis.
//
// Definition (include/skoots_hip.h: sk_filter_rank, sk_filter_taps).  Source index i of an axis of
// extent n, any integer i: zero (0 outside), edge (clamp) or mirror (j = i mod 2n, j < n ? j : 2n - 1 - j).  Rank: the
// rank-th smallest of the window's samples, border samples included.  Taps: (S + W / 2) / W with S the sum of wx wy wz v
// over the bordered samples and W = Wx Wy Wz.  Integers only (float32 ranks run on order-preserving 32-bit keys): the
// same bits on every run.
//
// One staging routine for every kernel.  A workgroup of 256 lanes owns a tile of TX x TY rows times nu units of 16 bytes
// along z and stages the tile plus its halo in LDS: a staged row is a 16-byte unit of left halo, the nu units of the tile
// and a unit of right halo (a halo of 16 bytes is at least the largest radius in every dtype).  Units that lie inside
// the row come as one 16-byte load where rows are dword multiples on a dword-aligned base; the others, and every unit
// that touches an end of the row, go sample by sample through the border rule, so that the loops behind know no border.
// A lane reads its own unit of a staged row as one 16-byte LDS load and the rz samples on either side as dwords, and
// takes the samples apart once per row; the z radius is a template parameter, so every index into them is a constant.
//   rank    tile 4 x 8 x 128 bytes, a lane on one unit.  min and max are one pass over the window (path EXTREME).  The
//           median of 3 x 3 x 1 and of 3 x 3 x 3 is a min/max exchange network (path NETWORK): forgetful selection --
//           of n / 2 + 2 samples neither the smallest nor the largest can be the median, so both are dropped and the
//           next sample joins, down to three -- on two outputs per instruction for the 8- and 16-bit dtypes.  Every
//           other rank and window is a bitwise radix descent from the top key bit down (path RADIX): the candidate
//           takes the bit when at most `rank` samples of the window lie below it.  Unsigned compares only; no
//           data-dependent branch anywhere.
//   taps    z sums of every staged row from the row in registers, then the y sums and the x sums through LDS, one
//           rounded division at the end.  The tile is the largest of a fixed list whose three arrays fit 64 KiB.  Sums
//           are 32-bit where W vmax < 2^32 (path ACC32) and 64-bit otherwise (ACC64); both are exact.
// All stores are ordinary vector stores.  Nothing is allocated.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRankTX = 4, kRankTY = 8, kRankUnits = 8;   // 4 x 8 rows x 8 units of 16 bytes: a lane a unit
constexpr int kMaxRankRadius = 2, kMaxTapRadius = 8, kMaxTapSum = 4096;
constexpr long long kMaxExtent = 1LL << 30;
constexpr size_t kLdsLimit = 64 * 1024;
constexpr int kRankLdsDwords = (kRankTX + 2 * kMaxRankRadius) * (kRankTY + 2 * kMaxRankRadius) * (kRankUnits + 2) * 4 + 4;

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Taps {
    int r[3];                               // radius of x, y, z
    unsigned w[3][2 * kMaxTapRadius + 1];
};

struct Tile {
    int tx, ty, nu;
};

// ---- helpers ----

// Source index of i on an axis of extent n under the border rule, or -1 for "the sample is 0"
__device__ __forceinline__ int border_index(int i, int n, int border) {
    if (i >= 0 && i < n) return i;
    if (border == SK_FILTER_BORDER_ZERO) return -1;
    if (border == SK_FILTER_BORDER_EDGE) return i < 0 ? 0 : n - 1;
    const int p = 2 * n;
    int j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}

// float32 bits <-> keys that order as the values do under an unsigned compare
__device__ __forceinline__ unsigned to_key(unsigned b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned from_key(unsigned k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// The samples -RZ .. kV + RZ - 1 of unit u of a staged row, kV = 16 / sizeof(T) the samples of the unit: the unit as one
// 16-byte load, the dwords that hold the RZ samples on either side one by one
template <typename T, int RZ>
__device__ __forceinline__ void load_elems(unsigned (&el)[16 / sizeof(T) + 2 * RZ], const unsigned* row, int u) {
    constexpr int kV = 16 / (int)sizeof(T), kS = (int)sizeof(T), kH = (RZ * kS + 3) / 4;
    unsigned w[4 + 2 * kH];
    const u32x4 own = *(const u32x4*)(row + (u + 1) * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[kH + k] = own[k];
#pragma unroll
    for (int k = 0; k < kH; ++k) {
        w[k] = row[(u + 1) * 4 - kH + k];
        w[kH + 4 + k] = row[(u + 2) * 4 + k];
    }
#pragma unroll
    for (int i = 0; i < kV + 2 * RZ; ++i) {
        constexpr unsigned kMask = kS == 4 ? 0xFFFFFFFFu : (1u << (8 * (kS & 3))) - 1u;
        const int byte = 4 * kH + (i - RZ) * kS;
        el[i] = (w[byte >> 2] >> ((byte & 3) * 8)) & kMask;
    }
}

template <typename T>
__device__ __forceinline__ void store_unit(T* out, const unsigned (&o)[16 / sizeof(T)], bool vec, int left) {
    constexpr int kV = 16 / (int)sizeof(T), per = 4 / (int)sizeof(T);
    if (vec && left >= kV) {
        unsigned p[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kV; ++k) p[k / per] |= o[k] << (8 * (int)sizeof(T) * (k % per));
        const u32x4_a4 s = {p[0], p[1], p[2], p[3]};
        *(u32x4_a4*)out = s;
    } else {
#pragma unroll
        for (int k = 0; k < kV; ++k)
            if (k < left) out[k] = (T)o[k];
    }
}

// Stages the rows x0 - hx .. x0 + tx + hx - 1 by y0 - hy .. y0 + ty + hy - 1, samples z0 - kV .. z0 + (nu + 1) kV - 1,
// border rule applied.  Of the two halo units only the rz samples next to the tile are formed; units that no output of
// the volume reads are left as they are.  KEY: float32 bits become keys on the way.
template <typename T, bool KEY>
__device__ __forceinline__ void stage(unsigned* lds, const T* __restrict__ src, int X, int Y, int Z, int x0, int y0, int z0,
                                      int tx, int ty, int nu, int hx, int hy, int rz, int border, int vec_src) {
    constexpr int kV = 16 / (int)sizeof(T), per = 4 / (int)sizeof(T);
    const int nyr = ty + 2 * hy, upr = nu + 2;
    const int units = (tx + 2 * hx) * nyr * upr;
    const unsigned zero = KEY ? to_key(0u) : 0u;
    for (int it = threadIdx.x; it < units; it += kThreads) {
        const int r = it / upr, j = it - r * upr;
        const int xx = r / nyr, yy = r - xx * nyr;
        const int zs = z0 + (j - 1) * kV;
        if (zs >= Z + rz) continue;
        const int sx = border_index(x0 - hx + xx, X, border), sy = border_index(y0 - hy + yy, Y, border);
        unsigned p[4] = {zero, zero, zero, zero};
        if (sx >= 0 && sy >= 0) {
            const T* row = src + ((size_t)sx * Y + sy) * Z;
            if (vec_src && zs >= 0 && zs + kV <= Z) {
                const u32x4_a4 v = *(const u32x4_a4*)(row + zs);
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = KEY ? to_key(v[k]) : v[k];
            } else {
                const int lo = j == 0 ? kV - rz : 0, hi = j == upr - 1 ? rz : kV;
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = 0u;
#pragma unroll
                for (int e = 0; e < kV; ++e) {
                    unsigned v = zero;
                    if (e >= lo && e < hi) {
                        const int zi = border_index(zs + e, Z, border);
                        if (zi >= 0) v = KEY ? to_key((unsigned)row[zi]) : (unsigned)row[zi];
                    }
                    p[e / per] |= v << (8 * (int)sizeof(T) * (e % per));
                }
            }
        }
        const u32x4 s = {p[0], p[1], p[2], p[3]};
        *(u32x4*)(lds + ((size_t)r * upr + j) * 4) = s;
    }
}

// The tile of workgroup b: tiles of z fastest, then y, then x
__device__ __forceinline__ void tile_origin(int tiles_y, int tiles_z, int& bx, int& by, int& bz) {
    const unsigned b = blockIdx.x;
    const unsigned q = b / (unsigned)tiles_z;
    bz = (int)(b - q * (unsigned)tiles_z);
    bx = (int)(q / (unsigned)tiles_y);
    by = (int)(q - (unsigned)bx * (unsigned)tiles_y);
}

// ---- rank filters ----

enum { kMin = 0, kMax = 1, kRadix = 2, kNetwork = 3 };

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void exchange(unsigned& a, unsigned& b) {
    const unsigned lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}
__device__ __forceinline__ void exchange(u16x2& a, u16x2& b) {
    const u16x2 lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
    a = lo;
    b = hi;
}

// The median of N samples (N odd) by forgetful selection.  Of m = (samples left) / 2 + 2 samples the smallest has
// m - 1 samples above it and the largest m - 1 below, more than half of those left, so neither is the median: both are
// dropped, the median of the rest is the same sample, and the next sample joins.  Three samples are left at the end.
template <typename V, int N>
__device__ __forceinline__ V median_of(const V (&s)[N]) {
    constexpr int kM = N / 2 + 2 > N ? N : N / 2 + 2;
    V a[kM];
#pragma unroll
    for (int i = 0; i < kM; ++i) a[i] = s[i];
    if constexpr (N == 1) return a[0];
    int next = kM;
#pragma unroll
    for (int m = kM; m >= 3; --m) {
#pragma unroll
        for (int i = 0; i < m / 2; ++i) exchange(a[i], a[m - 1 - i]);             // the smaller of every pair in front
#pragma unroll
        for (int i = 1; i < (m + 1) / 2; ++i) exchange(a[0], a[i]);               // the smallest to a[0]
#pragma unroll
        for (int i = m / 2; i < m - 1; ++i) exchange(a[i], a[m - 1]);             // the largest to a[m - 1]
        if (m > 3) a[0] = s[next++];                                              // a[0] and a[m - 1] are forgotten
    }
    return a[1];
}

// T: the unsigned sample type the staged rows hold (float32 as uint32_t with KEY)
template <typename T, bool KEY, int MODE, int RZ>
__global__ void __launch_bounds__(kThreads) rank_kernel(const T* __restrict__ src, T* __restrict__ dst, int X, int Y, int Z,
                                                        int rx, int ry, int rank, int border, int vec_src, int vec_dst,
                                                        int tiles_y, int tiles_z) {
    __shared__ __attribute__((aligned(16))) unsigned lds[kRankLdsDwords];
    constexpr int kV = 16 / (int)sizeof(T), kBits = 8 * (int)sizeof(T), kE = kV + 2 * RZ;
    int bx, by, bz;
    tile_origin(tiles_y, tiles_z, bx, by, bz);
    const int x0 = bx * kRankTX, y0 = by * kRankTY, z0 = bz * kRankUnits * kV;
    stage<T, KEY>(lds, src, X, Y, Z, x0, y0, z0, kRankTX, kRankTY, kRankUnits, rx, ry, RZ, border, vec_src);
    __syncthreads();
    const int u = threadIdx.x & (kRankUnits - 1), ly = (threadIdx.x >> 3) & (kRankTY - 1), lx = threadIdx.x >> 6;
    const int x = x0 + lx, y = y0 + ly, z = z0 + u * kV;
    if (x >= X || y >= Y || z >= Z) return;
    const int nyr = kRankTY + 2 * ry, row_dw = (kRankUnits + 2) * 4;
    unsigned v[kV];
    if constexpr (MODE == kNetwork) {
        // rx = ry = 1: the nine rows of the window, their samples taken apart once
        constexpr int kN = 9 * (2 * RZ + 1);
        unsigned el[9][kE];
#pragma unroll
        for (int k = 0; k < 9; ++k) load_elems<T, RZ>(el[k], lds + ((lx + k / 3) * (kRankTY + 2) + ly + k % 3) * row_dw, u);
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                unsigned s[kN];
#pragma unroll
                for (int k = 0; k < 9; ++k)
#pragma unroll
                    for (int dz = 0; dz <= 2 * RZ; ++dz) s[k * (2 * RZ + 1) + dz] = el[k][e + dz];
                v[e] = median_of<unsigned, kN>(s);
            }
        } else {
            // two outputs per instruction: sample i and sample i + 1 of a row side by side in 16-bit halves
            u16x2 pk[9][kE - 1];
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int i = 0; i < kE - 1; ++i) pk[k][i] = u16x2{(unsigned short)el[k][i], (unsigned short)el[k][i + 1]};
#pragma unroll
            for (int e = 0; e < kV; e += 2) {
                u16x2 s[kN];
#pragma unroll
                for (int k = 0; k < 9; ++k)
#pragma unroll
                    for (int dz = 0; dz <= 2 * RZ; ++dz) s[k * (2 * RZ + 1) + dz] = pk[k][e + dz];
                const u16x2 m = median_of<u16x2, kN>(s);
                v[e] = m[0];
                v[e + 1] = m[1];
            }
        }
    } else if constexpr (MODE == kRadix) {
#pragma unroll
        for (int e = 0; e < kV; ++e) v[e] = 0u;
        for (int bit = kBits - 1; bit >= 0; --bit) {
            unsigned cand[kV], below[kV];
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                cand[e] = v[e] | (1u << bit);
                below[e] = 0u;
            }
            for (int dx = 0; dx <= 2 * rx; ++dx)
                for (int dy = 0; dy <= 2 * ry; ++dy) {
                    unsigned el[kE];
                    load_elems<T, RZ>(el, lds + ((lx + dx) * nyr + ly + dy) * row_dw, u);
#pragma unroll
                    for (int e = 0; e < kV; ++e)
#pragma unroll
                        for (int dz = 0; dz <= 2 * RZ; ++dz) below[e] += el[e + dz] < cand[e] ? 1u : 0u;
                }
#pragma unroll
            for (int e = 0; e < kV; ++e) v[e] = below[e] <= (unsigned)rank ? cand[e] : v[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e) v[e] = MODE == kMin ? 0xFFFFFFFFu : 0u;
        for (int dx = 0; dx <= 2 * rx; ++dx)
            for (int dy = 0; dy <= 2 * ry; ++dy) {
                unsigned el[kE];
                load_elems<T, RZ>(el, lds + ((lx + dx) * nyr + ly + dy) * row_dw, u);
#pragma unroll
                for (int e = 0; e < kV; ++e)
#pragma unroll
                    for (int dz = 0; dz <= 2 * RZ; ++dz) v[e] = MODE == kMin ? min(v[e], el[e + dz]) : max(v[e], el[e + dz]);
            }
    }
    if constexpr (KEY) {
#pragma unroll
        for (int e = 0; e < kV; ++e) v[e] = from_key(v[e]);
    }
    store_unit<T>(dst + ((size_t)x * Y + y) * Z + z, v, vec_dst != 0, Z - z);
}

// ---- tap filters ----

// floor((2 S + W) / (2 W)) = (S + W / 2) / W for S <= W vmax, vmax < 2^16: the quotient from a floating-point estimate
// that is off by less than one, put right with the exact remainder
__device__ __forceinline__ unsigned round_div(unsigned S, unsigned W, float inv, double) {
    unsigned q = (unsigned)((float)S * inv);
    int r = (int)(S - q * W);   // -W < S - q W < 2 W and W < 2^25: right in wrapping 32-bit arithmetic
    if (r < 0) { --q; r += (int)W; }
    if (r >= (int)W) { ++q; r -= (int)W; }
    return q + (2 * r >= (int)W ? 1u : 0u);
}
__device__ __forceinline__ unsigned round_div(unsigned long long S, unsigned long long W, float, double inv) {
    unsigned long long q = (unsigned long long)((double)S * inv);
    long long r = (long long)(S - q * W);   // |S - q W| < 2 W < 2^38
    if (r < 0) { --q; r += (long long)W; }
    if (r >= (long long)W) { ++q; r -= (long long)W; }
    return (unsigned)q + (2 * r >= (long long)W ? 1u : 0u);
}

// The z sums of unit u of a staged row: every sample taken apart once, every index a constant
template <typename T, typename ACC, int RZ>
__device__ __forceinline__ void z_sums(ACC (&acc)[16 / sizeof(T)], const unsigned* row, int u, const unsigned (&w)[2 * kMaxTapRadius + 1]) {
    constexpr int kV = 16 / (int)sizeof(T);
    unsigned el[kV + 2 * RZ];
    load_elems<T, RZ>(el, row, u);
#pragma unroll
    for (int e = 0; e < kV; ++e) acc[e] = 0;
#pragma unroll
    for (int t = 0; t <= 2 * RZ; ++t) {
        const ACC wt = w[t];
#pragma unroll
        for (int e = 0; e < kV; ++e) acc[e] += wt * (ACC)el[e + t];
    }
}

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// LDS of a tap tile: region 1 holds the staged rows and later the y sums, region 2 the z sums
__host__ __device__ inline size_t taps_region1(const Tile& t, const int r[3], int elem_bytes, int acc_bytes) {
    const size_t kV = 16 / elem_bytes;
    const size_t raw = (size_t)(t.tx + 2 * r[0]) * (t.ty + 2 * r[1]) * (t.nu + 2) * 16 + 16;
    const size_t ysum = (size_t)(t.tx + 2 * r[0]) * t.ty * t.nu * kV * acc_bytes;
    return align16(raw > ysum ? raw : ysum);
}
__host__ __device__ inline size_t taps_region2(const Tile& t, const int r[3], int elem_bytes, int acc_bytes) {
    const size_t kV = 16 / elem_bytes;
    return (size_t)(t.tx + 2 * r[0]) * (t.ty + 2 * r[1]) * t.nu * kV * acc_bytes;
}

template <typename T, typename ACC>
__global__ void __launch_bounds__(kThreads) taps_kernel(const T* __restrict__ src, T* __restrict__ dst, int X, int Y, int Z,
                                                        Taps tp, Tile tile, int border, int vec_src, int vec_dst, int tiles_y,
                                                        int tiles_z, ACC W, float inv_f, double inv_d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int kV = 16 / (int)sizeof(T);
    const int rx = tp.r[0], ry = tp.r[1], rz = tp.r[2];
    const int tx = tile.tx, ty = tile.ty, nu = tile.nu;
    const int nxr = tx + 2 * rx, nyr = ty + 2 * ry, row_dw = (nu + 2) * 4;
    unsigned* raw = (unsigned*)lds_raw;
    ACC* ysum = (ACC*)lds_raw;
    ACC* zsum = (ACC*)(lds_raw + taps_region1(tile, tp.r, (int)sizeof(T), (int)sizeof(ACC)));
    int bx, by, bz;
    tile_origin(tiles_y, tiles_z, bx, by, bz);
    const int x0 = bx * tx, y0 = by * ty, z0 = bz * nu * kV;
    stage<T, false>(raw, src, X, Y, Z, x0, y0, z0, tx, ty, nu, rx, ry, rz, border, vec_src);
    __syncthreads();
    // z sums of every staged row, from the row in registers
    for (int it = threadIdx.x; it < nxr * nyr * nu; it += kThreads) {
        const int r = it / nu, u = it - r * nu;
        const unsigned* row = raw + (size_t)r * row_dw;
        ACC acc[kV];
        switch (rz) {
            case 0: z_sums<T, ACC, 0>(acc, row, u, tp.w[2]); break;
            case 1: z_sums<T, ACC, 1>(acc, row, u, tp.w[2]); break;
            case 2: z_sums<T, ACC, 2>(acc, row, u, tp.w[2]); break;
            case 3: z_sums<T, ACC, 3>(acc, row, u, tp.w[2]); break;
            case 4: z_sums<T, ACC, 4>(acc, row, u, tp.w[2]); break;
            case 5: z_sums<T, ACC, 5>(acc, row, u, tp.w[2]); break;
            case 6: z_sums<T, ACC, 6>(acc, row, u, tp.w[2]); break;
            case 7: z_sums<T, ACC, 7>(acc, row, u, tp.w[2]); break;
            default: z_sums<T, ACC, 8>(acc, row, u, tp.w[2]); break;
        }
        ACC* out = zsum + (size_t)it * kV;
#pragma unroll
        for (int e = 0; e < kV; ++e) out[e] = acc[e];
    }
    __syncthreads();     // the staged rows are dead from here: the y sums take their place
    for (int it = threadIdx.x; it < nxr * ty * nu; it += kThreads) {
        const int q = it / nu, u = it - q * nu;
        const int xx = q / ty, y = q - xx * ty;
        ACC acc[kV];
#pragma unroll
        for (int e = 0; e < kV; ++e) acc[e] = 0;
        for (int t = 0; t <= 2 * ry; ++t) {
            const ACC w = tp.w[1][t];
            const ACC* in = zsum + ((size_t)(xx * nyr + y + t) * nu + u) * kV;
#pragma unroll
            for (int e = 0; e < kV; ++e) acc[e] += w * in[e];
        }
        ACC* out = ysum + (size_t)it * kV;
#pragma unroll
        for (int e = 0; e < kV; ++e) out[e] = acc[e];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < tx * ty * nu; it += kThreads) {
        const int q = it / nu, u = it - q * nu;
        const int lx = q / ty, ly = q - lx * ty;
        const int x = x0 + lx, y = y0 + ly, z = z0 + u * kV;
        if (x >= X || y >= Y || z >= Z) continue;
        ACC acc[kV];
#pragma unroll
        for (int e = 0; e < kV; ++e) acc[e] = 0;
        for (int t = 0; t <= 2 * rx; ++t) {
            const ACC w = tp.w[0][t];
            const ACC* in = ysum + ((size_t)((lx + t) * ty + ly) * nu + u) * kV;
#pragma unroll
            for (int e = 0; e < kV; ++e) acc[e] += w * in[e];
        }
        unsigned o[kV];
#pragma unroll
        for (int e = 0; e < kV; ++e) o[e] = round_div(acc[e], W, inv_f, inv_d);
        store_unit<T>(dst + ((size_t)x * Y + y) * Z + z, o, vec_dst != 0, Z - z);
    }
}

// ---- host ----

int elem_bytes_of(int dtype) { return dtype == SK_U8 ? 1 : dtype == SK_U16 ? 2 : 4; }

int check_volume(const char* who, int dtype, bool with_float, int X, int Y, int Z, int border) {
    SK_CHECK_ARG(dtype == SK_U8 || dtype == SK_U16 || (with_float && dtype == SK_F32),
                 with_float ? "%s: dtype = %d, must be uint8 (4), uint16 (5) or float32 (1)"
                            : "%s: dtype = %d, must be uint8 (4) or uint16 (5): sums of float samples have no exact order",
                 who, dtype);
    SK_CHECK_ARG(X > 0 && Y > 0 && Z > 0, "%s: extents (%d, %d, %d) must be positive", who, X, Y, Z);
    SK_CHECK_ARG(X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent, "%s: extents (%d, %d, %d): the limit of an extent is 2^30",
                 who, X, Y, Z);
    SK_CHECK_ARG(border >= SK_FILTER_BORDER_ZERO && border <= SK_FILTER_BORDER_MIRROR,
                 "%s: border = %d, must be 0 (zero), 1 (edge) or 2 (mirror)", who, border);
    return SK_OK;
}

int check_rank(int dtype, int X, int Y, int Z, int rx, int ry, int rz, int rank, int border) {
    const int rc = check_volume("sk_filter_rank", dtype, true, X, Y, Z, border);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(rx >= 0 && rx <= kMaxRankRadius && ry >= 0 && ry <= kMaxRankRadius && rz >= 0 && rz <= kMaxRankRadius,
                 "sk_filter_rank: radius (%d, %d, %d), each must be in 0 .. %d", rx, ry, rz, kMaxRankRadius);
    const int n = (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1);
    SK_CHECK_ARG(rank >= 0 && rank < n, "sk_filter_rank: rank = %d, the window of radius (%d, %d, %d) has the ranks 0 .. %d", rank,
                 rx, ry, rz, n - 1);
    return SK_OK;
}

// Checks the three tap lists; fills tp and the total W
int check_taps(int dtype, int X, int Y, int Z, const int* const taps[3], const int count[3], int border, Taps* tp,
               unsigned long long* W) {
    const int rc = check_volume("sk_filter_taps", dtype, false, X, Y, Z, border);
    if (rc != SK_OK) return rc;
    const char* names = "xyz";
    *W = 1;
    for (int a = 0; a < 3; ++a) {
        SK_CHECK_ARG(taps[a] != nullptr, "sk_filter_taps: NULL tap list of %c", names[a]);
        SK_CHECK_ARG(count[a] >= 1 && count[a] <= 2 * kMaxTapRadius + 1 && (count[a] & 1),
                     "sk_filter_taps: %d taps on %c, the count must be odd and in 1 .. %d", count[a], names[a],
                     2 * kMaxTapRadius + 1);
        long long sum = 0;
        for (int t = 0; t < 2 * kMaxTapRadius + 1; ++t) tp->w[a][t] = 0u;
        for (int t = 0; t < count[a]; ++t) {
            SK_CHECK_ARG(taps[a][t] >= 0 && taps[a][t] <= kMaxTapSum, "sk_filter_taps: tap %d of %c is %d, taps are integers in 0 .. %d",
                         t, names[a], taps[a][t], kMaxTapSum);
            tp->w[a][t] = (unsigned)taps[a][t];
            sum += taps[a][t];
        }
        SK_CHECK_ARG(sum >= 1 && sum <= kMaxTapSum, "sk_filter_taps: the tap sum of %c is %lld, it must be in 1 .. %d", names[a], sum,
                     kMaxTapSum);
        tp->r[a] = count[a] / 2;
        *W *= (unsigned long long)sum;
    }
    return SK_OK;
}

bool taps_wide(int dtype, unsigned long long W) { return W * (dtype == SK_U8 ? 255ull : 65535ull) >= (1ull << 32); }

// The largest tile of the list whose LDS fits; the last one always does (17 x 17 rows of three units and their sums)
Tile taps_tile(const int r[3], int elem_bytes, int acc_bytes, size_t* lds_bytes) {
    static const Tile kTiles[] = {{8, 8, 8}, {8, 8, 4}, {4, 8, 4}, {8, 8, 2}, {4, 8, 2}, {4, 4, 2}, {4, 4, 1}, {2, 2, 1}, {1, 1, 1}};
    Tile t = kTiles[0];
    for (const Tile& c : kTiles) {
        t = c;
        *lds_bytes = taps_region1(c, r, elem_bytes, acc_bytes) + taps_region2(c, r, elem_bytes, acc_bytes);
        if (*lds_bytes <= kLdsLimit) break;
    }
    return t;
}

// tiles of a volume as one grid: z fastest
int grid_of(const char* who, int X, int Y, int Z, int tx, int ty, int tz, int* tiles_y, int* tiles_z, unsigned* blocks) {
    const long long gx = ((long long)X + tx - 1) / tx, gy = ((long long)Y + ty - 1) / ty, gz = ((long long)Z + tz - 1) / tz;
    SK_CHECK_ARG(gx * gy <= 0x7FFFFFFFLL && gx * gy * gz <= 0x7FFFFFFFLL, "%s: %lld x %lld x %lld workgroups do not fit one grid", who,
                 gx, gy, gz);
    *tiles_y = (int)gy;
    *tiles_z = (int)gz;
    *blocks = (unsigned)(gx * gy * gz);
    return SK_OK;
}

int check_pointers(const char* who, const void* in, const void* out, int dtype) {
    SK_CHECK_ARG(in && out, "%s: NULL pointer", who);
    SK_CHECK_ARG(in != out, "%s: in == out: a filter reads the neighbours of what it writes and cannot run in place", who);
    const int eb = elem_bytes_of(dtype);
    SK_CHECK_ARG(((uintptr_t)in & (eb - 1)) == 0 && ((uintptr_t)out & (eb - 1)) == 0, "%s: in or out is not aligned to its elements",
                 who);
    return SK_OK;
}

template <typename T, bool KEY, int MODE>
void launch_rank_rz(unsigned blocks, hipStream_t st, const void* in, void* out, int X, int Y, int Z, int rx, int ry, int rz,
                    int rank, int border, int vec_src, int vec_dst, int tiles_y, int tiles_z) {
    const dim3 grid(blocks), block(kThreads);
    if (rz == 0)
        rank_kernel<T, KEY, MODE, 0><<<grid, block, 0, st>>>((const T*)in, (T*)out, X, Y, Z, rx, ry, rank, border, vec_src, vec_dst,
                                                             tiles_y, tiles_z);
    else if (rz == 1)
        rank_kernel<T, KEY, MODE, 1><<<grid, block, 0, st>>>((const T*)in, (T*)out, X, Y, Z, rx, ry, rank, border, vec_src, vec_dst,
                                                             tiles_y, tiles_z);
    else if constexpr (MODE != kNetwork)
        rank_kernel<T, KEY, MODE, 2><<<grid, block, 0, st>>>((const T*)in, (T*)out, X, Y, Z, rx, ry, rank, border, vec_src, vec_dst,
                                                             tiles_y, tiles_z);
}

template <typename T, bool KEY>
void launch_rank(int mode, unsigned blocks, hipStream_t st, const void* in, void* out, int X, int Y, int Z, int rx, int ry, int rz,
                 int rank, int border, int vec_src, int vec_dst, int tiles_y, int tiles_z) {
    if (mode == kMin)
        launch_rank_rz<T, KEY, kMin>(blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    else if (mode == kMax)
        launch_rank_rz<T, KEY, kMax>(blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    else if (mode == kNetwork)
        launch_rank_rz<T, KEY, kNetwork>(blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    else
        launch_rank_rz<T, KEY, kRadix>(blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
}

// The selection of a rank filter: min / max at the ends, the network where it is built (the median of 3 x 3 x 1 and of
// 3 x 3 x 3), the radix descent everywhere else -- or where the caller asks for it
int rank_mode(int rx, int ry, int rz, int rank, int method) {
    const int n = (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1);
    if (method == SK_FILTER_METHOD_AUTO && (rank == 0 || rank == n - 1)) return rank == 0 ? kMin : kMax;   // n == 1: the sample
    const bool network = rx == 1 && ry == 1 && rz <= 1 && rank == n / 2;
    if (method == SK_FILTER_METHOD_NETWORK) return network ? kNetwork : -1;
    return method == SK_FILTER_METHOD_AUTO && network ? kNetwork : kRadix;
}

template <typename T, typename ACC>
void launch_taps(unsigned blocks, size_t lds_bytes, hipStream_t st, const void* in, void* out, int X, int Y, int Z, const Taps& tp,
                 const Tile& tile, int border, int vec_src, int vec_dst, int tiles_y, int tiles_z, unsigned long long W) {
    taps_kernel<T, ACC><<<dim3(blocks), dim3(kThreads), lds_bytes, st>>>((const T*)in, (T*)out, X, Y, Z, tp, tile, border, vec_src,
                                                                        vec_dst, tiles_y, tiles_z, (ACC)W, 1.0f / (float)W,
                                                                        1.0 / (double)W);
}

}  // namespace

extern "C" int sk_filter_tile(int axis) {
    return axis == 0 ? kRankTX : axis == 1 ? kRankTY : axis == 2 ? kRankUnits * 16 : 0;
}

extern "C" int sk_filter_path(int dtype, int X, int Y, int Z, int rx, int ry, int rz, int rank, const int* taps_x, int nx,
                              const int* taps_y, int ny, const int* taps_z, int nz, int aligned) {
    int kernel;
    if (taps_x || taps_y || taps_z) {
        const int* const taps[3] = {taps_x, taps_y, taps_z};
        const int count[3] = {nx, ny, nz};
        Taps tp;
        unsigned long long W;
        const int rc = check_taps(dtype, X, Y, Z, taps, count, SK_FILTER_BORDER_ZERO, &tp, &W);
        if (rc != SK_OK) return rc;
        kernel = taps_wide(dtype, W) ? SK_FILTER_PATH_ACC64 : SK_FILTER_PATH_ACC32;
    } else {
        const int rc = check_rank(dtype, X, Y, Z, rx, ry, rz, rank, SK_FILTER_BORDER_ZERO);
        if (rc != SK_OK) return rc;
        const int mode = rank_mode(rx, ry, rz, rank, SK_FILTER_METHOD_AUTO);
        kernel = mode == kRadix ? SK_FILTER_PATH_RADIX : mode == kNetwork ? SK_FILTER_PATH_NETWORK : SK_FILTER_PATH_EXTREME;
    }
    const bool vec = aligned && ((size_t)Z * elem_bytes_of(dtype)) % 4 == 0;
    return kernel | (vec ? SK_FILTER_PATH_VECTOR_ROWS : 0);
}

extern "C" int sk_filter_rank(const void* in, void* out, int dtype, int X, int Y, int Z, int rx, int ry, int rz, int rank,
                              int border, int method, void* stream) {
    int rc = check_pointers("sk_filter_rank", in, out, dtype == SK_U8 || dtype == SK_U16 ? dtype : SK_F32);
    if (rc != SK_OK) return rc;
    rc = check_rank(dtype, X, Y, Z, rx, ry, rz, rank, border);
    if (rc != SK_OK) return rc;
    const int eb = elem_bytes_of(dtype);
    int tiles_y, tiles_z;
    unsigned blocks;
    rc = grid_of("sk_filter_rank", X, Y, Z, kRankTX, kRankTY, kRankUnits * (16 / eb), &tiles_y, &tiles_z, &blocks);
    if (rc != SK_OK) return rc;
    const int row_vec = ((size_t)Z * eb) % 4 == 0;
    const int vec_src = row_vec && ((uintptr_t)in & 3) == 0, vec_dst = row_vec && ((uintptr_t)out & 3) == 0;
    SK_CHECK_ARG(method >= SK_FILTER_METHOD_AUTO && method <= SK_FILTER_METHOD_NETWORK,
                 "sk_filter_rank: method = %d, must be 0 (auto), 1 (radix) or 2 (network)", method);
    const int mode = rank_mode(rx, ry, rz, rank, method);
    SK_CHECK_ARG(mode >= 0, "sk_filter_rank: method 2 (network) is built for the median of radius (1, 1, 0) and (1, 1, 1), not for "
                 "rank %d of radius (%d, %d, %d)", rank, rx, ry, rz);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SK_U8)
        launch_rank<uint8_t, false>(mode, blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    else if (dtype == SK_U16)
        launch_rank<uint16_t, false>(mode, blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    else
        launch_rank<uint32_t, true>(mode, blocks, st, in, out, X, Y, Z, rx, ry, rz, rank, border, vec_src, vec_dst, tiles_y, tiles_z);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

extern "C" int sk_filter_taps(const void* in, void* out, int dtype, int X, int Y, int Z, const int* taps_x, int nx,
                              const int* taps_y, int ny, const int* taps_z, int nz, int border, void* stream) {
    int rc = check_pointers("sk_filter_taps", in, out, dtype == SK_U16 ? SK_U16 : SK_U8);
    if (rc != SK_OK) return rc;
    const int* const taps[3] = {taps_x, taps_y, taps_z};
    const int count[3] = {nx, ny, nz};
    Taps tp;
    unsigned long long W;
    rc = check_taps(dtype, X, Y, Z, taps, count, border, &tp, &W);
    if (rc != SK_OK) return rc;
    const int eb = elem_bytes_of(dtype);
    const bool wide = taps_wide(dtype, W);
    size_t lds_bytes = 0;
    const Tile tile = taps_tile(tp.r, eb, wide ? 8 : 4, &lds_bytes);
    SK_CHECK_ARG(lds_bytes <= kLdsLimit, "sk_filter_taps: %zu bytes of LDS, the limit is %zu", lds_bytes, kLdsLimit);
    int tiles_y, tiles_z;
    unsigned blocks;
    rc = grid_of("sk_filter_taps", X, Y, Z, tile.tx, tile.ty, tile.nu * (16 / eb), &tiles_y, &tiles_z, &blocks);
    if (rc != SK_OK) return rc;
    const int row_vec = ((size_t)Z * eb) % 4 == 0;
    const int vec_src = row_vec && ((uintptr_t)in & 3) == 0, vec_dst = row_vec && ((uintptr_t)out & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SK_U8) {
        if (wide) launch_taps<uint8_t, unsigned long long>(blocks, lds_bytes, st, in, out, X, Y, Z, tp, tile, border, vec_src, vec_dst, tiles_y, tiles_z, W);
        else launch_taps<uint8_t, unsigned>(blocks, lds_bytes, st, in, out, X, Y, Z, tp, tile, border, vec_src, vec_dst, tiles_y, tiles_z, W);
    } else {
        if (wide) launch_taps<uint16_t, unsigned long long>(blocks, lds_bytes, st, in, out, X, Y, Z, tp, tile, border, vec_src, vec_dst, tiles_y, tiles_z, W);
        else launch_taps<uint16_t, unsigned>(blocks, lds_bytes, st, in, out, X, Y, Z, tp, tile, border, vec_src, vec_dst, tiles_y, tiles_z, W);
    }
    SK_CHECK_LAUNCH();
    return SK_OK;
}
