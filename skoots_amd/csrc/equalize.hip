// Histogram-driven grey-value transforms: a histogram per tile of a volume (sk_tile_histograms)
// and the pass that sends every voxel through the look-up tables of the tiles around it (sk_apply_tile_luts).  The
// tables themselves are made on the host between the two (skoots_amd/lib/morphology.py: stretch_lut, equalize_lut,
// match_lut).  Everything is integer arithmetic; include/skoots_hip.h states the definitions.
//
// Both passes walk ROWS: the z segment [zs, ze) of one (x, y), cut into the 16-byte windows of the address space that
// it touches.  A window that lies inside the segment is one 16-byte load (and store); the first and the last window
// of a segment may be partial and go element by element.  The windows of the histogram pass are those of `in`, the
// windows of the apply pass those of `out`, so every full window is one aligned vector store; `in` is read by
// vectors where it has out's phase within 16 bytes and element by element otherwise.  A workgroup's 256 threads are
// `rpp` rows of `lpr` lanes; a lane walks the windows lane, lane + lpr, ... of its row.
//
// Histograms.  A workgroup owns one (kx, ky) tile column, a chunk of `zc` z-tiles of it and a share of its rows, and
// counts into 32-bit LDS counters [z-tile][bin][copy]:
//   one     the chunk is one z-tile (the whole axis, or tz >= the chunk): up to 32 copies of the table, picked by the
//           thread, so that a constant tile -- background, the normal case -- does not put 64 lanes on one counter; a
//           lane first merges runs of equal consecutive samples of its own 16 bytes (dataset_stats.hip's treatment)
//   planes  tz == 1: a table per z-plane, 8192 / bins planes per workgroup (32 at 256 bins, 2 at 4096)
//   ztiles  2 <= tz, several z-tiles per workgroup; the z-tile of a sample comes from one division per window and a
//           counter that runs along it
//   global  tile columns of fewer than 16 rows -- (1, 1, 1), (3, 5, 7): no LDS, 64-bit global atomics per run
// A workgroup counts fewer than 2^32 samples (the host sizes its share), so no LDS counter wraps; the flush adds the
// copies of a counter and issues one 64-bit integer global atomic per non-zero counter: exact, and the same on every run.
//
// Apply.  With interpolation an axis of n >= 2 tiles of t >= 2 samples is cut into n + 1 CELLS between neighbouring
// tile centres; inside a cell the two tiles of the axis are fixed.  A workgroup owns one (x cell, y cell), a chunk of
// z-tiles and a share of the rows, and stages the tables it needs as 16-bit values in LDS: 4 corners in (x, y) where
// either axis interpolates (1 otherwise) times the z-tiles of the chunk (where z interpolates the chunk is made of z
// cells and reads one tile more than it has cells: 4 x 2 tables for one 3-D cell, 64 KiB at 4096 bins).
// x and y weights are uniform per row; the z pair and its weights come from one division per window and a counter.
// Axes with one tile, t == 1 or interpolate == 0 drop out: both their weights fall on one tile, 2 t cancels in
// (S + W / 2) / W (the header proves it), and W shrinks to the product over the axes that are left.  With no axis left
// the pass is a plain look-up.  The division is round_div of filter.hip: a floating-point estimate of the quotient, put
// right with the exact remainder.  Cells of fewer than 16 rows gather from global memory.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kHistCounters = 8192;    // 32 KiB of 32-bit counters per workgroup
constexpr int kApplyEntries = 16384;   // 32 KiB of 16-bit table entries per workgroup; one 3-D cell at 4096 bins needs 64 KiB
constexpr int kMinRows = 16;           // tile columns and cells with fewer rows take the global paths
constexpr int kMaxExtent = 1 << 30;
enum { kZOne = 0, kZTile = 1, kZInterp = 2 };

struct Geo {
    int X, Y, Z, tx, ty, tz, ntx, nty, ntz, bins, shift;
};
// how the workgroups share the volume, and how a workgroup's threads share its rows
struct Walk {
    int nzc, zc;        // z chunks, and z-tiles per chunk
    int nsplit, rpw;    // shares of a region's rows, rows per share
    int U, lpr, rpp;    // windows per row at most, lanes per row, rows per pass
    int zmode;
};

template <typename T>
__device__ __forceinline__ void load_window(unsigned (&el)[16 / sizeof(T)], const T* p, bool vec, int e_lo, int e_hi) {
    constexpr int kV = 16 / (int)sizeof(T);
    if (vec) {
        const uint4 q = *(const uint4*)p;
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < kV; ++e) {
            if constexpr (sizeof(T) == 1) el[e] = (w[e >> 2] >> (8 * (e & 3))) & 255u;
            else el[e] = (w[e >> 1] >> (16 * (e & 1))) & 65535u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e) el[e] = (e >= e_lo && e < e_hi) ? (unsigned)p[e] : 0u;
    }
}

template <typename T>
__device__ __forceinline__ void store_window(T* p, const unsigned (&o)[16 / sizeof(T)], bool vec, int e_lo, int e_hi) {
    constexpr int kV = 16 / (int)sizeof(T);
    if (vec) {
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < kV; ++e) {
            if constexpr (sizeof(T) == 1) w[e >> 2] |= o[e] << (8 * (e & 3));
            else w[e >> 1] |= o[e] << (16 * (e & 1));
        }
        *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int e = 0; e < kV; ++e)
            if (e >= e_lo && e < e_hi) p[e] = (T)o[e];
    }
}

// the samples [lo, hi) of region r of an axis: tile r, or -- `cells` -- the cell between the centres of tiles r - 1 and r
__host__ __device__ inline void region_of(int r, int t, int n, int N, int cells, int* lo, int* hi) {
    long long a, b;
    if (!cells) {
        a = (long long)r * t;
        b = a + t;
    } else {
        a = r == 0 ? 0 : (long long)t * r - (t + 1) / 2;        // the first i with floor((2 i + 1 - t) / (2 t)) == r - 1
        b = r == n ? N : (long long)t * (r + 1) - (t + 1) / 2;
    }
    *lo = (int)(a < N ? a : N);
    *hi = (int)(b < N ? b : N);
}

// the first row of a workgroup's share as (x, y), then row `local` of the share
struct RowStart {
    int x0, yoff, ylo, ny;
    __device__ RowStart(long long r0, int xlo, int ylo_, int ny_) : ylo(ylo_), ny(ny_) {
        x0 = xlo + (int)(r0 / ny_);
        yoff = (int)(r0 % ny_);
    }
    __device__ __forceinline__ void at(int local, int* x, int* y) const {
        const unsigned v = (unsigned)yoff + (unsigned)local;   // < ny + rpw <= 2^31
        const unsigned q = v / (unsigned)ny;
        *x = x0 + (int)q;
        *y = ylo + (int)(v - q * (unsigned)ny);
    }
};

// ---- histograms ----

template <typename T>
__global__ void __launch_bounds__(kThreads) hist_lds_kernel(const T* __restrict__ in, const Geo g, const Walk w, const int ncopy,
                                                            unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned counters[];
    constexpr int kV = 16 / (int)sizeof(T);
    unsigned b = blockIdx.x;
    const int gz = (int)(b % (unsigned)w.nzc);
    b /= (unsigned)w.nzc;
    const int s = (int)(b % (unsigned)w.nsplit);
    b /= (unsigned)w.nsplit;
    const int ky = (int)(b % (unsigned)g.nty), kx = (int)(b / (unsigned)g.nty);
    int xlo, xhi, ylo, yhi;
    region_of(kx, g.tx, g.ntx, g.X, 0, &xlo, &xhi);
    region_of(ky, g.ty, g.nty, g.Y, 0, &ylo, &yhi);
    const int ny = yhi - ylo;
    const long long rows = (long long)(xhi - xlo) * ny, r0 = (long long)s * w.rpw;
    if (r0 >= rows) return;
    const int nrows = (int)(rows - r0 < w.rpw ? rows - r0 : w.rpw);
    const int t0 = w.zmode == kZOne ? 0 : gz * w.zc;                 // the first z-tile of the chunk
    const int nzl = w.zmode == kZOne ? 1 : (g.ntz - t0 < w.zc ? g.ntz - t0 : w.zc);
    const long long zs64 = (long long)t0 * g.tz, ze64 = zs64 + (long long)nzl * g.tz;
    const int zs = (int)zs64, ze = w.zmode == kZOne ? g.Z : (int)(ze64 < g.Z ? ze64 : g.Z);
    const int ncount = nzl * g.bins * ncopy;
    for (int i = threadIdx.x; i < ncount; i += kThreads) counters[i] = 0;
    __syncthreads();

    const int copy = threadIdx.x & (ncopy - 1);
    const int lr = threadIdx.x / w.lpr, lj = threadIdx.x - lr * w.lpr;
    const RowStart start(r0, xlo, ylo, ny);
    if (lr < w.rpp)
        for (int r = lr; r < nrows; r += w.rpp) {
            int x, y;
            start.at(r, &x, &y);
            const T* row = in + ((size_t)x * g.Y + y) * g.Z;
            const int lead = (int)(((uintptr_t)(row + zs) & 15) / sizeof(T));
            for (int j = lj; j < w.U; j += w.lpr) {
                const int zf = zs - lead + j * kV;
                if (zf >= ze) break;
                const int e_lo = zs > zf ? zs - zf : 0, e_hi = ze - zf < kV ? ze - zf : kV;
                unsigned el[kV];
                load_window<T>(el, row + zf, e_lo == 0 && e_hi == kV, e_lo, e_hi);
                int q = 0, rem = 0;            // the z-tile of the chunk and the place in it, run along the window
                if (w.zmode == kZTile) {
                    if (g.tz == 1) q = zf + e_lo - zs;
                    else {
                        const unsigned d = (unsigned)(zf + e_lo - zs);
                        q = (int)(d / (unsigned)g.tz);
                        rem = (int)(d - (unsigned)q * (unsigned)g.tz);
                    }
                }
                int prev = -1;
                unsigned cnt = 0;
#pragma unroll
                for (int e = 0; e < kV; ++e) {
                    if (e >= e_lo && e < e_hi) {
                        const unsigned v = el[e] >> g.shift;
                        const int key = q * g.bins + (int)(v < (unsigned)g.bins ? v : (unsigned)g.bins - 1u);
                        if (key != prev) {
                            if (cnt) atomicAdd(&counters[prev * ncopy + copy], cnt);
                            prev = key;
                            cnt = 0;
                        }
                        ++cnt;
                        if (w.zmode == kZTile) {
                            if (g.tz == 1) ++q;
                            else if (++rem == g.tz) { rem = 0; ++q; }
                        }
                    }
                }
                if (cnt) atomicAdd(&counters[prev * ncopy + copy], cnt);
            }
        }
    __syncthreads();
    unsigned long long* tile = out + (((size_t)kx * g.nty + ky) * g.ntz + t0) * g.bins;
    for (int i = threadIdx.x; i < nzl * g.bins; i += kThreads) {
        unsigned long long total = 0;
        for (int c = 0; c < ncopy; ++c) total += counters[i * ncopy + c];
        if (total) atomicAdd(&tile[i], total);
    }
}

// tile columns of a few rows: a workgroup takes a share of all the rows of the volume and counts in global memory
template <typename T>
__global__ void __launch_bounds__(kThreads) hist_global_kernel(const T* __restrict__ in, const Geo g, const Walk w,
                                                               unsigned long long* __restrict__ out) {
    constexpr int kV = 16 / (int)sizeof(T);
    const long long rows = (long long)g.X * g.Y, r0 = (long long)blockIdx.x * w.rpw;
    if (r0 >= rows) return;
    const int nrows = (int)(rows - r0 < w.rpw ? rows - r0 : w.rpw);
    const int lr = threadIdx.x / w.lpr, lj = threadIdx.x - lr * w.lpr;
    const RowStart start(r0, 0, 0, g.Y);
    if (lr >= w.rpp) return;
    for (int r = lr; r < nrows; r += w.rpp) {
        int x, y;
        start.at(r, &x, &y);
        const T* row = in + ((size_t)x * g.Y + y) * g.Z;
        unsigned long long* column = out + ((size_t)(x / g.tx) * g.nty + y / g.ty) * g.ntz * g.bins;
        const int lead = (int)(((uintptr_t)row & 15) / sizeof(T));
        for (int j = lj; j < w.U; j += w.lpr) {
            const int zf = -lead + j * kV;
            if (zf >= g.Z) break;
            const int e_lo = zf < 0 ? -zf : 0, e_hi = g.Z - zf < kV ? g.Z - zf : kV;
            unsigned el[kV];
            load_window<T>(el, row + zf, e_lo == 0 && e_hi == kV, e_lo, e_hi);
            int q = (zf + e_lo) / g.tz, rem = (zf + e_lo) - q * g.tz;
            int prev = -1;
            unsigned cnt = 0;
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                if (e >= e_lo && e < e_hi) {
                    const unsigned v = el[e] >> g.shift;
                    const int key = q * g.bins + (int)(v < (unsigned)g.bins ? v : (unsigned)g.bins - 1u);
                    if (key != prev) {
                        if (cnt) atomicAdd(&column[prev], (unsigned long long)cnt);
                        prev = key;
                        cnt = 0;
                    }
                    ++cnt;
                    if (++rem == g.tz) { rem = 0; ++q; }
                }
            }
            if (cnt) atomicAdd(&column[prev], (unsigned long long)cnt);
        }
    }
}

// ---- apply ----

// floor((2 S + W) / (2 W)) = (S + W / 2) / W for S <= W vmax, vmax < 2^16: the quotient from a floating-point estimate
// that is off by less than one, put right with the exact remainder (filter.hip's division)
__device__ __forceinline__ unsigned round_div(unsigned S, unsigned W, float inv, double) {
    unsigned q = (unsigned)((float)S * inv);
    int r = (int)(S - q * W);   // -W < S - q W < 2 W and W < 2^24: right in wrapping 32-bit arithmetic
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

// the pair of an interpolating axis at index i: k0 = floor(p / (2 t)) with p = 2 i + 1 - t > -2 t, and w1 = p - 2 t k0
__device__ __forceinline__ void axis_pair(int i, int t, int* k0, int* w1) {
    const int p = 2 * i + 1 - t;
    *k0 = p < 0 ? -1 : (int)((unsigned)p / (2u * (unsigned)t));
    *w1 = p - 2 * t * *k0;
}
__device__ __forceinline__ int clamp_tile(int k, int n) { return k < 0 ? 0 : (k >= n ? n - 1 : k); }

template <typename T, typename ACC, bool XY, int ZM>
__global__ void __launch_bounds__(kThreads) apply_lds_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             const int* __restrict__ luts, const Geo g, const Walk w,
                                                             const int onx, const int ony, const int same_phase, const ACC W,
                                                             const float inv_f, const double inv_d) {
    extern __shared__ __attribute__((aligned(16))) unsigned short tables[];
    constexpr int kV = 16 / (int)sizeof(T);
    constexpr bool kSum = XY || ZM == kZInterp;
    unsigned b = blockIdx.x;
    const int gz = (int)(b % (unsigned)w.nzc);
    b /= (unsigned)w.nzc;
    const int s = (int)(b % (unsigned)w.nsplit);
    b /= (unsigned)w.nsplit;
    const int nry = g.nty + ony;
    const int ry = (int)(b % (unsigned)nry), rx = (int)(b / (unsigned)nry);
    int xlo, xhi, ylo, yhi;
    region_of(rx, g.tx, g.ntx, g.X, onx, &xlo, &xhi);
    region_of(ry, g.ty, g.nty, g.Y, ony, &ylo, &yhi);
    const int ny = yhi - ylo;
    const long long rows = (long long)(xhi - xlo) * ny, r0 = (long long)s * w.rpw;
    if (r0 >= rows) return;
    const int nrows = (int)(rows - r0 < w.rpw ? rows - r0 : w.rpw);
    const int kxc[2] = {onx ? clamp_tile(rx - 1, g.ntx) : rx, onx ? clamp_tile(rx, g.ntx) : rx};
    const int kyc[2] = {ony ? clamp_tile(ry - 1, g.nty) : ry, ony ? clamp_tile(ry, g.nty) : ry};
    // the chunk's samples [zs, ze) and the z-tiles [tlo, tlo + nzl) they read
    int zs = 0, ze = g.Z, tlo = 0, nzl = 1;
    if (ZM == kZTile) {
        const int t0 = gz * w.zc, t1 = g.ntz - t0 < w.zc ? g.ntz : t0 + w.zc;
        const long long a = (long long)t0 * g.tz, e = (long long)t1 * g.tz;
        zs = (int)a;
        ze = (int)(e < g.Z ? e : g.Z);
        tlo = t0;
        nzl = t1 - t0;
    } else if (ZM == kZInterp) {   // a chunk of z cells c0 .. c1; cell c reads the tiles c - 1 and c
        const int c0 = gz * w.zc, c1 = (g.ntz + 1 - c0 < w.zc ? g.ntz + 1 : c0 + w.zc) - 1;
        int unused;
        region_of(c0, g.tz, g.ntz, g.Z, 1, &zs, &unused);
        region_of(c1, g.tz, g.ntz, g.Z, 1, &unused, &ze);
        tlo = clamp_tile(c0 - 1, g.ntz);
        nzl = clamp_tile(c1, g.ntz) - tlo + 1;
    }
    for (int c = 0; c < (XY ? 4 : 1); ++c)
        for (int zl = 0; zl < nzl; ++zl) {
            const int* src = luts + (((size_t)kxc[c & 1] * g.nty + kyc[c >> 1]) * g.ntz + tlo + zl) * g.bins;
            unsigned short* dst = tables + (size_t)(c * nzl + zl) * g.bins;
            for (int i = threadIdx.x; i < g.bins; i += kThreads) dst[i] = (unsigned short)src[i];
        }
    __syncthreads();

    const int lr = threadIdx.x / w.lpr, lj = threadIdx.x - lr * w.lpr;
    const RowStart start(r0, xlo, ylo, ny);
    const int corner = nzl * g.bins;
    if (lr >= w.rpp) return;
    for (int r = lr; r < nrows; r += w.rpp) {
        int x, y;
        start.at(r, &x, &y);
        ACC wc[4] = {1, 0, 0, 0};
        if (XY) {
            const int wx1 = onx ? 2 * x + 1 - g.tx - 2 * g.tx * (rx - 1) : 0, wx0 = onx ? 2 * g.tx - wx1 : 1;
            const int wy1 = ony ? 2 * y + 1 - g.ty - 2 * g.ty * (ry - 1) : 0, wy0 = ony ? 2 * g.ty - wy1 : 1;
            wc[0] = (ACC)wx0 * (ACC)wy0;
            wc[1] = (ACC)wx1 * (ACC)wy0;
            wc[2] = (ACC)wx0 * (ACC)wy1;
            wc[3] = (ACC)wx1 * (ACC)wy1;
        }
        const size_t base = ((size_t)x * g.Y + y) * g.Z;
        const T* src = in + base;
        T* dst = out + base;
        const int lead = (int)(((uintptr_t)(dst + zs) & 15) / sizeof(T));
        for (int j = lj; j < w.U; j += w.lpr) {
            const int zf = zs - lead + j * kV;
            if (zf >= ze) break;
            const int e_lo = zs > zf ? zs - zf : 0, e_hi = ze - zf < kV ? ze - zf : kV;
            const bool full = e_lo == 0 && e_hi == kV;
            unsigned el[kV], o[kV];
            load_window<T>(el, src + zf, full && same_phase, e_lo, e_hi);
            int q = 0, rem = 0;        // kZTile: the z-tile and the place in it; kZInterp: k0 and w1
            if (ZM == kZTile) {
                q = (zf + e_lo) / g.tz;
                rem = zf + e_lo - q * g.tz;
            } else if (ZM == kZInterp) {
                axis_pair(zf + e_lo, g.tz, &q, &rem);
            }
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                o[e] = 0;
                if (e >= e_lo && e < e_hi) {
                    const unsigned v = el[e] >> g.shift;
                    const int bin = (int)(v < (unsigned)g.bins ? v : (unsigned)g.bins - 1u);
                    if (!kSum) {
                        o[e] = tables[(ZM == kZTile ? q - tlo : 0) * g.bins + bin];
                    } else {
                        ACC S = 0;
                        if (ZM == kZInterp) {
                            const int a0 = (clamp_tile(q, g.ntz) - tlo) * g.bins + bin;
                            const int a1 = (clamp_tile(q + 1, g.ntz) - tlo) * g.bins + bin;
                            const ACC w1 = (ACC)rem, w0 = (ACC)(2 * g.tz - rem);
#pragma unroll
                            for (int c = 0; c < (XY ? 4 : 1); ++c)
                                S += wc[c] * (w0 * (ACC)tables[c * corner + a0] + w1 * (ACC)tables[c * corner + a1]);
                        } else {
                            const int a0 = (ZM == kZTile ? q - tlo : 0) * g.bins + bin;
#pragma unroll
                            for (int c = 0; c < 4; ++c) S += wc[c] * (ACC)tables[c * corner + a0];
                        }
                        o[e] = round_div(S, W, inv_f, inv_d);
                    }
                    if (ZM == kZTile) {
                        if (++rem == g.tz) { rem = 0; ++q; }
                    } else if (ZM == kZInterp) {
                        rem += 2;
                        if (rem >= 2 * g.tz) { rem -= 2 * g.tz; ++q; }
                    }
                }
            }
            store_window<T>(dst + zf, o, full, e_lo, e_hi);
        }
    }
}

// cells of a few rows: a workgroup takes a share of all the rows of the volume and reads the tables from global memory
template <typename T, typename ACC>
__global__ void __launch_bounds__(kThreads) apply_gather_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                const int* __restrict__ luts, const Geo g, const Walk w,
                                                                const int onx, const int ony, const int onz, const int same_phase,
                                                                const ACC W, const float inv_f, const double inv_d) {
    constexpr int kV = 16 / (int)sizeof(T);
    const long long rows = (long long)g.X * g.Y, r0 = (long long)blockIdx.x * w.rpw;
    if (r0 >= rows) return;
    const int nrows = (int)(rows - r0 < w.rpw ? rows - r0 : w.rpw);
    const int lr = threadIdx.x / w.lpr, lj = threadIdx.x - lr * w.lpr;
    const RowStart start(r0, 0, 0, g.Y);
    if (lr >= w.rpp) return;
    const bool sum = onx || ony || onz;
    for (int r = lr; r < nrows; r += w.rpp) {
        int x, y;
        start.at(r, &x, &y);
        int kx0 = x / g.tx, wx1 = 0, ky0 = y / g.ty, wy1 = 0;
        if (onx) axis_pair(x, g.tx, &kx0, &wx1);
        if (ony) axis_pair(y, g.ty, &ky0, &wy1);
        const int wx0 = onx ? 2 * g.tx - wx1 : 1, wy0 = ony ? 2 * g.ty - wy1 : 1;
        const int kxc[2] = {clamp_tile(kx0, g.ntx), clamp_tile(kx0 + (onx ? 1 : 0), g.ntx)};
        const int kyc[2] = {clamp_tile(ky0, g.nty), clamp_tile(ky0 + (ony ? 1 : 0), g.nty)};
        const ACC wc[4] = {(ACC)wx0 * (ACC)wy0, (ACC)wx1 * (ACC)wy0, (ACC)wx0 * (ACC)wy1, (ACC)wx1 * (ACC)wy1};
        const int* column[4];
        for (int c = 0; c < 4; ++c) column[c] = luts + ((size_t)kxc[c & 1] * g.nty + kyc[c >> 1]) * g.ntz * g.bins;
        const size_t base = ((size_t)x * g.Y + y) * g.Z;
        const T* src = in + base;
        T* dst = out + base;
        const int lead = (int)(((uintptr_t)dst & 15) / sizeof(T));
        for (int j = lj; j < w.U; j += w.lpr) {
            const int zf = -lead + j * kV;
            if (zf >= g.Z) break;
            const int e_lo = zf < 0 ? -zf : 0, e_hi = g.Z - zf < kV ? g.Z - zf : kV;
            const bool full = e_lo == 0 && e_hi == kV;
            unsigned el[kV], o[kV];
            load_window<T>(el, src + zf, full && same_phase, e_lo, e_hi);
            int q, rem;
            if (onz) axis_pair(zf + e_lo, g.tz, &q, &rem);
            else {
                q = (zf + e_lo) / g.tz;
                rem = zf + e_lo - q * g.tz;
            }
#pragma unroll
            for (int e = 0; e < kV; ++e) {
                o[e] = 0;
                if (e >= e_lo && e < e_hi) {
                    const unsigned v = el[e] >> g.shift;
                    const int bin = (int)(v < (unsigned)g.bins ? v : (unsigned)g.bins - 1u);
                    const size_t a0 = (size_t)clamp_tile(q, g.ntz) * g.bins + bin;
                    if (!sum) {
                        o[e] = (unsigned)column[0][a0];
                    } else {
                        const size_t a1 = (size_t)clamp_tile(q + (onz ? 1 : 0), g.ntz) * g.bins + bin;
                        const ACC w1 = onz ? (ACC)rem : (ACC)0, w0 = onz ? (ACC)(2 * g.tz - rem) : (ACC)1;
                        ACC S = 0;
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (wc[c] != 0) S += wc[c] * (w0 * (ACC)(unsigned)column[c][a0] + w1 * (ACC)(unsigned)column[c][a1]);
                        o[e] = round_div(S, W, inv_f, inv_d);
                    }
                    if (onz) {
                        rem += 2;
                        if (rem >= 2 * g.tz) { rem -= 2 * g.tz; ++q; }
                    } else if (++rem == g.tz) { rem = 0; ++q; }
                }
            }
            store_window<T>(dst + zf, o, full, e_lo, e_hi);
        }
    }
}

// ---- host ----

int check_geometry(const char* who, int dtype, int X, int Y, int Z, int tx, int ty, int tz, int bins, int shift, Geo* g) {
    SK_CHECK_ARG(dtype == SK_U8 || dtype == SK_U16, "%s: dtype = %d, must be uint8 (4) or uint16 (5)", who, dtype);
    SK_CHECK_ARG(X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent,
                 "%s: extents (%d, %d, %d) outside 1 .. 2^30", who, X, Y, Z);
    SK_CHECK_ARG(tx >= 0 && ty >= 0 && tz >= 0, "%s: tile (%d, %d, %d): every side must be >= 1, or 0 for the whole axis", who, tx,
                 ty, tz);
    if (dtype == SK_U8)
        SK_CHECK_ARG(bins == 256 && shift == 0, "%s: uint8 takes bins = 256 and shift = 0, got %d and %d", who, bins, shift);
    else {
        SK_CHECK_ARG(bins == 256 || bins == 1024 || bins == 4096, "%s: bins = %d, uint16 takes 256, 1024 or 4096", who, bins);
        SK_CHECK_ARG(shift >= 0 && shift <= 8, "%s: shift = %d outside 0 .. 8", who, shift);
    }
    const int N[3] = {X, Y, Z}, t[3] = {tx, ty, tz};
    int te[3], nt[3];
    for (int a = 0; a < 3; ++a) {
        te[a] = t[a] == 0 || t[a] > N[a] ? N[a] : t[a];
        nt[a] = (N[a] + te[a] - 1) / te[a];
    }
    *g = Geo{X, Y, Z, te[0], te[1], te[2], nt[0], nt[1], nt[2], bins, shift};
    return SK_OK;
}

// rows of `rows_max` at most per region, each a z segment of `span` samples at most: the shares and the thread layout
int plan_walk(const char* who, const Geo& g, int eb, long long regions, long long rows_max, int span, long long entries,
              bool lead_free, Walk* w) {
    const int kV = 16 / eb;
    const double work = (double)rows_max * (double)span;
    double want = work / (8.0 * (double)entries);                        // a share is worth 8 times its tables
    const double fill = 4096.0 / ((double)regions * (double)w->nzc);    // and there is no need for more than 4096 workgroups
    if (want > fill) want = fill;
    if (want < 1.0) want = 1.0;
    long long rpw = (long long)((double)rows_max / want);
    if (rpw < 1) rpw = 1;
    const long long cap = ((1LL << 31) / span) < (1LL << 30) ? (1LL << 31) / span : (1LL << 30);   // < 2^32 samples a share
    if (rpw > cap) rpw = cap;
    if (rpw > rows_max) rpw = rows_max;
    const long long nsplit = (rows_max + rpw - 1) / rpw;
    const unsigned __int128 blocks = (unsigned __int128)regions * (unsigned)w->nzc * (unsigned long long)nsplit;
    SK_CHECK_ARG(blocks <= 0x7FFFFFFFULL, "%s: the workgroups of this geometry do not fit one grid", who);
    w->nsplit = (int)nsplit;
    w->rpw = (int)rpw;
    w->U = lead_free ? (span + kV - 1) / kV : (span + 2 * kV - 2) / kV;
    w->lpr = w->U < kThreads ? w->U : kThreads;
    w->rpp = kThreads / w->lpr;
    return SK_OK;
}

struct HistPlan {
    int path, ncopy;
    Walk w;
    unsigned blocks;
    size_t lds;
};

int plan_hist(const char* who, const Geo& g, int eb, uintptr_t base, HistPlan* p) {
    Walk& w = p->w;
    const long long rows_max = (long long)g.tx * g.ty;
    const bool rows_aligned = (base & 15) == 0 && ((size_t)g.Z * eb) % 16 == 0;
    if (rows_max < kMinRows) {
        p->path = SK_EQUALIZE_HIST_GLOBAL;
        p->ncopy = 1;
        p->lds = 0;
        w.zmode = kZTile;
        w.nzc = 1;
        w.zc = g.ntz;
        const int rc = plan_walk(who, g, eb, 1, (long long)g.X * g.Y, g.Z, 4096, rows_aligned, &w);
        if (rc != SK_OK) return rc;
        p->blocks = (unsigned)w.nsplit;
        return SK_OK;
    }
    int per = kHistCounters / g.bins;                                  // z-tiles a workgroup can count
    if (g.ntz == 1) {
        w.zmode = kZOne;
        w.zc = 1;
        w.nzc = 1;
        p->path = SK_EQUALIZE_HIST_ONE;
    } else {
        if (g.tz > 1) {                                                // no more z-tiles than 256 samples need
            const int few = (256 + g.tz - 1) / g.tz;
            if (per > few) per = few;
        }
        w.zmode = kZTile;
        w.zc = per < g.ntz ? per : g.ntz;
        w.nzc = (g.ntz + w.zc - 1) / w.zc;
        p->path = g.tz == 1 ? SK_EQUALIZE_HIST_PLANES : w.zc == 1 ? SK_EQUALIZE_HIST_ONE : SK_EQUALIZE_HIST_ZTILES;
    }
    const long long span64 = w.zmode == kZOne ? g.Z : (long long)w.zc * g.tz;
    const int span = (int)(span64 < g.Z ? span64 : g.Z);
    int ncopy = 1;
    while (ncopy < 32 && w.zc * g.bins * ncopy * 2 <= kHistCounters) ncopy *= 2;
    p->ncopy = ncopy;
    p->lds = (size_t)w.zc * g.bins * ncopy * sizeof(unsigned);
    const bool lead_free = rows_aligned && (w.zmode == kZOne || ((size_t)span * eb) % 16 == 0);
    const int rc = plan_walk(who, g, eb, (long long)g.ntx * g.nty, rows_max, span, (long long)w.zc * g.bins * ncopy, lead_free, &w);
    if (rc != SK_OK) return rc;
    p->blocks = (unsigned)((long long)g.ntx * g.nty * w.nzc * w.nsplit);
    return SK_OK;
}

struct ApplyPlan {
    int path, onx, ony, onz, wide;
    unsigned long long W;
    Walk w;
    unsigned blocks;
    size_t lds;
};

int plan_apply(const char* who, const Geo& g, int eb, int interpolate, uintptr_t base, ApplyPlan* p) {
    Walk& w = p->w;
    p->onx = interpolate && g.ntx > 1 && g.tx > 1;
    p->ony = interpolate && g.nty > 1 && g.ty > 1;
    p->onz = interpolate && g.ntz > 1 && g.tz > 1;
    const unsigned long long top = eb == 1 ? 255 : 65535;
    unsigned __int128 W = 1;
    if (p->onx) W *= 2ULL * g.tx;
    if (p->ony) W *= 2ULL * g.ty;
    if (p->onz) W *= 2ULL * g.tz;
    SK_CHECK_ARG(W * top < ((unsigned __int128)1 << 62), "%s: the weights of tile (%d, %d, %d) do not fit 64-bit sums", who, g.tx, g.ty,
                 g.tz);
    p->W = (unsigned long long)W;
    p->wide = p->W * top >= (1ULL << 32);
    const bool sum = p->onx || p->ony || p->onz;
    const int xy = p->onx || p->ony;
    const int zmode = g.ntz == 1 ? kZOne : p->onz ? kZInterp : kZTile;
    p->path = zmode | (xy ? SK_EQUALIZE_APPLY_XY : 0) | (!sum ? 0 : p->wide ? SK_EQUALIZE_APPLY_ACC64 : SK_EQUALIZE_APPLY_ACC32);
    const bool rows_aligned = (base & 15) == 0 && ((size_t)g.Z * eb) % 16 == 0;
    const long long rows_max = (long long)g.tx * g.ty;
    if (rows_max < kMinRows) {
        p->path |= SK_EQUALIZE_APPLY_GATHER;
        p->lds = 0;
        w.zmode = zmode;
        w.nzc = 1;
        w.zc = g.ntz;
        const int rc = plan_walk(who, g, eb, 1, (long long)g.X * g.Y, g.Z, 4096, rows_aligned, &w);
        if (rc != SK_OK) return rc;
        p->blocks = (unsigned)w.nsplit;
        return SK_OK;
    }
    const int corners = xy ? 4 : 1, extra = zmode == kZInterp ? 1 : 0;   // z interpolates: chunks of cells, one tile more
    w.zmode = zmode;
    if (zmode == kZOne) {
        w.zc = 1;
        w.nzc = 1;
    } else {
        int per = kApplyEntries / (corners * g.bins) - extra;
        if (g.tz > 1) {                                                // no more z-tiles than 256 samples need
            const int few = (256 + g.tz - 1) / g.tz;
            if (per > few) per = few;
        }
        if (per < 1) per = 1;
        const int units = g.ntz + extra;                               // z-tiles, or the cells between their centres
        w.zc = per < units ? per : units;
        w.nzc = (units + w.zc - 1) / w.zc;
    }
    const int nzl = zmode == kZOne ? 1 : (w.zc + extra < g.ntz ? w.zc + extra : g.ntz);
    const long long entries = (long long)corners * nzl * g.bins;
    p->lds = (size_t)entries * sizeof(unsigned short);
    const long long span64 = zmode == kZOne ? g.Z : (long long)w.zc * g.tz;
    const int span = (int)(span64 < g.Z ? span64 : g.Z);
    const bool lead_free = rows_aligned && (zmode == kZOne || (zmode == kZTile && ((size_t)span * eb) % 16 == 0));
    const long long regions = (long long)(g.ntx + p->onx) * (g.nty + p->ony);
    const int rc = plan_walk(who, g, eb, regions, rows_max, span, entries, lead_free, &w);
    if (rc != SK_OK) return rc;
    p->blocks = (unsigned)(regions * w.nzc * w.nsplit);
    return SK_OK;
}

template <typename T, typename ACC, bool XY>
void launch_apply_z(const ApplyPlan& p, hipStream_t st, const void* in, void* out, const int* luts, const Geo& g, int same_phase) {
    const dim3 grid(p.blocks), block(kThreads);
    const ACC W = (ACC)p.W;
    const float inv_f = 1.0f / (float)p.W;
    const double inv_d = 1.0 / (double)p.W;
    if (p.w.zmode == kZOne)
        apply_lds_kernel<T, ACC, XY, kZOne><<<grid, block, p.lds, st>>>((const T*)in, (T*)out, luts, g, p.w, p.onx, p.ony, same_phase,
                                                                        W, inv_f, inv_d);
    else if (p.w.zmode == kZTile)
        apply_lds_kernel<T, ACC, XY, kZTile><<<grid, block, p.lds, st>>>((const T*)in, (T*)out, luts, g, p.w, p.onx, p.ony, same_phase,
                                                                         W, inv_f, inv_d);
    else
        apply_lds_kernel<T, ACC, XY, kZInterp><<<grid, block, p.lds, st>>>((const T*)in, (T*)out, luts, g, p.w, p.onx, p.ony,
                                                                           same_phase, W, inv_f, inv_d);
}

template <typename T>
void launch_apply(const ApplyPlan& p, hipStream_t st, const void* in, void* out, const int* luts, const Geo& g, int same_phase) {
    if (p.path & SK_EQUALIZE_APPLY_GATHER) {
        const dim3 grid(p.blocks), block(kThreads);
        if (p.wide)
            apply_gather_kernel<T, unsigned long long><<<grid, block, 0, st>>>((const T*)in, (T*)out, luts, g, p.w, p.onx, p.ony, p.onz,
                                                                               same_phase, p.W, 0.0f, 1.0 / (double)p.W);
        else
            apply_gather_kernel<T, unsigned><<<grid, block, 0, st>>>((const T*)in, (T*)out, luts, g, p.w, p.onx, p.ony, p.onz, same_phase,
                                                                     (unsigned)p.W, 1.0f / (float)p.W, 0.0);
        return;
    }
    const bool xy = p.onx || p.ony;
    if (p.wide) {
        if (xy) launch_apply_z<T, unsigned long long, true>(p, st, in, out, luts, g, same_phase);
        else launch_apply_z<T, unsigned long long, false>(p, st, in, out, luts, g, same_phase);
    } else {
        if (xy) launch_apply_z<T, unsigned, true>(p, st, in, out, luts, g, same_phase);
        else launch_apply_z<T, unsigned, false>(p, st, in, out, luts, g, same_phase);
    }
}

}  // namespace

extern "C" int sk_equalize_path(int which, int dtype, int X, int Y, int Z, int tx, int ty, int tz, int bins, int shift,
                                int interpolate) {
    SK_CHECK_ARG(which == 0 || which == 1, "sk_equalize_path: which = %d, must be 0 (histograms) or 1 (apply)", which);
    Geo g;
    int rc = check_geometry("sk_equalize_path", dtype, X, Y, Z, tx, ty, tz, bins, shift, &g);
    if (rc != SK_OK) return rc;
    const int eb = dtype == SK_U8 ? 1 : 2;
    if (which == 0) {
        HistPlan p;
        rc = plan_hist("sk_equalize_path", g, eb, 0, &p);
        return rc != SK_OK ? rc : p.path;
    }
    ApplyPlan p;
    rc = plan_apply("sk_equalize_path", g, eb, interpolate != 0, 0, &p);
    return rc != SK_OK ? rc : p.path;
}

extern "C" int sk_tile_histograms(const void* in, int dtype, int X, int Y, int Z, int tx, int ty, int tz, int bins, int shift,
                                  long long* out_counts, void* stream) {
    SK_CHECK_ARG(in && out_counts, "sk_tile_histograms: NULL pointer");
    Geo g;
    int rc = check_geometry("sk_tile_histograms", dtype, X, Y, Z, tx, ty, tz, bins, shift, &g);
    if (rc != SK_OK) return rc;
    const int eb = dtype == SK_U8 ? 1 : 2;
    SK_CHECK_ARG(((uintptr_t)in & (eb - 1)) == 0, "sk_tile_histograms: in is not aligned to its elements");
    SK_CHECK_ARG(((uintptr_t)out_counts & 7) == 0, "sk_tile_histograms: out_counts must be 8-byte aligned");
    HistPlan p;
    rc = plan_hist("sk_tile_histograms", g, eb, (uintptr_t)in, &p);
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)g.ntx * g.nty * g.ntz * g.bins * sizeof(long long);
    SK_CHECK_HIP(hipMemsetAsync(out_counts, 0, bytes, st));
    unsigned long long* out = (unsigned long long*)out_counts;
    const dim3 grid(p.blocks), block(kThreads);
    if (p.path == SK_EQUALIZE_HIST_GLOBAL) {
        if (eb == 1) hist_global_kernel<uint8_t><<<grid, block, 0, st>>>((const uint8_t*)in, g, p.w, out);
        else hist_global_kernel<uint16_t><<<grid, block, 0, st>>>((const uint16_t*)in, g, p.w, out);
    } else {
        if (eb == 1) hist_lds_kernel<uint8_t><<<grid, block, p.lds, st>>>((const uint8_t*)in, g, p.w, p.ncopy, out);
        else hist_lds_kernel<uint16_t><<<grid, block, p.lds, st>>>((const uint16_t*)in, g, p.w, p.ncopy, out);
    }
    SK_CHECK_LAUNCH();
    return SK_OK;
}

extern "C" int sk_apply_tile_luts(const void* in, void* out, int dtype, int X, int Y, int Z, int tx, int ty, int tz,
                                  const int* luts, int bins, int shift, int interpolate, void* stream) {
    SK_CHECK_ARG(in && out && luts, "sk_apply_tile_luts: NULL pointer");
    SK_CHECK_ARG(in != out, "sk_apply_tile_luts: in == out: the pass does not run in place");
    Geo g;
    int rc = check_geometry("sk_apply_tile_luts", dtype, X, Y, Z, tx, ty, tz, bins, shift, &g);
    if (rc != SK_OK) return rc;
    const int eb = dtype == SK_U8 ? 1 : 2;
    SK_CHECK_ARG(((uintptr_t)in & (eb - 1)) == 0 && ((uintptr_t)out & (eb - 1)) == 0,
                 "sk_apply_tile_luts: in or out is not aligned to its elements");
    SK_CHECK_ARG(((uintptr_t)luts & 3) == 0, "sk_apply_tile_luts: luts must be 4-byte aligned");
    SK_CHECK_ARG(interpolate == 0 || interpolate == 1, "sk_apply_tile_luts: interpolate = %d, must be 0 or 1", interpolate);
    ApplyPlan p;
    rc = plan_apply("sk_apply_tile_luts", g, eb, interpolate, (uintptr_t)out, &p);
    if (rc != SK_OK) return rc;
    const int same_phase = (((uintptr_t)in ^ (uintptr_t)out) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (eb == 1) launch_apply<uint8_t>(p, st, in, out, luts, g, same_phase);
    else launch_apply<uint16_t>(p, st, in, out, luts, g, same_phase);
    SK_CHECK_LAUNCH();
    return SK_OK;
}
