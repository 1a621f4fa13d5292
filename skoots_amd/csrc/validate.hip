// Dice and soft-clDice validation matrices (skoots/validate/lib.py:232-315 mask_dice / mask_soft_cldice, the
// metrics of skoots/validate/__main__.py).  The reference forms two full-volume binary masks per touching
// (gt, pred) pair and runs two soft skeletons on them.  On a (1, X, Y, Z) int mask its soft_skeletonize takes the 4-D
// branch, so the skeleton is 2-D in every (Y, Z) slice, and on a binary mask it is exactly binary: every clDice sum is
// an integer count.  Each voxel carries one label, so all instances are skeletonised in one stencil pass:
//   D(u)  own-label cross-erosion depth in its slice, capped at iters + 1 (step k keeps u if u and its in-slice
//         4-neighbours were kept at step k - 1 and carry u's label; out-of-slice neighbours are ignored: the
//         reference's max-pool padding is -inf);
//   skel  label(u) > 0 and no w in u's in-slice 3x3 window has label(u) and D(w) >= min(D(u), iters) + 1.
// One pass then fills three (N+1) x (M+1) int32 contingency tables (plain, pred skeleton at x >= 1, gt skeleton at
// x >= 1) and a finalize kernel writes IoU / Dice / clDice in the reference's fp32 operation order.
#include "common.h"

namespace {

constexpr int kTZ = 64;        // output tile: one wave row along z (the fastest index) ...
constexpr int kTY = 32;        // ... by 32 rows along y, 4 waves of 8 rows
constexpr int kMaxIters = 12;  // halo iters + 2 <= 14: two planes of (32 + 28) x (64 + 28) x 5 B = 55 KB of LDS

__host__ __device__ inline int halo_of(bool skel, int iters) { return skel ? iters + 2 : 0; }

// LDS bytes of one tile: P planes of int32 labels and uint8 depths
inline size_t tile_lds_bytes(int planes, int halo) {
    return (size_t)planes * (kTY + 2 * halo) * (kTZ + 2 * halo) * (sizeof(int) + 1);
}

// Stage plane (x, y0 - halo .. y0 + kTY + halo, z0 - halo .. z0 + kTZ + halo): raw id > 0 kept, every other id -> 0,
// out-of-slice -> -1.  Depths start at 0.
__device__ inline void stage(const int* __restrict__ lab, int Y, int Z, long long plane, int y0, int z0, int halo,
                             int W, int R, int* s_lab, uint8_t* s_d) {
    for (int p = threadIdx.x; p < W * R; p += 256) {
        const int y = y0 - halo + p / W, z = z0 - halo + p % W;
        int v = -1;
        if (y >= 0 && y < Y && z >= 0 && z < Z) {
            v = lab[plane + (long long)y * Z + z];
            v = v > 0 ? v : 0;
        }
        s_lab[p] = v;
        s_d[p] = 0;
    }
}

// Step k of the cross erosion, in place: a position at distance >= k from the staged border has every input it
// needs.  A step only raises k - 1 to k and its test reads ">= k - 1", so the in-place order does not matter.
__device__ inline void erode_step(const int* s_lab, uint8_t* s_d, int W, int R, int k) {
    const int w = W - 2 * k, h = R - 2 * k;
    for (int p = threadIdx.x; p < w * h; p += 256) {
        const int q = (k + p / w) * W + k + p % w;
        const int v = s_lab[q];
        if (v <= 0 || s_d[q] != k - 1) continue;
        bool keep = true;
        const int nb[4] = {q - W, q + W, q - 1, q + 1};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int u = s_lab[nb[t]];
            keep = keep && (u == -1 || (u == v && s_d[nb[t]] >= k - 1));
        }
        if (keep) s_d[q] = (uint8_t)k;
    }
}

// Skeleton flag of staged position q (an output position: at distance halo >= iters + 2 from the border)
__device__ inline bool skel_at(const int* s_lab, const uint8_t* s_d, int W, int q, int iters) {
    const int v = s_lab[q];
    if (v <= 0) return false;
    const int m = min((int)s_d[q], iters) + 1;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
            const int u = q + dy * W + dz;
            if (s_lab[u] == v && s_d[u] >= m) return false;
        }
    return true;
}

__global__ void __launch_bounds__(256) label_skeleton_kernel(const int* __restrict__ lab, int Y, int Z, int iters,
                                                             long long ntiles, int tiles_y, int tiles_z,
                                                             uint8_t* __restrict__ skel) {
    extern __shared__ int s_mem[];
    const int halo = iters + 2, W = kTZ + 2 * halo, R = kTY + 2 * halo;
    int* s_lab = s_mem;
    uint8_t* s_d = (uint8_t*)(s_lab + W * R);
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tz = (int)(t % tiles_z), ty = (int)(t / tiles_z % tiles_y);
        const long long x = t / ((long long)tiles_z * tiles_y);
        const long long plane = x * Y * Z;
        const int y0 = ty * kTY, z0 = tz * kTZ;
        __syncthreads();  // the previous tile's readers are done
        stage(lab, Y, Z, plane, y0, z0, halo, W, R, s_lab, s_d);
        for (int k = 1; k <= iters + 1; ++k) {
            __syncthreads();
            erode_step(s_lab, s_d, W, R, k);
        }
        __syncthreads();
        for (int p = threadIdx.x; p < kTY * kTZ; p += 256) {
            const int y = y0 + p / kTZ, z = z0 + p % kTZ;
            if (y >= Y || z >= Z) continue;
            const int q = (halo + p / kTZ) * W + halo + p % kTZ;
            skel[plane + (long long)y * Z + z] = skel_at(s_lab, s_d, W, q, iters) ? 1 : 0;
        }
    }
}

// One atomic per run of equal cells along the wave's row (lanes = consecutive z): the background-heavy cells
// (a, 0) / (0, b) otherwise take one atomic per voxel on the same address.  Measured: it pays in the
// skeleton kernel and not in the plain one, which keeps one atomic per voxel.  SK_VALIDATE_RUNS = 0 builds the
// one-atomic-per-voxel form everywhere, for the A/B.
#ifndef SK_VALIDATE_RUNS
#define SK_VALIDATE_RUNS 1
#endif
template <bool kRuns>
__device__ inline void add_runs(int* __restrict__ table, bool valid, int cell) {
    if (!kRuns || !SK_VALIDATE_RUNS) {
        if (valid) atomicAdd(&table[cell], 1);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int prev_cell = __shfl_up(cell, 1);
    const int prev_valid = __shfl_up((int)valid, 1);
    const bool cont = valid && lane > 0 && prev_valid && prev_cell == cell;
    const unsigned long long cmask = __ballot(cont);
    if (valid && !cont) {
        const unsigned long long rest = lane == 63 ? 0ull : cmask >> (lane + 1);
        atomicAdd(&table[cell], 1 + __builtin_ctzll(~rest));
    }
}

// kSkel = false: the plain table only (no halo, no skeleton; Dice / IoU alone)
template <bool kSkel>
__global__ void __launch_bounds__(256) metrics_table_kernel(const int* __restrict__ gt, const int* __restrict__ pred,
                                                            int Y, int Z, int iters, long long ntiles, int tiles_y,
                                                            int tiles_z, const int* __restrict__ lut_a, int max_a,
                                                            const int* __restrict__ lut_b, int max_b, int M1,
                                                            int* __restrict__ t_all, int* __restrict__ t_sp,
                                                            int* __restrict__ t_sg) {
    extern __shared__ int s_mem[];
    const int halo = halo_of(kSkel, iters), W = kTZ + 2 * halo, R = kTY + 2 * halo;
    int* s_a = s_mem;
    int* s_b = s_a + W * R;
    uint8_t* s_da = (uint8_t*)(s_b + W * R);
    uint8_t* s_db = s_da + W * R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tz = (int)(t % tiles_z), ty = (int)(t / tiles_z % tiles_y);
        const long long x = t / ((long long)tiles_z * tiles_y);
        const long long plane = x * Y * Z;
        const int y0 = ty * kTY, z0 = tz * kTZ;
        __syncthreads();
        stage(gt, Y, Z, plane, y0, z0, halo, W, R, s_a, s_da);
        stage(pred, Y, Z, plane, y0, z0, halo, W, R, s_b, s_db);
        if (kSkel) {
            for (int k = 1; k <= iters + 1; ++k) {
                __syncthreads();
                erode_step(s_a, s_da, W, R, k);
                erode_step(s_b, s_db, W, R, k);
            }
        }
        __syncthreads();
        const int z = z0 + lane;
        for (int r = wave; r < kTY; r += 4) {  // wave-uniform: every lane reaches the ballots
            const int y = y0 + r;
            const bool in = y < Y && z < Z;
            const int q = (halo + r) * W + halo + lane;
            const int va = in ? s_a[q] : 0, vb = in ? s_b[q] : 0;
            const int ra = (va > 0 && va <= max_a) ? lut_a[va] : 0;
            const int rb = (vb > 0 && vb <= max_b) ? lut_b[vb] : 0;
            const int cell = ra * M1 + rb;
            add_runs<kSkel>(t_all, (ra | rb) != 0, cell);  // (0, 0) is never needed
            if (kSkel) {
                const bool tail = in && x >= 1;      // the reference's [:, 1:, ...]: x = 0 is out of the clDice sums
                add_runs<true>(t_sp, tail && rb > 0 && skel_at(s_b, s_db, W, q, iters), cell);
                add_runs<true>(t_sg, tail && ra > 0 && skel_at(s_a, s_da, W, q, iters), cell);
            }
        }
    }
}

// rows of t_all and t_sg (one wave per row), then columns of t_all and t_sp (one thread per column)
__global__ void __launch_bounds__(256) row_sums_kernel(const int* __restrict__ t_all, const int* __restrict__ t_sg,
                                                       int N1, int M1, long long* __restrict__ row_all,
                                                       long long* __restrict__ row_sg) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N1) return;
    long long s0 = 0, s1 = 0;
    for (int j = lane; j < M1; j += 64) {
        s0 += t_all[(long long)i * M1 + j];
        if (t_sg) s1 += t_sg[(long long)i * M1 + j];
    }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
    }
    if (lane == 0) {
        row_all[i] = s0;
        row_sg[i] = s1;
    }
}

__global__ void __launch_bounds__(256) col_sums_kernel(const int* __restrict__ t_all, const int* __restrict__ t_sp,
                                                       int N1, int M1, long long* __restrict__ col_all,
                                                       long long* __restrict__ col_sp) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M1) return;
    long long s0 = 0, s1 = 0;
    for (int i = 0; i < N1; ++i) {
        s0 += t_all[(long long)i * M1 + j];
        if (t_sp) s1 += t_sp[(long long)i * M1 + j];
    }
    col_all[j] = s0;
    col_sp[j] = s1;
}

// Every matrix entry follows the reference's fp32 order (lib.py:224, 273-278, loss.py:329-338); the library builds
// with -ffp-contract=off.  A pair that does not touch (no voxel with gt = a and pred = b, any x) is 0.
__global__ void __launch_bounds__(256) finalize_kernel(const int* __restrict__ t_all, const int* __restrict__ t_sp,
                                                       const int* __restrict__ t_sg,
                                                       const long long* __restrict__ row_all,
                                                       const long long* __restrict__ col_all,
                                                       const long long* __restrict__ row_sg,
                                                       const long long* __restrict__ col_sp, int N, int M,
                                                       float* __restrict__ iou, float* __restrict__ dice,
                                                       float* __restrict__ cldice) {
    const long long n = (long long)N * M;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const int i = (int)(t / M), j = (int)(t % M);
        const long long c = (long long)(i + 1) * (M + 1) + (j + 1);
        const long long inter = t_all[c];
        const bool touch = inter > 0;
        const long long ra = row_all[i + 1], cb = col_all[j + 1];
        if (iou) iou[t] = touch ? (float)inter / (float)(ra + cb - inter) : 0.0f;
        if (dice) dice[t] = touch ? (float)(2 * inter) / (float)(ra + cb) : 0.0f;
        if (cldice) {
            float v = 0.0f;
            if (touch) {
                const float tprec = ((float)t_sp[c] + 1.0f) / ((float)col_sp[j + 1] + 1.0f);
                const float tsens = ((float)t_sg[c] + 1.0f) / ((float)row_sg[i + 1] + 1.0f);
                v = 1.0f - (2.0f * (tprec * tsens)) / (tprec + tsens);
            }
            cldice[t] = v;
        }
    }
}

inline size_t table_bytes(int N, int M) { return ((size_t)(N + 1) * (M + 1) * sizeof(int) + 15) / 16 * 16; }

struct Tiles {
    long long n;
    int ty, tz;
};
inline Tiles tiles_of(int X, int Y, int Z) {
    const int ty = (int)sk::cdiv(Y, kTY), tz = (int)sk::cdiv(Z, kTZ);
    return {(long long)X * ty * tz, ty, tz};
}
inline unsigned tile_grid(long long ntiles) { return (unsigned)(ntiles < 256 * 16 ? ntiles : 256 * 16); }

}  // namespace

extern "C" {

int sk_label_soft_skeleton2d(const int32_t* labels, int X, int Y, int Z, int iters, uint8_t* skel, void* stream) {
    SK_CHECK_ARG(labels && skel, "sk_label_soft_skeleton2d: NULL pointer");
    SK_CHECK_ARG(X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y * Z <= INT32_MAX,
                 "sk_label_soft_skeleton2d: extents %d x %d x %d (each >= 1, at most 2^31 - 1 voxels)", X, Y, Z);
    SK_CHECK_ARG(iters >= 0 && iters <= kMaxIters, "sk_label_soft_skeleton2d: iters %d not in [0, %d]", iters,
                 kMaxIters);
    hipStream_t st = (hipStream_t)stream;
    const Tiles t = tiles_of(X, Y, Z);
    label_skeleton_kernel<<<tile_grid(t.n), 256, tile_lds_bytes(1, iters + 2), st>>>(labels, Y, Z, iters, t.n, t.ty,
                                                                                     t.tz, skel);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

size_t sk_mask_metrics_workspace_bytes(int N, int M) {
    if (N < 0 || M < 0) return 0;
    return 3 * table_bytes(N, M) + (size_t)2 * (N + 1 + M + 1) * sizeof(long long);
}

int sk_mask_metrics(const int32_t* gt, const int32_t* pred, int X, int Y, int Z, const int32_t* lut_gt, int max_gt,
                    int N, const int32_t* lut_pred, int max_pred, int M, int iters, float* iou, float* dice,
                    float* cldice, void* workspace, size_t workspace_bytes, void* stream) {
    SK_CHECK_ARG(gt && pred && lut_gt && lut_pred && workspace, "sk_mask_metrics: NULL pointer");
    SK_CHECK_ARG(X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y * Z <= INT32_MAX,
                 "sk_mask_metrics: extents %d x %d x %d (each >= 1, at most 2^31 - 1 voxels: int32 table cells)", X,
                 Y, Z);
    SK_CHECK_ARG(N >= 0 && M >= 0 && max_gt >= 0 && max_pred >= 0 && (int64_t)(N + 1) * (M + 1) <= INT32_MAX,
                 "sk_mask_metrics: N = %d, M = %d, max ids %d / %d (tables of at most 2^31 - 1 cells)", N, M, max_gt,
                 max_pred);
    SK_CHECK_ARG(iters >= 0 && iters <= kMaxIters, "sk_mask_metrics: iters %d not in [0, %d]", iters, kMaxIters);
    SK_CHECK_ARG(workspace_bytes >= sk_mask_metrics_workspace_bytes(N, M), "sk_mask_metrics: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const bool skel = cldice != nullptr;
    const size_t tb = table_bytes(N, M);
    int* t_all = (int*)workspace;
    int* t_sp = (int*)((char*)workspace + tb);
    int* t_sg = (int*)((char*)workspace + 2 * tb);
    long long* row_all = (long long*)((char*)workspace + 3 * tb);
    long long* row_sg = row_all + (N + 1);
    long long* col_all = row_sg + (N + 1);
    long long* col_sp = col_all + (M + 1);
    SK_CHECK_HIP(hipMemsetAsync(workspace, 0, (skel ? 3 : 1) * tb, st));
    const Tiles t = tiles_of(X, Y, Z);
    if (skel) {
        metrics_table_kernel<true><<<tile_grid(t.n), 256, tile_lds_bytes(2, iters + 2), st>>>(
            gt, pred, Y, Z, iters, t.n, t.ty, t.tz, lut_gt, max_gt, lut_pred, max_pred, M + 1, t_all, t_sp, t_sg);
    } else {
        metrics_table_kernel<false><<<tile_grid(t.n), 256, tile_lds_bytes(2, 0), st>>>(
            gt, pred, Y, Z, iters, t.n, t.ty, t.tz, lut_gt, max_gt, lut_pred, max_pred, M + 1, t_all, nullptr,
            nullptr);
    }
    SK_CHECK_LAUNCH();
    row_sums_kernel<<<sk::cdiv(N + 1, 4), 256, 0, st>>>(t_all, skel ? t_sg : nullptr, N + 1, M + 1, row_all, row_sg);
    SK_CHECK_LAUNCH();
    col_sums_kernel<<<sk::cdiv(M + 1, 256), 256, 0, st>>>(t_all, skel ? t_sp : nullptr, N + 1, M + 1, col_all, col_sp);
    SK_CHECK_LAUNCH();
    if ((long long)N * M > 0 && (iou || dice || cldice)) {
        finalize_kernel<<<sk::stream_grid((long long)N * M, 256, 1), 256, 0, st>>>(
            t_all, t_sp, t_sg, row_all, col_all, row_sg, col_sp, N, M, iou, dice, cldice);
        SK_CHECK_LAUNCH();
    }
    return SK_OK;
}

}  // extern "C"
