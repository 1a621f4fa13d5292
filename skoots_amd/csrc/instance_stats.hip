// Per-instance measurements of an instance mask in one pass: voxel count, first and second
// moments of the voxel indices, exposed faces per axis and the bounding box of every instance at once.  The reference
// only sketches this step (skoots/validate/compare.py: stats_per_instance forms one full-volume mask per id, and
// validate/lib.py: mask_to_bbox takes one Python iteration per instance).
//
// Shape of the kernel
//   * A workgroup takes a tile of kTX x kTY x kTZ voxels.  It stages the tile's ROWS (the lut applied: 1..N, 0 for
//     background) with a one-voxel halo into LDS; a halo voxel outside the volume is staged as -1, which equals no row,
//     so "the neighbour lies outside" and "the neighbour has another row" are one comparison.  Staging rows and not raw
//     ids makes each voxel pay one lut look-up instead of seven.
//   * A wave takes one z row of the tile at a time, lanes = consecutive z.  A maximal run of one row along the lanes is
//     accumulated by its first lane alone, in closed form: L, x L, y L, sum z, sum z^2, ... (run_sums below).  The faces
//     of a run come from one packed inclusive scan over the wave, so the first lane also adds the run's faces; no lane
//     adds anything per voxel, and a wave row without any instance voxel skips all of it (background takes no atomic).
//   * The first lane of a run adds its 19 values to a small table in LDS keyed by row (kSlots slots, open addressing,
//     at most kProbes probes), with LDS integer atomics.  The table is flushed once per tile with 64-bit global
//     atomic add and 32-bit atomic min / max.  A run whose row finds no slot adds to global memory directly.
//   * Integer atomics only: every result is exact and independent of the order of arrival.
#include "instance_rows.h"

#include <limits.h>

namespace {

constexpr int kTX = 4, kTY = 16, kTZ = 64;            // tile; kTZ is the wave width: one lane per z
constexpr int kWX = kTX + 2, kWY = kTY + 2, kWZ = kTZ + 2;
constexpr int kStaged = kWX * kWY * kWZ;              // 7128 ints = 27.8 KiB
constexpr int kSlotBits = 5, kSlots = 1 << kSlotBits;  // rows the LDS table holds per tile
constexpr int kProbes = 8;                            // linear probes before a run goes to global memory
constexpr int kSums = 13, kBox = 6, kAcc = kSums + kBox;
constexpr int kThreads = 256;

static_assert(kTZ == 64, "one lane per z of the tile");

typedef unsigned long long u64;

struct RunSums {
    u64 v[kSums];
};

// Closed forms of one run [z0, z0 + L) at (x, y).  Every term is bounded by the run's own share of the final sum, so
// nothing here overflows while the totals fit (the entry point's guard).
__device__ inline RunSums run_sums(int x, int y, int z0, int L, unsigned faces) {
    const u64 ux = (u64)x, uy = (u64)y, uz = (u64)z0, n = (u64)L;
    const u64 tri = n * (n - 1) / 2;                       // sum of 0 .. L-1
    const u64 pyr = (n - 1) * n * (2 * n - 1) / 6;         // sum of squares of 0 .. L-1
    const u64 sz = n * uz + tri;
    const u64 szz = n * uz * uz + 2 * uz * tri + pyr;
    RunSums r;
    r.v[0] = n;
    r.v[1] = ux * n;
    r.v[2] = uy * n;
    r.v[3] = sz;
    r.v[4] = ux * ux * n;
    r.v[5] = uy * uy * n;
    r.v[6] = szz;
    r.v[7] = ux * uy * n;
    r.v[8] = ux * sz;
    r.v[9] = uy * sz;
    r.v[10] = faces & 1023u;
    r.v[11] = (faces >> 10) & 1023u;
    r.v[12] = faces >> 20;
    return r;
}

__global__ void __launch_bounds__(kThreads) instance_stats_kernel(const int* __restrict__ lab, int X, int Y, int Z,
                                                                  const int* __restrict__ lut, int max_id, int N,
                                                                  long long ntiles, int tiles_y, int tiles_z,
                                                                  u64* __restrict__ sums, int* __restrict__ boxes) {
    __shared__ int s_row[kStaged];
    __shared__ u64 s_sum[kSlots * kSums];
    __shared__ int s_box[kSlots * kBox];
    __shared__ int s_key[kSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int z0 = (int)(t % tiles_z) * kTZ, y0 = (int)(t / tiles_z % tiles_y) * kTY;
        const int x0 = (int)(t / ((long long)tiles_z * tiles_y)) * kTX;
        __syncthreads();                                   // the previous tile's flush has read the table
        sk::stage_rows<kWX, kWY, kWZ, kThreads, true, 1>(s_row, lab, lut, max_id, N, sk::Extents{X, Y, Z, 0}, x0, y0, z0, tid);
        for (int i = tid; i < kSlots * kSums; i += kThreads) s_sum[i] = 0;
        for (int i = tid; i < kSlots * kBox; i += kThreads) s_box[i] = (i % kBox) < 3 ? INT_MAX : -1;
        if (tid < kSlots) s_key[tid] = 0;
        __syncthreads();

        for (int r = wave; r < kTX * kTY; r += kThreads / 64) {   // wave-uniform: every lane reaches the shuffles
            const int ix = r / kTY, iy = r % kTY;
            const int c = ((ix + 1) * kWY + (iy + 1)) * kWZ + lane + 1;
            const int a = s_row[c];                        // -1 where the tile leaves the volume
            const bool valid = a > 0;
            if (__ballot(valid) == 0) continue;            // wave-uniform
            unsigned f = 0;
            if (valid) {
                f = (unsigned)((s_row[c - kWY * kWZ] != a) + (s_row[c + kWY * kWZ] != a)) |
                    (unsigned)((s_row[c - kWZ] != a) + (s_row[c + kWZ] != a)) << 10 |
                    (unsigned)((s_row[c - 1] != a) + (s_row[c + 1] != a)) << 20;
            }
            unsigned scan = f;                             // inclusive scan: three 10-bit fields, each at most 128
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(scan, d);
                if (lane >= d) scan += up;
            }
            const int prev = __shfl_up(a, 1);
            const bool cont = valid && lane > 0 && prev == a;
            const u64 cmask = __ballot(cont);
            const u64 rest = lane == 63 ? 0ull : cmask >> (lane + 1);
            const int L = 1 + __builtin_ctzll(~rest);      // lanes of the run that starts here (if one does)
            const unsigned scan_end = __shfl(scan, (lane + L - 1) & 63);
            if (!valid || cont) continue;
            const int x = x0 + ix, y = y0 + iy, z = z0 + lane;
            const RunSums rs = run_sums(x, y, z, L, scan_end - scan + f);
            const int s = sk::claim_slot<kSlotBits, kProbes>(s_key, a);
            if (s >= 0) {
#pragma unroll
                for (int k = 0; k < kSums; ++k) atomicAdd(&s_sum[s * kSums + k], rs.v[k]);
                atomicMin(&s_box[s * kBox + 0], x);
                atomicMin(&s_box[s * kBox + 1], y);
                atomicMin(&s_box[s * kBox + 2], z);
                atomicMax(&s_box[s * kBox + 3], x);
                atomicMax(&s_box[s * kBox + 4], y);
                atomicMax(&s_box[s * kBox + 5], z + L - 1);
            } else {                                       // the table is full for this row: global memory directly
                u64* gs = sums + (long long)(a - 1) * kSums;
                int* gb = boxes + (long long)(a - 1) * kBox;
#pragma unroll
                for (int k = 0; k < kSums; ++k)
                    if (rs.v[k]) atomicAdd(&gs[k], rs.v[k]);
                atomicMin(&gb[0], x);
                atomicMin(&gb[1], y);
                atomicMin(&gb[2], z);
                atomicMax(&gb[3], x);
                atomicMax(&gb[4], y);
                atomicMax(&gb[5], z + L - 1);
            }
        }
        __syncthreads();
        for (int i = tid; i < kSlots * kAcc; i += kThreads) {   // flush: one global atomic per used accumulator
            const int s = i / kAcc, k = i % kAcc, key = s_key[s];
            if (key == 0) continue;
            if (k < kSums) {
                const u64 v = s_sum[s * kSums + k];
                if (v) atomicAdd(&sums[(long long)(key - 1) * kSums + k], v);
            } else if (k < kSums + 3) {
                atomicMin(&boxes[(long long)(key - 1) * kBox + (k - kSums)], s_box[s * kBox + (k - kSums)]);
            } else {
                atomicMax(&boxes[(long long)(key - 1) * kBox + (k - kSums)], s_box[s * kBox + (k - kSums)]);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) instance_stats_init_kernel(int* __restrict__ boxes, long long n) {
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        boxes[i] = (i % kBox) < 3 ? INT_MAX : -1;
}

}  // namespace

extern "C" {

int sk_instance_stats_row_values(int which) { return which == 0 ? kSums : which == 1 ? kBox : 0; }

int sk_instance_stats(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int64_t* sums,
                      int32_t* boxes, void* stream) {
    const char* who = "sk_instance_stats";
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 0);    // the guard below covers X Y Z itself
    if (rc != SK_OK) return rc;
    const int m = X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z);
    const unsigned __int128 voxels = (unsigned __int128)X * Y * Z, lim = (unsigned __int128)1 << 63;   // below 2^93
    SK_CHECK_ARG(voxels < lim && voxels * ((unsigned __int128)m * m) < lim,                               // below 2^125
                 "sk_instance_stats: extents %d x %d x %d: X Y Z max(X, Y, Z)^2 must stay below 2^63 (int64 second "
                 "moments)", X, Y, Z);
    if (sk::mask_empty(X, Y, Z, N)) return SK_OK;
    rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}, {sums, 8}, {boxes, 4}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)N * kSums * sizeof(int64_t), st));
    instance_stats_init_kernel<<<sk::stream_grid((long long)N * kBox, kThreads), kThreads, 0, st>>>(
        boxes, (long long)N * kBox);
    SK_CHECK_LAUNCH();
    const sk::TileGrid tg = sk::tile_grid(X, Y, Z, kTX, kTY, kTZ);
    instance_stats_kernel<<<tg.blocks, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, tg.ntiles, tg.tiles_y,
                                                          tg.tiles_z, (u64*)sums, boxes);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
