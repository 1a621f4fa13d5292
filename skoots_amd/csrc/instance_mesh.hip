// Marching-cubes cell classes of every instance of an instance mask in one pass.  The reference
// measures a surface with scikit-image's marching cubes on one binary mask per id (skoots/validate/stats.py:30-48,
// validate/compare.py: stats_per_instance).  In a binary volume the triangles of a 2 x 2 x 2 cell depend on its 8-bit
// corner configuration alone, and configurations fall into a few classes of equal area at every spacing
// (skoots_amd/validate/mc_table.py), so the surface area of an instance is a count of its cells per class.
//
// Shape of the kernel
//   * A workgroup takes a tile of kTX x kTY x kTZ CELLS.  Cell (x, y, z) has the voxels (x .. x + 1, y .. y + 1,
//     z .. z + 1) as corners; bit b of its configuration is the corner (x + (b & 1), y + ((b >> 1) & 1),
//     z + ((b >> 2) & 1)).  The tile stages the ROWS (the lut applied: 1..N, 0 for background) of its
//     (kTX + 1) x (kTY + 1) x (kTZ + 1) corner voxels into LDS; a corner outside the volume is staged as -1, which
//     equals no row.  Open mode has the cells 0 .. extent - 2 per axis; closed mode (the mask padded with one layer of
//     background) has -1 .. extent - 1, and the tile grid simply starts at cell -1, so the first tile of every axis
//     owns the extra layer.
//   * Wave w takes the plane x = w of the tile, lanes = consecutive z, and walks y: the four corner rows at y + 1 of
//     one cell are the four at y of the next, so a cell costs four LDS reads.  A cell whose corners are all equal
//     (inside an instance, background, outside) or all non-positive ends there: no atomic.
//   * For every distinct positive row among the corners the configuration is the mask of corners that equal it; its
//     class comes from the 256-byte table in LDS, and the cell adds one to (row, class) in a table in LDS keyed by
//     row (kSlots slots of 32 32-bit counters, open addressing, at most kProbes probes).  The table is flushed once
//     per tile with 64-bit global atomics; a row that finds no slot adds to global memory directly.
//   * Integer atomics only: every result is exact and independent of the order of arrival.
#include "instance_rows.h"

namespace {

constexpr int kTX = 4, kTY = 16, kTZ = 64;            // tile of cells; kTZ is the wave width: one lane per z
constexpr int kWX = kTX + 1, kWY = kTY + 1, kWZ = kTZ + 1;
constexpr int kStaged = kWX * kWY * kWZ;              // 5525 ints = 21.6 KiB
constexpr int kSlotBits = 5, kSlots = 1 << kSlotBits;  // rows the LDS table holds per tile
constexpr int kProbes = 8;                            // linear probes before a cell goes to global memory
constexpr int kClasses = 32;                          // counters per slot: the widest row the entry point accepts
constexpr int kThreads = 256;

static_assert(kTZ == 64, "one lane per z of the tile");
static_assert(kTX == kThreads / 64, "one wave per x plane of the tile");

typedef unsigned long long u64;

// lo: the first cell of every axis (0 open, -1 closed); ncx, ncy, ncz: cells per axis, all positive
__global__ void __launch_bounds__(kThreads) instance_mesh_kernel(const int* __restrict__ lab, int X, int Y, int Z,
                                                                 const int* __restrict__ lut, int max_id, int N,
                                                                 const unsigned char* __restrict__ class_of,
                                                                 int n_classes, int lo, long long ncx, long long ncy,
                                                                 long long ncz, long long ntiles, int tiles_y,
                                                                 int tiles_z, u64* __restrict__ cells) {
    __shared__ int s_row[kStaged];
    __shared__ unsigned s_cnt[kSlots * kClasses];
    __shared__ int s_key[kSlots];
    __shared__ unsigned char s_class[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_class[tid] = class_of[tid];                          // kThreads == 256; the barriers below publish it
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long cx = (t / ((long long)tiles_z * tiles_y)) * kTX, cy = (t / tiles_z % tiles_y) * (long long)kTY;
        const long long cz = (t % tiles_z) * (long long)kTZ;           // the tile's first cell, counted from lo
        __syncthreads();                                   // the previous tile's flush has read the table
        sk::stage_rows<kWX, kWY, kWZ, kThreads, true>(s_row, lab, lut, max_id, N, sk::Extents{X, Y, Z, lo}, cx, cy, cz, tid);
        for (int i = tid; i < kSlots * kClasses; i += kThreads) s_cnt[i] = 0;
        if (tid < kSlots) s_key[tid] = 0;
        __syncthreads();

        // cells of this tile that exist: the last tile of an axis may be cut
        const int vx = (int)(ncx - cx < kTX ? ncx - cx : kTX), vy = (int)(ncy - cy < kTY ? ncy - cy : kTY);
        const int vz = (int)(ncz - cz < kTZ ? ncz - cz : kTZ);
        if (wave < vx && lane < vz) {
            const int base = wave * kWY * kWZ + lane;
            int r[8];                                      // r[b]: corner b of the cell, as the configuration's bits
            r[0] = s_row[base];
            r[1] = s_row[base + kWY * kWZ];
            r[4] = s_row[base + 1];
            r[5] = s_row[base + kWY * kWZ + 1];
            for (int iy = 0; iy < vy; ++iy) {
                const int c = base + (iy + 1) * kWZ;
                r[2] = s_row[c];
                r[3] = s_row[c + kWY * kWZ];
                r[6] = s_row[c + 1];
                r[7] = s_row[c + kWY * kWZ + 1];
                int top = r[0];
                bool same = true;
#pragma unroll
                for (int b = 1; b < 8; ++b) {
                    same &= r[b] == r[0];
                    top = r[b] > top ? r[b] : top;
                }
                // same: inside an instance, empty or outside; top <= 0: background and outside only
                if (!same && top > 0) {
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const int a = r[b];
                        if (a <= 0) continue;
                        unsigned cfg = 0;
#pragma unroll
                        for (int j = 0; j < 8; ++j) cfg |= (unsigned)(r[j] == a) << j;
                        if ((cfg & (0u - cfg)) != (1u << b)) continue;   // an earlier corner has counted this row
                        const unsigned cls = s_class[cfg];               // cfg != 255: the corners are not all equal
                        if (cls >= (unsigned)n_classes) continue;        // a wrong table cannot leave the row
                        const int s = sk::claim_slot<kSlotBits, kProbes>(s_key, a);
                        if (s >= 0)
                            atomicAdd(&s_cnt[s * kClasses + cls], 1u);
                        else                               // the table is full for this row: global memory directly
                            atomicAdd(&cells[(long long)(a - 1) * n_classes + cls], 1ull);
                    }
                }
                r[0] = r[2];
                r[1] = r[3];
                r[4] = r[6];
                r[5] = r[7];
            }
        }
        __syncthreads();
        for (int i = tid; i < kSlots * kClasses; i += kThreads) {   // flush: one global atomic per used counter
            const int s = i / kClasses, k = i % kClasses, key = s_key[s];
            const unsigned v = s_cnt[i];
            if (key != 0 && v != 0 && k < n_classes) atomicAdd(&cells[(long long)(key - 1) * n_classes + k], (u64)v);
        }
    }
}

}  // namespace

extern "C" {

int sk_instance_mesh_cells(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                           const uint8_t* class_of, int n_classes, int closed, int64_t* cells, void* stream) {
    const char* who = "sk_instance_mesh_cells";
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 62);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(n_classes >= 1 && n_classes <= kClasses, "sk_instance_mesh_cells: n_classes = %d must be in 1..%d",
                 n_classes, kClasses);
    SK_CHECK_ARG(closed == 0 || closed == 1, "sk_instance_mesh_cells: closed = %d must be 0 or 1", closed);
    if (sk::mask_empty(X, Y, Z, N)) return SK_OK;
    rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}, {class_of, 1}, {cells, 8}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(cells, 0, (size_t)N * n_classes * sizeof(int64_t), st));
    const int lo = closed ? -1 : 0;
    const long long ncx = (long long)X + (closed ? 1 : -1), ncy = (long long)Y + (closed ? 1 : -1);
    const long long ncz = (long long)Z + (closed ? 1 : -1);
    if (ncx <= 0 || ncy <= 0 || ncz <= 0) return SK_OK;    // open mode, an extent of 1: no cell, the zeros stand
    const sk::TileGrid tg = sk::tile_grid(ncx, ncy, ncz, kTX, kTY, kTZ);   // at most 2^62 / 4096 tiles + lower-order terms
    instance_mesh_kernel<<<tg.blocks, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, class_of, n_classes, lo, ncx,
                                                         ncy, ncz, tg.ntiles, tg.tiles_y, tg.tiles_z, (u64*)cells);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
