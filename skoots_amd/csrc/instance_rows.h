// What the per-instance passes share: the id -> row look-up, the tile's row table in LDS, the
// staging of a window of rows, and the host-side checks and tile-grid arithmetic of their entry points.  Every pass
// reads the same mask header -- labels, X, Y, Z, lut, max_id, N -- and means the same by it: voxel value v belongs to
// row lut[v] when 0 < v <= max_id and the row lies in 1..N, and to the background otherwise.
#pragma once
#include "common.h"

#include <stdint.h>
#include <cmath>
#include <initializer_list>

namespace sk {

// ---------------------------------------------------------------------------------------------------------- device

// the row (1..N) of voxel value v, 0 for background
__device__ inline int row_of(int v, const int* __restrict__ lut, int max_id, int N) {
    int r = (v > 0 && v <= max_id) ? lut[v] : 0;
    return (r >= 1 && r <= N) ? r : 0;                     // a row outside the outputs is background
}

// Slot of `row` in a tile's table of 1 << kSlotBits keys in LDS (0 = free; open addressing), or -1 when kProbes linear
// probes found neither the row nor a free slot: the caller then adds to global memory directly.
template <int kSlotBits, int kProbes>
__device__ inline int claim_slot(int* s_key, int row) {
    constexpr int kSlots = 1 << kSlotBits;
    const unsigned h = ((unsigned)row * 2654435761u) >> (32 - kSlotBits);
    for (int p = 0; p < kProbes; ++p) {
        const int s = (int)((h + p) & (kSlots - 1));
        int k = ((volatile int*)s_key)[s];                 // a key never changes once set within a tile
        if (k == 0) k = atomicCAS(&s_key[s], 0, row);
        if (k == 0 || k == row) return s;
    }
    return -1;
}

// The extents of the volume, and where a pass's tile grid starts on every axis: 0, or -1 for the mesh passes in closed
// mode, whose first tile owns one layer outside the volume.
struct Extents {
    int X, Y, Z, lo;
};

// Stages into s_row, z fastest, the rows of a kWX x kWY x kWZ window: the tile at (ox, oy, oz) of the grid that starts
// at e.lo, with kHalo voxels in front of it.  A voxel outside the volume is staged as -1, which equals no row.
//   C      the coordinate type: int, or long long where a tile origin can pass 2^31
//   kLow   the window can start below 0 (a halo, closed mode); without it only the upper bounds are tested
//   E      Extents, or a kernel's own geometry struct with the members X, Y, Z and lo
// The form of the index arithmetic is the kernels' own: e.lo is read and kHalo subtracted inside the loop, and the
// bounds are tested in this order.  An origin summed up by the caller, or a reordered test, changes their machine code.
template <int kWX, int kWY, int kWZ, int kThreads, bool kLow, int kHalo = 0, class C, class E>
__device__ inline void stage_rows(int* s_row, const int* __restrict__ lab, const int* __restrict__ lut, int max_id, int N,
                                  const E& e, C ox, C oy, C oz, int tid) {
    for (int i = tid; i < kWX * kWY * kWZ; i += kThreads) {
        const int wz = i % kWZ, wy = i / kWZ % kWY, wx = i / (kWZ * kWY);
        const C gx = ox + e.lo + wx - kHalo, gy = oy + e.lo + wy - kHalo, gz = oz + e.lo + wz - kHalo;
        int r = -1;
        if ((!kLow || gx >= 0) && gx < e.X && (!kLow || gy >= 0) && gy < e.Y && (!kLow || gz >= 0) && gz < e.Z)
            r = row_of(lab[((long long)gx * e.Y + gy) * e.Z + gz], lut, max_id, N);
        s_row[i] = r;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
// The checks of an entry point, in the order every entry point keeps: extents, N and max_id, the size guard, its own
// arguments, the early SK_OK of an empty call (mask_empty; no pointer is looked at before it), NULL pointers, alignment.

// X Y Z < 2^log2_limit, in 128 bits: the product of three ints stays below 2^93
inline int check_voxels(const char* who, int X, int Y, int Z, int log2_limit) {
    SK_CHECK_ARG((unsigned __int128)X * Y * Z < ((unsigned __int128)1 << log2_limit),
                 "%s: extents %d x %d x %d: X Y Z must stay below 2^%d", who, X, Y, Z, log2_limit);
    return SK_OK;
}

// Extents, N and max_id, X Y Z < 2^log2_limit.  log2_limit = 0: the entry point's own guard follows -- a stronger one
// with its own message, or check_voxels behind a check that comes first.
inline int check_mask_header(const char* who, int X, int Y, int Z, int max_id, int N, int log2_limit) {
    SK_CHECK_ARG(X >= 0 && Y >= 0 && Z >= 0, "%s: extents %d x %d x %d must not be negative", who, X, Y, Z);
    SK_CHECK_ARG(N >= 0 && max_id >= 0, "%s: N = %d, max_id = %d must not be negative", who, N, max_id);
    return log2_limit ? check_voxels(who, X, Y, Z, log2_limit) : SK_OK;
}

// the distance transforms square a coordinate difference in double
inline int check_exact_squares(const char* who, int X, int Y, int Z) {
    SK_CHECK_ARG(X <= (1 << 26) && Y <= (1 << 26) && Z <= (1 << 26),
                 "%s: extents %d x %d x %d: every extent must stay at or below 2^26 (d^2 exact in double)", who, X, Y, Z);
    return SK_OK;
}

inline int check_weights(const char* who, double wx, double wy, double wz) {
    SK_CHECK_ARG(std::isfinite(wx) && std::isfinite(wy) && std::isfinite(wz) && wx > 0 && wy > 0 && wz > 0,
                 "%s: the weights %g, %g, %g (squared spacing) must be finite and positive", who, wx, wy, wz);
    return SK_OK;
}

inline bool mask_empty(int X, int Y, int Z, int N) { return (long long)X * Y * Z == 0 || N == 0; }

struct Ptr {
    const void* p;
    unsigned bytes;                                        // of one element, a power of two
    bool may_be_null = false;
};

// every pointer present, then every pointer aligned to its elements
inline int check_pointers(const char* who, std::initializer_list<Ptr> ptrs) {
    for (const Ptr& q : ptrs) SK_CHECK_ARG(q.p || q.may_be_null, "%s: NULL pointer", who);
    for (const Ptr& q : ptrs)
        SK_CHECK_ARG(((uintptr_t)q.p & (q.bytes - 1)) == 0, "%s: a pointer is not aligned to its elements", who);
    return SK_OK;
}

// Tile-based passes launch at most 256 CUs x 8 workgroups, which stride over the tiles.
inline unsigned tile_blocks(long long ntiles) { return (unsigned)(ntiles < 256 * 8 ? ntiles : 256 * 8); }

struct TileGrid {
    long long ntiles;
    int tiles_y, tiles_z;
    unsigned blocks;
};

// nx x ny x nz positions in tiles of tx x ty x tz, the last tile of an axis cut
inline TileGrid tile_grid(long long nx, long long ny, long long nz, int tx, int ty, int tz) {
    const long long tiles_x = (nx + tx - 1) / tx, tiles_y = (ny + ty - 1) / ty, tiles_z = (nz + tz - 1) / tz;
    const long long ntiles = tiles_x * tiles_y * tiles_z;
    return {ntiles, (int)tiles_y, (int)tiles_z, tile_blocks(ntiles)};
}

}  // namespace sk
