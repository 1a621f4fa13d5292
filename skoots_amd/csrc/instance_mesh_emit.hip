// The marching-cubes mesh of every instance of an instance mask in one pass.  Section 21
// (instance_mesh.hip) counts every instance's cells per triangle class and never builds the surface; here the triangles
// themselves are written.  The definitions are section 21's: rows 1..N through lut, a corner outside the volume equals
// no row, open mode has the cells 0 .. extent - 2 and closed mode -1 .. extent - 1, and a cell shared by k instances
// belongs to each of them.  In a binary volume the triangles of a cell depend on its 8-bit configuration alone
// (skoots_amd/validate/mc_triangles.py), and every vertex is the midpoint of a cell edge whose two end voxels have
// exactly one of the row.
//
// Names
//   * voxel key: the linear index of a voxel in the volume padded by one layer, ((x + 1) (Y + 2) + y + 1) (Z + 2) + z + 1.
//   * edge key: the voxel key of the edge's low voxel x 3 + axis.  A vertex IS its edge key (per row).
//   * order key: the voxel key of the cell's low corner x 8 + the triangle's position in TRIANGLES[configuration].
//   * tri_table: 256 x uint64; bits 4 i .. 4 i + 3 hold edge number i % 3 of triangle i / 3, bits 60 .. 63 the number of
//     triangles.  Edge e = 4 axis + k starts at the k-th corner (ascending) whose bit `axis` is clear.
//
// Shape of the kernels
//   * A workgroup takes a tile of kTX x kTY x kTZ POSITIONS and stages the rows of its (kTX + 1) (kTY + 1) (kTZ + 1)
//     corner voxels into LDS exactly as section 21 does.  A position is a corner voxel of the cell range: there is one
//     more per axis than cells.  A position whose three coordinates are below the cell counts is a cell and gives
//     triangles; every position owns the three edges that start at it, and an edge along axis d exists when the
//     position's coordinate d is below the cell count of d.  So every edge is counted once, the edges on the high
//     faces of the cell range included (their positions are no cells), and in closed mode the -1 layer is simply the
//     first position of every axis.
//   * Wave w takes the plane x = w of the tile, lanes = consecutive z, and walks y as section 21 does.
//   * sk_instance_mesh_count adds (vertices, triangles) per row into a table in LDS keyed by row and flushes it once
//     per tile with 64-bit global atomics; a row that finds no slot adds to global memory directly.
//   * sk_instance_mesh_emit walks a tile twice.  The first walk counts the thread's records and takes the thread's
//     share of the tile with one LDS atomic per kind; one thread then takes the tile's share of the output with ONE
//     global atomic per kind; the second walk writes the records.  A record beyond the capacity is not written; the
//     counters still advance, so the caller learns what was needed.
//   * Integer atomics only.  Which slot a record lands in depends on the order of arrival; the set of records does
//     not, and the host sorts them (skoots_amd/validate/lib.py: instance_meshes).
#include "instance_rows.h"

namespace {

constexpr int kTX = 4, kTY = 16, kTZ = 64;            // tile of positions; kTZ is the wave width: one lane per z
constexpr int kWX = kTX + 1, kWY = kTY + 1, kWZ = kTZ + 1;
constexpr int kStaged = kWX * kWY * kWZ;              // 5525 ints = 21.6 KiB
constexpr int kSlotBits = 6, kSlots = 1 << kSlotBits;  // rows the LDS table of the count kernel holds per tile
constexpr int kProbes = 8;                            // linear probes before a count goes to global memory
constexpr int kThreads = 256;
constexpr int kVertexWords = 2, kTriangleWords = 5;   // int64 per record

static_assert(kTZ == 64, "one lane per z of the tile");
static_assert(kTX == kThreads / 64, "one wave per x plane of the tile");

typedef unsigned long long u64;

struct Geometry {
    int X, Y, Z, lo;                                  // lo: the first position of every axis (0 open, -1 closed)
    long long ncx, ncy, ncz;                          // cells per axis, all positive; positions: one more
    long long ntiles;
    int tiles_y, tiles_z;
};

// The records of this thread's column of positions (plane x = wave, z = lane, every y of the tile).
//   on_vertex(row, iy, axis): the edge that starts at position iy along `axis` is a vertex of `row`
//   on_triangles(row, iy, entry): the cell at iy has, for `row`, the triangles of the tri_table entry
template <class V, class T>
__device__ inline void walk_column(const int* s_row, const u64* s_tab, const Geometry& g, long long cx, long long cy,
                                   long long cz, int wave, int lane, V&& on_vertex, T&& on_triangles) {
    // positions of this tile that exist, and those among them that are cells / that start an edge along the axis
    const long long px = g.ncx + 1 - cx, py = g.ncy + 1 - cy, pz = g.ncz + 1 - cz;
    if (wave >= px || lane >= pz) return;
    const int vy = (int)(py < kTY ? py : kTY);
    const bool in_x = wave < px - 1, in_z = lane < pz - 1;
    const int base = wave * kWY * kWZ + lane;
    int r[8];                                              // r[b]: corner b of the cell, as the configuration's bits
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
        const bool in_y = iy < py - 1;
        const int a0 = r[0];
        // the three edges that start here: a vertex of each end's row when the rows differ
        if (in_x && r[1] != a0) {
            if (a0 > 0) on_vertex(a0, iy, 0);
            if (r[1] > 0) on_vertex(r[1], iy, 0);
        }
        if (in_y && r[2] != a0) {
            if (a0 > 0) on_vertex(a0, iy, 1);
            if (r[2] > 0) on_vertex(r[2], iy, 1);
        }
        if (in_z && r[4] != a0) {
            if (a0 > 0) on_vertex(a0, iy, 2);
            if (r[4] > 0) on_vertex(r[4], iy, 2);
        }
        if (in_x && in_y && in_z) {
            int top = a0;
            bool same = true;
#pragma unroll
            for (int b = 1; b < 8; ++b) {
                same &= r[b] == a0;
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
                    if ((cfg & (0u - cfg)) != (1u << b)) continue;   // an earlier corner has handled this row
                    on_triangles(a, iy, s_tab[cfg]);                 // cfg != 255: the corners are not all equal
                }
            }
        }
        r[0] = r[2];
        r[1] = r[3];
        r[4] = r[6];
        r[5] = r[7];
    }
}

// triangles of a table entry: never more than five, whatever the table says
__device__ inline int triangles_of(u64 entry) {
    const int n = (int)(entry >> 60);
    return n < 5 ? n : 5;
}

// first position of tile t, counted from lo
__device__ inline void tile_origin(const Geometry& g, long long t, long long& cx, long long& cy, long long& cz) {
    cx = (t / ((long long)g.tiles_z * g.tiles_y)) * kTX;
    cy = (t / g.tiles_z % g.tiles_y) * (long long)kTY;
    cz = (t % g.tiles_z) * (long long)kTZ;
}

__global__ void __launch_bounds__(kThreads) instance_mesh_count_kernel(const int* __restrict__ lab,
                                                                       const int* __restrict__ lut, int max_id, int N,
                                                                       const u64* __restrict__ tri_table, Geometry g,
                                                                       u64* __restrict__ counts) {
    __shared__ int s_row[kStaged];
    __shared__ u64 s_tab[256];
    __shared__ unsigned s_cnt[kSlots * 2];
    __shared__ int s_key[kSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_tab[tid] = tri_table[tid];                           // kThreads == 256; the barriers below publish it
    for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
        long long cx, cy, cz;
        tile_origin(g, t, cx, cy, cz);
        __syncthreads();                                   // the previous tile's flush has read the table
        sk::stage_rows<kWX, kWY, kWZ, kThreads, true>(s_row, lab, lut, max_id, N, g, cx, cy, cz, tid);
        if (tid < kSlots * 2) s_cnt[tid] = 0;
        if (tid < kSlots) s_key[tid] = 0;
        __syncthreads();
        auto add = [&](int row, int which, unsigned n) {
            const int s = sk::claim_slot<kSlotBits, kProbes>(s_key, row);
            if (s >= 0)
                atomicAdd(&s_cnt[s * 2 + which], n);
            else                                           // the table is full for this row: global memory directly
                atomicAdd(&counts[(long long)(row - 1) * 2 + which], (u64)n);
        };
        walk_column(s_row, s_tab, g, cx, cy, cz, wave, lane, [&](int row, int, int) { add(row, 0, 1u); },
                    [&](int row, int, u64 entry) {
                        const int n = triangles_of(entry);
                        if (n) add(row, 1, (unsigned)n);
                    });
        __syncthreads();
        if (tid < kSlots * 2) {                            // flush: one global atomic per used counter
            const int key = s_key[tid >> 1];
            const unsigned v = s_cnt[tid];
            if (key != 0 && v != 0) atomicAdd(&counts[(long long)(key - 1) * 2 + (tid & 1)], (u64)v);
        }
    }
}

static_assert(kSlots * 2 <= kThreads, "one thread per counter of the table");

__global__ void __launch_bounds__(kThreads) instance_mesh_emit_kernel(const int* __restrict__ lab,
                                                                      const int* __restrict__ lut, int max_id, int N,
                                                                      const u64* __restrict__ tri_table, Geometry g,
                                                                      long long* __restrict__ vertices,
                                                                      long long vertex_capacity,
                                                                      long long* __restrict__ triangles,
                                                                      long long triangle_capacity,
                                                                      u64* __restrict__ produced) {
    __shared__ int s_row[kStaged];
    __shared__ u64 s_tab[256];
    __shared__ unsigned s_total[2];
    __shared__ u64 s_first[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_tab[tid] = tri_table[tid];
    const long long sz = (long long)g.Z + 2, sy = ((long long)g.Y + 2) * sz;   // voxel key strides of y and x
    for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
        long long cx, cy, cz;
        tile_origin(g, t, cx, cy, cz);
        __syncthreads();                                   // the previous tile has read s_row, s_total and s_first
        sk::stage_rows<kWX, kWY, kWZ, kThreads, true>(s_row, lab, lut, max_id, N, g, cx, cy, cz, tid);
        if (tid < 2) s_total[tid] = 0;
        __syncthreads();

        unsigned nv = 0, nt = 0;                           // first walk: how many records this thread has
        walk_column(s_row, s_tab, g, cx, cy, cz, wave, lane, [&](int, int, int) { ++nv; },
                    [&](int, int, u64 entry) { nt += (unsigned)triangles_of(entry); });
        const unsigned my_v = nv ? atomicAdd(&s_total[0], nv) : 0u;
        const unsigned my_t = nt ? atomicAdd(&s_total[1], nt) : 0u;
        __syncthreads();
        if (tid < 2) {                                     // the tile's share of the output: one global atomic per kind
            const unsigned n = s_total[tid];
            s_first[tid] = n ? atomicAdd(&produced[tid], (u64)n) : 0ull;
        }
        __syncthreads();

        // voxel key of this thread's position at iy = 0: the volume padded by one layer, so -1 becomes 0
        const long long key0 = (cx + g.lo + wave + 1) * sy + (cy + g.lo + 1) * sz + (cz + g.lo + lane + 1);
        long long at_v = (long long)(s_first[0] + my_v), at_t = (long long)(s_first[1] + my_t);
        walk_column(
            s_row, s_tab, g, cx, cy, cz, wave, lane,
            [&](int row, int iy, int axis) {
                if (at_v < vertex_capacity) {
                    vertices[at_v * kVertexWords] = row;
                    vertices[at_v * kVertexWords + 1] = (key0 + iy * sz) * 3 + axis;
                }
                ++at_v;
            },
            [&](int row, int iy, u64 entry) {
                const int n = triangles_of(entry);
                const long long cell = key0 + iy * sz;
                for (int j = 0; j < n; ++j) {
                    if (at_t < triangle_capacity) {
                        long long* rec = triangles + at_t * kTriangleWords;
                        rec[0] = row;
                        for (int i = 0; i < 3; ++i) {
                            const int e = (int)(entry >> (4 * (3 * j + i))) & 15;
                            const int axis = (e >> 2) < 2 ? (e >> 2) : 2, k = e & 3;   // 12 .. 15: no edge; stays a number
                            // the k-th corner whose bit `axis` is clear, as an offset of voxel keys
                            const long long off = axis == 0   ? (k & 1) * sz + (k >> 1)
                                                  : axis == 1 ? (k & 1) * sy + (k >> 1)
                                                              : (k & 1) * sy + (k >> 1) * sz;
                            rec[1 + i] = (cell + off) * 3 + axis;
                        }
                        rec[4] = cell * 8 + j;
                    }
                    ++at_t;
                }
            });
    }
}

// the checks both entry points share; *run = false when there is nothing to launch
int prepare(const char* who, const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
            const uint64_t* tri_table, int closed, Geometry* g, bool* run) {
    *run = false;
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 62);
    if (rc != SK_OK) return rc;
    const unsigned __int128 padded = (unsigned __int128)((long long)X + 2) * ((long long)Y + 2) * ((long long)Z + 2);
    SK_CHECK_ARG(padded < ((unsigned __int128)1 << 60),
                 "%s: extents %d x %d x %d: (X + 2) (Y + 2) (Z + 2) must stay below 2^60, or the keys leave int64", who, X,
                 Y, Z);
    SK_CHECK_ARG(closed == 0 || closed == 1, "%s: closed = %d must be 0 or 1", who, closed);
    if (sk::mask_empty(X, Y, Z, N)) return SK_OK;
    rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}, {tri_table, 8}});
    if (rc != SK_OK) return rc;
    g->X = X, g->Y = Y, g->Z = Z, g->lo = closed ? -1 : 0;
    g->ncx = (long long)X + (closed ? 1 : -1), g->ncy = (long long)Y + (closed ? 1 : -1);
    g->ncz = (long long)Z + (closed ? 1 : -1);
    if (g->ncx <= 0 || g->ncy <= 0 || g->ncz <= 0) return SK_OK;   // open mode, an extent of 1: no cell, no mesh
    // tiles of POSITIONS: one more per axis than cells
    const sk::TileGrid tg = sk::tile_grid(g->ncx + 1, g->ncy + 1, g->ncz + 1, kTX, kTY, kTZ);
    g->ntiles = tg.ntiles, g->tiles_y = tg.tiles_y, g->tiles_z = tg.tiles_z;
    *run = true;
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_instance_mesh_count(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                           const uint64_t* tri_table, int closed, int64_t* counts, void* stream) {
    Geometry g;
    bool run;
    int rc = prepare("sk_instance_mesh_count", labels, X, Y, Z, lut, max_id, N, tri_table, closed, &g, &run);
    if (rc != SK_OK) return rc;
    if (sk::mask_empty(X, Y, Z, N)) return SK_OK;
    rc = sk::check_pointers("sk_instance_mesh_count", {{counts, 8}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)N * 2 * sizeof(int64_t), st));
    if (!run) return SK_OK;
    instance_mesh_count_kernel<<<sk::tile_blocks(g.ntiles), kThreads, 0, st>>>(labels, lut, max_id, N,
                                                                               (const u64*)tri_table, g, (u64*)counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_instance_mesh_emit(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                          const uint64_t* tri_table, int closed, int64_t* vertices, int64_t vertex_capacity,
                          int64_t* triangles, int64_t triangle_capacity, int64_t* produced, void* stream) {
    Geometry g;
    bool run;
    int rc = prepare("sk_instance_mesh_emit", labels, X, Y, Z, lut, max_id, N, tri_table, closed, &g, &run);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(vertex_capacity >= 0 && triangle_capacity >= 0,
                 "sk_instance_mesh_emit: capacities %lld, %lld must not be negative", (long long)vertex_capacity,
                 (long long)triangle_capacity);
    SK_CHECK_ARG(vertex_capacity < ((int64_t)1 << 58) && triangle_capacity < ((int64_t)1 << 58),
                 "sk_instance_mesh_emit: capacities %lld, %lld must stay below 2^58", (long long)vertex_capacity,
                 (long long)triangle_capacity);
    if (sk::mask_empty(X, Y, Z, N)) return SK_OK;
    rc = sk::check_pointers("sk_instance_mesh_emit", {{produced, 8}, {vertices, 8, vertex_capacity == 0},
                                                      {triangles, 8, triangle_capacity == 0}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(produced, 0, 2 * sizeof(int64_t), st));
    if (!run) return SK_OK;
    instance_mesh_emit_kernel<<<sk::tile_blocks(g.ntiles), kThreads, 0, st>>>(
        labels, lut, max_id, N, (const u64*)tri_table, g, (long long*)vertices, (long long)vertex_capacity,
        (long long*)triangles, (long long)triangle_capacity, (u64*)produced);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
