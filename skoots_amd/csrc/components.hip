// Connected pieces of every value of a label volume at once, and the table a clean-up decides on.
// No reference counterpart: the reference never checks that an instance id marks one body.
//
// sk_label_components labels an (X, Y, Z) int32 volume, Z fastest, in one launch sequence.  Two voxels are joined when
// they are neighbours and hold the same value: the positive values at connectivity 6 / 18 / 26 (the 3 / 9 / 13 backward
// neighbours of a voxel), or the zero voxels at connectivity 6.  sk_label_planes taken to three dimensions:
//   1. tiles     a workgroup labels a 4 x 8 x 64 tile in LDS: every z row is cut into runs with one ballot, the runs are
//                united by minimum index (atomicMin on LDS), and every voxel's parent is written as the global index of
//                its tile-local root;
//   2. borders   one thread per voxel on a face of its tile unites it with its backward neighbours in OTHER tiles: across
//                faces, and at 18 / 26 across tile edges and corners (lock-free atomicMin union in global memory);
//   3. flatten   every voxel of the kind points at its root; roots are counted per 2048-voxel chunk of the volume;
//   4. scan      one workgroup: exclusive prefix of the chunk counts and the total;
//   5. rank      a root gets 1 + its rank in raster order;  6. write  every other voxel copies its root's number.
// A union that other unions already imply is left out: a face pair whose twin one step down z (down y for the z
// direction) lies in the same two tiles and holds the same value, and a diagonal pair with a voxel of the same value on
// one of the axis-wise paths between its ends (those shorter steps are pairs of their own).  Leaving a union out is
// always optional, so the rules need no halo: what a tile cannot see counts as "not implied".
// A root is the minimum index of its piece, i.e. its first voxel in raster order over the whole volume, so the rank IS
// scipy.ndimage.label's number for a one-value mask.  No workgroup waits for another: every loop follows parents towards
// a strictly smaller index or retries an atomicMin that lowered one.
//
// sk_component_table fills one int64 row per piece in one pass with integer atomics only (add, min, max, or), so the
// rows do not depend on the order of execution.  Lanes run along z: a run of one piece inside a wave is reduced in
// registers first and its first lane issues the atomics, one set per run -- inside a large body one per 64 voxels.
#include "common.h"

namespace {

constexpr int kTX = 4, kTY = 8, kTZ = 64;      // tile: a wave per z row, lanes along z
constexpr int kTile = kTX * kTY * kTZ;         // 2048 voxels, 8 per thread
constexpr int kChunk = 2048;                   // voxels per block in the count / rank passes
constexpr int kCols = 6;                       // int64 values per row of the table
constexpr long long kNone = 0x7fffffffffffffffLL;

// the 13 backward neighbours: faces (connectivity 6), then edges (18), then corners (26)
__constant__ signed char kDir[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},  {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1},
                                        {0, -1, -1}, {0, -1, 1},  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

struct Geo {
    int X, Y, Z, n;
    int ntx, nty, ntz, nchunks;
    int ndir, which;
};

// what joins: the value itself for the kind that is labelled, -1 for the other kind
__device__ __forceinline__ int key_of(int v, int which) { return which ? (v > 0 ? v : -1) : (v == 0 ? 0 : -1); }

__device__ __forceinline__ int load_parent(const int* parent, int i) { return __atomic_load_n(parent + i, __ATOMIC_RELAXED); }

__device__ __forceinline__ int find_root(const int* parent, int i) {
    int p = load_parent(parent, i);
    while (p != i) {   // p < i: parents only point down
        i = p;
        p = load_parent(parent, i);
    }
    return i;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
    while (true) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&parent[a], b);   // a > b: hang a under b
        if (old == a) return;
        a = old;                                    // a had a parent already (old < a): unite that one with b
    }
}

// true when a voxel of key k on one of the axis-wise paths from (x, y, z) to its diagonal neighbour (+dx, +dy, +dz)
// already joins the two: the steps of that path are pairs with fewer non-zero components, united on their own
template <class K>
__device__ __forceinline__ bool diagonal_implied(const K& key, int x, int y, int z, int dx, int dy, int dz, int k) {
    for (int m = 1; m < 7; ++m) {
        const int ax = (m & 1) ? dx : 0, ay = (m & 2) ? dy : 0, az = (m & 4) ? dz : 0;
        if (((m & 1) && !dx) || ((m & 2) && !dy) || ((m & 4) && !dz)) continue;   // not a subset of the step
        if (ax == dx && ay == dy && az == dz) continue;                          // the step itself
        if (key(x + ax, y + ay, z + az) == k) return true;
    }
    return false;
}

__global__ void __launch_bounds__(256) label_tiles_kernel(const int32_t* __restrict__ labels, int* __restrict__ parent, Geo g) {
    __shared__ int kv[kTile];    // keys of the tile, -1 outside the volume
    __shared__ int lab[kTile];
    const int tz = blockIdx.x % g.ntz, ty = (blockIdx.x / g.ntz) % g.nty, tx = blockIdx.x / (g.ntz * g.nty);
    const int lz = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int z = tz * kTZ + lz;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, x = tx * kTX + (r >> 3), y = ty * kTY + (r & 7), l = r * kTZ + lz;
        int k = -1;
        if (x < g.X && y < g.Y && z < g.Z) k = key_of(labels[((long long)x * g.Y + y) * g.Z + z], g.which);
        // runs along z: a wave is one row, and a voxel starts under the first voxel of its run
        const int below = __shfl_up(k, 1);
        const unsigned long long heads = __ballot(k >= 0 && (lz == 0 || below != k));
        const unsigned long long mine = heads & ((2ull << lz) - 1ull);
        kv[l] = k;
        lab[l] = k >= 0 ? r * kTZ + (63 - __clzll((long long)mine)) : -1;
    }
    __syncthreads();
    auto key = [&](int lx, int ly, int lzz) -> int {
        return (lx < 0 || lx >= kTX || ly < 0 || ly >= kTY || lzz < 0 || lzz >= kTZ) ? -2 : kv[(lx * kTY + ly) * kTZ + lzz];
    };
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, lx = r >> 3, ly = r & 7, l = r * kTZ + lz;
        const int k = kv[l];
        if (k < 0) continue;
        // the z direction is done by the runs; x and y: once per pair of runs, at the lowest z they share
        if (lx > 0 && kv[l - kTY * kTZ] == k && !(lz > 0 && kv[l - 1] == k && kv[l - kTY * kTZ - 1] == k))
            unite(lab, l, l - kTY * kTZ);
        if (ly > 0 && kv[l - kTZ] == k && !(lz > 0 && kv[l - 1] == k && kv[l - kTZ - 1] == k)) unite(lab, l, l - kTZ);
        for (int d = 3; d < g.ndir; ++d) {
            const int dx = kDir[d][0], dy = kDir[d][1], dz = kDir[d][2];
            if (key(lx + dx, ly + dy, lz + dz) != k) continue;
            if (diagonal_implied(key, lx, ly, lz, dx, dy, dz, k)) continue;
            unite(lab, l, ((lx + dx) * kTY + ly + dy) * kTZ + lz + dz);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, x = tx * kTX + (r >> 3), y = ty * kTY + (r & 7), l = r * kTZ + lz;
        if (x >= g.X || y >= g.Y || z >= g.Z) continue;
        int out = -1;
        if (lab[l] >= 0) {
            const int q = find_root(lab, l);   // nothing writes lab any more
            const int qr = q >> 6;
            out = ((tx * kTX + (qr >> 3)) * g.Y + ty * kTY + (qr & 7)) * g.Z + tz * kTZ + (q & 63);
        }
        parent[(x * g.Y + y) * g.Z + z] = out;
    }
}

__global__ void __launch_bounds__(256) merge_borders_kernel(const int32_t* __restrict__ labels, int* __restrict__ parent, Geo g) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int yz = g.Y * g.Z;
    auto key = [&](int xx, int yy, int zz) -> int {
        return (xx < 0 || xx >= g.X || yy < 0 || yy >= g.Y || zz < 0 || zz >= g.Z) ? -2
                                                                                    : key_of(labels[(xx * g.Y + yy) * g.Z + zz], g.which);
    };
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n; e += stride) {
        const int i = (int)e, x = i / yz, q = i - x * yz, y = q / g.Z, z = q - y * g.Z;
        const int fx = x & (kTX - 1), fy = y & (kTY - 1), fz = z & (kTZ - 1);
        if (fx != 0 && fx != kTX - 1 && fy != 0 && fy != kTY - 1 && fz != 0 && fz != kTZ - 1) continue;   // inside its tile
        const int k = key_of(labels[i], g.which);
        if (k < 0) continue;
        for (int d = 0; d < g.ndir; ++d) {
            const int dx = kDir[d][0], dy = kDir[d][1], dz = kDir[d][2];
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            if (nx < 0 || ny < 0 || ny >= g.Y || nz < 0 || nz >= g.Z) continue;
            if ((nx / kTX == x / kTX) && (ny / kTY == y / kTY) && (nz / kTZ == z / kTZ)) continue;   // the tile's own pair
            if (key(nx, ny, nz) != k) continue;
            if (d < 3) {
                // the twin of this pair one step down z (down y for the z direction) lies in the same two tiles: when
                // it holds k too, both ends are joined to it inside their tiles, and it is united on its own
                if (d < 2 ? (fz != 0 && key(x, y, z - 1) == k && key(nx, ny, nz - 1) == k)
                          : (fy != 0 && key(x, y - 1, z) == k && key(nx, ny - 1, nz) == k))
                    continue;
            } else if (diagonal_implied(key, x, y, z, dx, dy, dz, k)) {
                continue;
            }
            unite(parent, i, (nx * g.Y + ny) * g.Z + nz);
        }
    }
}

// block = one chunk.  Roots do not change here, so reading an ancestor that another thread is compressing still leads
// to the root.
__global__ void __launch_bounds__(256) flatten_count_kernel(int* __restrict__ parent, Geo g, int* __restrict__ chunk_count) {
    __shared__ int wsum[4];
    const long long q0 = (long long)blockIdx.x * kChunk;
    int c = 0;
    for (int j = threadIdx.x; j < kChunk; j += 256) {
        const long long q = q0 + j;
        if (q >= g.n) break;
        const int i = (int)q;
        if (parent[i] < 0) continue;
        const int r = find_root(parent, i);
        if (r != i)
            parent[i] = r;
        else
            ++c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: chunk counts -> exclusive prefix (in place), *total
__global__ void __launch_bounds__(1024) scan_chunks_kernel(int* __restrict__ chunk, int nchunks, int32_t* __restrict__ total) {
    __shared__ int part[1024];
    const int per = (nchunks + 1023) / 1024;
    const int lo = min(nchunks, (int)threadIdx.x * per), hi = min(nchunks, lo + per);
    int s = 0;
    for (int j = lo; j < hi; ++j) s += chunk[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int t = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int j = lo; j < hi; ++j) {
        const int v = chunk[j];
        chunk[j] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total = part[1023];
}

// ranks[root] = 1 + the rank of the root in raster order; every voxel of the other kind gets 0 here
__global__ void __launch_bounds__(256) rank_roots_kernel(const int* __restrict__ parent, int32_t* __restrict__ ranks, Geo g,
                                                         const int* __restrict__ chunk_offset) {
    __shared__ int wpre[4];
    const long long q0 = (long long)blockIdx.x * kChunk;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int run = chunk_offset[blockIdx.x];
    for (int j = 0; j < kChunk; j += 256) {   // rounds of 256 consecutive voxels keep raster order
        const long long q = q0 + j + threadIdx.x;
        const int i = (int)q;
        const int p = q < g.n ? parent[i] : -1;
        const bool root = q < g.n && p == i;
        const unsigned long long bal = __ballot(root);
        if (lane == 0) wpre[wv] = __popcll(bal);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wpre[w];
        const int tot = wpre[0] + wpre[1] + wpre[2] + wpre[3];
        if (root)
            ranks[i] = run + before + __popcll(bal & ((1ull << lane) - 1ull)) + 1;
        else if (q < g.n && p < 0)
            ranks[i] = 0;
        run += tot;
        __syncthreads();
    }
}

// flattened: parent[i] is the root, whose slot the rank pass filled; a root's own slot is written by nobody here
__global__ void __launch_bounds__(256) write_ranks_kernel(const int* __restrict__ parent, int32_t* __restrict__ ranks, Geo g) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n; e += stride) {
        const int i = (int)e, p = parent[i];
        if (p >= 0 && p != i) ranks[i] = ranks[p];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// sk_component_table
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) init_rows_kernel(long long* __restrict__ rows, int P) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < P; r += stride) {
        long long* row = rows + r * kCols;
        row[0] = 0;
        row[1] = 0;
        row[2] = kNone;
        row[3] = 0;
        row[4] = kNone;
        row[5] = 0;
    }
}

__global__ void __launch_bounds__(256) table_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ piece, Geo g,
                                                    int P, long long* __restrict__ rows) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63, yz = g.Y * g.Z;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e - lane < g.n; e += stride) {   // whole waves iterate
        int p = 0, v = 0, bits = 0, nmin = 0x7fffffff, nmax = 0;
        if (e < g.n) {
            const int i = (int)e;
            p = piece[i];
            if (p < 0 || p > P) p = 0;   // not a piece of this table: never a row out of bounds
            if (p > 0) {
                v = labels[i];
                const int x = i / yz, q = i - x * yz, y = q / g.Z, z = q - y * g.Z;
                bits = (x == 0 ? 1 : 0) | (x == g.X - 1 ? 2 : 0) | (y == 0 ? 4 : 0) | (y == g.Y - 1 ? 8 : 0) | (z == 0 ? 16 : 0) |
                       (z == g.Z - 1 ? 32 : 0);
                if (v == 0) {   // a zero piece: the positive ids around it
                    int nb[6];
                    nb[0] = x > 0 ? labels[i - yz] : 0;
                    nb[1] = x < g.X - 1 ? labels[i + yz] : 0;
                    nb[2] = y > 0 ? labels[i - g.Z] : 0;
                    nb[3] = y < g.Y - 1 ? labels[i + g.Z] : 0;
                    nb[4] = z > 0 ? labels[i - 1] : 0;
                    nb[5] = z < g.Z - 1 ? labels[i + 1] : 0;
#pragma unroll
                    for (int j = 0; j < 6; ++j)
                        if (nb[j] > 0) {
                            nmin = min(nmin, nb[j]);
                            nmax = max(nmax, nb[j]);
                        }
                }
            }
        }
        const unsigned long long live = __ballot(p != 0);
        if (live == 0) continue;
        const int below = __shfl_up(p, 1);
        const bool head = p != 0 && (lane == 0 || below != p);
        const unsigned long long heads = __ballot(head);
        // the run of this lane ends before the next lane that starts a run or holds no piece
        const unsigned long long above = (heads | ~live) & ~((2ull << lane) - 1ull);
        const int last = above ? __ffsll((long long)above) - 2 : 63;
        if (__ballot(bits != 0 || nmax != 0)) {   // rare inside a body: or / min / max over the run, towards its first lane
            for (int o = 1; o < 64; o <<= 1) {
                const int b2 = __shfl_down(bits, o), mn2 = __shfl_down(nmin, o), mx2 = __shfl_down(nmax, o);
                if (lane + o <= last) {
                    bits |= b2;
                    nmin = min(nmin, mn2);
                    nmax = max(nmax, mx2);
                }
            }
        }
        if (head) {
            long long* row = rows + (long long)(p - 1) * kCols;
            atomicMax((unsigned long long*)&row[0], (unsigned long long)(unsigned)v);   // one value per piece
            atomicAdd((unsigned long long*)&row[1], (unsigned long long)(last - lane + 1));
            atomicMin(&row[2], (long long)e);
            if (bits) atomicOr((unsigned long long*)&row[3], (unsigned long long)bits);
            if (nmax > 0) {
                atomicMin(&row[4], (long long)nmin);
                atomicMax(&row[5], (long long)nmax);
            }
        }
    }
}

__global__ void __launch_bounds__(256) finish_rows_kernel(long long* __restrict__ rows, int P) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < P; r += stride) {
        long long* row = rows + r * kCols;
        if (row[2] == kNone) row[2] = -1;   // a row no voxel names
        if (row[4] == kNone) row[4] = 0;    // no positive neighbour
    }
}

__global__ void __launch_bounds__(256) apply_lut_kernel(const int32_t* __restrict__ piece, const int32_t* __restrict__ lut,
                                                        int n_lut, int32_t* __restrict__ out, long long n, int only_pieces) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int p = piece[e];
        if (only_pieces && p <= 0) continue;
        out[e] = (p >= 0 && p < n_lut) ? lut[p] : 0;
    }
}

bool make_geo(Geo& g, int X, int Y, int Z, int connectivity, int which) {
    if (X <= 0 || Y <= 0 || Z <= 0) return false;
    const long long n = (long long)X * Y * Z;
    if (n >= 0x80000000LL) return false;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return false;
    if (which != 0 && which != 1) return false;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    g.n = (int)n;
    g.ntx = (X + kTX - 1) / kTX;
    g.nty = (Y + kTY - 1) / kTY;
    g.ntz = (Z + kTZ - 1) / kTZ;
    g.nchunks = (int)((n + kChunk - 1) / kChunk);
    g.which = which;
    g.ndir = which == 0 ? 3 : connectivity == 6 ? 3 : connectivity == 18 ? 9 : 13;
    // one workgroup per tile: thin volumes have many tiles for their voxels (a 1 x 1 x Z line has Z / 64 of them, an
    // X x 1 x 1 line X); 2^31 - 1 is the grid's limit
    return (long long)g.ntx * g.nty * g.ntz <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int sk_component_table_row_values(void) { return kCols; }

size_t sk_label_components_workspace_bytes(int X, int Y, int Z) {
    Geo g;
    if (!make_geo(g, X, Y, Z, 6, 1)) return 0;
    return ((size_t)g.nchunks + 16) * sizeof(int);
}

int sk_label_components(const int32_t* labels, int X, int Y, int Z, int connectivity, int which, int32_t* parent, int32_t* ranks,
                        int32_t* n_components, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Geo g;
    SK_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "sk_label_components: connectivity must be 6, 18 or 26, got %d", connectivity);
    SK_CHECK_ARG(which == 0 || which == 1, "sk_label_components: which must be 1 (positive values) or 0 (zero voxels), got %d", which);
    SK_CHECK_ARG(make_geo(g, X, Y, Z, connectivity, which), "sk_label_components: a volume of %d x %d x %d: extents must be positive and X Y Z below 2^31 (parents are int32 voxel indices)", X, Y, Z);
    SK_CHECK_ARG(labels && parent && ranks && n_components && workspace, "sk_label_components: NULL pointer");
    SK_CHECK_ARG((((uintptr_t)labels | (uintptr_t)parent | (uintptr_t)ranks | (uintptr_t)n_components | (uintptr_t)workspace) & 3) == 0, "sk_label_components: pointers must be 4-byte aligned");
    SK_CHECK_ARG(workspace_bytes >= sk_label_components_workspace_bytes(X, Y, Z), "sk_label_components: workspace too small (%zu < %zu)",
                 workspace_bytes, sk_label_components_workspace_bytes(X, Y, Z));
    int* chunk = (int*)workspace;
    label_tiles_kernel<<<(unsigned)(g.ntx * g.nty * g.ntz), 256, 0, stream>>>(labels, parent, g);
    if (g.ntx * g.nty * g.ntz > 1) merge_borders_kernel<<<sk::stream_grid(g.n, 256), 256, 0, stream>>>(labels, parent, g);
    flatten_count_kernel<<<g.nchunks, 256, 0, stream>>>(parent, g, chunk);
    scan_chunks_kernel<<<1, 1024, 0, stream>>>(chunk, g.nchunks, n_components);
    rank_roots_kernel<<<g.nchunks, 256, 0, stream>>>(parent, ranks, g, chunk);
    write_ranks_kernel<<<sk::stream_grid(g.n, 256), 256, 0, stream>>>(parent, ranks, g);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_component_table(const int32_t* labels, const int32_t* piece, int X, int Y, int Z, int P, int64_t* rows, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Geo g;
    SK_CHECK_ARG(make_geo(g, X, Y, Z, 6, 1), "sk_component_table: a volume of %d x %d x %d: extents must be positive and X Y Z below 2^31", X, Y, Z);
    SK_CHECK_ARG(P >= 0, "sk_component_table: %d pieces", P);
    if (P == 0) return SK_OK;
    SK_CHECK_ARG(labels && piece && rows, "sk_component_table: NULL pointer");
    SK_CHECK_ARG((((uintptr_t)labels | (uintptr_t)piece) & 3) == 0 && ((uintptr_t)rows & 7) == 0, "sk_component_table: pointers must be aligned to their elements");
    init_rows_kernel<<<sk::stream_grid(P, 256), 256, 0, stream>>>((long long*)rows, P);
    table_kernel<<<sk::stream_grid(g.n, 256), 256, 0, stream>>>(labels, piece, g, P, (long long*)rows);
    finish_rows_kernel<<<sk::stream_grid(P, 256), 256, 0, stream>>>((long long*)rows, P);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_apply_piece_lut(const int32_t* piece, const int32_t* lut, int n_lut, int32_t* out, int64_t n, int only_pieces, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SK_CHECK_ARG(n >= 0 && n_lut >= 0, "sk_apply_piece_lut: n %lld, table of %d", (long long)n, n_lut);
    if (n == 0) return SK_OK;
    SK_CHECK_ARG(piece && out && (lut || n_lut == 0), "sk_apply_piece_lut: NULL pointer");
    SK_CHECK_ARG((((uintptr_t)piece | (uintptr_t)lut | (uintptr_t)out) & 3) == 0, "sk_apply_piece_lut: pointers must be 4-byte aligned");
    apply_lut_kernel<<<sk::stream_grid(n, 256), 256, 0, stream>>>(piece, lut, n_lut, out, (long long)n, only_pieces ? 1 : 0);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
