// Surface voxels of every instance and exact nearest-neighbour distances between surface voxel sets (DESIGN.md
// section 25): the kernels under validate/compare.py: compare().  The definitions are in include/skoots_hip.h.
//
// Names
//   * row: r(v), the row 1..N of voxel v through lut as in every per-instance kernel; 0 for background, unlisted ids
//     and every position outside the volume.
//   * surface voxel of row a: a voxel of row a with a face neighbour of another row (outside counts as row 0).
//   * surface key: (a - 1) X Y Z + ((x Y + y) Z + z), int64.  key mod X Y Z is the voxel, whatever the row.
//
// Shape of the kernels
//   * sk_instance_surface_count / _emit walk the volume in tiles of kThreads x kPer consecutive voxels, thread t taking
//     the voxels t, t + kThreads, ... of the tile (coalesced), and read the six neighbours of a foreground voxel from
//     global memory (they are the same cache lines a neighbouring thread or tile reads).  The count pass adds into a
//     table in LDS keyed by row and flushes it once per tile with 64-bit global atomics (the table of instance_mesh.hip;
//     a row that finds no slot adds to global memory directly).  The emit pass takes the thread's share of the tile with
//     one LDS atomic, one thread takes the tile's share of the output with ONE global atomic, and the keys are written;
//     a key whose slot is at or beyond the capacity is not written, the counter still advances.
//   * sk_surface_distances: the outputs of all pairs are one flat array; a workgroup takes kThreads consecutive outputs
//     (one query each) and the pairs that own them, one pair after another -- a large pair fills whole workgroups, many
//     tiny pairs share one.  For a pair the target segment goes through LDS in tiles of kTile decoded voxels, and every
//     thread scans the tile: all lanes read the same LDS address (a broadcast, no bank conflict), one 16-byte read per
//     target.  While staging a tile the workgroup takes the minimum and maximum x of its voxels (integer LDS atomics);
//     a thread whose query lies `gap` voxels outside that range skips the tile when fl(wx gap^2) is not below its best:
//     every candidate of the tile has |dx| >= gap, rounding is monotone and the other terms are >= 0, so none can be
//     smaller.  The bound is taken from the tile's own voxels, so it holds for keys in any order; sorted keys (x-major)
//     make the range narrow.  The tiles are visited outward from the one where the workgroup's first query would sort
//     in, so the best is small before the far tiles are looked at.  A minimum does not depend on the order: the result
//     is the definition's bits however the search is tiled, ordered or pruned.
//   * Integer atomics only, every d2 element has one writer, nothing accumulates in floating point.
#include "instance_rows.h"

#include <limits.h>

#include <new>
#include <vector>

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kPer = 8;                               // voxels per thread and tile of the surface kernels
constexpr int kSlotBits = 6, kSlots = 1 << kSlotBits;  // rows the LDS table of the count kernel holds per tile
constexpr int kProbes = 8;                            // linear probes before a count goes to global memory
constexpr int kTile = 1024;                           // target voxels per LDS tile of the distance kernel: 16 KiB
constexpr int kMaxExtent = 1 << 26;                   // d^2 < 2^52: exact in double

static_assert(kSlots <= kThreads, "one thread per counter of the table");
static_assert(kPer <= 32, "the surface flags of a thread are the bits of one word");

struct Vol {
    int X, Y, Z;
    u64 YZ, V;                                        // Y Z and X Y Z
};

struct Target {                                       // one decoded target voxel in LDS: one 16-byte broadcast read
    int x, y, z, pad;
};

// (x, y, z) of voxel `lin` < V; kSmall: V < 2^32, 32-bit divisions
template <bool kSmall>
__device__ inline void decode(u64 lin, const Vol& g, int& x, int& y, int& z) {
    if (kSmall) {
        const unsigned l = (unsigned)lin, yz = (unsigned)g.YZ;
        const unsigned qx = l / yz, r = l - qx * yz, qy = r / (unsigned)g.Z;
        x = (int)qx, y = (int)qy, z = (int)(r - qy * (unsigned)g.Z);
    } else {
        const u64 qx = lin / g.YZ, r = lin - qx * g.YZ, qy = r / (u64)g.Z;
        x = (int)qx, y = (int)qy, z = (int)(r - qy * (u64)g.Z);
    }
}

// the row of voxel v when it is a surface voxel of that row, else 0
template <bool kSmall>
__device__ inline int surface_row(const int* __restrict__ lab, const int* __restrict__ lut, int max_id, int N,
                                  const Vol& g, u64 v) {
    const int label = lab[v];
    const int a = sk::row_of(label, lut, max_id, N);
    if (a == 0) return 0;
    int x, y, z;
    decode<kSmall>(v, g, x, y, z);
    // a neighbour with the same label has the same row; another label goes through the table
    auto differs = [&](u64 n) {
        const int nl = lab[n];
        return nl != label && sk::row_of(nl, lut, max_id, N) != a;
    };
    const u64 sy = (u64)g.Z, sx = g.YZ;
    if (x == 0 || x == g.X - 1 || y == 0 || y == g.Y - 1 || z == 0 || z == g.Z - 1) return a;   // outside is row 0
    if (differs(v - 1) || differs(v + 1) || differs(v - sy) || differs(v + sy) || differs(v - sx) || differs(v + sx))
        return a;
    return 0;
}

template <bool kSmall>
__global__ void __launch_bounds__(kThreads) surface_count_kernel(const int* __restrict__ lab, const int* __restrict__ lut,
                                                                 int max_id, int N, Vol g, long long ntiles,
                                                                 u64* __restrict__ counts) {
    __shared__ unsigned s_cnt[kSlots];
    __shared__ int s_key[kSlots];
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();                                   // the previous tile's flush has read the table
        if (tid < kSlots) s_cnt[tid] = 0, s_key[tid] = 0;
        __syncthreads();
        const u64 base = (u64)t * (kThreads * kPer) + tid;
        for (int j = 0; j < kPer; ++j) {
            const u64 v = base + (u64)j * kThreads;
            if (v >= g.V) break;
            const int a = surface_row<kSmall>(lab, lut, max_id, N, g, v);
            if (a == 0) continue;
            const int s = sk::claim_slot<kSlotBits, kProbes>(s_key, a);
            if (s >= 0)
                atomicAdd(&s_cnt[s], 1u);
            else                                           // the table is full for this row: global memory directly
                atomicAdd(&counts[a - 1], (u64)1);
        }
        __syncthreads();
        if (tid < kSlots) {                                // flush: one global atomic per used counter
            const int key = s_key[tid];
            const unsigned n = s_cnt[tid];
            if (key != 0 && n != 0) atomicAdd(&counts[key - 1], (u64)n);
        }
    }
}

template <bool kSmall>
__global__ void __launch_bounds__(kThreads) surface_emit_kernel(const int* __restrict__ lab, const int* __restrict__ lut,
                                                                int max_id, int N, Vol g, long long ntiles,
                                                                long long* __restrict__ keys, long long capacity,
                                                                u64* __restrict__ produced) {
    __shared__ unsigned s_total;
    __shared__ u64 s_first;
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();                                   // the previous tile has read s_total and s_first
        if (tid == 0) s_total = 0;
        __syncthreads();
        const u64 base = (u64)t * (kThreads * kPer) + tid;
        int rows[kPer];
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const u64 v = base + (u64)j * kThreads;
            rows[j] = v < g.V ? surface_row<kSmall>(lab, lut, max_id, N, g, v) : 0;
            n += rows[j] != 0;
        }
        const unsigned mine = n ? atomicAdd(&s_total, n) : 0u;
        __syncthreads();
        if (tid == 0) {                                    // the tile's share of the output: one global atomic
            const unsigned total = s_total;
            s_first = total ? atomicAdd(produced, (u64)total) : 0ull;
        }
        __syncthreads();
        long long at = (long long)(s_first + mine);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (rows[j] == 0) continue;
            if (at < capacity) keys[at] = (long long)((u64)(rows[j] - 1) * g.V + (base + (u64)j * kThreads));
            ++at;
        }
    }
}

template <bool kSmall>
__global__ void __launch_bounds__(kThreads) surface_distances_kernel(
    const long long* __restrict__ q_keys, const long long* __restrict__ q_off, const long long* __restrict__ t_keys,
    const long long* __restrict__ t_off, const int* __restrict__ pairs, int P, const long long* __restrict__ out_off,
    Vol g, double wx, double wy, double wz, double* __restrict__ d2) {
    __shared__ Target s_t[kTile];
    __shared__ int s_lo[2], s_hi[2];                       // x range of the staged tile, one slot per parity of `round`
    const int tid = threadIdx.x;
    if (tid < 2) s_lo[tid] = INT_MAX, s_hi[tid] = INT_MIN; // the first barrier below publishes it
    unsigned round = 0;                                    // tiles this workgroup has staged
    const long long total = out_off[P];
    const long long nchunks = (total + kThreads - 1) / kThreads;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long lo = c * kThreads, hi = lo + kThreads < total ? lo + kThreads : total, i = lo + tid;
        int ka = 0, kb = P;                                // the last pair that starts at or before lo
        while (kb - ka > 1) {
            const int m = ka + (kb - ka) / 2;
            if (out_off[m] <= lo)
                ka = m;
            else
                kb = m;
        }
        for (int k = ka; k < P; ++k) {
            const long long o0 = out_off[k], o1 = out_off[k + 1];
            if (o0 >= hi) break;
            if (o1 <= lo || o1 == o0) continue;
            const long long qb = q_off[pairs[2 * k]] - o0;             // query of output i: q_keys[qb + i]
            const long long tb = t_off[pairs[2 * k + 1]], tn = t_off[pairs[2 * k + 1] + 1] - tb;
            const bool mine = i >= o0 && i < o1;
            int qx = 0, qy = 0, qz = 0;
            if (mine) decode<kSmall>((u64)q_keys[qb + i] % g.V, g, qx, qy, qz);
            double best = INFINITY;
            const long long ntiles = (tn + kTile - 1) / kTile;
            // the tile where the first query of this pair in the chunk would sort in: the last one that starts at or
            // before it.  Any start gives the same result; this one makes the best small early.
            long long above = 0;
            if (ntiles > 1) {
                const u64 first = (u64)q_keys[qb + (lo > o0 ? lo : o0)] % g.V;
                long long b = ntiles;
                while (b - above > 1) {
                    const long long m = above + (b - above) / 2;
                    if ((u64)t_keys[tb + m * kTile] % g.V <= first)
                        above = m;
                    else
                        b = m;
                }
            }
            long long below = above - 1;
            for (long long m = 0; m < ntiles; ++m) {
                const bool up = above < ntiles && (below < 0 || (m & 1) == 0);
                const long long t0 = (up ? above++ : below--) * kTile;
                const int n = (int)(tn - t0 < kTile ? tn - t0 : kTile);
                const int slot = (int)(round & 1u);
                __syncthreads();                           // the previous tile has been scanned
                int mn = INT_MAX, mx = INT_MIN;
                for (int j = tid; j < n; j += kThreads) {
                    Target v;
                    decode<kSmall>((u64)t_keys[tb + t0 + j] % g.V, g, v.x, v.y, v.z);
                    v.pad = 0;
                    s_t[j] = v;
                    mn = v.x < mn ? v.x : mn;
                    mx = v.x > mx ? v.x : mx;
                }
                if (mn <= mx) atomicMin(&s_lo[slot], mn), atomicMax(&s_hi[slot], mx);
                __syncthreads();
                const int xlo = s_lo[slot], xhi = s_hi[slot];
                // the other slot was last read one tile ago, before the first barrier above; it is written again only
                // behind the next one
                if (tid == 0) s_lo[slot ^ 1] = INT_MAX, s_hi[slot ^ 1] = INT_MIN;
                ++round;
                if (!mine) continue;
                const double gap = (double)(qx < xlo ? xlo - qx : qx > xhi ? qx - xhi : 0);
                if (!(wx * (gap * gap) < best)) continue;  // exact: see the head of the file
#pragma unroll 4
                for (int j = 0; j < n; ++j) {
                    const Target v = s_t[j];
                    const double dx = (double)(qx - v.x), dy = (double)(qy - v.y), dz = (double)(qz - v.z);
                    const double d = wx * (dx * dx) + (wy * (dy * dy) + wz * (dz * dz));
                    best = d < best ? d : best;
                }
            }
            if (mine) d2[i] = best;
        }
    }
}

// the checks the two surface entry points share; *run = false when there is nothing to launch
int prepare_surface(const char* who, const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                    Vol* g, long long* ntiles, bool* run) {
    *run = false;
    // not sk::check_mask_header: the extent limit stands between its two checks here
    SK_CHECK_ARG(X >= 0 && Y >= 0 && Z >= 0, "%s: extents %d x %d x %d must not be negative", who, X, Y, Z);
    SK_CHECK_ARG(X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent, "%s: extents %d x %d x %d must not exceed 2^26", who,
                 X, Y, Z);
    SK_CHECK_ARG(N >= 0 && max_id >= 0, "%s: N = %d, max_id = %d must not be negative", who, N, max_id);
    const unsigned __int128 voxels = (unsigned __int128)X * Y * Z;                                        // below 2^79
    SK_CHECK_ARG(voxels * (unsigned __int128)(N > 0 ? N : 1) < ((unsigned __int128)1 << 63),
                 "%s: N = %d rows of %d x %d x %d voxels: N X Y Z must stay below 2^63, or the keys leave int64", who, N, X,
                 Y, Z);
    if (voxels == 0 || N == 0) return SK_OK;
    const int rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}});
    if (rc != SK_OK) return rc;
    g->X = X, g->Y = Y, g->Z = Z, g->YZ = (u64)Y * Z, g->V = (u64)voxels;
    *ntiles = (long long)((g->V + (u64)(kThreads * kPer) - 1) / (u64)(kThreads * kPer));
    *run = true;
    return SK_OK;
}

bool finite_positive(double w) { return w > 0.0 && w < INFINITY; }

}  // namespace

extern "C" {

int sk_surface_distance_tile(void) { return kTile; }

int sk_instance_surface_count(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                              int64_t* counts, void* stream) {
    Vol g;
    long long ntiles = 0;
    bool run;
    int rc = prepare_surface("sk_instance_surface_count", labels, X, Y, Z, lut, max_id, N, &g, &ntiles, &run);
    if (rc != SK_OK || !run) return rc;
    rc = sk::check_pointers("sk_instance_surface_count", {{counts, 8}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)N * sizeof(int64_t), st));
    const unsigned grid = sk::tile_blocks(ntiles);
    if (g.V < (1ull << 32))
        surface_count_kernel<true><<<grid, kThreads, 0, st>>>(labels, lut, max_id, N, g, ntiles, (u64*)counts);
    else
        surface_count_kernel<false><<<grid, kThreads, 0, st>>>(labels, lut, max_id, N, g, ntiles, (u64*)counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_instance_surface_emit(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                             int64_t capacity, int64_t* keys, int64_t* produced, void* stream) {
    Vol g;
    long long ntiles = 0;
    bool run;
    int rc = prepare_surface("sk_instance_surface_emit", labels, X, Y, Z, lut, max_id, N, &g, &ntiles, &run);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(capacity >= 0, "sk_instance_surface_emit: capacity %lld must not be negative", (long long)capacity);
    SK_CHECK_ARG(capacity < ((int64_t)1 << 60), "sk_instance_surface_emit: capacity %lld must stay below 2^60",
                 (long long)capacity);
    if (!run) return SK_OK;
    rc = sk::check_pointers("sk_instance_surface_emit", {{produced, 8}, {keys, 8, capacity == 0}});
    if (rc != SK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(produced, 0, sizeof(int64_t), st));
    const unsigned grid = sk::tile_blocks(ntiles);
    if (g.V < (1ull << 32))
        surface_emit_kernel<true><<<grid, kThreads, 0, st>>>(labels, lut, max_id, N, g, ntiles, (long long*)keys,
                                                             (long long)capacity, (u64*)produced);
    else
        surface_emit_kernel<false><<<grid, kThreads, 0, st>>>(labels, lut, max_id, N, g, ntiles, (long long*)keys,
                                                              (long long)capacity, (u64*)produced);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_surface_distances(const int64_t* q_keys, const int64_t* q_offsets, int q_segments, const int64_t* t_keys,
                         const int64_t* t_offsets, int t_segments, const int32_t* pairs, int P,
                         const int64_t* out_offsets, int X, int Y, int Z, double wx, double wy, double wz, double* d2,
                         void* stream) {
    const char* who = "sk_surface_distances";
    SK_CHECK_ARG(X >= 0 && Y >= 0 && Z >= 0, "%s: extents %d x %d x %d must not be negative", who, X, Y, Z);
    SK_CHECK_ARG(X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent, "%s: extents %d x %d x %d must not exceed 2^26", who,
                 X, Y, Z);
    SK_CHECK_ARG(P >= 0 && q_segments >= 0 && t_segments >= 0,
                 "%s: P = %d, q_segments = %d, t_segments = %d must not be negative", who, P, q_segments, t_segments);
    SK_CHECK_ARG(finite_positive(wx) && finite_positive(wy) && finite_positive(wz),
                 "%s: the weights %g, %g, %g must be finite and > 0", who, wx, wy, wz);
    if (P == 0) return SK_OK;
    SK_CHECK_ARG(q_offsets && t_offsets && pairs && out_offsets, "%s: NULL pointer", who);
    SK_CHECK_ARG(((uintptr_t)q_offsets & 7) == 0 && ((uintptr_t)t_offsets & 7) == 0 && ((uintptr_t)out_offsets & 7) == 0 &&
                     ((uintptr_t)pairs & 3) == 0 && ((uintptr_t)q_keys & 7) == 0 && ((uintptr_t)t_keys & 7) == 0 &&
                     ((uintptr_t)d2 & 7) == 0,
                 "%s: a pointer is not aligned to its elements", who);
    // The segment tables are small and decide every index the kernel forms into the key arrays and d2: they are read
    // back and checked here.  What cannot be checked is that the key arrays hold q_offsets[q_segments] and
    // t_offsets[t_segments] elements: their lengths are not arguments, as the length of labels is not elsewhere.
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> qo, to, oo;
    std::vector<int32_t> pr;
    try {
        qo.resize((size_t)q_segments + 1), to.resize((size_t)t_segments + 1), oo.resize((size_t)P + 1);
        pr.resize((size_t)P * 2);
    } catch (const std::bad_alloc&) {
        sk::set_error("%s: no host memory for the tables of %d + %d segments and %d pairs", who, q_segments, t_segments, P);
        return SK_ERR_CAPACITY;
    }
    SK_CHECK_HIP(hipMemcpyAsync(qo.data(), q_offsets, qo.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SK_CHECK_HIP(hipMemcpyAsync(to.data(), t_offsets, to.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SK_CHECK_HIP(hipMemcpyAsync(oo.data(), out_offsets, oo.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SK_CHECK_HIP(hipMemcpyAsync(pr.data(), pairs, pr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SK_CHECK_HIP(hipStreamSynchronize(st));
    SK_CHECK_ARG(qo[0] >= 0 && to[0] >= 0, "%s: offsets must not be negative", who);
    for (int s = 0; s < q_segments; ++s)
        SK_CHECK_ARG(qo[s] <= qo[s + 1], "%s: q_offsets must be monotone (segment %d)", who, s);
    for (int s = 0; s < t_segments; ++s)
        SK_CHECK_ARG(to[s] <= to[s + 1], "%s: t_offsets must be monotone (segment %d)", who, s);
    SK_CHECK_ARG(oo[0] == 0, "%s: out_offsets must start at 0, got %lld", who, (long long)oo[0]);
    bool targets = false;
    for (int k = 0; k < P; ++k) {
        const int qs = pr[2 * k], ts = pr[2 * k + 1];
        SK_CHECK_ARG(qs >= 0 && qs < q_segments && ts >= 0 && ts < t_segments,
                     "%s: pair %d names the segments (%d, %d) of %d and %d", who, k, qs, ts, q_segments, t_segments);
        SK_CHECK_ARG(oo[k] <= oo[k + 1], "%s: out_offsets must be monotone (pair %d)", who, k);
        SK_CHECK_ARG(oo[k + 1] - oo[k] == qo[qs + 1] - qo[qs],
                     "%s: pair %d has %lld outputs and %lld queries", who, k, (long long)(oo[k + 1] - oo[k]),
                     (long long)(qo[qs + 1] - qo[qs]));
        targets |= oo[k + 1] > oo[k] && to[ts + 1] > to[ts];
    }
    const int64_t total = oo[P];
    if (total == 0) return SK_OK;
    SK_CHECK_ARG(q_keys && d2 && (t_keys || !targets), "%s: NULL pointer", who);
    SK_CHECK_ARG(X > 0 && Y > 0 && Z > 0, "%s: keys in an empty volume %d x %d x %d", who, X, Y, Z);
    SK_CHECK_ARG((unsigned __int128)X * Y * Z < ((unsigned __int128)1 << 63), "%s: X Y Z must stay below 2^63", who);
    Vol g;
    g.X = X, g.Y = Y, g.Z = Z, g.YZ = (u64)Y * Z, g.V = (u64)X * g.YZ;
    const unsigned grid = sk::tile_blocks((total + kThreads - 1) / kThreads);
    if (g.V < (1ull << 32))
        surface_distances_kernel<true><<<grid, kThreads, 0, st>>>(
            (const long long*)q_keys, (const long long*)q_offsets, (const long long*)t_keys, (const long long*)t_offsets,
            pairs, P, (const long long*)out_offsets, g, wx, wy, wz, d2);
    else
        surface_distances_kernel<false><<<grid, kThreads, 0, st>>>(
            (const long long*)q_keys, (const long long*)q_offsets, (const long long*)t_keys, (const long long*)t_offsets,
            pairs, P, (const long long*)out_offsets, g, wx, wy, wz, d2);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
