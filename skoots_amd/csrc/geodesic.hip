// Geodesic assignment: every voxel of an instance goes to the seed that is nearest along paths that stay inside the
// instance.  No reference counterpart: the reference has no tool that cuts a fused instance.
//
// labels and seeds are (X, Y, Z) int32 volumes, Z fastest; (cx, cy, cz) are integer step costs in 1..255.  A path is a
// chain of 6-neighbours that all hold the same positive `labels` value, its cost the sum of its steps.  Every voxel gets
// one 64-bit key, cost in the high and seed in the low 32 bits, all ones for "none":
//   key(v) = min( own seed (cost 0),  min over same-valued 6-neighbours u of key(u) + step << 32 ),
// pairs compared lexicographically -- as unsigned 64-bit words.  Adding to the cost alone keeps that order, so the
// equations have one solution and the order of execution cannot show in it.
//   init    key = seed where labels > 0 and seeds > 0, none elsewhere; every tile is marked "changed"; a negative value
//           of either volume sets the error word;
//   round   one launch, a workgroup per 4 x 8 x 64 tile (components.hip's: a wave is one z row).  The keys live in TWO
//           buffers: a round reads `src` only and writes `dst` only, so no key is read while it is written and nothing is
//           handed from workgroup to workgroup inside a launch.  A tile takes its own keys and, once, the candidates its
//           face voxels get from the neighbour tiles' keys in `src`; then it relaxes in LDS until nothing in it changes
//           -- Jacobi sweeps between two barriers: all reads, then all writes; a z row is a forward and a backward
//           min-plus scan inside the wave, cut where `labels` changes -- and writes all its keys.  A tile exits at once
//           when neither it nor a face neighbour changed in the round before: then `dst` already holds its keys (the
//           buffer was written two rounds ago from the same input);
//   finish  keys -> owner (0 for none) and cost (-1 for none).
// No workgroup waits for another and every loop is bounded: a sweep that goes on has lowered a key, keys are bounded
// below, and the sweep count is capped by the tile's voxels.  The host launches rounds until one changes nothing
// (lib/morphology.py: geodesic_assign), under a bound of its own.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kTX = 4, kTY = 8, kTZ = 64;      // tile: a wave per z row, lanes along z
constexpr int kTile = kTX * kTY * kTZ;         // 2048 voxels, 8 per thread
constexpr u64 kNoKey = ~0ull;
constexpr int kMaxRounds = 64;                 // rounds per sk_geodesic_rounds call: one counter each

struct Geo {
    int X, Y, Z, n;
    int ntx, nty, ntz, ntiles;
    int cx, cy, cz;
    unsigned max_cost;
};

__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
// a neighbour's key one step on; "none" stays none (and never wraps)
__device__ __forceinline__ u64 stepped(u64 k, int step) { return k == kNoKey ? kNoKey : k + ((u64)(unsigned)step << 32); }
__device__ __forceinline__ u64 pruned(u64 k, unsigned max_cost) { return (unsigned)(k >> 32) > max_cost ? kNoKey : k; }

__global__ void __launch_bounds__(256) init_keys_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ seeds,
                                                        u64* __restrict__ keys, int* __restrict__ flags, int* __restrict__ error,
                                                        Geo g) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    bool negative = false;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n; e += stride) {
        const int v = labels[e], s = seeds[e];
        negative |= v < 0 || s < 0;
        keys[e] = (v > 0 && s > 0) ? (u64)(unsigned)s : kNoKey;
    }
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.ntiles; e += stride) {
        flags[e] = 1;               // round 0 reads this copy: every tile runs
        flags[g.ntiles + e] = 0;
    }
    if (negative) atomicOr(error, 1);
}

__global__ void __launch_bounds__(256) relax_tiles_kernel(const int32_t* __restrict__ labels, const u64* __restrict__ src,
                                                          u64* __restrict__ dst, const int* __restrict__ flag_in,
                                                          int* __restrict__ flag_out, int* __restrict__ changed_tiles, Geo g) {
    __shared__ u64 kv[kTile];
    __shared__ int lab[kTile];
    const int t = blockIdx.x;
    const int tz = t % g.ntz, ty = (t / g.ntz) % g.nty, tx = t / (g.ntz * g.nty);
    {
        // the same for every thread: the whole workgroup leaves, before any barrier
        int live = flag_in[t];
        if (tx > 0) live |= flag_in[t - g.nty * g.ntz];
        if (tx < g.ntx - 1) live |= flag_in[t + g.nty * g.ntz];
        if (ty > 0) live |= flag_in[t - g.ntz];
        if (ty < g.nty - 1) live |= flag_in[t + g.ntz];
        if (tz > 0) live |= flag_in[t - 1];
        if (tz < g.ntz - 1) live |= flag_in[t + 1];
        if (!live) {
            if (threadIdx.x == 0) flag_out[t] = 0;
            return;
        }
    }
    const int lz = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int z = tz * kTZ + lz;
    const long long yz = (long long)g.Y * g.Z;
    u64 cur[8];
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, lx = r >> 3, ly = r & 7, x = tx * kTX + lx, y = ty * kTY + ly, l = r * kTZ + lz;
        int v = 0;
        u64 k = kNoKey;
        if (x < g.X && y < g.Y && z < g.Z) {
            const long long i = ((long long)x * g.Y + y) * g.Z + z;
            v = labels[i];
            if (v > 0) {
                const u64 own = src[i];
                k = own;
                // the halo: keys of the neighbour tiles as the round before left them, read once
                if (lx == 0 && x > 0 && labels[i - yz] == v) k = umin64(k, stepped(src[i - yz], g.cx));
                if (lx == kTX - 1 && x + 1 < g.X && labels[i + yz] == v) k = umin64(k, stepped(src[i + yz], g.cx));
                if (ly == 0 && y > 0 && labels[i - g.Z] == v) k = umin64(k, stepped(src[i - g.Z], g.cy));
                if (ly == kTY - 1 && y + 1 < g.Y && labels[i + g.Z] == v) k = umin64(k, stepped(src[i + g.Z], g.cy));
                if (lz == 0 && z > 0 && labels[i - 1] == v) k = umin64(k, stepped(src[i - 1], g.cz));
                if (lz == kTZ - 1 && z + 1 < g.Z && labels[i + 1] == v) k = umin64(k, stepped(src[i + 1], g.cz));
                k = pruned(k, g.max_cost);
                changed |= k < own;
            } else {
                v = 0;
            }
        }
        cur[j] = k;
        kv[l] = k;
        lab[l] = v;
    }
    __syncthreads();
    // what never changes: which in-tile x / y neighbours hold the voxel's value (4 bits per row of this thread) and the
    // ends of its run along z (first and last lane, a byte per row: rows 0..3 in one word, 4..7 in the other)
    unsigned same = 0, head = 0, tail = 0, head_hi = 0, tail_hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, lx = r >> 3, ly = r & 7, l = r * kTZ + lz;
        const int v = lab[l];
        if (v > 0) {
            if (lx > 0 && lab[l - kTY * kTZ] == v) same |= 1u << (4 * j);
            if (lx < kTX - 1 && lab[l + kTY * kTZ] == v) same |= 2u << (4 * j);
            if (ly > 0 && lab[l - kTZ] == v) same |= 4u << (4 * j);
            if (ly < kTY - 1 && lab[l + kTZ] == v) same |= 8u << (4 * j);
        }
        const int below = __shfl_up(v, 1);
        const u64 heads = __ballot(lz == 0 || below != v);
        const u64 upto = (2ull << lz) - 1ull;                      // lanes 0 .. lz
        const int h = 63 - __clzll((long long)(heads & upto));     // lane 0 is always a head
        const u64 above = heads & ~upto;
        const int e = above ? __ffsll((long long)above) - 2 : 63;
        if (j < 4) {
            head |= (unsigned)h << (8 * j);
            tail |= (unsigned)e << (8 * j);
        } else {
            head_hi |= (unsigned)h << (8 * (j - 4));
            tail_hi |= (unsigned)e << (8 * (j - 4));
        }
    }
    // Jacobi sweeps: every thread reads, barrier, every thread writes its own voxels, barrier.  A sweep that goes on has
    // lowered a key; with the halo fixed, every sweep settles at least one more voxel for good, hence the cap.
    for (int sweep = 0; sweep < kTile; ++sweep) {
        u64 nk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = r0 + 4 * j, l = r * kTZ + lz;
            const unsigned s = same >> (4 * j);
            const int h = ((j < 4 ? head : head_hi) >> (8 * (j & 3))) & 255, e = ((j < 4 ? tail : tail_hi) >> (8 * (j & 3))) & 255;
            u64 k = cur[j];
            if (s & 1u) k = umin64(k, stepped(kv[l - kTY * kTZ], g.cx));
            if (s & 2u) k = umin64(k, stepped(kv[l + kTY * kTZ], g.cx));
            if (s & 4u) k = umin64(k, stepped(kv[l - kTZ], g.cy));
            if (s & 8u) k = umin64(k, stepped(kv[l + kTZ], g.cy));
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {                     // forward: from lower z, inside the run
                const u64 from = __shfl_up(k, o);
                if (lz - o >= h) k = umin64(k, stepped(from, o * g.cz));
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {                     // backward: from higher z
                const u64 from = __shfl_down(k, o);
                if (lz + o <= e) k = umin64(k, stepped(from, o * g.cz));
            }
            nk[j] = pruned(k, g.max_cost);
        }
        __syncthreads();
        bool lowered = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (nk[j] < cur[j]) {
                cur[j] = nk[j];
                kv[(r0 + 4 * j) * kTZ + lz] = nk[j];
                lowered = true;
            }
        }
        changed |= lowered;
        if (!__syncthreads_or(lowered ? 1 : 0)) break;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = r0 + 4 * j, x = tx * kTX + (r >> 3), y = ty * kTY + (r & 7);
        if (x < g.X && y < g.Y && z < g.Z) dst[((long long)x * g.Y + y) * g.Z + z] = cur[j];
    }
    const int any = __syncthreads_or(changed ? 1 : 0);
    if (threadIdx.x == 0) {
        flag_out[t] = any ? 1 : 0;
        if (any) atomicAdd(changed_tiles, 1);
    }
}

__global__ void __launch_bounds__(256) finish_keys_kernel(const u64* __restrict__ keys, int32_t* __restrict__ owner,
                                                          int32_t* __restrict__ cost, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const u64 k = keys[e];
        owner[e] = k == kNoKey ? 0 : (int32_t)(unsigned)k;
        cost[e] = k == kNoKey ? -1 : (int32_t)(unsigned)(k >> 32);
    }
}

bool make_geo(Geo& g, int X, int Y, int Z, int cx, int cy, int cz, long long max_cost) {
    if (X <= 0 || Y <= 0 || Z <= 0) return false;
    const long long n = (long long)X * Y * Z;
    if (n >= 0x80000000LL) return false;
    if (cx < 1 || cx > 255 || cy < 1 || cy > 255 || cz < 1 || cz > 255) return false;
    const long long top = cx > cy ? (cx > cz ? cx : cz) : (cy > cz ? cy : cz);
    if (top * n >= 0x80000000LL) return false;   // a path has fewer than n steps: every cost stays an int32
    if (max_cost < -1) return false;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    g.n = (int)n;
    g.ntx = (X + kTX - 1) / kTX;
    g.nty = (Y + kTY - 1) / kTY;
    g.ntz = (Z + kTZ - 1) / kTZ;
    const long long ntiles = (long long)g.ntx * g.nty * g.ntz;
    if (ntiles > 0x3fffffffLL) return false;     // one workgroup per tile, two flags per tile
    g.ntiles = (int)ntiles;
    g.cx = cx;
    g.cy = cy;
    g.cz = cz;
    g.max_cost = (max_cost < 0 || max_cost > 0x7fffffffLL) ? 0x7fffffffu : (unsigned)max_cost;
    return true;
}

const char* kRefused =
    "%s: a volume of %d x %d x %d at costs (%d, %d, %d), max_cost %lld: extents must be positive, costs in 1..255, "
    "max(costs) X Y Z below 2^31 (costs are int32) and max_cost >= -1 (-1 = no limit)";

}  // namespace

extern "C" {

int sk_geodesic_tiles(int X, int Y, int Z) {
    Geo g;
    return make_geo(g, X, Y, Z, 1, 1, 1, -1) ? g.ntiles : 0;
}

int sk_geodesic_max_rounds(void) { return kMaxRounds; }

int sk_geodesic_init(const int32_t* labels, const int32_t* seeds, int X, int Y, int Z, uint64_t* keys, int32_t* flags,
                     int32_t* error, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Geo g;
    SK_CHECK_ARG(make_geo(g, X, Y, Z, 1, 1, 1, -1), "sk_geodesic_init: a volume of %d x %d x %d: extents must be positive and X Y Z below 2^31", X, Y, Z);
    SK_CHECK_ARG(labels && seeds && keys && flags && error, "sk_geodesic_init: NULL pointer");
    SK_CHECK_ARG((((uintptr_t)labels | (uintptr_t)seeds | (uintptr_t)flags | (uintptr_t)error) & 3) == 0 && ((uintptr_t)keys & 7) == 0,
                 "sk_geodesic_init: pointers must be aligned to their elements");
    SK_CHECK_HIP(hipMemsetAsync(error, 0, sizeof(int32_t), stream));
    init_keys_kernel<<<sk::stream_grid(g.n, 256), 256, 0, stream>>>(labels, seeds, (u64*)keys, flags, error, g);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_geodesic_rounds(const int32_t* labels, int X, int Y, int Z, int cx, int cy, int cz, int64_t max_cost, uint64_t* keys_a,
                       uint64_t* keys_b, int32_t* flags, int first_round, int n_rounds, int32_t* changed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Geo g;
    SK_CHECK_ARG(make_geo(g, X, Y, Z, cx, cy, cz, max_cost), kRefused, "sk_geodesic_rounds", X, Y, Z, cx, cy, cz, (long long)max_cost);
    SK_CHECK_ARG(first_round >= 0 && n_rounds >= 1 && n_rounds <= kMaxRounds && first_round <= 0x7fffffff - kMaxRounds,
                 "sk_geodesic_rounds: rounds %d .. + %d: at most %d per call", first_round, n_rounds, kMaxRounds);
    SK_CHECK_ARG(labels && keys_a && keys_b && flags && changed, "sk_geodesic_rounds: NULL pointer");
    SK_CHECK_ARG(keys_a != keys_b, "sk_geodesic_rounds: the two key buffers must be distinct");
    SK_CHECK_ARG((((uintptr_t)labels | (uintptr_t)flags | (uintptr_t)changed) & 3) == 0 && (((uintptr_t)keys_a | (uintptr_t)keys_b) & 7) == 0,
                 "sk_geodesic_rounds: pointers must be aligned to their elements");
    SK_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)n_rounds * sizeof(int32_t), stream));
    for (int k = 0; k < n_rounds; ++k) {
        const int r = first_round + k;            // even rounds read a and write b
        const u64* src = (const u64*)((r & 1) ? keys_b : keys_a);
        u64* dst = (u64*)((r & 1) ? keys_a : keys_b);
        const int* fin = flags + (size_t)(r & 1) * g.ntiles;
        int* fout = flags + (size_t)((r & 1) ^ 1) * g.ntiles;
        relax_tiles_kernel<<<(unsigned)g.ntiles, 256, 0, stream>>>(labels, src, dst, fin, fout, changed + k, g);
    }
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_geodesic_finish(const uint64_t* keys, int64_t n, int32_t* owner, int32_t* cost, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SK_CHECK_ARG(n >= 0 && n < 0x80000000LL, "sk_geodesic_finish: %lld voxels", (long long)n);
    if (n == 0) return SK_OK;
    SK_CHECK_ARG(keys && owner && cost, "sk_geodesic_finish: NULL pointer");
    SK_CHECK_ARG((((uintptr_t)owner | (uintptr_t)cost) & 3) == 0 && ((uintptr_t)keys & 7) == 0,
                 "sk_geodesic_finish: pointers must be aligned to their elements");
    finish_keys_kernel<<<sk::stream_grid(n, 256), 256, 0, stream>>>((const u64*)keys, owner, cost, (long long)n);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
