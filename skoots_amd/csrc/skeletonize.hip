// Lee (1994) 3-D thinning of training masks, one workgroup per object.
//
// Replaces the per-object skimage.morphology.skeletonize(crop, method="lee") call of
// skoots/train/generate_skeletons.py:65-157 (calculate_skeletons), whose thinning lives in scikit-image 0.18.3's
// skimage/morphology/_skeletonize_3d_cy.  The result is that of the sequential algorithm, bit for bit:
//
//   repeat until six border directions in a row delete nothing:
//     for d in (y-1, y+1, z+1, z-1, x+1, x-1):
//       C = foreground voxels p (raster order) whose neighbour p + d is background, that are not endpoints (exactly
//           one foreground 26-neighbour), are Euler invariant and are simple, all judged on the image as it is now;
//       for p in C (raster order): if p is still simple on the CURRENT image, delete p.
//
// Parallel re-check.  A candidate's re-check reads only its 26 neighbours; of those only candidates that come earlier
// in raster order can have changed, and they lie among its 13 raster-preceding neighbours.  So a candidate may be
// decided as soon as none of those is still pending ("ready"); two ready candidates are never 26-neighbours, so one
// round decides all ready candidates at once and reproduces the sequential result.  The earliest pending candidate is
// always ready: rounds <= candidates, and a pass that does not end the loop deletes a voxel: passes <= voxels + 1.
// Both bounds are enforced; a kernel that hits one sets a bit of the error word and stops that object.
//
// Storage.  The crop, padded by one background voxel on every side, is a bit plane: word ((x * PY + y) * WZ + wz)
// holds the voxels z = 32 wz .. 32 wz + 31 of row (x, y), WZ = ceil(PZ / 32).  Next to it a plane of pending
// candidates, the list of words that hold pending candidates (two, for this round and the next) and the list of
// (word, ready bits) pairs of the round: 6 words per plane word.  An object whose 24 * W bytes fit kLdsBytes keeps all
// of it in LDS; a larger one keeps it in a global workspace (same code, a device-scope fence at every barrier).
//
// Behind the thinning, on the image plane it leaves at the object's place in the workspace: emit_kernel (the points),
// graph_kernel (the skeleton as counts), pack_kernel (a given skeleton put there without
// thinning) and the branch tracing (trace_object: node and branch tables).
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBytes = 152 * 1024;  // dynamic LDS of the thinning kernel at most: 24 bytes per plane word
constexpr int kPlanes = 6;             // img, pending, list 0, list 1, ready words, ready bits

struct SkelObj {   // one object: crop origin, crop extent, where its planes live
    int x0, y0, z0;
    int cx, cy, cz;
    int lds;        // 1: working planes in LDS, result copied to `off`; 0: all six planes at `off`
    int pad;
    long long off;  // word offset of the object's planes in the workspace (after the table)
};

// 27-bit neighbourhood code: bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1)
constexpr uint32_t nb(int dx, int dy, int dz) { return 1u << (9 * (dx + 1) + 3 * (dy + 1) + (dz + 1)); }
constexpr uint32_t kFull = 0x7FFFFFFu;
constexpr uint32_t kCentre = 1u << 13;
constexpr uint32_t kK0 = 0x1249249u;  // dz = -1
constexpr uint32_t kK2 = kK0 << 2;    // dz = +1
constexpr uint32_t kJ0 = 0x01C0E07u;  // dy = -1
constexpr uint32_t kJ2 = kJ0 << 6;    // dy = +1

// The cells of the centre cube that other voxels share: 6 faces (1 voxel each), 12 edges (3), 8 vertices (7).
struct CubeCells {
    uint32_t face[6], edge[12], vert[8];
};
constexpr CubeCells make_cube_cells() {
    CubeCells c{};
    int f = 0, e = 0, v = 0;
    for (int s = -1; s <= 1; s += 2) {
        c.face[f++] = nb(s, 0, 0);
        c.face[f++] = nb(0, s, 0);
        c.face[f++] = nb(0, 0, s);
    }
    for (int a = -1; a <= 1; a += 2)
        for (int b = -1; b <= 1; b += 2) {
            c.edge[e++] = nb(a, 0, 0) | nb(0, b, 0) | nb(a, b, 0);
            c.edge[e++] = nb(a, 0, 0) | nb(0, 0, b) | nb(a, 0, b);
            c.edge[e++] = nb(0, a, 0) | nb(0, 0, b) | nb(0, a, b);
        }
    for (int a = -1; a <= 1; a += 2)
        for (int b = -1; b <= 1; b += 2)
            for (int d = -1; d <= 1; d += 2)
                c.vert[v++] = nb(a, 0, 0) | nb(0, b, 0) | nb(0, 0, d) | nb(a, b, 0) | nb(a, 0, d) | nb(0, b, d) |
                              nb(a, b, d);
    return c;
}

// Removing the centre leaves the Euler characteristic of the neighbourhood (foreground voxels as closed unit cubes)
// unchanged: chi drops by V - E + F - 1 over the centre cube's cells that no other foreground voxel covers.
__device__ __forceinline__ bool euler_invariant(uint32_t n) {
    constexpr CubeCells c = make_cube_cells();
    int d = -1;
#pragma unroll
    for (int i = 0; i < 6; ++i) d += (n & c.face[i]) == 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) d -= (n & c.edge[i]) == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += (n & c.vert[i]) == 0;
    return d == 0;
}

__device__ __forceinline__ uint32_t dilate26(uint32_t m) {
    m = (m | ((m << 1) & ~kK0) | ((m >> 1) & ~kK2)) & kFull;  // bits shifted past 26 must not come back
    m = (m | ((m << 3) & ~kJ0) | ((m >> 3) & ~kJ2)) & kFull;
    return (m | (m << 9) | (m >> 9)) & kFull;
}

// The foreground 26-neighbours (centre excluded) form at most one 26-connected component.
__device__ __forceinline__ bool is_simple(uint32_t n) {
    const uint32_t fg = n & kFull & ~kCentre;
    if (!fg) return true;
    uint32_t comp = fg & (0u - fg);
    for (int i = 0; i < 26; ++i) {  // a component of <= 26 voxels stops growing within 26 steps
        const uint32_t grown = dilate26(comp) & fg;
        if (grown == comp) break;
        comp = grown;
    }
    return comp == fg;
}

// Row (x, y) around word wz as 34 bits: bit 0 = voxel 32 wz - 1, bit b + 1 = voxel 32 wz + b, bit 33 = 32 wz + 32.
__device__ __forceinline__ uint64_t row_bits(const uint32_t* plane, int row, int wz, int WZ) {
    const uint32_t mid = plane[row + wz];
    const uint32_t lo = wz > 0 ? plane[row + wz - 1] : 0u;
    const uint32_t hi = wz + 1 < WZ ? plane[row + wz + 1] : 0u;
    return ((uint64_t)mid << 1) | (lo >> 31) | ((uint64_t)(hi & 1u) << 33);
}

// v[3 (dx + 1) + (dy + 1)] = row_bits of row (x + dx, y + dy): neighbourhood of bit b of the centre word
__device__ __forceinline__ uint32_t gather27(const uint64_t (&v)[9], int b) {
    uint32_t n = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) n |= (uint32_t)((v[r] >> b) & 7u) << (3 * r);
    return n;
}

template <bool kLds>
__device__ __forceinline__ void wg_barrier() {
    if (!kLds) __threadfence();  // the planes and lists live in global memory: make this wave's stores visible
    __syncthreads();
}

struct Counters {
    int n[2];        // entries of list 0 / list 1
    int nready[2];   // entries of the ready list, by round parity
    int ncand;       // candidates of the sub-iteration
    int changed;     // the sub-iteration deleted a voxel
    int total;       // skeleton voxels at the end
};

template <bool kLds>
__device__ void thin_object(const int* __restrict__ labels, int X, int Y, int Z, int id, const SkelObj& o,
                            uint32_t* planes, int W, uint32_t* result, int* count, int* stats, int* error,
                            Counters& s) {
    const int PY = o.cy + 2, PZ = o.cz + 2, WZ = (PZ + 31) >> 5;
    uint32_t* img = planes;
    uint32_t* pend = planes + W;
    int* list0 = (int*)(planes + 2 * W);
    int* list1 = (int*)(planes + 3 * W);
    int* rword = (int*)(planes + 4 * W);
    uint32_t* rbits = planes + 5 * W;
    const int tid = threadIdx.x;

    // binary crop [x0, x0 + cx) x [y0, y0 + cy) x [z0, z0 + cz) of `labels == id`, padded
    for (int w = tid; w < W; w += kThreads) {
        const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
        uint32_t bits = 0;
        if (x >= 1 && x <= o.cx && y >= 1 && y <= o.cy) {
            const int* src = labels + ((long long)(o.x0 + x - 1) * Y + (o.y0 + y - 1)) * Z + o.z0;
            const int zlo = max(32 * wz, 1), zhi = min(32 * wz + 31, o.cz);
            for (int z = zlo; z <= zhi; ++z) bits |= (uint32_t)(src[z - 1] == id) << (z - 32 * wz);
        }
        img[w] = bits;
        pend[w] = 0u;
    }
    const int pass_limit = o.cx * o.cy * o.cz + 1;
    int passes = 0, max_rounds = 0, failed = 0;
    for (;;) {
        if (passes >= pass_limit) {
            failed = 2;
            break;
        }
        ++passes;
        int unchanged = 0;
        for (int dir = 0; dir < 6 && !failed; ++dir) {
            wg_barrier<kLds>();
            if (tid == 0) {
                s.n[0] = s.n[1] = 0;
                s.nready[0] = s.nready[1] = 0;
                s.ncand = 0;
                s.changed = 0;
            }
            wg_barrier<kLds>();
            // candidates, judged on the image at the start of the sub-iteration
            // border directions in skimage's order 4, 3, 2, 1, 5, 6: y-1, y+1, z+1, z-1, x+1, x-1
            const int dx = dir == 4 ? 1 : dir == 5 ? -1 : 0;
            const int dy = dir == 0 ? -1 : dir == 1 ? 1 : 0;
            const int dz = dir == 2 ? 1 : dir == 3 ? -1 : 0;
            for (int w = tid; w < W; w += kThreads) {
                const uint32_t cur = img[w];
                if (!cur) continue;  // pad rows are all zero
                const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
                uint64_t v[9];
#pragma unroll
                for (int r = 0; r < 9; ++r) v[r] = row_bits(img, ((x + r / 3 - 1) * PY + (y + r % 3 - 1)) * WZ, wz, WZ);
                const uint64_t nrow = dx < 0 ? v[1] : dx > 0 ? v[7] : dy < 0 ? v[3] : dy > 0 ? v[5] : v[4];
                const uint32_t across = (uint32_t)(nrow >> (1 + dz));  // voxel p + d of every bit
                uint32_t border = cur & ~across;
                uint32_t cand = 0;
                while (border) {
                    const int b = __builtin_ctz(border);
                    border &= border - 1;
                    const uint32_t n = gather27(v, b);
                    if (__builtin_popcount(n & ~kCentre) == 1) continue;  // endpoint
                    if (!euler_invariant(n) || !is_simple(n)) continue;
                    cand |= 1u << b;
                }
                if (cand) {
                    pend[w] = cand;
                    list0[atomicAdd(&s.n[0], 1)] = w;
                    atomicAdd(&s.ncand, __builtin_popcount(cand));
                }
            }
            wg_barrier<kLds>();
            int nlist = s.n[0];
            const int ncand = s.ncand;
            int round = 0;
            while (nlist > 0) {
                if (round >= ncand) {  // impossible: every round decides the earliest pending candidate
                    failed = 1;
                    break;
                }
                const int cur = round & 1, nxt = cur ^ 1;
                const int* from = cur ? list1 : list0;
                int* to = cur ? list0 : list1;
                // ready = pending candidates none of whose 13 raster-preceding neighbours is pending
                for (int i = tid; i < nlist; i += kThreads) {
                    const int w = from[i];
                    const uint32_t p = pend[w];
                    const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
                    uint64_t blocked64 = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {  // rows (x-1, y-1), (x-1, y), (x-1, y+1), (x, y-1): z-1, z, z+1
                        const int rx = r < 3 ? x - 1 : x, ry = r < 3 ? y + r - 1 : y - 1;
                        const uint64_t q = row_bits(pend, (rx * PY + ry) * WZ, wz, WZ);
                        blocked64 |= q | (q >> 1) | (q >> 2);
                    }
                    blocked64 |= row_bits(pend, (x * PY + y) * WZ, wz, WZ);  // (x, y, z-1)
                    const uint32_t ready = p & ~(uint32_t)blocked64;
                    if (ready) {
                        const int j = atomicAdd(&s.nready[cur], 1);
                        rword[j] = w;
                        rbits[j] = ready;
                    }
                    if (p & ~ready) to[atomicAdd(&s.n[nxt], 1)] = w;
                }
                wg_barrier<kLds>();
                const int nready = s.nready[cur];
                const int nlist_next = s.n[nxt];
                if (tid == 0) {  // read last round (before its second barrier); written again next round
                    s.nready[nxt] = 0;
                    s.n[cur] = 0;
                }
                // decide the ready candidates on the current image; none of them is a neighbour of another
                for (int j = tid; j < nready; j += kThreads) {
                    const int w = rword[j];
                    const uint32_t ready = rbits[j];
                    const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
                    uint64_t v[9];
#pragma unroll
                    for (int r = 0; r < 9; ++r)
                        v[r] = row_bits(img, ((x + r / 3 - 1) * PY + (y + r % 3 - 1)) * WZ, wz, WZ);
                    uint32_t del = 0, rb = ready;
                    while (rb) {
                        const int b = __builtin_ctz(rb);
                        rb &= rb - 1;
                        if (is_simple(gather27(v, b))) del |= 1u << b;
                    }
                    if (del) {
                        img[w] = img[w] & ~del;  // the only writer of word w this round
                        s.changed = 1;
                    }
                    pend[w] = pend[w] & ~ready;
                }
                wg_barrier<kLds>();
                nlist = nlist_next;
                ++round;
            }
            max_rounds = max(max_rounds, round);
            if (failed) break;
            wg_barrier<kLds>();
            unchanged += s.changed == 0;
        }
        if (failed || unchanged == 6) break;
    }
    wg_barrier<kLds>();
    if (tid == 0) s.total = 0;
    wg_barrier<kLds>();
    int mine = 0;
    for (int w = tid; w < W; w += kThreads) {
        const uint32_t bits = img[w];
        if (kLds) result[w] = bits;
        mine += __builtin_popcount(bits);
    }
    if (mine) atomicAdd(&s.total, mine);
    wg_barrier<kLds>();
    if (tid == 0) {
        *count = s.total;
        stats[0] = passes;
        stats[1] = max_rounds;
        if (failed) atomicOr(error, failed);
    }
}

__global__ void __launch_bounds__(kThreads) thin_kernel(const int* __restrict__ labels, int X, int Y, int Z,
                                                        const int* __restrict__ ids, const SkelObj* __restrict__ objs,
                                                        uint32_t* __restrict__ work, int* __restrict__ counts,
                                                        int* __restrict__ stats, int* __restrict__ error) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_planes[];
    __shared__ Counters s;
    const int i = blockIdx.x;
    const SkelObj o = objs[i];
    const int W = (o.cx + 2) * (o.cy + 2) * ((o.cz + 2 + 31) >> 5);
    uint32_t* mine = work + o.off;
    if (o.lds)
        thin_object<true>(labels, X, Y, Z, ids[i], o, lds_planes, W, mine, counts + i, stats + 2 * i, error, s);
    else
        thin_object<false>(labels, X, Y, Z, ids[i], o, mine, W, mine, counts + i, stats + 2 * i, error, s);
}

// Skeleton voxels of object i, in raster order, as crop coordinates (x, y, z) at rows offsets[i] ..
__global__ void __launch_bounds__(kThreads) emit_kernel(const SkelObj* __restrict__ objs, const uint32_t* __restrict__ work,
                                                        const int* __restrict__ offsets, long long n_points,
                                                        int* __restrict__ points) {
    __shared__ int scan[kThreads];
    const int i = blockIdx.x, tid = threadIdx.x;
    const SkelObj o = objs[i];
    const int PY = o.cy + 2, WZ = (o.cz + 2 + 31) >> 5;
    const int W = (o.cx + 2) * PY * WZ;
    const uint32_t* img = work + o.off;
    const long long first = offsets[i], last = min((long long)offsets[i + 1], n_points);
    long long base = first;
    for (int w0 = 0; w0 < W; w0 += kThreads) {
        const int w = w0 + tid;
        uint32_t bits = w < W ? img[w] : 0u;
        const int c = __builtin_popcount(bits);
        scan[tid] = c;
        __syncthreads();
        for (int step = 1; step < kThreads; step <<= 1) {  // inclusive scan
            const int add = tid >= step ? scan[tid - step] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int total = scan[kThreads - 1];
        long long p = base + scan[tid] - c;
        if (bits) {
            const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
            while (bits) {
                const int b = __builtin_ctz(bits);
                bits &= bits - 1;
                if (p >= first && p < last) {
                    points[3 * p] = x - 1;
                    points[3 * p + 1] = y - 1;
                    points[3 * p + 2] = 32 * wz + b - 1;
                }
                ++p;
            }
        }
        base += total;
        __syncthreads();  // scan[] is rewritten by the next chunk
    }
}

// The skeleton of object i read as a graph: a link is an unordered pair of skeleton voxels that
// are 26-neighbours, the degree of a voxel the number of its links.  Row i of `graph`: voxels, voxels of degree 0, 1,
// 2 and >= 3, then the links by direction class (|dx|, |dy|, |dz|) in the order of kLinkClass.  A link is counted
// once, from the voxel that sees it among its 13 raster-following neighbours: bits 14 .. 26 of the neighbourhood code.
constexpr int kGraphValues = 12;
constexpr int kLinkClasses = 7;

struct LinkMasks {
    uint32_t m[kLinkClasses];
};
constexpr LinkMasks make_link_masks() {
    // (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), indexed by 4 |dx| + 2 |dy| + |dz|
    constexpr int kLinkClass[8] = {-1, 2, 1, 5, 0, 4, 3, 6};
    LinkMasks k{};
    for (int c = 14; c < 27; ++c) {
        const int dx = c / 9 - 1, dy = c / 3 % 3 - 1, dz = c % 3 - 1;
        k.m[kLinkClass[4 * (dx != 0) + 2 * (dy != 0) + (dz != 0)]] |= 1u << c;
    }
    return k;
}

__global__ void __launch_bounds__(kThreads) graph_kernel(const SkelObj* __restrict__ objs,
                                                         const uint32_t* __restrict__ work,
                                                         long long* __restrict__ graph) {
    constexpr LinkMasks kLink = make_link_masks();
    constexpr int kWaves = kThreads / 64;
    __shared__ long long part[kWaves][kGraphValues];
    const int i = blockIdx.x, tid = threadIdx.x;
    const SkelObj o = objs[i];
    const int PX = o.cx + 2, PY = o.cy + 2, WZ = (o.cz + 2 + 31) >> 5;
    const int W = PX * PY * WZ;
    const uint32_t* img = work + o.off;
    // 64-bit from the first addition on: a crop holds up to 2^30 voxels with 13 forward links each
    long long acc[kGraphValues];
#pragma unroll
    for (int k = 0; k < kGraphValues; ++k) acc[k] = 0;
    for (int w = tid; w < W; w += kThreads) {
        const uint32_t cur = img[w];
        if (!cur) continue;
        const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
        // the pad rows are zero after sk_skeletonize; a plane that is not its result must not send a read outside
        if (x < 1 || x > o.cx || y < 1 || y > o.cy) continue;
        uint64_t v[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) v[r] = row_bits(img, ((x + r / 3 - 1) * PY + (y + r % 3 - 1)) * WZ, wz, WZ);
        uint32_t bits = cur;
        while (bits) {
            const int b = __builtin_ctz(bits);
            bits &= bits - 1;
            const uint32_t n = gather27(v, b);
            const int degree = __builtin_popcount(n & ~kCentre);
            acc[0] += 1;
            acc[1] += degree == 0;
            acc[2] += degree == 1;
            acc[3] += degree == 2;
            acc[4] += degree >= 3;
#pragma unroll
            for (int k = 0; k < kLinkClasses; ++k) acc[5 + k] += __builtin_popcount(n & kLink.m[k]);
        }
    }
    // integer sums: wave shuffle, then one LDS row per wave, then one thread per column writes the row
#pragma unroll
    for (int k = 0; k < kGraphValues; ++k) {
        long long a = acc[k];
        for (int step = 32; step > 0; step >>= 1) a += __shfl_down(a, step, 64);
        if ((tid & 63) == 0) part[tid >> 6][k] = a;
    }
    __syncthreads();
    if (tid < kGraphValues) {
        long long a = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) a += part[wv][tid];
        graph[(long long)i * kGraphValues + tid] = a;
    }
}

// A given skeleton, packed into the workspace layout without thinning: plane 0 of object i, the
// crop of `labels == ids[i]` padded by one background voxel, where thin_kernel leaves its result in either mode.
__global__ void __launch_bounds__(kThreads) pack_kernel(const int* __restrict__ labels, int X, int Y, int Z,
                                                        const int* __restrict__ ids, const SkelObj* __restrict__ objs,
                                                        uint32_t* __restrict__ work, int* __restrict__ counts,
                                                        int* __restrict__ stats) {
    __shared__ int total;
    const int i = blockIdx.x, tid = threadIdx.x;
    const SkelObj o = objs[i];
    const int id = ids[i];
    const int PY = o.cy + 2, WZ = (o.cz + 2 + 31) >> 5;
    const int W = (o.cx + 2) * PY * WZ;
    uint32_t* img = work + o.off;
    if (tid == 0) total = 0;
    __syncthreads();
    int mine = 0;
    for (int w = tid; w < W; w += kThreads) {
        const int wz = w % WZ, t = w / WZ, y = t % PY, x = t / PY;
        uint32_t bits = 0;
        if (x >= 1 && x <= o.cx && y >= 1 && y <= o.cy) {
            const int* src = labels + ((long long)(o.x0 + x - 1) * Y + (o.y0 + y - 1)) * Z + o.z0;
            const int zlo = max(32 * wz, 1), zhi = min(32 * wz + 31, o.cz);
            for (int z = zlo; z <= zhi; ++z) bits |= (uint32_t)(src[z - 1] == id) << (z - 32 * wz);
        }
        img[w] = bits;
        mine += __builtin_popcount(bits);
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) {
        counts[i] = total;
        stats[2 * i] = stats[2 * i + 1] = 0;
    }
}

// The skeleton of object i traced into nodes and branches (include/skoots_hip.h states the
// definitions).  The n skeleton voxels are numbered p = 0 .. n - 1 in raster order of the crop, the order of
// emit_kernel and the lexicographic order of (x, y, z): a smaller p is an earlier voxel.  Everything per voxel lives in
// the object's slice of the scratch, kTraceInts int32 per voxel; all of it is written before it is read, in every call.
constexpr int kTraceInts = 11;
constexpr int kOwned = -2, kUnowned = -1, kAnchor = -3;  // states of a chain voxel in `label`

struct Trace {
    int* lin;      // (x cy + y) cz + z in crop coordinates, ascending in p
    int* code;     // 26 bits of the neighbourhood code: which neighbours are skeleton voxels
    int* nb2;      // of a chain voxel: the numbers of its two neighbours, lower direction code first
    int* label;    // junction voxel: smallest p of its 26-connected component; chain voxel: kUnowned / kOwned / kAnchor
    int* keep;     // direction codes of the branches kept from this end voxel
    int* nodeidx;  // 1 on the first voxel of a node, then its exclusive scan: the node's row within the object
    int* bidx;     // popcount(keep), then its exclusive scan: the row of the voxel's first branch within the object
    int* nvox;     // on a node's first voxel: its voxels, internal links and attached branch ends
    int* nint;
    int* nend;
    int n;
};

struct TraceShared {
    int changed, bad, total;
    int part[kThreads];
};

__device__ __forceinline__ int link_class(int c) {  // kLinkClass of make_link_masks, four bits per entry
    const int dx = c / 9 - 1, dy = c / 3 % 3 - 1, dz = c % 3 - 1;
    return (0x63405120u >> (4 * (4 * (dx != 0) + 2 * (dy != 0) + (dz != 0)))) & 7;
}

// the number of the voxel at `lin`, -1 if it is no skeleton voxel (a plane that is not a skeleton's)
__device__ __forceinline__ int find_voxel(const Trace& t, long long lin) {
    int lo = 0, hi = t.n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const long long v = t.lin[mid];
        if (v == lin) return mid;
        if (v < lin) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

__device__ __forceinline__ int neighbour(const Trace& t, const SkelObj& o, int p, int c) {
    // 64-bit: a crop of 1 x 1 x 2^30 voxels has neighbours whose index would leave int32
    return find_voxel(t, t.lin[p] + ((long long)(c / 9 - 1) * o.cy + (c / 3 % 3 - 1)) * o.cz + (c % 3 - 1));
}

__device__ __forceinline__ bool is_chain(const Trace& t, int p) { return __builtin_popcount(t.code[p]) == 2; }

// the first voxel of the node that node voxel v belongs to
__device__ __forceinline__ int node_of(const Trace& t, int v) { return t.label[v] >= 0 ? t.label[v] : v; }

struct Walk {
    int end, end_code, chain;
    int links[kLinkClasses];
};

// The branch that leaves end voxel p by direction code c: along chain voxels (each has exactly two neighbours, so no
// visited marks) to the next node voxel, or back to p.  kMark: chain voxels become kOwned; owner_row >= 0: they get it.
template <bool kMark>
__device__ bool walk_branch(const Trace& t, const SkelObj& o, int p, int c, int* owner, int owner_row, Walk& w) {
#pragma unroll
    for (int k = 0; k < kLinkClasses; ++k) w.links[k] = 0;
    w.chain = 0;
    int prev = p, cur = neighbour(t, o, p, c), dir = c;
    for (int steps = 0;; ++steps) {
        if (cur < 0 || steps > t.n) return false;
        const int cl = link_class(dir);
#pragma unroll
        for (int k = 0; k < kLinkClasses; ++k) w.links[k] += cl == k;
        if (cur == p || !is_chain(t, cur)) break;
        if (kMark) t.label[cur] = kOwned;
        if (owner_row >= 0) owner[cur] = owner_row;
        ++w.chain;
        const uint32_t code = t.code[cur];
        const bool first = t.nb2[2 * cur] != prev;
        dir = first ? __builtin_ctz(code) : 31 - __builtin_clz(code);
        const int next = t.nb2[2 * cur + (first ? 0 : 1)];
        prev = cur;
        cur = next;
    }
    w.end = cur;
    w.end_code = 26 - dir;  // the same link, seen from its other end
    return true;
}

// exclusive scan of a[0 .. n) in place by the workgroup; returns the total
__device__ int scan_exclusive(int* a, int n, TraceShared& s) {
    const int tid = threadIdx.x, seg = (n + kThreads - 1) / kThreads;
    const int lo = min(tid * seg, n), hi = min(lo + seg, n);
    int sum = 0;
    for (int k = lo; k < hi; ++k) sum += a[k];
    s.part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int k = 0; k < kThreads; ++k) {
            const int v = s.part[k];
            s.part[k] = run;
            run += v;
        }
        s.total = run;
    }
    __syncthreads();
    int run = s.part[tid];
    for (int k = lo; k < hi; ++k) {
        const int v = a[k];
        a[k] = run;
        run += v;
    }
    wg_barrier<false>();
    return s.total;
}

// kEmit = false: node_branch[2 i], [2 i + 1] = nodes and branches of object i, or -1, -1 when the plane does not hold
// offsets[i + 1] - offsets[i] voxels inside its crop.  kEmit = true: the rows, and the owner of every voxel.
template <bool kEmit>
__device__ void trace_object(const SkelObj* __restrict__ objs, const uint32_t* __restrict__ work,
                             const int* __restrict__ offsets, long long n_points, int* __restrict__ scratch,
                             int* __restrict__ node_branch, const int* __restrict__ node_offsets,
                             const int* __restrict__ branch_offsets, long long n_nodes, long long n_branches,
                             int* __restrict__ nodes, int* __restrict__ branches, int* __restrict__ owner,
                             TraceShared& s) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const SkelObj o = objs[i];
    const int PY = o.cy + 2, WZ = (o.cz + 2 + 31) >> 5;
    const int W = (o.cx + 2) * PY * WZ;
    const uint32_t* img = work + o.off;
    const long long first = offsets[i], last = offsets[i + 1];
    const bool sane = first >= 0 && last >= first && last <= n_points && last - first <= (long long)o.cx * o.cy * o.cz;
    const int n = sane ? (int)(last - first) : 0;
    Trace t;
    int* base = scratch + (sane ? first * kTraceInts : 0);
    t.lin = base, t.code = base + n, t.nb2 = base + 2 * (long long)n, t.label = base + 4 * (long long)n;
    t.keep = base + 5 * (long long)n, t.nodeidx = base + 6 * (long long)n, t.bidx = base + 7 * (long long)n;
    t.nvox = base + 8 * (long long)n, t.nint = base + 9 * (long long)n, t.nend = base + 10 * (long long)n;
    t.n = n;
    if (tid == 0) s.bad = !sane, s.total = 0;
    __syncthreads();

    // 1. number the voxels (the scan of emit_kernel) and read every one's neighbourhood
    int seen = 0;
    for (int w0 = 0; w0 < W; w0 += kThreads) {
        const int w = w0 + tid;
        const int wz = w % WZ, rest = w / WZ, y = rest % PY, x = rest / PY;
        // the pad rows are zero after sk_skeletonize; a plane that is not its result must not send a read outside
        const bool inside = w < W && x >= 1 && x <= o.cx && y >= 1 && y <= o.cy;
        uint32_t bits = inside ? img[w] : 0u;
        const int c = __builtin_popcount(bits);
        s.part[tid] = c;
        __syncthreads();
        for (int step = 1; step < kThreads; step <<= 1) {  // inclusive scan
            const int add = tid >= step ? s.part[tid - step] : 0;
            __syncthreads();
            s.part[tid] += add;
            __syncthreads();
        }
        const int chunk = s.part[kThreads - 1];
        int p = seen + s.part[tid] - c;
        if (bits) {
            uint64_t v[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) v[r] = row_bits(img, ((x + r / 3 - 1) * PY + (y + r % 3 - 1)) * WZ, wz, WZ);
            while (bits) {
                const int b = __builtin_ctz(bits);
                bits &= bits - 1;
                const int z = 32 * wz + b;  // padded
                if (z < 1 || z > o.cz) s.bad = 1;
                if (p < n) {
                    t.lin[p] = ((x - 1) * o.cy + (y - 1)) * o.cz + (z - 1);
                    t.code[p] = (int)(gather27(v, b) & kFull & ~kCentre);
                }
                ++p;
            }
        }
        seen += chunk;
        __syncthreads();  // part[] is rewritten by the next chunk
    }
    if (seen != n) s.bad = 1;
    wg_barrier<false>();
    if (s.bad) {
        if (!kEmit && tid == 0) node_branch[2 * i] = node_branch[2 * i + 1] = -1;
        return;
    }

    // 2. the two neighbours of every chain voxel; every junction voxel starts as its own component
    for (int p = tid; p < n; p += kThreads) {
        const uint32_t code = t.code[p];
        const int degree = __builtin_popcount(code);
        t.label[p] = degree >= 3 ? p : kUnowned;
        t.keep[p] = 0;
        t.nvox[p] = degree < 2;
        t.nint[p] = t.nend[p] = 0;
        t.nb2[2 * p] = t.nb2[2 * p + 1] = -1;
        if (degree == 2) {
            t.nb2[2 * p] = neighbour(t, o, p, __builtin_ctz(code));
            t.nb2[2 * p + 1] = neighbour(t, o, p, 31 - __builtin_clz(code));
            if (t.nb2[2 * p] < 0 || t.nb2[2 * p + 1] < 0) s.bad = 1;
        }
    }
    // 3. junctions: minimum propagation over the 26-neighbours of degree >= 3 to the workgroup-wide fixed point.  The
    // labels only fall, and every value a voxel can read is one of its own component: the fixed point, every voxel at
    // its component's smallest p, does not depend on the order of the reads and writes.
    for (;;) {
        wg_barrier<false>();
        if (tid == 0) s.changed = 0;
        wg_barrier<false>();
        if (s.bad) break;
        for (int p = tid; p < n; p += kThreads) {
            const int mine = t.label[p];
            if (mine < 0) continue;
            int m = mine;
            for (uint32_t code = t.code[p]; code; code &= code - 1) {
                const int q = neighbour(t, o, p, __builtin_ctz(code));
                if (q < 0) s.bad = 1;
                else if (t.label[q] >= 0) m = min(m, t.label[q]);
            }
            m = min(m, t.label[m]);  // and one jump along the labels: long components converge faster
            if (m < mine) {
                t.label[p] = m;
                s.changed = 1;
            }
        }
        wg_barrier<false>();
        if (!s.changed) break;
    }
    wg_barrier<false>();
    if (s.bad) {
        if (!kEmit && tid == 0) node_branch[2 * i] = node_branch[2 * i + 1] = -1;
        return;
    }

    // 4. from every node voxel along every link: internal links, and the branches, each kept from its canonical end
    for (int p = tid; p < n; p += kThreads) {
        const uint32_t code = t.code[p];
        const int degree = __builtin_popcount(code);
        if (degree >= 3) atomicAdd(&t.nvox[t.label[p]], 1);
        if (degree == 2 || degree == 0) continue;
        uint32_t keep = 0;
        for (uint32_t rest = code; rest; rest &= rest - 1) {
            const int c = __builtin_ctz(rest);
            Walk w;
            if (!walk_branch<true>(t, o, p, c, nullptr, -1, w)) {
                s.bad = 1;
                break;
            }
            const int e = w.end;
            if (w.chain == 0 && node_of(t, e) == node_of(t, p)) {  // two voxels of one junction
                if (p < e) atomicAdd(&t.nint[t.label[p]], 1);
                continue;
            }
            if (p < e || (p == e && c < w.end_code)) {
                keep |= 1u << c;
                atomicAdd(&t.nend[node_of(t, p)], 1);
                atomicAdd(&t.nend[node_of(t, e)], 1);
            }
        }
        t.keep[p] = (int)keep;
    }
    wg_barrier<false>();
    // 5. rings are what stays unowned: the first voxel of each is its anchor and carries its one branch
    for (int p = tid; p < n; p += kThreads) {
        if (!is_chain(t, p) || t.label[p] != kUnowned) continue;
        int smallest = p, prev = p, cur = t.nb2[2 * p];
        for (int steps = 0; cur != p; ++steps) {
            if (steps > n || !is_chain(t, cur)) {
                s.bad = 1;
                break;
            }
            smallest = min(smallest, cur);
            const int next = t.nb2[2 * cur + (t.nb2[2 * cur] == prev)];
            prev = cur;
            cur = next;
        }
        if (smallest == p) {  // no other thread reads or writes these four
            t.label[p] = kAnchor;
            t.keep[p] = 1 << __builtin_ctz(t.code[p]);
            t.nvox[p] = 1;
            t.nend[p] = 2;
        }
    }
    wg_barrier<false>();
    if (s.bad) {
        if (!kEmit && tid == 0) node_branch[2 * i] = node_branch[2 * i + 1] = -1;
        return;
    }
    // 6. rows within the object: nodes by first voxel, branches by (end voxel a, direction code at a)
    for (int p = tid; p < n; p += kThreads) {
        const int degree = __builtin_popcount(t.code[p]);
        t.nodeidx[p] = degree < 2 || t.label[p] == p || t.label[p] == kAnchor;
        t.bidx[p] = __builtin_popcount(t.keep[p]);
    }
    wg_barrier<false>();
    const int n_obj_nodes = scan_exclusive(t.nodeidx, n, s);
    const int n_obj_branches = scan_exclusive(t.bidx, n, s);
    if (!kEmit) {
        if (tid == 0) node_branch[2 * i] = n_obj_nodes, node_branch[2 * i + 1] = n_obj_branches;
        return;
    }
    const long long node0 = node_offsets[i], node1 = min((long long)node_offsets[i + 1], n_nodes);
    const long long branch0 = branch_offsets[i], branch1 = min((long long)branch_offsets[i + 1], n_branches);
    if (node0 < 0 || branch0 < 0) return;
    int* own = owner + first;
    for (int p = tid; p < n; p += kThreads) {
        const int degree = __builtin_popcount(t.code[p]);
        const bool node_voxel = degree != 2 || t.label[p] == kAnchor;
        if (node_voxel) own[p] = (int)(-1 - (node0 + t.nodeidx[node_of(t, p)]));
        const int lin = t.lin[p];
        if (node_voxel && node_of(t, p) == p) {
            const long long row = node0 + t.nodeidx[p];
            if (row < node1) {
                int* out = nodes + 8 * row;
                out[0] = i;
                out[1] = degree < 2 ? degree : degree == 2 ? 3 : 2;
                out[2] = t.nvox[p];
                out[3] = t.nint[p];
                out[4] = o.x0 + lin / (o.cy * o.cz);
                out[5] = o.y0 + lin / o.cz % o.cy;
                out[6] = o.z0 + lin % o.cz;
                out[7] = t.nend[p];
            }
        }
        long long row = branch0 + t.bidx[p];
        for (uint32_t rest = (uint32_t)t.keep[p]; rest; rest &= rest - 1, ++row) {
            const int c = __builtin_ctz(rest);
            Walk w;
            if (row >= branch1 || row >= (1LL << 31) || !walk_branch<false>(t, o, p, c, own, (int)row, w)) continue;
            const int e = t.lin[w.end];
            int* out = branches + 18 * row;
            out[0] = i;
            out[1] = (int)(node0 + t.nodeidx[node_of(t, p)]);
            out[2] = (int)(node0 + t.nodeidx[node_of(t, w.end)]);
            out[3] = w.chain;
#pragma unroll
            for (int k = 0; k < kLinkClasses; ++k) out[4 + k] = w.links[k];
            out[11] = o.x0 + lin / (o.cy * o.cz);
            out[12] = o.y0 + lin / o.cz % o.cy;
            out[13] = o.z0 + lin % o.cz;
            out[14] = o.x0 + e / (o.cy * o.cz);
            out[15] = o.y0 + e / o.cz % o.cy;
            out[16] = o.z0 + e % o.cz;
            out[17] = c;
        }
    }
}

__global__ void __launch_bounds__(kThreads) branches_count_kernel(const SkelObj* __restrict__ objs,
                                                                  const uint32_t* __restrict__ work,
                                                                  const int* __restrict__ offsets, long long n_points,
                                                                  int* __restrict__ scratch,
                                                                  int* __restrict__ node_branch) {
    __shared__ TraceShared s;
    trace_object<false>(objs, work, offsets, n_points, scratch, node_branch, nullptr, nullptr, 0, 0, nullptr, nullptr,
                        nullptr, s);
}

__global__ void __launch_bounds__(kThreads) branches_emit_kernel(const SkelObj* __restrict__ objs,
                                                                 const uint32_t* __restrict__ work,
                                                                 const int* __restrict__ offsets, long long n_points,
                                                                 int* __restrict__ scratch,
                                                                 const int* __restrict__ node_offsets,
                                                                 const int* __restrict__ branch_offsets,
                                                                 long long n_nodes, long long n_branches,
                                                                 int* __restrict__ nodes, int* __restrict__ branches,
                                                                 int* __restrict__ owner) {
    __shared__ TraceShared s;
    trace_object<true>(objs, work, offsets, n_points, scratch, nullptr, node_offsets, branch_offsets, n_nodes,
                       n_branches, nodes, branches, owner, s);
}

struct Layout {
    std::vector<SkelObj> objs;
    size_t table_bytes = 0;
    long long words = 0;
    int lds_bytes = 0;
};

// Validates the boxes and places every object: LDS when its six planes fit kLdsBytes, else the global workspace.
static int plan(const int32_t* boxes_host, int n, int X, int Y, int Z, Layout& L) {
    L.objs.resize(n);
    L.table_bytes = ((size_t)n * sizeof(SkelObj) + 255) & ~(size_t)255;
    long long words = 0;
    int lds = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* b = boxes_host + 6 * i;
        SK_CHECK_ARG(b[0] >= 0 && b[1] >= 0 && b[2] >= 0 && b[3] > b[0] && b[4] > b[1] && b[5] > b[2] &&
                         (X <= 0 || (b[3] <= X && b[4] <= Y && b[5] <= Z)),
                     "sk_skeletonize: box %d (%d, %d, %d)..(%d, %d, %d) is empty or outside the volume", i, b[0],
                     b[1], b[2], b[3], b[4], b[5]);
        SkelObj& o = L.objs[i];
        o.x0 = b[0], o.y0 = b[1], o.z0 = b[2];
        o.cx = b[3] - b[0], o.cy = b[4] - b[1], o.cz = b[5] - b[2];
        o.pad = 0;
        const long long w = (long long)(o.cx + 2) * (o.cy + 2) * ((o.cz + 2 + 31) >> 5);
        SK_CHECK_ARG(w * kPlanes < (1LL << 31) && (long long)o.cx * o.cy * o.cz < (1LL << 30),
                     "sk_skeletonize: crop %d of %d x %d x %d voxels is too large", i, o.cx, o.cy, o.cz);
        o.lds = w * kPlanes * 4 <= kLdsBytes;
        o.off = words;
        words += o.lds ? w : w * kPlanes;
        if (o.lds) lds = std::max(lds, (int)(w * kPlanes * 4));
    }
    L.words = words;
    L.lds_bytes = lds;
    return SK_OK;
}

}  // namespace

extern "C" {

size_t sk_skeletonize_workspace_bytes(const int32_t* boxes_host, int n) {
    Layout L;
    if (n <= 0 || !boxes_host || plan(boxes_host, n, 0, 0, 0, L) != SK_OK) return 0;
    return L.table_bytes + (size_t)L.words * 4;
}

int sk_skeletonize(const int32_t* labels, int X, int Y, int Z, const int32_t* ids, const int32_t* boxes_host, int n,
                   void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* stats, int32_t* error,
                   void* stream) {
    SK_CHECK_ARG(labels && ids && boxes_host && workspace && counts && stats && error && X > 0 && Y > 0 && Z > 0 && n > 0,
                 "sk_skeletonize: bad arguments");
    Layout L;
    const int rc = plan(boxes_host, n, X, Y, Z, L);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= L.table_bytes + (size_t)L.words * 4,
                 "sk_skeletonize: workspace of %zu bytes, %zu needed", workspace_bytes,
                 L.table_bytes + (size_t)L.words * 4);
    SK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "sk_skeletonize: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the table goes through pageable memory: wait for the copy before L.objs goes away
    SK_CHECK_HIP(hipMemcpyAsync(workspace, L.objs.data(), (size_t)n * sizeof(SkelObj), hipMemcpyHostToDevice, s));
    SK_CHECK_HIP(hipMemsetAsync(error, 0, sizeof(int32_t), s));
    if (L.lds_bytes > 0)
        SK_CHECK_HIP(hipFuncSetAttribute((const void*)thin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         L.lds_bytes));
    thin_kernel<<<n, kThreads, L.lds_bytes, s>>>(labels, X, Y, Z, ids, (const SkelObj*)workspace,
                                                 (uint32_t*)((char*)workspace + L.table_bytes), counts, stats, error);
    SK_CHECK_LAUNCH();
    SK_CHECK_HIP(hipStreamSynchronize(s));
    return SK_OK;
}

int sk_skeletonize_emit(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                        const int32_t* offsets, int64_t n_points, int32_t* points, void* stream) {
    SK_CHECK_ARG(boxes_host && workspace && offsets && n > 0 && n_points >= 0 && (points || n_points == 0),
                 "sk_skeletonize_emit: bad arguments");
    Layout L;
    const int rc = plan(boxes_host, n, 0, 0, 0, L);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= L.table_bytes + (size_t)L.words * 4,
                 "sk_skeletonize_emit: workspace of %zu bytes, %zu needed", workspace_bytes,
                 L.table_bytes + (size_t)L.words * 4);
    emit_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>((const SkelObj*)workspace,
                                                         (const uint32_t*)((const char*)workspace + L.table_bytes),
                                                         offsets, n_points, points);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_skeleton_graph_row_values(void) { return kGraphValues; }

int sk_skeleton_graph(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes, int64_t* graph,
                      void* stream) {
    SK_CHECK_ARG(boxes_host && workspace && graph && n > 0, "sk_skeleton_graph: bad arguments");
    Layout L;
    const int rc = plan(boxes_host, n, 0, 0, 0, L);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= L.table_bytes + (size_t)L.words * 4,
                 "sk_skeleton_graph: workspace of %zu bytes, %zu needed", workspace_bytes,
                 L.table_bytes + (size_t)L.words * 4);
    SK_CHECK_ARG(((uintptr_t)graph & 7) == 0, "sk_skeleton_graph: graph must be 8-byte aligned");
    graph_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>((const SkelObj*)workspace,
                                                          (const uint32_t*)((const char*)workspace + L.table_bytes),
                                                          (long long*)graph);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_skeleton_pack(const int32_t* labels, int X, int Y, int Z, const int32_t* ids, const int32_t* boxes_host, int n,
                     void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* stats, int32_t* error,
                     void* stream) {
    SK_CHECK_ARG(labels && ids && boxes_host && workspace && counts && stats && error && X > 0 && Y > 0 && Z > 0 && n > 0,
                 "sk_skeleton_pack: bad arguments");
    Layout L;
    const int rc = plan(boxes_host, n, X, Y, Z, L);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= L.table_bytes + (size_t)L.words * 4,
                 "sk_skeleton_pack: workspace of %zu bytes, %zu needed", workspace_bytes,
                 L.table_bytes + (size_t)L.words * 4);
    SK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "sk_skeleton_pack: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemcpyAsync(workspace, L.objs.data(), (size_t)n * sizeof(SkelObj), hipMemcpyHostToDevice, s));
    SK_CHECK_HIP(hipMemsetAsync(error, 0, sizeof(int32_t), s));
    pack_kernel<<<n, kThreads, 0, s>>>(labels, X, Y, Z, ids, (const SkelObj*)workspace,
                                       (uint32_t*)((char*)workspace + L.table_bytes), counts, stats);
    SK_CHECK_LAUNCH();
    SK_CHECK_HIP(hipStreamSynchronize(s));  // the table went through pageable memory, as in sk_skeletonize
    return SK_OK;
}

int sk_skeleton_nodes_row_values(void) { return 8; }
int sk_skeleton_branches_row_values(void) { return 18; }

size_t sk_skeleton_branches_scratch_bytes(const int32_t* boxes_host, const int32_t* counts_host, int n) {
    Layout L;
    if (n <= 0 || !boxes_host || !counts_host || plan(boxes_host, n, 0, 0, 0, L) != SK_OK) return 0;
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        const SkelObj& o = L.objs[i];
        if (counts_host[i] < 0 || counts_host[i] > (long long)o.cx * o.cy * o.cz) return 0;
        total += counts_host[i];
    }
    if (total >= (1LL << 31)) return 0;
    return 16 + (size_t)total * kTraceInts * sizeof(int32_t);
}

// the checks that the count and the emit pass share; on success L holds the layout
static int check_trace(const char* what, const int32_t* boxes_host, int n, const void* workspace,
                       size_t workspace_bytes, const int32_t* offsets, int64_t n_points, const void* scratch,
                       size_t scratch_bytes, Layout& L) {
    SK_CHECK_ARG(boxes_host && workspace && offsets && scratch && n > 0 && n_points >= 0 && n_points < (1LL << 31),
                 "%s: bad arguments", what);
    const int rc = plan(boxes_host, n, 0, 0, 0, L);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workspace_bytes >= L.table_bytes + (size_t)L.words * 4, "%s: workspace of %zu bytes, %zu needed", what,
                 workspace_bytes, L.table_bytes + (size_t)L.words * 4);
    SK_CHECK_ARG(scratch_bytes >= 16 + (size_t)n_points * kTraceInts * sizeof(int32_t),
                 "%s: scratch of %zu bytes, %zu needed for %lld points", what, scratch_bytes,
                 16 + (size_t)n_points * kTraceInts * sizeof(int32_t), (long long)n_points);
    SK_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)scratch & 3) == 0 && ((uintptr_t)offsets & 3) == 0,
                 "%s: workspace must be 16-byte aligned, scratch and offsets 4-byte aligned", what);
    return SK_OK;
}

int sk_skeleton_branches_count(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                               const int32_t* offsets, int64_t n_points, void* scratch, size_t scratch_bytes,
                               int32_t* node_branch_counts, void* stream) {
    SK_CHECK_ARG(node_branch_counts && ((uintptr_t)node_branch_counts & 3) == 0,
                 "sk_skeleton_branches_count: bad arguments");
    Layout L;
    const int rc = check_trace("sk_skeleton_branches_count", boxes_host, n, workspace, workspace_bytes, offsets,
                               n_points, scratch, scratch_bytes, L);
    if (rc != SK_OK) return rc;
    branches_count_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>(
        (const SkelObj*)workspace, (const uint32_t*)((const char*)workspace + L.table_bytes), offsets, n_points,
        (int*)scratch, node_branch_counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_skeleton_branches_emit(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                              const int32_t* offsets, int64_t n_points, void* scratch, size_t scratch_bytes,
                              const int32_t* node_offsets, const int32_t* branch_offsets, int64_t n_nodes,
                              int64_t n_branches, int32_t* nodes, int32_t* branches, int32_t* owner, void* stream) {
    SK_CHECK_ARG(node_offsets && branch_offsets && n_nodes >= 0 && n_branches >= 0 && n_nodes < (1LL << 31) &&
                     n_branches < (1LL << 31) && (nodes || n_nodes == 0) && (branches || n_branches == 0) &&
                     (owner || n_points == 0),
                 "sk_skeleton_branches_emit: bad arguments");
    SK_CHECK_ARG((((uintptr_t)node_offsets | (uintptr_t)branch_offsets | (uintptr_t)nodes | (uintptr_t)branches |
                   (uintptr_t)owner) & 3) == 0,
                 "sk_skeleton_branches_emit: the tables and offsets must be 4-byte aligned");
    Layout L;
    const int rc = check_trace("sk_skeleton_branches_emit", boxes_host, n, workspace, workspace_bytes, offsets,
                               n_points, scratch, scratch_bytes, L);
    if (rc != SK_OK) return rc;
    branches_emit_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>(
        (const SkelObj*)workspace, (const uint32_t*)((const char*)workspace + L.table_bytes), offsets, n_points,
        (int*)scratch, node_offsets, branch_offsets, n_nodes, n_branches, nodes, branches, owner);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
