// skoots/utils/flood_and_stitch.py on the device: the two voxel passes of watershed_and_stitch.
//
// Replaces (reference file:line)
//   flood_and_stitch.py:63-69    scipy.ndimage.label on every slice            -> sk_label_planes
//   flood_and_stitch.py:93-101   np.unique(slice_b[slice_a == u], counts)      -> sk_plane_overlaps (all u, all slices, once)
// The greedy walk between them (:74-128) needs no voxel and runs on the host: stitch_host.cpp.
//
// sk_label_planes labels P planes of H x W in one launch sequence, 4-connected, every plane on its own:
//   1. tiles     a workgroup labels a 16 x 64 tile in LDS (union by minimum index, atomicMin on LDS) and writes every
//                voxel's parent as the global index of its tile-local root;
//   2. borders   one thread per voxel on a tile's left column or top row unites it with its neighbour across the border
//                (lock-free atomicMin union in global memory; a run along a border is united once, at its start);
//   3. flatten   every foreground voxel points at its root; roots are counted per 2048-voxel chunk of a plane;
//   4. scan      one workgroup: exclusive prefix of the chunk counts, the per-plane offsets and the total;
//   5. rank      roots get 1 + their rank in (plane, row, column) order;  6. write  labels through the output strides.
// A root is the minimum index of its component, i.e. its first voxel in raster order, and planes follow each other in
// the index, so the rank IS the global id of the contract and, inside a plane, scipy's number.  No workgroup waits for
// another: every loop follows parents towards a strictly smaller index or retries an atomicMin that lowered one.
#include "common.h"

namespace {

constexpr int kTW = 64, kTH = 16;   // tile: one wave per row group, lanes along W
constexpr int kChunk = 2048;        // voxels of one plane per block in the count / rank passes
constexpr int kMaxBlocks = 1 << 22; // tiles, and chunks, of one call (256 x 1024 x 1024: 2^18 tiles, 2^17 chunks)
constexpr int kMaxProbe = 128;      // slots an insertion looks at before it reports the table full

struct Geo {
    int P, H, W;
    long long isp, ish, isw;   // element strides of the uint8 input
    long long osp, osh, osw;   // element strides of the int32 labels
    int ntx, nty, cpp;         // tiles per row / column, chunks per plane
};

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

__global__ void __launch_bounds__(256) label_tiles_kernel(const uint8_t* __restrict__ src, int* __restrict__ parent, Geo g) {
    __shared__ int lab[kTH * kTW];
    const int tx = blockIdx.x % g.ntx, ty = (blockIdx.x / g.ntx) % g.nty, p = blockIdx.x / (g.ntx * g.nty);
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    const int x = tx * kTW + lx;
    const long long in0 = (long long)p * g.isp + (long long)x * g.isw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, y = ty * kTH + ly, l = ly * kTW + lx;
        const bool fg = x < g.W && y < g.H && src[in0 + (long long)y * g.ish] != 0;
        lab[l] = fg ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, l = ly * kTW + lx;
        if (lab[l] < 0) continue;   // the sign of an entry never changes
        if (lx > 0 && lab[l - 1] >= 0) unite(lab, l, l - 1);
        if (ly > 0 && lab[l - kTW] >= 0) unite(lab, l, l - kTW);
    }
    __syncthreads();
    const int base = p * g.H * g.W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, y = ty * kTH + ly, l = ly * kTW + lx;
        if (x >= g.W || y >= g.H) continue;
        int out = -1;
        if (lab[l] >= 0) {
            const int r = find_root(lab, l);   // nothing writes lab any more
            out = base + (ty * kTH + (r >> 6)) * g.W + tx * kTW + (r & 63);
        }
        parent[base + y * g.W + x] = out;
    }
}

__global__ void __launch_bounds__(256) merge_borders_kernel(int* __restrict__ parent, Geo g) {
    const long long nv = (long long)g.P * g.H * (g.ntx - 1), nh = (long long)g.P * (g.nty - 1) * g.W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int hw = g.H * g.W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nv + nh; e += stride) {
        if (e < nv) {   // left column of a tile against the column before it
            const int x = ((int)(e % (g.ntx - 1)) + 1) * kTW;
            const long long q = e / (g.ntx - 1);
            const int y = (int)(q % g.H), p = (int)(q / g.H);
            const int i = p * hw + y * g.W + x;
            if (parent[i] < 0 || parent[i - 1] < 0) continue;
            // the pair above, in the same two tiles, is foreground too: it is united with this one inside the tiles
            if (y % kTH != 0 && parent[i - g.W] >= 0 && parent[i - g.W - 1] >= 0) continue;
            unite(parent, i, i - 1);
        } else {        // top row of a tile against the row before it
            const long long f = e - nv;
            const int x = (int)(f % g.W);
            const long long q = f / g.W;
            const int y = ((int)(q % (g.nty - 1)) + 1) * kTH, p = (int)(q / (g.nty - 1));
            const int i = p * hw + y * g.W + x;
            if (parent[i] < 0 || parent[i - g.W] < 0) continue;
            if (x % kTW != 0 && parent[i - 1] >= 0 && parent[i - g.W - 1] >= 0) continue;
            unite(parent, i, i - g.W);
        }
    }
}

// block = one chunk of one plane.  Roots do not change here, so reading an ancestor that another thread is compressing
// still leads to the root.
__global__ void __launch_bounds__(256) flatten_count_kernel(int* __restrict__ parent, Geo g, int* __restrict__ chunk_count) {
    __shared__ int wsum[4];
    const int hw = g.H * g.W, p = blockIdx.x / g.cpp, q0 = (blockIdx.x % g.cpp) * kChunk;
    int c = 0;
    for (int k = threadIdx.x; k < kChunk; k += 256) {
        const int q = q0 + k;
        if (q >= hw) break;
        const int i = p * hw + q;
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

// one workgroup: chunk counts -> exclusive prefix (in place), offsets[p] = components before plane p, *total
__global__ void __launch_bounds__(1024) scan_chunks_kernel(int* __restrict__ chunk, int nchunks, int cpp, int P,
                                                           int32_t* __restrict__ offsets, int32_t* __restrict__ total) {
    __shared__ int part[1024];
    const int per = (nchunks + 1023) / 1024;
    const int lo = min(nchunks, (int)threadIdx.x * per), hi = min(nchunks, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += chunk[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int t = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int k = lo; k < hi; ++k) {
        const int v = chunk[k];
        chunk[k] = run;
        run += v;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += 1024) offsets[p] = chunk[p * cpp];
    if (threadIdx.x == 0) {
        offsets[P] = part[1023];
        *total = part[1023];
    }
}

// parent[root] = -(id) - 2, id = 1 + rank of the root in (plane, row, column) order
__global__ void __launch_bounds__(256) rank_roots_kernel(int* __restrict__ parent, Geo g, const int* __restrict__ chunk_offset) {
    __shared__ int wpre[4];
    const int hw = g.H * g.W, p = blockIdx.x / g.cpp, q0 = (blockIdx.x % g.cpp) * kChunk;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int run = chunk_offset[blockIdx.x];
    for (int k = 0; k < kChunk; k += 256) {   // rounds of 256 consecutive voxels keep raster order
        const int q = q0 + k + threadIdx.x;
        const int i = p * hw + q;
        const bool root = q < hw && parent[i] == i;
        const unsigned long long bal = __ballot(root);
        if (lane == 0) wpre[wv] = __popcll(bal);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wpre[w];
        const int tot = wpre[0] + wpre[1] + wpre[2] + wpre[3];
        if (root) parent[i] = -(run + before + __popcll(bal & ((1ull << lane) - 1ull)) + 1) - 2;
        run += tot;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) write_labels_kernel(const int* __restrict__ parent, int32_t* __restrict__ labels, Geo g) {
    const int hw = g.H * g.W, n = g.P * hw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int i = (int)e, p = i / hw, q = i - p * hw, y = q / g.W, x = q - y * g.W;
        int v = parent[i], lab = 0;
        if (v != -1) {
            if (v >= 0) v = parent[v];   // flattened: v is the root, whose slot holds the code
            lab = -(v + 2);
        }
        labels[(long long)p * g.osp + (long long)y * g.osh + (long long)x * g.osw] = lab;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// sk_plane_overlaps: counts of (id in plane p, id in plane p + 1) over all voxel positions, all plane pairs in one launch.
// key = id_a << 32 | id_b (never 0) in an open-addressing table; a wave first merges the equal keys of neighbouring
// lanes, so a run of one key costs one atomicAdd of its length.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// slot of `key`, inserting it if absent; -1 when the kMaxProbe slots from its home hold other keys (they always will:
// a slot never empties, so a key is either stored for the whole launch or refused for the whole launch)
__device__ __forceinline__ int table_slot(unsigned long long* keys, int cap, unsigned long long key, unsigned* counters) {
    int s = (int)(mix64(key) % (unsigned long long)cap);
    const int probes = cap < kMaxProbe ? cap : kMaxProbe;
    for (int j = 0; j < probes; ++j) {
        unsigned long long cur = __atomic_load_n(keys + s, __ATOMIC_RELAXED);
        if (cur == 0) {
            cur = atomicCAS(keys + s, 0ULL, key);
            if (cur == 0) {
                atomicAdd(&counters[0], 1u);
                return s;
            }
        }
        if (cur == key) return s;
        s = s + 1 == cap ? 0 : s + 1;
    }
    return -1;
}

__device__ __forceinline__ unsigned long long pair_key(const int32_t* __restrict__ labels, long long o, long long sp) {
    const int a = labels[o], b = labels[o + sp];
    return (a > 0 && b > 0) ? ((unsigned long long)(unsigned)a << 32) | (unsigned)b : 0ULL;
}

__global__ void __launch_bounds__(256) plane_overlaps_kernel(const int32_t* __restrict__ labels, int P, int H, int W, long long sp,
                                                             long long sh, long long sw, unsigned long long* __restrict__ keys,
                                                             int* __restrict__ hits, int cap, unsigned* __restrict__ counters) {
    const long long n = (long long)(P - 1) * H * W, stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63, hw = H * W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e - lane < n; e += stride) {   // whole waves iterate
        unsigned long long key = 0;
        int y = 0, x = 0;
        long long o = 0;
        if (e < n) {
            const int p = (int)(e / hw), q = (int)(e - (long long)p * hw);
            y = q / W;
            x = q - y * W;
            o = (long long)p * sp + (long long)y * sh + (long long)x * sw;
            key = pair_key(labels, o, sp);
        }
        const unsigned long long nonzero = __ballot(key != 0);
        if (nonzero == 0) continue;
        const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
        const unsigned plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
        const bool head = key != 0 && (lane == 0 || plo != klo || phi != khi);
        const unsigned long long heads = __ballot(head);
        // the run ends before the next lane that starts a run or holds no pair
        const unsigned long long above = (heads | ~nonzero) & ~((2ull << lane) - 1ull);
        const int len = above ? (__ffsll((long long)above) - 1 - lane) : 64 - lane;
        int refused = 0;
        if (head) {
            const int s = table_slot(keys, cap, key, counters);
            if (s >= 0)
                atomicAdd(&hits[s], len);
            else
                refused = 1;
        }
        // a refused key is counted once per top-left corner of its region (no such voxel to the left nor above): every
        // refused key has at least one, so stored + corners is never less than the number of distinct keys
        const unsigned long long mine = heads & ((2ull << lane) - 1ull);
        const int head_lane = (key != 0 && mine) ? 63 - __clzll((long long)mine) : lane;
        const bool lost = __shfl(refused, head_lane) != 0 && key != 0;
        bool corner = false;
        if (lost) corner = (x == 0 || pair_key(labels, o - sw, sp) != key) && (y == 0 || pair_key(labels, o - sh, sp) != key);
        const unsigned long long corners = __ballot(corner);
        if (lane == 0 && corners) atomicAdd(&counters[1], (unsigned)__popcll(corners));
    }
}

__global__ void __launch_bounds__(256) compact_rows_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ hits,
                                                           int cap, int32_t* __restrict__ rows, unsigned* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s - lane < cap; s += stride) {
        const unsigned long long k = s < cap ? keys[s] : 0ULL;
        const unsigned long long bal = __ballot(k != 0);
        if (bal == 0) continue;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&counters[2], (unsigned)__popcll(bal));
        base = __shfl(base, 0);
        if (k != 0) {
            const long long r = (long long)base + __popcll(bal & ((1ull << lane) - 1ull));   // < cap: one row per slot
            rows[3 * r] = (int32_t)(k >> 32);
            rows[3 * r + 1] = (int32_t)(k & 0xffffffffULL);
            rows[3 * r + 2] = hits[s];
        }
    }
}

bool make_geo(Geo& g, int P, int H, int W) {
    if (P <= 0 || H <= 0 || W <= 0) return false;
    const long long n = (long long)P * H * W;
    if (n > 0x7fffffffLL - 2 * kChunk) return false;
    g.P = P;
    g.H = H;
    g.W = W;
    g.ntx = (W + kTW - 1) / kTW;
    g.nty = (H + kTH - 1) / kTH;
    g.cpp = (H * W + kChunk - 1) / kChunk;
    // one workgroup per tile and per chunk: very many very small planes would pass the grid limit (and make the
    // one-workgroup scan long) with few voxels to show for it
    if ((long long)P * g.ntx * g.nty > kMaxBlocks || (long long)P * g.cpp > kMaxBlocks) return false;
    return true;
}

}  // namespace

extern "C" {

size_t sk_label_planes_workspace_bytes(int P, int H, int W) {
    Geo g;
    if (!make_geo(g, P, H, W)) return 0;
    return ((size_t)P * H * W + (size_t)P * g.cpp + 16) * sizeof(int);
}

int sk_label_planes(const uint8_t* mask, int P, int H, int W, int64_t in_sp, int64_t in_sh, int64_t in_sw, int32_t* labels,
                    int64_t out_sp, int64_t out_sh, int64_t out_sw, int32_t* offsets, int32_t* total, void* workspace,
                    size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Geo g;
    SK_CHECK_ARG(make_geo(g, P, H, W), "sk_label_planes: %d planes of %d x %d: extents must be positive, P H W < 2^31 - 4096, and at most 2^22 tiles of 16 x 64 and chunks of 2048 voxels per plane", P, H, W);
    SK_CHECK_ARG(mask && labels && offsets && total && workspace, "sk_label_planes: NULL pointer");
    SK_CHECK_ARG(in_sp > 0 && in_sh > 0 && in_sw > 0 && out_sp > 0 && out_sh > 0 && out_sw > 0, "sk_label_planes: strides must be positive");
    SK_CHECK_ARG(workspace_bytes >= sk_label_planes_workspace_bytes(P, H, W), "sk_label_planes: workspace too small (%zu < %zu)",
                 workspace_bytes, sk_label_planes_workspace_bytes(P, H, W));
    g.isp = in_sp; g.ish = in_sh; g.isw = in_sw;
    g.osp = out_sp; g.osh = out_sh; g.osw = out_sw;
    const long long n = (long long)P * H * W;
    int* parent = (int*)workspace;
    int* chunk = parent + n;
    const int nchunks = P * g.cpp;
    label_tiles_kernel<<<(unsigned)((long long)P * g.ntx * g.nty), 256, 0, stream>>>(mask, parent, g);
    const long long borders = (long long)P * H * (g.ntx - 1) + (long long)P * (g.nty - 1) * W;
    if (borders > 0) merge_borders_kernel<<<sk::stream_grid(borders, 256), 256, 0, stream>>>(parent, g);
    flatten_count_kernel<<<nchunks, 256, 0, stream>>>(parent, g, chunk);
    scan_chunks_kernel<<<1, 1024, 0, stream>>>(chunk, nchunks, g.cpp, P, offsets, total);
    rank_roots_kernel<<<nchunks, 256, 0, stream>>>(parent, g, chunk);
    write_labels_kernel<<<sk::stream_grid(n, 256), 256, 0, stream>>>(parent, labels, g);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

size_t sk_plane_overlaps_workspace_bytes(int capacity) {
    return capacity > 0 ? (size_t)capacity * (sizeof(unsigned long long) + sizeof(int)) : 0;
}

int sk_plane_overlaps(const int32_t* labels, int P, int H, int W, int64_t sp, int64_t sh, int64_t sw, int32_t* rows, int capacity,
                      uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SK_CHECK_ARG(labels && rows && counts && workspace, "sk_plane_overlaps: NULL pointer");
    Geo g;
    SK_CHECK_ARG(make_geo(g, P, H, W), "sk_plane_overlaps: %d planes of %d x %d: extents must be positive, P H W < 2^31 - 4096, and at most 2^22 tiles of 16 x 64 and chunks of 2048 voxels per plane", P, H, W);
    SK_CHECK_ARG(sp > 0 && sh > 0 && sw > 0, "sk_plane_overlaps: strides must be positive");
    SK_CHECK_ARG(capacity > 0 && capacity <= 0x7fffffff / 3, "sk_plane_overlaps: capacity %d out of range", capacity);
    SK_CHECK_ARG(workspace_bytes >= sk_plane_overlaps_workspace_bytes(capacity), "sk_plane_overlaps: workspace too small (%zu < %zu)",
                 workspace_bytes, sk_plane_overlaps_workspace_bytes(capacity));
    SK_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "sk_plane_overlaps: workspace must be 8-byte aligned");
    unsigned long long* keys = (unsigned long long*)workspace;
    int* hits = (int*)(keys + capacity);
    SK_CHECK_HIP(hipMemsetAsync(workspace, 0, sk_plane_overlaps_workspace_bytes(capacity), stream));
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), stream));
    const long long n = (long long)(P - 1) * H * W;
    if (n == 0) return SK_OK;
    plane_overlaps_kernel<<<sk::stream_grid(n, 256), 256, 0, stream>>>(labels, P, H, W, sp, sh, sw, keys, hits, capacity, counts);
    compact_rows_kernel<<<sk::stream_grid(capacity, 256), 256, 0, stream>>>(keys, hits, capacity, rows, counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
