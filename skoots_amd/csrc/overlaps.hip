// Which instance of one mask lies in which instance of another: for two label volumes of one
// shape, each with its own (lut, max_id, N) header, one row `ra, rb, voxels` per pair of rows that share a voxel -- the
// nonzero entries of the (N + 1) x (M + 1) contingency table of sk_mask_iou, without the table.  The reference declares
// the consumer (skoots/validate/lib.py: sparse_mask_iou) and raises NotImplementedError in it.
//
// Shape of the kernel
//   * The count is geometry-free: the volumes are one line of n = X Y Z voxels.  A workgroup takes a chunk of kChunk
//     consecutive voxels at a time; a lane reads 4 consecutive voxels of both volumes with one 16-byte load each, all
//     loads of the chunk issued before the first is used.  Up to 3 voxels in front of the first 16-byte boundary of `a`
//     are read one by one by the first workgroup, and the tail of the line by scalar loads with a bound; two pointers
//     that do not reach a 16-byte boundary at the same voxel are read by scalar loads throughout.
//   * A voxel is booked under key = ra << 32 | rb (0: nothing to book -- both background, or one of them without
//     `background`).  A wave-load is 256 consecutive voxels, 4 per lane in lane order; every position where the key
//     changes is the head of a run, found inside the lane by comparison and across lanes with one shuffle of the previous
//     lane's last key; the run's length is the distance to the next head (one ballot, one shuffle).  The head adds the
//     length to a table of kSlots keys in LDS (open addressing, at most kProbes probes, LDS integer atomics).  Inside an
//     object a whole wave-load is one run; a wave-load of background does nothing.
//   * The chunk flushes its table once into the global table: slots claimed with a 64-bit compare-and-swap on the key,
//     open addressing with at most kMaxProbe probes, counts added with 64-bit atomic adds.  A slot never empties, so a
//     key is either stored for the whole launch or refused for the whole launch; a refusal adds 1 to counts[1] and
//     writes nothing else.  A run whose key finds no LDS slot goes to the global table directly.
//   * A second kernel compacts the used slots into rows.  Integer atomics only, no loop without a bound, no workgroup
//     waits for another: the counts are exact and the set of rows is the same on every run.
// mix64, table_slot and the compaction are those of contacts.hip, kept twice so that this pass leaves that file's
// machine code alone; a shared header is the next "one copy" clean-up.
#include "instance_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;                            // voxels of one 16-byte load
constexpr int kLoads = 4;                              // 16-byte loads per lane, volume and chunk
constexpr int kStep = kThreads * kPerLane;             // voxels the workgroup reads per load
constexpr int kChunk = kStep * kLoads;                 // 4096 voxels between two flushes
constexpr int kSlotBits = 8, kSlots = 1 << kSlotBits;  // pairs the LDS table holds per chunk; one slot per thread in the flush
constexpr int kProbes = 8;                             // linear probes before a run goes to global memory
constexpr int kRow = 3;
constexpr int kMaxProbe = 128;                         // slots a global insertion looks at before it reports the table full
constexpr long long kMaxCapacity = 1ll << 40;

static_assert(kSlots == kThreads, "the flush gives every thread one slot");

typedef unsigned long long u64;

__device__ __forceinline__ u64 mix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// slot of `key` in the global table, inserting it if absent; -1 when the kMaxProbe slots from its home hold other keys
// (they always will: a slot never empties, so a key is either stored for the whole launch or refused for the whole launch)
__device__ __forceinline__ long long table_slot(u64* keys, long long cap, u64 key) {
    long long s = (long long)(mix64(key) & (u64)(cap - 1));
    const int probes = cap < kMaxProbe ? (int)cap : kMaxProbe;
    for (int j = 0; j < probes; ++j) {
        u64 cur = __atomic_load_n(keys + s, __ATOMIC_RELAXED);
        if (cur == 0) cur = atomicCAS(keys + s, 0ULL, key);
        if (cur == 0 || cur == key) return s;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

// slot of `key` in the chunk's table, or -1 when kProbes probes found neither the key nor a free slot
__device__ __forceinline__ int lds_slot(u64* s_key, u64 key) {
    const unsigned h = (unsigned)(mix64(key) >> (64 - kSlotBits));
    for (int p = 0; p < kProbes; ++p) {
        const int s = (int)((h + p) & (kSlots - 1));
        u64 k = ((volatile u64*)s_key)[s];                 // a key never changes once set within a chunk
        if (k == 0) k = atomicCAS(&s_key[s], 0ULL, key);
        if (k == 0 || k == key) return s;
    }
    return -1;
}

struct Tables {
    u64* s_key;
    unsigned* s_cnt;
    u64* keys;
    u64* hits;
    long long cap;
    u64* counts;
};

struct Side {
    const int* lab;                                        // NULL: a side without instances, all background
    const int* lut;
    int max_id, N;
};

// adds `len` voxels to `key`: the chunk's table, or the global one when the chunk's has no slot for it
__device__ __forceinline__ void add_run(const Tables& t, u64 key, unsigned len) {
    const int s = lds_slot(t.s_key, key);
    if (s >= 0) {
        atomicAdd(&t.s_cnt[s], len);
    } else {
        const long long g = table_slot(t.keys, t.cap, key);
        if (g >= 0)
            atomicAdd(&t.hits[g], (u64)len);
        else
            atomicAdd(&t.counts[1], 1ull);
    }
}

// Books the 4 consecutive keys of every lane, lanes in voxel order.  Called by whole waves.
__device__ __forceinline__ void book(const Tables& t, const u64 (&k)[kPerLane], int lane) {
    if (__ballot((k[0] | k[1] | k[2] | k[3]) != 0) == 0) return;      // wave-uniform: background only
    const unsigned plo = __shfl_up((unsigned)k[kPerLane - 1], 1), phi = __shfl_up((unsigned)(k[kPerLane - 1] >> 32), 1);
    const u64 prev = ((u64)phi << 32) | plo;
    unsigned heads = (lane == 0 || prev != k[0]) ? 1u : 0u;           // bit j: the key changes at voxel j of the lane
#pragma unroll
    for (int j = 1; j < kPerLane; ++j) heads |= (k[j] != k[j - 1]) ? (1u << j) : 0u;
    // the first head behind this lane: the lane that has one, and the voxel in it
    const u64 lanes = __ballot(heads != 0);
    const u64 above = lane < 63 ? lanes & ~((2ull << lane) - 1ull) : 0ull;
    const int next_lane = above ? __ffsll((long long)above) - 1 : 64;
    const unsigned next_heads = __shfl(heads, next_lane & 63);
    const int next_pos = above ? next_lane * kPerLane + (__ffs((int)next_heads) - 1) : 64 * kPerLane;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        if (!((heads >> j) & 1u) || k[j] == 0) continue;
        const unsigned later = heads >> (j + 1);
        const int end = later ? j + __ffs((int)later) : next_pos - lane * kPerLane;   // within the lane, or beyond it
        add_run(t, k[j], (unsigned)(end - j));
    }
}

__device__ __forceinline__ u64 key_of(int va, int vb, const Side& A, const Side& B, int background) {
    const unsigned ra = (unsigned)sk::row_of(va, A.lut, A.max_id, A.N), rb = (unsigned)sk::row_of(vb, B.lut, B.max_id, B.N);
    return (background ? (ra | rb) != 0 : (ra != 0 && rb != 0)) ? ((u64)ra << 32) | rb : 0ULL;
}

// `head` voxels in front of the body are the first workgroup's; the body starts at a 16-byte boundary of both volumes
// when `wide` says so
__global__ void __launch_bounds__(kThreads) overlaps_kernel(Side A, Side B, long long n, int head, int wide, int background,
                                                            long long nchunks, u64* __restrict__ keys,
                                                            u64* __restrict__ hits, long long cap,
                                                            u64* __restrict__ counts) {
    __shared__ u64 s_key[kSlots];
    __shared__ unsigned s_cnt[kSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    const Tables t = {s_key, s_cnt, keys, hits, cap, counts};
    s_key[tid] = 0;                                        // the flush leaves the table empty again: cleared once
    s_cnt[tid] = 0;
    __syncthreads();
    const int* __restrict__ pa = A.lab ? A.lab + head : nullptr;
    const int* __restrict__ pb = B.lab ? B.lab + head : nullptr;
    const long long body = n - head;
    if (blockIdx.x == 0 && tid < 64) {                     // the first wave: the voxels in front of the body
        u64 k[kPerLane] = {0, 0, 0, 0};
        if (lane < head) k[0] = key_of(A.lab ? A.lab[lane] : 0, B.lab ? B.lab[lane] : 0, A, B, background);
        book(t, k, lane);
    }
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long base = chunk * kChunk + (long long)tid * kPerLane;
        int va[kLoads][kPerLane], vb[kLoads][kPerLane];
#pragma unroll
        for (int l = 0; l < kLoads; ++l) {
            const long long p = base + (long long)l * kStep;
            if (wide && p + kPerLane <= body) {
                const int4 qa = pa ? *reinterpret_cast<const int4*>(pa + p) : make_int4(0, 0, 0, 0);
                const int4 qb = pb ? *reinterpret_cast<const int4*>(pb + p) : make_int4(0, 0, 0, 0);
                va[l][0] = qa.x, va[l][1] = qa.y, va[l][2] = qa.z, va[l][3] = qa.w;
                vb[l][0] = qb.x, vb[l][1] = qb.y, vb[l][2] = qb.z, vb[l][3] = qb.w;
            } else {
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    const bool in = p + j < body;
                    va[l][j] = (in && pa) ? pa[p + j] : 0;
                    vb[l][j] = (in && pb) ? pb[p + j] : 0;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < kLoads; ++l) {                 // wave-uniform: every lane reaches the ballots
            u64 k[kPerLane];
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) k[j] = key_of(va[l][j], vb[l][j], A, B, background);
            book(t, k, lane);
        }
        __syncthreads();
        const u64 key = s_key[tid];                        // flush: one global insert and one add per used slot
        if (key != 0) {
            const long long g = table_slot(keys, cap, key);
            if (g >= 0)
                atomicAdd(&hits[g], (u64)s_cnt[tid]);
            else
                atomicAdd(&counts[1], 1ull);
            s_cnt[tid] = 0;
            s_key[tid] = 0;
        }
        __syncthreads();                                   // the next chunk books into an empty table
    }
}

__global__ void __launch_bounds__(kThreads) overlaps_compact_kernel(const u64* __restrict__ keys, const u64* __restrict__ hits,
                                                                    long long cap, long long* __restrict__ rows,
                                                                    u64* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s - lane < cap; s += stride) {   // whole waves iterate
        const u64 k = s < cap ? keys[s] : 0ULL;
        const u64 bal = __ballot(k != 0);
        if (bal == 0) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(&counts[0], (u64)__popcll(bal));
        base = ((u64)(unsigned)__shfl((unsigned)(base >> 32), 0) << 32) | (unsigned)__shfl((unsigned)base, 0);
        if (k != 0) {
            const long long r = (long long)base + __popcll(bal & ((1ull << lane) - 1ull));   // < cap: one row per slot
            rows[kRow * r] = (long long)(k >> 32);
            rows[kRow * r + 1] = (long long)(k & 0xffffffffULL);
            rows[kRow * r + 2] = (long long)hits[s];
        }
    }
}

}  // namespace

extern "C" {

int sk_instance_overlaps_row_values(void) { return kRow; }

size_t sk_instance_overlaps_workspace_bytes(int64_t capacity) {
    return (capacity >= 1 && capacity <= kMaxCapacity) ? (size_t)capacity * 2 * sizeof(u64) : 0;
}

int sk_instance_overlaps(const int32_t* labels_a, int X, int Y, int Z, const int32_t* lut_a, int max_a, int N,
                         const int32_t* labels_b, const int32_t* lut_b, int max_b, int M, int background, int64_t* rows,
                         int64_t capacity, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sk_instance_overlaps";
    int rc = sk::check_mask_header(who, X, Y, Z, max_a, N, 62);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(M >= 0 && max_b >= 0, "sk_instance_overlaps: M = %d, max_b = %d must not be negative", M, max_b);
    SK_CHECK_ARG(background == 0 || background == 1, "sk_instance_overlaps: background %d must be 0 or 1", background);
    SK_CHECK_ARG(capacity >= 1 && capacity <= kMaxCapacity && (capacity & (capacity - 1)) == 0,
                 "sk_instance_overlaps: capacity %lld must be a power of two in [1, 2^40]", (long long)capacity);
    SK_CHECK_ARG(workspace_bytes >= sk_instance_overlaps_workspace_bytes(capacity),
                 "sk_instance_overlaps: workspace too small (%zu < %zu)", workspace_bytes,
                 sk_instance_overlaps_workspace_bytes(capacity));
    rc = sk::check_pointers(who, {{rows, 8}, {counts, 8}, {workspace, 8}});   // the outputs are written in an empty call too
    if (rc != SK_OK) return rc;
    const long long n = (long long)X * Y * Z;
    const bool empty = n == 0 || (N == 0 && M == 0) || (!background && (N == 0 || M == 0));
    if (!empty) {                                          // a side without instances is all background: not looked at
        rc = sk::check_pointers(who, {{labels_a, 4, N == 0}, {lut_a, 4, N == 0}, {labels_b, 4, M == 0}, {lut_b, 4, M == 0}});
        if (rc != SK_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (empty) return SK_OK;
    SK_CHECK_HIP(hipMemsetAsync(workspace, 0, sk_instance_overlaps_workspace_bytes(capacity), st));
    u64* keys = (u64*)workspace;
    u64* hits = keys + capacity;
    const Side A = {N ? labels_a : nullptr, lut_a, max_a, N}, B = {M ? labels_b : nullptr, lut_b, max_b, M};
    // the voxels in front of the first 16-byte boundary of a side that is read; the other side has to reach one there too
    const int32_t* lead = A.lab ? A.lab : B.lab;
    long long head = (long long)((16 - ((uintptr_t)lead & 15)) & 15) / 4;
    if (head > n) head = n;
    const int wide = (!A.lab || ((uintptr_t)(A.lab + head) & 15) == 0) && (!B.lab || ((uintptr_t)(B.lab + head) & 15) == 0);
    long long nchunks = (n - head + kChunk - 1) / kChunk;
    if (nchunks < 1) nchunks = 1;                          // nothing behind the head: its runs are still flushed
    const unsigned blocks = sk::tile_blocks(nchunks);
    overlaps_kernel<<<blocks, kThreads, 0, st>>>(A, B, n, (int)head, wide, background, nchunks, keys, hits, capacity,
                                                 (u64*)counts);
    SK_CHECK_LAUNCH();
    overlaps_compact_kernel<<<sk::stream_grid(capacity, kThreads), kThreads, 0, st>>>(keys, hits, capacity,
                                                                                      (long long*)rows, (u64*)counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
