// Which instances touch and by how much: for every unordered pair of rows the number of voxel
// pairs (p, p + d), d in {-1, 0, 1}^3, that carry the two rows, by the class of d -- shared faces along x / y / z, shared
// edges in the xy / xz / yz planes, shared corners.  sk_instance_stats counts the faces of an instance that are exposed
// to "another row"; this pass says which row.  The reference has no counterpart (skoots/lib/merge.py states the purpose
// -- objects that carry two labels -- and needs this table to serve it).
//
// Shape of the kernel
//   * A workgroup takes a tile of kTX x kTY x kTZ voxels and stages the tile's ROWS (the lut applied) with a one-voxel
//     halo on the three forward sides into LDS; a voxel outside the volume is staged as -1.  Every unordered voxel pair
//     belongs to exactly one 2 x 2 x 2 cell, the one whose low corner is the componentwise minimum of the two voxels:
//     its 3 axis edges from the low corner, the 2 diagonals of each of the 3 faces at the low corner and its 4 space
//     diagonals are the 13 "forward neighbours".  The lane of the low corner books them, so backward halos are not needed.
//   * A wave takes one z row of the tile at a time, lanes = consecutive z.  A wave row in which no lane's cell holds two
//     different rows skips everything else: interior voxels and background take no atomic.
//   * A contact is booked under key = lo << 32 | hi (never 0: hi >= 1).  Equal keys of neighbouring lanes are merged
//     first (a flat wall is one run), then the head of a run adds the run's length to a table in LDS (kSlots slots of a
//     key and seven 32-bit counters, open addressing, at most kProbes probes, LDS integer atomics).
//   * The tile flushes its table once into the global table: slots claimed with a 64-bit compare-and-swap on the key,
//     open addressing with at most kMaxProbe probes, counts added with 64-bit atomic adds.  A slot never empties, so a
//     key is either stored for the whole launch or refused for the whole launch; a refusal adds 1 to counts[1] and
//     writes nothing else.  A run whose key finds no LDS slot goes to the global table directly.
//   * A second kernel compacts the used slots into rows.  Integer atomics only, no loop without a bound, no workgroup
//     waits for another: the counts are exact and the set of rows is the same on every run.
#include "instance_rows.h"

namespace {

constexpr int kTX = 4, kTY = 16, kTZ = 64;            // tile; kTZ is the wave width: one lane per z
constexpr int kWX = kTX + 1, kWY = kTY + 1, kWZ = kTZ + 1;
constexpr int kStaged = kWX * kWY * kWZ;              // 5525 ints = 21.6 KiB
constexpr int kThreads = 256;
constexpr int kSlotBits = 8, kSlots = 1 << kSlotBits;  // pairs the LDS table holds per tile; one slot per thread in the flush
constexpr int kProbes = 8;                            // linear probes before a run goes to global memory
constexpr int kClasses = 7, kRow = 2 + kClasses;
constexpr int kMaxProbe = 128;                        // slots a global insertion looks at before it reports the table full
constexpr long long kMaxCapacity = 1ll << 40;

static_assert(kTZ == 64, "one lane per z of the tile");
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

// slot of `key` in the tile's table, or -1 when kProbes probes found neither the key nor a free slot
__device__ __forceinline__ int lds_slot(u64* s_key, u64 key) {
    const unsigned h = (unsigned)(mix64(key) >> (64 - kSlotBits));
    for (int p = 0; p < kProbes; ++p) {
        const int s = (int)((h + p) & (kSlots - 1));
        u64 k = ((volatile u64*)s_key)[s];                 // a key never changes once set within a tile
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

// key of the contact between two staged rows, 0 when there is none: different rows, both inside the volume, both
// positive -- or, with `floor` 0 (background on), at least one positive
__device__ __forceinline__ u64 contact_key(int a, int b, int floor) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return (a != b && lo >= floor) ? ((u64)(unsigned)lo << 32) | (unsigned)hi : 0ULL;
}

// Books one contact of class `cls` per lane with a nonzero key.  Called by whole waves: a run of equal keys along the
// lanes is added once, by its first lane.  (ck, cs) is the lane's last key and its LDS slot within this wave row: the
// pairs of a cell that cross one wall carry one key, and only the first of them is hashed and probed.
__device__ __forceinline__ void book(const Tables& t, u64 key, int cls, int lane, u64& ck, int& cs) {
    const u64 nonzero = __ballot(key != 0);
    if (nonzero == 0) return;                              // wave-uniform
    const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
    const unsigned plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    const bool head = key != 0 && (lane == 0 || plo != klo || phi != khi);
    const u64 heads = __ballot(head);
    // the run ends before the next lane that starts a run or holds no contact
    const u64 above = (heads | ~nonzero) & ~((2ull << lane) - 1ull);
    const unsigned len = above ? (unsigned)(__ffsll((long long)above) - 1 - lane) : (unsigned)(64 - lane);
    if (!head) return;
    int s = cs;
    if (key != ck) {
        s = lds_slot(t.s_key, key);
        if (s >= 0) {
            ck = key;
            cs = s;
        }
    }
    if (s >= 0) {
        atomicAdd(&t.s_cnt[s * kClasses + cls], len);
    } else {                                               // the tile's table is full for this key: global table directly
        const long long g = table_slot(t.keys, t.cap, key);
        if (g >= 0)
            atomicAdd(&t.hits[g * kClasses + cls], (u64)len);
        else
            atomicAdd(&t.counts[1], 1ull);
    }
}

template <int kConn>
__global__ void __launch_bounds__(kThreads) contacts_kernel(const int* __restrict__ lab, int X, int Y, int Z,
                                                            const int* __restrict__ lut, int max_id, int N, int floor,
                                                            long long ntiles, int tiles_y, int tiles_z,
                                                            u64* __restrict__ keys, u64* __restrict__ hits, long long cap,
                                                            u64* __restrict__ counts) {
    __shared__ int s_row[kStaged];
    __shared__ u64 s_key[kSlots];
    __shared__ unsigned s_cnt[kSlots * kClasses];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Tables t = {s_key, s_cnt, keys, hits, cap, counts};
    s_key[tid] = 0;                                        // the flush leaves the table empty again: cleared once
    for (int k = 0; k < kClasses; ++k) s_cnt[tid * kClasses + k] = 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int z0 = (int)(tile % tiles_z) * kTZ, y0 = (int)(tile / tiles_z % tiles_y) * kTY;
        const int x0 = (int)(tile / ((long long)tiles_z * tiles_y)) * kTX;
        // the previous tile's s_row is read before its flush barrier
        sk::stage_rows<kWX, kWY, kWZ, kThreads, false>(s_row, lab, lut, max_id, N, sk::Extents{X, Y, Z, 0}, x0, y0, z0, tid);
        __syncthreads();

        for (int r = wave; r < kTX * kTY; r += kThreads / 64) {   // wave-uniform: every lane reaches the ballots
            const int ix = r / kTY, iy = r % kTY;
            const int c = (ix * kWY + iy) * kWZ + lane;
            constexpr int dx = kWY * kWZ, dy = kWZ, dz = 1;
            const int v000 = s_row[c];                     // -1 where the tile leaves the volume: then the whole cell is
            const int v100 = s_row[c + dx], v010 = s_row[c + dy], v001 = s_row[c + dz];
            int v110 = v000, v101 = v000, v011 = v000, v111 = v000;
            if (kConn >= 18) {
                v110 = s_row[c + dx + dy];
                v101 = s_row[c + dx + dz];
                v011 = s_row[c + dy + dz];
            }
            if (kConn >= 26) v111 = s_row[c + dx + dy + dz];
            // a cell whose voxels inside the volume all carry one row has no contact
            const bool differ = v000 >= 0 && ((v100 >= 0 && v100 != v000) || (v010 >= 0 && v010 != v000) ||
                                              (v001 >= 0 && v001 != v000) || (v110 >= 0 && v110 != v000) ||
                                              (v101 >= 0 && v101 != v000) || (v011 >= 0 && v011 != v000) ||
                                              (v111 >= 0 && v111 != v000));
            if (__ballot(differ) == 0) continue;           // wave-uniform
            u64 ck = 0;                                    // slots stay claimed until the tile's flush: valid for the row
            int cs = -1;
            book(t, contact_key(v000, v100, floor), 0, lane, ck, cs);
            book(t, contact_key(v000, v010, floor), 1, lane, ck, cs);
            book(t, contact_key(v000, v001, floor), 2, lane, ck, cs);
            if (kConn >= 18) {
                book(t, contact_key(v000, v110, floor), 3, lane, ck, cs);
                book(t, contact_key(v100, v010, floor), 3, lane, ck, cs);
                book(t, contact_key(v000, v101, floor), 4, lane, ck, cs);
                book(t, contact_key(v100, v001, floor), 4, lane, ck, cs);
                book(t, contact_key(v000, v011, floor), 5, lane, ck, cs);
                book(t, contact_key(v010, v001, floor), 5, lane, ck, cs);
            }
            if (kConn >= 26) {
                book(t, contact_key(v000, v111, floor), 6, lane, ck, cs);
                book(t, contact_key(v100, v011, floor), 6, lane, ck, cs);
                book(t, contact_key(v010, v101, floor), 6, lane, ck, cs);
                book(t, contact_key(v001, v110, floor), 6, lane, ck, cs);
            }
        }
        __syncthreads();
        const u64 key = s_key[tid];                        // flush: one global insert per used slot, one add per count
        if (key != 0) {
            const long long g = table_slot(keys, cap, key);
            if (g < 0) atomicAdd(&counts[1], 1ull);
            for (int k = 0; k < kClasses; ++k) {
                const unsigned v = s_cnt[tid * kClasses + k];
                if (v) {
                    if (g >= 0) atomicAdd(&hits[g * kClasses + k], (u64)v);
                    s_cnt[tid * kClasses + k] = 0;
                }
            }
            s_key[tid] = 0;
        }
        // no barrier here: the next tile's staging writes s_row only, and its barrier comes before the table is used
    }
}

__global__ void __launch_bounds__(kThreads) contacts_compact_kernel(const u64* __restrict__ keys, const u64* __restrict__ hits,
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
            for (int c = 0; c < kClasses; ++c) rows[kRow * r + 2 + c] = (long long)hits[s * kClasses + c];
        }
    }
}

}  // namespace

extern "C" {

int sk_instance_contacts_row_values(void) { return kRow; }

size_t sk_instance_contacts_workspace_bytes(int64_t capacity) {
    return (capacity >= 1 && capacity <= kMaxCapacity) ? (size_t)capacity * (1 + kClasses) * sizeof(u64) : 0;
}

int sk_instance_contacts(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                         int connectivity, int background, int64_t* rows, int64_t capacity, int64_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sk_instance_contacts";
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 62);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26,
                 "sk_instance_contacts: connectivity %d must be 6, 18 or 26", connectivity);
    SK_CHECK_ARG(background == 0 || background == 1, "sk_instance_contacts: background %d must be 0 or 1", background);
    SK_CHECK_ARG(capacity >= 1 && capacity <= kMaxCapacity && (capacity & (capacity - 1)) == 0,
                 "sk_instance_contacts: capacity %lld must be a power of two in [1, 2^40]", (long long)capacity);
    SK_CHECK_ARG(workspace_bytes >= sk_instance_contacts_workspace_bytes(capacity),
                 "sk_instance_contacts: workspace too small (%zu < %zu)", workspace_bytes,
                 sk_instance_contacts_workspace_bytes(capacity));
    rc = sk::check_pointers(who, {{rows, 8}, {counts, 8}, {workspace, 8}});   // the outputs are written in an empty call too
    if (rc != SK_OK) return rc;
    const bool empty = sk::mask_empty(X, Y, Z, N);
    if (!empty) {
        rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}});
        if (rc != SK_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (empty) return SK_OK;
    SK_CHECK_HIP(hipMemsetAsync(workspace, 0, sk_instance_contacts_workspace_bytes(capacity), st));
    u64* keys = (u64*)workspace;
    u64* hits = keys + capacity;
    const sk::TileGrid tg = sk::tile_grid(X, Y, Z, kTX, kTY, kTZ);
    const int floor = background ? 0 : 1;
#define SK_CONTACTS_LAUNCH(C)                                                                                              \
    contacts_kernel<C><<<tg.blocks, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, floor, tg.ntiles, tg.tiles_y,     \
                                                       tg.tiles_z, keys, hits, capacity, (u64*)counts)
    if (connectivity == 6) SK_CONTACTS_LAUNCH(6);
    else if (connectivity == 18) SK_CONTACTS_LAUNCH(18);
    else SK_CONTACTS_LAUNCH(26);
#undef SK_CONTACTS_LAUNCH
    SK_CHECK_LAUNCH();
    contacts_compact_kernel<<<sk::stream_grid(capacity, kThreads), kThreads, 0, st>>>(keys, hits, capacity,
                                                                                      (long long*)rows, (u64*)counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
