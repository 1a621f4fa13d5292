// The pair table of the passes that book (row, row) keys (DESIGN.md sections 29, 34, 35): an open-addressing table of
// `capacity` 64-bit keys in global memory with kVals planes of 64-bit values behind it, filled with integer atomics
// and compacted into rows by a second kernel.  contacts.hip and overlaps.hip carry their own copies of mix64,
// table_slot and the compaction (interleaved values there, planes here); proximity.hip is the first user of this one.
//   workspace: keys[capacity], then vals[c * capacity + slot] for c in 0 .. kVals - 1
//   counts[0]: rows stored by the compaction, counts[1]: insertions refused
// A slot never empties, so a key is either stored for the whole launch or refused for the whole launch.
#pragma once
#include "common.h"

namespace sk {
namespace pair_table {

typedef unsigned long long u64;

constexpr long long kMaxCapacity = 1ll << 40;

inline bool capacity_ok(long long capacity) {
    return capacity >= 1 && capacity <= kMaxCapacity && (capacity & (capacity - 1)) == 0;
}

__device__ __forceinline__ u64 mix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// slot of `key` (never 0) in the global table, inserting it if absent; -1 when the kMaxProbe slots from its home hold
// other keys
template <int kMaxProbe>
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

// slot of `key` in a table of 1 << kSlotBits keys in LDS (0 = free), or -1 when kProbes probes found neither the key
// nor a free slot
template <int kSlotBits, int kProbes>
__device__ __forceinline__ int lds_slot(u64* s_key, u64 key) {
    constexpr int kSlots = 1 << kSlotBits;
    const unsigned h = (unsigned)(mix64(key) >> (64 - kSlotBits));
    for (int p = 0; p < kProbes; ++p) {
        const int s = (int)((h + p) & (kSlots - 1));
        u64 k = ((volatile u64*)s_key)[s];                 // a key never changes once set within a tile
        if (k == 0) k = atomicCAS(&s_key[s], 0ULL, key);
        if (k == 0 || k == key) return s;
    }
    return -1;
}

// One row of 2 + kVals int64 per used slot -- key >> 32, key & 0xffffffff, the slot's values -- in no particular order;
// counts[0] receives their number.  Whole waves iterate; launch with kThreads threads per workgroup.
template <int kVals, int kThreads>
__global__ void __launch_bounds__(kThreads) compact_kernel(const u64* __restrict__ keys, const u64* __restrict__ vals,
                                                           long long cap, long long* __restrict__ rows,
                                                           u64* __restrict__ counts) {
    constexpr int kRow = 2 + kVals;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s - lane < cap; s += stride) {
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
            for (int c = 0; c < kVals; ++c) rows[kRow * r + 2 + c] = (long long)vals[(long long)c * cap + s];
        }
    }
}

}  // namespace pair_table
}  // namespace sk
