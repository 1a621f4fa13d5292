// Which instances lie within a distance of each other: for two label volumes of one shape, each
// with its own (lut, max_id, N) header, one row `ra, rb, near_voxels, gap2_bits` per pair of rows that has a voxel pair
// (p, q) with d2(p, q) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)) <= limit2 -- the pair tables of contacts.hip (reach 1, one
// mask) and overlaps.hip (reach 0, two masks) at reach D.  include/skoots_hip.h has the definition.
//
// Shape of the kernel
//   * A workgroup takes a tile of kTX x kTY x kTZ voxels, lanes along z.  A wave keeps the rows of A of its kRows z rows
//     of the tile in registers; the rows of B of the tile grown by the reach (hx, hy, hz) on all six sides are staged
//     into LDS, outside the volume as 0, kStage loads in flight per lane.  The window is sized to the reach at launch
//     (dynamic LDS): 34 KiB at reach 1, 129 KiB at reach 5, and so is the workgroup (below: 8 waves where several
//     windows fit a CU, 16 where one does).  Every staged piece of 64 z of an (x, y) line of B gets a flag "holds a
//     row", written by the wave that staged it.
//   * The offsets within the limit are listed once per workgroup, in the fixed order of the walk (x outermost, then y,
//     then z), each with its d2 and its displacement in the window: an offset beyond limit2 costs nothing afterwards.
//   * A tile without a voxel of A, or with an empty window of B, leaves after staging.  A z row without a voxel of A, or
//     with no flagged piece of B within (hx, hy), skips the walk.
//   * The walk goes down the list, kBatch positions read from LDS before the first is used; the offset is wave-uniform.
//   * A lane keeps the first kSeen rows of B it meets, each with its minimum d2, in registers, and books them after the
//     walk: list entry by list entry, runs of equal keys along the lanes merged -- the run's head adds the run's length
//     and the run's minimum (a segmented minimum over the lanes) once.  The union row (ra, 0) is booked the same way.
//     A row of B that finds the list full is booked at once: it counts for near_voxels only where no earlier position
//     of the list carries it, decided by walking those positions again; the minimum needs no such care.
//   * Booking goes into a table of kSlots keys in LDS (a 32-bit count and a 64-bit minimum each), flushed once per tile
//     into the global table of pair_table.h; a key without an LDS slot goes to the global table directly.  Non-negative
//     doubles order as their bit patterns, so the minimum is an integer atomicMin.
//   * Integer atomics only, no loop without a bound, no workgroup waits for another: the same rows on every run.
#include "instance_rows.h"
#include "pair_table.h"

namespace {

using sk::pair_table::u64;

constexpr int kTX = 4, kTY = 16, kTZ = 64;             // tile; kTZ is the wave width: one lane per z
// Two workgroup sizes, chosen by the reach at launch (plan_of): where LDS leaves room for two windows or more on a CU,
// workgroups of 8 waves, compiled for 5 waves per SIMD (at most 96 registers; 6 would spill), so that two are resident
// and overlap each other's staging; where only one window fits, one workgroup of 16 waves, so that every SIMD still
// has 4 waves to hide the LDS latency of the walk.  sk_instance_proximity_resident asks the runtime for the same figure.
constexpr int kSmallThreads = 512, kSmallWavesPerSimd = 5;
constexpr int kLargeThreads = 1024, kLargeWavesPerSimd = 4;
constexpr int kMaxWaves = kLargeThreads / 64;
constexpr int kStage = 4;                              // global loads of the staging in flight per lane
constexpr int kBatch = 4;                              // positions of the list read from LDS before the first is used
constexpr int kSlotBits = 8, kSlots = 1 << kSlotBits;  // pairs the LDS table holds per tile
constexpr int kProbes = 8;                             // linear probes before a booking goes to global memory
constexpr int kVals = 2, kRow = 2 + kVals;             // near_voxels, gap2_bits
constexpr int kMaxProbe = 128;                         // slots a global insertion looks at before it reports the table full
constexpr int kCompactThreads = 256;
constexpr int kSeen = 4;                               // rows of B a lane keeps in registers
constexpr long long kLdsLimit = 160 * 1024;            // of one CU
constexpr long long kStaticLds = kSlots * (8 + 8 + 4) + 2 * kMaxWaves * 4 + 16;   // the table, s_any, s_listed padded
constexpr int kMaxReach = 1 << 26;                     // k^2 exact in double far beyond it; keeps the sums in int
constexpr u64 kNone = ~0ULL;

static_assert(kTZ == 64, "one lane per z of the tile");
static_assert(kSlots <= kSmallThreads, "the flush gives every slot a thread");

struct Side {
    const int* lab;
    const int* lut;
    int max_id, N;
};

struct Geom {
    int X, Y, Z;
    int hx, hy, hz;
    int WY, WZ;                                            // the window of B: (kTX + 2 hx) x WY x WZ
    double wx, wy, wz, limit2;
    int exclude_same;
};

struct Tables {
    u64* s_key;
    u64* s_min;
    unsigned* s_cnt;
    u64* keys;
    u64* vals;                                             // vals[slot]: near_voxels, vals[cap + slot]: gap2 bits
    long long cap;
    u64* counts;
};

__device__ __forceinline__ u64 bits_of(double v) { return (u64)__double_as_longlong(v); }

// adds `cnt` voxels to `key` and lowers its minimum to `m`: the tile's table, or the global one when the tile's has no
// slot for the key
__device__ __forceinline__ void add_pair(const Tables& t, u64 key, unsigned cnt, u64 m) {
    const int s = sk::pair_table::lds_slot<kSlotBits, kProbes>(t.s_key, key);
    if (s >= 0) {
        if (cnt) atomicAdd(&t.s_cnt[s], cnt);
        atomicMin(&t.s_min[s], m);
    } else {
        const long long g = sk::pair_table::table_slot<kMaxProbe>(t.keys, t.cap, key);
        if (g >= 0) {
            if (cnt) atomicAdd(&t.vals[g], (u64)cnt);
            atomicMin(&t.vals[t.cap + g], m);
        } else {
            atomicAdd(&t.counts[1], 1ull);
        }
    }
}

// Books one voxel per lane with a nonzero key, with the lane's minimum m.  Called by whole waves: a run of equal keys
// along the lanes is added once, by its first lane, with the run's length and the run's minimum.
__device__ __forceinline__ void book(const Tables& t, u64 key, u64 m, int lane) {
    if (__ballot(key != 0) == 0) return;                   // wave-uniform
    const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
    const unsigned plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    const bool head = lane == 0 || plo != klo || phi != khi;   // a lane without a key starts a run too: it ends one
    const u64 heads = __ballot(head);
    const u64 upto = (2ull << lane) - 1ull;                // lanes 0 .. lane (all 64 bits at lane 63)
    const u64 above = heads & ~upto;
    const unsigned len = above ? (unsigned)(__ffsll((long long)above) - 1 - lane) : (unsigned)(64 - lane);
    const int run = 63 - __clzll((long long)(heads & upto));   // the head of this lane's run; bit 0 is always set
    if (key == 0) m = kNone;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                     // segmented minimum: the head ends with its run's
        const unsigned lo = __shfl_down((unsigned)m, o), hi = __shfl_down((unsigned)(m >> 32), o);
        const int other_run = __shfl_down(run, o);
        const u64 other = ((u64)hi << 32) | lo;
        if (lane + o < 64 && other_run == run && other < m) m = other;
    }
    if (head && key != 0) add_pair(t, key, len, m);
}

template <int kThreads, int kWavesPerSimd>
__global__ void __launch_bounds__(kThreads, kWavesPerSimd) proximity_kernel(Side A, Side B, Geom g, long long ntiles,
                                                                            int tiles_y, int tiles_z,
                                                                            u64* __restrict__ keys, u64* __restrict__ vals,
                                                                            long long cap, u64* __restrict__ counts) {
    constexpr int kWaves = kThreads / 64;
    constexpr int kRows = kTX * kTY / kWaves;              // z rows of the tile a wave walks
    static_assert(kRows * kWaves == kTX * kTY, "every wave takes the same number of z rows");
    extern __shared__ __attribute__((aligned(16))) int smem[];
    __shared__ u64 s_key[kSlots];
    __shared__ u64 s_min[kSlots];
    __shared__ unsigned s_cnt[kSlots];
    __shared__ int s_any[kMaxWaves][2];                       // per staging wave: a voxel of A in the tile, a row in the window
    __shared__ int s_listed;                               // offsets within the limit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int WX = kTX + 2 * g.hx, WY = g.WY, WZ = g.WZ;
    const int nx = 2 * g.hx + 1, ny = 2 * g.hy + 1, nz = 2 * g.hz + 1;
    const int npiece = (WZ + 63) >> 6;                     // pieces of 64 z of a staged line
    const int noffsets = nx * ny * nz;
    double* s_d2 = reinterpret_cast<double*>(smem);        // the list: d2 of every offset within the limit, walk order
    int* s_off = smem + 2 * noffsets;                      // ... and its displacement in the window
    int* s_b = s_off + noffsets;                           // WX WY WZ rows of B
    int* s_flag = s_b + WX * WY * WZ;                      // WX WY npiece flags
    const Tables t = {s_key, s_min, s_cnt, keys, vals, cap, counts};
    if (tid < kSlots) {                                    // the flush leaves the table empty again: cleared once
        s_key[tid] = 0;
        s_min[tid] = kNone;
        s_cnt[tid] = 0;
    }
    if (wave == 0) {                                       // the list, read behind the first tile's staging barrier
        int listed = 0;
        for (int base = 0; base < noffsets; base += 64) {
            const int i = base + lane;
            bool in = false;
            double d2 = 0.0;
            int off = 0;
            if (i < noffsets) {
                const int ez = i % nz, ey = i / nz % ny, ex = i / (nz * ny);
                const int dx = ex - g.hx, dy = ey - g.hy, dz = ez - g.hz;
                d2 = g.wx * (double)(dx * dx) + (g.wy * (double)(dy * dy) + g.wz * (double)(dz * dz));
                in = d2 <= g.limit2;
                off = (ex * WY + ey) * WZ + ez;
            }
            const u64 bal = __ballot(in);
            if (in) {
                const int at = listed + __popcll(bal & ((1ull << lane) - 1ull));   // < noffsets
                s_d2[at] = d2;
                s_off[at] = off;
            }
            listed += __popcll(bal);
        }
        if (lane == 0) s_listed = listed;
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long z0 = (tile % tiles_z) * kTZ, y0 = (tile / tiles_z % tiles_y) * kTY;
        const long long x0 = (tile / ((long long)tiles_z * tiles_y)) * kTX;
        // ---- staging: the previous tile's LDS is no longer read (the barrier in front of its flush, or of its leave)
        int va[kRows];                                     // row r = wave + kWaves i of the tile: the wave's own
        {
            int v[kRows];
#pragma unroll
            for (int i = 0; i < kRows; ++i) {
                const int r = wave + kWaves * i;
                const long long gx = x0 + r / kTY, gy = y0 + r % kTY, gz = z0 + lane;
                v[i] = (gx < g.X && gy < g.Y && gz < g.Z) ? A.lab[(gx * g.Y + gy) * g.Z + gz] : 0;
            }
#pragma unroll
            for (int i = 0; i < kRows; ++i) va[i] = sk::row_of(v[i], A.lut, A.max_id, A.N);
        }
        bool any_b = false;
        const int npieces = WX * WY * npiece;
        for (int e0 = wave; e0 < npieces; e0 += kWaves * kStage) {
            int v[kStage], at[kStage];
#pragma unroll
            for (int u = 0; u < kStage; ++u) {             // every load is issued before the first is used
                const int e = e0 + kWaves * u;
                const int line = e / npiece, z = (e - line * npiece) * 64 + lane;
                const int wx = line / WY, wy = line - wx * WY;
                const long long gx = x0 - g.hx + wx, gy = y0 - g.hy + wy, gz = z0 - g.hz + z;
                const bool staged = e < npieces && z < WZ;
                const bool inside = gx >= 0 && gx < g.X && gy >= 0 && gy < g.Y && gz >= 0 && gz < g.Z;
                at[u] = staged ? line * WZ + z : -1;
                v[u] = (staged && inside) ? B.lab[(gx * g.Y + gy) * g.Z + gz] : 0;
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u) v[u] = sk::row_of(v[u], B.lut, B.max_id, B.N);
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int e = e0 + kWaves * u;
                if (at[u] >= 0) s_b[at[u]] = v[u];
                const bool flag = __ballot(v[u] > 0) != 0;
                if (e < npieces && lane == 0) s_flag[e] = flag ? 1 : 0;
                any_b |= flag;
            }
        }
        bool any_a = false;
#pragma unroll
        for (int i = 0; i < kRows; ++i) any_a |= va[i] > 0;
        const bool wave_a = __ballot(any_a) != 0;
        if (lane == 0) {
            s_any[wave][0] = wave_a ? 1 : 0;
            s_any[wave][1] = any_b ? 1 : 0;
        }
        __syncthreads();
        int has_a = 0, has_b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            has_a |= s_any[w][0];
            has_b |= s_any[w][1];
        }
        if (!(has_a && has_b)) {                           // workgroup-uniform: nothing of A here, or nothing of B in reach
            __syncthreads();                               // the next staging overwrites what was just read
            continue;
        }
        const int listed = s_listed;

#pragma unroll
        for (int i = 0; i < kRows; ++i) {                  // wave-uniform: every lane reaches the ballots
            const int r = wave + kWaves * i;
            const int ix = r / kTY, iy = r % kTY;
            const int a = va[i];
            if (__ballot(a > 0) == 0) continue;
            bool near_piece = false;
            for (int j = lane; j < nx * ny * npiece; j += 64) {
                const int exy = j / npiece, piece = j - exy * npiece;
                near_piece |= s_flag[((ix + exy / ny) * WY + iy + exy % ny) * npiece + piece] != 0;
            }
            if (__ballot(near_piece) == 0) continue;

            // The lane's partners: the first kSeen rows of B it meets (0: unused), each with its minimum; the row met last
            // is kept apart with its minimum (cur_row, cur_min), so a run of hits on one partner costs one comparison each.
            int seen_row[kSeen];
            double seen_min[kSeen];
#pragma unroll
            for (int j = 0; j < kSeen; ++j) {
                seen_row[j] = 0;
                seen_min[j] = (double)INFINITY;
            }
            int nseen = 0, last_over = 0, cur_row = 0;
            double cur_min = (double)INFINITY, over_min = (double)INFINITY, last_over_min = (double)INFINITY;
            const int* b_at = s_b + (ix * WY + iy) * WZ + lane;   // the window position of offset (-hx, -hy, -hz)
            for (int k0 = 0; k0 < listed; k0 += kBatch) {
                int rows[kBatch];
                double dist[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {         // every LDS read of the batch is issued before the first is used
                    const int k = k0 + u < listed ? k0 + u : listed - 1;
                    rows[u] = b_at[s_off[k]];
                    dist[u] = s_d2[k];
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    if (k0 + u >= listed) continue;        // wave-uniform
                    const int rb = rows[u];
                    const double d2 = dist[u];
                    if (a <= 0 || rb <= 0 || (g.exclude_same && rb == a)) continue;
                    if (rb != cur_row) {
                        bool found = false;
#pragma unroll
                        for (int j = 0; j < kSeen; ++j) {
                            if (cur_row != 0 && seen_row[j] == cur_row) seen_min[j] = cur_min;   // put it back
                            if (seen_row[j] == rb) found = true;
                        }
                        cur_row = 0;
                        if (!found && nseen < kSeen) {
#pragma unroll
                            for (int j = 0; j < kSeen; ++j)
                                if (j == nseen) seen_row[j] = rb;
                            ++nseen;
                            found = true;
                        }
                        if (!found) {
                            // the list is full: does an earlier position of the walk carry rb?
                            bool earlier = rb == last_over;
                            if (earlier && !(d2 < last_over_min)) continue;   // counted before, and as close: no atomic
                            last_over_min = d2;                // of last_over, which rb becomes below
                            for (int f = 0; f < k0 + u && !earlier; ++f) earlier = b_at[s_off[f]] == rb;
                            last_over = rb;
                            over_min = d2 < over_min ? d2 : over_min;
                            add_pair(t, ((u64)(unsigned)a << 32) | (unsigned)rb, earlier ? 0u : 1u, bits_of(d2));
                            continue;
                        }
                        cur_row = rb;
#pragma unroll
                        for (int j = 0; j < kSeen; ++j)
                            if (seen_row[j] == rb) cur_min = seen_min[j];
                    }
                    cur_min = d2 < cur_min ? d2 : cur_min;
                }
            }
            double all_min = over_min;
#pragma unroll
            for (int j = 0; j < kSeen; ++j) {
                if (cur_row != 0 && seen_row[j] == cur_row) seen_min[j] = cur_min;
                all_min = seen_min[j] < all_min ? seen_min[j] : all_min;   // +inf where unused
            }
            const u64 hi = (u64)(unsigned)a << 32;
#pragma unroll
            for (int j = 0; j < kSeen; ++j)
                book(t, j < nseen ? hi | (unsigned)seen_row[j] : 0ULL, bits_of(seen_min[j]), lane);
            book(t, nseen > 0 ? hi : 0ULL, bits_of(all_min), lane);   // the union row (ra, 0): overflow comes after a full list
        }
        __syncthreads();
        const u64 key = tid < kSlots ? s_key[tid] : 0ULL;  // flush: one global insert per used slot
        if (key != 0) {
            const long long gs = sk::pair_table::table_slot<kMaxProbe>(keys, cap, key);
            if (gs >= 0) {
                if (s_cnt[tid]) atomicAdd(&vals[gs], (u64)s_cnt[tid]);
                atomicMin(&vals[cap + gs], s_min[tid]);
            } else {
                atomicAdd(&counts[1], 1ull);
            }
            s_key[tid] = 0;
            s_min[tid] = kNone;
            s_cnt[tid] = 0;
        }
        // no barrier here: the next tile's staging does not touch the table, and its barrier comes before the table is used
    }
}

// the largest k in [0, kMaxReach] with fl(w k^2) <= limit2: fl is monotone, so the predicate is, and 0 always holds
int reach_of(double w, double limit2) {
    int lo = 0, hi = kMaxReach;
    if (w * ((double)hi * (double)hi) <= limit2) return hi;
    while (hi - lo > 1) {                                  // holds at lo, fails at hi
        const int mid = lo + (hi - lo) / 2;
        if (w * ((double)mid * (double)mid) <= limit2)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// dynamic LDS of a workgroup at a reach, in bytes: the list (a double and an int per offset of the box), the window of B
// and the flags of its pieces
long long window_bytes(long long hx, long long hy, long long hz) {
    const long long WX = kTX + 2 * hx, WY = kTY + 2 * hy, WZ = kTZ + 2 * hz;
    const long long noffsets = (2 * hx + 1) * (2 * hy + 1) * (2 * hz + 1);
    return (3 * noffsets + WX * WY * WZ + WX * WY * ((WZ + 63) / 64)) * 4;
}

struct Reach {
    int hx, hy, hz;
    bool taken;
    long long lds;                                         // dynamic + static bytes of a workgroup, when taken
    int threads;                                           // of the workgroup that is launched at this reach
    int per_cu;                                            // workgroups one CU holds: LDS, 32 wave slots, registers
};

// workgroups of `threads` one CU holds when the kernel is compiled for waves_per_simd on each of its 4 SIMDs
int resident(long long lds, int threads, int waves_per_simd) {
    const long long by_lds = kLdsLimit / lds, by_registers = 4 * waves_per_simd / (threads / 64);   // 32 wave slots: <= 8 per SIMD
    return (int)(by_lds < by_registers ? by_lds : by_registers);
}

Reach reach(double wx, double wy, double wz, double limit2) {
    Reach r = {reach_of(wx, limit2), reach_of(wy, limit2), reach_of(wz, limit2), false, 0, 0, 0};
    const long long cut = 1 << 12;                         // far beyond any window that fits: keeps the product small
    if (r.hx < cut && r.hy < cut && r.hz < cut) {
        r.lds = window_bytes(r.hx, r.hy, r.hz) + kStaticLds;
        r.taken = r.lds <= kLdsLimit;
    }
    if (!r.taken) {
        r.lds = 0;
        return r;
    }
    const bool small = 2 * r.lds <= kLdsLimit;             // two windows fit: smaller workgroups, several resident
    r.threads = small ? kSmallThreads : kLargeThreads;
    r.per_cu = resident(r.lds, r.threads, small ? kSmallWavesPerSimd : kLargeWavesPerSimd);
    return r;
}

int check_metric(const char* who, double wx, double wy, double wz, double limit2) {
    const int rc = sk::check_weights(who, wx, wy, wz);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(limit2 >= 0 && std::isfinite(limit2), "%s: limit2 = %g must be a finite number and not negative", who,
                 limit2);
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_instance_proximity_row_values(void) { return kRow; }

size_t sk_instance_proximity_workspace_bytes(int64_t capacity) {
    return sk::pair_table::capacity_ok(capacity) ? (size_t)capacity * (1 + kVals) * sizeof(u64) : 0;
}

int sk_instance_proximity_reach(double wx, double wy, double wz, double limit2, int32_t* out) {
    const char* who = "sk_instance_proximity_reach";
    const int rc = check_metric(who, wx, wy, wz, limit2);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(out != nullptr && ((uintptr_t)out & 3) == 0, "%s: out must be an aligned pointer to 8 int32", who);
    const Reach r = reach(wx, wy, wz, limit2);
    out[0] = r.hx;
    out[1] = r.hy;
    out[2] = r.hz;
    out[3] = r.taken ? 1 : 0;
    out[4] = (int32_t)r.lds;
    out[5] = r.per_cu;
    out[6] = r.threads;
    out[7] = 0;
    return SK_OK;
}

// what the runtime says for the kernel and the dynamic LDS that sk_instance_proximity launches at this reach
int sk_instance_proximity_resident(double wx, double wy, double wz, double limit2, int32_t* workgroups) {
    const char* who = "sk_instance_proximity_resident";
    const int rc = check_metric(who, wx, wy, wz, limit2);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(workgroups != nullptr && ((uintptr_t)workgroups & 3) == 0, "%s: NULL or unaligned pointer", who);
    const Reach r = reach(wx, wy, wz, limit2);
    SK_CHECK_ARG(r.taken, "%s: the reach (%d, %d, %d) is beyond what the kernel stages", who, r.hx, r.hy, r.hz);
    const int lds = (int)window_bytes(r.hx, r.hy, r.hz);
    const void* fn = r.threads == kSmallThreads ? (const void*)proximity_kernel<kSmallThreads, kSmallWavesPerSimd>
                                                : (const void*)proximity_kernel<kLargeThreads, kLargeWavesPerSimd>;
    if (lds > 48 * 1024) SK_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int n = 0;
    SK_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, r.threads, (size_t)lds));
    *workgroups = n;
    return SK_OK;
}

int sk_instance_proximity(const int32_t* labels_a, int X, int Y, int Z, const int32_t* lut_a, int max_a, int N,
                          const int32_t* labels_b, const int32_t* lut_b, int max_b, int M, double wx, double wy, double wz,
                          double limit2, int exclude_same, int64_t* rows, int64_t capacity, int64_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sk_instance_proximity";
    int rc = sk::check_mask_header(who, X, Y, Z, max_a, N, 62);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(M >= 0 && max_b >= 0, "%s: M = %d, max_b = %d must not be negative", who, M, max_b);
    rc = check_metric(who, wx, wy, wz, limit2);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(exclude_same == 0 || exclude_same == 1, "%s: exclude_same %d must be 0 or 1", who, exclude_same);
    const Reach r = reach(wx, wy, wz, limit2);
    SK_CHECK_ARG(r.taken,
                 "%s: the reach (%d, %d, %d) voxels of limit2 = %g at the weights %g, %g, %g is beyond what the kernel "
                 "stages (%lld bytes of LDS for one tile's window); it is not truncated",
                 who, r.hx, r.hy, r.hz, limit2, wx, wy, wz, kLdsLimit);
    SK_CHECK_ARG(sk::pair_table::capacity_ok(capacity), "%s: capacity %lld must be a power of two in [1, 2^40]", who,
                 (long long)capacity);
    SK_CHECK_ARG(workspace_bytes >= sk_instance_proximity_workspace_bytes(capacity), "%s: workspace too small (%zu < %zu)",
                 who, workspace_bytes, sk_instance_proximity_workspace_bytes(capacity));
    rc = sk::check_pointers(who, {{rows, 8}, {counts, 8}, {workspace, 8}});   // the outputs are written in an empty call too
    if (rc != SK_OK) return rc;
    const bool empty = (long long)X * Y * Z == 0 || N == 0 || M == 0;
    if (!empty) {
        rc = sk::check_pointers(who, {{labels_a, 4}, {lut_a, 4}, {labels_b, 4}, {lut_b, 4}});
        if (rc != SK_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    SK_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (empty) return SK_OK;
    u64* keys = (u64*)workspace;
    u64* vals = keys + capacity;
    SK_CHECK_HIP(hipMemsetAsync(keys, 0, (size_t)capacity * 2 * sizeof(u64), st));             // keys and near_voxels
    SK_CHECK_HIP(hipMemsetAsync(vals + capacity, 0xff, (size_t)capacity * sizeof(u64), st));   // gap2 bits: kNone
    const Side A = {labels_a, lut_a, max_a, N}, B = {labels_b, lut_b, max_b, M};
    const Geom g = {X, Y, Z, r.hx, r.hy, r.hz, kTY + 2 * r.hy, kTZ + 2 * r.hz, wx, wy, wz, limit2, exclude_same};
    const sk::TileGrid tg = sk::tile_grid(X, Y, Z, kTX, kTY, kTZ);
    const int lds = (int)window_bytes(r.hx, r.hy, r.hz);
#define SK_PROXIMITY_LAUNCH(T, W)                                                                                          \
    do {                                                                                                                   \
        if (lds > 48 * 1024)                                                                                               \
            SK_CHECK_HIP(hipFuncSetAttribute((const void*)proximity_kernel<T, W>,                                          \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds));                           \
        proximity_kernel<T, W><<<tg.blocks, T, lds, st>>>(A, B, g, tg.ntiles, tg.tiles_y, tg.tiles_z, keys, vals,         \
                                                         capacity, (u64*)counts);                                         \
    } while (0)
    if (r.threads == kSmallThreads)
        SK_PROXIMITY_LAUNCH(kSmallThreads, kSmallWavesPerSimd);
    else
        SK_PROXIMITY_LAUNCH(kLargeThreads, kLargeWavesPerSimd);
#undef SK_PROXIMITY_LAUNCH
    SK_CHECK_LAUNCH();
    sk::pair_table::compact_kernel<kVals, kCompactThreads>
        <<<sk::stream_grid(capacity, kCompactThreads), kCompactThreads, 0, st>>>(keys, vals, capacity, (long long*)rows,
                                                                                 (u64*)counts);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
