// Exact squared Euclidean distance transform of every instance of a label volume at an anisotropic voxel spacing
// (DESIGN.md section 23): for every voxel of an instance, the squared distance to the nearest voxel that is not of that
// instance.  The reference has nothing of the kind (its stats_per_instance cannot run); the local width of an
// instance -- the radius of the largest sphere that fits inside -- is the maximum of this transform.
//
// The definition (include/skoots_hip.h) is a nested minimum,
//     D2(p) = min over q with row(q) != row(p) of fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),
// and rounding is monotone, so three passes along z, y and x reproduce it bit for bit: each pass takes the minimum of
// fl(w d^2 + g_prev(q)) along its axis.  -ffp-contract=off (Makefile) keeps every product and sum rounded on its own.
//
// Shape of the kernels
//   * One thread per voxel, the thread index fastest along z, the contiguous axis: in the y and x passes the lanes of a
//     wave read adjacent addresses at every step of the walk, in the z pass a shifted copy of their own line.
//   * All three passes are one pruned walk (edt_walk): from `best` -- +inf in the z pass, the previous pass's value
//     after it -- outward in both directions, d = 1, 2, ..., while w d^2 < best.  A voxel of the same row offers
//     fl(w d^2 + g_prev(q)); a voxel of another row offers w d^2 and ends its direction, because everything behind it
//     is farther; the end of the volume does the same in closed mode and offers nothing in open mode.  Stopping at
//     w d^2 >= best is exact: g >= 0 and rounding is monotone, so every farther offer is at least w d^2.
//   * A step compares the raw ids first (equal ids are equal rows), so the lut is read only where the id changes.
//   * No floating-point accumulation anywhere.  The last pass feeds row_max with a 64-bit integer atomicMax of the bit
//     pattern (non-negative doubles order like unsigned integers, +inf last): the lanes of a wave that hold one row
//     reduce by shuffles first, and the atomic is skipped where a plain load already shows a value as large -- the
//     value only grows.
#include "instance_rows.h"

namespace {

constexpr int kThreads = 256;

typedef unsigned long long u64;

// The walk of voxel p (coordinate c along the pass's axis of extent E and element stride S), whose id is vp and row rp.
template <bool kFirst>
__device__ inline double edt_walk(const int* __restrict__ lab, const int* __restrict__ lut, int max_id, int N,
                                  const double* __restrict__ g, long long p, int c, int E, long long S, double w,
                                  int closed, int vp, int rp, double best) {
    bool up = true, down = true;
    for (int d = 1; up || down; ++d) {
        const double wd = w * ((double)d * (double)d);     // d <= 2^26: the square is exact
        if (!(wd < best)) break;
        if (up) {
            if (c + d >= E) {
                up = false;
                if (closed) best = wd;
            } else {
                const long long q = p + d * S;
                const int v = lab[q];
                if (v == vp || sk::row_of(v, lut, max_id, N) == rp) {
                    if (!kFirst) best = fmin(best, wd + g[q]);
                } else {
                    best = wd;
                    up = false;
                }
            }
        }
        if (down) {
            if (c - d < 0) {
                down = false;
                if (closed) best = fmin(best, wd);
            } else {
                const long long q = p - d * S;
                const int v = lab[q];
                if (v == vp || sk::row_of(v, lut, max_id, N) == rp) {
                    if (!kFirst) best = fmin(best, wd + g[q]);
                } else {
                    best = fmin(best, wd);
                    down = false;
                }
            }
        }
    }
    return best;
}

// kAxis: 2 = z (the first pass: g is not read), 1 = y, 0 = x.  row_max: NULL except in the pass that finishes.
template <int kAxis>
__global__ void __launch_bounds__(kThreads) edt_pass_kernel(const int* __restrict__ lab, int X, int Y, int Z,
                                                            const int* __restrict__ lut, int max_id, int N, double w,
                                                            int closed, const double* __restrict__ g,
                                                            double* __restrict__ out, u64* __restrict__ row_max,
                                                            long long total) {
    const int lane = threadIdx.x & 63;
    // block-uniform trip count: every lane of a wave reaches the shuffles below
    for (long long base = (long long)blockIdx.x * kThreads; base < total; base += (long long)gridDim.x * kThreads) {
        const long long p = base + threadIdx.x;
        int rp = 0;
        double best = 0.0;
        if (p < total) {
            const int vp = lab[p];
            rp = sk::row_of(vp, lut, max_id, N);
            if (rp > 0) {
                const int z = (int)(p % Z), y = (int)(p / Z % Y), x = (int)(p / ((long long)Z * Y));
                const int c = kAxis == 2 ? z : kAxis == 1 ? y : x;
                const int E = kAxis == 2 ? Z : kAxis == 1 ? Y : X;
                const long long S = kAxis == 2 ? 1 : kAxis == 1 ? (long long)Z : (long long)Z * Y;
                best = edt_walk<kAxis == 2>(lab, lut, max_id, N, g, p, c, E, S, w, closed, vp, rp,
                                            kAxis == 2 ? (double)INFINITY : g[p]);
            }
            out[p] = best;
        }
        if (row_max == nullptr) continue;                  // uniform over the grid
        u64 todo = __ballot(rp > 0);
        while (todo) {                                     // wave-uniform: one turn per row the wave holds
            const int leader = __builtin_ctzll(todo);
            const int row = __shfl(rp, leader);
            const bool mine = rp == row;
            u64 m = mine ? (u64)__double_as_longlong(best) : 0ull;
            for (int off = 32; off > 0; off >>= 1) {
                const u64 o = __shfl_xor(m, off);
                m = o > m ? o : m;
            }
            if (lane == leader && row_max[row - 1] < m) atomicMax(&row_max[row - 1], m);
            todo &= ~__ballot(mine);
        }
    }
}

int edt_check(const char* who, const void* labels, int X, int Y, int Z, const void* lut, int max_id, int N, double wx,
              double wy, double wz, int closed, const void* a, bool a_is_read, const void* b, const void* row_max,
              bool* empty) {
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 0);
    if (rc == SK_OK) rc = sk::check_exact_squares(who, X, Y, Z);
    if (rc == SK_OK) rc = sk::check_voxels(who, X, Y, Z, 62);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(closed == 0 || closed == 1, "%s: closed = %d must be 0 or 1", who, closed);
    rc = sk::check_weights(who, wx, wy, wz);
    if (rc != SK_OK) return rc;
    *empty = sk::mask_empty(X, Y, Z, N);
    if (*empty) return SK_OK;
    rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}, {a, 8, !a_is_read}, {b, 8}, {row_max, 8, true}});
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(a != b, "%s: a pass cannot run in place: source and destination are one buffer", who);
    return SK_OK;
}

int edt_launch(int axis, const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double w,
               int closed, const double* src, double* dst, u64* row_max, hipStream_t st) {
    const long long total = (long long)X * Y * Z;
    const unsigned grid = sk::stream_grid(total, kThreads);
    if (axis == 2)
        edt_pass_kernel<2><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, closed, src, dst, row_max,
                                                      total);
    else if (axis == 1)
        edt_pass_kernel<1><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, closed, src, dst, row_max,
                                                      total);
    else
        edt_pass_kernel<0><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, closed, src, dst, row_max,
                                                      total);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_label_edt_pass(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int axis,
                      double w, int closed, const double* src, double* dst, uint64_t* row_max, void* stream) {
    SK_CHECK_ARG(axis >= 0 && axis <= 2, "sk_label_edt_pass: axis = %d must be 0 (x), 1 (y) or 2 (z)", axis);
    bool empty = false;
    const int rc = edt_check("sk_label_edt_pass", labels, X, Y, Z, lut, max_id, N, w, w, w, closed, src, axis != 2, dst,
                             row_max, &empty);                 // the z pass reads no source
    if (rc != SK_OK || empty) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (row_max) SK_CHECK_HIP(hipMemsetAsync(row_max, 0, (size_t)N * sizeof(uint64_t), st));
    return edt_launch(axis, labels, X, Y, Z, lut, max_id, N, w, closed, src, dst, (u64*)row_max, st);
}

int sk_label_edt(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double wx, double wy,
                 double wz, int closed, double* dist2, double* scratch, uint64_t* row_max, void* stream) {
    bool empty = false;
    const int rc = edt_check("sk_label_edt", labels, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, true, scratch,
                             row_max, &empty);
    if (rc != SK_OK || empty) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (row_max) SK_CHECK_HIP(hipMemsetAsync(row_max, 0, (size_t)N * sizeof(uint64_t), st));
    // three passes between two buffers end in the buffer the first one wrote
    int e = edt_launch(2, labels, X, Y, Z, lut, max_id, N, wz, closed, nullptr, dist2, nullptr, st);
    if (e != SK_OK) return e;
    e = edt_launch(1, labels, X, Y, Z, lut, max_id, N, wy, closed, dist2, scratch, nullptr, st);
    if (e != SK_OK) return e;
    return edt_launch(0, labels, X, Y, Z, lut, max_id, N, wx, closed, scratch, dist2, (u64*)row_max, st);
}

}  // extern "C"
