// Exact nearest-instance transform of a label volume at an anisotropic voxel spacing: for every
// voxel, the squared distance to the nearest voxel of any instance (a site) and that instance's row.  It is the feature
// transform that edt.hip left out: utils/grow.py grows instances with it and repairs unassigned foreground.
//
// The definition (include/skoots_hip.h) is the nested minimum of edt.hip,
//     D2(p) = min over sites q of fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),
// taken as three passes along z, y and x; each pass minimises fl(w d^2 + g_prev(q)) along its axis and, where several
// positions give the same value, keeps the smallest coordinate.  A pass carries (g, row) per voxel.  -ffp-contract=off
// (Makefile) keeps every product and sum rounded on its own.
//
// Shape of the kernels
//   * One thread per voxel, the thread index fastest along z, with a grid-stride loop and 64-bit voxel indices, as in
//     edt.hip; no LDS and no wave-level primitive, so the result cannot depend on the launch geometry.
//   * One pruned walk (nl_walk) for all three passes.  It starts from the voxel's own position (d = 0: the previous
//     pass's value, or 0 / +inf in the z pass) and goes outward, d = 1, 2, ..., the low side before the high side.  The
//     low side has the smaller coordinates, so there an equal value wins (<=) and the walk goes on while w d^2 <= best:
//     a farther position can tie with a nearer one (9 + 16 = 16 + 9 = 25 + 0).  The high side wins only with a smaller
//     value (<) and is looked at only while w d^2 < best.  Every offer at distance d is at least w d^2 (g >= 0, rounding
//     is monotone), so nothing behind the stop can win or tie.
//   * limit2 bounds the walk as well: an offer with w d^2 > limit2 is above limit2 and so is everything built on it
//     (fl(a + b) >= max(a, b)), and the last pass discards what is above limit2.  A value at or below limit2 is made of
//     terms at or below limit2 only, so it and its ties are found exactly.  A pass reads at most
//     2 floor(sqrt(limit2 / w)) positions per voxel; with limit2 = +inf it is O(extent) per voxel.
//   * The x pass, the last one, applies limit2 and `where`; the z and y passes answer every voxel, because other lines
//     read them.
#include "instance_rows.h"

namespace {

constexpr int kThreads = 256;

// The walk of voxel p (coordinate c along the pass's axis of extent E and element stride S) from (best, row), its own
// position's offer.  kFirst: the z pass, where a position offers w d^2 if it is a site and nothing otherwise.
template <bool kFirst>
__device__ inline void nl_walk(const int* __restrict__ lab, const int* __restrict__ lut, int max_id, int N,
                               const double* __restrict__ g, const int* __restrict__ grow, long long p, int c, int E,
                               long long S, double w, double limit2, double& best, int& row) {
    for (int d = 1; c - d >= 0 || c + d < E; ++d) {
        const double wd = w * ((double)d * (double)d);     // d <= 2^26: the square is exact
        if (!(wd <= best) || wd > limit2) break;
        if (c - d >= 0) {
            const long long q = p - d * S;
            if (kFirst) {
                const int r = sk::row_of(lab[q], lut, max_id, N);
                if (r > 0) { best = wd; row = r; }         // wd <= best
            } else {
                const double v = wd + g[q];
                if (v <= best) { best = v; row = grow[q]; }
            }
        }
        if (c + d < E && wd < best) {
            const long long q = p + d * S;
            if (kFirst) {
                const int r = sk::row_of(lab[q], lut, max_id, N);
                if (r > 0) { best = wd; row = r; }         // wd < best
            } else {
                const double v = wd + g[q];
                if (v < best) { best = v; row = grow[q]; }
            }
        }
    }
}

// kAxis: 2 = z (the first pass: src is not read), 1 = y, 0 = x (the last pass: limit2 and `where` decide the output).
template <int kAxis>
__global__ void __launch_bounds__(kThreads) nl_pass_kernel(const int* __restrict__ lab, int X, int Y, int Z,
                                                           const int* __restrict__ lut, int max_id, int N, double w,
                                                           double limit2, const double* __restrict__ g,
                                                           const int* __restrict__ grow,
                                                           const unsigned char* __restrict__ where,
                                                           double* __restrict__ out, int* __restrict__ out_row,
                                                           long long total) {
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < total;
         p += (long long)gridDim.x * kThreads) {
        const int rp = sk::row_of(lab[p], lut, max_id, N);
        double best = (double)INFINITY;
        int row = 0;
        if (rp > 0) {                                      // a site: nothing is nearer, and `where` does not apply
            best = 0.0;
            row = rp;
        } else if (kAxis != 0 || where == nullptr || where[p] != 0) {
            const int z = (int)(p % Z), y = (int)(p / Z % Y), x = (int)(p / ((long long)Z * Y));
            const int c = kAxis == 2 ? z : kAxis == 1 ? y : x;
            const int E = kAxis == 2 ? Z : kAxis == 1 ? Y : X;
            const long long S = kAxis == 2 ? 1 : kAxis == 1 ? (long long)Z : (long long)Z * Y;
            if (kAxis != 2) {
                best = g[p];
                row = grow[p];
            }
            nl_walk<kAxis == 2>(lab, lut, max_id, N, g, grow, p, c, E, S, w, limit2, best, row);
        }
        if (kAxis == 0 && !(best <= limit2 && best < (double)INFINITY)) {
            best = (double)INFINITY;                       // out of reach, or no site at all
            row = 0;
        }
        out[p] = best;
        out_row[p] = row;
    }
}

__global__ void __launch_bounds__(kThreads) nl_fill_kernel(double* __restrict__ out, int* __restrict__ out_row,
                                                           long long total) {
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < total;
         p += (long long)gridDim.x * kThreads) {
        out[p] = (double)INFINITY;
        out_row[p] = 0;
    }
}

// d2 / row: the buffers of doubles / of ints the call names, NULL where one may be absent; n2: how many of each
int nl_check(const char* who, const void* labels, int X, int Y, int Z, const void* lut, int max_id, int N, double wx,
             double wy, double wz, double limit2, const void* where, const void* const* d2, const void* const* row,
             int n2, int first_required, bool* empty) {
    (void)where;                                           // bytes: any address is aligned, and NULL means "everywhere"
    int rc = sk::check_mask_header(who, X, Y, Z, max_id, N, 0);
    if (rc == SK_OK) rc = sk::check_exact_squares(who, X, Y, Z);
    if (rc == SK_OK) rc = sk::check_voxels(who, X, Y, Z, 62);
    if (rc == SK_OK) rc = sk::check_weights(who, wx, wy, wz);
    if (rc != SK_OK) return rc;
    SK_CHECK_ARG(limit2 >= 0, "%s: limit2 = %g must be a number and not negative (+inf: no limit)", who, limit2);
    *empty = (long long)X * Y * Z == 0;                    // N = 0 is no empty call here: every voxel is answered +inf
    if (*empty) return SK_OK;
    rc = sk::check_pointers(who, {{labels, 4}, {lut, 4}});
    for (int i = 0; i < n2 && rc == SK_OK; ++i)
        rc = sk::check_pointers(who, {{d2[i], 8, i < first_required}, {row[i], 4, i < first_required}});
    if (rc != SK_OK) return rc;
    const void* all[4] = {d2[0], row[0], d2[1], row[1]};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            SK_CHECK_ARG(all[i] == nullptr || all[i] != all[j],
                         "%s: the buffers of distances and rows, sources, scratch and outputs, must be four distinct "
                         "buffers: a pass cannot run in place", who);
    return SK_OK;
}

int nl_launch(int axis, const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double w,
              double limit2, const double* src, const int32_t* src_row, const unsigned char* where, double* dst,
              int32_t* dst_row, hipStream_t st) {
    const long long total = (long long)X * Y * Z;
    const unsigned grid = sk::stream_grid(total, kThreads);
    if (N == 0)
        nl_fill_kernel<<<grid, kThreads, 0, st>>>(dst, dst_row, total);
    else if (axis == 2)
        nl_pass_kernel<2><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, limit2, src, src_row, where,
                                                     dst, dst_row, total);
    else if (axis == 1)
        nl_pass_kernel<1><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, limit2, src, src_row, where,
                                                     dst, dst_row, total);
    else
        nl_pass_kernel<0><<<grid, kThreads, 0, st>>>(labels, X, Y, Z, lut, max_id, N, w, limit2, src, src_row, where,
                                                     dst, dst_row, total);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // namespace

extern "C" {

int sk_nearest_label_pass(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int axis,
                          double w, double limit2, const double* src_d2, const int32_t* src_row, const uint8_t* where,
                          double* dst_d2, int32_t* dst_row, void* stream) {
    SK_CHECK_ARG(axis >= 0 && axis <= 2, "sk_nearest_label_pass: axis = %d must be 0 (x), 1 (y) or 2 (z)", axis);
    bool empty = false;
    const void* d2[2] = {src_d2, dst_d2};
    const void* row[2] = {src_row, dst_row};
    const int rc = nl_check("sk_nearest_label_pass", labels, X, Y, Z, lut, max_id, N, w, w, w, limit2, where, d2, row, 2,
                            axis == 2 ? 1 : 0, &empty);        // the z pass reads no source
    if (rc != SK_OK || empty) return rc;
    return nl_launch(axis, labels, X, Y, Z, lut, max_id, N, w, limit2, src_d2, src_row, where, dst_d2, dst_row,
                     (hipStream_t)stream);
}

int sk_nearest_label(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double wx,
                     double wy, double wz, double limit2, const uint8_t* where, double* dist2, int32_t* nearest,
                     double* scratch_d2, int32_t* scratch_row, void* stream) {
    bool empty = false;
    const void* d2[2] = {dist2, scratch_d2};
    const void* row[2] = {nearest, scratch_row};
    const int rc = nl_check("sk_nearest_label", labels, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, row, 2, 0,
                            &empty);
    if (rc != SK_OK || empty) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0)
        return nl_launch(0, labels, X, Y, Z, lut, max_id, N, wx, limit2, nullptr, nullptr, where, dist2, nearest, st);
    // three passes between two pairs of buffers end in the pair the first one wrote
    int e = nl_launch(2, labels, X, Y, Z, lut, max_id, N, wz, limit2, nullptr, nullptr, nullptr, dist2, nearest, st);
    if (e != SK_OK) return e;
    e = nl_launch(1, labels, X, Y, Z, lut, max_id, N, wy, limit2, dist2, nearest, nullptr, scratch_d2, scratch_row, st);
    if (e != SK_OK) return e;
    return nl_launch(0, labels, X, Y, Z, lut, max_id, N, wx, limit2, scratch_d2, scratch_row, where, dist2, nearest, st);
}

}  // extern "C"
