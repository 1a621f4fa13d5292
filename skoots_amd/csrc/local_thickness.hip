// Local thickness of every instance of a label volume: for every instance voxel, the squared
// radius of the largest open ball around a voxel centre that lies inside the instance and contains the voxel
// (Hildebrand and Ruegsegger's local thickness, as a radius).  The reference has nothing of the kind.
//
// The definition (include/skoots_hip.h), on the output D2 of sk_label_edt:
//     T2(p) = max over voxels c with d2(p, c) < D2(c) of D2(c),   d2(p, c) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),
// every square exact, every product and sum rounded once (-ffp-contract=off, Makefile), the form w (d d).  D2(c) is the
// minimum of the same expression over the voxels of other rows, so a ball never holds a voxel of another row and this
// file reads no labels.  thick2 starts as a copy of dist2 (c = p always qualifies); sk_local_thickness_paint raises it.
//
// Shape of the kernel
//   * One wave per centre, the waves of the grid striding over the centre list.  Nothing crosses lanes and there is no
//     LDS: a lane's work depends on the centre and its lane number only.
//   * Per axis the half-extent h is the largest d with w d^2 < Dc.  floor(sqrt(Dc / w)) only seeds it: the exact test
//     corrects it up and down, so the box is the bounding box of the open ball whatever the square root rounded to.
//   * Lanes run over the flattened (y, z) rectangle of the clipped box, z fastest (at spacing (1, 1, 3) the z extent
//     alone is far too short to fill a wave) and carry fl(wy dy^2 + wz dz^2) along x.  A (y, z) whose carried term is
//     not below Dc is skipped: fl(a + b) >= b for a >= 0.  Membership is decided by d2 < Dc alone.
//   * Non-negative doubles order like unsigned 64-bit integers, so the value is raised with a vector 64-bit atomicMax
//     of the bit pattern, as edt_pass_kernel raises row_max.  A plain load comes first and the atomic is skipped where
//     the stored value is already as large: the value only grows, so a stale load costs an atomic and never a result.
//     The maximum does not depend on the order, so two runs are identical.
//   * A centre whose dist2 is not finite paints nothing (its ball is the whole volume; thick2 holds +inf there already).
//   * Centre indices are not checked on the device: the caller guarantees 0 <= centres[i] < X Y Z
//     (lib/morphology.py: local_thickness builds them from the volume itself).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;

typedef unsigned long long u64;

// the largest d in [0, E] with w d^2 < Dc (Dc > 0 and finite, so d = 0 qualifies); E <= 2^26 keeps (d + 1)^2 exact
__device__ inline int lt_half_extent(double Dc, double w, int E) {
    const double q = sqrt(Dc / w);
    int h = q < (double)E ? (int)q : E;
    while (h < E && w * ((double)(h + 1) * (double)(h + 1)) < Dc) ++h;
    while (h > 0 && !(w * ((double)h * (double)h) < Dc)) --h;
    return h;
}

__global__ void __launch_bounds__(kThreads) lt_paint_kernel(const double* __restrict__ dist2, int X, int Y, int Z,
                                                            double wx, double wy, double wz,
                                                            const long long* __restrict__ centres, long long n_centres,
                                                            u64* thick2) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long wave = (long long)blockIdx.x * (kThreads / kWave) + (threadIdx.x / kWave);
    const long long waves = (long long)gridDim.x * (kThreads / kWave);
    for (long long k = wave; k < n_centres; k += waves) {
        const long long c = centres[k];
        const double Dc = dist2[c];
        if (!(Dc > 0.0 && Dc < (double)INFINITY)) continue;
        const int cz = (int)(c % Z), cy = (int)(c / Z % Y), cx = (int)(c / ((long long)Z * Y));
        const int hx = lt_half_extent(Dc, wx, X), hy = lt_half_extent(Dc, wy, Y), hz = lt_half_extent(Dc, wz, Z);
        const int x0 = max(cx - hx, 0), x1 = min(cx + hx, X - 1);
        const int y0 = max(cy - hy, 0), y1 = min(cy + hy, Y - 1);
        const int z0 = max(cz - hz, 0), z1 = min(cz + hz, Z - 1);
        const int nz = z1 - z0 + 1;
        const long long nyz = (long long)(y1 - y0 + 1) * nz;   // at most 2^52
        const u64 bits = (u64)__double_as_longlong(Dc);
        for (long long j = lane; j < nyz; j += kWave) {
            const int y = y0 + (int)(j / nz), z = z0 + (int)(j % nz);
            const double dy = (double)(y - cy), dz = (double)(z - cz);
            const double inner = wy * (dy * dy) + wz * (dz * dz);
            if (!(inner < Dc)) continue;
            u64* line = thick2 + ((long long)y * Z + z);
            for (int x = x0; x <= x1; ++x) {
                const double dx = (double)(x - cx);
                const double d2 = wx * (dx * dx) + inner;
                if (d2 < Dc) {
                    u64* t = line + (long long)x * Y * Z;
                    if (*t < bits) atomicMax(t, bits);
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int sk_local_thickness_paint(const double* dist2, int X, int Y, int Z, double wx, double wy, double wz,
                             const int64_t* centres, int64_t n_centres, double* thick2, void* stream) {
    const char* who = "sk_local_thickness_paint";
    SK_CHECK_ARG(X >= 0 && Y >= 0 && Z >= 0, "%s: extents %d x %d x %d must not be negative", who, X, Y, Z);
    SK_CHECK_ARG(X <= (1 << 26) && Y <= (1 << 26) && Z <= (1 << 26),
                 "%s: extents %d x %d x %d: every extent must stay at or below 2^26 (d^2 exact in double)", who, X, Y, Z);
    const unsigned __int128 voxels = (unsigned __int128)X * Y * Z;                                        // below 2^78
    SK_CHECK_ARG(voxels < ((unsigned __int128)1 << 62), "%s: extents %d x %d x %d: X Y Z must stay below 2^62", who, X,
                 Y, Z);
    SK_CHECK_ARG(std::isfinite(wx) && std::isfinite(wy) && std::isfinite(wz) && wx > 0 && wy > 0 && wz > 0,
                 "%s: the weights %g, %g, %g (squared spacing) must be finite and positive", who, wx, wy, wz);
    SK_CHECK_ARG(n_centres >= 0, "%s: n_centres = %lld must not be negative", who, (long long)n_centres);
    if (voxels == 0 || n_centres == 0) return SK_OK;
    SK_CHECK_ARG(dist2 && centres && thick2, "%s: NULL pointer", who);
    SK_CHECK_ARG(((uintptr_t)dist2 & 7) == 0 && ((uintptr_t)centres & 7) == 0 && ((uintptr_t)thick2 & 7) == 0,
                 "%s: a pointer is not aligned to its elements", who);
    SK_CHECK_ARG((const void*)dist2 != (const void*)thick2,
                 "%s: thick2 and dist2 are one buffer: the radii of the centres are read while the map is raised", who);
    const unsigned grid = sk::stream_grid(n_centres, kThreads / kWave);
    lt_paint_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(dist2, X, Y, Z, wx, wy, wz, (const long long*)centres,
                                                               (long long)n_centres, (u64*)thick2);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
