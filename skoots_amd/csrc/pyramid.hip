// One level of a multiscale pyramid: an (X, Y, Z) volume, Z innermost, pooled by (fx, fy, fz), every factor 1 or 2.
//
// Output extents are ceil(n / f); the block of an output voxel is clipped to the source voxels that exist, so a block
// holds nx * ny * nz = 1, 2, 4 or 8 voxels.  Three reductions (include/skoots_hip.h: sk_pool_volume):
//   mode   the value that occurs most often in the block, ties to the smallest value in the dtype's order; with sparse,
//          zeros are not counted unless the whole block is zero.  The result is a function of the block's multiset of
//          values -- of counts alone -- so it does not depend on the order in which a lane visits the block.
//   mean   (sum + n / 2) / n in integers, n the clipped block's voxel count: always a power of two, so a shift.
//   max    the largest value.
//
// Memory-bound: every source byte is read once, 1/2 to 1/8 of them are written.  No LDS.
//   lane    a lane owns runs of output voxels along z.  One step is a "unit": 16 source bytes (kV = 16 / sizeof(T)
//           voxels) of each of the fx * fy source rows of its output row, one 16-byte load per row, reduced in registers
//           (mode over 8 values: the 28 equalities of the pairs, each counted for both, then the best by (count,
//           value)), and one store of the kV / fz outputs: 16 bytes at fz = 1, 8 bytes at fz = 2.
//   wave    the units of one output row are consecutive lanes, so a wave's loads of a source row are one contiguous
//           run.  A row with fewer than 64 units shares its wave with the next rows (64 / lanes-per-row of them), so
//           short rows do not idle lanes.  The row of a lane, its (x, y) and its source row addresses are formed once per
//           lane and launch with 32-bit divisions; inside the z loop there is none.
//   grid    x: groups of output rows (4 waves a workgroup), y: z chunks of kUnitsPerLane units a lane.
//   scalar  the z tail of a row (Z not a multiple of kV), and every unit of an output row whose block is clipped in x
//           or y, go voxel by voxel through the same reductions on n <= 8 gathered values.  A volume whose rows are not
//           4-byte multiples (vector loads want dword alignment) goes that way as a whole.
// All stores are ordinary vector stores.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnitsPerLane = 4;   // units a lane walks in its z chunk

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// ---- the reductions on n <= N gathered values (n >= 1) ----

template <typename T, int N>
__device__ __forceinline__ T reduce_mode(const T (&v)[N], int n, int sparse) {
    int c[N];
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = 1;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            const int eq = (v[i] == v[j]) && j < n;   // i < j < n
            c[i] += eq;
            c[j] += eq;
        }
    }
    T best = v[0];
    int bc = (sparse && v[0] == (T)0) ? 0 : c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) {
        const int ci = (sparse && v[i] == (T)0) ? 0 : c[i];
        const bool better = i < n && (ci > bc || (ci == bc && v[i] < best));
        best = better ? v[i] : best;
        bc = better ? ci : bc;
    }
    return best;
}

template <typename T, int N>
__device__ __forceinline__ T reduce_mean(const T (&v)[N], int n) {
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) sum += i < n ? (unsigned)v[i] : 0u;
    const int sh = n >= 8 ? 3 : n >= 4 ? 2 : n >= 2 ? 1 : 0;   // n is 1, 2, 4 or 8
    return (T)((sum + ((unsigned)n >> 1)) >> sh);
}

template <typename T, int N>
__device__ __forceinline__ T reduce_max(const T (&v)[N], int n) {
    T m = v[0];
#pragma unroll
    for (int i = 1; i < N; ++i) m = (i < n && v[i] > m) ? v[i] : m;
    return m;
}

template <typename T, int N, int HOW>
__device__ __forceinline__ T reduce(const T (&v)[N], int n, int sparse) {
    if (HOW == SK_POOL_MODE) return reduce_mode<T, N>(v, n, sparse);
    if (HOW == SK_POOL_MEAN) return reduce_mean<T, N>(v, n);
    return reduce_max<T, N>(v, n);
}

// element k of 16 loaded bytes
template <typename T>
__device__ __forceinline__ T elem(const u32x4_a4& w, int k) {
    constexpr int per = 4 / (int)sizeof(T);
    if constexpr (per == 1) return (T)w[k];
    else return (T)(w[k / per] >> (8 * (int)sizeof(T) * (k % per)));
}

// One output voxel from the source, voxel by voxel: the block of (zo) in the rows row[0 .. nrows), clipped at Z.
template <typename T, int FXY, int FZ, int HOW>
__device__ __forceinline__ T pool_scalar(const T* const (&row)[FXY], int nrows, int zo, int Z, int sparse) {
    T v[FXY * FZ];
#pragma unroll
    for (int s = 0; s < FXY * FZ; ++s) v[s] = (T)0;
    const int z0 = zo * FZ;
    const int nz = (FZ == 2 && z0 + 1 < Z) ? 2 : 1;
    int n = 0;
#pragma unroll
    for (int r = 0; r < FXY; ++r) {
#pragma unroll
        for (int k = 0; k < FZ; ++k) {
            // the gathered values are packed to the front: a compile-time slot, filled by selection
            const bool in = r < nrows && k < nz;
            const T x = in ? row[r][z0 + k] : (T)0;
#pragma unroll
            for (int s = 0; s < FXY * FZ; ++s) v[s] = (in && s == n) ? x : v[s];
            n += in;
        }
    }
    return reduce<T, FXY * FZ, HOW>(v, n, sparse);
}

// FXY = fx * fy source rows of an output row, FZ = fz.  vec: rows are dword aligned, units go by 16-byte loads.
template <typename T, int FXY, int FZ, int HOW>
__global__ void __launch_bounds__(kThreads) pool_kernel(const T* __restrict__ src, T* __restrict__ dst, int X, int Y, int Z,
                                                        int Xo, int Yo, int Zo, int fx, int fy, int sparse, int vec,
                                                        int lanes_log2, int units, int full_units) {
    constexpr int kV = 16 / (int)sizeof(T);   // source voxels of a unit
    constexpr int kO = kV / FZ;               // outputs of a unit
    constexpr int N = FXY * FZ;
    const int lane_in_row = threadIdx.x & ((1 << lanes_log2) - 1);
    // Xo * Yo < 2^31 (checked by the host): the row index is a 32-bit number
    const long long at = ((long long)blockIdx.x * kThreads + threadIdx.x) >> lanes_log2;
    if (at >= (long long)Xo * Yo) return;
    const unsigned orow = (unsigned)at;
    const int xo = (int)(orow / (unsigned)Yo), yo = (int)(orow - (unsigned)xo * (unsigned)Yo);
    const int x0 = xo * fx, y0 = yo * fy;
    const int nx = (fx == 2 && x0 + 1 < X) ? 2 : 1, ny = (fy == 2 && y0 + 1 < Y) ? 2 : 1;
    const int nrows = nx * ny;
    // the rows that exist first; a missing row repeats row 0, so that no address leaves the volume
    const T* row[FXY];
#pragma unroll
    for (int r = 0; r < FXY; ++r) {
        const int dx = ny == 2 ? r >> 1 : r, dy = ny == 2 ? r & 1 : 0;
        const bool in = r < nrows;
        row[r] = src + ((size_t)(x0 + (in ? dx : 0)) * Y + (y0 + (in ? dy : 0))) * Z;
    }
    T* out = dst + (size_t)orow * Zo;
    const bool whole = nrows == FXY;
    const int lanes = 1 << lanes_log2;
    const int u_begin = blockIdx.y * (lanes * kUnitsPerLane);
    const int u_end = min(units, u_begin + lanes * kUnitsPerLane);
    for (int u = u_begin + lane_in_row; u < u_end; u += lanes) {
        if (vec && whole && u < full_units) {
            u32x4_a4 w[FXY];
#pragma unroll
            for (int r = 0; r < FXY; ++r) w[r] = *(const u32x4_a4*)(row[r] + (size_t)u * kV);
            T o[kO];
#pragma unroll
            for (int k = 0; k < kO; ++k) {
                T v[N];
#pragma unroll
                for (int r = 0; r < FXY; ++r) {
#pragma unroll
                    for (int q = 0; q < FZ; ++q) v[r * FZ + q] = elem<T>(w[r], k * FZ + q);
                }
                o[k] = reduce<T, N, HOW>(v, N, sparse);
            }
            constexpr int kWords = kO * (int)sizeof(T) / 4;   // 4 at fz = 1, 2 at fz = 2
            unsigned p[kWords];
#pragma unroll
            for (int i = 0; i < kWords; ++i) p[i] = 0u;
            constexpr unsigned kMask = sizeof(T) == 4 ? 0xFFFFFFFFu : (1u << (8 * (sizeof(T) & 3))) - 1u;
#pragma unroll
            for (int k = 0; k < kO; ++k) {
                constexpr int per = 4 / (int)sizeof(T);
                p[k / per] |= ((unsigned)o[k] & kMask) << (8 * (int)sizeof(T) * (k % per));
            }
            if (kWords == 4) {
                const u32x4_a4 s = {p[0], p[1], p[2 % kWords], p[3 % kWords]};
                *(u32x4_a4*)(out + (size_t)u * kO) = s;
            } else {
                const u32x2_a4 s = {p[0], p[1]};
                *(u32x2_a4*)(out + (size_t)u * kO) = s;
            }
        } else {
            const int zo_end = min(Zo, (u + 1) * kO);
            for (int zo = u * kO; zo < zo_end; ++zo) out[zo] = pool_scalar<T, FXY, FZ, HOW>(row, nrows, zo, Z, sparse);
        }
    }
}

template <typename T, int FXY, int FZ, int HOW>
int launch_one(const void* src, void* dst, int X, int Y, int Z, int fx, int fy, int sparse, hipStream_t stream) {
    constexpr int kV = 16 / (int)sizeof(T), kO = kV / FZ;
    const int Xo = (X + fx - 1) / fx, Yo = (Y + fy - 1) / fy, Zo = (Z + FZ - 1) / FZ;
    const int units = (Zo + kO - 1) / kO, full_units = Z / kV;
    const int vec = ((size_t)Z * sizeof(T)) % 4 == 0 && ((size_t)Zo * sizeof(T)) % 4 == 0 &&
                    ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    int lanes_log2 = 0;
    while (lanes_log2 < 6 && (1 << lanes_log2) < units) ++lanes_log2;   // lanes of a wave one output row takes
    const long long rows = (long long)Xo * Yo;
    SK_CHECK_ARG(rows <= 0x7FFFFFFFLL, "sk_pool_volume: %lld output rows, the limit is 2^31 - 1", rows);
    const long long gx = ((rows << lanes_log2) + kThreads - 1) / kThreads;
    const long long gy = (units + (kUnitsPerLane << lanes_log2) - 1) / (kUnitsPerLane << lanes_log2);
    SK_CHECK_ARG(gx <= 0x7FFFFFFFLL && gy <= 65535, "sk_pool_volume: %lld x %lld workgroups do not fit one grid", gx, gy);
    pool_kernel<T, FXY, FZ, HOW><<<dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, stream>>>(
        (const T*)src, (T*)dst, X, Y, Z, Xo, Yo, Zo, fx, fy, sparse, vec, lanes_log2, units, full_units);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

template <typename T, int HOW>
int launch(const void* src, void* dst, int X, int Y, int Z, int fx, int fy, int fz, int sparse, hipStream_t stream) {
    const int fxy = fx * fy;
    if (fz == 2) {
        if (fxy == 4) return launch_one<T, 4, 2, HOW>(src, dst, X, Y, Z, fx, fy, sparse, stream);
        if (fxy == 2) return launch_one<T, 2, 2, HOW>(src, dst, X, Y, Z, fx, fy, sparse, stream);
        return launch_one<T, 1, 2, HOW>(src, dst, X, Y, Z, fx, fy, sparse, stream);
    }
    if (fxy == 4) return launch_one<T, 4, 1, HOW>(src, dst, X, Y, Z, fx, fy, sparse, stream);
    return launch_one<T, 2, 1, HOW>(src, dst, X, Y, Z, fx, fy, sparse, stream);
}

}  // namespace

extern "C" int sk_pool_volume(const void* src, int dtype, int X, int Y, int Z, int fx, int fy, int fz, int how, int sparse,
                              void* dst, void* stream) {
    SK_CHECK_ARG(src && dst, "sk_pool_volume: NULL pointer");
    SK_CHECK_ARG(X > 0 && Y > 0 && Z > 0, "sk_pool_volume: extents (%d, %d, %d) must be positive", X, Y, Z);
    SK_CHECK_ARG((fx == 1 || fx == 2) && (fy == 1 || fy == 2) && (fz == 1 || fz == 2),
                 "sk_pool_volume: factors (%d, %d, %d): each must be 1 or 2", fx, fy, fz);
    SK_CHECK_ARG(fx * fy * fz > 1, "sk_pool_volume: factors (1, 1, 1) pool nothing");
    SK_CHECK_ARG(how >= SK_POOL_MODE && how <= SK_POOL_MAX, "sk_pool_volume: how = %d, must be 0 (mode), 1 (mean) or 2 (max)", how);
    const int elem_bytes = dtype == SK_I32 ? 4 : (dtype == SK_I16 || dtype == SK_U16) ? 2 : 1;
    if (how == SK_POOL_MODE)
        SK_CHECK_ARG(dtype == SK_I32 || dtype == SK_I16 || dtype == SK_U8,
                     "sk_pool_volume: dtype = %d, mode takes int32 (3), int16 (2) or uint8 (4)", dtype);
    else
        SK_CHECK_ARG(dtype == SK_U8 || dtype == SK_U16, "sk_pool_volume: dtype = %d, mean and max take uint8 (4) or uint16 (5)",
                     dtype);
    SK_CHECK_ARG(((uintptr_t)src & (elem_bytes - 1)) == 0 && ((uintptr_t)dst & (elem_bytes - 1)) == 0,
                 "sk_pool_volume: src or dst is not aligned to its elements");
    hipStream_t st = (hipStream_t)stream;
    sparse = sparse != 0;
    if (how == SK_POOL_MODE) {
        if (dtype == SK_I32) return launch<int32_t, SK_POOL_MODE>(src, dst, X, Y, Z, fx, fy, fz, sparse, st);
        if (dtype == SK_I16) return launch<int16_t, SK_POOL_MODE>(src, dst, X, Y, Z, fx, fy, fz, sparse, st);
        return launch<uint8_t, SK_POOL_MODE>(src, dst, X, Y, Z, fx, fy, fz, sparse, st);
    }
    if (how == SK_POOL_MEAN) {
        if (dtype == SK_U16) return launch<uint16_t, SK_POOL_MEAN>(src, dst, X, Y, Z, fx, fy, fz, 0, st);
        return launch<uint8_t, SK_POOL_MEAN>(src, dst, X, Y, Z, fx, fy, fz, 0, st);
    }
    if (dtype == SK_U16) return launch<uint16_t, SK_POOL_MAX>(src, dst, X, Y, Z, fx, fy, fz, 0, st);
    return launch<uint8_t, SK_POOL_MAX>(src, dst, X, Y, Z, fx, fy, fz, 0, st);
}
