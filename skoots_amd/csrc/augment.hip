// Training-crop augmentation (skoots/train/merged_transform.py:402-762, TransformFromCfg) and the skeleton mask
// target (skoots/lib/skeleton.py:531-593, skeleton_to_mask).
//
// sk_aug_resample is the reference's whole geometric chain -- crop 1, elastic_deform (grid_sample nearest,
// align_corners True), ttf.affine per z-slice (grid_sample nearest, align_corners False), crop 2, the three flips --
// as ONE gather over the crop-2 output.  Every stage maps integer voxel positions to integer voxel positions, so the
// composition is exact as long as each stage's coordinate arithmetic is torch's fp32 arithmetic, written here in the
// order of ATen's CUDA kernels (linspace, upsample_trilinear3d with align_corners False, grid_sampler_unnormalize,
// nearbyint) with no contraction (the library compiles with -ffp-contract=off).  The (1, 3, 2, 6, 6) elastic field
// is interpolated on the fly for the voxels the gather touches; the full-size field is never formed.  The same pass
// applies the elementwise invert and brightness and leaves per-(z, block) partial sums of image / 255 for the
// contrast means.
//
// sk_aug_intensity is two launches: contrast blend + clamp (one mean per z-slice, ttf.adjust_contrast on
// [Z, 1, X, Y]), noise add and per-(z, block) partial sums / sums of squares; then the normalisation with the mean
// and unbiased std when the reference computes them.  Every reduction has a fixed order and no atomics: two runs give
// the same bits.
//
// sk_skeleton_to_mask writes 1.0 at every in-range voxel of (point + offset) over all points and the host-built
// offset table (get_cached_disk_coords).  Every store is the value 1.0, so concurrent stores to one voxel are benign.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocksPerZ = 64;   // partial sums per z-slice: fixed by the extents alone

__host__ __device__ inline int blocks_per_z(int plane) {
    const int b = (plane + kBlock - 1) / kBlock;
    return b < 1 ? 1 : (b > kMaxBlocksPerZ ? kMaxBlocksPerZ : b);
}

// torch.linspace(-1, 1, n)[i] in fp32 (ATen RangeFactories: the first half counts up from start, the rest down from
// end)
__device__ inline float linspace_pm1(int i, int n) {
    if (n == 1) return -1.0f;
    const float step = (1.0f - (-1.0f)) / (float)(n - 1);
    if (i < n / 2) return -1.0f + step * (float)i;
    return 1.0f - step * (float)(n - i - 1);
}

// upsample_trilinear3d, align_corners False, one output index along one axis: source index and the two weights
struct Lin {
    int i0, ip;
    float l0, l1;
};

__device__ inline Lin lin_weights(int dst, int in_size, int out_size) {
    const float scale = (float)in_size / (float)out_size;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.0f) src = 0.0f;
    Lin r;
    r.i0 = (int)src;
    r.ip = (r.i0 < in_size - 1) ? 1 : 0;
    r.l1 = src - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

// nearest grid_sample index: nearbyint of the unnormalised coordinate, -1 when it lies outside [0, size)
__device__ inline int nearest_index(float coord, int size) {
    if (!(coord > -1.0e7f && coord < 1.0e7f)) return -1;
    const int i = (int)__builtin_rintf(coord);
    return (i >= 0 && i < size) ? i : -1;
}

template <typename T>
__device__ inline float load_image(const void* p, long long i) {
    return (float)((const T*)p)[i];
}

__device__ inline float read_image(const void* p, int dtype, long long i) {
    if (dtype == SK_U8) return load_image<uint8_t>(p, i);
    if (dtype == SK_F16) return load_image<_Float16>(p, i);
    return load_image<float>(p, i);
}

__device__ inline int read_mask(const void* p, int dtype, long long i) {
    if (dtype == SK_U8) return ((const uint8_t*)p)[i];
    if (dtype == SK_I16) return ((const int16_t*)p)[i];
    return ((const int32_t*)p)[i];
}

// fixed-order block sum of one double per thread (kBlock threads); the result is valid in thread 0
__device__ inline double block_sum(double v, double* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// fixed-order sum of n doubles by the whole block (every thread gets the result)
__device__ inline double block_sum_array(const double* a, int n, double* lds) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += a[i];
    return block_sum(s, lds);
}

// grid: (blocks_per_z(w2 * h2), d2); one z-slice per block row, columns (x, y) in a block-stride loop
__global__ void __launch_bounds__(kBlock) aug_resample_kernel(sk_aug_params p, const void* __restrict__ image,
                                                              int image_dtype, const void* __restrict__ masks,
                                                              int masks_dtype, const float* __restrict__ field,
                                                              float* __restrict__ out_image, int32_t* __restrict__ out_masks,
                                                              double* __restrict__ zpartial) {
    __shared__ double lds[kBlock];
    const int z = blockIdx.y;
    const int plane = p.w2 * p.h2;
    const float brightness = p.brightness_val;
    double zsum = 0.0;
    for (int col = blockIdx.x * kBlock + threadIdx.x; col < plane; col += gridDim.x * kBlock) {
        const int x = col / p.h2, y = col % p.h2;
        // flips, then the crop-2 origin: a position in the crop-1 window (the affine / elastic output)
        int xa = (p.flip_x ? p.w2 - 1 - x : x) + p.c2_x0;
        int ya = (p.flip_y ? p.h2 - 1 - y : y) + p.c2_y0;
        int za = (p.flip_z ? p.d2 - 1 - z : z) + p.c2_z0;
        bool inside = true;
        if (p.affine) {
            // torchvision _gen_affine_grid on [C, Z, H = X, W = Y]: base (col + 0.5 - W/2, row + 0.5 - H/2, 1) times
            // the rescaled theta (a 3-term inner product: an FMA chain in k order, as the matmul computes it), then
            // grid_sample (align_corners False): x of the grid indexes W (= Y), y indexes H (= X)
            const float bx = (float)ya - 0.5f * (float)p.h1 + 0.5f;
            const float by = (float)xa - 0.5f * (float)p.w1 + 0.5f;
            const float gx = __builtin_fmaf(1.0f, p.theta[2], __builtin_fmaf(by, p.theta[1], bx * p.theta[0]));
            const float gy = __builtin_fmaf(1.0f, p.theta[5], __builtin_fmaf(by, p.theta[4], bx * p.theta[3]));
            const int sy = nearest_index(((gx + 1.0f) * (float)p.h1 - 1.0f) / 2.0f, p.h1);
            const int sx = nearest_index(((gy + 1.0f) * (float)p.w1 - 1.0f) / 2.0f, p.w1);
            inside = sx >= 0 && sy >= 0;
            xa = sx;
            ya = sy;
        }
        if (inside && p.elastic) {
            // F.interpolate(field (1, 3, FD, FH, FW), (w1, h1, d1), trilinear) at (xa, ya, za); grid = linspace +
            // offset; grid_sample (align_corners True): grid[..., 0] indexes z, [..., 1] y, [..., 2] x
            const Lin ld = lin_weights(xa, p.field_d, p.w1);
            const Lin lh = lin_weights(ya, p.field_h, p.h1);
            const Lin lw = lin_weights(za, p.field_w, p.d1);
            const int sh = p.field_w, sd = p.field_h * p.field_w, sc = p.field_d * sd;
            float g[3];
            for (int c = 0; c < 3; ++c) {
                const float* f = field + c * sc;
                const int a0 = ld.i0 * sd, a1 = (ld.i0 + ld.ip) * sd;
                const int b0 = lh.i0 * sh, b1 = (lh.i0 + lh.ip) * sh;
                const int c0 = lw.i0, c1 = lw.i0 + lw.ip;
                const float v = ld.l0 * (lh.l0 * (lw.l0 * f[a0 + b0 + c0] + lw.l1 * f[a0 + b0 + c1]) +
                                         lh.l1 * (lw.l0 * f[a0 + b1 + c0] + lw.l1 * f[a0 + b1 + c1])) +
                                ld.l1 * (lh.l0 * (lw.l0 * f[a1 + b0 + c0] + lw.l1 * f[a1 + b0 + c1]) +
                                         lh.l1 * (lw.l0 * f[a1 + b1 + c0] + lw.l1 * f[a1 + b1 + c1]));
                g[c] = v * p.magnitude[c];
            }
            const float gz = linspace_pm1(za, p.d1) + g[0];
            const float gy = linspace_pm1(ya, p.h1) + g[1];
            const float gx = linspace_pm1(xa, p.w1) + g[2];
            const int sz = nearest_index(((gz + 1.0f) / 2.0f) * (float)(p.d1 - 1), p.d1);
            const int sy = nearest_index(((gy + 1.0f) / 2.0f) * (float)(p.h1 - 1), p.h1);
            const int sx = nearest_index(((gx + 1.0f) / 2.0f) * (float)(p.w1 - 1), p.w1);
            inside = sx >= 0 && sy >= 0 && sz >= 0;
            xa = sx;
            ya = sy;
            za = sz;
        }
        float v = 0.0f;
        int m = 0;
        if (inside) {
            const long long s = ((long long)(xa + p.c1_x0) * p.src_y + (ya + p.c1_y0)) * p.src_z + (za + p.c1_z0);
            v = read_image(image, image_dtype, s);
            m = read_mask(masks, masks_dtype, s);
        }
        if (p.invert) v = (v - 255.0f) * -1.0f;
        if (p.brightness) v = fminf(fmaxf(v + brightness, 0.0f), 255.0f);
        const long long o = (long long)col * p.d2 + z;
        out_image[o] = v;
        out_masks[o] = m;
        zsum += (double)(v / 255.0f);
    }
    const double s = block_sum(zsum, lds);
    if (threadIdx.x == 0) zpartial[(long long)z * gridDim.x + blockIdx.x] = s;
}

// contrast (per-z mean from the resample pass's partials) and noise, in place; partial sum / sum of squares per block
__global__ void __launch_bounds__(kBlock) aug_contrast_noise_kernel(float* __restrict__ img, int w2, int h2, int d2,
                                                                    const double* __restrict__ zpartial, int contrast,
                                                                    float ratio, float one_minus_ratio,
                                                                    const float* __restrict__ noise, float gamma,
                                                                    double* __restrict__ gpartial) {
    __shared__ double lds[kBlock];
    const int z = blockIdx.y;
    const int plane = w2 * h2;
    float mean = 0.0f;
    if (contrast) mean = (float)(block_sum_array(zpartial + (long long)z * gridDim.x, gridDim.x, lds) / (double)plane);
    double s = 0.0, q = 0.0;
    for (int col = blockIdx.x * kBlock + threadIdx.x; col < plane; col += gridDim.x * kBlock) {
        const long long o = (long long)col * d2 + z;
        float v = img[o];
        if (contrast) {
            const float t = v / 255.0f;
            const float u = ratio * t + one_minus_ratio * mean;
            v = fminf(fmaxf(u, 0.0f), 1.0f) * 255.0f;
        }
        if (noise) v = v + noise[o] * gamma;
        img[o] = v;
        s += (double)v;
        q += (double)v * (double)v;
    }
    const double bs = block_sum(s, lds);
    const double bq = block_sum(q, lds);
    if (threadIdx.x == 0) {
        const long long k = (long long)z * gridDim.x + blockIdx.x;
        gpartial[2 * k] = bs;
        gpartial[2 * k + 1] = bq;
    }
}

// (v - mean) / std; mean and std from the partials when the caller asks for them
__global__ void __launch_bounds__(kBlock) aug_normalize_kernel(float* __restrict__ img, long long n,
                                                               const double* __restrict__ gpartial, int n_partial,
                                                               int own_mean, float mean_in, int own_std, float std_in) {
    __shared__ double lds[kBlock];
    float mean = mean_in, stdv = std_in;
    if (own_mean || own_std) {
        double s = 0.0, q = 0.0;
        for (int i = threadIdx.x; i < n_partial; i += kBlock) {
            s += gpartial[2 * i];
            q += gpartial[2 * i + 1];
        }
        const double ts = block_sum(s, lds);
        const double tq = block_sum(q, lds);
        if (own_mean) mean = (float)(ts / (double)n);
        if (own_std) stdv = (float)sqrt((tq - ts * ts / (double)n) / (double)(n - 1));
    }
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
        img[i] = (img[i] - mean) / stdv;
}

__global__ void __launch_bounds__(kBlock) skeleton_to_mask_kernel(const float* __restrict__ points, long long n_points,
                                                                  const int32_t* __restrict__ offsets, int n_offsets,
                                                                  int X, int Y, int Z, float* __restrict__ out) {
    const long long n = n_points * n_offsets;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const long long p = i / n_offsets;
        const int k = (int)(i - p * n_offsets);
        // fp32 point + offset, then .long() (truncation toward zero): in range iff -1 < s < extent
        const float sx = points[3 * p] + (float)offsets[3 * k];
        const float sy = points[3 * p + 1] + (float)offsets[3 * k + 1];
        const float sz = points[3 * p + 2] + (float)offsets[3 * k + 2];
        if (!(sx > -1.0f && sx < (float)X && sy > -1.0f && sy < (float)Y && sz > -1.0f && sz < (float)Z)) continue;
        out[((long long)(int)sx * Y + (int)sy) * Z + (int)sz] = 1.0f;
    }
}

bool valid_image_dtype(int d) { return d == SK_U8 || d == SK_F16 || d == SK_F32; }
bool valid_mask_dtype(int d) { return d == SK_U8 || d == SK_I16 || d == SK_I32; }

}  // namespace

extern "C" {

size_t sk_aug_workspace_bytes(int w2, int h2, int d2) {
    if (w2 <= 0 || h2 <= 0 || d2 <= 0 || (long long)w2 * h2 > 0x7fffffffLL) return 0;
    // resample's per-z partials, then the intensity pass's (sum, sum of squares) pairs
    return (size_t)blocks_per_z(w2 * h2) * d2 * 3 * sizeof(double);
}

int sk_aug_resample(const sk_aug_params* params, const void* image, int image_dtype, const void* masks,
                    int masks_dtype, const float* field, float* out_image, int32_t* out_masks, void* workspace,
                    size_t workspace_bytes, void* stream) {
    SK_CHECK_ARG(params, "sk_aug_resample: params is NULL");
    const sk_aug_params p = *params;
    SK_CHECK_ARG(image && masks && out_image && out_masks && workspace, "sk_aug_resample: NULL buffer");
    SK_CHECK_ARG(valid_image_dtype(image_dtype), "sk_aug_resample: image dtype must be uint8, fp16 or fp32");
    SK_CHECK_ARG(valid_mask_dtype(masks_dtype), "sk_aug_resample: masks dtype must be uint8, int16 or int32");
    SK_CHECK_ARG(p.src_x > 0 && p.src_y > 0 && p.src_z > 0, "sk_aug_resample: empty source volume");
    SK_CHECK_ARG(p.w1 > 0 && p.h1 > 0 && p.d1 > 0 && p.c1_x0 >= 0 && p.c1_y0 >= 0 && p.c1_z0 >= 0 &&
                     (long long)p.c1_x0 + p.w1 <= p.src_x && (long long)p.c1_y0 + p.h1 <= p.src_y &&
                     (long long)p.c1_z0 + p.d1 <= p.src_z,
                 "sk_aug_resample: crop-1 window (%d, %d, %d) + (%d, %d, %d) outside the source (%d, %d, %d)", p.c1_x0,
                 p.c1_y0, p.c1_z0, p.w1, p.h1, p.d1, p.src_x, p.src_y, p.src_z);
    SK_CHECK_ARG(p.w2 > 0 && p.h2 > 0 && p.d2 > 0 && p.c2_x0 >= 0 && p.c2_y0 >= 0 && p.c2_z0 >= 0 &&
                     (long long)p.c2_x0 + p.w2 <= p.w1 && (long long)p.c2_y0 + p.h2 <= p.h1 &&
                     (long long)p.c2_z0 + p.d2 <= p.d1,
                 "sk_aug_resample: crop-2 window (%d, %d, %d) + (%d, %d, %d) outside crop 1 (%d, %d, %d)", p.c2_x0,
                 p.c2_y0, p.c2_z0, p.w2, p.h2, p.d2, p.w1, p.h1, p.d1);
    SK_CHECK_ARG((long long)p.w2 * p.h2 <= 0x7fffffffLL && p.d2 <= 65535,
                 "sk_aug_resample: output (%d, %d, %d) too large", p.w2, p.h2, p.d2);
    SK_CHECK_ARG(!p.elastic || (field && p.field_d > 0 && p.field_h > 0 && p.field_w > 0 &&
                                (long long)p.field_d * p.field_h * p.field_w <= (1 << 20)),
                 "sk_aug_resample: elastic needs a (1, 3, D, H, W) field");
    const size_t need = sk_aug_workspace_bytes(p.w2, p.h2, p.d2);
    SK_CHECK_ARG(workspace_bytes >= need, "sk_aug_resample: workspace %zu bytes, need %zu", workspace_bytes, need);
    const dim3 grid(blocks_per_z(p.w2 * p.h2), p.d2);
    aug_resample_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(p, image, image_dtype, masks, masks_dtype, field,
                                                                  out_image, out_masks, (double*)workspace);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_aug_intensity(float* image, int w2, int h2, int d2, int contrast, float contrast_val, const float* noise,
                     float noise_gamma, int own_mean, float mean, int own_std, float std_value, void* workspace,
                     size_t workspace_bytes, void* stream) {
    SK_CHECK_ARG(image && workspace, "sk_aug_intensity: NULL buffer");
    SK_CHECK_ARG(w2 > 0 && h2 > 0 && d2 > 0 && (long long)w2 * h2 <= 0x7fffffffLL && d2 <= 65535,
                 "sk_aug_intensity: bad extents (%d, %d, %d)", w2, h2, d2);
    SK_CHECK_ARG(!own_std || (long long)w2 * h2 * d2 > 1, "sk_aug_intensity: the std of one voxel is undefined");
    const size_t need = sk_aug_workspace_bytes(w2, h2, d2);
    SK_CHECK_ARG(workspace_bytes >= need, "sk_aug_intensity: workspace %zu bytes, need %zu", workspace_bytes, need);
    const int nb = blocks_per_z(w2 * h2);
    double* zpartial = (double*)workspace;
    double* gpartial = zpartial + (long long)nb * d2;
    const double r = (double)contrast_val;
    aug_contrast_noise_kernel<<<dim3(nb, d2), kBlock, 0, (hipStream_t)stream>>>(
        image, w2, h2, d2, zpartial, contrast, (float)r, (float)(1.0 - r), noise, noise_gamma, gpartial);
    SK_CHECK_LAUNCH();
    const long long n = (long long)w2 * h2 * d2;
    unsigned grid = sk::stream_grid(n, kBlock, 4);
    if (grid > 256) grid = 256;   // every block re-reduces the nb * d2 partials: keep their number small
    aug_normalize_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(image, n, gpartial, nb * d2, own_mean, mean, own_std,
                                                                   std_value);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_skeleton_to_mask(const float* points, int64_t n_points, const int32_t* offsets, int n_offsets, int X, int Y,
                        int Z, float* out, void* stream) {
    SK_CHECK_ARG(out, "sk_skeleton_to_mask: out is NULL");
    SK_CHECK_ARG(X > 0 && Y > 0 && Z > 0, "sk_skeleton_to_mask: bad extents (%d, %d, %d)", X, Y, Z);
    SK_CHECK_ARG(n_points >= 0 && n_points <= 0x7fffffffLL, "sk_skeleton_to_mask: %lld points do not fit in int32",
                 (long long)n_points);
    SK_CHECK_ARG(n_offsets > 0 && offsets, "sk_skeleton_to_mask: empty offset table");
    SK_CHECK_ARG(n_points == 0 || points, "sk_skeleton_to_mask: points is NULL");
    SK_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)X * Y * Z * sizeof(float), (hipStream_t)stream));
    if (n_points == 0) return SK_OK;
    const long long n = n_points * (long long)n_offsets;
    skeleton_to_mask_kernel<<<sk::stream_grid(n, kBlock, 4), kBlock, 0, (hipStream_t)stream>>>(points, n_points, offsets,
                                                                                             n_offsets, X, Y, Z, out);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
