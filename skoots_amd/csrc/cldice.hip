// Soft clDice loss of the training step (reference skoots/train/loss.py:269-310 soft skeleton, 344-391
// soft_dice_cldice), value and input gradient, and the pieces that chain it into the fused step's d(loss)/d(logits).
//
// Soft skeleton (fp32, bit-identical to the reference: only min, max, sub, mul, add, relu):
//   e_0 = img, e_{k+1} = erode(e_k) = min(min(p_x, p_y), p_z), p_a = 3-wide min along axis a (out-of-range ignored);
//   open_k = dilate(e_{k+1}) = 3x3x3 max (out-of-range ignored); d_k = relu(e_k - open_k);
//   skel_0 = d_0, skel_k = skel_{k-1} + relu(d_k - skel_{k-1} * d_k), k = 1..iter.
// Forward, per level k: one pass writes e_{k+1}, one pass the 27-max, d_k and skel_k (prediction and ground truth in
// the same thread); the last level also folds the seven batch sums into per-block partials, then one block finalizes
// the loss and the coefficients of its gradient in double (fixed order: deterministic).
// Backward, per level k in reverse, in gather form (no atomics, bit-reproducible), three passes:
//   B1 pointwise: d(skel) -> d(d_k), d(skel_{k-1}); relu -> direct part of d(e_k) and d(open_k); the arg-max code of
//      the 27-window centred on each voxel (first maximum in x, y, z scan order with strict >, torch's max_pool3d);
//   B2 gather: T = d(e_{k+1}) = the gradient from the levels above + the d(open_k) of every window whose arg-max it is;
//   B3 gather: d(e_k) = direct part + T routed back through the erosion: torch.min ties split 1/2 / 1/2 (nested: a
//      three-way tie gives 1/4, 1/4, 1/2), each axis min to its first minimum (strict <).
// Every tensor is (B, X, Y, Z) fp32, Z fastest; one thread per voxel in a grid-stride loop.
#include "common.h"

namespace {

constexpr int kCldSums = 7;   // sum p g, sum g, sum p, sum S_p g, sum S_p, sum S_t p, sum S_t
constexpr int kCldCoef = 8;   // c0..c4 (see cld_finalize_kernel), the rest spare

struct Geo {
    long long N;   // B * X * Y * Z
    int X, Y, Z;
    long long sx;  // Y * Z
};

__device__ inline void coords(const Geo& g, long long i, int& x, int& y, int& z) {
    if (g.N <= 0xffffffffLL) {   // 32-bit division (the 64-bit one is a long software sequence)
        const unsigned u = (unsigned)i, t = u / (unsigned)g.Z;
        z = (int)(u - t * (unsigned)g.Z);
        const unsigned w = t / (unsigned)g.Y;
        y = (int)(t - w * (unsigned)g.Y);
        x = (int)(w % (unsigned)g.X);
        return;
    }
    z = (int)(i % g.Z);
    const long long t = i / g.Z;
    y = (int)(t % g.Y);
    x = (int)((t / g.Y) % g.X);
}

// 3-wide min along one axis, centre at `pos` of extent `ext`, element stride `st`: value and the offset (-1, 0, 1) of its
// first minimum (scan low -> high, strict <: torch's max_pool of -x keeps its first maximum)
__device__ inline float min3(const float* __restrict__ e, long long i, int pos, int ext, long long st, int& arg) {
    int a = pos > 0 ? -1 : 0;
    float p = e[i + a * st];
    const int hi = pos + 1 < ext ? 1 : 0;
    for (int d = a + 1; d <= hi; ++d) {
        const float v = e[i + d * st];
        if (v < p) {
            p = v;
            a = d;
        }
    }
    arg = a;
    return p;
}

__device__ inline float erode_at(const float* __restrict__ e, const Geo& g, long long i, int x, int y, int z) {
    int a;
    const float p1 = min3(e, i, x, g.X, g.sx, a);
    const float p2 = min3(e, i, y, g.Y, g.Z, a);
    const float p3 = min3(e, i, z, g.Z, 1, a);
    return fminf(fminf(p1, p2), p3);
}

// 3x3x3 max over the in-range window and the code (dx+1)*9 + (dy+1)*3 + (dz+1) of its first maximum.  Unrolled on
// clamped offsets (an out-of-range neighbour reads the centre plane again) so that all 27 loads issue at once; the
// duplicates cannot change the max, and the arg-max skips them (`in`).
template <bool CODE>
__device__ inline float max27(const float* __restrict__ e, const Geo& g, long long i, int x, int y, int z, int& code) {
    const long long ox[3] = {x > 0 ? -g.sx : 0, 0, x + 1 < g.X ? g.sx : 0};
    const long long oy[3] = {y > 0 ? -(long long)g.Z : 0, 0, y + 1 < g.Y ? (long long)g.Z : 0};
    const long long oz[3] = {z > 0 ? -1 : 0, 0, z + 1 < g.Z ? 1 : 0};
    const bool ix[3] = {x > 0, true, x + 1 < g.X}, iy[3] = {y > 0, true, y + 1 < g.Y}, iz[3] = {z > 0, true, z + 1 < g.Z};
    float v[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) v[k] = e[i + ox[k / 9] + oy[(k / 3) % 3] + oz[k % 3]];
    float m = v[13];
    if (!CODE) {
#pragma unroll
        for (int k = 0; k < 27; ++k) m = fmaxf(m, v[k]);
        return m;
    }
    int c = -1;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const bool in = ix[k / 9] && iy[(k / 3) % 3] && iz[k % 3];
        if (in && (c < 0 || v[k] > m)) {
            m = v[k];
            c = k;
        }
    }
    code = c;
    return m;
}

// ------------------------------------------------------------------------------------------
// Forward
// ------------------------------------------------------------------------------------------
struct FwdSide {
    const float* e;     // e_k
    float* e1;          // e_{k+1}
    const float* sp;    // skel_{k-1}, NULL at k = 0
    float* sn;          // skel_k (may equal sp: the update is pointwise)
};

template <int NS>
__global__ void __launch_bounds__(256) cld_erode_kernel(Geo g, FwdSide s0, FwdSide s1) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.N; i += (long long)gridDim.x * 256) {
        int x, y, z;
        coords(g, i, x, y, z);
        s0.e1[i] = erode_at(s0.e, g, i, x, y, z);
        if (NS == 2) s1.e1[i] = erode_at(s1.e, g, i, x, y, z);
    }
}

__device__ inline float skel_update(const FwdSide& s, const Geo& g, long long i, int x, int y, int z) {
    int c;
    const float open = max27<false>(s.e1, g, i, x, y, z, c);
    const float t = s.e[i] - open;
    const float d = t > 0.0f ? t : 0.0f;
    if (!s.sp) return d;
    const float sk = s.sp[i];
    const float u = d - sk * d;
    return sk + (u > 0.0f ? u : 0.0f);
}

// NS sides (1: a lone skeleton, 2: prediction + ground truth).  REDUCE (last level, NS = 2): per-block partials
// (nblk, kCldSums) of the seven batch sums; pred / gt = the level-0 images.
template <int NS, bool REDUCE>
__global__ void __launch_bounds__(256) cld_skel_kernel(Geo g, FwdSide s0, FwdSide s1, const float* __restrict__ pred,
                                                       const float* __restrict__ gt, float* __restrict__ partial) {
    __shared__ float red[4][kCldSums];
    float acc[kCldSums];
#pragma unroll
    for (int k = 0; k < kCldSums; ++k) acc[k] = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.N; i += (long long)gridDim.x * 256) {
        int x, y, z;
        coords(g, i, x, y, z);
        const float sp = skel_update(s0, g, i, x, y, z);
        s0.sn[i] = sp;
        if (NS == 2) {
            const float st = skel_update(s1, g, i, x, y, z);
            s1.sn[i] = st;
            if (REDUCE) {
                const float p = pred[i], q = gt[i];
                acc[0] += p * q;
                acc[1] += q;
                acc[2] += p;
                acc[3] += sp * q;
                acc[4] += sp;
                acc[5] += st * p;
                acc[6] += st;
            }
        }
    }
    if (!REDUCE) return;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCldSums; ++k) {
        float t = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m);
        if ((tid & 63) == 0) red[tid >> 6][k] = t;
    }
    __syncthreads();
    if (tid < kCldSums) partial[(long long)blockIdx.x * kCldSums + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// loss = (1 - alpha) dice + alpha cl_dice (loss.py:379-391); dice with smooth 1 (soft_dice's default: loss.py:378
// does not pass self.smooth).  coef: dL/dp_v (direct) = c0 + c1 g_v + c2 S_t(v);  dL/dS_p(v) = c3 g_v + c4.
__global__ void __launch_bounds__(256) cld_finalize_kernel(const float* __restrict__ partial, int nblk, double alpha,
                                                           double smooth, float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ double acc[256];
    __shared__ double sums[kCldSums];
    const int tid = threadIdx.x;
    for (int k = 0; k < kCldSums; ++k) {
        double s = 0.0;
        for (int j = tid; j < nblk; j += 256) s += (double)partial[(long long)j * kCldSums + k];
        acc[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int j = 0; j < 256; ++j) t += acc[j];
            sums[k] = t;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double I = sums[0], G = sums[1], P = sums[2], SPG = sums[3], SP = sums[4], STP = sums[5], ST = sums[6];
    const double N = 2.0 * I + 1.0, D = G + P + 1.0;
    const double dice = 1.0 - N / D;
    const double tp = (SPG + smooth) / (SP + smooth), ts = (STP + smooth) / (ST + smooth);
    const double cl = 1.0 - 2.0 * (tp * ts) / (tp + ts);
    loss[0] = (float)((1.0 - alpha) * dice + alpha * cl);
    const double q = (tp + ts) * (tp + ts);
    const double dtp = -2.0 * ts * ts / q, dts = -2.0 * tp * tp / q;
    coef[0] = (float)((1.0 - alpha) * N / (D * D));
    coef[1] = (float)(-2.0 * (1.0 - alpha) / D);
    coef[2] = (float)(alpha * dts / (ST + smooth));
    const double c3 = alpha * dtp / (SP + smooth);
    coef[3] = (float)c3;
    coef[4] = (float)(-c3 * tp);
}

// ------------------------------------------------------------------------------------------
// Backward (level k)
// ------------------------------------------------------------------------------------------
struct BwdArgs {
    const float* ek;      // e_k (k = 0: the prediction)
    const float* ek1;     // e_{k+1}
    const float* sprev;   // skel_{k-1}, NULL at k = 0
    const float* gs_in;   // dL/dskel_k, NULL at k = iter (then c3 g + c4)
    float* gs_out;        // dL/dskel_{k-1} (k >= 1)
    const float* gt;
    const float* st;      // S_t (the last level's direct term)
    const float* coef;
    float* dopen;         // dL/d open_k
    float* direct;        // dL/de_k through d_k = relu(e_k - open_k)
    unsigned char* code;  // arg-max code of the 27-window centred on the voxel
    const float* de_up;   // dL/de_{k+1} from the levels above, NULL at k = iter
    float* tgrad;         // T = total dL/de_{k+1}
    float* de_out;        // dL/de_k
};

__global__ void __launch_bounds__(256) cld_bwd_point_kernel(Geo g, BwdArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.N; i += (long long)gridDim.x * 256) {
        int x, y, z;
        coords(g, i, x, y, z);
        int c;
        const float open = max27<true>(a.ek1, g, i, x, y, z, c);
        const float t = a.ek[i] - open;
        const float d = t > 0.0f ? t : 0.0f;
        const float G = a.gs_in ? a.gs_in[i] : a.coef[3] * a.gt[i] + a.coef[4];
        float dd = G;
        if (a.sprev) {   // skel_k = s + relu(d - s*d)
            const float s = a.sprev[i];
            const float u = d - s * d;
            const float gr = u > 0.0f ? G : 0.0f;
            dd = gr + (-gr) * s;
            a.gs_out[i] = G + (-gr) * d;
        }
        const float dt = t > 0.0f ? dd : 0.0f;
        a.direct[i] = dt;
        a.dopen[i] = -dt;
        a.code[i] = (unsigned char)c;
    }
}

// T(v) = de_up(v) + sum over the windows centred at v + delta (raster order) whose arg-max is v of dopen(centre); loads
// on clamped offsets as in max27
__global__ void __launch_bounds__(256) cld_bwd_dilate_kernel(Geo g, BwdArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.N; i += (long long)gridDim.x * 256) {
        int x, y, z;
        coords(g, i, x, y, z);
        const long long ox[3] = {x > 0 ? -g.sx : 0, 0, x + 1 < g.X ? g.sx : 0};
        const long long oy[3] = {y > 0 ? -(long long)g.Z : 0, 0, y + 1 < g.Y ? (long long)g.Z : 0};
        const long long oz[3] = {z > 0 ? -1 : 0, 0, z + 1 < g.Z ? 1 : 0};
        const bool ix[3] = {x > 0, true, x + 1 < g.X}, iy[3] = {y > 0, true, y + 1 < g.Y}, iz[3] = {z > 0, true, z + 1 < g.Z};
        unsigned char cd[27];
        float dv[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const long long j = i + ox[k / 9] + oy[(k / 3) % 3] + oz[k % 3];
            cd[k] = a.code[j];
            dv[k] = a.dopen[j];
        }
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 27; ++k)
            if (ix[k / 9] && iy[(k / 3) % 3] && iz[k % 3] && cd[k] == 26 - k) s += dv[k];
        a.tgrad[i] = a.de_up ? a.de_up[i] + s : s;
    }
}

// share of T that the erosion min(min(p1, p2), p3) routes to p_{ax+1} (torch.min ties: halves)
__device__ inline float erode_share(float p1, float p2, float p3, float T, int ax) {
    const float m12 = fminf(p1, p2);
    const float g12 = m12 < p3 ? T : (m12 == p3 ? T * 0.5f : 0.0f);
    if (ax == 2) return m12 > p3 ? T : (m12 == p3 ? T * 0.5f : 0.0f);
    if (ax == 0) return p1 < p2 ? g12 : (p1 == p2 ? g12 * 0.5f : 0.0f);
    return p2 < p1 ? g12 : (p1 == p2 ? g12 * 0.5f : 0.0f);
}

// de_k(v) = direct(v) + sum over the erosion centres c in {v - 1, v, v + 1} along each axis whose axis minimum is v of
// that axis's share of T(c); at k = 0 also the loss's direct terms c0 + c1 g + c2 S_t.  Every load is unconditional
// on a clamped in-range address (an out-of-range centre reads v's neighbourhood and is masked by `cin`).
template <bool LAST>
__global__ void __launch_bounds__(256) cld_bwd_erode_kernel(Geo g, BwdArgs a) {
    const long long st[3] = {g.sx, (long long)g.Z, 1};
    const int ext[3] = {g.X, g.Y, g.Z};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.N; i += (long long)gridDim.x * 256) {
        int p[3];
        coords(g, i, p[0], p[1], p[2]);
        float de = a.direct[i];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            float s = 0.0f;
#pragma unroll
            for (int d = -1; d <= 1; ++d) {
                const int pc = p[ax] + d;
                const bool cin = pc >= 0 && pc < ext[ax];
                const long long c = i + (cin ? d * st[ax] : 0);
                float pm[3];
                int am[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int q = (b == ax && cin) ? pc : p[b];
                    const bool lo = q > 0, hi = q + 1 < ext[b];
                    const float vlo = a.ek[c - (lo ? st[b] : 0)], vc = a.ek[c], vhi = a.ek[c + (hi ? st[b] : 0)];
                    float m = lo ? vlo : vc;   // first minimum, scan low -> high, strict <
                    int am_ = lo ? -1 : 0;
                    if (vc < m) {
                        m = vc;
                        am_ = 0;
                    }
                    if (hi && vhi < m) {
                        m = vhi;
                        am_ = 1;
                    }
                    pm[b] = m;
                    am[b] = am_;
                }
                const float share = erode_share(pm[0], pm[1], pm[2], a.tgrad[c], ax);
                if (cin && am[ax] == -d) s += share;
            }
            de += s;
        }
        if (LAST) de += a.coef[0] + a.coef[1] * a.gt[i] + a.coef[2] * a.st[i];
        a.de_out[i] = de;
    }
}

// ------------------------------------------------------------------------------------------
// Fused step: the probability field of one term and its gradient chained into d(loss)/d(logits)
// ------------------------------------------------------------------------------------------
struct TermArgs {
    const float* logits;  // (B, n, 5)
    const float* target;  // (B, n), > 0 = foreground
    const float* baked;   // (B, 3, n)
    long long n;
    int B, Y, Z, term;
    float scale[3];
    float inv_var[3];
};

__device__ inline float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

// embedding probability of loss_reduce_kernel (train.hip): E = index + tanh(l)*scale, exp(sum (E - S)^2 * inv_var)
__device__ inline float term_embed(const TermArgs& a, int b, long long i, const float* l, float* dmin, float* v) {
    const int z = (int)(i % a.Z);
    const long long t = i / a.Z;
    const int y = (int)(t % a.Y);
    const int x = (int)(t / a.Y);
    const float idx[3] = {(float)x, (float)y, (float)z};
    float ssum = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = tanhf(l[k]);
        const float e = idx[k] + v[k] * a.scale[k];
        dmin[k] = e - a.baked[((long long)b * 3 + k) * a.n + i];
        ssum += (dmin[k] * dmin[k]) * a.inv_var[k];
    }
    return expf(ssum);
}

__global__ void __launch_bounds__(256) cld_term_field_kernel(TermArgs a, float* __restrict__ prob, float* __restrict__ gt) {
    const long long N = a.n * a.B;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < N; j += (long long)gridDim.x * 256) {
        const int b = (int)(j / a.n);
        const long long i = j - (long long)b * a.n;
        const float* l = a.logits + j * 5;
        float d[3], v[3];
        prob[j] = a.term == 0 ? term_embed(a, b, i, l, d, v) : sigmoid_(l[a.term == 1 ? 4 : 3]);
        gt[j] = a.target[j] > 0.0f ? 1.0f : 0.0f;
    }
}

__global__ void __launch_bounds__(256) cld_chain_kernel(TermArgs a, float weight, const float* __restrict__ dprob,
                                                        float* __restrict__ dlogits) {
    const long long N = a.n * a.B;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < N; j += (long long)gridDim.x * 256) {
        const float* l = a.logits + j * 5;
        float* o = dlogits + j * 5;
        const float dp = weight * dprob[j];
        if (a.term == 0) {
            const int b = (int)(j / a.n);
            float d[3], v[3];
            const float pe = term_embed(a, b, j - (long long)b * a.n, l, d, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] += dp * pe * (2.0f * d[k] * a.inv_var[k]) * a.scale[k] * (1.0f - v[k] * v[k]);
        } else {
            const int c = a.term == 1 ? 4 : 3;
            const float p = sigmoid_(l[c]);
            o[c] += dp * p * (1.0f - p);
        }
    }
}

__global__ void cld_chain_loss_kernel(int term, float weight, const float* __restrict__ term_loss, float* __restrict__ losses) {
    if (threadIdx.x == 0) {
        losses[term] = term_loss[0];
        losses[3] = losses[3] + weight * term_loss[0];
    }
}

int fill_term_args(TermArgs& a, const float* logits, const float* target, const float* baked, int B, int X, int Y, int Z,
                   const float* scale_host, const float* sigma_host, int term) {
    a.logits = logits;
    a.target = target;
    a.baked = baked;
    a.n = (long long)X * Y * Z;
    a.B = B;
    a.Y = Y;
    a.Z = Z;
    a.term = term;
    for (int k = 0; k < 3; ++k) {
        a.scale[k] = scale_host[k];
        const float s = sigma_host[k] + 1e-16f;  // as fill_loss_args (train.hip)
        a.inv_var[k] = 1.0f / (s * s * 2.0f * -1.0f);
    }
    return 0;
}

bool geo_ok(int B, int X, int Y, int Z) { return B >= 1 && X >= 1 && Y >= 1 && Z >= 1; }

Geo make_geo(int B, int X, int Y, int Z) {
    Geo g;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    g.sx = (long long)Y * Z;
    g.N = (long long)B * X * Y * Z;
    return g;
}

}  // namespace

extern "C" {

int64_t sk_train_soft_skeleton_workspace_floats(int B, int X, int Y, int Z) {
    return 2 * (int64_t)B * X * Y * Z;
}

int sk_train_soft_skeleton(const float* img, float* skel, int B, int X, int Y, int Z, int iter, float* workspace,
                           void* stream) {
    SK_CHECK_ARG(img && skel && workspace, "sk_train_soft_skeleton: NULL pointer");
    SK_CHECK_ARG(geo_ok(B, X, Y, Z), "sk_train_soft_skeleton: bad extents B=%d X=%d Y=%d Z=%d", B, X, Y, Z);
    SK_CHECK_ARG(iter >= 0 && iter <= SK_CLDICE_MAX_ITER, "sk_train_soft_skeleton: iter=%d outside [0, %d]", iter,
                 SK_CLDICE_MAX_ITER);
    const Geo g = make_geo(B, X, Y, Z);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = sk::stream_grid(g.N, 256);
    for (int k = 0; k <= iter; ++k) {
        FwdSide s{};
        s.e = k == 0 ? img : workspace + (long long)((k - 1) & 1) * g.N;
        s.e1 = workspace + (long long)(k & 1) * g.N;
        s.sp = k == 0 ? nullptr : skel;
        s.sn = skel;
        cld_erode_kernel<1><<<grid, 256, 0, st>>>(g, s, s);
        SK_CHECK_LAUNCH();
        cld_skel_kernel<1, false><<<grid, 256, 0, st>>>(g, s, s, nullptr, nullptr, nullptr);
        SK_CHECK_LAUNCH();
    }
    return SK_OK;
}

int64_t sk_train_soft_dice_cldice_workspace_floats(int B, int X, int Y, int Z, int iter) {
    const int64_t N = (int64_t)B * X * Y * Z;
    const int64_t nblk = sk::stream_grid(N, 256);
    // e_1..e_{iter+1}, skel_0..skel_iter (prediction); 2 ping-pong e + S_t (ground truth; the ping-pong pair holds
    // dL/dskel in the backward); dopen, direct, T; the arg-max codes (bytes); partials; coefficients
    return (int64_t)(2 * (iter + 1) + 6) * N + (N + 3) / 4 + nblk * kCldSums + kCldCoef;
}

int sk_train_soft_dice_cldice(const float* pred, const float* gt, int B, int X, int Y, int Z, int iter, float alpha,
                              float smooth, float* loss, float* dpred, float* workspace, void* stream) {
    SK_CHECK_ARG(pred && gt && loss && workspace, "sk_train_soft_dice_cldice: NULL pointer");
    SK_CHECK_ARG(geo_ok(B, X, Y, Z), "sk_train_soft_dice_cldice: bad extents B=%d X=%d Y=%d Z=%d", B, X, Y, Z);
    SK_CHECK_ARG(iter >= 0 && iter <= SK_CLDICE_MAX_ITER, "sk_train_soft_dice_cldice: iter=%d outside [0, %d]", iter,
                 SK_CLDICE_MAX_ITER);
    SK_CHECK_ARG(std::isfinite(alpha) && std::isfinite(smooth), "sk_train_soft_dice_cldice: alpha and smooth must be finite");
    SK_CHECK_ARG(dpred != pred && dpred != gt, "sk_train_soft_dice_cldice: dpred must not alias an input");
    const Geo g = make_geo(B, X, Y, Z);
    const long long N = g.N;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = sk::stream_grid(N, 256);
    float* E = workspace;                              // E + (j-1) N = e_j, j = 1..iter+1
    float* S = E + (long long)(iter + 1) * N;          // S + j N = skel_j, j = 0..iter
    float* G2 = S + (long long)(iter + 1) * N;         // ground truth e ping-pong; backward: dL/dskel ping-pong
    float* ST = G2 + 2 * N;
    float* dopen = ST + N;
    float* direct = dopen + N;
    float* tgrad = direct + N;
    unsigned char* code = (unsigned char*)(tgrad + N);
    float* partial = tgrad + N + (N + 3) / 4;
    float* coef = partial + (long long)grid * kCldSums;

    for (int k = 0; k <= iter; ++k) {
        FwdSide sp{}, sg{};
        sp.e = k == 0 ? pred : E + (long long)(k - 1) * N;
        sp.e1 = E + (long long)k * N;
        sp.sp = k == 0 ? nullptr : S + (long long)(k - 1) * N;
        sp.sn = S + (long long)k * N;
        sg.e = k == 0 ? gt : G2 + (long long)((k - 1) & 1) * N;
        sg.e1 = G2 + (long long)(k & 1) * N;
        sg.sp = k == 0 ? nullptr : ST;
        sg.sn = ST;
        cld_erode_kernel<2><<<grid, 256, 0, st>>>(g, sp, sg);
        SK_CHECK_LAUNCH();
        if (k < iter)
            cld_skel_kernel<2, false><<<grid, 256, 0, st>>>(g, sp, sg, nullptr, nullptr, nullptr);
        else
            cld_skel_kernel<2, true><<<grid, 256, 0, st>>>(g, sp, sg, pred, gt, partial);
        SK_CHECK_LAUNCH();
    }
    cld_finalize_kernel<<<1, 256, 0, st>>>(partial, (int)grid, (double)alpha, (double)smooth, loss, coef);
    SK_CHECK_LAUNCH();
    if (!dpred) return SK_OK;

    // backward: dpred doubles as dL/de_k between the levels (written by level k's B3, read by level k-1's B2)
    for (int k = iter; k >= 0; --k) {
        BwdArgs a{};
        a.ek = k == 0 ? pred : E + (long long)(k - 1) * N;
        a.ek1 = E + (long long)k * N;
        a.sprev = k == 0 ? nullptr : S + (long long)(k - 1) * N;
        a.gs_in = k == iter ? nullptr : G2 + (long long)((k + 1) & 1) * N;
        a.gs_out = G2 + (long long)(k & 1) * N;
        a.gt = gt;
        a.st = ST;
        a.coef = coef;
        a.dopen = dopen;
        a.direct = direct;
        a.code = code;
        a.de_up = k == iter ? nullptr : dpred;
        a.tgrad = tgrad;
        a.de_out = dpred;
        cld_bwd_point_kernel<<<grid, 256, 0, st>>>(g, a);
        SK_CHECK_LAUNCH();
        cld_bwd_dilate_kernel<<<grid, 256, 0, st>>>(g, a);
        SK_CHECK_LAUNCH();
        if (k == 0)
            cld_bwd_erode_kernel<true><<<grid, 256, 0, st>>>(g, a);
        else
            cld_bwd_erode_kernel<false><<<grid, 256, 0, st>>>(g, a);
        SK_CHECK_LAUNCH();
    }
    return SK_OK;
}

int sk_train_cldice_term_field(const float* logits, const float* target, const float* baked, int B, int X, int Y, int Z,
                               const float* vector_scale_host, const float* sigma_host, int term, float* prob, float* gt,
                               void* stream) {
    SK_CHECK_ARG(logits && target && prob && gt && vector_scale_host && sigma_host, "sk_train_cldice_term_field: NULL pointer");
    SK_CHECK_ARG(term >= 0 && term <= 2 && (term != 0 || baked), "sk_train_cldice_term_field: bad term %d", term);
    SK_CHECK_ARG(geo_ok(B, X, Y, Z), "sk_train_cldice_term_field: bad extents");
    TermArgs a{};
    fill_term_args(a, logits, target, baked, B, X, Y, Z, vector_scale_host, sigma_host, term);
    cld_term_field_kernel<<<sk::stream_grid(a.n * B, 256), 256, 0, (hipStream_t)stream>>>(a, prob, gt);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_train_cldice_chain(const float* logits, const float* baked, int B, int X, int Y, int Z,
                          const float* vector_scale_host, const float* sigma_host, int term, float weight,
                          const float* dprob, const float* term_loss, float* losses, float* dlogits, void* stream) {
    SK_CHECK_ARG(logits && term_loss && losses && vector_scale_host && sigma_host, "sk_train_cldice_chain: NULL pointer");
    SK_CHECK_ARG(term >= 0 && term <= 2 && (term != 0 || baked), "sk_train_cldice_chain: bad term %d", term);
    SK_CHECK_ARG(geo_ok(B, X, Y, Z), "sk_train_cldice_chain: bad extents");
    SK_CHECK_ARG(!dlogits == !dprob, "sk_train_cldice_chain: dlogits and dprob go together");
    hipStream_t st = (hipStream_t)stream;
    if (dlogits) {
        TermArgs a{};
        fill_term_args(a, logits, nullptr, baked, B, X, Y, Z, vector_scale_host, sigma_host, term);
        cld_chain_kernel<<<sk::stream_grid(a.n * B, 256), 256, 0, st>>>(a, weight, dprob, dlogits);
        SK_CHECK_LAUNCH();
    }
    cld_chain_loss_kernel<<<1, 64, 0, st>>>(term, weight, term_loss, losses);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
