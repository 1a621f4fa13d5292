// Stage-1 tail of skoots.lib.eval.eval(): gate, dilate, threshold, interior scatter.
//
// Replaces (reference file:line)
//   skoots/lib/eval.py:145-150      channel split + gating by prob > 0.8
//   skoots/lib/morphology.py:155-199 binary_dilation (3x3x3 max) + 2x binary_dilation_2d
//                                   (3x3x1 max), called at eval.py:152-157
//   skoots/lib/eval.py:160-176      interior crop scatter, skeleton > 0.8
//
// The reference materialises 3 x 27-channel one-hot conv3d outputs (194 MB fp32 per
// call).  Max filters commute with the final threshold and compose to one box of
// radius (3,3,1), zero padded at the tile faces, so the whole thing is a separable
// OR over a byte mask staged in LDS: HBM traffic is one read of channels 3,4 around
// the interior, one read of channels 0..2 on the interior, and the interior writes.
#include "common.h"

namespace {

constexpr int kMaxTiles = 16;

struct TileGeom {
    long long off;        // element offset of this tile's (channel 0, 0, 0, 0) in out5
    int ox, oy, oz;       // tile origin in the volume
    int lx, ly, lz;       // write box (tile-local, inside the interior): [l, h)
    int hx, hy, hz;
    int nbx, nblocks;     // patch grid of this tile
};

struct GateGeom {
    int w, h, d;          // tile extents
    long long sc, sx, sy; // element strides of out5: channel, x, y (z is contiguous)
    int X, Y, Z;          // volume extents
    int px, py;           // interior patch handled per block
    float prob_thr, skel_thr;
    int ntiles;
    TileGeom t[kMaxTiles];
};

template <typename T>
__device__ __forceinline__ float ld(const T* p, long long i);
template <>
__device__ __forceinline__ float ld<__half>(const __half* p, long long i) {
    return __half2float(p[i]);
}
template <>
__device__ __forceinline__ float ld<float>(const float* p, long long i) {
    return p[i];
}

constexpr int RX = 3, RY = 3;  // 1+1+1 in x,y (eval.py:152-157); z radius 1 is hard-wired in phase 2

template <typename T>
__global__ void __launch_bounds__(256)
gate_dilate_scatter_kernel(const T* __restrict__ out5_all, GateGeom g, uint2* __restrict__ vec4,
                           __half* __restrict__ vec_planar, uint8_t* __restrict__ skeleton) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TileGeom tg = g.t[blockIdx.y];
    if ((int)blockIdx.x >= tg.nblocks) return;  // grid.x is sized for the largest write box
    const T* out5 = out5_all + tg.off;
    const int bx = blockIdx.x % tg.nbx, by = blockIdx.x / tg.nbx;
    const int x0 = tg.lx + bx * g.px, y0 = tg.ly + by * g.py;  // tile-local patch origin
    const int sx = g.px + 2 * RX, sy = g.py + 2 * RY;          // staged columns
    const int d = g.d;
    unsigned char* m0 = smem;                      // [sx][sy][d]
    unsigned char* m1 = smem + (size_t)sx * sy * d;  // [sx][sy][d]
    const long long plane = g.sc;
    const int tid = threadIdx.x, nth = blockDim.x;

    // phase 1: mask = skel > skel_thr && prob > prob_thr, zero outside the tile
    for (int i = tid; i < sx * sy * d; i += nth) {
        int z = i % d;
        int c = i / d;
        int ly = c % sy, lx = c / sy;
        int tx = x0 - RX + lx, ty = y0 - RY + ly;
        unsigned char m = 0;
        if (tx >= 0 && tx < g.w && ty >= 0 && ty < g.h) {
            long long o = (long long)tx * g.sx + (long long)ty * g.sy + z;
            float skel = ld(out5, 3 * plane + o);
            float prob = ld(out5, 4 * plane + o);
            m = (prob > g.prob_thr && skel > g.skel_thr) ? 1 : 0;
        }
        m0[i] = m;
    }
    __syncthreads();
    // phase 2: z dilation (radius 1), zero padded at the tile faces
    for (int i = tid; i < sx * sy * d; i += nth) {
        int z = i % d;
        unsigned char m = m0[i];
        if (z > 0) m |= m0[i - 1];
        if (z + 1 < d) m |= m0[i + 1];
        m1[i] = m;
    }
    __syncthreads();
    // phase 3: y dilation (radius 3) for the columns the x pass needs -> m0[sx][py][d]
    for (int i = tid; i < sx * g.py * d; i += nth) {
        int z = i % d;
        int c = i / d;
        int ly = c % g.py, lx = c / g.py;
        unsigned char m = 0;
#pragma unroll
        for (int k = 0; k <= 2 * RY; ++k) m |= m1[((size_t)lx * sy + ly + k) * d + z];
        m0[i] = m;
    }
    __syncthreads();
    // phase 4: x dilation (radius 3) + scatter of the interior
    const int iz0 = tg.lz, iz1 = tg.hz;
    const int idp = iz1 - iz0;
    for (int i = tid; i < g.px * g.py * idp; i += nth) {
        int zz = i % idp;
        int c = i / idp;
        int ly = c % g.py, lx = c / g.py;
        int tx = x0 + lx, ty = y0 + ly, tz = iz0 + zz;
        if (tx >= tg.hx || ty >= tg.hy) continue;
        unsigned char m = 0;
#pragma unroll
        for (int k = 0; k <= 2 * RX; ++k) m |= m0[((size_t)(lx + k) * g.py + ly) * d + tz];
        long long vo = ((long long)(tg.ox + tx) * g.Y + (tg.oy + ty)) * g.Z + (tg.oz + tz);
        skeleton[vo] = m;
        // vectors: vec * (prob > thr), stored fp16 (eval.py:149,175)
        long long o = (long long)tx * g.sx + (long long)ty * g.sy + tz;
        bool gate = ld(out5, 4 * plane + o) > g.prob_thr;
        float v0 = ld(out5, o), v1 = ld(out5, plane + o), v2 = ld(out5, 2 * plane + o);
        if (!gate) {
            v0 = copysignf(0.0f, v0);
            v1 = copysignf(0.0f, v1);
            v2 = copysignf(0.0f, v2);
        }
        __half h0 = __float2half_rn(v0), h1 = __float2half_rn(v1), h2 = __float2half_rn(v2);
        if (vec4) {
            __half2 lo = __halves2half2(h0, h1);
            __half2 hi = __halves2half2(h2, __ushort_as_half(0));
            uint2 r;
            r.x = *reinterpret_cast<unsigned*>(&lo);
            r.y = *reinterpret_cast<unsigned*>(&hi);
            vec4[vo] = r;
        }
        if (vec_planar) {
            long long nv = (long long)g.X * g.Y * g.Z;
            vec_planar[vo] = h0;
            vec_planar[vo + nv] = h1;
            vec_planar[vo + 2 * nv] = h2;
        }
    }
}

// ---- d <= 32: one 32-bit mask word per staged column --------------------------------------------
// A column (x, y) of the tile has at most 32 voxels, so its mask is one word: bit z = voxel z.  The z
// dilation is two shifts, the y and x dilations are ORs of 7 neighbouring words, and the per-voxel
// phases of the kernel above (each with its own % and /) become per-column phases.  Work is handed out
// in quads: four z-neighbours that start at a multiple of 4, which is 8 aligned bytes of an fp16 row.
constexpr int PX = 16, PY = 16;                      // interior patch of a block
constexpr int SXW = PX + 2 * RX, SYW = PY + 2 * RY;  // staged columns

// Four fp16 values held in 8 bytes, as floats.
__device__ __forceinline__ void unpack_quad(uint2 r, float v[4]) {
    __half2 a = *reinterpret_cast<__half2*>(&r.x), b = *reinterpret_cast<__half2*>(&r.y);
    v[0] = __low2float(a);
    v[1] = __high2float(a);
    v[2] = __low2float(b);
    v[3] = __high2float(b);
}
// Four z-neighbours of one plane as floats.  VEC: one 8-byte load (fp16 rows whose quads are 8-byte
// aligned and whole); otherwise n <= 4 scalar loads, the rest reads as 0.
template <typename T, bool VEC>
__device__ __forceinline__ void load_quad(const T* p, int n, float v[4]) {
    if constexpr (VEC) {
        unpack_quad(*reinterpret_cast<const uint2*>(p), v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? ld(p, k) : 0.0f;
    }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
gate_dilate_scatter_words_kernel(const T* __restrict__ out5_all, GateGeom g, uint2* __restrict__ vec4,
                                 __half* __restrict__ vec_planar, uint8_t* __restrict__ skeleton) {
    __shared__ unsigned w0[SXW * SYW];  // gate mask of every staged column
    __shared__ unsigned w1[SXW * PY];   // after the y dilation
    const TileGeom tg = g.t[blockIdx.y];
    if ((int)blockIdx.x >= tg.nblocks) return;  // grid.x is sized for the largest write box
    const T* out5 = out5_all + tg.off;
    const int bx = blockIdx.x % tg.nbx, by = blockIdx.x / tg.nbx;
    const int x0 = tg.lx + bx * PX, y0 = tg.ly + by * PY;  // tile-local patch origin
    const int d = g.d;
    const long long plane = g.sc;
    const int tid = threadIdx.x, nth = blockDim.x;   // nth = PX * PY: thread tid scatters items tid + nth k, k < nq3

    // What phase 3 reads does not depend on the mask.  With 8-byte quads the first kPre items of a thread are
    // requested here, ahead of phase 1, so that a block waits for memory once and not twice.
    constexpr int kPre = VEC ? 3 : 0;
    const int q3 = tg.lz >> 2, nq3 = ((tg.hz + 3) >> 2) - q3;   // the quads that hold planes [lz, hz)
    uint2 pre[kPre ? kPre : 1][4];
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int i = tid + k * (PX * PY);
            const int c = i / nq3;
            const int tx = x0 + c / PY, ty = y0 + c % PY;
#pragma unroll
            for (int j = 0; j < 4; ++j) pre[k][j] = make_uint2(0, 0);
            if (k < nq3 && tx < tg.hx && ty < tg.hy) {
                const T* p = out5 + (long long)tx * g.sx + (long long)ty * g.sy + 4 * (q3 + i % nq3);
                pre[k][0] = *reinterpret_cast<const uint2*>(p);
                pre[k][1] = *reinterpret_cast<const uint2*>(p + plane);
                pre[k][2] = *reinterpret_cast<const uint2*>(p + 2 * plane);
                pre[k][3] = *reinterpret_cast<const uint2*>(p + 4 * plane);
            }
        }
    }

    for (int i = tid; i < SXW * SYW; i += nth) w0[i] = 0;
    __syncthreads();
    // phase 1: bit z of a column = skel > skel_thr && prob > prob_thr; columns outside the tile stay 0.
    // The written planes [lz, hz) see bits lz-1 .. hz only, so only the quads that hold those are read.
    {
        const int q0 = max(tg.lz - 1, 0) >> 2, nq = ((min(tg.hz + 1, d) + 3) >> 2) - q0;
        for (int i = tid; i < SXW * SYW * nq; i += nth) {
            int q = q0 + i % nq;
            int c = i / nq;
            int ly = c % SYW, lx = c / SYW;
            int tx = x0 - RX + lx, ty = y0 - RY + ly;
            if (tx < 0 || tx >= g.w || ty < 0 || ty >= g.h) continue;
            long long o = (long long)tx * g.sx + (long long)ty * g.sy + 4 * q;
            float skel[4], prob[4];
            load_quad<T, VEC>(out5 + 3 * plane + o, d - 4 * q, skel);
            load_quad<T, VEC>(out5 + 4 * plane + o, d - 4 * q, prob);
            unsigned bits = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < d && prob[k] > g.prob_thr && skel[k] > g.skel_thr) bits |= 1u << k;
            if (bits) atomicOr(&w0[c], bits << (4 * q));
        }
    }
    __syncthreads();
    // phase 2: y dilation (radius 3) for the columns the x pass needs -> w1[SXW][PY]
    for (int i = tid; i < SXW * PY; i += nth) {
        int ly = i % PY, lx = i / PY;
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k <= 2 * RY; ++k) m |= w0[lx * SYW + ly + k];
        w1[i] = m;
    }
    __syncthreads();
    // phase 3: x dilation (radius 3), z dilation (radius 1, zero padded at the tile faces: bits shifted
    // out of [0, d) are dropped) and the scatter of the interior, one quad of one column per thread
    const unsigned dmask = d >= 32 ? 0xffffffffu : (1u << d) - 1u;
    const long long nv = (long long)g.X * g.Y * g.Z;
    auto scatter_item = [&](int i, const uint2* raw) {   // raw: the item's four quads as requested above, or NULL
        int q = q3 + i % nq3;
        int c = i / nq3;
        int ly = c % PY, lx = c / PY;
        int tx = x0 + lx, ty = y0 + ly, z0 = 4 * q;
        if (tx >= tg.hx || ty >= tg.hy) return;
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k <= 2 * RX; ++k) m |= w1[(lx + k) * PY + ly];
        m = (m | (m << 1) | (m >> 1)) & dmask;
        // vectors: vec * (prob > thr), stored fp16 (eval.py:149,175)
        long long o = (long long)tx * g.sx + (long long)ty * g.sy + z0;
        float v0[4], v1[4], v2[4], prob[4];
        if (raw) {
            unpack_quad(raw[0], v0);
            unpack_quad(raw[1], v1);
            unpack_quad(raw[2], v2);
            unpack_quad(raw[3], prob);
        } else {
            load_quad<T, VEC>(out5 + o, d - z0, v0);
            load_quad<T, VEC>(out5 + plane + o, d - z0, v1);
            load_quad<T, VEC>(out5 + 2 * plane + o, d - z0, v2);
            load_quad<T, VEC>(out5 + 4 * plane + o, d - z0, prob);
        }
        bool ok[4];
        unsigned short h[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = z0 + k >= tg.lz && z0 + k < tg.hz;
            bool gate = prob[k] > g.prob_thr;
            h[0][k] = __half_as_ushort(__float2half_rn(gate ? v0[k] : copysignf(0.0f, v0[k])));
            h[1][k] = __half_as_ushort(__float2half_rn(gate ? v1[k] : copysignf(0.0f, v1[k])));
            h[2][k] = __half_as_ushort(__float2half_rn(gate ? v2[k] : copysignf(0.0f, v2[k])));
        }
        const bool all = ok[0] && ok[1] && ok[2] && ok[3];
        const long long vo = ((long long)(tg.ox + tx) * g.Y + (tg.oy + ty)) * g.Z + (tg.oz + z0);
        // every run below is contiguous in z: the widest store its address allows, else one per voxel
        uint8_t* sp = skeleton + vo;
        if (all && (reinterpret_cast<uintptr_t>(sp) & 3) == 0) {
            *reinterpret_cast<unsigned*>(sp) = ((m >> z0) & 1u) | ((m >> (z0 + 1)) & 1u) << 8 |
                                               ((m >> (z0 + 2)) & 1u) << 16 | ((m >> (z0 + 3)) & 1u) << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) sp[k] = (m >> (z0 + k)) & 1u;
        }
        if (vec4) {
            uint2* vp = vec4 + vo;
            uint2 r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = make_uint2(h[0][k] | (unsigned)h[1][k] << 16, h[2][k]);
            auto one = [&](int k) {
                if (ok[k]) vp[k] = r[k];
            };
            auto two = [&](int k) {  // vp + k is 16-byte aligned
                if (ok[k] && ok[k + 1])
                    *reinterpret_cast<uint4*>(vp + k) = make_uint4(r[k].x, r[k].y, r[k + 1].x, r[k + 1].y);
                else {
                    one(k);
                    one(k + 1);
                }
            };
            if ((reinterpret_cast<uintptr_t>(vp) & 15) == 0) {
                two(0);
                two(2);
            } else {
                one(0);
                two(1);
                one(3);
            }
        }
        if (vec_planar) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                __half* pp = vec_planar + vo + ch * nv;
                if (all && (reinterpret_cast<uintptr_t>(pp) & 7) == 0) {
                    *reinterpret_cast<uint2*>(pp) = make_uint2(h[ch][0] | (unsigned)h[ch][1] << 16,
                                                               h[ch][2] | (unsigned)h[ch][3] << 16);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ok[k]) pp[k] = __ushort_as_half(h[ch][k]);
                }
            }
        }
    };
#pragma unroll
    for (int k = 0; k < kPre; ++k)
        if (k < nq3) scatter_item(tid + k * (PX * PY), pre[k]);
    for (int k = kPre; k < nq3; ++k) scatter_item(tid + k * (PX * PY), nullptr);
}

// Library max filter (binary_dilation / binary_dilation_2d on arbitrary fp32 maps).
__global__ void __launch_bounds__(256) max_filter_kernel(const float* __restrict__ in,
                                                         float* __restrict__ out, int w, int h,
                                                         int d, int rx, int ry, int rz) {
    long long n = (long long)w * h * d;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int z = (int)(i % d);
    long long c = i / d;
    int y = (int)(c % h), x = (int)(c / h);
    // zero padding: out-of-bounds taps contribute 0.0 (morphology.py:170-175)
    bool clipped = (x - rx < 0) || (x + rx >= w) || (y - ry < 0) || (y + ry >= h) || (z - rz < 0) ||
                   (z + rz >= d);
    float m = clipped ? 0.0f : -INFINITY;
    bool any = clipped;
    for (int dx = -rx; dx <= rx; ++dx) {
        int xx = x + dx;
        if (xx < 0 || xx >= w) continue;
        for (int dy = -ry; dy <= ry; ++dy) {
            int yy = y + dy;
            if (yy < 0 || yy >= h) continue;
            for (int dz = -rz; dz <= rz; ++dz) {
                int zz = z + dz;
                if (zz < 0 || zz >= d) continue;
                float v = in[((long long)xx * h + yy) * d + zz];
                m = any ? fmaxf(m, v) : v;
                any = true;
            }
        }
    }
    out[i] = m;
}

}  // namespace

extern "C" {

int sk_gate_dilate_scatter(const void* out5, int out_dtype, int n_tiles, const int64_t* tile_offsets_host,
                           int64_t stride_c, int64_t stride_x, int64_t stride_y, int w, int h, int d,
                           const int* origins_host, const int* box_lo_host, const int* box_hi_host,
                           void* vec4, void* vec_planar, uint8_t* skeleton, int X, int Y, int Z,
                           float prob_thr, float skel_thr, void* stream) {
    SK_CHECK_ARG(out5 && skeleton && tile_offsets_host && origins_host && box_lo_host && box_hi_host,
                 "sk_gate_dilate_scatter: NULL pointer");
    SK_CHECK_ARG(out_dtype == SK_F16 || out_dtype == SK_F32,
                 "sk_gate_dilate_scatter: out dtype must be fp16 or fp32");
    SK_CHECK_ARG(n_tiles >= 1 && n_tiles <= kMaxTiles, "sk_gate_dilate_scatter: 1..%d tiles per call", kMaxTiles);
    SK_CHECK_ARG(w > 0 && h > 0 && d > 0 && stride_y >= d && stride_x >= stride_y && stride_c > 0,
                 "sk_gate_dilate_scatter: bad tile extents / strides");
    GateGeom g{};
    g.w = w;
    g.h = h;
    g.d = d;
    g.sc = stride_c;
    g.sx = stride_x;
    g.sy = stride_y;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    g.px = g.py = 16;
    g.prob_thr = prob_thr;
    g.skel_thr = skel_thr;
    g.ntiles = n_tiles;
    size_t lds = 2ull * (g.px + 2 * RX) * (g.py + 2 * RY) * d;
    if (lds > 64 * 1024) {
        g.px = g.py = 8;
        lds = 2ull * (g.px + 2 * RX) * (g.py + 2 * RY) * d;
    }
    SK_CHECK_ARG(lds <= 96 * 1024, "sk_gate_dilate_scatter: tile depth %d too large", d);
    int max_blocks = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const int* lo = box_lo_host + 3 * i;
        const int* hi = box_hi_host + 3 * i;
        const int* org = origins_host + 3 * i;
        SK_CHECK_ARG(0 <= lo[0] && lo[0] < hi[0] && hi[0] <= w && 0 <= lo[1] && lo[1] < hi[1] && hi[1] <= h &&
                         0 <= lo[2] && lo[2] < hi[2] && hi[2] <= d,
                     "sk_gate_dilate_scatter: write box [%d:%d,%d:%d,%d:%d) must be a non-empty box inside the "
                     "tile (%d,%d,%d)", lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], w, h, d);
        SK_CHECK_ARG(org[0] >= 0 && org[1] >= 0 && org[2] >= 0 && org[0] + w <= X && org[1] + h <= Y &&
                         org[2] + d <= Z,
                     "sk_gate_dilate_scatter: tile [%d+%d,%d+%d,%d+%d) outside volume (%d,%d,%d)", org[0], w,
                     org[1], h, org[2], d, X, Y, Z);
        TileGeom& t = g.t[i];
        t.off = tile_offsets_host[i];
        t.ox = org[0];
        t.oy = org[1];
        t.oz = org[2];
        t.lx = lo[0];
        t.ly = lo[1];
        t.lz = lo[2];
        t.hx = hi[0];
        t.hy = hi[1];
        t.hz = hi[2];
        t.nbx = (hi[0] - lo[0] + g.px - 1) / g.px;
        t.nblocks = t.nbx * ((hi[1] - lo[1] + g.py - 1) / g.py);
        if (t.nblocks > max_blocks) max_blocks = t.nblocks;
    }
    dim3 grid(max_blocks, n_tiles);
    if (d <= 32) {  // mask words; px = py = 16 holds here (lds above is at most 31 KiB)
        // 8-byte quad loads need fp16 rows made of whole, 8-byte aligned quads
        bool vec = out_dtype == SK_F16 && d % 4 == 0 && stride_c % 4 == 0 && stride_x % 4 == 0 &&
                   stride_y % 4 == 0 && reinterpret_cast<uintptr_t>(out5) % 8 == 0;
        for (int i = 0; i < n_tiles; ++i) vec = vec && tile_offsets_host[i] % 4 == 0;
        if (out_dtype == SK_F32)
            gate_dilate_scatter_words_kernel<float, false><<<grid, 256, 0, (hipStream_t)stream>>>(
                (const float*)out5, g, (uint2*)vec4, (__half*)vec_planar, skeleton);
        else if (vec)
            gate_dilate_scatter_words_kernel<__half, true><<<grid, 256, 0, (hipStream_t)stream>>>(
                (const __half*)out5, g, (uint2*)vec4, (__half*)vec_planar, skeleton);
        else
            gate_dilate_scatter_words_kernel<__half, false><<<grid, 256, 0, (hipStream_t)stream>>>(
                (const __half*)out5, g, (uint2*)vec4, (__half*)vec_planar, skeleton);
    } else if (out_dtype == SK_F16) {
        if (lds > 48 * 1024)
            SK_CHECK_HIP(hipFuncSetAttribute((const void*)gate_dilate_scatter_kernel<__half>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        gate_dilate_scatter_kernel<__half><<<grid, 256, lds, (hipStream_t)stream>>>(
            (const __half*)out5, g, (uint2*)vec4, (__half*)vec_planar, skeleton);
    } else {
        if (lds > 48 * 1024)
            SK_CHECK_HIP(hipFuncSetAttribute((const void*)gate_dilate_scatter_kernel<float>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        gate_dilate_scatter_kernel<float><<<grid, 256, lds, (hipStream_t)stream>>>(
            (const float*)out5, g, (uint2*)vec4, (__half*)vec_planar, skeleton);
    }
    SK_CHECK_LAUNCH();
    return SK_OK;
}

int sk_max_filter3d(const float* in, float* out, int w, int h, int d, int rx, int ry, int rz,
                    void* stream) {
    SK_CHECK_ARG(in && out && in != out, "sk_max_filter3d: bad pointers");
    SK_CHECK_ARG(w > 0 && h > 0 && d > 0 && rx >= 0 && ry >= 0 && rz >= 0,
                 "sk_max_filter3d: bad extents");
    long long n = (long long)w * h * d;
    max_filter_kernel<<<sk::cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(in, out, w, h, d, rx, ry, rz);
    SK_CHECK_LAUNCH();
    return SK_OK;
}

}  // extern "C"
