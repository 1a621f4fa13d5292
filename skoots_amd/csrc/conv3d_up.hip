// Decoder 3x3x3 convolution over torch.cat([skip, interpolate(x, scale 2, nearest)]) with the nearest-neighbour
// upsample FOLDED INTO THE WEIGHTS of the upsampled half -- same result as sk_conv3d with an upsampled second source,
// 35 % fewer matrix instructions.
//
// Replaces the first conv of each decoder level of the network that skoots/lib/utils.py:17-107 builds (graph:
// oracle/unet_spec.py) and that eval runs at skoots/lib/eval.py:142-143.
//
// Why it folds.  U[x] = L[x >> 1].  Along one axis an output voxel of parity p reads U at x-1, x, x+1, i.e.
//   p = 0 (x = 2m):     L[m-1], L[m], L[m]     ->  w[-1] L[m-1] + (w[0] + w[+1]) L[m]
//   p = 1 (x = 2m + 1): L[m], L[m], L[m+1]     ->  (w[-1] + w[0]) L[m] + w[+1] L[m+1]
// so the 27 taps on U collapse to 2 x 2 x 2 = 8 taps on L with weights that depend on the output voxel's parity class
// (px, py, pz): 8 tap-chunks instead of 27 for the upsampled channels (zero padding of U at the tile faces = zero
// padding of L: the folded sums only ever pair taps that read the same L voxel).  The sums are formed on the host in
// fp32 and rounded to fp16 once (sk_conv3d_pack_weight_upfold_host).
//
// What it costs: the A operand (weights) of an MFMA must be the same for all its voxel columns, so the columns of a
// matrix tile must share (py, pz) and an output plane has one px.  Hence a different voxel -> column map than
// conv3d.hip's: a workgroup owns K whole rows of the LOW-resolution (y, z) plane (K * Zl <= 32 positions) = the
// 2K x Zt fine voxels above them; wave w = parity class (py, pz) = (w >> 1, w & 1) owns the <= 32 fine voxels of that
// class, column m <-> low-resolution position m of the segment.  The staged fine planes are stored DE-INTERLEAVED --
// four sub-planes (y parity, z parity), each linear over (y >> 1, z >> 1) with no z halo -- so that for every tap the 16
// columns of an MFMA read 16 CONSECUTIVE positions (+ a wave-uniform offset): the conflict-free swizzle of
// conv3_m16_kernel carries over unchanged.  z faces: a lane whose tap would wrap into the neighbouring row reads the
// plane's zero position (conv3d.hip's linear mode).  The low-resolution source is staged as it is (4 planes of
// (K + 2) rows) in the ring slots of the fine planes the step is done with; fine planes XS, XS + 1 survive the upsampled
// phases and are planes 0, 1 of the next step (one skip chunk).
//
// 32 output channels per launch on v_mfma_f32_16x16x32_f16 (COUT 64: two launches); B fragments in half-row bodies one
// body ahead, weight rows one (skip chunks; rows 0, 1 from LDS when there is one skip chunk) or two (upsampled chunks)
// rows ahead; everything else (x-marching ring, LDS-DMA through buffer descriptors, permlane epilogue, GroupNorm partials on
// v_dot2c) as in conv3_m16_kernel, whose comments explain those parts.
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <type_traits>
#include <vector>

#include "conv3_device.h"

namespace {

constexpr int kMaxDma = 3;       // LDS-DMA wave-instructions per fine plane per wave (nposp <= 192)
constexpr int kMaxDmaL = 2;      // per low-resolution plane per wave (nposl <= 128)
constexpr int kSkipFrags = 54;   // fragments of a skip chunk: [dydz 9][cout half 2][dx 3]
constexpr int kUpFrags = 128;    // fragments of an upsampled chunk: [class (py,pz) 4][tytz 4][cout half 2][px 2][tx 2]

struct UpfArgs {
    const char* skip;            // (B, Xt, Yt, Zt, skipC) fp16, activated
    const char* up;              // (B, Xt/2, Yt/2, Zt/2, upC) fp16, activated
    long long skip_plane, skip_batch, up_plane, up_batch;   // bytes
    int skipC, upC;
    int ns, nu;                  // 32-channel chunks of the two sources
    const char* wpk;
    const float* bias;
    char* out;
    float* partial;
    int B, Xt, Yt, Zt, Yl, Zl;
    int XC, nxc, npatch;
    int K;                       // low-resolution rows per workgroup
    int SUBP, nposp, nposl;      // positions per fine sub-plane / fine plane / low-resolution plane
    int out_vs, cout_off;        // bytes per output voxel line; first output channel of this launch (a launch computes 32)
    int pstride, poff;           // floats per gn_partial row (cout/4 * 2); offset of this launch's 16 in it
    long long* dbg;              // -DSK_TIMING builds: per-wave phase cycle sums (tools/upfold_phase_timing.py)
    int w8_off, w8_scale, wpk_bytes;   // MIX8: byte offset of the fp8 fragments, E8M0 scale of the weights (x 4), bytes of the image
};

constexpr int kSkipFrags8 = 30;  // MIX8, 2 KiB fp8 fragments of a skip chunk: [tap-row pair 5][cout half 2][dx 3]
constexpr int kUpFrags8 = 64;    // of an upsampled chunk: [class 4][ty 2][cout half 2][px 2][tx 2] (K = two tz taps)

#define SK_UPF_NAME conv3_upf_kernel
#define SK_UPF_MIX8 0
#include "conv3d_up_kernel.inc"
#undef SK_UPF_NAME
#undef SK_UPF_MIX8
#define SK_UPF_NAME conv3_upf_mix8_kernel
#define SK_UPF_MIX8 1
#include "conv3d_up_kernel.inc"
#undef SK_UPF_NAME
#undef SK_UPF_MIX8

// ------------------------------------------------------------------------------------------
// conv3_upf_px_kernel (round 5): the fp16 folded conv of ONE skip chunk and ONE upsampled chunk into 32 channels (dec0.0)
// with conv3_px_kernel's plane streaming.  conv3_upf_kernel streams its weights: per step of four output planes a wave
// issues ~106 vector-memory instructions for 560 MFMAs, 74 of them weight fragments from L2 (the folded set of a parity
// class is 32 fragments per wave, 128 KiB per workgroup: too large to stay).  Here a workgroup computes ONE cout half
// (grid = 2 x npatch x x-chunks x B, the two halves of a region adjacent in the XCD-aware order: the second one's planes
// come from L2), and then every weight stays:
//   * the wave's 16 folded fragments (class (py, pz) = w, this cout half: [tytz 4][px 2][tx 2]) in registers;
//   * the 27 skip fragments of the cout half: tap rows 0 .. RES-1 in registers, the others in LDS (one copy per
//     workgroup, loaded once) -- no weight load in the step loop;
//   * a step consumes fine planes A = 2i, B = 2i + 1 and low-resolution plane i: the fine planes reach output planes
//     A-1 .. B+1 through their x taps, and plane i's four folded (px, tx) taps land in output planes 2i-1 .. 2i+2 -- the
//     SAME four rolling accumulator planes (4 planes x 2 voxel halves x 1 cout half = 32 registers); A-1 and A complete;
//   * the ring: 4 fine slots + 2 low-resolution slots; the next step's planes (2 fine, 1 low-resolution) are requested at
//     the START of the step, into the slots the step before read; one barrier per step;
//   * uniform pair steps: an x-chunk of n planes runs n/2 + 2 steps from fine plane xa - 2; the planes outside
//     [xa - 1, xb] (which reach no stored output plane) and outside the tile are staged as zeros (out-of-range LDS-DMA);
//   * per step and wave 108 skip MFMAs (9 tap rows x 12) + 32 upsampled (4 tap rows x 8); the next row's LDS reads are
//     pinned into the first MFMA gaps of the row before (conv3_px_kernel's finding).
// x-chunks: kUpxChunks consecutive chunks of make_upf_plan per workgroup (fewer half-idle end steps and prologues); the
// GroupNorm partials are still reduced and written per chunk of the plan -- the rows sk_conv3d_upfold_num_blocks reports,
// in conv3_upf_kernel's summation order -- so the finalize pass and its order do not change.
// Summation order of a voxel: by input plane (fine planes and low-resolution planes interleaved), not by tap row: fp32
// rounding differs from conv3_upf_kernel's; bit-exact on integer operands.
constexpr int kUpxChunks = 4;
constexpr int kUpxResRows = 3;   // skip tap rows held in registers (36 VGPRs); the other 6 rows (18 KiB) in LDS
constexpr int kUpxPosP = 176;    // the planes it is built for: Zl 10 (the production tile's level 0; also Zl 8) --
constexpr int kUpxPosL = 64;     // make_upf_plan's nposp / nposl there

template <int NPOSP, int NPOSL>
constexpr size_t upx_lds_bytes() {
    return (size_t)4 * (NPOSP + sk::kZeroPos) * kPosBytes + (size_t)2 * (NPOSL + sk::kZeroPos) * kPosBytes +
           (size_t)(9 - kUpxResRows) * 3 * 1024 + (size_t)kUpxChunks * 4 * 8 * sizeof(float);
}

template <int NPOSP, int NPOSL>
__global__ void __launch_bounds__(256, 2) conv3_upf_px_kernel(UpfArgs a) {
    constexpr int RES = kUpxResRows;
    constexpr int FS = (NPOSP + sk::kZeroPos) * kPosBytes;   // a fine plane slot (compile-time: slot offsets are immediates)
    constexpr int LS = (NPOSL + sk::kZeroPos) * kPosBytes;   // a low-resolution plane slot
    constexpr int kLow = 4 * FS;                             // the two low-resolution slots
    constexpr int kWl = kLow + 2 * LS;                       // skip tap rows RES .. 8 of the cout half
    constexpr int kRed = kWl + (9 - RES) * 3 * 1024;         // GroupNorm partials [plan chunk][wave][quad][2]
    constexpr int zf = NPOSP * kPosBytes, zl = NPOSL * kPosBytes;   // the zero windows, behind the staged positions
    constexpr int NDMA = NPOSP / 16, NDMAL = NPOSL / 16;
    static_assert(!SK_ZERO_WINDOW || (zf % 256 == 0 && zl % 256 == 0), "a zero window must cover the 64 banks once");
    static_assert(NDMA <= 4 * kMaxDma && NDMAL <= 4 * kMaxDmaL, "LDS-DMA pieces per plane");
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int py = w >> 1, pz = w & 1;   // parity class of this wave's output voxels
    const int c16 = lane & 15, g = lane >> 4;

    int blk = xcd_remap(blockIdx.x);   // the two cout halves of a region are neighbours in the XCD-aware order
    const int h = blk & 1;   // cout half
    blk >>= 1;
    const int patch = blk % a.npatch;
    blk /= a.npatch;
    const int nxc2 = (a.nxc + kUpxChunks - 1) / kUpxChunks;
    const int xc2 = blk % nxc2;
    const int b = blk / nxc2;
    const int nblk = a.npatch * a.nxc;

    const int Zl = a.Zl, Zt = a.Zt;
    const int yl0 = patch * a.K;
    const int nseg = a.K * Zl;

    // per-lane column flags and the store voxel: conv3_upf_kernel's
    unsigned vflags = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = 16 * j + c16;
        const int r = m / Zl, c = m - r * Zl;
        vflags |= (unsigned)(pz == 0 && c == 0) << j;
        vflags |= (unsigned)(pz == 1 && c == Zl - 1) << (8 + j);
        vflags |= (unsigned)(m < nseg && yl0 + r < a.Yl) << (16 + j);
    }
    auto zlo = [&](int j) { return (vflags >> j) & 1u; };
    auto zhi = [&](int j) { return (vflags >> (8 + j)) & 1u; };
    auto vvalid = [&](int j) { return (vflags >> (16 + j)) & 1u; };
    int ovox;
    {
        const int m = c16 + 16 * (g & 1);
        const int r = m / Zl, c = m - r * Zl;
        ovox = (m < nseg && yl0 + r < a.Yl) ? (2 * (yl0 + r) + py) * Zt + 2 * c + pz : -1;
    }

    // ---- LDS-DMA bookkeeping (conv3_upf_kernel's de-interleaved fine planes, low-resolution planes as they are) -------
    const int d_cs = ((lane & 3) ^ (((lane >> 4) & 1) << 1)) * 16;
    int d_vox[kMaxDma], d_low[kMaxDmaL];   // BYTE offsets of this lane's pieces in a plane, -1: outside the tile
#pragma unroll
    for (int k = 0; k < kMaxDma; ++k) {
        const int t = w + 4 * k;
        const int q = (64 * t + lane) >> 2;
        const int sub = q / a.SUBP, rem = q - sub * a.SUBP - 1;
        const int ylr = rem >= 0 ? rem / Zl : 0, zl_ = rem - ylr * Zl;
        const int yp = sub >> 1, zp = sub & 1;
        const int y = 2 * (yl0 - yp + ylr) + yp, z = 2 * zl_ + zp;
        const bool ok = t < NDMA && sub < 4 && rem >= 0 && ylr <= a.K && y >= 0 && y < a.Yt;
        d_vox[k] = ok ? (y * Zt + z) * kPosBytes + d_cs : -1;
    }
#pragma unroll
    for (int k = 0; k < kMaxDmaL; ++k) {
        const int t = w + 4 * k;
        const int q = (64 * t + lane) >> 2;
        const int rem = q - 1;
        const int ylr = rem >= 0 ? rem / Zl : 0, zl_ = rem - ylr * Zl;
        const int yl = yl0 - 1 + ylr;
        const bool ok = t < NDMAL && rem >= 0 && ylr < a.K + 2 && yl >= 0 && yl < a.Yl;
        d_low[k] = ok ? (yl * Zl + zl_) * kPosBytes + d_cs : -1;
    }

    const int xa = xc2 * kUpxChunks * a.XC;
    const int xb = min(xa + kUpxChunks * a.XC, a.Xt);
    const int Xl = a.Xt >> 1;
    const int nsteps = (xb - xa) / 2 + 2;   // step s: fine planes xa - 2 + 2s, xa - 1 + 2s, low-resolution plane xa/2 - 1 + s
    const long long out_plane = (long long)a.Yt * Zt * a.out_vs;
    char* outb = a.out + (long long)b * a.Xt * out_plane;
    const char* skipb = a.skip + (long long)b * a.skip_batch;
    const char* upb = a.up + (long long)b * a.up_batch;

    // fine plane f (x = xa - 2 + f) into slot f & 3, low-resolution plane s into slot s & 1
    auto issue_fine = [&](int f, int slot) {
        const int x = xa - 2 + f;
        const bool xok = x >= xa - 1 && x <= xb && x >= 0 && x < a.Xt;
        const int xs = min(max(x, 0), a.Xt - 1);
        const __amdgpu_buffer_rsrc_t rsrc = sk::make_rsrc(skipb + (long long)xs * a.skip_plane, (unsigned)a.skip_plane);
        char* lbase = lds + slot * FS;
#pragma unroll
        for (int k = 0; k < kMaxDma; ++k) {
            const int t = w + 4 * k;
            if (t < NDMA) {
                const unsigned voff = (xok && d_vox[k] >= 0) ? (unsigned)d_vox[k] : sk::kOob;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + t * 1024), 16, voff, 0, 0, 0);
            }
        }
    };
    auto issue_low = [&](int s, int slot) {
        const int xl = (xa >> 1) - 1 + s;
        const bool xok = xl >= 0 && xl < Xl;
        const int xs = min(max(xl, 0), Xl - 1);
        const __amdgpu_buffer_rsrc_t rsrc = sk::make_rsrc(upb + (long long)xs * a.up_plane, (unsigned)a.up_plane);
        char* lbase = lds + kLow + slot * LS;
#pragma unroll
        for (int k = 0; k < kMaxDmaL; ++k) {
            const int t = w + 4 * k;
            if (t < NDMAL) {
                const unsigned voff = (xok && d_low[k] >= 0) ? (unsigned)d_low[k] : sk::kOob;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + t * 1024), 16, voff, 0, 0, 0);
            }
        }
    };

    // ---- weights: loaded once --------------------------------------------------------------------------------------
    // skip fragment (tap row r, cout half h, x tap d): ((r * 2 + h) * 3 + d) KiB; folded fragment of (class w, tap row tytz,
    // cout half h, px, tx): kSkipFrags + w * 32 + tytz * 8 + h * 4 + px * 2 + tx
    const __amdgpu_buffer_rsrc_t wrsrc = sk::make_rsrc(a.wpk, (unsigned)((kSkipFrags + kUpFrags) * 1024));
    auto wload = [&](int frag) {
        return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane * 16, frag * 1024, 0));
    };
    half8 wres[RES][3];
#pragma unroll
    for (int r = 0; r < RES; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) wres[r][d] = wload((r * 2 + h) * 3 + d);
    half8 wup[4][2][2];   // [tytz][px][tx]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int tx = 0; tx < 2; ++tx) wup[t][px][tx] = wload(kSkipFrags + w * 32 + t * 8 + h * 4 + px * 2 + tx);
    for (int i = tid; i < (9 - RES) * 3 * 64; i += 256) {
        const int r = RES + i / 192, e = i % 192;
        *reinterpret_cast<uint4*>(lds + kWl + i * 16) = *reinterpret_cast<const uint4*>(a.wpk + (r * 2 + h) * 3 * 1024 + e * 16);
    }
    if (tid < 6 * 4 * sk::kZeroPos) {
        const int sl = tid / (4 * sk::kZeroPos), e = tid % (4 * sk::kZeroPos);
        char* zp = sl < 4 ? lds + sl * FS + zf : lds + kLow + (sl - 4) * LS + zl;
        *reinterpret_cast<uint4*>(zp + e * 16) = make_uint4(0, 0, 0, 0);
    }
    issue_fine(0, 0);
    issue_fine(1, 1);
    issue_low(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- accumulators and tap addresses --------------------------------------------------------------------------------
    // element r of [j]: cout 16 h + 4 g + r, column 16 j + c16 of the wave's segment
    const f32x4 bias4 = *reinterpret_cast<const f32x4*>(a.bias + 16 * h + 4 * g);
    f32x4 P0[2], P1[2], Q0[2], Q1[2];
    auto reset = [&](f32x4 (&o)[2]) { o[0] = o[1] = bias4; };
    reset(P0);
    reset(P1);
    reset(Q0);
    reset(Q1);
    float gsum = 0.0f, gsq = 0.0f;

    // fine plane, tap row dydz of the wave's class (conv3_upf_kernel's load_body)
    auto saddr = [&](int dydz, int j) {
        const int dy = dydz / 3 - 1, dz = dydz % 3 - 1;
        const int Y = py + dy, Z = pz + dz;
        const int tapoff = ((Y & 1) * 2 + (Z & 1)) * a.SUBP + 1 + (Y >= 1 ? Zl : 0) + (Z >> 1);
        const int q = c16 + tapoff;
        int addr = (q * 4 + (g ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;
        if (dz < 0) addr = zlo(j) ? sk::zero_of(zf, addr) : addr;
        if (dz > 0) addr = zhi(j) ? sk::zero_of(zf, addr) : addr;
        return addr;
    };
    // low-resolution plane, folded tap row tytz (conv3_upf_kernel's load_low)
    auto laddr = [&](int tytz, int j) {
        const int sy = (tytz >> 1) + py - 1, sz = (tytz & 1) + pz - 1;
        const int q = c16 + 1 + (1 + sy) * Zl + sz;
        int addr = (q * 4 + (g ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;
        addr = (sz < 0 && zlo(j)) ? sk::zero_of(zl, addr) : addr;
        addr = (sz > 0 && zhi(j)) ? sk::zero_of(zl, addr) : addr;
        return addr;
    };

    // A step over fine planes A (slot sA), B = A + 1 (slot sA + 1) and low-resolution plane A / 2 (slot sL).  oA1 / oA / oB /
    // oB1: the accumulators of output planes A-1, A, B, B+1.
    auto pair_step = [&](auto SA, auto SL, f32x4 (&oA1)[2], f32x4 (&oA)[2], f32x4 (&oB)[2], f32x4 (&oB1)[2]) {
        const char* pa = lds + decltype(SA)::value * FS;
        const char* pb = pa + FS;
        const char* pl = lds + kLow + decltype(SL)::value * LS;
        const char* wl = lds + kWl + lane * 16;
        half8 bq[2][2][2];   // [buffer][plane][j]: the B fragments of a skip tap row, one row ahead
        half8 wq[2][3];      // [buffer][d]: the weight fragments of a skip tap row, one row ahead
        half8 bl[2][2];      // [buffer][j]: the B fragments of a folded tap row
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ad = saddr(0, j);
            bq[0][0][j] = *reinterpret_cast<const half8*>(pa + ad);
            bq[0][1][j] = *reinterpret_cast<const half8*>(pb + ad);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) wq[0][d] = wres[0][d];
        // skip: 9 tap rows of 12 MFMAs; the reads of row r + 1 (its weights when they live in LDS, then its four B fragments;
        // after row 8 the B fragments of the first folded row) in the first MFMA gaps of row r, in consumption order
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const half8(&W)[3] = wq[r & 1];
            const int nr = r + 1;
            const bool wread = nr < 9 && nr >= RES;
            if (nr < 9 && !wread) {
#pragma unroll
                for (int d = 0; d < 3; ++d) wq[nr & 1][d] = wres[nr][d];
            }
            auto next_read = [&](int k) {
                if (nr == 9) {   // B fragments of folded row 0
                    bl[0][k] = *reinterpret_cast<const half8*>(pl + laddr(0, k));
                    return;
                }
                const char* wp = wl + (nr - RES) * 3 * 1024;
                int kk = k;   // W0, A0, B0, W1, W2, A1, B1
                if (!wread) kk = (k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 5 : 6);
                switch (kk) {
                    case 0: wq[nr & 1][0] = *reinterpret_cast<const half8*>(wp); break;
                    case 1: bq[nr & 1][0][0] = *reinterpret_cast<const half8*>(pa + saddr(nr, 0)); break;
                    case 2: bq[nr & 1][1][0] = *reinterpret_cast<const half8*>(pb + saddr(nr, 0)); break;
                    case 3: wq[nr & 1][1] = *reinterpret_cast<const half8*>(wp + 1024); break;
                    case 4: wq[nr & 1][2] = *reinterpret_cast<const half8*>(wp + 2048); break;
                    case 5: bq[nr & 1][0][1] = *reinterpret_cast<const half8*>(pa + saddr(nr, 1)); break;
                    default: bq[nr & 1][1][1] = *reinterpret_cast<const half8*>(pb + saddr(nr, 1)); break;
                }
            };
            const int nreads = nr == 9 ? 2 : (wread ? 7 : 4);
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                const int j = m / 6;
                const half8 fa = bq[r & 1][0][j], fb = bq[r & 1][1][j];
                switch (m % 6) {   // tap d of a weight row multiplies x_in = x_out + d - 1
                    case 0: oB[j] = SK_MFMA_16x16x32_T16(W[0], fa, oB[j], 0, 0, 0); break;
                    case 1: oB1[j] = SK_MFMA_16x16x32_T16(W[0], fb, oB1[j], 0, 0, 0); break;
                    case 2: oA[j] = SK_MFMA_16x16x32_T16(W[1], fa, oA[j], 0, 0, 0); break;
                    case 3: oA1[j] = SK_MFMA_16x16x32_T16(W[2], fa, oA1[j], 0, 0, 0); break;
                    case 4: oB[j] = SK_MFMA_16x16x32_T16(W[1], fb, oB[j], 0, 0, 0); break;
                    default: oA[j] = SK_MFMA_16x16x32_T16(W[2], fb, oA[j], 0, 0, 0); break;
                }
                if (m < nreads) next_read(m);
                if (m <= nreads) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // upsampled: 4 folded tap rows of 8 MFMAs.  Output plane A-1 (px 1) reads this plane through tx 1, A (px 0) through
        // tx 1, B (px 1) through tx 0, B+1 (px 0) through tx 0.
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int nreads = t < 3 ? 2 : 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = m / 4;
                const half8 f = bl[t & 1][j];
                switch (m % 4) {
                    case 0: oA1[j] = SK_MFMA_16x16x32_T16(wup[t][1][1], f, oA1[j], 0, 0, 0); break;
                    case 1: oA[j] = SK_MFMA_16x16x32_T16(wup[t][0][1], f, oA[j], 0, 0, 0); break;
                    case 2: oB[j] = SK_MFMA_16x16x32_T16(wup[t][1][0], f, oB[j], 0, 0, 0); break;
                    default: oB1[j] = SK_MFMA_16x16x32_T16(wup[t][0][0], f, oB1[j], 0, 0, 0); break;
                }
                if (m < nreads) bl[(t + 1) & 1][m] = *reinterpret_cast<const half8*>(pl + laddr(t + 1, m));
                if (m <= nreads) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- epilogue: raw fp16 store of a finished plane + its GroupNorm sums (conv3_upf_kernel's, one cout half) ----------
    // Always two stores per step (a plane outside [xa, xb) stores to an out-of-range offset: dropped): the counted wait
    // below relies on it.
    auto finish_plane = [&](f32x4 (&o)[2], int x) {
        const bool st = x >= xa && x < xb;   // wave-uniform
        const int xs = min(max(x, 0), a.Xt - 1);
        const __amdgpu_buffer_rsrc_t rout = sk::make_rsrc(outb + (long long)xs * out_plane, (unsigned)out_plane);
        unsigned d[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 r = o[j];
            const half4 hv = {(t16)r[0], (t16)r[1], (t16)r[2], (t16)r[3]};
            const uint2 u = __builtin_bit_cast(uint2, hv);
            d[j][0] = u.x;
            d[j][1] = u.y;
            const bool in = st && vvalid(j);
            const t16x2 z2 = {(t16)0.0f, (t16)0.0f}, one2 = {(t16)1.0f, (t16)1.0f};
            const t16x2 lo2 = in ? t16x2{hv[0], hv[1]} : z2, hi2 = in ? t16x2{hv[2], hv[3]} : z2;
            gsum = SK_DOT2_T16(lo2, one2, gsum);
            gsum = SK_DOT2_T16(hi2, one2, gsum);
            gsq = SK_DOT2_T16(lo2, lo2, gsq);
            gsq = SK_DOT2_T16(hi2, hi2, gsq);
        }
        const auto s0 = __builtin_amdgcn_permlane16_swap(d[0][0], d[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(d[0][1], d[1][1], false, false);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 lv = {s0[0], s1[0], s0[1], s1[1]};   // channels 16 h + 8 (g >> 1) .. +7 of column c16 + 16 (g & 1)
        const unsigned off = (unsigned)(ovox * a.out_vs + a.cout_off * 2 + 32 * h + 16 * (g >> 1));
        __builtin_amdgcn_raw_buffer_store_b128(lv, rout, (st && ovox >= 0) ? off : sk::kOob, 0, 0);
    };
    // GroupNorm partials of plan chunk u: this wave's share, reduced over the 16 lanes of a quad (conv3_upf_kernel's order)
    float* red = reinterpret_cast<float*>(lds + kRed);
    auto flush = [&](int u) {
        float s = gsum, ss = gsq;
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) {
            s += __shfl_xor(s, m);
            ss += __shfl_xor(ss, m);
        }
        if (c16 == 0) {
            red[((u * 4 + w) * 4 + g) * 2 + 0] = s;
            red[((u * 4 + w) * 4 + g) * 2 + 1] = ss;
        }
        gsum = gsq = 0.0f;
    };
    int xnext = xa + a.XC, unext = 0;   // the next boundary between two plan chunks, the chunk it closes
    auto end_step = [&](int s, f32x4 (&oA1)[2], f32x4 (&oA)[2]) {
        const int xA = xa - 2 + 2 * s;
        finish_plane(oA1, xA - 1);
        if (xA == xnext && xA < xb) {
            flush(unext);
            ++unext;
            xnext += a.XC;
        }
        finish_plane(oA, xA);
        reset(oA1);
        reset(oA);
        // vmcnt retires in order: the step's LDS-DMA (older than its two stores) has landed
        asm volatile("s_waitcnt vmcnt(2)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };

    typedef std::integral_constant<int, 0> S0_;
    typedef std::integral_constant<int, 1> S1_;
    typedef std::integral_constant<int, 2> S2_;
    // Steps alternate between two fixed role assignments: even steps read fine slots (0, 1) and low slot 0 with (P0, P1, Q0,
    // Q1) = output planes (A-1, A, B, B+1); odd steps fine slots (2, 3), low slot 1, the pairs P / Q swapped.
    int s = 0;
    auto even_step = [&]() {
        if (s + 1 < nsteps) {
            issue_fine(2 * s + 2, 2);
            issue_fine(2 * s + 3, 3);
            issue_low(s + 1, 1);
        }
        pair_step(S0_{}, S0_{}, P0, P1, Q0, Q1);
        end_step(s, P0, P1);
        ++s;
    };
    auto odd_step = [&]() {
        if (s + 1 < nsteps) {
            issue_fine(2 * s + 2, 0);
            issue_fine(2 * s + 3, 1);
            issue_low(s + 1, 0);
        }
        pair_step(S2_{}, S1_{}, Q0, Q1, P0, P1);
        end_step(s, Q0, Q1);
        ++s;
    };
    while (s + 1 < nsteps) {
        even_step();
        odd_step();
    }
    if (s < nsteps) even_step();
    flush(unext);

    // ---- one partial row per plan chunk: the four waves' shares in wave order ---------------------------------------------
    if (a.partial) {
        __syncthreads();
        if (tid < kUpxChunks * 8) {
            const int u = tid >> 3, k = tid & 7;
            const int xo = xc2 * kUpxChunks + u;
            if (xo < a.nxc) {
                float t = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) t += red[(u * 4 + q) * 8 + k];
                a.partial[((long long)b * nblk + xo * a.npatch + patch) * a.pstride + a.poff + 8 * h + k] = t;
            }
        }
    }
}

struct UpfPlan {
    int K, SUBP, nposp, nposl, npatch, XC, nxc;
    size_t lds;
};

// 0: supported.  The folded kernel covers the geometries whose low-resolution rows fit a 32-column segment.
int make_upf_plan(UpfPlan& p, int Xt, int Yt, int Zt) {
    if (Xt % 2 || Yt % 2 || Zt % 2) return -1;
    const int Zl = Zt / 2, Yl = Yt / 2;
    if (Zl < 1 || Zl > 32) return -1;
    p.K = 32 / Zl;
    const int over = 32 - p.K * Zl;                       // columns past the segment still form addresses
    p.SUBP = (p.K + 1) * Zl + 2;
    p.nposp = (4 * p.SUBP + over + 15) / 16 * 16;
    p.nposl = ((p.K + 2) * Zl + 2 + over + 15) / 16 * 16;
    if (p.nposp > 64 * kMaxDma || p.nposl > 64 * kMaxDmaL || p.nposl > p.nposp) return -1;
    p.lds = (size_t)6 * (p.nposp + sk::kZeroPos) * kPosBytes;
    if (p.lds > 80 * 1024) return -1;
    p.npatch = (Yl + p.K - 1) / p.K;
    // x-chunks as conv3d.hip's make_plan: a function of the tile geometry only (batch-invariant bits)
    const int kPlanBatch = 8, xs = 4;
    const int target = 256 * 2 * 6;
    int nxc = (target + p.npatch * kPlanBatch - 1) / (p.npatch * kPlanBatch);
    const int max_nxc = (Xt + 2 * xs - 1) / (2 * xs);
    if (nxc > max_nxc) nxc = max_nxc;
    if (nxc < 1) nxc = 1;
    int XC = (Xt + nxc - 1) / nxc;
    XC = (XC + xs - 1) / xs * xs;
    p.XC = XC;
    p.nxc = (Xt + XC - 1) / XC;
    return 0;
}

}  // namespace

extern "C" {

int sk_conv3d_upfold_num_blocks(int ox, int oy, int oz, int cout) {
    UpfPlan p;
    if ((cout != 32 && cout != 64) || make_upf_plan(p, ox, oy, oz)) return -1;
    return p.npatch * p.nxc;
}

static int64_t pack_upfold(const float* w, int cout, int c_skip, int c_up, void* dst, bool split) {
    if ((cout != 32 && cout != 64) || c_skip <= 0 || c_up <= 0 || c_skip % 32 || c_up % 32) {
        sk::set_error("sk_conv3d_pack_weight_upfold_host: unsupported shape cout=%d c_skip=%d c_up=%d", cout, c_skip, c_up);
        return SK_ERR_ARG;
    }
    const int ns = c_skip / 32, nu = c_up / 32, cin = c_skip + c_up;
    const int nsets = split ? 2 : 1;   // split: per chunk the lo-weight fragments, then the hi-weight fragments
    const int64_t nfrag = ((int64_t)ns * kSkipFrags + (int64_t)nu * kUpFrags) * nsets * (cout / 32);
    if (!dst) return nfrag * 1024;
    t16* out = (t16*)dst;
    auto W = [&](int co, int ci, int kx, int ky, int kz) { return w[((((int64_t)co * cin + ci) * 3 + kx) * 3 + ky) * 3 + kz]; };
    // plain: fp16(v); split set 0: lo = fp16(v - fp16(v)), set 1: hi = fp16(v)
    auto part = [&](double v, int set) {
        const t16 hi = (t16)(float)v;
        if (!split || set == 1) return hi;
        return (t16)(float)(v - (double)(float)hi);
    };
    int64_t f = 0;
    // the folded weight of parity p, tap t along an axis sums the kernel taps k (0..2) that read the same low-resolution
    // voxel: p=0: t=0 {0}, t=1 {1,2}; p=1: t=0 {0,1}, t=1 {2}
    auto lo = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2); };
    auto hi = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2); };
    for (int cg = 0; cg < cout / 32; ++cg) {   // one fragment set per 32 output channels (= per launch of the kernel)
        // skip chunks: conv3_m16_kernel's order [chunk][dy*3+dz][cout half][dx]; lane l holds W[16 i + (l&15)][c0 + 8 (l>>4) + e]
        for (int ch = 0; ch < ns; ++ch)
            for (int set = 0; set < nsets; ++set)
                for (int dydz = 0; dydz < 9; ++dydz)
                    for (int i = 0; i < 2; ++i)
                        for (int dx = 0; dx < 3; ++dx, ++f)
                            for (int l = 0; l < 64; ++l)
                                for (int e = 0; e < 8; ++e)
                                    out[f * 512 + l * 8 + e] =
                                        part(W(32 * cg + 16 * i + (l & 15), ch * 32 + 8 * (l >> 4) + e, dx, dydz / 3, dydz % 3), set);
        // upsampled chunks: [chunk][class 2 py + pz][ty*2+tz][cout half][px][tx]; the fold is summed in double, then split
        for (int ch = 0; ch < nu; ++ch)
            for (int set = 0; set < nsets; ++set)
                for (int cls = 0; cls < 4; ++cls)
                    for (int tytz = 0; tytz < 4; ++tytz)
                        for (int i = 0; i < 2; ++i)
                            for (int px = 0; px < 2; ++px)
                                for (int tx = 0; tx < 2; ++tx, ++f) {
                                    const int py = cls >> 1, pz = cls & 1, ty = tytz >> 1, tz = tytz & 1;
                                    for (int l = 0; l < 64; ++l)
                                        for (int e = 0; e < 8; ++e) {
                                            const int co = 32 * cg + 16 * i + (l & 15), ci = c_skip + ch * 32 + 8 * (l >> 4) + e;
                                            double sacc = 0.0;
                                            for (int kx = lo(px, tx); kx <= hi(px, tx); ++kx)
                                                for (int ky = lo(py, ty); ky <= hi(py, ty); ++ky)
                                                    for (int kz = lo(pz, tz); kz <= hi(pz, tz); ++kz) sacc += (double)W(co, ci, kx, ky, kz);
                                            out[f * 512 + l * 8 + e] = part(split ? sacc : (double)(float)sacc, set);
                                        }
                                }
    }
    return nfrag * 1024;
}

int64_t sk_conv3d_pack_weight_upfold_host(const float* w, int cout, int c_skip, int c_up, void* dst) {
    return pack_upfold(w, cout, c_skip, c_up, dst, false);
}

int64_t sk_conv3d_pack_weight_upfold_split_host(const float* w, int cout, int c_skip, int c_up, void* dst) {
    return pack_upfold(w, cout, c_skip, c_up, dst, true);
}

// precision "mix8": per 32 output channels [the fp16 fragments of the hi weights, as sk_conv3d_pack_weight_upfold_host lays them
// out][fp8 fragments of 2 KiB: skip chunks [chunk][tap-row pair 5][cout half 2][dx 3] -- lane l: cout 16 i + (l & 15), K block
// g = l >> 4: row 2 rp + (g >> 1), g & 1 = 0: e4m3(2^(b+11) w_lo) | 1: e4m3(2^b w) -- then upsampled chunks [chunk][class 4][ty 2]
// [cout half 2][px 2][tx 2] -- K block g: tap tz = g >> 1, g & 1 as above, of the FOLDED weight (summed in double; w_lo = sum -
// fp16(sum))].  b = *scale_exp: the largest power of two with 2^b max(|w|, |folded sums|) <= 240.
int64_t sk_conv3d_pack_weight_upfold_mix8_host(const float* w, int cout, int c_skip, int c_up, void* dst, int* scale_exp) {
    const int64_t f16b = pack_upfold(w, cout, c_skip, c_up, nullptr, false);
    if (f16b < 0) return f16b;
    const int ns = c_skip / 32, nu = c_up / 32, cin = c_skip + c_up, ncg = cout / 32;
    const int64_t f16_cg = f16b / ncg, f8_cg = ((int64_t)ns * kSkipFrags8 + (int64_t)nu * kUpFrags8) * 2048;
    const int64_t total = (f16_cg + f8_cg) * ncg;
    if (!dst) return total;
    auto W = [&](int co, int ci, int kx, int ky, int kz) { return w[((((int64_t)co * cin + ci) * 3 + kx) * 3 + ky) * 3 + kz]; };
    auto lo = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2); };
    auto hi = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2); };
    auto folded = [&](int co, int ci, int px, int tx, int py, int ty, int pz, int tz) {
        double sacc = 0.0;
        for (int kx = lo(px, tx); kx <= hi(px, tx); ++kx)
            for (int ky = lo(py, ty); ky <= hi(py, ty); ++ky)
                for (int kz = lo(pz, tz); kz <= hi(pz, tz); ++kz) sacc += (double)W(co, ci, kx, ky, kz);
        return sacc;
    };
    double wmax = 0.0;
    for (int co = 0; co < cout; ++co) {
        for (int ci = 0; ci < c_skip; ++ci)
            for (int t = 0; t < 27; ++t) wmax = std::fmax(wmax, std::fabs((double)W(co, ci, t / 9, (t / 3) % 3, t % 3)));
        for (int ci = c_skip; ci < cin; ++ci)
            for (int c = 0; c < 64; ++c)
                wmax = std::fmax(wmax, std::fabs(folded(co, ci, c & 1, (c >> 1) & 1, (c >> 2) & 1, (c >> 3) & 1, (c >> 4) & 1, (c >> 5) & 1)));
    }
    int b = 0;
    while (b < 40 && std::ldexp(wmax, b + 1) <= 240.0) ++b;
    if (scale_exp) *scale_exp = b;
    auto enc = [&](double v, int kind) {   // kind 0: the lo part at 2^(b+11), 1: the value at 2^b
        const double h = (double)(float)(t16)(float)v;
        return sk::f32_to_e4m3((float)std::ldexp(kind ? v : v - h, kind ? b : b + 11));
    };
    std::vector<char> f16(f16b);
    if (pack_upfold(w, cout, c_skip, c_up, f16.data(), false) != f16b) return SK_ERR_ARG;
    for (int cg = 0; cg < ncg; ++cg) {
        char* img = reinterpret_cast<char*>(dst) + cg * (f16_cg + f8_cg);
        memcpy(img, f16.data() + cg * f16_cg, (size_t)f16_cg);
        uint8_t* o = reinterpret_cast<uint8_t*>(img + f16_cg);
        int64_t f = 0;
        for (int ch = 0; ch < ns; ++ch)
            for (int rp = 0; rp < 5; ++rp)
                for (int i = 0; i < 2; ++i)
                    for (int dx = 0; dx < 3; ++dx, ++f)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 32; ++j) {
                                const int g = l >> 4, row = 2 * rp + (g >> 1);
                                o[f * 2048 + l * 32 + j] =
                                    row < 9 ? enc((double)W(32 * cg + 16 * i + (l & 15), ch * 32 + j, dx, row / 3, row % 3), g & 1) : 0;
                            }
        for (int ch = 0; ch < nu; ++ch)
            for (int cls = 0; cls < 4; ++cls)
                for (int ty = 0; ty < 2; ++ty)
                    for (int i = 0; i < 2; ++i)
                        for (int px = 0; px < 2; ++px)
                            for (int tx = 0; tx < 2; ++tx, ++f)
                                for (int l = 0; l < 64; ++l)
                                    for (int j = 0; j < 32; ++j) {
                                        const int g = l >> 4;
                                        const double v = folded(32 * cg + 16 * i + (l & 15), c_skip + ch * 32 + j, px, tx, cls >> 1, ty, cls & 1, g >> 1);
                                        o[f * 2048 + l * 32 + j] = enc(v, g & 1);
                                    }
    }
    return total;
}

static int upfold_impl(const void* skip, int c_skip, const void* up, int c_up, const void* weight, const float* bias,
                       void* out, int B, int ox, int oy, int oz, int cout, float* gn_partial, void* stream_, const bool split,
                       const bool mix8 = false, const int w8_scale_exp = 0) {
    hipStream_t stream = (hipStream_t)stream_;
    SK_CHECK_ARG(skip && up && weight && bias && out, "sk_conv3d_upfold: NULL pointer");
    SK_CHECK_ARG(cout == 32 || cout == 64, "sk_conv3d_upfold: cout must be 32 or 64 (got %d)", cout);
    SK_CHECK_ARG(c_skip > 0 && c_up > 0 && c_skip % 32 == 0 && c_up % 32 == 0 && c_skip + c_up <= 256,
                 "sk_conv3d_upfold: channel counts must be multiples of 32 (got %d + %d)", c_skip, c_up);
    SK_CHECK_ARG(B > 0 && ox > 0 && oy > 0 && oz > 0, "sk_conv3d_upfold: bad output extents");
    UpfPlan p;
    SK_CHECK_ARG(make_upf_plan(p, ox, oy, oz) == 0,
                 "sk_conv3d_upfold: geometry (%d,%d,%d) unsupported (sk_conv3d_upfold_num_blocks < 0: use sk_conv3d)", ox, oy, oz);
    UpfArgs a{};
    a.skip = (const char*)skip;
    a.up = (const char*)up;
    a.skipC = c_skip;
    a.upC = c_up;
    const int lanes = split ? 2 : 1;   // fp16 values per logical channel in a voxel line: [hi | lo]
    a.skip_plane = (long long)oy * oz * c_skip * 2 * lanes;
    a.skip_batch = a.skip_plane * ox;
    a.up_plane = (long long)(oy / 2) * (oz / 2) * c_up * 2 * lanes;
    a.up_batch = a.up_plane * (ox / 2);
    a.ns = c_skip / 32;
    a.nu = c_up / 32;
    a.wpk = (const char*)weight;
    a.bias = bias;
    a.out = (char*)out;
    a.partial = gn_partial;
    a.B = B;
    a.Xt = ox;
    a.Yt = oy;
    a.Zt = oz;
    a.Yl = oy / 2;
    a.Zl = oz / 2;
    a.XC = p.XC;
    a.nxc = p.nxc;
    a.npatch = p.npatch;
    a.K = p.K;
    a.SUBP = p.SUBP;
    a.nposp = p.nposp;
    a.nposl = p.nposl;
    a.dbg = nullptr;
#ifdef SK_TIMING
    a.dbg = sk::timing_buffer();
#endif
    a.out_vs = cout * 2 * lanes;
    a.pstride = (cout / 4) * 2;
    if (!split && !mix8 && a.ns == 1 && a.nu == 1 && cout == 32 && p.nposp == kUpxPosP && p.nposl == kUpxPosL) {
        // the plane-streaming form (conv3_upf_px_kernel): one cout half per workgroup, kUpxChunks plan chunks along x
        auto kern = conv3_upf_px_kernel<kUpxPosP, kUpxPosL>;
        constexpr size_t lds = upx_lds_bytes<kUpxPosP, kUpxPosL>();
        static_assert(lds <= 80 * 1024, "two workgroups per CU");
        SK_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const unsigned grid = (unsigned)(2 * p.npatch * ((p.nxc + kUpxChunks - 1) / kUpxChunks) * B);
        a.cout_off = 0;
        a.poff = 0;
        kern<<<grid, 256, lds, stream>>>(a);
        SK_CHECK_LAUNCH();
        return SK_OK;
    }
    const bool wlds = !split && a.ns == 1 && p.lds + 12288 <= 80 * 1024;   // two tap rows of the single skip chunk in LDS
    auto kern = mix8 ? conv3_upf_mix8_kernel<4, false, true>
                     : (split ? conv3_upf_kernel<4, false, true> : (wlds ? conv3_upf_kernel<4, true, false> : conv3_upf_kernel<4, false, false>));
    const size_t f16_cg = (size_t)(a.ns * kSkipFrags + a.nu * kUpFrags) * 1024, f8_cg = (size_t)(a.ns * kSkipFrags8 + a.nu * kUpFrags8) * 2048;
    if (mix8) {
        SK_CHECK_ARG(split && w8_scale_exp >= 0 && w8_scale_exp < 64, "sk_conv3d_upfold_mix8: bad weight scale exponent %d", w8_scale_exp);
        // a low-resolution plane holds both halves of its lines in one ring slot, in front of the slot's zero window
        SK_CHECK_ARG(2 * p.nposl <= p.nposp, "sk_conv3d_upfold_mix8: geometry (%d,%d,%d) unsupported", ox, oy, oz);
        a.w8_off = (int)f16_cg;
        a.wpk_bytes = (int)(f16_cg + f8_cg);
        a.w8_scale = 0x01010101 * (127 - w8_scale_exp);
    }
    const size_t lds = p.lds + (wlds ? 12288 : 0);
    if (lds > 48 * 1024)
        SK_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = (unsigned)(p.npatch * p.nxc * B);
    // 32 output channels per launch (COUT 64: two launches over the same inputs -- twice the staging, but on the
    // 16x16x32 matrix instruction and at 70 instead of 108 tap-chunks; measured against conv3_kernel<64> in DESIGN.md)
    for (int cg = 0; cg < cout / 32; ++cg) {
        a.cout_off = 32 * cg;
        a.poff = 16 * cg;
        a.wpk = (const char*)weight + (mix8 ? (size_t)cg * (f16_cg + f8_cg) : (size_t)cg * (a.ns * kSkipFrags + a.nu * kUpFrags) * lanes * 1024);
        kern<<<grid, 256, lds, stream>>>(a);
        SK_CHECK_LAUNCH();
    }
    return SK_OK;
}


int sk_conv3d_upfold(const void* skip, int c_skip, const void* up, int c_up, const void* weight, const float* bias,
                     void* out, int B, int ox, int oy, int oz, int cout, float* gn_partial, void* stream) {
    return upfold_impl(skip, c_skip, up, c_up, weight, bias, out, B, ox, oy, oz, cout, gn_partial, stream, false);
}

int sk_conv3d_upfold_split(const void* skip, int c_skip, const void* up, int c_up, const void* weight, const float* bias,
                           void* out, int B, int ox, int oy, int oz, int cout, float* gn_partial, void* stream) {
    return upfold_impl(skip, c_skip, up, c_up, weight, bias, out, B, ox, oy, oz, cout, gn_partial, stream, true);
}

int sk_conv3d_upfold_mix8(const void* skip, int c_skip, const void* up, int c_up, const void* weight, int weight_scale_exp,
                          const float* bias, void* out, int B, int ox, int oy, int oz, int cout, float* gn_partial, void* stream) {
    return upfold_impl(skip, c_skip, up, c_up, weight, bias, out, B, ox, oy, oz, cout, gn_partial, stream, true, true, weight_scale_exp);
}

}  // extern "C"
