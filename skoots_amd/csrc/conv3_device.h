// Device-side scaffolding shared by the 3x3x3 conv kernels of conv3d.hip and conv3d_up.hip: ONE definition of the vector
// types, the layout constants, the timing / ablation macros, the XCD-aware workgroup order, the block decode and the
// GroupNorm-partials reduction.  Everything has internal linkage (the twin-built sources are linked into one library) and is
// force-inlined.  These kernels' register allocation follows the shape of their source: a helper stays only in a form in
// which every kernel that uses it compiles to the machine code it had with its own copy (tools/kernel_isa_diff.py,
// profiles/conv3_scaffold_isa.txt), and the few kernels no form did that for say so where they keep their copy.  The larger
// pieces that two kernels share as identical text are included into both bodies (conv3_issue_dma.inc, conv3_px_*.inc).
#pragma once
#include <type_traits>

#include "common.h"

namespace {

typedef t16 half8 __attribute__((ext_vector_type(8)));
typedef t16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kChunk = 32;       // input channels per LDS image
constexpr int kPosBytes = 64;    // kChunk * sizeof(fp16)
constexpr int kPatch = 128;      // voxels per (y,z) patch = 4 waves x 32 columns
constexpr int kPadStride = 64;   // bytes per voxel in the epilogue transpose pad (16-B chunks XOR-swizzled)
constexpr int kPadBytes = 32 * kPadStride;

// Timing experiments (wrong results by design) exist only in the -DSK_TUNING build that tools/ use: in the release
// library no environment variable can change what a kernel computes.
// (non-temporal epilogue stores: -1.7 % on the conv kernels, +4.5 % on the GroupNorm pass that reads the tensor next --
// it loses what the conv's stores leave in the Infinity Cache; net zero, not used)
// Phase timing (tools/conv_phase_timing.py, tools/upfold_phase_timing.py, -DSK_TIMING build only): per wave, cycles
// between the marks of a phase; a workgroup for which `in_window` holds dumps them as record `row` of the timing buffer
#ifdef SK_TIMING
#define SK_T_DECL long long tacc_[sk::kTimingSlots] = {0}; long long tprev_ = __builtin_readcyclecounter();
#define SK_T(i) { const long long t_ = __builtin_readcyclecounter(); tacc_[i] += t_ - tprev_; tprev_ = t_; }
#define SK_T_DUMP_ROW(a, in_window, row, w, lane) if ((a).dbg && in_window && (w) < 4 && (lane) == 0) { \
        for (int i_ = 0; i_ < sk::kTimingSlots; ++i_) (a).dbg[((long long)(row) * 4 + (w)) * sk::kTimingSlots + i_] = tacc_[i_]; }
#else
#define SK_T_DECL
#define SK_T(i)
#define SK_T_DUMP_ROW(a, in_window, row, w, lane)
#endif
#ifdef SK_TUNING
#define SK_ABL(a, bits) ((a).ablate & (bits))
#else
#define SK_ABL(a, bits) 0
#endif
// compile-time ablations of conv3_px_kernel's MFMA body (a run-time switch there changes the schedule it is meant to
// measure): make ... EXTRA="-DSK_TUNING -DSK_PX_ABLATE=48"; 16: no LDS weight reads, 32: no B fragment reads after a
// step's first tap row, 64: no barrier between the steps.  Results are wrong by design.
#ifndef SK_PX_ABLATE
#define SK_PX_ABLATE 0
#endif
#define SK_PX_ABL(bits) ((SK_PX_ABLATE) & (bits))

// Workgroups are dealt round-robin over the 8 XCDs (private L2 each).  Neighbouring patches
// share their y/z halo and consecutive x-chunks share two planes: give each XCD a contiguous
// run of the (batch, x-chunk, patch) order so those re-reads hit its own L2 (bijective remap).
__device__ __forceinline__ int xcd_remap(int blk) {
    const int nwg = gridDim.x, xcd = blk & 7, qn = nwg >> 3, rn = nwg & 7;
    return (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (blk >> 3);
}

// position of a workgroup in the (batch, x-chunk, patch) order; block_in_batch / nblk: its GroupNorm-partials row inside
// the batch item / rows per batch item
__device__ __forceinline__ void decode_block(int blk, int npatch, int nxc, int& patch, int& xc, int& b, int& block_in_batch,
                                             int& nblk) {
    patch = blk % npatch;
    blk /= npatch;
    xc = blk % nxc;
    b = blk / nxc;
    block_in_batch = xc * npatch + patch;
    nblk = npatch * nxc;
}

// ---- block-level reduction of the GroupNorm partials ------------------------------------
// red: [4 waves][8 quads of the wave's cout tile][2] (sum, sumsq), reduced in a fixed order (deterministic, no float
// atomics) into the NT * 16 floats of the workgroup's row b * nblk + block_in_batch of `partial`: `stride` floats per row,
// from float `off` of it (by reference: a kernel argument is then read where the row is written, as the kernels did)
template <int NT>
__device__ __forceinline__ void gn_block_sum(const float* red, float* partial, const int& b, const int& nblk, const int& block_in_batch,
                                             const int& stride, const int& off, int tid) {
    __syncthreads();
    if (tid < NT * 16) {
        // channel quad Q = cout/4 = 8*nt + k ; waves with wn == nt: w = wm*NT + nt
        const int nt = tid / 16, k2 = tid % 16;
        float t = 0.0f;
#pragma unroll
        for (int g = 0; g < 4 / NT; ++g) t += red[(g * NT + nt) * 16 + k2];
        partial[((long long)b * nblk + block_in_batch) * stride + off + tid] = t;
    }
}
// a wave's share on the 16x16x32 accumulator layout: gsum / gsq[i] = channel quad 4 i + g of the wave's cout tile, summed
// over the 16 lanes that share g
__device__ __forceinline__ void gn_wave_sum16(float* red, const float (&gsum)[2], const float (&gsq)[2], int w, int c16, int g) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float s = gsum[i], ss = gsq[i];
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) {
            s += __shfl_xor(s, m);
            ss += __shfl_xor(ss, m);
        }
        if (c16 == 0) {
            red[(w * 8 + 4 * i + g) * 2 + 0] = s;
            red[(w * 8 + 4 * i + g) * 2 + 1] = ss;
        }
    }
}

}  // namespace
