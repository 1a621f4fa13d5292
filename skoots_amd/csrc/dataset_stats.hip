// Dataset statistics of the training command: the 256-bin histogram of a uint8 volume that lives on the device.
// Reference: skoots/train/dataloader.py:246-310 (dataset.sum / subtract_square_sum copy every volume to the host and
// loop over it there).  From the histogram the host gets the exact integer sum and sum_v h[v] (v - other)^2 for any
// `other` without touching the volume again (skoots_amd/train/dataloader.py).
//
// A plain memory-bound pass: 16-byte loads per lane on the aligned body (scalar head and tail for an unaligned x and
// n % 16, done by workgroup 0), a capped grid with a grid-stride loop, 32-bit counters privatised per wave in LDS, one
// flush per workgroup with 64-bit integer global atomics -- exact, and the same from run to run.
//
// A training volume is mostly a few grey values, so many lanes of a wave hitting one counter is the normal case.  Two
// ways of dealing with it are built (DESIGN.md section 14 has the measurement):
//   kCopies  each wave keeps 8 copies of its 256 counters, selected by lane & 7 and laid out [bin][copy] so that the
//            copies of one bin sit in 8 neighbouring banks; a lane first merges runs of equal consecutive bytes of its
//            own 16, so a constant volume costs one LDS atomic per lane and load;
//   kMatch   one copy per wave; per byte position, lanes whose lower neighbour holds the same value are merged into the
//            run's first lane with one __ballot (what validate.hip does for its contingency tables).
// The release library runs kDefaultVariant; a -DSK_TUNING build reads SK_HIST_VARIANT (0 / 1) for the A/B.
#include <stdlib.h>

#include "common.h"

namespace sk {

constexpr int kHistBlock = 256;                 // 4 waves
constexpr int kHistWaves = kHistBlock / 64;
constexpr int kHistCopies = 8;
constexpr int kCopies = 0, kMatch = 1;
constexpr int kDefaultVariant = kCopies;
constexpr int64_t kHistMaxN = (int64_t)1 << 40;  // keeps a workgroup's 32-bit LDS counters far from wrapping

template <int VARIANT>
__device__ inline void hist_add16(unsigned* wave_hist, const uint4 v, const int lane) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    if (VARIANT == kCopies) {
        const int copy = lane & (kHistCopies - 1);
        unsigned prev = w[0] & 255u, cnt = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned cur = (w[j >> 2] >> (8 * (j & 3))) & 255u;
            if (cur != prev) {
                atomicAdd(&wave_hist[prev * kHistCopies + copy], cnt);
                prev = cur;
                cnt = 0;
            }
            ++cnt;
        }
        atomicAdd(&wave_hist[prev * kHistCopies + copy], cnt);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {   // every lane of the wave is here: the loop around it is wave-uniform
            const int cur = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            const int below = __shfl_up(cur, 1);
            const bool cont = lane > 0 && below == cur;
            const unsigned long long cmask = __ballot(cont);
            if (!cont) {
                const unsigned long long rest = lane == 63 ? 0ull : cmask >> (lane + 1);
                atomicAdd(&wave_hist[cur], 1u + (unsigned)__builtin_ctzll(~rest));
            }
        }
    }
}

template <int VARIANT>
__global__ __launch_bounds__(kHistBlock) void u8_histogram_kernel(const uint8_t* __restrict__ x, const int64_t head,
                                                                  const int64_t nvec, const int64_t tail,
                                                                  unsigned long long* __restrict__ hist) {
    constexpr int kPerWave = VARIANT == kCopies ? 256 * kHistCopies : 256;
    __shared__ unsigned lds[kHistWaves * kPerWave];
    for (int i = threadIdx.x; i < kHistWaves * kPerWave; i += kHistBlock) lds[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* wave_hist = lds + wave * kPerWave;
    const int stride1 = VARIANT == kCopies ? kHistCopies : 1;   // distance of two bins of one copy
    const int copy = VARIANT == kCopies ? (lane & (kHistCopies - 1)) : 0;

    const uint4* body = (const uint4*)(x + head);   // 16-byte aligned by the choice of head
    const int64_t step = (int64_t)gridDim.x * kHistBlock;
    // whole waves iterate together (the ballots of kMatch need every lane): the vectors past the last full wave of
    // 64 go through the scalar path below with the head and the tail
    const int64_t nvec_waves = nvec & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * kHistBlock + threadIdx.x; i < nvec_waves; i += step)
        hist_add16<VARIANT>(wave_hist, body[i], lane);
    if (blockIdx.x == 0) {
        const uint8_t* rest = x + head + nvec_waves * 16;
        const int64_t nrest = (nvec - nvec_waves) * 16 + tail;   // < 64 * 16 + 16
        for (int64_t i = threadIdx.x; i < head; i += kHistBlock) atomicAdd(&wave_hist[x[i] * stride1 + copy], 1u);
        for (int64_t i = threadIdx.x; i < nrest; i += kHistBlock) atomicAdd(&wave_hist[rest[i] * stride1 + copy], 1u);
    }
    __syncthreads();
    // flush: thread t owns bin t
    unsigned long long total = 0;
    for (int w = 0; w < kHistWaves; ++w)
        for (int c = 0; c < stride1; ++c) total += lds[w * kPerWave + threadIdx.x * stride1 + c];
    if (total) atomicAdd(&hist[threadIdx.x], total);
}

}  // namespace sk

extern "C" int sk_u8_histogram(const uint8_t* x, int64_t n, unsigned long long* hist256, void* stream) {
    SK_CHECK_ARG(hist256 != nullptr, "sk_u8_histogram: hist256 is NULL");
    SK_CHECK_ARG(n >= 0 && n <= sk::kHistMaxN, "sk_u8_histogram: n = %lld outside [0, 2^40]", (long long)n);
    SK_CHECK_ARG(n == 0 || x != nullptr, "sk_u8_histogram: x is NULL with n = %lld", (long long)n);
    SK_CHECK_ARG(((uintptr_t)hist256 & 7) == 0, "sk_u8_histogram: hist256 must be 8-byte aligned");
    if (n == 0) return SK_OK;
    int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 16, tail = (n - head) % 16;
    int variant = sk::kDefaultVariant;
#ifdef SK_TUNING
    if (const char* e = getenv("SK_HIST_VARIANT")) variant = atoi(e) == sk::kMatch ? sk::kMatch : sk::kCopies;
#endif
    // 4 loads of 16 bytes per thread before the grid cap (256 CUs x 8 workgroups) takes over
    unsigned grid = sk::stream_grid(nvec, sk::kHistBlock, 4);
    if (grid > 256 * 8) grid = 256 * 8;
    hipStream_t st = (hipStream_t)stream;
    if (variant == sk::kMatch)
        hipLaunchKernelGGL(sk::u8_histogram_kernel<sk::kMatch>, dim3(grid), dim3(sk::kHistBlock), 0, st, x, head, nvec, tail,
                           hist256);
    else
        hipLaunchKernelGGL(sk::u8_histogram_kernel<sk::kCopies>, dim3(grid), dim3(sk::kHistBlock), 0, st, x, head, nvec, tail,
                           hist256);
    SK_CHECK_LAUNCH();
    return SK_OK;
}
