#!/usr/bin/env python
"""Run skoots_amd/csrc/instance_stats.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

The kernel's text is compiled as host C++ behind a small shim: a workgroup is 256 host threads, ``__syncthreads`` is
a barrier over them, and the wave operations (``__shfl_up``, ``__shfl``, ``__ballot``) exchange values through one
array per wave between two barriers over the wave's 64 threads; the LDS arrays are static arrays and the atomics are
the compiler's.  Workgroups run one after another.  Mask, table, sums and boxes are heap blocks of exactly the arrays'
sizes, so an access past either end of any of them, or of an LDS array, is a sanitizer report.  Every case is compared
with the numpy oracle of tests/test_hip_instance_stats.py, exactly.

    python tools/instance_stats_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the halo, the run logic, the table and both accumulation paths as written; what only a device
has (real LDS atomics, the hardware's wave scheduling) it cannot see.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHIM = r"""
#pragma once
#include <pthread.h>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "skoots_hip.h"
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
static pthread_barrier_t g_block, g_wave[4];
static unsigned long long g_xch[4][64];
static void shim_init() {
    pthread_barrier_init(&g_block, nullptr, 256);
    for (int w = 0; w < 4; ++w) pthread_barrier_init(&g_wave[w], nullptr, 64);
}
#define __syncthreads() pthread_barrier_wait(&g_block)
template <class T> static T wave_read(T v, int src) {      // every lane of the wave calls this together
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = (unsigned long long)(long long)v;
    pthread_barrier_wait(&g_wave[w]);
    const T r = (T)g_xch[w][src];
    pthread_barrier_wait(&g_wave[w]);
    return r;
}
template <class T> static T __shfl_up(T v, int d) { const int l = threadIdx.x & 63; return wave_read(v, l >= d ? l - d : l); }
template <class T> static T __shfl(T v, int src) { return wave_read(v, src & 63); }
static unsigned long long __ballot(bool p) {
    unsigned long long m = 0;
    const unsigned long long mine = p ? 1 : 0;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = mine;
    pthread_barrier_wait(&g_wave[w]);
    for (int i = 0; i < 64; ++i) m |= g_xch[w][i] << i;
    pthread_barrier_wait(&g_wave[w]);
    return m;
}
static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static int atomicCAS(int* p, int expect, int v) { __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }
static int atomicMin(int* p, int v) { int o = __atomic_load_n(p, __ATOMIC_RELAXED); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
static int atomicMax(int* p, int v) { int o = __atomic_load_n(p, __ATOMIC_RELAXED); while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
namespace sk { static unsigned stream_grid(int64_t n, int block) { int64_t g = (n + block - 1) / block; return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g); } }
static int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return SK_ERR_ARG; } } while (0)
#define SK_CHECK_HIP(expr) do { if ((expr) != 0) return SK_ERR_HIP; } while (0)
#define SK_CHECK_LAUNCH() do {} while (0)
#define LAUNCH(kernel, grid, block, ...) \
    for (unsigned b_ = 0, g_ = (grid); b_ < g_; ++b_) { \
        std::vector<std::thread> th_; \
        for (unsigned t_ = 0; t_ < 256u; ++t_) \
            th_.emplace_back([=] { blockIdx.x = b_; threadIdx.x = t_; gridDim.x = g_; kernel(__VA_ARGS__); }); \
        for (auto& t : th_) t.join(); \
    }
"""

MAIN = r"""
template <class T> static T* slurp(const char* path, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    FILE* f = fopen(path, "rb");
    if (!f || fread(p, sizeof(T), n, f) != n) exit(3);
    fclose(f);
    return p;
}
int main(int argc, char** argv) {   // lab.bin X Y Z lut.bin max_id N sums.bin boxes.bin
    if (argc != 10) return 2;
    shim_init();
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), max_id = atoi(argv[6]), N = atoi(argv[7]);
    int32_t* lab = slurp<int32_t>(argv[1], (size_t)X * Y * Z);
    int32_t* lut = slurp<int32_t>(argv[5], (size_t)max_id + 1);
    int64_t* want_s = slurp<int64_t>(argv[8], (size_t)N * 13);
    int32_t* want_b = slurp<int32_t>(argv[9], (size_t)N * 6);
    int64_t* sums = (int64_t*)malloc((size_t)N * 13 * 8 + (N == 0));
    int32_t* boxes = (int32_t*)malloc((size_t)N * 6 * 4 + (N == 0));
    memset(sums, 0xAB, (size_t)N * 13 * 8);
    memset(boxes, 0xAB, (size_t)N * 6 * 4);
    if (sk_instance_stats(lab, X, Y, Z, lut, max_id, N, sums, boxes, nullptr) != SK_OK) return 5;
    size_t bad = 0;
    for (size_t i = 0; i < (size_t)N * 13; ++i) bad += sums[i] != want_s[i];
    for (size_t i = 0; i < (size_t)N * 6; ++i) bad += boxes[i] != want_b[i];
    printf("%d rows, %zu mismatches", N, bad);
    free(lab); free(lut); free(want_s); free(want_b); free(sums); free(boxes);
    return bad ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_stats.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(instance_stats\w*_kernel)<<<([^;]*?), kThreads, 0, st>>>\(", r"LAUNCH(\1, \2, kThreads, ", text,
                      flags=re.S)
    if n != 2:
        raise SystemExit(f"instance_stats.hip: expected 2 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "instance_stats_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "instance_stats_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "instance_stats_host.cpp")])
    return exe


def run(exe, workdir, lab, label, oracle):
    ids, sums, boxes = oracle(lab)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    max_id = int(ids.max()) if len(ids) else 0
    lut = np.zeros(max_id + 1, np.int32)
    lut[ids] = np.arange(1, len(ids) + 1)
    paths = [os.path.join(workdir, n) for n in ("lab.bin", "lut.bin", "sums.bin", "boxes.bin")]
    for p, a in zip(paths, (lab, lut, sums.astype(np.int64), boxes.astype(np.int32))):
        a.tofile(p)
    r = subprocess.run([exe, paths[0]] + [str(s) for s in lab.shape] + [paths[1], str(max_id), str(len(ids)),
                                                                         paths[2], paths[3]],
                       capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})")
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    from tests.test_hip_instance_stats import blobs, oracle
    cases = []
    lab = blobs((19, 45, 130), 30, seed=18)
    lab[2:9, 3:12, 60:70] = 41000
    lab[2:9, 12:20, 60:70] = 41001
    lab[:, 22, 64] = lab[9, :, 64] = 77777
    lab[9, 22, :] = 77777
    lab[0, 0, 0], lab[18, 44, 129] = 90001, 90002
    cases.append(("blobs (19, 45, 130)", lab))
    rng = np.random.default_rng(5)
    cases.append(("own label per voxel (8, 16, 64)", (rng.permutation(8 * 16 * 64) + 1).reshape(8, 16, 64)))
    cases.append(("checkerboard (6, 18, 70)", np.indices((6, 18, 70)).sum(0) % 2 + 1))
    for shape in ((1, 1, 1), (5, 1, 1), (1, 1, 70), (3, 70, 1), (8, 9, 10)):
        cases.append((f"one label {shape}", np.full(shape, 3)))
        cases.append((f"random {shape}", np.random.default_rng(sum(shape)).integers(0, 4, shape) * 7))
    cases.append(("all background (4, 5, 6)", np.zeros((4, 5, 6))))
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases:
            run(exe, workdir, lab, label, oracle)
    print(f"{len(cases)} cases, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
