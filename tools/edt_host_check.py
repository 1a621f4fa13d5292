#!/usr/bin/env python
"""Run skoots_amd/csrc/edt.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/skeleton_graph_host_check.py does for its kernels: the file's text is compiled as host C++ behind a small shim
into a stand-alone program.  A workgroup is 256 host threads; ``__ballot``, ``__shfl`` and ``__shfl_xor`` go through an
array between two barriers of the wave's 64 threads, the atomic is the compiler's, and the grid is two workgroups that
run one after another, so the grid-stride loop takes many turns.  Labels, lut, dist2, scratch and row_max are heap blocks
of exactly the arrays' sizes, so an access past either end of any of them is a sanitizer report.  Every case of
tests/edt_cases.py runs at the four spacings, open and closed, through ``sk_label_edt`` and once more pass by pass through
``sk_label_edt_pass``, and dist2 and row_max are compared bit for bit with the numpy oracle; the argument checks are
called with outputs that must stay untouched.

    python tools/edt_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the walk and the reduction as written; what only a device has (real wave shuffles, the
hardware's scheduling and its floating point) it cannot see.
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
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "skoots_hip.h"
using std::fmin;
#define __device__
#define __global__
#define __launch_bounds__(x)
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
static pthread_barrier_t g_wave[4];
static void shim_init() { for (auto& b : g_wave) pthread_barrier_init(&b, nullptr, 64); }
static unsigned long long g_lanes[256];
static unsigned long long wave_exchange(unsigned long long v, int src_lane) {
    const int t = threadIdx.x, w = t >> 6;
    g_lanes[t] = v;
    pthread_barrier_wait(&g_wave[w]);
    const unsigned long long r = g_lanes[(t & ~63) + (src_lane & 63)];
    pthread_barrier_wait(&g_wave[w]);
    return r;
}
static int __shfl(int v, int lane) { return (int)wave_exchange((unsigned long long)(unsigned)v, lane); }
static unsigned long long __shfl_xor(unsigned long long v, int mask) { return wave_exchange(v, (threadIdx.x & 63) ^ mask); }
static unsigned long long __ballot(bool pred) {
    const int t = threadIdx.x, w = t >> 6;
    g_lanes[t] = pred;
    pthread_barrier_wait(&g_wave[w]);
    unsigned long long r = 0;
    for (int i = 0; i < 64; ++i) r |= (unsigned long long)(g_lanes[(t & ~63) + i] != 0) << i;
    pthread_barrier_wait(&g_wave[w]);
    return r;
}
static long long __double_as_longlong(double v) { long long r; memcpy(&r, &v, 8); return r; }
static unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
namespace sk { static unsigned stream_grid(long long n, int block) { return n > block ? 2u : 1u; } }
static char g_err[512];
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof(g_err), __VA_ARGS__); return SK_ERR_ARG; } } while (0)
#define SK_CHECK_HIP(expr) do { if ((expr) != 0) return SK_ERR_HIP; } while (0)
static int atomicCAS(int* p, int expect, int v) { __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }   // instance_rows.h: claim_slot
#define SK_CHECK_LAUNCH() do {} while (0)
#define LAUNCH(kernel, grid, ...) \
    do for (unsigned b_ = 0, g_ = (grid); b_ < g_; ++b_) { \
        std::vector<std::thread> th_; \
        for (unsigned t_ = 0; t_ < 256u; ++t_) \
            th_.emplace_back([=] { blockIdx.x = b_; threadIdx.x = t_; gridDim.x = g_; kernel(__VA_ARGS__); }); \
        for (auto& t : th_) t.join(); \
    } while (0)
"""

MAIN = r"""
template <class T> static T* slurp(const char* path, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    FILE* f = fopen(path, "rb");
    if (!f || fread(p, sizeof(T), n, f) != n) exit(3);
    fclose(f);
    return p;
}
// lab.bin X Y Z lut.bin max_id N, then per run: wx wy wz closed dist2.bin row_max.bin
int main(int argc, char** argv) {
    if (argc < 8 || (argc - 8) % 6) return 2;
    shim_init();
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), max_id = atoi(argv[6]), N = atoi(argv[7]);
    const size_t n = (size_t)X * Y * Z;
    int32_t* lab = slurp<int32_t>(argv[1], n);
    int32_t* lut = slurp<int32_t>(argv[5], (size_t)max_id + 1);
    double* dist2 = (double*)malloc(8 * n);
    double* scratch = (double*)malloc(8 * n);
    uint64_t* row_max = (uint64_t*)malloc(8 * (size_t)N);
    size_t bad = 0, bad_max = 0, bad_pass = 0, runs = 0;
    for (int a = 8; a < argc; a += 6, ++runs) {
        const double wx = strtod(argv[a], nullptr), wy = strtod(argv[a + 1], nullptr), wz = strtod(argv[a + 2], nullptr);
        const int closed = atoi(argv[a + 3]);
        double* want = slurp<double>(argv[a + 4], n);
        uint64_t* want_max = slurp<uint64_t>(argv[a + 5], N);
        memset(dist2, 0xCD, 8 * n);
        memset(scratch, 0xCD, 8 * n);
        memset(row_max, 0xCD, 8 * (size_t)N);
        if (sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr) != SK_OK)
            return 5;
        bad += memcmp(dist2, want, 8 * n) != 0;
        bad_max += memcmp(row_max, want_max, 8 * (size_t)N) != 0;
        // pass by pass, row_max from the last one, and without row_max
        memset(dist2, 0xCD, 8 * n);
        memset(row_max, 0xCD, 8 * (size_t)N);
        if (sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 2, wz, closed, nullptr, dist2, nullptr, nullptr) != SK_OK ||
            sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 1, wy, closed, dist2, scratch, nullptr, nullptr) != SK_OK ||
            sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, closed, scratch, dist2, row_max, nullptr) != SK_OK)
            return 6;
        bad_pass += memcmp(dist2, want, 8 * n) != 0 || memcmp(row_max, want_max, 8 * (size_t)N) != 0;
        // the argument checks: nothing is launched or written
        memset(dist2, 0xAB, 8 * n);
        memset(row_max, 0xAB, 8 * (size_t)N);
        const double inf = INFINITY;
        int rc[] = {
            sk_label_edt(nullptr, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, nullptr, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, nullptr, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, nullptr, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, dist2, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, 2, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, 0.0, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, -1.0, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, inf, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, -1, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, -1, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, -1, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, (1 << 26) + 1, 1, 1, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr),
            sk_label_edt(lab, 1 << 26, 1 << 26, 1 << 26, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max,
                         nullptr),
            sk_label_edt(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, closed, (double*)((char*)dist2 + 4), scratch, row_max,
                         nullptr),
            sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 3, wx, closed, scratch, dist2, row_max, nullptr),
            sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 1, wx, closed, nullptr, dist2, row_max, nullptr),
            sk_label_edt_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, closed, dist2, dist2, row_max, nullptr)};
        for (int v : rc)
            if (v != SK_ERR_ARG) return 7;
        for (size_t i = 0; i < 8 * n; ++i)
            if (((unsigned char*)dist2)[i] != 0xAB) return 8;
        for (size_t i = 0; i < 8 * (size_t)N; ++i)
            if (((unsigned char*)row_max)[i] != 0xAB) return 8;
        if (sk_label_edt(lab, 0, Y, Z, lut, max_id, N, wx, wy, wz, closed, dist2, scratch, row_max, nullptr) != SK_OK ||
            sk_label_edt(lab, X, Y, Z, lut, max_id, 0, wx, wy, wz, closed, dist2, scratch, row_max, nullptr) != SK_OK ||
            ((unsigned char*)dist2)[0] != 0xAB)
            return 9;
        free(want); free(want_max);
    }
    printf("%zu runs: %zu dist2, %zu row_max, %zu pass-by-pass mismatches", runs, bad, bad_max, bad_pass);
    free(lab); free(lut); free(dist2); free(scratch); free(row_max);
    return bad || bad_max || bad_pass ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "edt.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(edt_pass_kernel<\d>)<<<grid, kThreads, 0, st>>>\(", r"LAUNCH(\1, grid, ", text)
    if n != 3:
        raise SystemExit(f"edt.hip: expected 3 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "edt_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "edt_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(workdir, "edt_host.cpp")])
    return exe


def kernel_inputs(lab):
    """(labels int32, lut int32, max_id) as ``validate.lib._id_rows`` hands a mask to the kernels: the ids and a table of
    max id + 1 entries, or the rows themselves and the identity where the largest id is huge"""
    from tests.edt_cases import rows_of
    ids, rows = rows_of(lab)
    mx = int(ids.max()) if ids.size else 0
    if mx > 4 * lab.size or mx > 2 ** 31 - 1:
        return rows.astype(np.int32), np.arange(ids.size + 1, dtype=np.int32), int(ids.size)
    lut = np.zeros(mx + 1, np.int32)
    lut[ids] = np.arange(1, ids.size + 1)
    return np.ascontiguousarray(lab, dtype=np.int32), lut, mx


def run(exe, workdir, label, lab):
    from tests.edt_cases import MODES, SPACINGS, expected, row_max, weights
    a, lut, max_id = kernel_inputs(lab)
    a.tofile(os.path.join(workdir, "lab.bin"))
    lut.tofile(os.path.join(workdir, "lut.bin"))
    ids, rows, _ = expected(label, SPACINGS[0], False)
    args = [exe, os.path.join(workdir, "lab.bin")] + [str(s) for s in lab.shape] + \
        [os.path.join(workdir, "lut.bin"), str(max_id), str(ids.size)]
    k = 0
    for spacing in SPACINGS:
        for closed in MODES:
            d2 = expected(label, spacing, closed)[2]
            paths = [os.path.join(workdir, f"{n}{k}.bin") for n in ("d", "m")]
            np.ascontiguousarray(d2).tofile(paths[0])
            row_max(rows, d2).view(np.uint64).tofile(paths[1])
            args += [float(w).hex() for w in weights(spacing)] + [str(int(closed))] + paths
            k += 1
    r = subprocess.run(args, capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    from tests.edt_cases import cases
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            run(exe, workdir, label, lab)
            runs += 1
    print(f"{runs} cases, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
