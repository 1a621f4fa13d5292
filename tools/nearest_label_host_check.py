#!/usr/bin/env python
"""Run skoots_amd/csrc/nearest_label.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/edt_host_check.py does for its kernels: the file's text is compiled as host C++ behind a small shim into a
stand-alone program.  The kernels use no wave-level primitive and no LDS, so a workgroup is a loop over its 256 threads,
and the grid is two workgroups, so the grid-stride loop takes many turns.  Labels, lut, where and the four buffers of
distances and rows are heap blocks of exactly the arrays' sizes, so an access past either end of any of them is a
sanitizer report.  Every case of tests/nearest_label_cases.py runs at the four spacings and at every limit of
``limits()`` through ``sk_nearest_label`` and once more pass by pass through ``sk_nearest_label_pass``; the ``where``
volumes run on their case; dist2 and nearest are compared bit for bit with the numpy oracle; the argument checks are
called with outputs that must stay untouched.

    python tools/nearest_label_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing and the walk as written; what only a device has (the hardware's scheduling and its floating
point) it cannot see.
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
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "skoots_hip.h"
#define __device__
#define __global__
#define __launch_bounds__(x)
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
namespace sk { static unsigned stream_grid(long long n, int block) { return n > block ? 2u : 1u; } }
static char g_err[512];
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof(g_err), __VA_ARGS__); return SK_ERR_ARG; } } while (0)
static int atomicCAS(int* p, int expect, int v) { __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }   // instance_rows.h: claim_slot
#define SK_CHECK_LAUNCH() do {} while (0)
#define LAUNCH(kernel, grid, ...) \
    do for (unsigned b_ = 0, g_ = (grid); b_ < g_; ++b_) \
        for (unsigned t_ = 0; t_ < 256u; ++t_) { \
            blockIdx.x = b_; threadIdx.x = t_; gridDim.x = g_; kernel(__VA_ARGS__); \
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
static bool all_bytes(const void* p, size_t n, unsigned char v) {
    for (size_t i = 0; i < n; ++i)
        if (((const unsigned char*)p)[i] != v) return false;
    return true;
}
// lab.bin X Y Z lut.bin max_id N, then per run: wx wy wz limit2 where.bin|- dist2.bin nearest.bin
int main(int argc, char** argv) {
    if (argc < 8 || (argc - 8) % 7) return 2;
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), max_id = atoi(argv[6]), N = atoi(argv[7]);
    const size_t n = (size_t)X * Y * Z;
    int32_t* lab = slurp<int32_t>(argv[1], n);
    int32_t* lut = slurp<int32_t>(argv[5], (size_t)max_id + 1);
    double* d2 = (double*)malloc(8 * n);
    double* s2 = (double*)malloc(8 * n);
    int32_t* nr = (int32_t*)malloc(4 * n);
    int32_t* sr = (int32_t*)malloc(4 * n);
    size_t bad = 0, bad_pass = 0, runs = 0, refused = 0;
    for (int a = 8; a < argc; a += 7, ++runs) {
        const double wx = strtod(argv[a], nullptr), wy = strtod(argv[a + 1], nullptr), wz = strtod(argv[a + 2], nullptr);
        const double limit2 = strtod(argv[a + 3], nullptr);
        uint8_t* where = strcmp(argv[a + 4], "-") ? slurp<uint8_t>(argv[a + 4], n) : nullptr;
        double* want = slurp<double>(argv[a + 5], n);
        int32_t* want_row = slurp<int32_t>(argv[a + 6], n);
        memset(d2, 0xCD, 8 * n); memset(s2, 0xCD, 8 * n); memset(nr, 0xCD, 4 * n); memset(sr, 0xCD, 4 * n);
        if (sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr) != SK_OK)
            return 5;
        bad += memcmp(d2, want, 8 * n) != 0 || memcmp(nr, want_row, 4 * n) != 0;
        memset(d2, 0xCD, 8 * n); memset(s2, 0xCD, 8 * n); memset(nr, 0xCD, 4 * n); memset(sr, 0xCD, 4 * n);
        if (sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 2, wz, limit2, nullptr, nullptr, nullptr, s2, sr, nullptr) != SK_OK ||
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 1, wy, limit2, s2, sr, nullptr, d2, nr, nullptr) != SK_OK ||
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, limit2, d2, nr, where, s2, sr, nullptr) != SK_OK)
            return 6;
        bad_pass += memcmp(s2, want, 8 * n) != 0 || memcmp(sr, want_row, 4 * n) != 0;
        // the argument checks: nothing is launched or written
        memset(d2, 0xAB, 8 * n); memset(s2, 0xAB, 8 * n); memset(nr, 0xAB, 4 * n); memset(sr, 0xAB, 4 * n);
        const double inf = INFINITY, nan = NAN;
        int rc[] = {
            sk_nearest_label(nullptr, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, nullptr, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, nullptr, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nullptr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, nullptr, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, nullptr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, d2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, nr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, (int32_t*)d2, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, (int32_t*)s2, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, 0.0, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, -1.0, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, inf, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, nan, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, nan, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, -1.0, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, -inf, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, -1, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, -1, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, -1, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, (1 << 26) + 1, 1, 1, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr),
            sk_nearest_label(lab, 1 << 26, 1 << 26, 1 << 26, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr,
                             nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, (double*)((char*)d2 + 4), nr, s2, sr,
                             nullptr),
            sk_nearest_label(lab, X, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, (int32_t*)((char*)nr + 2), s2, sr,
                             nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 3, wx, limit2, s2, sr, where, d2, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, -1, wx, limit2, s2, sr, where, d2, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 1, wx, limit2, nullptr, sr, where, d2, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, limit2, s2, nullptr, where, d2, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 2, wx, limit2, nullptr, nullptr, where, nullptr, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, limit2, d2, sr, where, d2, nr, nullptr),
            sk_nearest_label_pass(lab, X, Y, Z, lut, max_id, N, 0, wx, limit2, s2, nr, where, d2, nr, nullptr)};
        for (int v : rc) {
            if (v != SK_ERR_ARG) return 7;
            ++refused;
        }
        if (!all_bytes(d2, 8 * n, 0xAB) || !all_bytes(s2, 8 * n, 0xAB) || !all_bytes(nr, 4 * n, 0xAB) ||
            !all_bytes(sr, 4 * n, 0xAB))
            return 8;
        // an empty volume writes nothing; N == 0 fills the outputs and leaves the scratch alone
        if (sk_nearest_label(lab, 0, Y, Z, lut, max_id, N, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr) != SK_OK ||
            sk_nearest_label(nullptr, X, 0, Z, nullptr, max_id, N, wx, wy, wz, limit2, where, nullptr, nullptr, nullptr,
                             nullptr, nullptr) != SK_OK ||
            !all_bytes(d2, 8 * n, 0xAB) || !all_bytes(nr, 4 * n, 0xAB))
            return 9;
        if (sk_nearest_label(lab, X, Y, Z, lut, max_id, 0, wx, wy, wz, limit2, where, d2, nr, s2, sr, nullptr) != SK_OK)
            return 10;
        for (size_t i = 0; i < n; ++i)
            if (!(d2[i] == inf) || nr[i] != 0) return 11;
        if (!all_bytes(s2, 8 * n, 0xAB) || !all_bytes(sr, 4 * n, 0xAB)) return 12;
        free(want); free(want_row); free(where);
    }
    printf("%zu runs, %zu refused calls: %zu fused, %zu pass-by-pass mismatches", runs, refused, bad, bad_pass);
    free(lab); free(lut); free(d2); free(s2); free(nr); free(sr);
    return bad || bad_pass ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "nearest_label.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(nl_pass_kernel<\d>|nl_fill_kernel)<<<grid, kThreads, 0, st>>>\(", r"LAUNCH(\1, grid, ", text)
    if n != 4:
        raise SystemExit(f"nearest_label.hip: expected 4 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "nearest_label_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "nearest_label_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "nearest_label_host.cpp")])
    return exe


def run(exe, workdir, label, lab):
    from tests.nearest_label_cases import SPACINGS, WHERE_CASE, expected, limits, weights, where_cases
    from tools.edt_host_check import kernel_inputs
    a, lut, max_id = kernel_inputs(lab)
    a.tofile(os.path.join(workdir, "lab.bin"))
    lut.tofile(os.path.join(workdir, "lut.bin"))
    ids = expected(label, SPACINGS[0])[0]
    args = [exe, os.path.join(workdir, "lab.bin")] + [str(s) for s in lab.shape] + \
        [os.path.join(workdir, "lut.bin"), str(max_id), str(ids.size)]
    wheres = {"-": None}
    if label == WHERE_CASE:
        for name, where in where_cases(lab).items():
            path = os.path.join(workdir, f"where_{len(wheres)}.bin")
            where.tofile(path)
            wheres[path] = where
    k = 0
    for spacing in SPACINGS:
        for limit2 in limits(label, spacing):
            for wpath, where in wheres.items():
                _, _, d2, near = expected(label, spacing, limit2, where)
                paths = [os.path.join(workdir, f"{n}{k}.bin") for n in ("d", "r")]
                np.ascontiguousarray(d2).tofile(paths[0])
                np.ascontiguousarray(near, dtype=np.int32).tofile(paths[1])
                args += [float(w).hex() for w in weights(spacing)] + [float(limit2).hex(), wpath] + paths
                k += 1
    r = subprocess.run(args, capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)
    return k


def main():
    from tests.nearest_label_cases import cases
    n_cases = runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            runs += run(exe, workdir, label, lab)
            n_cases += 1
    print(f"{n_cases} cases, {runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
