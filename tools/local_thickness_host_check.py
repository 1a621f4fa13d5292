#!/usr/bin/env python
"""Run skoots_amd/csrc/local_thickness.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/nearest_label_host_check.py does for its kernels: the file's text is compiled as host C++ behind a small shim
into a stand-alone program.  The kernel uses no wave-level primitive and no LDS -- a lane's work depends on its centre
and its lane number only -- so a workgroup is a loop over its 256 threads, the atomic maximum is a plain one, and the
grid is two workgroups, so the loop over the centre list takes many turns.  dist2, thick2 and the centre list are heap
blocks of exactly the arrays' sizes, so an access past either end of any of them is a sanitizer report.  Every case of
tests/local_thickness_cases.py runs at the four spacings, open and closed, three times: all centres in one call, the
centres in reversed order in calls of three, and with every voxel of the volume as a centre (background and infinite
ones, which must paint nothing); thick2 is compared bit for bit with the numpy statement; the argument checks are
called with an output that must stay untouched.

    python tools/local_thickness_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing and the boxes as written; what only a device has (the hardware's scheduling, its atomics and its
floating point) it cannot see.
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
#include <algorithm>
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
using std::max;
using std::min;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
namespace sk { static unsigned stream_grid(long long n, int block) { return n > block ? 2u : 1u; } }
static char g_err[512];
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof(g_err), __VA_ARGS__); return SK_ERR_ARG; } } while (0)
#define SK_CHECK_LAUNCH() do {} while (0)
static long long __double_as_longlong(double v) { long long b; memcpy(&b, &v, 8); return b; }
static void atomicMax(unsigned long long* p, unsigned long long v) { if (*p < v) *p = v; }
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
// X Y Z, then per run: wx wy wz dist2.bin centres.bin n_centres thick2.bin
int main(int argc, char** argv) {
    if (argc < 4 || (argc - 4) % 7) return 2;
    const int X = atoi(argv[1]), Y = atoi(argv[2]), Z = atoi(argv[3]);
    const size_t n = (size_t)X * Y * Z;
    double* t2 = (double*)malloc(8 * n);
    size_t bad = 0, bad_split = 0, bad_all = 0, runs = 0, refused = 0;
    for (int a = 4; a < argc; a += 7, ++runs) {
        const double wx = strtod(argv[a], nullptr), wy = strtod(argv[a + 1], nullptr), wz = strtod(argv[a + 2], nullptr);
        double* d2 = slurp<double>(argv[a + 3], n);
        const long long nc = atoll(argv[a + 5]);
        int64_t* centres = slurp<int64_t>(argv[a + 4], (size_t)nc);
        double* want = slurp<double>(argv[a + 6], n);
        // every centre in one call
        memcpy(t2, d2, 8 * n);
        if (sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, centres, nc, t2, nullptr) != SK_OK) return 5;
        bad += memcmp(t2, want, 8 * n) != 0;
        // reversed, three centres a call: each slice is its own heap block
        memcpy(t2, d2, 8 * n);
        for (long long hi = nc; hi > 0; hi -= 3) {
            const long long lo = hi > 3 ? hi - 3 : 0;
            int64_t* part = (int64_t*)malloc(8 * (size_t)(hi - lo));
            for (long long k = lo; k < hi; ++k) part[hi - 1 - k] = centres[k];
            if (sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, part, hi - lo, t2, nullptr) != SK_OK) return 6;
            free(part);
        }
        bad_split += memcmp(t2, want, 8 * n) != 0;
        // every voxel a centre: background (0) and infinite ones paint nothing, the small balls only themselves
        int64_t* every = (int64_t*)malloc(8 * n);
        for (size_t k = 0; k < n; ++k) every[k] = (int64_t)k;
        memcpy(t2, d2, 8 * n);
        if (sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, every, (int64_t)n, t2, nullptr) != SK_OK) return 7;
        bad_all += memcmp(t2, want, 8 * n) != 0;
        free(every);
        // the argument checks: nothing is launched or written
        memset(t2, 0xAB, 8 * n);
        const double inf = INFINITY, nan = NAN;
        int rc[] = {
            sk_local_thickness_paint(nullptr, X, Y, Z, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, nullptr, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, centres, nc, nullptr, nullptr),
            sk_local_thickness_paint(t2, X, Y, Z, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, centres, -1, t2, nullptr),
            sk_local_thickness_paint(d2, -1, Y, Z, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, -1, Z, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, -1, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, (1 << 26) + 1, 1, 1, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, 1 << 26, 1 << 26, 1 << 26, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, 0.0, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, -1.0, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, inf, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, nan, centres, nc, t2, nullptr),
            sk_local_thickness_paint((double*)((char*)d2 + 4), X, Y, Z, wx, wy, wz, centres, nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, (int64_t*)((char*)centres + 4), nc, t2, nullptr),
            sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, centres, nc, (double*)((char*)t2 + 4), nullptr)};
        for (int v : rc) {
            if (n && nc && v != SK_ERR_ARG) return 8;
            ++refused;
        }
        // no centre, or an empty volume, is not an error and writes nothing
        if (sk_local_thickness_paint(d2, X, Y, Z, wx, wy, wz, centres, 0, t2, nullptr) != SK_OK ||
            sk_local_thickness_paint(nullptr, X, Y, Z, wx, wy, wz, nullptr, 0, nullptr, nullptr) != SK_OK ||
            sk_local_thickness_paint(d2, 0, Y, Z, wx, wy, wz, centres, nc, t2, nullptr) != SK_OK ||
            sk_local_thickness_paint(nullptr, X, 0, Z, wx, wy, wz, nullptr, nc, nullptr, nullptr) != SK_OK)
            return 9;
        if (!all_bytes(t2, 8 * n, 0xAB)) return 10;
        free(d2); free(centres); free(want);
    }
    printf("%zu runs, %zu refused calls: %zu whole, %zu split, %zu every-voxel mismatches", runs, refused, bad, bad_split,
           bad_all);
    free(t2);
    return bad || bad_split || bad_all ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "local_thickness.hip")) as f:
        text = f.read()
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"lt_paint_kernel<<<grid, kThreads, 0, \(hipStream_t\)stream>>>\(", "LAUNCH(lt_paint_kernel, grid, ",
                      text)
    if n != 1:
        raise SystemExit(f"local_thickness.hip: expected 1 launch, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "local_thickness_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "local_thickness_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "local_thickness_host.cpp")])
    return exe


def centres_of(d2, w):
    """the centre list of ``lib.morphology.paint_centres``: finite, above min(w), raster order"""
    flat = np.asarray(d2).reshape(-1)
    return np.flatnonzero(np.isfinite(flat) & (flat > min(w))).astype(np.int64)


def run(exe, workdir, label, lab):
    from tests.local_thickness_cases import MODES, SPACINGS, expected, weights
    args = [exe] + [str(s) for s in lab.shape]
    k = 0
    for spacing in SPACINGS:
        for closed in MODES:
            _, _, d2, t2 = expected(label, spacing, closed)
            w = weights(spacing)
            centres = centres_of(d2, w)
            paths = [os.path.join(workdir, f"{n}{k}.bin") for n in ("d", "c", "t")]
            np.ascontiguousarray(d2).tofile(paths[0])
            centres.tofile(paths[1])
            np.ascontiguousarray(t2).tofile(paths[2])
            args += [float(v).hex() for v in w] + [paths[0], paths[1], str(centres.size), paths[2]]
            k += 1
    r = subprocess.run(args, capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)
    return k


def main():
    from tests.local_thickness_cases import cases
    n_cases = runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            runs += run(exe, workdir, label, lab)
            n_cases += 1
    print(f"{n_cases} cases, {runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
