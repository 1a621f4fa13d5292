#!/usr/bin/env python
"""Run skoots_amd/csrc/instance_mesh.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/instance_stats_host_check.py does for its kernel: the kernel's text is compiled as host C++ behind a small
shim into a stand-alone program.  A workgroup is 256 host threads, ``__syncthreads`` is a barrier over them, the LDS
arrays are static arrays and the atomics are the compiler's; workgroups run one after another.  Mask, look-up table,
class table and counts are heap blocks of exactly the arrays' sizes, so an access past either end of any of them, or of
an LDS array, is a sanitizer report.  Every case of tests/test_hip_surface_area.py runs in both modes and is compared,
exactly, with the numpy oracle of tests/test_surface_area_cpu.py; one more run hands the kernel a row narrower than the
table's classes, which must skip those cells and write nothing past the row.

    python tools/instance_mesh_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the shifted tile grid of closed mode, the table and both accumulation paths as written; what
only a device has (real LDS atomics, the hardware's wave scheduling) it cannot see.
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
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
static pthread_barrier_t g_block;
static void shim_init() { pthread_barrier_init(&g_block, nullptr, 256); }
#define __syncthreads() pthread_barrier_wait(&g_block)
static unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static int atomicCAS(int* p, int expect, int v) { __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }
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
int main(int argc, char** argv) {   // lab.bin X Y Z lut.bin max_id N class_of.bin n_classes closed cells.bin
    if (argc != 12) return 2;
    shim_init();
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), max_id = atoi(argv[6]), N = atoi(argv[7]);
    const int n_classes = atoi(argv[9]), closed = atoi(argv[10]);
    int32_t* lab = slurp<int32_t>(argv[1], (size_t)X * Y * Z);
    int32_t* lut = slurp<int32_t>(argv[5], (size_t)max_id + 1);
    uint8_t* class_of = slurp<uint8_t>(argv[8], 256);
    int64_t* want = slurp<int64_t>(argv[11], (size_t)N * n_classes);
    int64_t* cells = (int64_t*)malloc((size_t)N * n_classes * 8 + (N == 0));
    memset(cells, 0xAB, (size_t)N * n_classes * 8);
    if (sk_instance_mesh_cells(lab, X, Y, Z, lut, max_id, N, class_of, n_classes, closed, cells, nullptr) != SK_OK)
        return 5;
    size_t bad = 0;
    for (size_t i = 0; i < (size_t)N * n_classes; ++i) bad += cells[i] != want[i];
    printf("%d rows, %zu mismatches", N, bad);
    free(lab); free(lut); free(class_of); free(want); free(cells);
    return bad ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_mesh.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(instance_mesh\w*_kernel)<<<([^;]*?), kThreads, 0, st>>>\(", r"LAUNCH(\1, \2, kThreads, ", text,
                      flags=re.S)
    if n != 1:
        raise SystemExit(f"instance_mesh.hip: expected 1 launch, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "instance_mesh_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "instance_mesh_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "instance_mesh_host.cpp")])
    return exe


def run(exe, workdir, lab, label, closed, n_classes, oracle, class_of):
    ids, cells = oracle(lab, closed)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    max_id = int(ids.max()) if len(ids) else 0
    lut = np.zeros(max_id + 1, np.int32)
    lut[ids] = np.arange(1, len(ids) + 1)
    paths = [os.path.join(workdir, n) for n in ("lab.bin", "lut.bin", "class_of.bin", "cells.bin")]
    want = np.ascontiguousarray(cells[:, :n_classes], dtype=np.int64)
    for p, a in zip(paths, (lab, lut, class_of, want)):
        a.tofile(p)
    r = subprocess.run([exe, paths[0]] + [str(s) for s in lab.shape] + [paths[1], str(max_id), str(len(ids)), paths[2],
                                                                         str(n_classes), str(int(closed)), paths[3]],
                       capture_output=True, text=True)
    print(f"{label}, {'closed' if closed else 'open'}, {n_classes} classes: {r.stdout.strip()} (exit {r.returncode})")
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    from skoots_amd.validate.mc_table import CLASS_OF, CLASS_TRIANGLES
    from tests.test_hip_surface_area import cases
    from tests.test_surface_area_cpu import mesh_cells_oracle
    class_of = np.array(CLASS_OF, np.uint8)
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            for closed in (False, True):
                run(exe, workdir, lab, label, closed, len(CLASS_TRIANGLES), mesh_cells_oracle, class_of)
                runs += 1
        label = "all configurations (12, 24, 24)"
        run(exe, workdir, cases()[label], label, True, 7, mesh_cells_oracle, class_of)
        runs += 1
    print(f"{runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
