#!/usr/bin/env python
"""Run skoots_amd/csrc/skeletonize.hip on the CPU under AddressSanitizer + UBSan before it runs on a device: the
thinning, the new graph kernel and the emit kernel, in the order ``validate.lib.instance_skeleton_graph`` calls them.

As tools/instance_mesh_host_check.py does for its kernel: the file's text is compiled as host C++ behind a small shim
into a stand-alone program.  A workgroup is 256 host threads, ``__syncthreads`` is a barrier over them, ``__shfl_down``
goes through an array between two barriers, the LDS arrays are static arrays and the atomics are the compiler's;
workgroups run one after another.  Labels, workspace, graph and points are heap blocks of exactly the arrays' sizes, so
an access past either end of any of them, or of an LDS array, is a sanitizer report.  Every case of
tests/skeleton_graph_cases.py is thinned instance by instance in its full box and compared, exactly, with the golden
skeletons of scikit-image 0.18.3 (the points) and with the numpy oracle of tests/test_skeleton_graph_cpu.py on them
(the graph rows); two more runs thin ``tests.test_skeletonize.large_object()`` in its box and in the whole volume,
which does not fit the LDS path.

    python tools/skeleton_graph_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the bit planes and the reduction as written; what only a device has (real wave shuffles, LDS,
the hardware's scheduling) it cannot see.
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
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "skoots_hip.h"
using std::max;
using std::min;
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 blockIdx, threadIdx, gridDim;
typedef void* hipStream_t;
static pthread_barrier_t g_block;
static void shim_init() { pthread_barrier_init(&g_block, nullptr, 256); }
#define __syncthreads() pthread_barrier_wait(&g_block)
#define __threadfence() __atomic_thread_fence(__ATOMIC_SEQ_CST)
static int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static long long g_shfl[256];
static long long __shfl_down(long long v, int step, int width) {
    const int t = threadIdx.x;
    g_shfl[t] = v;
    pthread_barrier_wait(&g_block);
    const long long r = (t & 63) + step < width ? g_shfl[t + step] : v;
    pthread_barrier_wait(&g_block);
    return r;
}
enum { hipMemcpyHostToDevice = 1, hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
static int hipMemcpyAsync(void* d, const void* s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
static int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
static int hipFuncSetAttribute(const void*, int, int) { return 0; }
static int hipStreamSynchronize(hipStream_t) { return 0; }
static char g_err[512];
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof(g_err), __VA_ARGS__); return SK_ERR_ARG; } } while (0)
#define SK_CHECK_HIP(expr) do { if ((expr) != 0) return SK_ERR_HIP; } while (0)
#define SK_CHECK_LAUNCH() do {} while (0)
#define LAUNCH(kernel, grid, ...) \
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
int main(int argc, char** argv) {   // lab.bin X Y Z ids.bin boxes.bin n graph.bin points.bin n_points
    if (argc != 11) return 2;
    shim_init();
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), n = atoi(argv[7]);
    const long long n_points = atoll(argv[10]);
    int32_t* lab = slurp<int32_t>(argv[1], (size_t)X * Y * Z);
    int32_t* ids = slurp<int32_t>(argv[5], n);
    int32_t* boxes = slurp<int32_t>(argv[6], 6 * (size_t)n);
    int64_t* want = slurp<int64_t>(argv[8], 12 * (size_t)n);
    int32_t* want_points = slurp<int32_t>(argv[9], 3 * (size_t)n_points);
    const size_t bytes = sk_skeletonize_workspace_bytes(boxes, n);
    void* work = nullptr;
    if (!bytes || posix_memalign(&work, 16, bytes)) return 4;
    memset(work, 0xCD, bytes);
    int32_t* counts = (int32_t*)malloc(4 * (size_t)n);
    int32_t* stats = (int32_t*)malloc(8 * (size_t)n);
    int32_t error = -1;
    if (sk_skeletonize(lab, X, Y, Z, ids, boxes, n, work, bytes, counts, stats, &error, nullptr) != SK_OK || error)
        return 5;
    if (sk_skeleton_graph_row_values() != 12) return 6;
    int64_t* graph = (int64_t*)malloc(96 * (size_t)n);
    memset(graph, 0xAB, 96 * (size_t)n);
    if (sk_skeleton_graph(boxes, n, work, bytes, graph, nullptr) != SK_OK) return 7;
    // the argument checks: nothing is launched
    if (sk_skeleton_graph(boxes, n, work, bytes - 1, graph, nullptr) != SK_ERR_ARG) return 8;
    if (sk_skeleton_graph(boxes, n, nullptr, bytes, graph, nullptr) != SK_ERR_ARG) return 8;
    if (sk_skeleton_graph(boxes, n, work, bytes, nullptr, nullptr) != SK_ERR_ARG) return 8;
    if (sk_skeleton_graph(nullptr, n, work, bytes, graph, nullptr) != SK_ERR_ARG) return 8;
    if (sk_skeleton_graph(boxes, 0, work, bytes, graph, nullptr) != SK_ERR_ARG) return 8;
    size_t bad = 0, bad_counts = 0, bad_points = 0;
    for (size_t i = 0; i < 12 * (size_t)n; ++i) bad += graph[i] != want[i];
    int32_t* offsets = (int32_t*)malloc(4 * ((size_t)n + 1));
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) {
        offsets[i + 1] = offsets[i] + counts[i];
        bad_counts += counts[i] != graph[12 * (size_t)i];
    }
    if (offsets[n] != n_points) return 9;
    int32_t* points = (int32_t*)malloc(12 * (size_t)n_points + (n_points == 0));
    if (sk_skeletonize_emit(boxes, n, work, bytes, offsets, n_points, points, nullptr) != SK_OK) return 10;
    for (size_t i = 0; i < 3 * (size_t)n_points; ++i) bad_points += points[i] != want_points[i];
    printf("%d objects, %lld points: %zu graph, %zu count, %zu point mismatches", n, n_points, bad, bad_counts,
           bad_points);
    free(lab); free(ids); free(boxes); free(want); free(want_points); free(work); free(counts); free(stats);
    free(graph); free(offsets); free(points);
    return bad || bad_counts || bad_points ? 1 : 0;
}
"""


def build(workdir, main=MAIN):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "skeletonize.hip")) as f:
        text = f.read()
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(\w+_kernel)<<<n, kThreads, [^>]*>>>\(", r"LAUNCH(\1, n, ", text)
    if n != 6:
        raise SystemExit(f"skeletonize.hip: expected 6 launches, found {n}: the shim needs an update")
    text, n = re.subn(r"extern __shared__ __attribute__\(\(aligned\(16\)\)\) uint32_t lds_planes\[\];",
                      "static uint32_t lds_planes[kLdsBytes / 4];", text)
    if n != 1:
        raise SystemExit("skeletonize.hip: the dynamic LDS declaration changed: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "skeletonize_host.cpp"), "w") as f:
        f.write(text + main)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "skeletonize_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "skeletonize_host.cpp")])
    return exe


def run(exe, workdir, label, rows, skeleton_rows, graph, whole_volume=False):
    """rows (X, Y, Z) int32: the instances as 1 .. N; skeleton_rows: their golden skeletons, labelled alike; every
    instance is thinned in its own box, or in the whole volume"""
    n = int(rows.max())
    boxes, points = [], []
    for r in range(1, n + 1):
        nz = np.argwhere(rows == r)
        lo, hi = (np.zeros(3, np.int64), np.array(rows.shape)) if whole_volume else (nz.min(0), nz.max(0) + 1)
        boxes.append(np.concatenate((lo, hi)))
        points.append(np.argwhere(skeleton_rows == r) - lo)
    arrays = (np.ascontiguousarray(rows, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32),
              np.array(boxes, np.int32), np.ascontiguousarray(graph, dtype=np.int64),
              np.concatenate(points).astype(np.int32))
    paths = [os.path.join(workdir, f) for f in ("lab.bin", "ids.bin", "boxes.bin", "graph.bin", "points.bin")]
    for p, a in zip(paths, arrays):
        a.tofile(p)
    r = subprocess.run([exe, paths[0]] + [str(s) for s in rows.shape] + [paths[1], paths[2], str(n), paths[3], paths[4],
                                                                         str(arrays[4].shape[0])],
                       capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    from tests.skeleton_graph_cases import cases, positive_ids
    from tests.test_skeleton_graph_cpu import golden_rows, skeleton_graph_oracle, want_graph
    from tests.test_skeletonize import golden, large_object
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            ids = positive_ids(lab)
            rows = (np.searchsorted(ids, lab.clip(min=0)) + 1) * (lab > 0)
            run(exe, workdir, label, rows, golden_rows(label), want_graph(label, lab)[1])
            runs += 1
        big = large_object().astype(np.int32)
        skel = np.zeros(big.shape, np.int32)
        skel[tuple(golden()["c_points"].astype(np.int64).T)] = 1
        for whole in (False, True):
            run(exe, workdir, f"large object (84, 84, 40), whole volume: {whole}", big, skel,
                skeleton_graph_oracle(skel)[1], whole)
            runs += 1
    print(f"{runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
