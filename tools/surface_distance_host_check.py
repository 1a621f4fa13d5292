#!/usr/bin/env python
"""Run skoots_amd/csrc/surface_distance.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/edt_host_check.py and tools/instance_mesh_emit_host_check.py do for their kernels, and with the latter's shim:
the file's text is compiled as host C++ into a stand-alone program.  A workgroup is 256 host threads, ``__syncthreads``
is a barrier over them, the LDS arrays are static arrays and the atomics are the compiler's; workgroups run one after
another.  Every array -- masks, look-up tables, counts, keys, offsets, pairs, distances -- is a heap block of exactly
the array's size, so an access past either end of any of them, or of an LDS array, is a sanitizer report.

  * Every mask of tests/surface_distance_cases.py: the count pass must equal the numpy oracle, the emit pass at the
    exact capacity must give exactly the oracle's keys (sorted), and at a capacity one short -- into a block one key
    shorter -- and at capacity 0 with a NULL array it must report the full count.
  * Every case at the four spacings, both directions, the synthetic key lists around the tile and workgroup sizes
    (``synthetic``) and those of a declared 2^26 x 2^26 x 4 volume, which take the 64-bit decode (``synthetic_wide``):
    ``sk_surface_distances`` must equal the oracle bit for bit.
  * The argument checks are called with outputs that must stay untouched.

    python tools/surface_distance_host_check.py     # builds into a temporary directory, prints one line per run

It checks the indexing, the tile order, the pruning and the slot arithmetic as written; what only a device has (real LDS
atomics, the hardware's scheduling and its floating point) it cannot see.
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

from tools.instance_mesh_host_check import SHIM as MESH_SHIM  # noqa: E402

SHIM = MESH_SHIM + r"""
#include <cmath>
#include <new>
namespace sk { static void set_error(const char*, ...) {} }
static int atomicMin(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static int atomicMax(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
enum { hipMemcpyDeviceToHost = 2 };
static int hipMemcpyAsync(void* dst, const void* src, size_t n, int, hipStream_t) { memcpy(dst, src, n); return 0; }
static int hipStreamSynchronize(hipStream_t) { return 0; }
#undef SK_CHECK_ARG
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) return SK_ERR_ARG; } while (0)
#undef LAUNCH
#define LAUNCH(kernel, grid, block, ...) \
    do for (unsigned b_ = 0, g_ = (grid); b_ < g_; ++b_) { \
        std::vector<std::thread> th_; \
        for (unsigned t_ = 0; t_ < 256u; ++t_) \
            th_.emplace_back([=] { blockIdx.x = b_; threadIdx.x = t_; gridDim.x = g_; kernel(__VA_ARGS__); }); \
        for (auto& t : th_) t.join(); \
    } while (0)
"""

MAIN = r"""
#include <algorithm>
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
// surface lab.bin X Y Z lut.bin max_id N counts.bin keys.bin K
static int surface_main(char** a) {
    const int X = atoi(a[1]), Y = atoi(a[2]), Z = atoi(a[3]), max_id = atoi(a[5]), N = atoi(a[6]);
    const size_t K = (size_t)atoll(a[9]);
    int32_t* lab = slurp<int32_t>(a[0], (size_t)X * Y * Z);
    int32_t* lut = slurp<int32_t>(a[4], (size_t)max_id + 1);
    int64_t* want_counts = slurp<int64_t>(a[7], N);
    int64_t* want_keys = slurp<int64_t>(a[8], K);
    int64_t* counts = (int64_t*)malloc((size_t)N * 8 + (N == 0));
    memset(counts, 0xAB, (size_t)N * 8);
    if (sk_instance_surface_count(lab, X, Y, Z, lut, max_id, N, counts, nullptr) != SK_OK) return 5;
    size_t bad = 0, total = 0;
    for (int i = 0; i < N; ++i) bad += counts[i] != want_counts[i], total += (size_t)counts[i];
    bad += total != K;
    for (int round = 0; round < 3; ++round) {               // the exact capacity, one short, none
        const size_t cap = round == 0 ? K : round == 1 ? (K ? K - 1 : 0) : 0;
        int64_t* keys = round == 2 ? nullptr : (int64_t*)malloc(cap * 8 + (cap == 0));
        int64_t* produced = (int64_t*)malloc(8);
        *produced = -1;
        if (sk_instance_surface_emit(lab, X, Y, Z, lut, max_id, N, (int64_t)cap, keys, produced, nullptr) != SK_OK) return 6;
        bad += (size_t)*produced != K;
        if (round == 0) {
            std::sort(keys, keys + K);
            for (size_t i = 0; i < K; ++i) bad += keys[i] != want_keys[i];
        }
        if (round == 1)
            for (size_t i = 0; i < cap; ++i) bad += !std::binary_search(want_keys, want_keys + K, keys[i]);
        free(keys); free(produced);
    }
    // the argument checks: nothing is launched or written
    memset(counts, 0xAB, (size_t)N * 8);
    int64_t produced = -7, key = -7;
    int rc[] = {sk_instance_surface_count(nullptr, X, Y, Z, lut, max_id, N, counts, nullptr),
                sk_instance_surface_count(lab, X, Y, Z, nullptr, max_id, N, counts, nullptr),
                sk_instance_surface_count(lab, X, Y, Z, lut, max_id, N, nullptr, nullptr),
                sk_instance_surface_count(lab, -1, Y, Z, lut, max_id, N, counts, nullptr),
                sk_instance_surface_count(lab, X, Y, Z, lut, -1, N, counts, nullptr),
                sk_instance_surface_count(lab, X, Y, Z, lut, max_id, -1, counts, nullptr),
                sk_instance_surface_count(lab, (1 << 26) + 1, 1, 1, lut, max_id, N, counts, nullptr),
                sk_instance_surface_count(lab, 1 << 26, 1 << 26, 1 << 11, lut, max_id, N, counts, nullptr),
                sk_instance_surface_count(lab, X, Y, Z, lut, max_id, N, (int64_t*)((char*)counts + 4), nullptr),
                sk_instance_surface_emit(lab, X, Y, Z, lut, max_id, N, -1, &key, &produced, nullptr),
                sk_instance_surface_emit(lab, X, Y, Z, lut, max_id, N, 1, nullptr, &produced, nullptr),
                sk_instance_surface_emit(lab, X, Y, Z, lut, max_id, N, 1, &key, nullptr, nullptr),
                sk_instance_surface_emit(lab, X, -1, Z, lut, max_id, N, 1, &key, &produced, nullptr)};
    for (int v : rc)
        if (v != SK_ERR_ARG) return 7;
    if (!all_bytes(counts, (size_t)N * 8, 0xAB) || produced != -7 || key != -7) return 8;
    if (sk_instance_surface_count(lab, 0, Y, Z, lut, max_id, N, counts, nullptr) != SK_OK ||
        sk_instance_surface_count(lab, X, Y, Z, lut, max_id, 0, counts, nullptr) != SK_OK ||
        sk_instance_surface_emit(lab, X, Y, 0, lut, max_id, N, 1, &key, &produced, nullptr) != SK_OK ||
        !all_bytes(counts, (size_t)N * 8, 0xAB) || produced != -7 || key != -7)
        return 9;
    printf("%d rows, %zu surface voxels, %zu mismatches", N, total, bad);
    free(lab); free(lut); free(want_counts); free(want_keys); free(counts);
    return bad ? 1 : 0;
}
// distances X Y Z qkeys.bin nq qoff.bin qsegs tkeys.bin nt toff.bin tsegs pairs.bin P outoff.bin, then per run: wx wy wz want.bin
static int distances_main(int argc, char** a) {
    const int X = atoi(a[0]), Y = atoi(a[1]), Z = atoi(a[2]);
    const size_t nq = (size_t)atoll(a[4]), nt = (size_t)atoll(a[8]);
    const int qsegs = atoi(a[6]), tsegs = atoi(a[10]), P = atoi(a[12]);
    int64_t* qk = slurp<int64_t>(a[3], nq);
    int64_t* qo = slurp<int64_t>(a[5], (size_t)qsegs + 1);
    int64_t* tk = slurp<int64_t>(a[7], nt);
    int64_t* to = slurp<int64_t>(a[9], (size_t)tsegs + 1);
    int32_t* pr = slurp<int32_t>(a[11], (size_t)P * 2);
    int64_t* oo = slurp<int64_t>(a[13], (size_t)P + 1);
    const size_t total = (size_t)oo[P];
    double* d2 = (double*)malloc(total * 8 + (total == 0));
    size_t bad = 0, runs = 0;
    for (int i = 14; i + 3 < argc; i += 4, ++runs) {
        const double wx = strtod(a[i], nullptr), wy = strtod(a[i + 1], nullptr), wz = strtod(a[i + 2], nullptr);
        double* want = slurp<double>(a[i + 3], total);
        memset(d2, 0xCD, total * 8);
        if (sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr) != SK_OK)
            return 5;
        bad += memcmp(d2, want, total * 8) != 0;
        free(want);
        if (runs || P == 0 || total == 0) continue;
        // the argument checks: nothing is launched or written
        memset(d2, 0xAB, total * 8);
        int64_t* down = (int64_t*)malloc(((size_t)qsegs + 1) * 8);           // not monotone
        memcpy(down, qo, ((size_t)qsegs + 1) * 8);
        down[qsegs] = down[0] - 1;
        int64_t* shifted = (int64_t*)malloc(((size_t)P + 1) * 8);           // does not start at 0
        for (int k = 0; k <= P; ++k) shifted[k] = oo[k] + 1;
        int32_t* wild = (int32_t*)malloc((size_t)P * 8);                     // a segment that does not exist
        memcpy(wild, pr, (size_t)P * 8);
        wild[1] = tsegs;
        const double inf = INFINITY, nan = NAN;
        int rc[] = {
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, -1, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, (1 << 26) + 1, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, -1, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, -1, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, 0.0, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, -1.0, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, inf, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, nan, wy, wz, d2, nullptr),
            sk_surface_distances(nullptr, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, nullptr, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, nullptr, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, nullptr, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, nullptr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, nullptr, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, nullptr, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, (double*)((char*)d2 + 4),
                                 nullptr),
            sk_surface_distances(qk, down, qsegs, tk, to, tsegs, pr, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, P, shifted, X, Y, Z, wx, wy, wz, d2, nullptr),
            sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, wild, P, oo, X, Y, Z, wx, wy, wz, d2, nullptr)};
        for (int v : rc)
            if (v != SK_ERR_ARG) return 7;
        if (!all_bytes(d2, total * 8, 0xAB)) return 8;
        if (sk_surface_distances(qk, qo, qsegs, tk, to, tsegs, pr, 0, oo, X, Y, Z, wx, wy, wz, d2, nullptr) != SK_OK ||
            sk_surface_distances(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, wx, wy, wz, nullptr,
                                 nullptr) != SK_OK ||
            !all_bytes(d2, total * 8, 0xAB))
            return 9;
        free(down); free(shifted); free(wild);
    }
    printf("%d pairs, %zu distances, %zu runs, %zu mismatches", P, total, runs, bad);
    free(qk); free(qo); free(tk); free(to); free(pr); free(oo); free(d2);
    return bad ? 1 : 0;
}
int main(int argc, char** argv) {
    shim_init();
    if (argc == 12 && !strcmp(argv[1], "surface")) return surface_main(argv + 2);
    if (argc >= 16 && !strcmp(argv[1], "distances")) return distances_main(argc - 2, argv + 2);
    return 2;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "surface_distance.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(surface_\w+_kernel<\w+>)<<<grid, kThreads, 0, st>>>\(", r"LAUNCH(\1, grid, kThreads, ", text)
    if n != 6:
        raise SystemExit(f"surface_distance.hip: expected 6 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "surface_distance_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "surface_distance_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(workdir, "surface_distance_host.cpp")])
    return exe


def finish(label, r):
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def run_surface(exe, workdir, label, lab, counts, keys):
    from tools.edt_host_check import kernel_inputs
    a, lut, max_id = kernel_inputs(lab)
    paths = [os.path.join(workdir, n) for n in ("lab.bin", "lut.bin", "counts.bin", "keys.bin")]
    for p, arr in zip(paths, (a, lut, counts, keys)):
        np.ascontiguousarray(arr).tofile(p)
    finish(label, subprocess.run([exe, "surface", paths[0]] + [str(s) for s in lab.shape] +
                                 [paths[1], str(max_id), str(counts.size), paths[2], paths[3], str(keys.size)],
                                 capture_output=True, text=True))


def run_distances(exe, workdir, label, shape, q_off, q_keys, t_off, t_keys, pairs, spacings):
    from tests.surface_distance_cases import pair_d2, weights
    names = ("qk.bin", "qo.bin", "tk.bin", "to.bin", "pairs.bin", "oo.bin")
    paths = [os.path.join(workdir, n) for n in names]
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out_off = pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, weights(spacings[0]))[0]
    for p, arr in zip(paths, (q_keys, q_off, t_keys, t_off, pairs, out_off)):
        np.ascontiguousarray(arr, dtype=arr.dtype).tofile(p)
    args = [exe, "distances"] + [str(s) for s in shape] + \
        [paths[0], str(q_keys.size), paths[1], str(q_off.size - 1), paths[2], str(t_keys.size), paths[3],
         str(t_off.size - 1), paths[4], str(len(pairs)), paths[5]]
    for k, spacing in enumerate(spacings):
        w = weights(spacing)
        want = os.path.join(workdir, f"want{k}.bin")
        pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, w)[1].tofile(want)
        args += [float(v).hex() for v in w] + [want]
    finish(label, subprocess.run(args, capture_output=True, text=True))


def main():
    from tests import surface_distance_cases as S
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for name, (gt, pred) in S.cases().items():
            _, _, counts_g, keys_g, _, _, counts_p, keys_p = S.surfaces_of(name)
            run_surface(exe, workdir, f"{name}, ground truth", gt, counts_g, keys_g)
            run_surface(exe, workdir, f"{name}, prediction", pred, counts_p, keys_p)
            off_g = np.concatenate(([0], np.cumsum(counts_g))).astype(np.int64)
            off_p = np.concatenate(([0], np.cumsum(counts_p))).astype(np.int64)
            pairs = S.expected(name)["pairs"]
            run_distances(exe, workdir, f"{name}, ground truth -> prediction", gt.shape, off_g, keys_g, off_p, keys_p,
                          pairs, S.SPACINGS)
            run_distances(exe, workdir, f"{name}, prediction -> ground truth", gt.shape, off_p, keys_p, off_g, keys_g,
                          pairs[:, ::-1], S.SPACINGS)
            runs += 4
        tile = 1024                                          # sk_surface_distance_tile(); the program checks nothing of it
        shape, q_off, q_keys, t_off, t_keys, pairs = S.synthetic(tile)
        run_distances(exe, workdir, "synthetic key lists", shape, q_off, q_keys, t_off, t_keys, pairs,
                      (S.SPACINGS[0], S.SPACINGS[3]))
        wide = S.synthetic_wide()
        run_distances(exe, workdir, "synthetic key lists, X Y Z = 2^54 (64-bit decode)", *wide,
                      (S.SPACINGS[0], S.SPACINGS[3]))
        run_distances(exe, workdir, "no pairs", shape, q_off, q_keys, t_off, t_keys, pairs[:0], S.SPACINGS[:1])
        runs += 3
    print(f"{runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
