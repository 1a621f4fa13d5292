#!/usr/bin/env python
"""Run skoots_amd/csrc/instance_mesh_emit.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

As tools/instance_mesh_host_check.py does for section 21's kernel, and with its shim: the kernels' text is compiled as
host C++ into a stand-alone program.  A workgroup is 256 host threads, ``__syncthreads`` is a barrier over them, the LDS
arrays are static arrays and the atomics are the compiler's; workgroups run one after another.  Mask, look-up table,
triangle table, counts and both record arrays are heap blocks of exactly the arrays' sizes, so an access past either
end of any of them, or of an LDS array, is a sanitizer report.

Every case of tests/mesh_cases.py runs in both modes: the count pass must equal the numpy oracle, the emit pass at the
exact capacities must give exactly the oracle's records (sorted on both sides), and the emit pass at HALF the
capacities -- into blocks of half the size -- and at capacities of zero with NULL record arrays must report the full
counts.  Two more runs hand the kernels a triangle table of garbage and a look-up table that names rows outside 1..N:
neither may touch anything outside the outputs.

    python tools/instance_mesh_emit_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the positions on the high faces and the -1 layer, both accumulation paths and the slot
arithmetic as written; what only a device has (real LDS atomics, the hardware's wave scheduling) it cannot see.
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

from tools.instance_mesh_host_check import SHIM  # noqa: E402

MAIN = r"""
#include <algorithm>
#include <array>
template <class T> static T* slurp(const char* path, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    FILE* f = fopen(path, "rb");
    if (!f || fread(p, sizeof(T), n, f) != n) exit(3);
    fclose(f);
    return p;
}
template <size_t W> static size_t differ(int64_t* got, const int64_t* want, size_t n, size_t key) {
    typedef std::array<int64_t, W> R;
    R* g = (R*)got;
    std::sort(g, g + n, [key](const R& a, const R& b) { return a[0] != b[0] ? a[0] < b[0] : a[key] < b[key]; });
    size_t bad = 0;
    for (size_t i = 0; i < n * W; ++i) bad += got[i] != want[i];
    return bad;
}
// lab.bin X Y Z lut.bin max_id N table.bin closed counts.bin vrec.bin V trec.bin F compare
int main(int argc, char** argv) {
    if (argc != 16) return 2;
    shim_init();
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), max_id = atoi(argv[6]), N = atoi(argv[7]);
    const int closed = atoi(argv[9]), compare = atoi(argv[15]);
    const size_t V = (size_t)atoll(argv[12]), F = (size_t)atoll(argv[14]);
    int32_t* lab = slurp<int32_t>(argv[1], (size_t)X * Y * Z);
    int32_t* lut = slurp<int32_t>(argv[5], (size_t)max_id + 1);
    uint64_t* table = slurp<uint64_t>(argv[8], 256);
    int64_t* want_counts = slurp<int64_t>(argv[10], (size_t)N * 2);
    int64_t* want_v = slurp<int64_t>(argv[11], V * 2);
    int64_t* want_t = slurp<int64_t>(argv[13], F * 5);
    int64_t* counts = (int64_t*)malloc((size_t)N * 16 + (N == 0));
    memset(counts, 0xAB, (size_t)N * 16);
    if (sk_instance_mesh_count(lab, X, Y, Z, lut, max_id, N, table, closed, counts, nullptr) != SK_OK) return 5;
    size_t bad = 0, total_v = 0, total_t = 0;
    for (size_t i = 0; i < (size_t)N; ++i) total_v += (size_t)counts[2 * i], total_t += (size_t)counts[2 * i + 1];
    if (compare) {
        for (size_t i = 0; i < (size_t)N * 2; ++i) bad += counts[i] != want_counts[i];
        bad += total_v != V || total_t != F;
    }
    // the capacities the count pass gives, then half of them, then none: blocks of exactly those sizes
    for (int round = 0; round < 3; ++round) {
        const size_t cv = round == 0 ? total_v : round == 1 ? total_v / 2 : 0;
        const size_t ct = round == 0 ? total_t : round == 1 ? total_t / 2 : 0;
        int64_t* vrec = round == 2 ? nullptr : (int64_t*)malloc(cv * 16 + (cv == 0));
        int64_t* trec = round == 2 ? nullptr : (int64_t*)malloc(ct * 40 + (ct == 0));
        int64_t* produced = (int64_t*)malloc(16);
        produced[0] = produced[1] = -1;
        if (sk_instance_mesh_emit(lab, X, Y, Z, lut, max_id, N, table, closed, vrec, (int64_t)cv, trec, (int64_t)ct,
                                  produced, nullptr) != SK_OK)
            return 6;
        bad += (size_t)produced[0] != total_v || (size_t)produced[1] != total_t;
        if (round == 0 && compare) bad += differ<2>(vrec, want_v, V, 1) + differ<5>(trec, want_t, F, 4);
        free(vrec); free(trec); free(produced);
    }
    printf("%d rows, %zu vertices, %zu triangles, %zu mismatches", N, total_v, total_t, bad);
    free(lab); free(lut); free(table); free(want_counts); free(want_v); free(want_t); free(counts);
    return bad ? 1 : 0;
}
"""


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_mesh_emit.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "instance_rows.h")) as f:   # the shared header, in place
        text = text.replace('#include "instance_rows.h"', f.read().replace("#pragma once", ""))
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(instance_mesh\w*_kernel)<<<([^;]*?), kThreads, 0, st>>>\(", r"LAUNCH(\1, \2, kThreads, ", text,
                      flags=re.S)
    if n != 2:
        raise SystemExit(f"instance_mesh_emit.hip: expected 2 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "instance_mesh_emit_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "instance_mesh_emit_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "instance_mesh_emit_host.cpp")])
    return exe


def run(exe, workdir, lab, label, closed, table, oracle, lut=None, compare=True):
    ids, counts, vrec, trec = oracle
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    max_id = int(ids.max()) if len(ids) else 0
    if lut is None:
        lut = np.zeros(max_id + 1, np.int32)
        lut[ids] = np.arange(1, len(ids) + 1)
    names = ("lab.bin", "lut.bin", "table.bin", "counts.bin", "vrec.bin", "trec.bin")
    paths = [os.path.join(workdir, n) for n in names]
    for p, a in zip(paths, (lab, lut, table, counts, vrec, trec)):
        np.ascontiguousarray(a).tofile(p)
    r = subprocess.run([exe, paths[0]] + [str(s) for s in lab.shape] +
                       [paths[1], str(max_id), str(len(ids)), paths[2], str(int(closed)), paths[3], paths[4],
                        str(len(vrec)), paths[5], str(len(trec)), str(int(compare))], capture_output=True, text=True)
    print(f"{label}, {'closed' if closed else 'open'}: {r.stdout.strip()} (exit {r.returncode})")
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    from skoots_amd.validate.lib import packed_triangle_table
    from tests.mesh_cases import cases, record_oracle
    table = packed_triangle_table()
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for label, lab in cases().items():
            for closed in (False, True):
                run(exe, workdir, lab, label, closed, table, record_oracle(lab, closed))
                runs += 1
        label = "blobs (9, 35, 70)"
        lab = cases()[label]
        oracle = record_oracle(lab, True)
        garbage = np.full(256, 2 ** 64 - 1, np.uint64)         # 15 triangles of edge 15 in every configuration
        run(exe, workdir, lab, label + ", a table of garbage", True, garbage, oracle, compare=False)
        ids = oracle[0]
        lut = np.zeros(int(ids.max()) + 1, np.int32)
        lut[ids] = np.arange(1, len(ids) + 1)
        lut[ids[::3]] += len(ids)                              # rows beyond N
        lut[ids[1::3]] = -7
        run(exe, workdir, lab, label + ", rows outside 1..N", True, table, oracle, lut=lut, compare=False)
        runs += 2
    print(f"{runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
