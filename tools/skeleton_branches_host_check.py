#!/usr/bin/env python
"""Run the branch tracing of skoots_amd/csrc/skeletonize.hip on the CPU under AddressSanitizer + UBSan before it runs on
a device: ``sk_skeleton_pack`` (or the thinning), ``sk_skeleton_graph``, ``sk_skeletonize_emit``,
``sk_skeleton_branches_count`` and ``sk_skeleton_branches_emit``, in the order ``lib.morphology.skeleton_branches``
calls them.

The shim and the build are those of tools/skeleton_graph_host_check.py: the file's text compiled as host C++ into a
stand-alone program with its own ``main``, a workgroup as 256 host threads, workgroups one after another.  Labels,
workspace, scratch, tables and owner are heap blocks of exactly the sizes the library asks for (the workspace and the
scratch filled with 0xCD first: the kernels must write what they read), so an access past either end of any of them is
a sanitizer report.  Every hand-built case of tests/skeleton_branch_cases.py is packed without thinning, every case of
tests/skeleton_graph_cases.py is thinned, and ``tests.test_skeletonize.large_object()`` is thinned in the whole volume,
which does not fit the LDS path; the tables, the owner, the points and the graph rows are compared, exactly, with the
oracles of tests/test_skeleton_branches_cpu.py and tests/test_skeleton_graph_cpu.py.  The argument checks are called
with every kind of bad argument: nothing may be launched.

    python tools/skeleton_branches_host_check.py     # builds into a temporary directory, prints one line per case

It checks the indexing, the scans and the walks as written; what only a device has it cannot see.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.skeleton_graph_host_check import build  # noqa: E402

MAIN = r"""
template <class T> static T* slurp(const char* path, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    FILE* f = fopen(path, "rb");
    if (!f || fread(p, sizeof(T), n, f) != n) exit(3);
    fclose(f);
    return p;
}
#define WANT_ARG(call) do { if ((call) != SK_ERR_ARG) { printf("no SK_ERR_ARG: %s\n", #call); return 8; } } while (0)
int main(int argc, char** argv) {   // dir X Y Z n thin n_points n_nodes n_branches
    if (argc != 10) return 2;
    shim_init();
    const std::string dir = argv[1];
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), n = atoi(argv[5]), thin = atoi(argv[6]);
    const long long n_points = atoll(argv[7]), n_nodes = atoll(argv[8]), n_branches = atoll(argv[9]);
    int32_t* lab = slurp<int32_t>((dir + "/lab.bin").c_str(), (size_t)X * Y * Z);
    int32_t* ids = slurp<int32_t>((dir + "/ids.bin").c_str(), n);
    int32_t* boxes = slurp<int32_t>((dir + "/boxes.bin").c_str(), 6 * (size_t)n);
    int64_t* want_graph = slurp<int64_t>((dir + "/graph.bin").c_str(), 12 * (size_t)n);
    int32_t* want_points = slurp<int32_t>((dir + "/points.bin").c_str(), 3 * (size_t)n_points);
    int32_t* want_nodes = slurp<int32_t>((dir + "/nodes.bin").c_str(), 8 * (size_t)n_nodes);
    int32_t* want_branches = slurp<int32_t>((dir + "/branches.bin").c_str(), 18 * (size_t)n_branches);
    int32_t* want_owner = slurp<int32_t>((dir + "/owner.bin").c_str(), (size_t)n_points);
    const size_t bytes = sk_skeletonize_workspace_bytes(boxes, n);
    void* work = nullptr;
    if (!bytes || posix_memalign(&work, 16, bytes)) return 4;
    memset(work, 0xCD, bytes);
    int32_t* counts = (int32_t*)malloc(4 * (size_t)n);
    int32_t* stats = (int32_t*)malloc(8 * (size_t)n);
    int32_t error = -1;
    if ((thin ? sk_skeletonize : sk_skeleton_pack)(lab, X, Y, Z, ids, boxes, n, work, bytes, counts, stats, &error,
                                                   nullptr) != SK_OK || error)
        return 5;
    WANT_ARG(sk_skeleton_pack(nullptr, X, Y, Z, ids, boxes, n, work, bytes, counts, stats, &error, nullptr));
    WANT_ARG(sk_skeleton_pack(lab, X, Y, Z, ids, boxes, n, work, bytes - 1, counts, stats, &error, nullptr));
    WANT_ARG(sk_skeleton_pack(lab, X, Y, Z, ids, boxes, n, (char*)work + 4, bytes, counts, stats, &error, nullptr));
    WANT_ARG(sk_skeleton_pack(lab, X, Y, Z, ids, boxes, 0, work, bytes, counts, stats, &error, nullptr));
    WANT_ARG(sk_skeleton_pack(lab, X, Y, Z, ids, boxes, n, work, bytes, nullptr, stats, &error, nullptr));
    int64_t* graph = (int64_t*)malloc(96 * (size_t)n);
    if (sk_skeleton_graph(boxes, n, work, bytes, graph, nullptr) != SK_OK) return 7;
    size_t bad_graph = 0, bad_points = 0, bad_counts = 0, bad_nodes = 0, bad_branches = 0, bad_owner = 0;
    for (size_t i = 0; i < 12 * (size_t)n; ++i) bad_graph += graph[i] != want_graph[i];
    int32_t* offsets = (int32_t*)malloc(4 * ((size_t)n + 1));
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + counts[i];
    if (offsets[n] != n_points) { printf("%d points, %lld wanted\n", offsets[n], n_points); return 9; }
    int32_t* points = (int32_t*)malloc(12 * (size_t)n_points + (n_points == 0));
    if (sk_skeletonize_emit(boxes, n, work, bytes, offsets, n_points, points, nullptr) != SK_OK) return 10;
    for (size_t i = 0; i < 3 * (size_t)n_points; ++i) bad_points += points[i] != want_points[i];
    if (sk_skeleton_nodes_row_values() != 8 || sk_skeleton_branches_row_values() != 18) return 6;
    const size_t sbytes = sk_skeleton_branches_scratch_bytes(boxes, counts, n);
    if (sbytes != 16 + 44 * (size_t)n_points) return 11;
    void* scratch = malloc(sbytes);
    memset(scratch, 0xCD, sbytes);
    int32_t* nb = (int32_t*)malloc(8 * (size_t)n);
    if (sk_skeleton_branches_count(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, nb, nullptr) != SK_OK)
        return 12;
    int32_t* noff = (int32_t*)malloc(4 * ((size_t)n + 1));
    int32_t* boff = (int32_t*)malloc(4 * ((size_t)n + 1));
    noff[0] = boff[0] = 0;
    for (int i = 0; i < n; ++i) {
        bad_counts += nb[2 * i] < 0 || nb[2 * i + 1] < 0;
        noff[i + 1] = noff[i] + nb[2 * i];
        boff[i + 1] = boff[i] + nb[2 * i + 1];
    }
    if (bad_counts || noff[n] != n_nodes || boff[n] != n_branches) {
        printf("%d nodes, %d branches, %zu refused objects: %lld and %lld wanted\n", noff[n], boff[n], bad_counts,
               n_nodes, n_branches);
        return 13;
    }
    int32_t* nodes = (int32_t*)malloc(32 * (size_t)n_nodes + (n_nodes == 0));
    int32_t* branches = (int32_t*)malloc(72 * (size_t)n_branches + (n_branches == 0));
    int32_t* owner = (int32_t*)malloc(4 * (size_t)n_points + (n_points == 0));
    memset(scratch, 0xCD, sbytes);   // the passes hand each other nothing
    if (sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, n_nodes,
                                  n_branches, nodes, branches, owner, nullptr) != SK_OK)
        return 14;
    for (size_t i = 0; i < 8 * (size_t)n_nodes; ++i) bad_nodes += nodes[i] != want_nodes[i];
    for (size_t i = 0; i < 18 * (size_t)n_branches; ++i) bad_branches += branches[i] != want_branches[i];
    for (size_t i = 0; i < (size_t)n_points; ++i) bad_owner += owner[i] != want_owner[i];
    // smaller totals than the truth: the blocks are smaller too, and nothing may be written past them
    if (n_nodes > 0 && n_branches > 0) {
        int32_t* fewer_nodes = (int32_t*)malloc(32 * (size_t)(n_nodes - 1) + 1);
        int32_t* fewer_branches = (int32_t*)malloc(72 * (size_t)(n_branches - 1) + 1);
        if (sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, n_nodes - 1,
                                      n_branches - 1, fewer_nodes, fewer_branches, owner, nullptr) != SK_OK)
            return 15;
        for (size_t i = 0; i < 8 * (size_t)(n_nodes - 1); ++i) bad_nodes += fewer_nodes[i] != want_nodes[i];
        for (size_t i = 0; i < 18 * (size_t)(n_branches - 1); ++i) bad_branches += fewer_branches[i] != want_branches[i];
        free(fewer_nodes); free(fewer_branches);
    }
    // offsets that do not match the planes: the objects are refused, nothing is written outside
    if (n_points > 0) {
        int32_t* wrong = (int32_t*)malloc(4 * ((size_t)n + 1));
        for (int i = 0; i <= n; ++i) wrong[i] = i == 0 ? 0 : offsets[i] - 1 < 0 ? 0 : offsets[i] - 1;
        if (sk_skeleton_branches_count(boxes, n, work, bytes, wrong, n_points, scratch, sbytes, nb, nullptr) != SK_OK)
            return 16;
        size_t refused = 0;
        for (int i = 0; i < n; ++i) refused += nb[2 * i] == -1 && nb[2 * i + 1] == -1;
        if (!refused) { printf("wrong offsets were not refused\n"); return 16; }
        free(wrong);
    }
    // the argument checks: nothing is launched
    WANT_ARG(sk_skeleton_branches_count(nullptr, n, work, bytes, offsets, n_points, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, 0, work, bytes, offsets, n_points, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, nullptr, bytes, offsets, n_points, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes - 1, offsets, n_points, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, nullptr, n_points, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, offsets, -1, scratch, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, offsets, n_points, nullptr, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, offsets, n_points, scratch, sbytes - 1, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, offsets, n_points, (char*)scratch + 2, sbytes, nb, nullptr));
    WANT_ARG(sk_skeleton_branches_count(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, nullptr, nullptr));
    WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, nullptr, boff, n_nodes,
                                       n_branches, nodes, branches, owner, nullptr));
    WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, nullptr, n_nodes,
                                       n_branches, nodes, branches, owner, nullptr));
    WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, -1,
                                       n_branches, nodes, branches, owner, nullptr));
    WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, n_nodes,
                                       1LL << 31, nodes, branches, owner, nullptr));
    WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes - 1, noff, boff, n_nodes,
                                       n_branches, nodes, branches, owner, nullptr));
    if (n_nodes > 0)
        WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, n_nodes,
                                           n_branches, nullptr, branches, owner, nullptr));
    if (n_points > 0)
        WANT_ARG(sk_skeleton_branches_emit(boxes, n, work, bytes, offsets, n_points, scratch, sbytes, noff, boff, n_nodes,
                                           n_branches, nodes, branches, nullptr, nullptr));
    if (sk_skeleton_branches_scratch_bytes(boxes, nullptr, n) != 0 || sk_skeleton_branches_scratch_bytes(nullptr, counts, n) != 0)
        return 17;
    counts[0] = -1;
    if (sk_skeleton_branches_scratch_bytes(boxes, counts, n) != 0) return 17;
    printf("%d objects, %lld points, %lld nodes, %lld branches: %zu graph, %zu point, %zu node, %zu branch, %zu owner "
           "mismatches", n, n_points, n_nodes, n_branches, bad_graph, bad_points, bad_nodes, bad_branches, bad_owner);
    free(lab); free(ids); free(boxes); free(want_graph); free(want_points); free(want_nodes); free(want_branches);
    free(want_owner); free(work); free(counts); free(stats); free(graph); free(offsets); free(points); free(scratch);
    free(nb); free(noff); free(boff); free(nodes); free(branches); free(owner);
    return bad_graph || bad_points || bad_nodes || bad_branches || bad_owner ? 1 : 0;
}
"""


def want_tables(skeleton_rows, n):
    """(graph (n, 12), nodes, branches, owner, points per object) a run must give for the skeleton volume
    ``skeleton_rows`` (0 or the instance's row 1 .. n): the oracles, with the object index of an instance = row - 1"""
    from tests.test_skeleton_branches_cpu import skeleton_branches_oracle
    from tests.test_skeleton_graph_cpu import skeleton_graph_oracle
    rows, nodes, branches, points, owner = skeleton_branches_oracle(skeleton_rows)
    nodes, branches = nodes.copy(), branches.copy()
    if len(rows):
        nodes[:, 0] = rows[nodes[:, 0]] - 1
        branches[:, 0] = rows[branches[:, 0]] - 1
    graph = np.zeros((n, 12), np.int64)
    grows, g = skeleton_graph_oracle(skeleton_rows)
    graph[grows - 1] = g
    return graph, nodes, branches, owner, points


def run(exe, workdir, label, rows, skeleton_rows, thin, whole_volume=False):
    """rows (X, Y, Z) int32: the instances as 1 .. N, each packed or thinned in its own box or in the whole volume;
    skeleton_rows: the skeletons the tracing must see, labelled alike"""
    n = int(rows.max())
    graph, nodes, branches, owner, points = want_tables(skeleton_rows, n)
    boxes, origin = [], []
    for r in range(1, n + 1):
        nz = np.argwhere(rows == r)
        lo, hi = (np.zeros(3, np.int64), np.array(rows.shape)) if whole_volume else (nz.min(0), nz.max(0) + 1)
        boxes.append(np.concatenate((lo, hi)))
        origin.append(np.repeat(lo[None], int((skeleton_rows == r).sum()), 0))
    crop_points = points - np.concatenate(origin) if len(points) else points
    files = {"lab": np.ascontiguousarray(rows, dtype=np.int32), "ids": np.arange(1, n + 1, dtype=np.int32),
             "boxes": np.array(boxes, np.int32), "graph": graph, "points": crop_points.astype(np.int32),
             "nodes": nodes.astype(np.int32), "branches": branches.astype(np.int32), "owner": owner.astype(np.int32)}
    for name, a in files.items():
        np.ascontiguousarray(a).tofile(os.path.join(workdir, name + ".bin"))
    r = subprocess.run([exe, workdir] + [str(s) for s in rows.shape] +
                       [str(n), str(int(thin)), str(len(points)), str(len(nodes)), str(len(branches))],
                       capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})", flush=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def as_rows(lab):
    ids = np.unique(lab)
    ids = ids[ids > 0]
    return ((np.searchsorted(ids, lab.clip(min=0)) + 1) * (lab > 0)).astype(np.int32)


def main():
    from tests.skeleton_branch_cases import cases as branch_cases
    from tests.skeleton_graph_cases import cases as graph_cases
    from tests.test_skeleton_graph_cpu import golden_rows
    from tests.test_skeletonize import golden, large_object
    runs = 0
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir, MAIN.replace("template <class T>", "#include <string>\ntemplate <class T>", 1))
        for label, lab in branch_cases().items():
            rows = as_rows(lab)
            run(exe, workdir, "packed " + label, rows, rows, thin=False)
            runs += 1
        for label, lab in graph_cases().items():
            run(exe, workdir, "thinned " + label, as_rows(lab), golden_rows(label), thin=True)
            runs += 1
        big = large_object().astype(np.int32)
        skel = np.zeros(big.shape, np.int32)
        skel[tuple(golden()["c_points"].astype(np.int64).T)] = 1
        for thin in (True, False):
            run(exe, workdir, f"large object (84, 84, 40), whole volume, thinned: {thin}", big if thin else skel, skel,
                thin=thin, whole_volume=True)
            runs += 1
    print(f"{runs} runs, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
