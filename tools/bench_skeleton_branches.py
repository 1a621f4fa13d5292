#!/usr/bin/env python
"""Time the branch tracing of every instance (``sk_skeleton_branches_count`` + ``sk_skeleton_branches_emit``, DESIGN.md
section 32) on the synthetic mask of tools/bench_skeleton_graph.py: 512 x 512 x 128 int32, 1 000 ellipsoidal blobs.

Batch by batch as ``instance_skeleton_branches`` forms them, device events around each library call, buffers allocated
before: the thinning, the graph kernel, the point emit, the count pass and the emit pass separately, min / median / max
of the repeats summed over the batches.  The figure of interest is count + emit next to the thinning time of the same
run; ``sk_skeleton_pack`` of the thinned skeletons is timed too, since it is what ``skeleton=`` / ``--skeleton-from``
pay instead of the thinning.  ``instance_skeleton_branches`` end to end (prologue given) closes the report.

It asserts no threshold.

    python tools/bench_skeleton_branches.py --out profiles/skeleton_branches_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_instance_stats import build_mask, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget", type=int, default=None, help="bytes of thinning workspace per batch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_branches needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.lib import morphology
    from skoots_amd.validate import lib as VL

    shape = tuple(args.shape)
    x = build_mask(shape, args.blobs, device)
    budget = VL.SKELETON_BUDGET if args.budget is None else args.budget
    rows = VL.id_rows(x)
    m = VL._Rows(None, rows)
    ids, _, boxes = VL.instance_sums(x, rows)
    first = VL.instance_skeleton_branches(x, rows, boxes, budget)                    # warm-up, and to compare
    b, values = VL._thinning_boxes(m, boxes)
    batches = VL._skeleton_batches(b, budget)
    N = int(ids.numel())
    nodes, branches = first[2], first[3]
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs, "instances": N,
              "batches": len(batches), "budget_bytes": budget, "skeleton_voxels": int(first[1][:, 0].sum().item()),
              "nodes": int(nodes.shape[0]), "junction_nodes": int((nodes[:, 1] == 2).sum().item()),
              "junction_voxels": int(first[1][:, 4].sum().item()), "branches": int(branches.shape[0]),
              "longest_branch_chain_voxels": int(branches[:, 3].max().item()) if branches.shape[0] else 0,
              "repeats": args.repeats}
    stream = _ffi.stream_ptr(device)
    times = {k: [] for k in ("thinning", "graph", "points", "count", "emit", "pack")}
    whole_s = []
    # the skeletons as a label volume in the values of `m.a`, for the pack timing
    row = torch.repeat_interleave(torch.arange(N, device=device), first[1][:, 0])
    saved = torch.zeros(shape, dtype=torch.int32, device=device)
    p = first[4].long()
    saved[p[:, 0], p[:, 1], p[:, 2]] = torch.from_numpy(values).to(device)[row]
    same = True
    for _ in range(args.repeats):
        t = {k: 0.0 for k in times}
        n_nodes = n_branches = 0
        for lo, hi in batches:
            (thinned, _), s = timed(lambda: morphology._thin(m.a, values[lo:hi], b[lo:hi]), device)
            t["thinning"] += s
            _, boxes_p, n, work, nbytes, counts = thinned
            graph = torch.empty((n, morphology.N_GRAPH), dtype=torch.int64, device=device)
            _, s = timed(lambda: _ffi.check(_ffi.lib.sk_skeleton_graph(boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes),
                                                                       _ffi.ptr(graph), stream)), device)
            t["graph"] += s
            (points, offsets), s = timed(lambda: morphology._emit(thinned, want_offsets=True), device)
            t["points"] += s
            total = int(points.shape[0])
            counts_host = np.ascontiguousarray(counts.cpu().numpy().astype(np.int32))
            sbytes = int(_ffi.lib.sk_skeleton_branches_scratch_bytes(boxes_p, counts_host.ctypes.data_as(_ffi.ip), n))
            scratch = torch.empty(sbytes, dtype=torch.uint8, device=device)
            per = torch.empty((n, 2), dtype=torch.int32, device=device)
            common = (boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(offsets), total, _ffi.ptr(scratch),
                      C.c_size_t(sbytes))
            _, s = timed(lambda: _ffi.check(_ffi.lib.sk_skeleton_branches_count(*common, _ffi.ptr(per), stream)), device)
            t["count"] += s
            noff = morphology._offsets(per[:, 0]).to(torch.int32)
            boff = morphology._offsets(per[:, 1]).to(torch.int32)
            nn, nb = int(noff[-1].item()), int(boff[-1].item())
            out_nodes = torch.empty((nn, morphology.N_NODE), dtype=torch.int32, device=device)
            out_branches = torch.empty((nb, morphology.N_BRANCH), dtype=torch.int32, device=device)
            owner = torch.empty(total, dtype=torch.int32, device=device)
            _, s = timed(lambda: _ffi.check(_ffi.lib.sk_skeleton_branches_emit(
                *common, _ffi.ptr(noff), _ffi.ptr(boff), nn, nb, _ffi.ptr(out_nodes), _ffi.ptr(out_branches),
                _ffi.ptr(owner), stream)), device)
            t["emit"] += s
            same = same and torch.equal(out_nodes[:, 1:], nodes[n_nodes:n_nodes + nn, 1:])
            same = same and torch.equal(out_branches[:, 3:], branches[n_branches:n_branches + nb, 3:])
            n_nodes, n_branches = n_nodes + nn, n_branches + nb
            _, s = timed(lambda: morphology._thin(saved, values[lo:hi], b[lo:hi], thin=False), device)
            t["pack"] += s
        for k in times:
            times[k].append(t[k])
        _, s = timed(lambda: VL.instance_skeleton_branches(x, rows, boxes, budget), device)
        whole_s.append(s)
    for k in times:
        report[k] = summary(times[k])
    report["tables_equal_first_run"] = bool(same)
    trace = report["count"]["median_s"] + report["emit"]["median_s"]
    report["count_plus_emit_median_s"] = trace
    report["count_plus_emit_over_thinning_at_median"] = trace / report["thinning"]["median_s"]
    report["instance_skeleton_branches"] = summary(whole_s)

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
