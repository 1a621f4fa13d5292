#!/usr/bin/env python
"""Time the skeleton graph of every instance (``sk_skeletonize`` + ``sk_skeleton_graph``) on a
synthetic 512 x 512 x 128 int32 mask of 1 000 ellipsoidal blobs (the generator of tools/bench_instance_stats.py):

  * the thinning launches and the graph launches separately, batch by batch as ``instance_skeleton_graph`` forms them
    (device events around each library call; the workspace is allocated before): min / median / max of the repeats,
    summed over the batches.  The thinning call includes its table upload and its stream synchronisation;
  * the graph kernel against the bytes of image plane it reads -- one bit per voxel of every padded crop, nothing
    else of any size -- over the 8.0 TB/s HBM peak of the MI355X.  With one workgroup per object and a few KiB per
    object the launch, not the memory, is the scale; the figure says how far from a bandwidth question this kernel is;
  * ``instance_skeleton_graph`` end to end (prologue given), and ``--sustained`` graph calls back to back on the last
    batch inside one pair of events, divided by that number.

It asserts no threshold.

    python tools/bench_skeleton_graph.py --out profiles/skeleton_graph_bench.json
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

from tools.bench_instance_stats import HBM_PEAK, build_mask, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sustained", type=int, default=50, help="graph calls back to back in one timed window")
    ap.add_argument("--budget", type=int, default=None, help="bytes of thinning workspace per batch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_graph needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.lib import morphology
    from skoots_amd.validate import lib as VL

    shape = tuple(args.shape)
    x = build_mask(shape, args.blobs, device)
    budget = VL.SKELETON_BUDGET if args.budget is None else args.budget
    rows = VL.id_rows(x)
    ids, _, boxes = VL.instance_sums(x, rows)
    first = VL.instance_skeleton_graph(x, rows, boxes, budget)[1]                    # warm-up, and to compare
    a, _, lut, _ = rows[1]
    values = torch.nonzero(lut)[:, 0].to(torch.int32).cpu().numpy()
    b = boxes.cpu().numpy().astype(np.int64)
    b[:, 3:] += 1
    ext = b[:, 3:] - b[:, :3]
    plane_bytes = int(((ext[:, 0] + 2) * (ext[:, 1] + 2) * ((ext[:, 2] + 2 + 31) >> 5)).sum()) * 4
    b = np.ascontiguousarray(b.astype(np.int32))
    batches = VL._skeleton_batches(b, budget)
    N = int(ids.numel())
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs, "instances": N,
              "foreground_share": float((x > 0).sum().item() / x.numel()), "batches": len(batches),
              "budget_bytes": budget, "image_plane_bytes": plane_bytes, "skeleton_voxels": int(first[:, 0].sum().item()),
              "links": int(first[:, 5:].sum().item()), "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats}

    def graph_call(thinned, out):
        _, boxes_p, n, work, nbytes, _ = thinned
        _ffi.check(_ffi.lib.sk_skeleton_graph(boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(out),
                                              _ffi.stream_ptr(device)))

    thin_s, graph_s, whole_s = [], [], []
    graph = torch.empty((N, morphology.N_GRAPH), dtype=torch.int64, device=device)
    thinned = None
    for _ in range(args.repeats):
        t_thin = t_graph = 0.0
        for lo, hi in batches:
            (thinned, _), s = timed(lambda: morphology._thin(a, values[lo:hi], b[lo:hi]), device)
            t_thin += s                                              # with the workspace allocation: cached after warm-up
            _, s = timed(lambda: graph_call(thinned, graph[lo:hi]), device)
            t_graph += s
        thin_s.append(t_thin)
        graph_s.append(t_graph)
        _, s = timed(lambda: VL.instance_skeleton_graph(x, rows, boxes, budget), device)
        whole_s.append(s)
    report["thinning"] = summary(thin_s)
    report["graph"] = summary(graph_s)
    report["graph"]["equals_first_run"] = bool(torch.equal(graph, first))
    report["graph"]["bytes_per_s_at_median"] = plane_bytes / report["graph"]["median_s"]
    report["graph"]["share_of_hbm_peak_at_median"] = plane_bytes / report["graph"]["median_s"] / HBM_PEAK
    report["graph_over_thinning_at_median"] = report["graph"]["median_s"] / report["thinning"]["median_s"]
    report["instance_skeleton_graph"] = summary(whole_s)
    lo, hi = batches[-1]
    _, s = timed(lambda: [graph_call(thinned, graph[lo:hi]) for _ in range(args.sustained)], device)
    report["sustained_graph_last_batch"] = {"calls": args.sustained, "objects": hi - lo, "per_call_s": s / args.sustained}

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
