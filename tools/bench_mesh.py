#!/usr/bin/env python
"""Time the per-instance meshes (``sk_instance_mesh_count``, ``sk_instance_mesh_emit``) on the
synthetic 1024 x 1024 x 256 int32 mask of tools/bench_instance_stats.py, closed mode, in one process and alternating
within every window:

  * the count pass alone and the emit pass alone (device events around the library call; ids, look-up table and
    buffers prepared before);
  * the whole ``instance_meshes`` call with the prologue given (count, emit, the sorts and the look-up that turns
    edge keys into local indices);
  * ``sk_instance_mesh_cells`` (section 21) on the same mask: the yardstick, a kernel with the same staging that
    writes almost nothing.

The bytes the algorithm needs are 4 per voxel read once plus the records written (16 per vertex, 40 per triangle; none
for the count pass); the achieved rate is those bytes over the median time, stated against the 8.0 TB/s HBM peak of
the MI355X.  One warm-up of every piece, then ``--repeats`` windows; nothing is asserted about time.

    python tools/bench_mesh.py --out profiles/mesh_bench.json
"""
import argparse
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
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--blobs", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.mc_table import CLASS_OF, CLASS_TRIANGLES

    shape = tuple(args.shape)
    X, Y, Z = shape
    x = build_mask(shape, args.blobs, device)
    rows = VL.id_rows(x)
    a, ids, lut, max_id = rows[1]
    N = int(ids.numel())
    st = _ffi.stream_ptr(device)
    first = VL.instance_meshes(x, True, rows)                       # warm-up of every piece, and the result to compare
    V, F = int(first["vertices"].shape[0]), int(first["faces"].shape[0])
    mask_bytes = x.numel() * 4
    record_bytes = 16 * V + 40 * F
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs, "instances": N,
              "closed": True, "vertices": V, "triangles": F, "mask_bytes": mask_bytes, "record_bytes": record_bytes,
              "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats}

    table = torch.from_numpy(VL.packed_triangle_table().view(np.int64)).to(device)
    class_of = torch.tensor(CLASS_OF, dtype=torch.uint8, device=device)
    n_classes = len(CLASS_TRIANGLES)
    counts = torch.empty((N, 2), dtype=torch.int64, device=device)
    cells = torch.empty((N, n_classes), dtype=torch.int64, device=device)
    vrec = torch.empty((V, 2), dtype=torch.int64, device=device)
    trec = torch.empty((F, 5), dtype=torch.int64, device=device)
    produced = torch.empty(2, dtype=torch.int64, device=device)

    def count():
        _ffi.check(_ffi.lib.sk_instance_mesh_count(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(table), 1,
                                                   _ffi.ptr(counts), st))

    def emit():
        _ffi.check(_ffi.lib.sk_instance_mesh_emit(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(table), 1,
                                                  _ffi.ptr(vrec), V, _ffi.ptr(trec), F, _ffi.ptr(produced), st))

    def yardstick():
        _ffi.check(_ffi.lib.sk_instance_mesh_cells(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(class_of),
                                                   n_classes, 1, _ffi.ptr(cells), st))

    for fn in (count, emit, yardstick):
        fn()
    torch.cuda.synchronize(device)
    times = {"count": [], "emit": [], "instance_meshes": [], "mesh_cells_yardstick": []}
    same = True
    for _ in range(args.repeats):
        times["count"].append(timed(count, device)[1])
        times["emit"].append(timed(emit, device)[1])
        again, s = timed(lambda: VL.instance_meshes(x, True, rows), device)
        times["instance_meshes"].append(s)
        same &= all(torch.equal(again[k], first[k]) for k in first)
        del again
        times["mesh_cells_yardstick"].append(timed(yardstick, device)[1])
    report["every_run_equals_the_first"] = bool(same and produced.tolist() == [V, F] and
                                                torch.equal(counts[:, 0], first["vertex_offsets"].diff()) and
                                                torch.equal(counts[:, 1], first["face_offsets"].diff()))
    needed = {"count": mask_bytes, "emit": mask_bytes + record_bytes, "instance_meshes": 2 * mask_bytes + record_bytes,
              "mesh_cells_yardstick": mask_bytes}
    for k, t in times.items():
        report[k] = summary(t)
        report[k]["needed_bytes"] = needed[k]
        report[k]["bytes_per_s_at_median"] = needed[k] / report[k]["median_s"]
        report[k]["share_of_hbm_peak_at_median"] = needed[k] / report[k]["median_s"] / HBM_PEAK

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
