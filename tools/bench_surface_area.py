#!/usr/bin/env python
"""Time the marching-cubes cell count of every instance (``sk_instance_mesh_cells``) on the
synthetic 1024 x 1024 x 256 int32 mask of 4 000 ellipsoidal blobs of tools/bench_instance_stats.py:

  * the kernel alone in both modes (device events around the library call, ids, look-up table and class table prepared
    before): min / median / max of ten, and the mask's bytes over those times against the 8.0 TB/s HBM peak of the
    MI355X -- the kernel reads the volume once, everything else it moves is negligible;
  * ``sk_instance_stats`` on the same mask in the same process, for scale: both kernels read the same 4 B per voxel, so
    the ratio of the two says what the extra LDS work of the cells costs;
  * each of the three calls ``--sustained`` times back to back inside one pair of events, divided by that number: a
    single call is a window of a few milliseconds, which measures the clock state and the launch as much as the kernel.

It asserts no threshold.

    python tools/bench_surface_area.py --out profiles/surface_area_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_instance_stats import HBM_PEAK, build_mask, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--blobs", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sustained", type=int, default=50, help="calls back to back in one timed window")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_area needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.compare import mesh_area
    from skoots_amd.validate.mc_table import CLASS_OF, CLASS_TRIANGLES

    shape = tuple(args.shape)
    X, Y, Z = shape
    x = build_mask(shape, args.blobs, device)
    nbytes = x.numel() * x.element_size()
    first = {closed: VL.instance_mesh_cells(x, closed)[1] for closed in (False, True)}    # warm-up, and to compare
    VL.instance_sums(x)
    ids, lut, max_id = VL._lut(x)
    N, n_classes = int(ids.numel()), len(CLASS_TRIANGLES)
    class_of = torch.tensor(CLASS_OF, dtype=torch.uint8, device=device)
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs, "instances": N,
              "foreground_share": float((x > 0).sum().item() / x.numel()), "mask_bytes": nbytes,
              "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats,
              "surface_cells_per_voxel_open": float(first[False].sum().item() / x.numel()),
              "total_area_unit_spacing_open": float(mesh_area(first[False]).sum().item()),
              "total_area_unit_spacing_closed": float(mesh_area(first[True]).sum().item())}

    def add(name, times, same=None):
        r = summary(times)
        r["bytes_per_s_at_median"] = nbytes / r["median_s"]
        r["share_of_hbm_peak_at_median"] = nbytes / r["median_s"] / HBM_PEAK
        if same is not None:
            r["equals_first_run"] = same
        report[name] = r

    def mesh(closed, out):
        _ffi.check(_ffi.lib.sk_instance_mesh_cells(
            _ffi.ptr(x), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(class_of), n_classes, int(closed), _ffi.ptr(out),
            _ffi.stream_ptr(device)))

    def stats(sums, boxes):
        _ffi.check(_ffi.lib.sk_instance_stats(
            _ffi.ptr(x), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(sums), _ffi.ptr(boxes), _ffi.stream_ptr(device)))

    times = {"open": [], "closed": [], "stats": []}
    cells = {False: None, True: None}
    for _ in range(args.repeats):                                     # the three kernels alternate
        for closed in (False, True):
            cells[closed] = torch.empty((N, n_classes), dtype=torch.int64, device=device)
            _, s = timed(lambda: mesh(closed, cells[closed]), device)
            times["closed" if closed else "open"].append(s)
        sums = torch.empty((N, VL.N_SUMS), dtype=torch.int64, device=device)
        boxes = torch.empty((N, VL.N_BOX), dtype=torch.int32, device=device)
        _, s = timed(lambda: stats(sums, boxes), device)
        times["stats"].append(s)
    add("mesh_cells_open", times["open"], bool(torch.equal(cells[False], first[False])))
    add("mesh_cells_closed", times["closed"], bool(torch.equal(cells[True], first[True])))
    add("instance_stats", times["stats"])
    report["mesh_cells_open_over_instance_stats"] = report["mesh_cells_open"]["median_s"] / \
        report["instance_stats"]["median_s"]

    def sustained(fn):
        _, s = timed(lambda: [fn() for _ in range(args.sustained)], device)
        per_call = s / args.sustained
        return {"calls": args.sustained, "per_call_s": per_call, "bytes_per_s": nbytes / per_call,
                "share_of_hbm_peak": nbytes / per_call / HBM_PEAK}

    report["sustained"] = {"mesh_cells_open": sustained(lambda: mesh(False, cells[False])),
                           "mesh_cells_closed": sustained(lambda: mesh(True, cells[True])),
                           "instance_stats": sustained(lambda: stats(sums, boxes))}

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
