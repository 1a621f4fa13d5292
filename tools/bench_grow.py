#!/usr/bin/env python
"""Time the nearest-instance transform (``sk_nearest_label``) and ``utils.grow.grow`` on two int32
masks:

  * the synthetic 512 x 512 x 128 mask of 1 000 ellipsoidal blobs of tools/bench_edt.py, at spacing (1, 1, 3) and the
    distances 2, 5 and 15;
  * the (1024, 1024, 256) mask of tools/bench_clean.py, at distance 5.

Per mask and distance: each of the three passes on its own (``sk_nearest_label_pass``, device events around the call,
buffers allocated before), min / median / max of the repeats, against the bytes the pass must move -- 4 B of label, 12 B
of (distance, row) read and 12 B written per voxel (the z pass reads no source: 16 B) -- over the 8.0 TB/s HBM peak of the
MI355X; the whole ``sk_nearest_label`` call; ``grow`` as a whole call (id table, transform, selection, report); and the
mean number of positions a voxel's walk reads in each pass, counted from the pass's own output: a walk ends at the first
d with w d^2 above its result or above limit2 (or at the volume's end), so floor(sqrt(min(result, limit2) / w)) on either
side, clipped to the positions the volume has there, is its reads to within one per side.  A read is 4 B of label in the z
pass and 8 B of distance in the others (4 B of row more where the position wins), mostly from cache; the share of peak
above does not count them, so it says how far the pass is from a plain streaming pass.

Beside them, ``sk_label_edt`` on the same mask in the same process (the same kind of walk on the instance voxels only),
and for context one ``scipy.ndimage.distance_transform_edt(mask == 0, sampling, return_indices=True)`` of the first mask
on the CPU.

It asserts no threshold.

    python tools/bench_grow.py --out profiles/grow_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_instance_stats import HBM_PEAK, build_mask, summary, timed  # noqa: E402


def walk_reads(g, w, axis, limit2, walked):
    """mean positions read per voxel of the volume by the pass along ``axis`` that produced ``g`` (float64 device tensor);
    ``walked``: the voxels that walk at all (no sites, and in the last pass only the wanted ones)"""
    E = g.shape[axis]
    k = torch.floor(torch.sqrt(torch.clamp(g, max=limit2) / w) + 1e-9)
    c = torch.arange(E, device=g.device, dtype=torch.float64).reshape([E if a == axis else 1 for a in range(3)])
    reads = torch.minimum(k, c.expand_as(k)) + torch.minimum(k, (E - 1 - c).expand_as(k))
    return float((reads * walked).sum().item() / g.numel())


def measure(x, spacing, distance, repeats, device):
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import nearest_label
    from skoots_amd.utils.grow import grow
    from skoots_amd.validate import lib as VL
    rows = VL.id_rows(x)
    a, ids, lut, max_id = rows[1]
    X, Y, Z = (int(v) for v in a.shape)
    N = int(ids.numel())
    w = [s * s for s in spacing]
    limit2 = float(distance) * float(distance)
    first = nearest_label(x, spacing, distance, rows=rows)          # warm-up, and to compare
    d = [torch.empty((X, Y, Z), dtype=torch.float64, device=device) for _ in range(2)]
    r = [torch.empty((X, Y, Z), dtype=torch.int32, device=device) for _ in range(2)]
    st = _ffi.stream_ptr(device)
    head = (_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N)
    walked = first[1] > 0                                           # the sites are the voxels at distance 0

    def one(axis, src, dst):
        _ffi.check(_ffi.lib.sk_nearest_label_pass(*head, axis, w[axis], limit2,
                                                  _ffi.ptr(d[src]) if src is not None else None,
                                                  _ffi.ptr(r[src]) if src is not None else None, None,
                                                  _ffi.ptr(d[dst]), _ffi.ptr(r[dst]), st))

    plan = (("z", 2, None, 0), ("y", 1, 0, 1), ("x", 0, 1, 0))
    times = {name: [] for name, *_ in plan}
    whole, grow_s, edt_s = [], [], []
    reads = {}
    edt_bufs = [torch.empty((X, Y, Z), dtype=torch.float64, device=device) for _ in range(2)]
    for rep in range(repeats + 1):                                   # the first turn warms every call up
        for name, axis, src, dst in plan:
            _, s = timed(lambda: one(axis, src, dst), device)
            if rep:
                times[name].append(s)
            else:
                reads[name] = walk_reads(d[dst], w[axis], axis, limit2, walked)
        if rep == 0:
            passes_equal = bool(torch.equal(d[0].view(torch.int64), first[1].view(torch.int64)))
        _, s = timed(lambda: _ffi.check(_ffi.lib.sk_nearest_label(*head, w[0], w[1], w[2], limit2, None, _ffi.ptr(d[0]),
                                                                   _ffi.ptr(r[0]), _ffi.ptr(d[1]), _ffi.ptr(r[1]), st)),
                     device)
        out, g = timed(lambda: grow(x, distance, spacing), device)
        _, e = timed(lambda: _ffi.check(_ffi.lib.sk_label_edt(*head, w[0], w[1], w[2], 0, _ffi.ptr(edt_bufs[0]),
                                                               _ffi.ptr(edt_bufs[1]), None, st)), device)
        if rep:
            whole.append(s)
            grow_s.append(g)
            edt_s.append(e)
    voxels = X * Y * Z
    res = {"shape": [X, Y, Z], "instances": N, "spacing": list(spacing), "distance": distance,
           "foreground_share": float((a > 0).sum().item() / voxels),
           "passes_equal_first_run": passes_equal,
           "fused_equals_first_run": bool(torch.equal(d[0].view(torch.int64), first[1].view(torch.int64))),
           "voxels_added": out[1].voxels_added, "ids_grown": out[1].ids_grown, "passes": {}}
    for name, axis, src, _ in plan:
        nbytes = voxels * (16 if src is None else 28)
        t = summary(times[name])
        t.update({"bytes_moved": nbytes, "bytes_per_s_at_median": nbytes / t["median_s"],
                  "share_of_hbm_peak_at_median": nbytes / t["median_s"] / HBM_PEAK,
                  "mean_reads_per_voxel": reads[name],
                  "read_bound_per_voxel": 2 * int((limit2 / w[axis]) ** 0.5 + 1e-9)})
        res["passes"][name] = t
    res["sk_nearest_label"] = summary(whole)
    res["sk_nearest_label"]["voxels_per_s_at_median"] = voxels / res["sk_nearest_label"]["median_s"]
    res["grow"] = summary(grow_s)
    res["sk_label_edt_same_mask_open"] = summary(edt_s)
    return res


def scipy_context(x, spacing):
    from scipy import ndimage
    lab = x.cpu().numpy()
    t0 = time.perf_counter()
    ndimage.distance_transform_edt(lab == 0, sampling=spacing, return_indices=True)
    return {"threads": 1, "distance_transform_edt_return_indices_s": time.perf_counter() - t0, "shape": list(lab.shape)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 3.0))
    ap.add_argument("--distances", type=float, nargs="+", default=(2.0, 5.0, 15.0))
    ap.add_argument("--big-shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--big-distance", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grow needs the GPU it measures")
    from tools.bench_clean import build_mask as build_cells
    device = torch.device(args.device)
    spacing = tuple(args.spacing)
    report = {"device": torch.cuda.get_device_name(device), "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats,
              "blobs": []}
    x = build_mask(tuple(args.shape), args.blobs, device)
    for distance in args.distances:
        report["blobs"].append(measure(x, spacing, float(distance), args.repeats, device))
    if not args.no_scipy:
        report["scipy_cpu"] = scipy_context(x, spacing)
    del x
    torch.cuda.empty_cache()
    big, _ = build_cells(tuple(args.big_shape), device)
    report["cells"] = measure(big, spacing, float(args.big_distance), args.repeats, device)
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
