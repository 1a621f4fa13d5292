#!/usr/bin/env python
"""Time the labelled Euclidean distance transform (``sk_label_edt``) on two int32 masks:

  * the synthetic 512 x 512 x 128 mask of 1 000 ellipsoidal blobs of tools/bench_skeleton_graph.py, open mode;
  * one object that fills the same volume, closed mode: the walk's worst case, where a walk is as long as the object is
    thick.

Per mask: each of the three passes on its own (``sk_label_edt_pass``, device events around the call, buffers allocated
before), min / median / max of the repeats, against the bytes the pass moves -- 4 B of label, 8 B read and 8 B written
per voxel (the z pass reads no distance: 12 B) -- over the 8.0 TB/s HBM peak of the MI355X; the whole ``sk_label_edt``
call; and the mean number of steps a voxel's walk takes in each pass, counted from the pass's own output: a walk ends
at the first d with w d^2 >= its result (or at the volume's end), so floor(sqrt(result / w)), clipped to the steps the
volume allows, is its length to within one step.  The steps read 4 B of label and 8 B of distance each, mostly from
cache; the share of peak above does not count them, so it says how far the pass is from a plain streaming pass.

For context, ``scipy.ndimage.distance_transform_edt`` of the first mask on the CPU: ``--scipy-full`` instances as a user
of the reference would call it (one full-volume binary mask per id) and ``--scipy-crop`` instances cropped to their box
plus one voxel, which is less than the kernel computes (another instance outside the crop is not seen).

It asserts no threshold.

    python tools/bench_edt.py --out profiles/edt_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_instance_stats import HBM_PEAK, build_mask, summary, timed  # noqa: E402

AXES = (("z", 2), ("y", 1), ("x", 0))


def walk_steps(result, w, axis, closed):
    """mean steps per instance voxel of the pass along ``axis`` that produced ``result`` (float64 device tensor)"""
    E = result.shape[axis]
    k = torch.floor(torch.sqrt(result / w) + 1e-9)
    c = torch.arange(E, device=result.device, dtype=torch.float64).reshape([E if a == axis else 1 for a in range(3)])
    limit = torch.maximum(E - c, c + 1)                    # the step at which the farther direction leaves the volume
    k = torch.minimum(k, limit.expand_as(k))
    fg = result > 0
    return float(k[fg].sum().item() / max(1, int(fg.sum().item())))


def measure(x, spacing, closed, repeats, device):
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import label_edt
    from skoots_amd.validate import lib as VL
    rows = VL.id_rows(x)
    a, ids, lut, max_id = rows[1]
    X, Y, Z = (int(v) for v in a.shape)
    N = int(ids.numel())
    w = [s * s for s in spacing]
    first = label_edt(x, spacing, closed, rows)            # warm-up, and to compare
    bufs = [torch.empty((X, Y, Z), dtype=torch.float64, device=device) for _ in range(2)]
    mx = torch.zeros(N, dtype=torch.int64, device=device)
    st = _ffi.stream_ptr(device)
    head = (_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N)

    def one(axis, src, dst, row_max):
        _ffi.check(_ffi.lib.sk_label_edt_pass(*head, axis, w[axis], int(closed), _ffi.ptr(src) if src is not None else None,
                                              _ffi.ptr(dst), _ffi.ptr(row_max) if row_max is not None else None, st))

    plan = (("z", 2, None, bufs[0], None), ("y", 1, bufs[0], bufs[1], None), ("x", 0, bufs[1], bufs[0], mx))
    times = {name: [] for name, *_ in plan}
    whole = []
    steps = {}
    for r in range(repeats):
        for name, axis, src, dst, row_max in plan:
            _, s = timed(lambda: one(axis, src, dst, row_max), device)
            times[name].append(s)
            if r == 0:
                steps[name] = walk_steps(dst, w[axis], axis, closed)
        _, s = timed(lambda: _ffi.check(_ffi.lib.sk_label_edt(*head, w[0], w[1], w[2], int(closed), _ffi.ptr(bufs[0]),
                                                               _ffi.ptr(bufs[1]), _ffi.ptr(mx), st)), device)
        whole.append(s)
    voxels = X * Y * Z
    out = {"shape": [X, Y, Z], "instances": N, "spacing": list(spacing), "closed": bool(closed),
           "foreground_share": float((a > 0).sum().item() / voxels),
           "equals_first_run": bool(torch.equal(bufs[0].view(torch.int64), first[0].view(torch.int64)) and
                                    torch.equal(mx, first[1].view(torch.int64))),
           "largest_radius": float(torch.sqrt(first[1][torch.isfinite(first[1])].max()).item()) if N else 0.0,
           "passes": {}}
    for name, axis, src, *_ in plan:
        nbytes = voxels * (12 if src is None else 20)
        t = summary(times[name])
        t.update({"bytes_moved": nbytes, "bytes_per_s_at_median": nbytes / t["median_s"],
                  "share_of_hbm_peak_at_median": nbytes / t["median_s"] / HBM_PEAK,
                  "mean_walk_steps_per_instance_voxel": steps[name]})
        out["passes"][name] = t
    out["sk_label_edt"] = summary(whole)
    out["sk_label_edt"]["voxels_per_s_at_median"] = voxels / out["sk_label_edt"]["median_s"]
    return out, first


def scipy_context(x, spacing, n_full, n_crop):
    from scipy import ndimage
    lab = x.cpu().numpy()
    ids = np.unique(lab[lab > 0])
    rng = np.random.default_rng(0)
    out = {"threads": 1}
    pick = rng.choice(ids, min(n_full, len(ids)), replace=False)
    t = []
    for u in pick:
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(lab == u, sampling=spacing)
        t.append(time.perf_counter() - t0)
    if t:
        out["full_volume_per_instance"] = summary(t)
        out["full_volume_all_instances_extrapolated_s"] = float(np.median(t)) * len(ids)
    pick = rng.choice(ids, min(n_crop, len(ids)), replace=False)
    t = []
    for u in pick:
        nz = np.argwhere(lab == u)
        lo, hi = np.maximum(nz.min(0) - 1, 0), nz.max(0) + 2
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == u, sampling=spacing)
        t.append(time.perf_counter() - t0)
    if t:
        out["cropped_per_instance"] = summary(t)
        out["cropped_all_instances_extrapolated_s"] = float(np.median(t)) * len(ids)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 3.0))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scipy-full", type=int, default=2)
    ap.add_argument("--scipy-crop", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edt needs the GPU it measures")
    device = torch.device(args.device)
    shape, spacing = tuple(args.shape), tuple(args.spacing)
    report = {"device": torch.cuda.get_device_name(device), "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats}
    x = build_mask(shape, args.blobs, device)
    report["blobs_open"], _ = measure(x, spacing, False, args.repeats, device)
    report["scipy_cpu"] = scipy_context(x, spacing, args.scipy_full, args.scipy_crop)
    del x
    full = torch.ones(shape, dtype=torch.int32, device=device)
    report["one_object_closed"], _ = measure(full, spacing, True, args.repeats, device)
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
