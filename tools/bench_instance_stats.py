#!/usr/bin/env python
"""Time the per-instance measurement (``sk_instance_stats``) on a synthetic 1024 x 1024 x 256
int32 mask of a few thousand ellipsoidal blobs (the generator is below):

  * the kernel alone (device events around the library call, ids and look-up table prepared before): min / median /
    max, and the mask's bytes over those times against the 8.0 TB/s HBM peak of the MI355X -- the kernel reads the
    volume once, everything else it moves is negligible;
  * the prologue every call of ``stats_per_instance`` pays before the kernel, ``torch.unique`` plus the id -> row
    table, and its share of prologue + kernel;
  * the per-instance formulation the reference sketches (validate/compare.py: one full-volume ``x == id`` per instance;
    validate/lib.py: mask_to_bbox), restated in a few lines of torch -- ``(x == id).sum()`` and the box from
    ``nonzero()`` -- timed on a sample of the instances and extrapolated to all of them;
  * that the two agree on the sample (voxel count and box).

    python tools/bench_instance_stats.py --out profiles/instance_stats_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def build_mask(shape, n_blobs, device, seed=18):
    """int32 (X, Y, Z): n_blobs ellipsoids with semi-axes 6..22 x 6..22 x 3..9 at random places, ids 1..n_blobs shuffled;
    a later blob overwrites an earlier one where they overlap, so some objects end up cut or split."""
    gen = torch.Generator().manual_seed(seed)
    X, Y, Z = shape
    lab = torch.zeros(shape, dtype=torch.int32, device=device)
    ids = torch.randperm(n_blobs, generator=gen) + 1
    centre = torch.rand((n_blobs, 3), generator=gen) * torch.tensor([X, Y, Z])
    rad = torch.rand((n_blobs, 3), generator=gen) * torch.tensor([16.0, 16.0, 6.0]) + torch.tensor([6.0, 6.0, 3.0])
    for i in range(n_blobs):
        lo = [max(0, int(centre[i, k] - rad[i, k])) for k in range(3)]
        hi = [min(shape[k], int(centre[i, k] + rad[i, k]) + 2) for k in range(3)]
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        g = [(torch.arange(lo[k], hi[k], device=device, dtype=torch.float32) - centre[i, k].item()) / rad[i, k].item()
             for k in range(3)]
        inside = (g[0][:, None, None] ** 2 + g[1][None, :, None] ** 2 + g[2][None, None, :] ** 2) <= 1
        box = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        box[inside] = int(ids[i])
    return lab


def timed(fn, device):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(device))
    out = fn()
    b.record(torch.cuda.current_stream(device))
    b.synchronize()
    return out, a.elapsed_time(b) * 1e-3


def summary(times_s):
    return {"min_s": min(times_s), "median_s": statistics.median(times_s), "max_s": max(times_s), "all_s": times_s}


def per_instance(x, i):
    """the reference's formulation for one id: a full-volume mask, its count and its box"""
    m = x == i
    n = m.sum()
    nz = m.nonzero()
    return n, nz.min(0)[0], nz.max(0)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--blobs", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sample", type=int, default=24, help="instances the per-instance formulation is timed on")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instance_stats needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.compare import stats_per_instance

    shape = tuple(args.shape)
    x = build_mask(shape, args.blobs, device)
    nbytes = x.numel() * x.element_size()
    st = stats_per_instance(x)                                      # warm-up of every piece, and the result to compare
    N = int(st["id"].numel())
    report = {"device": torch.cuda.get_device_name(device), "shape": list(shape), "blobs": args.blobs, "instances": N,
              "foreground_share": float((st["voxels"].sum() / x.numel()).item()), "mask_bytes": nbytes,
              "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats}

    # ---- prologue (unique + table) and kernel, alternating
    tp, tk = [], []
    X, Y, Z = shape
    for _ in range(args.repeats):
        (ids, lut, max_id), s = timed(lambda: VL._lut(x), device)
        tp.append(s)
        sums = torch.empty((N, VL.N_SUMS), dtype=torch.int64, device=device)
        boxes = torch.empty((N, VL.N_BOX), dtype=torch.int32, device=device)
        _, s = timed(lambda: _ffi.check(_ffi.lib.sk_instance_stats(
            _ffi.ptr(x), X, Y, Z, _ffi.ptr(lut), max_id, N, _ffi.ptr(sums), _ffi.ptr(boxes), _ffi.stream_ptr(device))),
            device)
        tk.append(s)
    report["kernel_equals_first_run"] = bool(torch.equal(sums, st["sums"]) and torch.equal(boxes, st["bbox"]))
    report["kernel"] = summary(tk)
    report["kernel"]["bytes_per_s_at_median"] = nbytes / report["kernel"]["median_s"]
    report["kernel"]["share_of_hbm_peak_at_median"] = nbytes / report["kernel"]["median_s"] / HBM_PEAK
    report["prologue_unique_lut"] = summary(tp)
    report["prologue_share_of_prologue_plus_kernel"] = report["prologue_unique_lut"]["median_s"] / (
        report["prologue_unique_lut"]["median_s"] + report["kernel"]["median_s"])

    # ---- the per-instance formulation on a sample of the ids
    pick = torch.linspace(0, N - 1, min(args.sample, N)).long().tolist()
    id_list = st["id"].tolist()
    per_instance(x, id_list[pick[0]])                               # warm-up
    ts, agree = [], True
    for k in pick:
        (n, lo, hi), s = timed(lambda: per_instance(x, id_list[k]), device)
        ts.append(s)
        agree &= n.item() == st["voxels"][k].item() and torch.cat([lo, hi]).tolist() == st["bbox"][k].tolist()
    per = summary(ts)
    per["sample"] = len(pick)
    per["extrapolated_all_instances_s"] = statistics.mean(ts) * N
    per["agrees_with_kernel_on_sample"] = bool(agree)
    report["per_instance_formulation"] = per
    report["per_instance_over_one_pass"] = per["extrapolated_all_instances_s"] / (
        report["prologue_unique_lut"]["median_s"] + report["kernel"]["median_s"])

    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
