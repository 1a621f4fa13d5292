#!/usr/bin/env python
"""Time ``watershed_and_stitch`` on one (256, 1024, 1024) semantic mask, stage by stage, for every ``dim``: the plane
labelling (``sk_label_planes``; for dim 2 with its permuted copy), the overlap table (``sk_plane_overlaps`` + the sort of
the rows), the host walk (``sk_stitch_walk_host``), and relabel + renumber (``sk_relabel_lut``, ``sk_renumber``, for dim 2
with the copy back).  Device events around the device stages, wall time around the host walk and the whole call; min /
median / max over the repeats.  The labelling's floor is 1 byte read + 4 bytes written per voxel: the report gives
that many bytes over its time beside the HBM peak (8.0 TB/s; a float4 copy reaches 6.3 TB/s).  Then the CPU route of
the same module (scipy per slice, numpy.unique, the same host walk) on the same host, for the dims of ``--cpu-dims``.

The mask: the probability channel (> 0.5) of ``tests/workload.blob_field`` on a (256, 256, 64) block, Z first, tiled
4 x 4 x 4 -- the field's own generator holds five float32 channels and a noise array of the whole shape on the host, 11 GB
at the full size.  No object crosses a block's faces (the generator's margins), so the volume holds 64 x the block's blobs.

    python tools/bench_flood_and_stitch.py --out profiles/flood_and_stitch_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def build_mask(shape, blobs_per_block):
    from tests.workload import blob_field
    Z, X, Y = shape
    bz, bx, by = min(Z, 64), min(X, 256), min(Y, 256)
    out, placed = blob_field((bx, by, bz), seed=7, n_blobs=blobs_per_block, noise=0.0)
    block = (out[4] > 0.5).permute(2, 0, 1).to(torch.uint8)
    reps = (-(-Z // bz), -(-X // bx), -(-Y // by))
    return block.repeat(*reps)[:Z, :X, :Y].contiguous(), placed * reps[0] * reps[1] * reps[2]


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def timed(fn, device):
    """(result, seconds): device events on a GPU, wall time on the CPU."""
    if device.type != "cuda":
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(device))
    out = fn()
    b.record(torch.cuda.current_stream(device))
    b.synchronize()
    return out, a.elapsed_time(b) * 1e-3


def spread(times):
    return {"min_s": min(times), "median_s": statistics.median(times), "max_s": max(times), "all_s": times}


def staged(mask, dim, device):
    """One run of watershed_and_stitch's own steps with a timer around each.  Returns (labels, times, facts)."""
    from skoots_amd.utils import flood_and_stitch as F
    from skoots_amd.utils.renumber import renumber_first_seen
    permuted = mask.is_cuda and dim == 2
    t, facts = {}, {}

    def label():
        m = F._planes_first(mask, dim)
        if permuted:
            m = m.contiguous()
            store = lab = torch.empty(m.shape, dtype=torch.int32, device=m.device)
        else:
            store = torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
            lab = F._planes_first(store, dim)
        return store, lab, F._label_view(m, lab)

    (store, lab, offsets), t["label_s"] = timed(label, device)
    total = int(offsets[-1])
    rows, t["overlaps_s"] = timed(lambda: F._overlaps_view(lab, total), device)
    rows_host, offsets_host = rows.cpu(), offsets.cpu()
    t0 = time.perf_counter()
    lut, max_label = F.stitch_tables(offsets_host, rows_host)
    t["walk_s"] = time.perf_counter() - t0

    def finish():
        uniq, inverse = torch.unique(lut[1:], return_inverse=True)
        lut[1:] = inverse.to(torch.int32) + 1
        out = F._apply_lut(store, lut)
        out = F._planes_back(out, dim).contiguous() if permuted else out
        return renumber_first_seen(out, int(uniq.numel())), int(uniq.numel())

    (labels, k), t["relabel_renumber_s"] = timed(finish, device)
    facts.update(components=total, overlap_rows=int(rows.shape[0]), max_stitched_id=max_label, objects=k)
    return labels, t, facts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(256, 1024, 1024))
    ap.add_argument("--blobs-per-block", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-dims", type=int, nargs="*", default=[0], help="dims the CPU route is timed for (once each)")
    ap.add_argument("--device", default="cuda:0", help="'cpu' rehearses the plumbing; its times mean nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device(args.device)
    if device.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("bench_flood_and_stitch needs the GPU it measures (use --device cpu only to rehearse)")
    from skoots_amd.utils import flood_and_stitch as F
    shape = tuple(args.shape)
    mask_host, blobs = build_mask(shape, args.blobs_per_block)
    mask = mask_host.to(device)
    n = mask.numel()
    report = {"device": torch.cuda.get_device_name(device) if device.type == "cuda" else "cpu (rehearsal)", "shape": list(shape),
              "blobs_placed": blobs, "foreground_fraction": float(mask_host.float().mean()), "repeats": args.repeats,
              "label_floor_bytes": 5 * n, "hbm_peak_bytes_per_s": HBM_PEAK, "dims": {}}
    results = {}
    for dim in range(3):
        staged(mask, dim, device)                    # warm-up: allocator, kernels loaded
        runs, wholes = [], []
        for _ in range(args.repeats):
            labels, t, facts = staged(mask, dim, device)
            runs.append(t)
            sync(device)
            t0 = time.perf_counter()
            whole = F.watershed_and_stitch(mask, dim)
            sync(device)
            wholes.append(time.perf_counter() - t0)
        entry = {k: spread([r[k] for r in runs]) for k in runs[0]}
        entry["whole_call_wall"] = spread(wholes)
        entry["staged_equals_whole_call"] = bool(torch.equal(labels, whole))
        entry.update(facts)
        med = entry["label_s"]["median_s"]
        entry["label_floor_bytes_per_s_at_median"] = 5 * n / med
        entry["label_floor_fraction_of_hbm_peak"] = 5 * n / med / HBM_PEAK
        report["dims"][str(dim)] = entry
        results[dim] = whole.cpu()
        del labels, whole
    cpu = {}
    for dim in args.cpu_dims:
        t0 = time.perf_counter()
        want = F.watershed_and_stitch(mask_host, dim)
        cpu[str(dim)] = {"wall_s": time.perf_counter() - t0, "equals_device_route": bool(torch.equal(want, results[dim]))}
    report["cpu_route"] = cpu
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
