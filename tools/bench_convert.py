#!/usr/bin/env python
"""Time the value transform of ``--convert`` on one (3, 1024, 1024, 256) fp16 vector array (mode 1: a store with
max < 2): (A) one pass of ``sk_convert_pages_u8`` against (B) the reference's chain of torch operations + permute on the
same device, alternating A, B, A, B ... in one process on the same tensor, device events around each; min / median /
max per route and the bytes the algorithm has to move (2 bytes read + 1 byte written per element) over those times.
The two results are compared at the timed size.  Then the whole ``convert()`` of that array as a zarr store: read,
min / max, transform, deflate, file -- wall time per read path, and the stages of one run timed one by one.

The array is zero outside random 32 x 32 x 16 blocks (about 30 % of the volume), uniform in [-1, 1] inside: incompressible
where it is not zero, so the deflate and file stages see more bytes than a real (smooth) vector field gives them.

    python tools/bench_convert.py --dir /tmp/convert_bench --out profiles/convert_bench.json
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


def build_vectors(shape, device, seed=17):
    gen = torch.Generator(device=device).manual_seed(seed)
    C, X, Y, Z = shape
    coarse = (torch.rand((1, -(-X // 32), -(-Y // 32), -(-Z // 16)), generator=gen, device=device) < 0.3).to(torch.uint8)
    mask = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2).repeat_interleave(16, 3)[:, :X, :Y, :Z]
    x = torch.rand(shape, generator=gen, device=device) * 2 - 1
    return (x * mask).to(torch.float16).contiguous()


def summary(times_s, nbytes):
    lo, med, hi = min(times_s), statistics.median(times_s), max(times_s)
    return {"min_s": lo, "median_s": med, "max_s": hi, "all_s": times_s,
            "bytes_per_s_at_median": nbytes / med, "bytes_per_s_at_min": nbytes / lo}


def timed(fn, device):
    if device.type != "cuda":
        return wall(fn, device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(device))
    out = fn()
    b.record(torch.cuda.current_stream(device))
    b.synchronize()
    return out, a.elapsed_time(b) * 1e-3


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def wall(fn, device):
    sync(device)
    t0 = time.perf_counter()
    out = fn()
    sync(device)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="directory for the store and the TIFF")
    ap.add_argument("--shape", type=int, nargs=4, default=(3, 1024, 1024, 256))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--whole-repeats", type=int, default=2)
    ap.add_argument("--device", default="cuda:0", help="'cpu' rehearses the plumbing (torch route on both sides); its "
                                                       "times mean nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device(args.device)
    if device.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("bench_convert needs the GPU it measures (use --device cpu only to rehearse)")
    from skoots_amd.lib import tiff, zarr_store
    from skoots_amd.utils import convert_trch_to_tif as CV
    kernel = CV.pages_kernel if device.type == "cuda" else CV.pages_torch
    shape = tuple(args.shape)
    os.makedirs(args.dir, exist_ok=True)
    x = build_vectors(shape, device)
    mode = CV.MODE_TRUNC
    nbytes = x.numel() * (x.element_size() + 1)
    report = {"device": torch.cuda.get_device_name(device) if device.type == "cuda" else "cpu (rehearsal)", "shape": list(shape), "dtype": "float16", "mode": mode,
              "algorithm_bytes": nbytes, "repeats": args.repeats}

    # ---- the transform alone: A / B alternating, after a warm-up of both
    a = kernel(x, mode)
    b = CV.pages_torch(x, mode)
    report["routes_equal"] = bool(torch.equal(a, b))
    del a, b
    tk, tt = [], []
    for _ in range(args.repeats):
        out, s = timed(lambda: kernel(x, mode), device)
        tk.append(s)
        del out
        out, s = timed(lambda: CV.pages_torch(x, mode), device)
        tt.append(s)
        del out
    report["kernel"] = summary(tk, nbytes)
    report["torch_route"] = summary(tt, nbytes)
    report["torch_over_kernel_median"] = report["torch_route"]["median_s"] / report["kernel"]["median_s"]

    # ---- the whole conversion of the store
    store = os.path.join(args.dir, "bench_skoots_vectors.zarr")
    zarr_store.save_device(store, x)
    tif = os.path.join(args.dir, "bench_skoots_vectors.tif")
    whole = {}
    for on_device in (True, False):
        runs = []
        for _ in range(args.whole_repeats if on_device else 1):   # the host reader inflates on one CPU thread: once
            _, s = wall(lambda: CV.convert(store, device=device, read_on_device=on_device), device)
            runs.append(s)
        whole["read_on_device" if on_device else "read_on_host"] = {"wall_s": runs}
    stages = {}
    tm = {}
    y, stages["read_s"] = wall(lambda: zarr_store.load_device(store, device, timings=tm), device)
    stages["read_detail"] = tm
    report["store_equal"] = bool(torch.equal(y.view(torch.int16), x.view(torch.int16)))
    vmax, stages["max_s"] = wall(lambda: y.max().item(), device)
    pages, stages["transform_s"] = wall(lambda: kernel(y, mode), device)
    tm = {}
    _, stages["write_s"] = wall(lambda: tiff.write_stack(tif, pages, timings=tm), device)
    stages["write_detail"] = tm
    whole["stages"] = stages
    whole["tif_bytes"] = os.path.getsize(tif)
    whole["store_bytes"] = sum(os.path.getsize(os.path.join(store, f)) for f in os.listdir(store))
    back = tiff.read_stack(tif, device)
    whole["tif_reads_back_equal"] = bool(torch.equal(back, pages))
    report["convert"] = whole

    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
