#!/usr/bin/env python
"""Time the device readers against the host readers they stand in for, on the outputs of the 1024 x 1024 x 256 blob field
(tools/bench_eval_io.py: build_arrays): for the skeleton and vector stores written by zarr_store.save (host zlib level 1)
and by zarr_store.save_device, ``load_device`` against ``load`` + upload; for the mask TIFF written by Pillow
(eval._write_mask_tif), by tiff.write_label_stack on the device and by tiff.write_stack on the host (zlib level 1),
``read_stack`` against ``read_image`` + upload.  The two sides alternate (host, device, host, device, ...) on the same
files; per file and side: min / median / max of the wall times, and for the device side the kernel's own time from device
events with the bytes it produced per second in aggregate.  One chunk / one page alone gives the rate of a single stream.

    python tools/bench_inflate.py --out profiles/inflate_bench.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def tree_bytes(path):
    if os.path.isfile(path):
        return os.path.getsize(path)
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=None, help="directory for the files (default: a temporary one, removed at the end)")
    ap.add_argument("--tiles", type=int, nargs=3, default=(2, 2, 4))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", default="cuda:0", help="'cpu' rehearses the plumbing; its times mean nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device(args.device)
    cuda = device.type == "cuda"
    if cuda and not torch.cuda.is_available():
        raise SystemExit("bench_inflate needs the GPU it measures (use --device cpu only to rehearse)")
    from bench_eval_io import build_arrays

    from skoots_amd.lib import deflate, tiff, zarr_store
    from skoots_amd.lib.eval import _write_mask_tif
    d = args.dir or tempfile.mkdtemp(prefix="bench_inflate_")
    os.makedirs(d, exist_ok=True)

    def sync():
        if cuda:
            torch.cuda.synchronize(device)

    vectors, skeleton, inst = build_arrays(tuple(args.tiles), device)
    mask = inst.permute(2, 0, 1).contiguous()
    report = {"device": torch.cuda.get_device_name(device) if cuda else "cpu (rehearsal)", "shape": list(inst.shape),
              "repeats": args.repeats, "files": {}}
    files = []
    t0 = time.perf_counter()
    for name, arr in (("skeleton", skeleton), ("vectors", vectors)):
        a, b = os.path.join(d, f"{name}_save.zarr"), os.path.join(d, f"{name}_save_device.zarr")
        zarr_store.save(a, arr.cpu().numpy())
        zarr_store.save_device(b, arr)
        files += [(f"{name}:save", "zarr", a), (f"{name}:save_device", "zarr", b)]
    host_mask = mask.cpu().numpy()
    _write_mask_tif(os.path.join(d, "mask_pillow.tif"), host_mask)
    tiff.write_label_stack(os.path.join(d, "mask_write_label_stack.tif"), mask)
    narrow = host_mask.astype(np.uint16) if host_mask.max() < 65536 else host_mask
    tiff.write_stack(os.path.join(d, "mask_host_zlib1.tif"), narrow)
    files += [("mask:pillow", "tiff", os.path.join(d, "mask_pillow.tif")),
              ("mask:write_label_stack", "tiff", os.path.join(d, "mask_write_label_stack.tif")),
              ("mask:host_zlib1", "tiff", os.path.join(d, "mask_host_zlib1.tif"))]
    del vectors, skeleton, inst, mask
    report["write_files_s"] = time.perf_counter() - t0
    print(f"files written in {report['write_files_s']:.1f} s", flush=True)

    for label, kind, path in files:
        host_t, dev_t, kern_t, out_bytes, equal = [], [], [], 0, None
        for r in range(args.repeats + 1):          # the first round warms both sides up and checks equality
            sync()
            t0 = time.perf_counter()
            if kind == "zarr":
                h = torch.from_numpy(zarr_store.load(path)).to(device)
            else:
                h = torch.from_numpy(tiff.read_image(path)).to(device)
            sync()
            th = time.perf_counter() - t0
            tm = {}
            t0 = time.perf_counter()
            g = zarr_store.load_device(path, device, timings=tm) if kind == "zarr" else tiff.read_stack(path, device, timings=tm)
            sync()
            td = time.perf_counter() - t0
            if r == 0:
                equal = bool(torch.equal(h.view(torch.uint8), g.view(torch.uint8)))
                out_bytes = g.numel() * g.element_size()
            else:
                host_t.append(th)
                dev_t.append(td)
                kern_t.append(tm.get("kernel_s", 0.0))
            inflated = tm.get("inflated_bytes", 0)
            del h, g
        e = {"file_bytes": tree_bytes(path), "array_bytes": out_bytes, "equal": equal, "host_wall_s": stats(host_t),
             "device_wall_s": stats(dev_t), "kernel_s": stats(kern_t), "inflated_bytes": inflated,
             "kernel_bytes_out_per_s": inflated / statistics.median(kern_t) if statistics.median(kern_t) > 0 else None,
             "speedup_median": statistics.median(host_t) / statistics.median(dev_t)}
        report["files"][label] = e
        print(label, json.dumps(e), flush=True)

    # one stream alone: the first chunk of the vectors store, one page of each mask file
    single = {}
    vdir = os.path.join(d, "vectors_save.zarr")
    meta = json.load(open(os.path.join(vdir, ".zarray")))
    chunk_bytes = int(np.prod(meta["chunks"])) * np.dtype(meta["dtype"]).itemsize
    chunk_files = sorted(f for f in os.listdir(vdir) if f != ".zarray")
    streams = {"vectors_chunk:save": (open(os.path.join(vdir, chunk_files[len(chunk_files) // 2]), "rb").read(), chunk_bytes)}
    vdir = os.path.join(d, "vectors_save_device.zarr")
    streams["vectors_chunk:save_device"] = (open(os.path.join(vdir, chunk_files[len(chunk_files) // 2]), "rb").read(), chunk_bytes)
    for label, kind, path in files:
        if kind == "tiff":
            plan = tiff.scan(path)
            p = plan.pages[len(plan.pages) // 2]
            buf = open(path, "rb").read()
            size = min(p.rows_per_strip, p.height) * p.width * (p.bits // 8)
            streams[f"{label}:strip"] = (buf[p.strip_offsets[0]:p.strip_offsets[0] + p.strip_byte_counts[0]], size)
    for label, (stream, size) in streams.items():
        ks = []
        for r in range(args.repeats + 1):
            tm = {}
            deflate.inflate_streams([stream], size, device, timings=tm)
            if r:
                ks.append(tm.get("kernel_s", 0.0))
        k = statistics.median(ks)
        single[label] = {"stream_bytes": len(stream), "bytes_out": size, "kernel_s": stats(ks),
                         "bytes_out_per_s": size / k if k > 0 else None}
        print(label, json.dumps(single[label]), flush=True)
    report["single_stream"] = single
    if args.dir is None:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
