#!/usr/bin/env python
"""Time eval()'s output writers on device-resident arrays: (A) the host path -- tensor.cpu().numpy() +
zarr_store.save + eval._write_mask_tif, one zlib stream at a time on one CPU thread -- against (B) the device path --
zarr_store.save_device + tiff.write_label_stack on top of the HIP deflate encoder (skoots_amd/csrc/deflate.hip).

The arrays are the three outputs of the 512 x 512 x 64 blob field of the tests (planar fp16 vectors and uint8 skeleton as
the pipeline's gate leaves them, the label mask), tiled --tiles times along X, Y, Z with labels renumbered per tile:
2 2 4 gives the 1024 x 1024 x 256 volume of BASELINE configs[2].  (A) runs once, (B) --repeats times after a warm-up;
per output: wall time, and for (B) the encoder's time (device events), the device-to-host copy of the compressed
bytes, the file writes, and the bytes on disk.  Both paths write into --dir; with --verify the stores and the TIFF of
(B) are read back and compared with the arrays.

--huffman names the codes of the device encoder to measure (fixed, dynamic, or both).  With both, the modes run in one
call and alternate (fixed, dynamic, fixed, ...), each warmed up once, and the median of --repeats is taken per mode:
"modes" holds the figures of each, "dynamic_vs_fixed" the bytes saved per output next to the encoder time it costs and
the copy and write time it saves.  "device_path" stays the first mode named.

    python tools/bench_eval_io.py --dir /tmp/evalio --huffman fixed dynamic --verify --out profiles/eval_io_bench.json
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_arrays(tiles, device):
    import scipy.ndimage as ndi

    from oracle import pipeline as O
    from tests.workload import blob_field
    out, k = blob_field((512, 512, 64), seed=3, n_blobs=300)
    vec, skel = O.gate_dilate(out.unsqueeze(0))
    vectors = vec[0].half().to(device).repeat(1, *tiles).contiguous()
    skeleton = skel[0].gt(O.SKEL_THR).to(torch.uint8).to(device).repeat(1, *tiles).contiguous()
    lab = torch.from_numpy(ndi.label(out[4].float().numpy() > 0.8)[0].astype(np.int32)).to(device)
    n_lab = int(lab.max())
    inst = torch.zeros([512 * tiles[0], 512 * tiles[1], 64 * tiles[2]], dtype=torch.int32, device=device)
    t = 0
    for i in range(tiles[0]):
        for j in range(tiles[1]):
            for l in range(tiles[2]):
                inst[i * 512:(i + 1) * 512, j * 512:(j + 1) * 512, l * 64:(l + 1) * 64] = \
                    torch.where(lab > 0, lab + t * n_lab, lab)
                t += 1
    return vectors, skeleton, inst


def tree_bytes(path):
    if os.path.isfile(path):
        return os.path.getsize(path)
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def run_host(arrays, d, device):
    from skoots_amd.lib import zarr_store
    from skoots_amd.lib.eval import _write_mask_tif
    vectors, skeleton, inst = arrays
    res = {}
    for name, path, fn in (
            ("skeleton", os.path.join(d, "a_skeleton.zarr"), lambda p: zarr_store.save(p, skeleton.cpu().numpy())),
            ("vectors", os.path.join(d, "a_vectors.zarr"), lambda p: zarr_store.save(p, vectors.cpu().numpy())),
            ("mask", os.path.join(d, "a_mask.tif"),
             lambda p: _write_mask_tif(p, inst.cpu().numpy().transpose(2, 0, 1)))):
        sync(device)
        t0 = time.perf_counter()
        fn(path)
        res[name] = {"wall_s": time.perf_counter() - t0, "bytes": tree_bytes(path)}
    return res


def run_device(arrays, d, device, huffman="fixed"):
    from skoots_amd.lib import tiff, zarr_store
    vectors, skeleton, inst = arrays
    res = {}
    for name, path, fn in (
            ("skeleton", os.path.join(d, "b_skeleton.zarr"), lambda p, tm: zarr_store.save_device(p, skeleton, timings=tm, huffman=huffman)),
            ("vectors", os.path.join(d, "b_vectors.zarr"), lambda p, tm: zarr_store.save_device(p, vectors, timings=tm, huffman=huffman)),
            ("mask", os.path.join(d, "b_mask.tif"),
             lambda p, tm: tiff.write_label_stack(p, inst.permute(2, 0, 1), timings=tm, huffman=huffman))):
        tm = {}
        sync(device)
        t0 = time.perf_counter()
        fn(path, tm)
        sync(device)
        tm["wall_s"] = time.perf_counter() - t0
        tm["bytes"] = tree_bytes(path)
        res[name] = tm
    return res


def verify(arrays, d):
    from skoots_amd.lib import tiff, zarr_store
    vectors, skeleton, inst = arrays
    ok = {"skeleton": bool(np.array_equal(zarr_store.load(os.path.join(d, "b_skeleton.zarr")), skeleton.cpu().numpy()))}
    got = zarr_store.load(os.path.join(d, "b_vectors.zarr"))
    ok["vectors"] = bool(np.array_equal(got.view(np.uint16), vectors.cpu().numpy().view(np.uint16)))   # -0.0 kept
    ok["mask"] = bool(np.array_equal(tiff.read_image(os.path.join(d, "b_mask.tif")),
                                     inst.cpu().numpy().transpose(2, 0, 1)))
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="directory both paths write into")
    ap.add_argument("--tiles", type=int, nargs=3, default=(2, 2, 4))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="'cpu' rehearses the plumbing; its times mean nothing")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--huffman", nargs="+", choices=("fixed", "dynamic"), default=["fixed"],
                    help="codes of the device encoder to measure; several alternate within one call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device(args.device)
    if device.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("bench_eval_io needs the GPU it measures (use --device cpu only to rehearse)")
    os.makedirs(args.dir, exist_ok=True)
    arrays = build_arrays(tuple(args.tiles), device)
    report = {"device": torch.cuda.get_device_name(device) if device.type == "cuda" else "cpu (rehearsal)",
              "shape": list(arrays[2].shape), "tiles": list(args.tiles),
              "raw_bytes": {"vectors": arrays[0].numel() * 2, "skeleton": arrays[1].numel(),
                            "mask": arrays[2].numel() * 2}}
    modes = list(dict.fromkeys(args.huffman))
    keys = ("wall_s", "kernel_s", "d2h_s", "file_s", "bytes", "compressed_bytes")
    for m in modes:
        run_device(arrays, args.dir, device, m)   # warm-up: code objects, allocator
    runs = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:                           # alternating, so that drift hits the modes alike
            runs[m].append(run_device(arrays, args.dir, device, m))
    report["repeats"] = args.repeats
    report["modes"] = {m: {name: {k: statistics.median(r[name].get(k, 0.0) for r in runs[m]) for k in keys}
                           for name in runs[m][0]} for m in modes}
    report["modes_kernel_all"] = {m: {name: [r[name].get("kernel_s", 0.0) for r in runs[m]] for name in runs[m][0]}
                                  for m in modes}
    report["device_path"] = report["modes"][modes[0]]
    report["device_path_wall_all"] = {name: [r[name]["wall_s"] for r in runs[modes[0]]] for name in runs[modes[0]][0]}
    if "fixed" in modes and "dynamic" in modes:
        f, d = report["modes"]["fixed"], report["modes"]["dynamic"]
        report["dynamic_vs_fixed"] = {
            name: {"bytes_ratio": d[name]["bytes"] / f[name]["bytes"], "bytes_saved": f[name]["bytes"] - d[name]["bytes"],
                   "kernel_s_added": d[name]["kernel_s"] - f[name]["kernel_s"],
                   "d2h_s_saved": f[name]["d2h_s"] - d[name]["d2h_s"], "file_s_saved": f[name]["file_s"] - d[name]["file_s"],
                   "wall_s_saved": f[name]["wall_s"] - d[name]["wall_s"]} for name in f}
    if args.verify:
        report["verified"] = {}
        for m in modes:                           # the files of the mode that ran last are on disk: write each again
            run_device(arrays, args.dir, device, m)
            report["verified"][m] = verify(arrays, args.dir)
    if not args.skip_host:
        report["host_path"] = run_host(arrays, args.dir, device)
        report["speedup_wall"] = {n: report["host_path"][n]["wall_s"] / report["device_path"][n]["wall_s"]
                                  for n in report["host_path"]}
        report["size_ratio"] = {n: report["device_path"][n]["bytes"] / report["host_path"][n]["bytes"]
                                for n in report["host_path"]}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
