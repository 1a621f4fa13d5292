#!/usr/bin/env python
"""Time the device Blosc reader against the two things it stands next to, on real c-blosc output: the chunk frames of
tests/golden/blosc.npz, parts (a) (<f2 vectors: 262 144-byte blocks split in two byte planes, what an 8 MiB chunk of
the reference's stores consists of) and (b) (|u1 mask), replicated to at least 4096 LZ4 streams per launch.

Three sides, alternating (device, host, zlib, device, host, zlib, ...) in one process on the same bytes:
  device   blosc.decode_device: the frames uploaded as they are, sk_lz4_streams + sk_blosc_unshuffle; the kernels' own
           time from device events (GB/s of expanded bytes) and the wall time of the whole call (walk + upload included)
  host     blosc.decode_host (sk_blosc_decode_host per frame) + the upload of the expanded bytes, wall time
  zlib     the same chunks as zlib level 1 streams through deflate.inflate_streams (sk_inflate_streams), kernel and wall
The first round warms every side up and checks that all three give the same bytes.

    python tools/bench_blosc.py --out profiles/blosc_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=4096, help="LZ4 streams per launch, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="'cpu' rehearses the plumbing; its times mean nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device(args.device)
    cuda = device.type == "cuda"
    if cuda and not torch.cuda.is_available():
        raise SystemExit("bench_blosc needs the GPU it measures (use --device cpu only to rehearse)")
    from skoots_amd.lib import blosc, deflate
    from tests import blosc_corpus as C

    def sync():
        if cuda:
            torch.cuda.synchronize(device)

    d = np.load(os.path.join(ROOT, "tests", "golden", "blosc.npz"))
    frames = C.good_frames(d)
    report = {"device": torch.cuda.get_device_name(device) if cuda else "cpu (rehearsal)", "repeats": args.repeats, "sets": {}}
    for prefix, label in (("a", "vectors_f2"), ("b", "skeleton_u1")):
        base = [(f, raw) for n, f, raw in frames if n.startswith(prefix + ":")]
        chunk_bytes = len(base[0][1])
        per = len(blosc.plan([f for f, _ in base], chunk_bytes).streams)
        copies = -(-args.streams // per)
        fr = [f for f, _ in base] * copies
        zl = [zlib.compress(raw, 1) for _, raw in base] * copies
        total = len(fr) * chunk_bytes
        p = blosc.plan(fr, chunk_bytes)
        t = {k: [] for k in ("device_kernel_s", "device_wall_s", "host_wall_s", "zlib_kernel_s", "zlib_wall_s")}
        equal = None
        for r in range(args.repeats + 1):
            tm = {}
            sync()
            t0 = time.perf_counter()
            g = blosc.decode_device(fr, chunk_bytes, device, timings=tm)
            sync()
            td = time.perf_counter() - t0
            t0 = time.perf_counter()
            h = torch.from_numpy(blosc.decode_host(fr, chunk_bytes)).to(device)
            sync()
            th = time.perf_counter() - t0
            tz = {}
            t0 = time.perf_counter()
            z = deflate.inflate_streams(zl, chunk_bytes, device, timings=tz)
            sync()
            tzw = time.perf_counter() - t0
            if r == 0:
                equal = bool(torch.equal(g, h)) and bool(torch.equal(g, z))
            else:
                t["device_kernel_s"].append(tm.get("kernel_s", 0.0))
                t["device_wall_s"].append(td)
                t["host_wall_s"].append(th)
                t["zlib_kernel_s"].append(tz.get("kernel_s", 0.0))
                t["zlib_wall_s"].append(tzw)
            del g, h, z
        med = {k: statistics.median(v) for k, v in t.items()}
        e = {"frames": len(fr), "lz4_streams": int(p.streams.shape[0]), "unshuffle_blocks": int(p.blocks.shape[0]),
             "frame_bytes": sum(len(f) for f in fr), "zlib_bytes": sum(len(s) for s in zl), "expanded_bytes": total,
             "equal": equal, **{k: stats(v) for k, v in t.items()},
             "expanded_GB_per_s": {k: (total / v / 1e9 if v > 0 else None) for k, v in med.items()}}
        report["sets"][label] = e
        print(label, json.dumps(e), flush=True)
    print(json.dumps(report))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
