#!/usr/bin/env python
"""Time the change of grid (``sk_resample_volume``) on synthetic volumes built on the device.

Cases, at (1024, 1024, 256) and at (512, 512, 128), which sits inside the Infinity Cache:

  ``image_up``      uint8 image, ``auto`` at (1.5, 1.5, 1): linear in x and y, z kept
  ``image_down``    uint8 image, ``auto`` at (0.5, 0.5, 1): area in x and y, z kept
  ``image_iso``     uint8 image, ``auto`` at (1, 1, 3): the isotropic case, linear in z
  ``mask_back``     int32 mask, ``nearest`` from the (1.5, 1.5, 1) grid back to the volume's own

Per case the call alone is timed -- the C entry point on a preallocated output and workspace, the three prologue launches
included, ``--inner`` calls between two device events, the time divided by that number -- after a warm-up, min / median
/ max over the repeats, with the bytes the call must move (source + result; tap rows read again by neighbouring output
rows are not counted, and ``nearest`` onto a coarser grid counts one source voxel per output voxel) and that over the
median time.  In the same process, alternating with it repeat by repeat:

  ``copy``          ``dst.copy_(src)`` that moves the same bytes (half of them read, half written): the bandwidth yardstick
  ``interpolate``   ``torch.nn.functional.interpolate`` on a float32 copy (``trilinear`` / ``area`` / ``nearest``), the
                    conversion to float and back inside the time: what a user would otherwise run

``over_copy`` and ``over_interpolate`` are the launch's median time over theirs.  There is no pass or fail number.

    python tools/bench_resample.py --out profiles/resample_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_clean import spread, timed  # noqa: E402
from tools.bench_pyramid import build_image  # noqa: E402


def build_labels(shape, device, seed=17):
    """(X, Y, Z) int32: one id per 16 x 16 x 8 cell, a third of the cells background"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    X, Y, Z = shape
    cells = (-(-X // 16), -(-Y // 16), -(-Z // 8))
    ids = torch.arange(1, cells[0] * cells[1] * cells[2] + 1, device=device, dtype=torch.int32).reshape(cells)
    ids = torch.where(torch.rand(cells, generator=g, device=device) < 1 / 3, torch.zeros_like(ids), ids)
    return ids.repeat_interleave(16, 0)[:X].repeat_interleave(16, 1)[:, :Y].repeat_interleave(8, 2)[:, :, :Z].contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256), help="X Y Z [X Y Z ...]")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="calls between two events")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs the GPU it measures")
    device = torch.device(args.device)
    import torch.nn.functional as F

    from skoots_amd import _ffi
    from skoots_amd.lib import morphology as M
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "inner": args.inner, "volumes": []}

    def once(fn, inner):
        def many():
            for _ in range(inner):
                fn()
        return timed(many, device)[1] / inner

    def alternating(fns, inner):
        """one series per function, a repeat of each in turn"""
        for fn in fns:
            fn()                                                         # warm-up: allocator, kernels loaded
        torch.cuda.synchronize(device)
        runs = [[] for _ in fns]
        for _ in range(args.repeats):
            for k, fn in enumerate(fns):
                runs[k].append(once(fn, inner[k]))
        return runs

    def case(src, factors, how, mode):
        shape = tuple(int(n) for n in src.shape)
        out_shape = M.resample_shape(shape, factors)
        _, ops = M.check_resample(src, out_shape, how)
        code = _ffi.dtype_code(src)
        geometry = (code, *shape, *out_shape, *(M.RESAMPLE_OP[o] for o in ops))
        nbytes_ws = int(_ffi.lib.sk_resample_workspace_bytes(*geometry))
        dst = torch.empty(out_shape, dtype=src.dtype, device=device)
        ws = torch.empty(nbytes_ws, dtype=torch.uint8, device=device)
        # nearest reads one source voxel per output voxel: when the grid gets coarser, not the whole source
        read = min(src.numel(), dst.numel()) if how == "nearest" else src.numel()
        moved = (read + dst.numel()) * src.element_size()
        half = torch.empty(moved // 2, dtype=torch.uint8, device=device).random_(0, 256)
        other = torch.empty_like(half)

        def launch():
            _ffi.check(_ffi.lib.sk_resample_volume(_ffi.ptr(src), _ffi.ptr(dst), *geometry, _ffi.ptr(ws), nbytes_ws,
                                                   _ffi.stream_ptr(device)))

        def interpolate():
            kw = {"align_corners": False} if mode == "trilinear" else {}
            y = F.interpolate(src[None, None].float(), size=out_shape, mode=mode, **kw)
            return (y.add_(0.5).floor_() if mode != "nearest" else y).to(src.dtype)

        t_launch, t_copy, t_torch = alternating((launch, lambda: other.copy_(half), interpolate), (args.inner, args.inner, 1))
        assert torch.equal(dst, M.resample(src, shape=out_shape, how=how))
        row = {"source_shape": list(shape), "shape": list(out_shape), "dtype": str(src.dtype).split(".")[-1],
               "operators": list(ops), "path": M.resample_path(src.dtype, shape, out_shape, ops),
               "workspace_bytes": nbytes_ws, "launch": spread(t_launch, moved), "copy": spread(t_copy, moved),
               "interpolate": dict(spread(t_torch), mode=mode)}
        row["over_copy"] = row["launch"]["median_s"] / row["copy"]["median_s"]
        row["over_interpolate"] = row["launch"]["median_s"] / row["interpolate"]["median_s"]
        del dst, ws, half, other
        torch.cuda.empty_cache()
        return row

    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]
    for shape in shapes:
        image = build_image(shape, device)
        entry = {"shape": list(shape)}
        entry["image_up"] = case(image, (1.5, 1.5, 1), "auto", "trilinear")
        entry["image_down"] = case(image, (0.5, 0.5, 1), "auto", "area")
        entry["image_iso"] = case(image, (1, 1, 3), "auto", "trilinear")
        del image
        grid = M.resample_shape(shape, (1.5, 1.5, 1))
        mask = build_labels(grid, device)
        row = case(mask, tuple(n / m for n, m in zip(shape, grid)), "nearest", "nearest")
        assert tuple(row["shape"]) == tuple(shape)
        entry["mask_back"] = row
        del mask
        report["volumes"].append(entry)
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
