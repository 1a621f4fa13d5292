#!/usr/bin/env python
"""Time the pooling pass of the multiscale pyramids (``sk_pool_volume``) and ``write_ome_zarr`` on
synthetic volumes built on the device.

The masks are ``tools/bench_clean.py``'s: one ball per 32^3 cell with specks and pockets, at (512, 512, 128), about 1 000
balls, and at (1024, 1024, 256), 8192 balls.  The image is a seeded uint8 volume of the same shape (smooth ramps plus
noise), the binary volume the mask's ``> 0`` thinned to every fourth voxel.

Per level of ``plan_pyramid(shape, (1, 1, 3))`` the launch alone is timed -- the library call on a preallocated output,
``--inner`` launches between two device events, the time divided by that number -- after a warm-up, min / median / max
over the repeats, for ``mode`` on int32, ``mean`` on uint8 and ``max`` on uint8; with the bytes the launch moves (source
+ result) and that over the median time.  In the same process, the same way:

  ``clone``        ``dst.copy_(src)`` of the level-0 source: the bandwidth yardstick, 2 bytes moved per source byte
  ``avg_pool3d``   the torch composition for ``mean``: ``avg_pool3d`` on a float copy, rounded, cast back (the copy and the
                   cast are inside the time), level 0 -> 1 only
  ``max_pool3d``   the torch composition for ``max``: ``max_pool3d`` on a float copy and the cast back, level 0 -> 1 only
  ``write_ome_zarr``  the whole call -- image, ``labels/instances``, ``labels/skeleton`` -- into a temporary directory, wall
                   clock, with its ``timings`` dict: pooling, deflate kernels, device-to-host copies, file writes

``mode_level1_over_clone`` is the ratio the pass is judged by: the pool moves about 1.25 bytes per source byte (1.125 at
factors (2, 2, 1) ... 1.5 at one factor of 2) where the clone moves 2, so a launch slower than the clone needs an
explanation.  There is no pass or fail number.

    python tools/bench_pyramid.py --out profiles/pyramid_bench.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_clean import build_mask, spread, timed  # noqa: E402


def build_image(shape, device, seed=13):
    """(X, Y, Z) uint8: ramps along the three axes plus seeded noise"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    X, Y, Z = shape
    x = torch.arange(X, device=device)[:, None, None]
    y = torch.arange(Y, device=device)[None, :, None]
    z = torch.arange(Z, device=device)[None, None, :]
    out = torch.empty(shape, dtype=torch.uint8, device=device)
    for x0 in range(0, X, 64):
        sl = slice(x0, min(x0 + 64, X))
        noise = torch.randint(0, 64, (sl.stop - sl.start, Y, Z), generator=g, device=device)
        out[sl] = ((x[sl] // 8 + y // 4 + z * 2 + noise) % 256).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=int, nargs="+", default=(512, 512, 128, 1024, 1024, 256), help="X Y Z [X Y Z ...]")
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 3.0))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="launches between two events")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if len(args.shapes) % 3:
        raise SystemExit("--shapes takes triples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyramid needs the GPU it measures")
    device = torch.device(args.device)
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import POOL_HOW
    from skoots_amd.utils.pyramid import plan_pyramid, pyramid, write_ome_zarr
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "inner": args.inner,
              "spacing": list(args.spacing), "volumes": []}

    def series(fn, nbytes=None):
        fn()                                                             # warm-up: allocator, kernels loaded
        torch.cuda.synchronize(device)
        runs = []
        for _ in range(args.repeats):
            def many():
                for _ in range(args.inner):
                    fn()
            _, t = timed(many, device)
            runs.append(t / args.inner)
        return spread(runs, nbytes)

    def launch(src, dst, factors, how):
        X, Y, Z = src.shape
        _ffi.check(_ffi.lib.sk_pool_volume(_ffi.ptr(src), _ffi.dtype_code(src), X, Y, Z, *factors, POOL_HOW[how], 0,
                                           _ffi.ptr(dst), _ffi.stream_ptr(device)))

    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]
    for shape in shapes:
        mask, cells = build_mask(shape, device)
        image = build_image(shape, device)
        binary = ((mask > 0) & (torch.arange(shape[2], device=device) % 4 == 0)).to(torch.uint8)
        plan = plan_pyramid(shape, args.spacing)
        entry = {"shape": list(shape), "instances": cells, "foreground_fraction": float((mask > 0).float().mean()),
                 "plan": [{"factors": list(lv.factors), "shape": list(lv.shape), "spacing": list(lv.spacing)} for lv in plan]}
        for how, vol in (("mode", mask), ("mean", image), ("max", binary)):
            levels, _ = pyramid(vol, args.spacing, how, plan=plan)
            rows = []
            for k in range(1, len(plan)):
                src, dst = levels[k - 1], torch.empty_like(levels[k])
                nbytes = (src.numel() + dst.numel()) * src.element_size()
                d = series(lambda: launch(src, dst, plan[k].factors, how), nbytes)
                assert torch.equal(dst, levels[k])
                d.update({"level": k, "factors": list(plan[k].factors), "source_shape": list(src.shape)})
                rows.append(d)
            key = f"{how}_{str(vol.dtype).split('.')[-1]}"
            entry[key] = rows
            scratch = torch.empty_like(vol)
            entry[key + "_clone"] = series(lambda: scratch.copy_(vol), 2 * vol.numel() * vol.element_size())
            rows[0]["over_clone"] = rows[0]["median_s"] / entry[key + "_clone"]["median_s"]
            del scratch, levels
        entry["mode_level1_over_clone"] = entry["mode_int32"][0]["over_clone"]
        f1 = tuple(plan[1].factors) if len(plan) > 1 else None
        if f1 is not None:
            import torch.nn.functional as F
            entry["torch_avg_pool3d"] = series(lambda: F.avg_pool3d(image[None, None].float(), f1, ceil_mode=True)
                                               .add_(0.5).floor_().to(torch.uint8))
            entry["torch_max_pool3d"] = series(lambda: F.max_pool3d(binary[None, None].float(), f1, ceil_mode=True)
                                               .to(torch.uint8))
        tmp = tempfile.mkdtemp(prefix="bench_pyramid_")
        try:
            runs, last = [], {}
            for _ in range(2):                                           # the first is the warm-up
                timings = {}
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                rep = write_ome_zarr(os.path.join(tmp, "v.ome.zarr"), args.spacing, image=image,
                                     labels={"instances": mask, "skeleton": (binary, "max")}, timings=timings)
                runs.append(time.perf_counter() - t0)
                last = {"wall_s": runs[-1], "bytes_written": rep["bytes_written"], "levels": rep["levels"],
                        "pool_s": timings.get("pool_s"), "deflate_kernel_s": timings.get("kernel_s"),
                        "d2h_s": timings.get("d2h_s"), "file_s": timings.get("file_s"),
                        "compressed_bytes": timings.get("compressed_bytes")}
            last["first_call_wall_s"] = runs[0]
            entry["write_ome_zarr"] = last
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        report["volumes"].append(entry)
        del mask, image, binary
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
