#!/usr/bin/env python
"""Time the rank and tap filters (``sk_filter_rank`` / ``sk_filter_taps``) on a noise image built
on the device, (1024, 1024, 256) uint8 and its uint16 twin (the same samples times 257), mirror borders.

Cases: the median of 3 x 3 x 1, 3 x 3 x 3 and 5 x 5 x 3, min and max of 3 x 3 x 3, the box mean of 3 x 3 x 3, and the
Gaussian at sigma (1, 1, 0.5) and (2, 2, 1).  Per case the C entry point alone is timed on a preallocated output --
``--inner`` calls between two device events, the time divided by that number -- after a warm-up, min / median / max over
the repeats, with the bytes the call must move (source + result; halo rows read again by neighbouring workgroups are not
counted) and that over the median time.  In the same process, alternating with it repeat by repeat:

  ``copy``        ``dst.copy_(src)`` that moves the same bytes (half of them read, half written): the floor every volume
                  pass here is set against
  ``other``       the two medians that have two selections: the same launch with the selection that ``auto`` does not
                  take (``radix`` against ``network``), the same-box A/B behind the choice

and, on the crop ``--crop`` of the volume (the 5 x 5 x 3 median on ``--crop-wide``, whose one-hot kernel has 75 channels),
where the 27-channel float32 feature tensor of the reference's formulation stays at a few GB:

  ``reference``   the reference's formulation on the device (skoots/lib/morphology.py): ``F.conv3d`` of a float32 copy with
                  the one-hot kernel of the window, then ``torch.median`` / ``min`` / ``max`` / ``mean`` over the channels,
                  and for the Gaussian ``F.conv3d`` with the dense float kernel; zero padding, the conversion to float
                  inside the time, the result left in float
  ``launch_crop`` this library on the same crop

``over_copy`` and ``over_reference`` are the launch's median time over theirs.  There is no pass or fail number.

    python tools/bench_filter.py --out profiles/filter_bench.json
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


def build_noise(shape, device, seed=29):
    """(X, Y, Z) uint8 noise over the whole range, slab by slab"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty(shape, dtype=torch.uint8, device=device)
    for x0 in range(0, shape[0], 64):
        sl = slice(x0, min(x0 + 64, shape[0]))
        out[sl] = torch.randint(0, 256, (sl.stop - sl.start,) + tuple(shape[1:]), generator=g, device=device).to(torch.uint8)
    return out


def widen(image):
    """the uint16 twin: every sample times 257, so that it covers 0 .. 65535"""
    return (image.to(torch.int32) * 257).to(torch.int16).view(torch.uint16)     # int32 -> int16 wraps: the bit pattern


CASES = (("median_3x3x1", "median", dict(radius=(1, 1, 0))),
         ("median_3x3x3", "median", dict(radius=(1, 1, 1))),
         ("median_5x5x3", "median", dict(radius=(2, 2, 1))),
         ("min_3x3x3", "min", dict(radius=(1, 1, 1))),
         ("max_3x3x3", "max", dict(radius=(1, 1, 1))),
         ("mean_3x3x3", "mean", dict(radius=(1, 1, 1))),
         ("gauss_1_1_0.5", "gauss", dict(sigma=(1, 1, 0.5))),
         ("gauss_2_2_1", "gauss", dict(sigma=(2, 2, 1))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--crop", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--crop-wide", type=int, nargs=3, default=(256, 256, 128))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="calls between two events")
    ap.add_argument("--dtypes", nargs="+", default=("uint8", "uint16"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter needs the GPU it measures")
    device = torch.device(args.device)
    import torch.nn.functional as F

    from skoots_amd import _ffi
    from skoots_amd.lib import morphology as M
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "inner": args.inner, "border": "mirror",
              "shape": list(args.shape), "volumes": []}

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

    def launcher(src, dst, plan, method="auto"):
        X, Y, Z = (int(n) for n in src.shape)
        code, stream = M._FILTER_CODE[src.dtype], _ffi.stream_ptr(device)
        if plan[0] == "rank":
            def launch():
                _ffi.check(_ffi.lib.sk_filter_rank(_ffi.ptr(src), _ffi.ptr(dst), code, X, Y, Z, *plan[1], plan[2],
                                                   M.FILTER_BORDER["mirror"], M.FILTER_METHOD[method], stream))
            return launch
        arrays = [M._int_array(t) for t in plan[1]]
        lists = [arg for a in arrays for arg in (a, len(a))]

        def launch():
            _ffi.check(_ffi.lib.sk_filter_taps(_ffi.ptr(src), _ffi.ptr(dst), code, X, Y, Z, *lists, M.FILTER_BORDER["mirror"],
                                               stream))
        return launch

    def reference(crop, how, plan):
        """the reference's formulation on a float32 copy, zero padding"""
        if plan[0] == "rank":
            size = tuple(2 * r + 1 for r in plan[1])
        else:
            size = tuple(len(t) for t in plan[1])
        n = size[0] * size[1] * size[2]
        if how == "gauss":
            kx, ky, kz = (torch.tensor(t, dtype=torch.float32) / sum(t) for t in plan[1])
            kernel = (kx[:, None, None] * ky[None, :, None] * kz[None, None, :]).reshape((1, 1) + size).to(device)
        else:
            kernel = torch.zeros((n, n), device=device)
            kernel.fill_diagonal_(1.0)
            kernel = kernel.reshape((n, 1) + size)
        padding = tuple(s // 2 for s in size)
        reduce = {"median": lambda f: torch.median(f, dim=1)[0], "min": lambda f: torch.min(f, dim=1)[0],
                  "max": lambda f: torch.max(f, dim=1)[0], "mean": lambda f: torch.mean(f, dim=1),
                  "gauss": lambda f: f[:, 0]}[how]

        def run():
            x = (crop.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32) if crop.dtype == torch.uint16 \
                else crop.to(torch.float32)
            return reduce(F.conv3d(x[None, None], kernel, padding=padding))
        return run

    def case(image, name, how, kwargs):
        shape = tuple(int(n) for n in image.shape)
        _, plan = M.check_filter(image, how, **kwargs)
        dst = torch.empty_like(image)
        moved = 2 * image.numel() * image.element_size()
        half = torch.empty(moved // 2, dtype=torch.uint8, device=device).random_(0, 256)
        other = torch.empty_like(half)
        path = M.filter_path(image.dtype, shape, how, **kwargs)
        fns, inner, names = [launcher(image, dst, plan), lambda: other.copy_(half)], [args.inner, args.inner], ["launch", "copy"]
        if path[0] == "network":
            fns.append(launcher(image, dst, plan, "radix"))
            inner.append(args.inner)
            names.append("other")
        runs = alternating(fns, inner)
        assert torch.equal(dst.view(torch.uint8), M.filter_volume(image, how, **kwargs).view(torch.uint8))
        row = {"operator": how, "arguments": {k: list(v) for k, v in kwargs.items()}, "dtype": str(image.dtype).split(".")[-1],
               "path": list(path)}
        if plan[0] == "taps":
            row["taps"] = [list(t) for t in plan[1]]
        for label, series in zip(names, runs):
            row[label] = spread(series, moved)
        if "other" in row:
            row["other"]["method"] = "radix"
            row["other_over_launch"] = row["other"]["median_s"] / row["launch"]["median_s"]
        row["over_copy"] = row["launch"]["median_s"] / row["copy"]["median_s"]
        del dst, half, other
        # the same crop for this library and the reference's formulation
        cs = tuple(args.crop_wide if name == "median_5x5x3" else args.crop)
        bits = image.view(torch.int16) if image.dtype == torch.uint16 else image
        crop = bits[:cs[0], :cs[1], :cs[2]].contiguous().view(image.dtype)
        crop_dst = torch.empty_like(crop)
        t_crop, t_ref = alternating((launcher(crop, crop_dst, plan), reference(crop, how, plan)), (args.inner, 1))
        row["crop"] = list(cs)
        row["launch_crop"] = spread(t_crop)
        row["reference"] = spread(t_ref)
        row["over_reference"] = row["launch_crop"]["median_s"] / row["reference"]["median_s"]
        del crop, crop_dst
        torch.cuda.empty_cache()
        return row

    base = build_noise(tuple(args.shape), device)
    for dtype in args.dtypes:
        image = base if dtype == "uint8" else widen(base)
        entry = {"dtype": dtype}
        for name, how, kwargs in CASES:
            entry[name] = case(image, name, how, kwargs)
            print(name, dtype, f"{entry[name]['launch']['median_s'] * 1e3:.3f} ms", file=sys.stderr, flush=True)
        report["volumes"].append(entry)
        del image
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
