#!/usr/bin/env python
"""Time the tile histograms and the table pass (``sk_tile_histograms`` / ``sk_apply_tile_luts``) on
a noise image built on the device, (1024, 1024, 256) uint8 and its uint16 twin (the same samples times 257; 1024 bins,
shift 6).

Histograms under three tilings -- one tile, ``"slices"`` and (64, 64, 16) -- and, for one tile, also on a constant
volume, where every sample meets one counter.  The table pass under one tile, slices, and (64, 64, 16) interpolated,
with tables of arbitrary values.  Per case the C entry point alone is timed on preallocated outputs -- ``--inner`` calls
between two device events, the time divided by that number -- after a warm-up, min / median / max over the repeats, with
the bytes the call must move (the volume read; for the table pass also written) and that over the median time.  In the
same process, alternating with it repeat by repeat:

  ``copy``         ``dst.copy_(src)`` that moves the same bytes (half of them read, half written)
  ``u8_histogram`` one tile, uint8 only: ``sk_u8_histogram`` of csrc/dataset_stats.hip, the whole-volume histogram the
                   training command uses -- the natural yardstick of the one-tile case

and on the crop ``--crop`` of the volume a torch formulation next to this library on the same crop:

  ``torch``        histograms: ``torch.bincount`` of ``tile_index * bins + bin``; table pass: the eight corner gathers
                   by indexing with broadcast per-axis weights in int64, then ``(S + W // 2) // W`` (no ``grid_sample``)
  ``launch_crop``  this library on the same crop

``over_copy``, ``over_u8_histogram`` and ``over_torch`` are the launch's median time over theirs.  There is no pass or
fail number.

    python tools/bench_equalize.py --out profiles/equalize_bench.json
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
from tools.bench_filter import build_noise, widen  # noqa: E402

TILINGS = (("one_tile", None), ("slices", "slices"), ("blocks_64x64x16", (64, 64, 16)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--crop", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="calls between two events")
    ap.add_argument("--dtypes", nargs="+", default=("uint8", "uint16"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_equalize needs the GPU it measures")
    device = torch.device(args.device)

    from skoots_amd import _ffi
    from skoots_amd.lib import morphology as M
    report = {"device": torch.cuda.get_device_name(device), "repeats": args.repeats, "inner": args.inner,
              "shape": list(args.shape), "volumes": []}
    stream = _ffi.stream_ptr(device)

    def once(fn, inner):
        def many():
            for _ in range(inner):
                fn()
        return timed(many, device)[1] / inner

    def alternating(fns, inner):
        for fn in fns:
            fn()
        torch.cuda.synchronize(device)
        runs = [[] for _ in fns]
        for _ in range(args.repeats):
            for k, fn in enumerate(fns):
                runs[k].append(once(fn, inner[k]))
        return runs

    def numbers(v):
        return M._FILTER_CODE[v.dtype], tuple(int(n) for n in v.shape)

    def hist_launcher(v, tile, bins, shift, out):
        code, s = numbers(v)
        sides, _ = M.tile_grid(s, tile)
        return lambda: _ffi.check(_ffi.lib.sk_tile_histograms(_ffi.ptr(v), code, *s, *sides, bins, shift, _ffi.ptr(out), stream))

    def apply_launcher(v, dst, luts, tile, bins, shift, interpolate):
        code, s = numbers(v)
        sides, _ = M.tile_grid(s, tile)
        return lambda: _ffi.check(_ffi.lib.sk_apply_tile_luts(_ffi.ptr(v), _ffi.ptr(dst), code, *s, *sides, _ffi.ptr(luts), bins,
                                                              shift, int(interpolate), stream))

    def wide(v):
        return (v.view(torch.int16).to(torch.int32) & 0xFFFF) if v.dtype == torch.uint16 else v.to(torch.int32)

    def axis_tiles(n, t):
        return torch.arange(n, device=device) // t

    def torch_hist(v, tile, bins, shift):
        s = tuple(int(n) for n in v.shape)
        sides, counts = M.tile_grid(s, tile)
        kx, ky, kz = (axis_tiles(n, t) for n, t in zip(s, sides))

        def run():
            b = torch.clamp(wide(v) >> shift, max=bins - 1).to(torch.int64)
            key = ((kx[:, None, None] * counts[1] + ky[None, :, None]) * counts[2] + kz[None, None, :]) * bins + b
            return torch.bincount(key.reshape(-1), minlength=counts[0] * counts[1] * counts[2] * bins).view(*counts, bins)
        return run

    def torch_apply(v, luts, tile, bins, shift, interpolate):
        s = tuple(int(n) for n in v.shape)
        sides, counts = M.tile_grid(s, tile)
        pairs = [[torch.from_numpy(a).to(device) for a in M._axis_pairs(n, t, c, interpolate)] for n, t, c in zip(s, sides, counts)]
        table = luts.to(torch.int64)
        W = 8 * sides[0] * sides[1] * sides[2]

        def run():
            b = torch.clamp(wide(v) >> shift, max=bins - 1).to(torch.int64)
            if not interpolate:
                return table[pairs[0][0][:, None, None], pairs[1][0][None, :, None], pairs[2][0][None, None, :], b]
            S = torch.zeros(s, dtype=torch.int64, device=device)
            for cx in (0, 1):
                for cy in (0, 1):
                    for cz in (0, 1):
                        w = pairs[0][2 + cx][:, None, None] * pairs[1][2 + cy][None, :, None] * pairs[2][2 + cz][None, None, :]
                        S += w * table[pairs[0][cx][:, None, None], pairs[1][cy][None, :, None], pairs[2][cz][None, None, :], b]
            return (S + W // 2) // W
        return run

    def crop_of(image):
        cs = tuple(args.crop)
        bits = image.view(torch.int16) if image.dtype == torch.uint16 else image
        return bits[:cs[0], :cs[1], :cs[2]].contiguous().view(image.dtype)

    def hist_case(image, tile, bins, shift, with_stats):
        s = tuple(int(n) for n in image.shape)
        _, counts = M.tile_grid(s, tile)
        out = torch.empty(counts + (bins,), dtype=torch.int64, device=device)
        moved = image.numel() * image.element_size()
        half = torch.empty(moved // 2, dtype=torch.uint8, device=device).random_(0, 256)
        other = torch.empty_like(half)
        fns, inner, names = [hist_launcher(image, tile, bins, shift, out), lambda: other.copy_(half)], [args.inner] * 2, ["launch", "copy"]
        if with_stats:
            stats = torch.zeros(256, dtype=torch.int64, device=device)
            fns.append(lambda: _ffi.check(_ffi.lib.sk_u8_histogram(_ffi.ptr(image), image.numel(), _ffi.ptr(stats), stream)))
            inner.append(args.inner)
            names.append("u8_histogram")
        runs = alternating(fns, inner)
        row = {"tile": tile if tile is None or isinstance(tile, str) else list(tile), "grid": list(counts), "bins": bins,
               "shift": shift, "path": M.equalize_path(image.dtype, s, tile, bins, shift)[0]}
        for label, series in zip(names, runs):
            row[label] = spread(series, moved)
        row["over_copy"] = row["launch"]["median_s"] / row["copy"]["median_s"]
        if with_stats:
            row["over_u8_histogram"] = row["launch"]["median_s"] / row["u8_histogram"]["median_s"]
        del half, other
        crop = crop_of(image)
        cs = tuple(int(n) for n in crop.shape)
        crop_out = torch.empty(M.tile_grid(cs, tile)[1] + (bins,), dtype=torch.int64, device=device)
        reference = torch_hist(crop, tile, bins, shift)
        t_crop, t_ref = alternating((hist_launcher(crop, tile, bins, shift, crop_out), reference), (args.inner, 1))
        assert torch.equal(crop_out, reference())
        row["crop"] = list(cs)
        row["launch_crop"] = spread(t_crop)
        row["torch"] = spread(t_ref)
        row["over_torch"] = row["launch_crop"]["median_s"] / row["torch"]["median_s"]
        del crop, crop_out
        torch.cuda.empty_cache()
        return row

    def apply_case(image, tile, bins, shift, interpolate):
        s = tuple(int(n) for n in image.shape)
        _, counts = M.tile_grid(s, tile)
        top = 255 if image.dtype == torch.uint8 else 65535
        g = torch.Generator(device=device)
        g.manual_seed(31)
        luts = torch.randint(0, top + 1, counts + (bins,), generator=g, device=device, dtype=torch.int32)
        dst = torch.empty_like(image)
        moved = 2 * image.numel() * image.element_size()
        half = torch.empty(moved // 2, dtype=torch.uint8, device=device).random_(0, 256)
        other = torch.empty_like(half)
        runs = alternating([apply_launcher(image, dst, luts, tile, bins, shift, interpolate), lambda: other.copy_(half)],
                           [args.inner] * 2)
        row = {"tile": tile if tile is None or isinstance(tile, str) else list(tile), "grid": list(counts), "bins": bins,
               "shift": shift, "interpolate": interpolate, "path": M.equalize_path(image.dtype, s, tile, bins, shift, interpolate)[1]}
        row["launch"], row["copy"] = spread(runs[0], moved), spread(runs[1], moved)
        row["over_copy"] = row["launch"]["median_s"] / row["copy"]["median_s"]
        del half, other, dst
        crop = crop_of(image)
        cs = tuple(int(n) for n in crop.shape)
        crop_counts = M.tile_grid(cs, tile)[1]
        crop_luts = luts[:crop_counts[0], :crop_counts[1], :crop_counts[2]].contiguous()
        crop_dst = torch.empty_like(crop)
        reference = torch_apply(crop, crop_luts, tile, bins, shift, interpolate)
        t_crop, t_ref = alternating((apply_launcher(crop, crop_dst, crop_luts, tile, bins, shift, interpolate), reference),
                                    (args.inner, 1))
        assert torch.equal(wide(crop_dst).to(torch.int64), reference())
        row["crop"] = list(cs)
        row["launch_crop"] = spread(t_crop)
        row["torch"] = spread(t_ref)
        row["over_torch"] = row["launch_crop"]["median_s"] / row["torch"]["median_s"]
        del crop, crop_dst, crop_luts, luts
        torch.cuda.empty_cache()
        return row

    base = build_noise(tuple(args.shape), device)
    for dtype in args.dtypes:
        image = base if dtype == "uint8" else widen(base)
        bins, shift = (256, 0) if dtype == "uint8" else (1024, 6)
        entry = {"dtype": dtype, "histograms": {}, "apply": {}}
        for name, tile in TILINGS:
            entry["histograms"][name] = hist_case(image, tile, bins, shift, dtype == "uint8" and tile is None)
            print("histograms", name, dtype, f"{entry['histograms'][name]['launch']['median_s'] * 1e3:.3f} ms", file=sys.stderr, flush=True)
        const = torch.full_like(image.view(torch.int16) if dtype == "uint16" else image, 77).view(image.dtype)
        entry["histograms"]["one_tile_constant"] = hist_case(const, None, bins, shift, dtype == "uint8")
        del const
        for name, tile in TILINGS:
            entry["apply"][name] = apply_case(image, tile, bins, shift, True)
            print("apply", name, dtype, f"{entry['apply'][name]['launch']['median_s'] * 1e3:.3f} ms", file=sys.stderr, flush=True)
        report["volumes"].append(entry)
        del image
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
