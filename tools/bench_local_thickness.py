#!/usr/bin/env python
"""Time the local thickness (``sk_local_thickness_paint``) on two int32 masks at spacing (1, 1, 3):

  * ``blobs``: the synthetic 512 x 512 x 128 mask of 1 000 ellipsoidal blobs of tools/bench_edt.py;
  * ``cells``: the (1024, 1024, 256) mask of 8 192 balls of tools/bench_clean.py.

Per mask: the centres (voxels whose ball holds more than itself), the box voxels they ask for -- the sum of the exact
clipped bounding boxes, which is what a launch is budgeted by; the kernel skips the (y, z) columns of a box that cannot
reach the ball, so it forms fewer distances than that -- the voxels the painting raised above their own distance, every
launch of the split centre list on its own (device events around the call), box voxels per second, the whole
``lib.morphology.local_thickness`` call with and without a given distance transform, and ``sk_label_edt`` alone.  The
atomics that the plain load avoids are not counted: that needs the ball memberships, which only the kernel forms.

Each mask is a step: a child process of its own under its own time limit, and a step that fails or runs out of time ends
the run.  It asserts no threshold.

    python tools/bench_local_thickness.py --out profiles/local_thickness_bench.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = ("blobs", "cells")


def exact_boxes(dist2, centres, w):
    """(n) int64: the clipped bounding box of every centre's open ball, half-extents by the kernel's exact rule"""
    import torch
    X, Y, Z = (int(v) for v in dist2.shape)
    D = dist2.reshape(-1)[centres]
    coords = (centres // (Y * Z), centres // Z % Y, centres % Z)
    boxes = torch.ones_like(centres)
    for wk, E, c in zip(w, (X, Y, Z), coords):
        h = torch.sqrt(D / wk).floor().clamp_(max=float(E))
        h = h + (wk * ((h + 1) * (h + 1)) < D).to(h.dtype)
        h = h - ((h > 0) & ~(wk * (h * h) < D)).to(h.dtype)
        h = h.to(torch.int64)
        boxes *= torch.clamp(c + h, max=E - 1) - torch.clamp(c - h, min=0) + 1
    return boxes


def measure(x, spacing, repeats, device):
    import torch

    from skoots_amd import _ffi
    from skoots_amd.lib import morphology as M
    from skoots_amd.validate import lib as VL
    from tools.bench_instance_stats import summary, timed
    rows = VL.id_rows(x)
    a, ids, _, _ = rows[1]
    X, Y, Z = (int(v) for v in a.shape)
    w = tuple(s * s for s in spacing)
    first = M.local_thickness(x, spacing, False, rows)                 # warm-up, and to compare
    dist2, row_max = first[1], first[2]
    centres, estimate = M.paint_centres(dist2, w)
    boxes = exact_boxes(dist2, centres, w)
    n = int(centres.numel())
    ends = torch.cumsum(estimate, 0)
    cuts, at, done = [0], 0, 0
    while at < n:                                                       # the split of lib.morphology.local_thickness
        last = max(int(torch.searchsorted(ends, done + M.PAINT_BUDGET, right=True).item()), at + 1)
        done, at = int(ends[last - 1].item()), last
        cuts.append(at)
    st = _ffi.stream_ptr(device)
    launches = [[] for _ in cuts[1:]]
    paint_s, whole_s, given_s, edt_s = [], [], [], []
    for rep in range(repeats + 1):                                      # the first turn warms every call up
        thick2 = dist2.clone()
        total = 0.0
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            _, s = timed(lambda: _ffi.check(_ffi.lib.sk_local_thickness_paint(
                _ffi.ptr(dist2), X, Y, Z, w[0], w[1], w[2], _ffi.ptr(centres[lo:hi]), hi - lo, _ffi.ptr(thick2), st)),
                device)
            total += s
            if rep:
                launches[k].append(s)
        _, e = timed(lambda: M.label_edt(x, spacing, False, rows), device)
        _, g = timed(lambda: M.local_thickness(x, spacing, False, rows, (dist2, row_max)), device)
        _, t = timed(lambda: M.local_thickness(x, spacing, False, rows), device)
        if rep:
            paint_s.append(total)
            edt_s.append(e)
            given_s.append(g)
            whole_s.append(t)
    tested = int(boxes.sum().item())
    res = {"shape": [X, Y, Z], "instances": int(ids.numel()), "spacing": list(spacing),
           "foreground_voxels": int((a > 0).sum().item()), "foreground_share": float((a > 0).sum().item() / (X * Y * Z)),
           "centres": n, "box_voxels": tested, "box_voxels_per_centre": tested / max(n, 1),
           "box_voxels_estimate_for_splitting": int(estimate.sum().item()), "paint_budget": int(M.PAINT_BUDGET),
           "largest_dist2": float(dist2[torch.isfinite(dist2)].max().item()),
           "voxels_raised_above_dist2": int((thick2 > dist2).sum().item()),
           "equals_first_run": bool(torch.equal(thick2.view(torch.int64), first[0].view(torch.int64))),
           "launches": [dict(summary(t), centres=hi - lo, box_voxels=int(boxes[lo:hi].sum().item()))
                        for t, lo, hi in zip(launches, cuts[:-1], cuts[1:])],
           "paint_all_launches": summary(paint_s), "sk_label_edt_open": summary(edt_s),
           "local_thickness_given_dist2": summary(given_s), "local_thickness_whole_call": summary(whole_s)}
    res["box_voxels_per_s_at_median"] = tested / res["paint_all_launches"]["median_s"]
    return res


def step(name, args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_thickness needs the GPU it measures")
    device = torch.device(args.device)
    if name == "blobs":
        from tools.bench_instance_stats import build_mask
        x = build_mask(tuple(args.shape), args.blobs, device)
    else:
        from tools.bench_clean import build_mask as build_cells
        x, _ = build_cells(tuple(args.big_shape), device)
    res = measure(x, tuple(args.spacing), args.repeats, device)
    res["device"] = torch.cuda.get_device_name(device)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 128))
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--big-shape", type=int, nargs=3, default=(1024, 1024, 256))
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 3.0))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step may take")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    report = {"repeats": args.repeats, "step_timeout_s": args.step_timeout}
    passed = [a for a in sys.argv[1:]]
    for name in STEPS:
        # a fresh child per step: the parent never opens the device, and a step that hangs is ended by its limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ["--step", name], capture_output=True,
                           text=True, timeout=args.step_timeout)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {name} failed with exit status {r.returncode}: nothing more is run")
        report[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
