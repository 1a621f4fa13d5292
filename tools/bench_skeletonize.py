"""Time calculate_skeletons on a seeded ~1000-instance 256 x 256 x 64 label volume (isotropic and anisotropyZ = 3) and
print one JSON line: milliseconds per call (median of --reps), object count, largest crop, and the most passes and
re-check rounds any object needed (the thinning kernel's counters).  Each leg launches the thinning kernel
--reps + 2 times (a warm-up, the timed calls, one for the counters).

    python tools/bench_skeletonize.py [--reps 5] [--legs iso,z3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from skoots_amd.lib import morphology  # noqa: E402
from skoots_amd.train.generate_skeletons import _object_boxes, calculate_skeletons  # noqa: E402

LEGS = {"iso": (1.0, 1.0, 1.0), "z3": (1.0, 1.0, 3.0)}


def many_instances(seed=11, shape=(256, 256, 64), n=1000):
    """Seeded label volume: n boxes of half-widths 2-6 in x / y and 1-3 in z, later ones painted over earlier ones
    (the volume of tests/test_hip_skeletonize.py's one-launch test)."""
    rng = np.random.default_rng(seed)
    v = torch.zeros(shape, dtype=torch.int32)
    cx = rng.integers(0, shape[0], n)
    cy = rng.integers(0, shape[1], n)
    cz = rng.integers(0, shape[2], n)
    r = rng.integers(2, 7, (n, 3))
    for i in range(n):
        xs = slice(max(cx[i] - r[i, 0], 0), cx[i] + r[i, 0])
        ys = slice(max(cy[i] - r[i, 1], 0), cy[i] + r[i, 1])
        zs = slice(max(cz[i] - r[i, 2] // 2, 0), cz[i] + r[i, 2] // 2 + 1)
        v[xs, ys, zs] = i + 1
    return v


def _counters(lab):
    ids, lower, upper = _object_boxes(lab)
    ext = np.maximum(upper - lower, 1)
    boxes = np.concatenate([lower, lower + ext], 1)
    _, _, stats = morphology.thin_objects(lab, ids.cpu().numpy(), boxes)
    big = ext[np.argmax(ext.prod(1))]
    return {"objects": int(ids.numel()), "largest_crop": [int(v) for v in big],
            "max_passes": int(stats[:, 0].max()), "max_rounds": int(stats[:, 1].max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="iso,z3", help="comma-separated subset of " + ",".join(LEGS))
    args = ap.parse_args()
    lab = many_instances().to("cuda")
    out = {"volume": list(lab.shape)}
    for name in args.legs.split(","):
        scale = LEGS[name]
        calculate_skeletons(lab, torch.tensor(scale))   # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calculate_skeletons(lab, torch.tensor(scale))
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"{name}_ms"] = round(float(np.median(times)), 2)
        if name == "iso":
            out[name] = _counters(lab)
        else:
            size = torch.tensor(list(lab.shape)).mul(torch.tensor(scale)).float().round().int().tolist()
            large = torch.nn.functional.interpolate(lab[None, None].float(), size=size, mode="nearest")[0, 0].int()
            out[name] = _counters(large.contiguous())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
