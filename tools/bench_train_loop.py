#!/usr/bin/env python3
"""Measurements of the training command.

    python tools/bench_train_loop.py [--out profiles/train_loop_bench.json] [--tuning-lib PATH] [--repeats 5]

(a) ``sk_u8_histogram`` on a 1024 x 1024 x 64 uint8 volume (micrograph-like and constant contents) against what it
    replaces, on the same GPU in the same call, alternating: torch's ``x.sum(dtype=int64)`` plus
    ``(x.double() - mu).square().sum()``, and the reference's route of a device-to-host copy plus a host loop
    (``numpy.bincount`` stands in for numba).  ms, bytes over time against the HBM rate, peak extra device memory.
    With ``--tuning-lib`` (a ``make tuning`` build) the kernel's two ways of handling equal bytes in a wave are timed
    against each other (SK_HIST_VARIANT).
(b) one epoch of the default configuration (300 x 300 x 20, every augmentation at its default rate) through
    ``run_training``, batch 1 and 4, the volume on the device and on the host: wall time per sample against the sum of
    ``TransformFromCfg.forward`` + collate and of ``TrainStep.__call__`` timed on their own on the same samples.

Every clock read follows a device synchronise; every leg is warmed up; the repeats alternate the legs and the spread
(min / median / max over the repeats) is reported.  Prints one JSON line and writes it to ``--out``."""
import argparse
import ctypes as C
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_GBPS = 8000.0   # MI355X HBM3E peak, GB/s
DEV = "cuda:0"


def spread(values):
    return {"min": round(min(values), 4), "median": round(statistics.median(values), 4), "max": round(max(values), 4)}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def skewed_volume(shape, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = math.prod(shape)
    x = torch.randint(28, 34, (n // 64,), generator=g, device=DEV, dtype=torch.int32).repeat_interleave(64)
    bright = torch.rand(n // 16, generator=g, device=DEV).lt(0.06).repeat_interleave(16)
    x = torch.where(bright, torch.randint(150, 256, (n,), generator=g, device=DEV, dtype=torch.int32), x)
    return x.to(torch.uint8).reshape(shape)


def bench_histogram(args):
    from skoots_amd import _ffi
    shape = (1024, 1024, 64)
    n = math.prod(shape)
    hist = torch.zeros(256, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(DEV)
    libs = {"release": _ffi.lib.sk_u8_histogram}
    if args.tuning_lib:
        tuning = C.CDLL(args.tuning_lib)
        tuning.sk_u8_histogram.restype, tuning.sk_u8_histogram.argtypes = _ffi._SIGS["sk_u8_histogram"]
        libs["tuning"] = tuning.sk_u8_histogram
    out = {}
    for name, x in (("skewed", skewed_volume(shape)), ("constant", torch.full(shape, 37, dtype=torch.uint8, device=DEV))):
        mu = 88.5

        def hip(fn=libs["release"]):
            hist.zero_()
            _ffi.check(fn(_ffi.ptr(x), n, _ffi.ptr(hist), st))

        def via_torch():
            return x.sum(dtype=torch.int64), (x.double() - mu).square().sum()

        def via_host():
            return np.bincount(x.cpu().numpy().reshape(-1), minlength=256)

        legs = {"hip": (hip, 200), "torch": (via_torch, 10), "host": (via_host, 1)}
        if "tuning" in libs:
            for v, label in ((0, "tuning_copies"), (1, "tuning_match")):
                def variant(v=v):
                    os.environ["SK_HIST_VARIANT"] = str(v)
                    hip(libs["tuning"])
                legs[label] = (variant, 200)
        for fn, _ in legs.values():
            fn()                                   # warm-up
        hip()
        want = torch.bincount(x.reshape(-1).to(torch.int64), minlength=256)
        assert torch.equal(hist, want), "histogram differs from torch.bincount"
        times = {k: [] for k in legs}
        for _ in range(args.repeats):              # the legs alternate inside every repeat
            for k, (fn, iters) in legs.items():
                times[k].append(timed(fn, iters))
        res = {}
        for k, (fn, _) in legs.items():
            med = statistics.median(times[k])
            res[k] = {"ms": spread(times[k]), "GBps": round(n / med / 1e6, 1), "hbm_fraction": round(n / med / 1e6 / HBM_GBPS, 4),
                      "peak_extra_device_bytes": peak_extra(fn)}
        res["host"]["host_bytes"] = n
        out[name] = res
    return {"volume": list(shape), "bytes": n, "hbm_GBps_assumed": HBM_GBPS, **out}


def bench_epoch(args):
    from torch.utils.data.distributed import DistributedSampler
    from skoots_amd.config import get_cfg_defaults
    from skoots_amd.train import TrainStep, TrainUNet, TransformFromCfg, skeleton_colate
    from skoots_amd.train.dataloader import MultiDataset, dataset
    from skoots_amd.train.sigma import init_sigma
    from skoots_amd.train.trainer import Batches, run_training
    from skoots_amd.unet import random_state_dict
    cfg = get_cfg_defaults()
    cfg.TRAIN.NUM_EPOCHS, cfg.TRAIN.N_WARMUP = 1, 0
    X, Y, Z = 1024, 1024, 64
    gen = torch.Generator().manual_seed(0)
    image = torch.randint(0, 256, (1, X, Y, Z), generator=gen, dtype=torch.uint8)
    masks = torch.zeros((1, X, Y, Z), dtype=torch.int16)
    skeletons = {}
    for k in range(1, 41):
        c = [int(torch.randint(40, s - 40, (1,), generator=gen)) if s > 80 else s // 2 for s in (X, Y, Z)]
        masks[0, c[0] - 30:c[0] + 30, c[1] - 30:c[1] + 30, max(0, c[2] - 6):c[2] + 6] = k
        skeletons[k] = torch.stack([torch.linspace(c[0] - 25, c[0] + 25, 60), torch.full((60,), float(c[1])),
                                    torch.full((60,), float(c[2]))], 1)
    samples = args.samples
    step = TrainStep(TrainUNet(random_state_dict(), DEV, precision="bf16"))
    out = {}
    for where in ("device", "host"):
        for bs in (1, 4):
            cfg.TRAIN.TRAIN_BATCH_SIZE = bs
            t = TransformFromCfg(cfg, DEV).set_dataset_mean(127.0).set_dataset_std(70.0)
            ds = dataset([], transforms=t, device=DEV, sample_per_image=samples)
            ds.image, ds.masks, ds.skeletons, ds.baked_skeleton = [image], [masks], [skeletons], [None]
            ds.to(DEV if where == "device" else "cpu")
            multi = MultiDataset(ds)
            batches = Batches(multi, DistributedSampler(multi, num_replicas=1, rank=0), bs, skeleton_colate)
            sigma = init_sigma(cfg)
            kept = []

            def seed():
                random.seed(5)
                torch.manual_seed(5)

            def epoch():
                seed()
                run_training(step, batches, None, cfg, sigma)

            def transforms():
                seed()
                kept.clear()
                kept.extend(batches(0))

            def steps():
                for images, m, _, sk, baked in kept:
                    step(images, m, sk, baked, sigma(0), [1.0, 1.0, 0.0])

            transforms(), steps(), epoch()         # warm-up
            times = {"epoch": [], "transform": [], "step": []}
            for _ in range(args.repeats):
                times["epoch"].append(timed(epoch, 1) / samples)
                times["transform"].append(timed(transforms, 1) / samples)
                times["step"].append(timed(steps, 1) / samples)
            parts = statistics.median(times["transform"]) + statistics.median(times["step"])
            out[f"volume_{where}_batch{bs}"] = {
                "epoch_ms_per_sample": spread(times["epoch"]), "transform_ms_per_sample": spread(times["transform"]),
                "step_ms_per_sample": spread(times["step"]),
                "loop_overhead_ms_per_sample": round(statistics.median(times["epoch"]) - parts, 4)}
            kept.clear()
    return {"crop": [300, 300, 20], "samples_per_epoch": samples, "precision": "bf16", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tuning-lib", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--only", choices=("histogram", "epoch"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_loop needs the MI355X")
    line = {"metric": "train_loop", "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    if args.only != "epoch":
        line["histogram"] = bench_histogram(args)
    if args.only != "histogram":
        line["epoch"] = bench_epoch(args)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
