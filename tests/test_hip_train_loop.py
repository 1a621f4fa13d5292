"""GPU tests of the training command: the dataset-statistics kernel, device-resident statistics, the loop against the
steps written out, the command's determinism, the chain labelled TIFFs -> skeletons -> training -> checkpoint ->
eval() through files, the default crop's step, and (two devices only) a two-rank run."""
import csv
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# -- 7. sk_u8_histogram -------------------------------------------------------------------------------------------------
def _hist(x, counters=None):
    from skoots_amd import _ffi
    h = torch.zeros(256, dtype=torch.int64, device=DEV) if counters is None else counters
    _ffi.check(_ffi.lib.sk_u8_histogram(_ffi.ptr(x), x.numel(), _ffi.ptr(h), _ffi.stream_ptr(DEV)))
    return h


def _bincount(x):
    return np.bincount(x.cpu().numpy().reshape(-1), minlength=256).astype(np.int64)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099, 300 * 300 * 20])
def test_histogram_random_bytes(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(DEV)
    assert np.array_equal(_hist(x).cpu().numpy(), _bincount(x))


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("n", [5, 4099, 1 << 20])
def test_histogram_unaligned_pointer(offset, n):
    g = torch.Generator().manual_seed(7 * n + offset)
    base = torch.randint(0, 256, (n + 64,), generator=g, dtype=torch.uint8).to(DEV)
    assert base.data_ptr() % 16 == 0
    x = base[offset:offset + n]
    assert x.data_ptr() % 16 == offset
    assert np.array_equal(_hist(x).cpu().numpy(), _bincount(x))


def test_histogram_constant_volume():
    """64 Mi bytes of one value: every lane of every wave on one counter."""
    x = torch.full((64 << 20,), 37, dtype=torch.uint8, device=DEV)
    want = np.zeros(256, dtype=np.int64)
    want[37] = 64 << 20
    assert np.array_equal(_hist(x).cpu().numpy(), want)


def skewed_volume(shape=(1024, 1024, 64), seed=3):
    """A micrograph-like volume: a dark background of a few grey values in long runs, some bright structures."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = math.prod(shape)
    coarse = torch.randint(28, 34, (n // 64,), generator=g, device=DEV, dtype=torch.int32)
    x = coarse.repeat_interleave(64)
    bright = torch.rand(n // 16, generator=g, device=DEV).lt(0.06).repeat_interleave(16)
    x = torch.where(bright, torch.randint(150, 256, (n,), generator=g, device=DEV, dtype=torch.int32), x)
    return x.to(torch.uint8).reshape(shape)


def test_histogram_skewed_volume_and_accumulation():
    x = skewed_volume()
    want = torch.bincount(x.reshape(-1).to(torch.int64), minlength=256).cpu().numpy()
    h = _hist(x)
    assert np.array_equal(h.cpu().numpy(), want) and want.sum() == x.numel()
    again = _hist(x)
    assert torch.equal(h, again)                                      # the same from run to run
    y = torch.randint(0, 256, (12345,), dtype=torch.uint8).to(DEV)
    _hist(y, counters=h)                                              # a second call adds into the same counters
    assert np.array_equal(h.cpu().numpy(), want + _bincount(y))


def test_histogram_refused_arguments_write_nothing():
    from skoots_amd import _ffi
    x = torch.zeros(64, dtype=torch.uint8, device=DEV)
    h = torch.full((257,), 7, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(DEV)
    odd = _ffi.vp(h.data_ptr() + 4)
    bad = [_ffi.lib.sk_u8_histogram(_ffi.ptr(x), 64, None, st),
           _ffi.lib.sk_u8_histogram(None, 64, _ffi.ptr(h), st),
           _ffi.lib.sk_u8_histogram(_ffi.ptr(x), -1, _ffi.ptr(h), st),
           _ffi.lib.sk_u8_histogram(_ffi.ptr(x), (1 << 40) + 1, _ffi.ptr(h), st),
           _ffi.lib.sk_u8_histogram(_ffi.ptr(x), 64, odd, st)]
    assert _ffi.lib.sk_u8_histogram(None, 0, _ffi.ptr(h), st) == 0     # nothing to add: accepted, nothing written
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad)
    assert "sk_u8_histogram" in _ffi.last_error()
    assert bool((h == 7).all())


# -- 8. device-resident statistics ----------------------------------------------------------------------------------------
def test_device_statistics_match_the_reference():
    from tests.test_train_loop import check_statistics, golden_datasets
    g, multi, sets = golden_datasets(DEV)
    assert all(im.is_cuda for s in sets for im in s.image)
    check_statistics(g, multi, sets)
    _, host, _ = golden_datasets("cpu")
    for flag in (False, True):
        assert multi.mean(flag) == host.mean(flag) and multi.std(flag) == host.std(flag)


# -- synthetic labelled volumes -------------------------------------------------------------------------------------------
def ellipsoid_volume(shape=(128, 120, 24), seed=0, pitch=32):
    """A seeded labelled volume: non-overlapping ellipsoids on a jittered grid as the instance mask (X, Y, Z) int32, the
    image uint8 bright inside them plus noise."""
    g = np.random.default_rng(seed)
    X, Y, Z = shape
    xs, ys, zs = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    labels = np.zeros(shape, dtype=np.int32)
    k = 0
    for cx in range(pitch // 2, X - pitch // 2 + 1, pitch):
        for cy in range(pitch // 2, Y - pitch // 2 + 1, pitch):
            k += 1
            c = (cx + g.integers(-3, 4), cy + g.integers(-3, 4), Z // 2 + g.integers(-2, 3))
            r = (g.uniform(8, 11), g.uniform(8, 11), g.uniform(3.5, 5))
            inside = ((xs - c[0]) / r[0]) ** 2 + ((ys - c[1]) / r[1]) ** 2 + ((zs - c[2]) / r[2]) ** 2 <= 1.0
            labels[inside] = k
    image = np.clip(np.rint(40 + 150 * (labels > 0) + g.normal(0, 10, size=shape)), 0, 255).astype(np.uint8)
    return image, labels


def memory_dataset(volumes, transform, sample_per_image, store):
    """A ``dataset`` holding the given (image, labels) volumes, with the centre line of every ellipsoid as its
    skeleton (no folder is read)."""
    from skoots_amd.train.dataloader import dataset
    ds = dataset([], transforms=transform, device=DEV, sample_per_image=sample_per_image)
    for image, labels in volumes:
        ds.image.append(torch.from_numpy(image)[None])
        ds.masks.append(torch.from_numpy(labels.astype(np.uint8))[None])
        skel = {}
        for k in range(1, int(labels.max()) + 1):
            pts = np.argwhere(labels == k).astype(np.float32)
            c = pts.mean(0)
            skel[k] = torch.tensor([[c[0] - 3, c[1], c[2]], [c[0], c[1], c[2]], [c[0] + 3, c[1], c[2]]]).round()
        ds.skeletons.append(skel)
        ds.baked_skeleton.append(None)
    return ds.to(store)


def small_cfg(save_path, **train):
    from skoots_amd.config import get_cfg_defaults, validate_cfg
    cfg = get_cfg_defaults()
    cfg.SYSTEM.NUM_GPUS = 1
    cfg.AUGMENTATION.CROP_WIDTH, cfg.AUGMENTATION.CROP_HEIGHT, cfg.AUGMENTATION.CROP_DEPTH = 16, 16, 8
    cfg.TRAIN.SAVE_PATH = str(save_path)
    for k, v in train.items():
        cfg.TRAIN[k] = v
    validate_cfg(cfg)
    return cfg


# -- 9. the loop is the steps ------------------------------------------------------------------------------------------------
def test_the_loop_is_the_steps(tmp_path):
    """Three epochs of run_training in fp32 == the same transform / collate / step calls written out here."""
    from torch.utils.data.distributed import DistributedSampler
    from skoots_amd.train import TrainStep, TrainUNet, TransformFromCfg, skeleton_colate
    from skoots_amd.train.dataloader import MultiDataset
    from skoots_amd.train.sigma import init_sigma
    from skoots_amd.train.trainer import Batches, run_training
    from skoots_amd.unet import random_state_dict

    base_lr, seed = 1e-3, 77
    cfg = small_cfg(tmp_path, NUM_EPOCHS=3, N_WARMUP=2, TRAIN_BATCH_SIZE=4, VALIDATE_EPOCH_SKIP=2, SCHEDULER_T0=2,
                    LEARNING_RATE=base_lr, INITIAL_SIGMA=[20.0, 20.0, 10.0], SIGMA_DECAY=[[0.5, 0]],
                    LOSS_EMBED_START_EPOCH=-1, LOSS_PROBABILITY_START_EPOCH=0, LOSS_SKELETON_START_EPOCH=1,
                    LOSS_EMBED_RELATIVE_WEIGHT=1.0, LOSS_PROBABILITY_RELATIVE_WEIGHT=2.0,
                    LOSS_SKELETON_RELATIVE_WEIGHT=0.5)
    vols = [ellipsoid_volume((64, 64, 16), seed=s) for s in (1, 2, 3, 4)]

    def build():
        random.seed(seed)
        torch.manual_seed(seed)
        t = TransformFromCfg(cfg, DEV).set_dataset_mean(90.0).set_dataset_std(60.0)
        train = MultiDataset(memory_dataset(vols[:2], t, 2, DEV), memory_dataset(vols[2:3], t, 2, "cpu"))   # 6 samples
        val = MultiDataset(memory_dataset(vols[3:], t, 3, DEV))                                             # 3 samples
        step = TrainStep(TrainUNet(random_state_dict(seed=seed), DEV, precision="fp32"), lr=base_lr)
        return t, train, val, step

    # (a) the loop
    t, train, val, step = build()
    hist = run_training(step, Batches(train, DistributedSampler(train, num_replicas=1, rank=0), 4, skeleton_colate),
                        Batches(val, DistributedSampler(val, num_replicas=1, rank=0), 4, skeleton_colate), cfg,
                        init_sigma(cfg))
    loop_param, loop_m, loop_v = step.model.flat_param.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone()
    loop_steps = step.step_count

    # (b) the steps, written out; the table of the CPU sequence test, for this configuration
    lr = [base_lr, base_lr * (1 + math.cos(math.pi * 1 / 2)) / 2, base_lr]          # T_0 = 2: restart at epoch 2
    sigma = [[20.0, 20.0, 10.0], [10.0, 10.0, 5.0], [10.0, 10.0, 5.0]]               # the decay at epoch 0 acts from 1
    weights = [[1.0, 0.0, 0.0], [1.0, 2.0, 0.0], [1.0, 2.0, 0.5]]                    # on from the epoch after the start
    t, train, val, step = build()

    def batch(ds, indices):
        return skeleton_colate([ds[i] for i in indices])

    def order(n, epoch):
        g = torch.Generator().manual_seed(epoch)
        return torch.randperm(n, generator=g).tolist()

    images, masks, _, skele_masks, baked = batch(train, order(6, 0)[:4])
    for _ in range(2):
        step(images, masks, skele_masks, baked, [20.0, 20.0, 10.0], [1.0, 2.0, 0.5])
    from statistics import mean
    want = {k: [9999999999.9999999999] for k in hist}
    for e in range(3):
        step.lr = lr[e]
        rows = []
        for lo in (0, 4):
            images, masks, _, skele_masks, baked = batch(train, order(6, e)[lo:lo + 4])
            rows.append(step(images, masks, skele_masks, baked, sigma[e], weights[e]).tolist())
        for k, col in zip(("avg_epoch_loss", "avg_epoch_embed_loss", "avg_epoch_prob_loss", "avg_epoch_skele_loss"),
                          (3, 0, 1, 2)):
            want[k].append(mean([rows[0][col], rows[1][col]]))
        if e % 2 == 0:
            images, masks, _, skele_masks, baked = batch(val, order(3, 0))
            row = step.evaluate(images, masks, skele_masks, baked, sigma[e], weights[e]).tolist()
            for k, col in zip(("avg_val_loss", "avg_val_embed_loss", "avg_val_prob_loss", "avg_val_skele_loss"),
                              (3, 0, 1, 2)):
                want[k].append(row[col])
    assert step.step_count == loop_steps == 2 + 3 * 2
    assert torch.equal(step.model.flat_param, loop_param)
    assert torch.equal(step.exp_avg, loop_m) and torch.equal(step.exp_avg_sq, loop_v)
    assert hist == want
    assert all(math.isfinite(v) for k in hist for v in hist[k])
    assert hist["avg_epoch_loss"][1] != hist["avg_epoch_loss"][3]


# -- 10 / 11. the command ------------------------------------------------------------------------------------------------
def _write_tif(path, stack):
    from PIL import Image
    pages = [Image.fromarray(p) for p in stack]
    pages[0].save(path, save_all=True, append_images=pages[1:])


def _child(args, timeout):
    """A child process under its own timeout; its exit status is checked and nothing is retried."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, timeout=timeout, capture_output=True, text=True)
    assert done.returncode == 0, f"{args}: exit {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}"
    return done


def training_folder(tmp_path, shape=(128, 120, 24)):
    """<tmp>/data/x.tif, x.labels.tif and the skeleton file the skeletonize command writes next to them."""
    data = tmp_path / "data"
    data.mkdir()
    image, labels = ellipsoid_volume(shape, seed=11)
    _write_tif(str(data / "x.tif"), np.ascontiguousarray(image.transpose(2, 0, 1)))
    _write_tif(str(data / "x.labels.tif"), np.ascontiguousarray(labels.transpose(2, 0, 1)).astype(np.uint16))
    _child(["-m", "skoots_amd", "--skeletonize-train-data", str(data)], timeout=300)
    assert os.path.exists(data / "x.labels.tif.skeletons.trch")
    return str(data), image, labels


def _yaml(path, data_dir, save_dir, epochs, crop=(32, 32, 16), rates=0.0, extra="", samples=1):
    path.write_text(f"""SYSTEM:
  NUM_GPUS: 1
TRAIN:
  TRAIN_DATA_DIR: ['{data_dir}']
  TRAIN_SAMPLE_PER_IMAGE: [{samples}]
  TRAIN_STORE_DATA_ON_GPU: [true]
  NUM_EPOCHS: {epochs}
  N_WARMUP: 0
  SAVE_PATH: '{save_dir}'
  SAVE_INTERVAL: 10
  LOSS_SKELETON_START_EPOCH: -1
  SIGMA_DECAY: []
  LEARNING_RATE: 0.001
{extra}AUGMENTATION:
  CROP_WIDTH: {crop[0]}
  CROP_HEIGHT: {crop[1]}
  CROP_DEPTH: {crop[2]}
  FLIP_RATE: {rates}
  BRIGHTNESS_RATE: {rates}
  NOISE_RATE: {rates}
  CONTRAST_RATE: {rates}
  AFFINE_RATE: {rates}
  ELASTIC_RATE: {rates}
""")
    return str(path)


def test_same_seed_same_run(tmp_path):
    """Two runs of the command with one seed write identical checkpoints; another seed gives other parameters."""
    from skoots_amd.train.__main__ import main
    data, _, _ = training_folder(tmp_path, shape=(96, 96, 16))
    out = []
    for name, seed in (("a", 5), ("b", 5), ("c", 6)):
        save = tmp_path / name
        save.mkdir()
        extra = f"  VALIDATION_DATA_DIR: ['{data}']\n  VALIDATION_SAMPLE_PER_IMAGE: [2]\n  VALIDATION_STORE_DATA_ON_GPU: [false]\n" \
                "  VALIDATE_EPOCH_SKIP: 2\n  TRAIN_BATCH_SIZE: 2\n"
        cfg = _yaml(save / "run.yaml", data, save, epochs=3, crop=(16, 16, 8), rates=0.5, extra=extra, samples=3)
        written = main(["--config-file", cfg, "--precision", "fp32", "--seed", str(seed)])
        assert written == [str(save / "run.trch")]
        out.append(torch.load(written[0], weights_only=True))
    a, b, c = out
    for k in a["model_state_dict"]:
        assert torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(a["optimizer_state_dict"][k], b["optimizer_state_dict"][k])
    from skoots_amd.train.trainer import HISTORY_KEYS
    assert all(a[k] == b[k] for k in HISTORY_KEYS) and len(a["avg_val_loss"]) == 3
    assert a["seed"] == 5 and c["seed"] == 6
    assert any(not torch.equal(a["model_state_dict"][k], c["model_state_dict"][k]) for k in a["model_state_dict"])


def test_end_to_end_through_files(tmp_path):
    """labelled TIFFs -> --skeletonize-train-data -> python -m skoots_amd.train -> checkpoint -> eval().  The last
    epoch's total loss must lie below the first's; both are printed (how far below is not fixed in advance)."""
    from skoots_amd.lib import zarr_store
    from skoots_amd.lib.eval import eval as sk_eval
    from skoots_amd.train.dataloader import MultiDataset, dataset
    from skoots_amd.train.trainer import HISTORY_KEYS
    data, image, labels = training_folder(tmp_path)
    save = tmp_path / "models"
    save.mkdir()
    epochs = 30
    cfg = _yaml(tmp_path / "e2e.yaml", data, save, epochs=epochs)
    _child(["-m", "skoots_amd.train", "--config-file", cfg, "--log", "1"], timeout=600)
    path = str(save / "e2e.trch")
    ck = torch.load(path, weights_only=True)
    for k in ("cfg", "model_state_dict", "optimizer_state_dict", "dataset_mean", "dataset_std", "epoch", "seed",
              "precision") + HISTORY_KEYS:
        assert k in ck, k
    assert ck["epoch"] == epochs and ck["precision"] == "bf16" and ck["seed"] == 101196
    assert ck["cfg"]["TRAIN"]["NUM_EPOCHS"] == epochs and ck["cfg"]["AUGMENTATION"]["CROP_WIDTH"] == 32
    assert all(len(ck[k]) == epochs + 1 for k in HISTORY_KEYS[:4]) and all(len(ck[k]) == 1 for k in HISTORY_KEYS[4:])
    own = MultiDataset(dataset(data))
    assert isinstance(ck["dataset_mean"], float) and isinstance(ck["dataset_std"], float)
    assert ck["dataset_mean"] == own.mean(with_invert=True) and ck["dataset_std"] == own.std(with_invert=True)
    rows = list(csv.reader(open(save / "e2e.csv")))
    assert len(rows) == epochs + 1 and [r[0] for r in rows[1:]] == [str(e) for e in range(epochs)]
    first, last = ck["avg_epoch_loss"][1], ck["avg_epoch_loss"][-1]
    print(f"end to end: total loss of epoch 0 = {first!r}, of epoch {epochs - 1} = {last!r}, ratio {last / first:.4f}")
    assert math.isfinite(first) and math.isfinite(last)
    assert last < first

    sk_eval(os.path.join(data, "x.tif"), path)
    base = os.path.join(data, "x")
    X, Y, Z = labels.shape
    assert zarr_store.load(base + "_skoots_skeleton.zarr").shape == (1, X, Y, Z)
    assert zarr_store.load(base + "_skoots_vectors.zarr").shape == (3, X, Y, Z)
    assert os.path.exists(base + "_skoots_benchmark.txt") and os.path.exists(base + "_instance_mask.tif")


# -- 12. the default crop --------------------------------------------------------------------------------------------------
def test_bf16_step_at_the_default_crop():
    """300 x 300 x 20 (the configuration's default crop), batch 2 and then batch 1 in the same TrainStep (the last
    batch of an epoch is smaller): finite losses, and a second run from the same state gives the same bits."""
    from skoots_amd.train import TrainStep, TrainUNet
    from skoots_amd.unet import random_state_dict
    X, Y, Z = 300, 300, 20
    g = torch.Generator().manual_seed(12)
    image, labels = ellipsoid_volume((X, Y, Z), seed=12, pitch=50)
    img = torch.from_numpy(image).float().sub(90.0).div(60.0)
    lab = torch.from_numpy(labels)
    images = torch.stack([img, img.flip(0)])[:, None].contiguous().to(DEV)
    masks = torch.stack([lab, lab.flip(0)])[:, None].contiguous().to(DEV)
    skele = (torch.rand((2, 1, X, Y, Z), generator=g) < 0.05).float().to(DEV) * (masks > 0)
    baked = (torch.rand((2, 3, X, Y, Z), generator=g) * torch.tensor([X, Y, Z]).view(1, 3, 1, 1, 1)).to(DEV)
    runs = []
    for _ in range(2):
        step = TrainStep(TrainUNet(random_state_dict(), DEV, precision="bf16"))
        l2 = step(images, masks, skele, baked, [20.0, 20.0, 20.0])
        l1 = step(images[:1], masks[:1], skele[:1], baked[:1], [20.0, 20.0, 20.0])
        torch.cuda.synchronize()
        print("300x300x20 bf16 step: batch 2", l2.tolist(), "batch 1", l1.tolist())
        assert torch.isfinite(l2).all() and torch.isfinite(l1).all()
        assert torch.isfinite(step.model.flat_param).all()
        runs.append((l2.clone(), l1.clone(), step.model.flat_param.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone()))
        del step
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# -- 13. two ranks ----------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, cfg_plain, out_dir):
    import torch.distributed as dist
    from skoots_amd.config import get_cfg_defaults, merge_cfg
    from skoots_amd.train.trainer import train
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
    try:
        train(merge_cfg(get_cfg_defaults(), cfg_plain), "fp32", 9, rank, world, "two",
              on_finish=lambda step: torch.save(step.model.flat_param.cpu(), os.path.join(out_dir, f"rank{rank}.pt")))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_two_ranks_end_with_identical_parameters(tmp_path):
    data, _, _ = training_folder(tmp_path, shape=(96, 96, 16))
    extra = "  TRAIN_BATCH_SIZE: 1\n"
    cfg = _yaml(tmp_path / "two.yaml", data, tmp_path, epochs=2, crop=(16, 16, 8), rates=0.5, extra=extra, samples=4)
    _child([os.path.abspath(__file__), cfg, str(tmp_path)], timeout=600)
    a, b = (torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert os.path.exists(tmp_path / "two.trch")


if __name__ == "__main__":   # the two-rank test's launcher: fresh processes, started before this one touches the GPU
    import socket
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    from skoots_amd.config import cfg_to_dict, load_cfg_from_file
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        free = s.getsockname()[1]
    mp.spawn(_two_rank_worker, args=(2, free, cfg_to_dict(load_cfg_from_file(sys.argv[1])), sys.argv[2]), nprocs=2,
             join=True)
