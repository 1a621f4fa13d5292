"""CPU tests of the training command: configuration, learning-rate schedule, dataset discovery and layout, dataset
statistics against the reference's own (tests/golden/dataset_stats.npz), the loop's sequence with a recording stand-in
for the step, and the sampler's partition.  No GPU compute is called here."""
import csv
import json
import math
import os

import numpy as np
import pytest
import torch

from skoots_amd import config as C
from skoots_amd.train import dataloader as D
from skoots_amd.train import trainer as T
from skoots_amd.train.schedule import cosine_annealing_warm_restarts
from skoots_amd.train.sigma import init_sigma

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# -- 1. configuration -----------------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def test_defaults_equal_the_reference_tree():
    want = json.load(open(os.path.join(GOLDEN, "cfg_defaults.json")))
    got = _plain(C.get_cfg_defaults())
    assert sorted(got) == sorted(want) == ["AUGMENTATION", "EXPERIMENTAL", "MODEL", "SKOOTS", "SYSTEM", "TRAIN"]
    for section in want:
        assert sorted(got[section]) == sorted(want[section]), section
        for key, value in want[section].items():
            if (section, key) == ("TRAIN", "SAVE_PATH"):
                # the one permitted difference: the reference's default is its author's home directory
                assert got[section][key] == "."
                continue
            assert got[section][key] == value, (section, key)
            assert type(got[section][key]) is type(value), (section, key)


def test_attribute_and_dict_access_and_clone():
    cfg = C.get_cfg_defaults()
    assert cfg.TRAIN.N_WARMUP == cfg["TRAIN"]["N_WARMUP"] == 1500
    other = cfg.clone()
    other.TRAIN.N_WARMUP = 3
    assert cfg.TRAIN.N_WARMUP == 1500 and C.get_cfg_defaults().TRAIN.N_WARMUP == 1500
    from skoots_amd.train.transforms import _cfg_get
    assert _cfg_get(cfg, "AUGMENTATION", "CROP_DEPTH") == _cfg_get(C.cfg_to_dict(cfg), "AUGMENTATION", "CROP_DEPTH") == 20


def _write(tmp_path, text, name="c.yaml"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_yaml_override_and_merge_rules(tmp_path):
    cfg = C.load_cfg_from_file(_write(tmp_path, "TRAIN:\n  NUM_EPOCHS: 7\n  LEARNING_RATE: 1\n  INITIAL_SIGMA: [1.0, 2.0, 3.0]\n"
                                                "SKOOTS:\n  VECTOR_SCALING: [30, 30, 6]\n"))
    assert cfg.TRAIN.NUM_EPOCHS == 7
    assert cfg.TRAIN.LEARNING_RATE == 1.0 and isinstance(cfg.TRAIN.LEARNING_RATE, float)   # int -> float
    assert cfg.TRAIN.INITIAL_SIGMA == [1.0, 2.0, 3.0]
    assert cfg.SKOOTS.VECTOR_SCALING == (30, 30, 6)                                        # list -> tuple
    assert cfg.TRAIN.N_WARMUP == 1500
    with pytest.raises(KeyError, match="TRAIN.NUM_EPOCH"):
        C.load_cfg_from_file(_write(tmp_path, "TRAIN:\n  NUM_EPOCH: 7\n"))
    with pytest.raises(KeyError, match="TRAINING"):
        C.load_cfg_from_file(_write(tmp_path, "TRAINING:\n  NUM_EPOCHS: 7\n"))
    for bad in ("TRAIN:\n  NUM_EPOCHS: 7.5\n", "TRAIN:\n  NUM_EPOCHS: '7'\n", "TRAIN:\n  DISTRIBUTED: 1\n",
                "TRAIN:\n  N_WARMUP: true\n", "TRAIN:\n  INITIAL_SIGMA: 3.0\n", "TRAIN:\n  OPTIMIZER: 3\n", "TRAIN: 3\n"):
        with pytest.raises(ValueError):
            C.load_cfg_from_file(_write(tmp_path, bad))
    with pytest.raises(ValueError, match="Could not find"):
        C.load_cfg_from_file(str(tmp_path / "absent.yaml"))


@pytest.mark.parametrize("section,key,value,match", [
    ("MODEL", "DEPTHS", [2, 2, 2], "MODEL.DIMS"),
    ("MODEL", "IN_CHANNELS", 3, "MODEL.IN_CHANNELS"),
    ("TRAIN", "TARGET", "bism", "TRAIN.TARGET"),
    ("TRAIN", "LOSS_EMBED_VALUES", [0.25, 0.75], "LOSS_EMBED_KEYWORDS"),
    ("TRAIN", "LOSS_PROBABILITY_KEYWORDS", ["alpha"], "LOSS_PROBABILITY_KEYWORDS"),
    ("TRAIN", "LOSS_SKELETON_VALUES", [], "LOSS_SKELETON_KEYWORDS"),
    ("TRAIN", "LOSS_EMBED_RELATIVE_WEIGHT", -1.0, "LOSS_EMBED_RELATIVE_WEIGHT"),
    ("TRAIN", "LOSS_PROBABILITY_RELATIVE_WEIGHT", -0.5, "LOSS_PROBABILITY_RELATIVE_WEIGHT"),
    ("TRAIN", "LOSS_SKELETON_RELATIVE_WEIGHT", -2.0, "LOSS_SKELETON_RELATIVE_WEIGHT"),
    ("TRAIN", "TRAIN_DATA_DIR", ["a"], "TRAIN_DATA_DIR"),
    ("TRAIN", "VALIDATION_SAMPLE_PER_IMAGE", [1], "VALIDATION_DATA_DIR"),
    ("TRAIN", "BACKGROUND_STORE_DATA_ON_GPU", [True], "BACKGROUND_DATA_DIR"),
    ("TRAIN", "OPTIMIZER_KEYWORD_VALUES", [[0.9, 0.99]], "OPTIMIZER_KEYWORD_ARGUMENTS"),
    ("TRAIN", "TRAIN_BATCH_SIZE", 0, "TRAIN_BATCH_SIZE"),
    ("TRAIN", "VALIDATION_BATCH_SIZE", 0, "VALIDATION_BATCH_SIZE"),
    ("TRAIN", "VALIDATE_EPOCH_SKIP", 0, "VALIDATE_EPOCH_SKIP"),
    ("TRAIN", "SAVE_PATH", "/no/such/folder/anywhere", "SAVE_PATH"),
    ("TRAIN", "PRETRAINED_MODEL_PATH", ["/no/such/model.trch"], "PRETRAINED_MODEL_PATH"),
    ("TRAIN", "OPTIMIZER", "sgd", "not supported"),
    ("TRAIN", "SCHEDULER", "step", "not supported"),
    ("EXPERIMENTAL", "IS_SPARSE", True, "not supported"),
    ("TRAIN", "TRANSFORM_DEVICE", "cpu", "not supported"),
    ("TRAIN", "DATALOADER_OUTPUT_DEVICE", "cpu", "not supported"),
    ("TRAIN", "DATALOADER_NUM_WORKERS", 2, "not supported"),
])
def test_validate_cfg_rules(section, key, value, match):
    cfg = C.get_cfg_defaults()
    C.validate_cfg(cfg)
    cfg[section][key] = value
    with pytest.raises(ValueError, match=match):
        C.validate_cfg(cfg)


def test_background_data_is_refused():
    cfg = C.get_cfg_defaults()
    cfg.TRAIN.BACKGROUND_DATA_DIR, cfg.TRAIN.BACKGROUND_SAMPLE_PER_IMAGE, cfg.TRAIN.BACKGROUND_STORE_DATA_ON_GPU = ["x"], [1], [0]
    with pytest.raises(ValueError, match="BACKGROUND_DATA_DIR is not supported"):
        C.validate_cfg(cfg)


def test_cfg_to_dict_survives_weights_only_load(tmp_path):
    cfg = C.get_cfg_defaults()
    plain = C.cfg_to_dict(cfg)
    path = str(tmp_path / "c.trch")
    torch.save({"cfg": plain}, path)
    back = torch.load(path, weights_only=True)["cfg"]
    assert back == plain and type(back["TRAIN"]) is dict and back["SKOOTS"]["VECTOR_SCALING"] == [60, 60, 12]
    assert C.merge_cfg(C.get_cfg_defaults(), back) == cfg


# -- 2. learning rate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_0", [1, 3, 10001])
def test_cosine_annealing_warm_restarts_is_torchs(T_0):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=5e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=T_0)
    for epoch in range(25):
        want = opt.param_groups[0]["lr"]
        got = cosine_annealing_warm_restarts(5e-4, T_0, epoch)
        assert abs(got - want) <= 1e-12 * abs(want), (epoch, got, want)
        opt.step()
        sched.step()


def test_cosine_annealing_with_t_mult_and_eta_min():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2, eta_min=1e-5)
    for epoch in range(20):
        want = opt.param_groups[0]["lr"]
        assert abs(cosine_annealing_warm_restarts(1e-3, 2, epoch, 1e-5, 2) - want) <= 1e-12 * want
        opt.step()
        sched.step()


# -- 3. dataset discovery and layout -------------------------------------------------------------------------------------
def _save_tif(path, stack):
    from PIL import Image
    pages = [Image.fromarray(p) for p in stack]
    pages[0].save(path, save_all=True, append_images=pages[1:])


def _make_volume(folder, name, shape_zxy=(4, 9, 7), max_id=3, channels=None, seed=0, skeletons="base"):
    g = np.random.default_rng(seed)
    z, x, y = shape_zxy
    image = g.integers(0, 256, size=shape_zxy if channels is None else shape_zxy + (channels,), dtype=np.uint8)
    ids = np.zeros(shape_zxy, dtype=np.int32)
    ids[:, :3, :3] = 1
    ids[:, 4:, 4:] = max_id
    _save_tif(os.path.join(folder, name + ".tif"), image)
    _save_tif(os.path.join(folder, name + ".labels.tif"), ids.astype(np.uint16) if max_id < 65536 else ids)
    skel = {1: torch.tensor([[1.0, 1.0, 2.0]]), max_id: torch.tensor([[6.0, 5.0, 1.0], [7.0, 5.0, 1.0]])}
    if skeletons == "base":
        torch.save(skel, os.path.join(folder, name + ".skeletons.trch"))
    elif skeletons == "labels":
        torch.save(skel, os.path.join(folder, name + ".labels.tif.skeletons.trch"))
    return image, ids


def test_dataset_discovery_and_layout(tmp_path):
    a = tmp_path / "a"
    a.mkdir()
    img0, ids0 = _make_volume(str(a), "v0", max_id=3, seed=1)
    img1, ids1 = _make_volume(str(a), "v1", max_id=300, seed=2, skeletons="labels")
    img2, ids2 = _make_volume(str(a), "v2", max_id=40000, seed=3)
    img3, _ = _make_volume(str(a), "v3", channels=4, seed=4)
    img4, _ = _make_volume(str(a), "v4", channels=3, seed=5)
    seen = []

    def transform(dd):
        seen.append(dd["image"])
        return dd

    ds = D.dataset(str(a), transforms=transform, sample_per_image=3)
    assert [os.path.basename(f) for f in ds.files] == [f"v{i}.labels.tif" for i in range(5)]
    assert len(ds) == 15
    assert [tuple(m.shape) for m in ds.masks] == [(1, 9, 7, 4)] * 5
    assert [m.dtype for m in ds.masks[:3]] == [torch.uint8, torch.int16, torch.int32]
    assert torch.equal(ds.masks[2][0], torch.from_numpy(ids2.transpose(1, 2, 0)))
    assert [tuple(i.shape) for i in ds.image] == [(1, 9, 7, 4)] * 4 + [(3, 9, 7, 4)]
    assert all(i.dtype == torch.uint8 for i in ds.image)
    assert torch.equal(ds.image[0][0], torch.from_numpy(img0.transpose(1, 2, 0)))
    assert torch.equal(ds.image[3][0], torch.from_numpy(img3[..., 2].transpose(1, 2, 0)))   # channel 2 when C > 3
    assert torch.equal(ds.image[4], torch.from_numpy(img4.transpose(3, 1, 2, 0)))
    assert sorted(ds.skeletons[1]) == [1, 300]
    item = ds[7]                                                                               # 7 // 3 = volume 2
    assert item["image"] is seen[-1] and torch.equal(item["masks"], ds.masks[2]) and sorted(item["skeletons"]) == [1, 40000]
    assert item["baked_skeleton"] is None

    b = tmp_path / "b"
    b.mkdir()
    _make_volume(str(b), "w0", seed=6)
    other = D.dataset([str(b)], sample_per_image=2)
    multi = D.MultiDataset(ds, other, "not a dataset")
    assert len(multi) == 17 and multi.num_datasets == 2
    assert torch.equal(multi[14]["image"], ds.image[4]) and torch.equal(multi[15]["image"], other.image[0])
    assert torch.equal(multi[16]["image"], other.image[0])
    with pytest.raises(IndexError):
        multi[17]
    from skoots_amd.train.transforms import skeleton_colate
    assert D.skeleton_colate is skeleton_colate


def test_dataset_error_cases(tmp_path):
    _make_volume(str(tmp_path), "v0")
    os.remove(tmp_path / "v0.tif")
    with pytest.raises(FileNotFoundError, match="v0.tif"):
        D.dataset(str(tmp_path))
    _make_volume(str(tmp_path), "v0", skeletons=None)
    os.remove(tmp_path / "v0.skeletons.trch")
    with pytest.raises(FileNotFoundError, match="skeleton file for.*v0.labels.tif"):
        D.dataset(str(tmp_path))
    torch.save({1: torch.zeros((1, 3)), 3: torch.zeros((0, 3))}, tmp_path / "v0.skeletons.trch")
    with pytest.raises(ValueError, match="v0.labels.tif instance label 3"):
        D.dataset(str(tmp_path))
    torch.save({1: torch.zeros((1, 3))}, tmp_path / "v0.skeletons.trch")
    _save_tif(str(tmp_path / "v0.tif"), np.zeros((4, 9, 7), dtype=np.uint16))
    with pytest.raises(ValueError, match="8bit"):
        D.dataset(str(tmp_path))


# -- 4. statistics ----------------------------------------------------------------------------------------------------
def golden_datasets(device="cpu"):
    """The datasets of tests/golden/dataset_stats.npz, built without reading a folder."""
    g = np.load(os.path.join(GOLDEN, "dataset_stats.npz"))
    sets = []
    for d, n in enumerate(g["layout"].tolist()):
        ds = D.dataset([])
        ds.image = [torch.from_numpy(g[f"v{d}_{i}"]).to(device) for i in range(n)]
        sets.append(ds)
    return g, D.MultiDataset(*sets), sets


def check_statistics(g, multi, sets):
    for flag in (False, True):
        t = int(flag)
        assert multi.sum(with_invert=flag) == int(g[f"sum_{t}"])
        assert multi.numel(with_invert=flag) == int(g[f"numel_{t}"])
        assert [s.sum(with_invert=flag) for s in sets] == g[f"ds_sum_{t}"].tolist()
        assert [s.numel(with_invert=flag) for s in sets] == g[f"ds_numel_{t}"].tolist()
        mean = multi.mean(with_invert=flag)
        assert isinstance(mean, float) and np.float32(mean) == g[f"mean_{t}"] and float(np.float32(mean)) == mean
        std = multi.std(with_invert=flag)
        print(f"with_invert={flag}: mean {mean!r} std {std!r} (reference {float(g[f'std_{t}'])!r})")
        assert abs(std - float(g[f"std_{t}"])) <= 1e-10 * float(g[f"std_{t}"])
    for k, other in enumerate(g["others"].tolist()):
        for s, want in zip(sets, g["ds_sss"][:, k].tolist()):
            assert abs(s.subtract_square_sum(other) - want) <= 1e-10 * want
        assert abs(sum(s.subtract_square_sum(other) for s in sets) - float(g["sss"][k])) <= 1e-10 * float(g["sss"][k])


def test_host_statistics_match_the_reference():
    check_statistics(*golden_datasets("cpu"))


def test_statistics_quirks_are_the_reference_s():
    g, multi, sets = golden_datasets("cpu")
    vols = [[g[f"v{d}_{i}"].astype(np.int64) for i in range(n)] for d, n in enumerate(g["layout"].tolist())]
    plain = sum(int(v.sum()) for group in vols for v in group)
    last_only = plain + sum(int((255 - group[-1]).sum()) for group in vols)
    every = plain + sum(int((255 - v).sum()) for group in vols for v in group)
    assert multi.sum(with_invert=True) == last_only != every            # the inverted sum of the last image only
    n = sum(v.size for group in vols for v in group)
    assert multi.numel(with_invert=True) == 2 * n                        # ... over the doubled count of all images
    mean = multi.mean(with_invert=True)
    assert mean == float(np.float32(last_only) / np.float32(2 * n)) != last_only / (2 * n)   # fp32, not float64
    sq = sum(float(((v - mean) ** 2).sum()) for group in vols for v in group)
    assert abs(multi.std(with_invert=True) - math.sqrt(sq / (2 * n))) <= 1e-12 * multi.std(with_invert=True)
    # dataset.std as written: the numerator squared
    d0 = sets[0]
    assert d0.std() == math.sqrt(d0.subtract_square_sum(d0.mean()) ** 2 / d0.numel())


def test_empty_multidataset_gives_none():
    for multi in (D.MultiDataset(), D.MultiDataset(D.dataset([]))):
        assert len(multi) == 0
        for flag in (False, True):
            assert multi.sum(flag) is None and multi.numel(flag) is None and multi.mean(flag) is None
            assert multi.std(flag) is None


def test_histogram_is_cached_and_reset_by_map():
    _, _, sets = golden_datasets("cpu")
    ds = sets[2]
    h = ds.histogram(1)
    assert h is ds.histogram(1) and h.dtype == np.int64 and h.sum() == ds.image[1].numel()
    before = ds.sum()
    ds.map(lambda x: x * 0, "image")
    assert ds.sum() == 0 != before
    with pytest.raises(ValueError, match="invalid"):
        ds.map(lambda x: x, "background")


# -- 5. the sequence -------------------------------------------------------------------------------------------------
class _Items(torch.utils.data.Dataset):
    """Sample i is its own index in every tensor, so that a batch shows which samples it holds."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        one = torch.full((1, 1, 1, 1), float(i))
        return {"image": one.clone(), "masks": one.clone().int(), "skele_masks": one.clone(),
                "baked_skeleton": one.expand(3, 1, 1, 1).clone(), "skeletons": {1: torch.zeros((1, 3))}}


class RecordingStep:
    """Stands in for TrainStep: records every call, returns losses that encode the call number."""

    def __init__(self):
        self.lr = None
        self.calls = []

    def _record(self, kind, images, masks, skele_masks, baked, sigma, weights):
        assert images.shape[1:] == (1, 1, 1, 1) and baked.shape[1:] == (3, 1, 1, 1)
        assert torch.equal(images.flatten(), skele_masks.flatten()) and torch.equal(images.flatten().int(), masks.flatten())
        n = len(self.calls)
        self.calls.append((kind, [int(v) for v in images.flatten().tolist()], self.lr, list(sigma), list(weights)))
        return torch.tensor([n + 0.25, n + 0.5, n + 0.75, float(n)])

    def __call__(self, images, masks, skele_masks, baked, sigma, weights):
        return self._record("train", images, masks, skele_masks, baked, sigma, weights)

    def evaluate(self, images, masks, skele_masks, baked, sigma, weights):
        return self._record("validate", images, masks, skele_masks, baked, sigma, weights)

    def checkpoint(self, cfg):
        return {"cfg": cfg, "model_state_dict": {"w": torch.tensor([float(len(self.calls))])},
                "optimizer_state_dict": {"step": len(self.calls)}}


def _sequence_cfg(tmp_path):
    cfg = C.get_cfg_defaults()
    t = cfg.TRAIN
    t.NUM_EPOCHS, t.N_WARMUP, t.VALIDATE_EPOCH_SKIP, t.SCHEDULER_T0, t.TRAIN_BATCH_SIZE = 6, 2, 2, 4, 2
    t.VALIDATION_BATCH_SIZE = 1                       # not used: validation batches take TRAIN_BATCH_SIZE
    t.LOSS_EMBED_START_EPOCH, t.LOSS_PROBABILITY_START_EPOCH, t.LOSS_SKELETON_START_EPOCH = -1, 0, 2
    t.LOSS_EMBED_RELATIVE_WEIGHT, t.LOSS_PROBABILITY_RELATIVE_WEIGHT, t.LOSS_SKELETON_RELATIVE_WEIGHT = 1.0, 2.0, 0.5
    t.LEARNING_RATE, t.INITIAL_SIGMA, t.SIGMA_DECAY = 1e-3, [20.0, 20.0, 10.0], [[0.5, 1], [0.5, 3]]
    t.SAVE_INTERVAL, t.SAVE_PATH = 4, str(tmp_path)
    C.validate_cfg(cfg)
    return cfg


def _sources(cfg, n_train=5, n_val=3):
    from torch.utils.data.distributed import DistributedSampler
    from skoots_amd.train.transforms import skeleton_colate
    tr, va = _Items(n_train), _Items(n_val)
    bs = cfg.TRAIN.TRAIN_BATCH_SIZE
    return (T.Batches(tr, DistributedSampler(tr, num_replicas=1, rank=0), bs, skeleton_colate),
            T.Batches(va, DistributedSampler(va, num_replicas=1, rank=0), bs, skeleton_colate))


# DistributedSampler(range(5), num_replicas=1, rank=0), shuffle with seed 0 + epoch
ORDER = {0: [4, 0, 1, 3, 2], 1: [0, 4, 2, 3, 1], 2: [3, 4, 1, 0, 2], 3: [1, 0, 3, 4, 2], 4: [0, 3, 1, 4, 2], 5: [1, 3, 0, 4, 2]}
VAL_ORDER = [2, 0, 1]                                  # the validation sampler never gets set_epoch
LR = {0: 1e-3, 1: 1e-3 * (1 + math.cos(math.pi / 4)) / 2, 2: 1e-3 * (1 + math.cos(math.pi / 2)) / 2,
      3: 1e-3 * (1 + math.cos(3 * math.pi / 4)) / 2, 4: 1e-3, 5: 1e-3 * (1 + math.cos(math.pi / 4)) / 2}
SIGMA = {0: [20.0, 20.0, 10.0], 1: [20.0, 20.0, 10.0], 2: [10.0, 10.0, 5.0], 3: [10.0, 10.0, 5.0], 4: [5.0, 5.0, 2.5],
         5: [5.0, 5.0, 2.5]}                           # a multiplier applies from the epoch AFTER its own
WEIGHTS = {0: [1.0, 0.0, 0.0], 1: [1.0, 2.0, 0.0], 2: [1.0, 2.0, 0.0], 3: [1.0, 2.0, 0.5], 4: [1.0, 2.0, 0.5],
           5: [1.0, 2.0, 0.5]}                         # a term is on from the epoch AFTER its start epoch


def expected_calls(epochs=6):
    table = [("train", ORDER[0][:2], 1e-3, SIGMA[0], [1.0, 2.0, 0.5])] * 2          # warm-up: first batch, no gates
    for e in range(epochs):
        for i in range(0, 5, 2):
            table.append(("train", ORDER[e][i:i + 2], LR[e], SIGMA[e], WEIGHTS[e]))
        if e % 2 == 0:
            for i in range(0, 3, 2):
                table.append(("validate", VAL_ORDER[i:i + 2], LR[e], SIGMA[e], WEIGHTS[e]))
    return table


def _same_calls(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and g[3] == w[3] and g[4] == w[4], (n, g, w)
        assert abs(g[2] - w[2]) <= 1e-15, (n, g, w)


def test_the_sequence_of_calls(tmp_path):
    cfg = _sequence_cfg(tmp_path)
    step = RecordingStep()
    train_b, val_b = _sources(cfg)
    save, rows = str(tmp_path / "run.trch"), str(tmp_path / "run.csv")
    saves = []
    real = T.save_checkpoint

    def spy(path, payload):
        saves.append((payload["epoch"], payload["optimizer_state_dict"]["step"]))
        real(path, payload)

    T.save_checkpoint = spy
    try:
        hist = T.run_training(step, train_b, val_b, cfg, init_sigma(cfg), save_path=save, csv_path=rows,
                              extra={"dataset_mean": 1.5, "dataset_std": 2.5, "seed": 3, "precision": "fp32"})
    finally:
        T.save_checkpoint = real
    _same_calls(step.calls, expected_calls())
    # histories: the sentinel, then one value per (validated) epoch; the means are over the batches in order
    for k in T.HISTORY_KEYS:
        assert hist[k][0] == 9999999999.9999999999
    assert all(len(hist[k]) == 7 for k in T.HISTORY_KEYS[:4]) and all(len(hist[k]) == 4 for k in T.HISTORY_KEYS[4:])
    assert hist["avg_epoch_loss"][1] == (2 + 3 + 4) / 3 and hist["avg_epoch_embed_loss"][1] == (2.25 + 3.25 + 4.25) / 3
    assert hist["avg_epoch_prob_loss"][1] == 3.5 and hist["avg_epoch_skele_loss"][1] == 3.75
    assert hist["avg_val_loss"][1] == (5 + 6) / 2 and hist["avg_val_skele_loss"][1] == 6.25
    # saved at the interval (after 4 epochs) and at the end
    assert saves == [(4, 2 + 4 * 3 + 2 * 2), (6, len(step.calls))]
    ck = torch.load(save, weights_only=True)
    assert ck["epoch"] == 6 and ck["dataset_mean"] == 1.5 and ck["dataset_std"] == 2.5 and ck["seed"] == 3
    assert ck["precision"] == "fp32" and ck["cfg"] == C.cfg_to_dict(cfg)
    assert all(ck[k] == hist[k] for k in T.HISTORY_KEYS)
    assert not os.path.exists(save + ".tmp")
    table = list(csv.reader(open(rows)))
    assert table[0] == list(T.CSV_COLUMNS) and len(table) == 7
    assert [r[0] for r in table[1:]] == [str(e) for e in range(6)]
    assert table[2][9:] == ["", "", "", ""] and float(table[1][9]) == 5.5 and float(table[3][2]) == 10.0


def test_not_distributed_never_sets_the_epoch(tmp_path):
    cfg = _sequence_cfg(tmp_path)
    cfg.TRAIN.DISTRIBUTED, cfg.TRAIN.NUM_EPOCHS = False, 2
    step = RecordingStep()
    train_b, _ = _sources(cfg)
    hist = T.run_training(step, train_b, None, cfg, init_sigma(cfg))
    assert [c[1] for c in step.calls[2:]] == [ORDER[0][i:i + 2] for i in (0, 2, 4)] * 2
    assert all(c[0] == "train" for c in step.calls) and len(hist["avg_val_loss"]) == 1


def test_empty_validation_set_is_skipped(tmp_path):
    cfg = _sequence_cfg(tmp_path)
    step = RecordingStep()
    train_b, val_b = _sources(cfg, n_val=0)
    hist = T.run_training(step, train_b, val_b, cfg, init_sigma(cfg))
    assert all(c[0] == "train" for c in step.calls) and hist["avg_val_loss"] == [T.SENTINEL]


class _FailingStep(RecordingStep):
    def __init__(self, fail_at_call):
        super().__init__()
        self.fail_at_call = fail_at_call

    def __call__(self, *args):
        if len(self.calls) == self.fail_at_call:
            raise RuntimeError("the stand-in fails here")
        return self._record("train", *args)


def test_checkpoint_after_an_exception(tmp_path):
    cfg = _sequence_cfg(tmp_path)
    # calls before epoch 3: 2 warm-up + epochs 0..2 (3 + 2, 3, 3 + 2) = 15; fail at the second batch of epoch 3
    step = _FailingStep(fail_at_call=16)
    train_b, val_b = _sources(cfg)
    save = str(tmp_path / "run.trch")
    with pytest.raises(RuntimeError, match="the stand-in fails here"):
        T.run_training(step, train_b, val_b, cfg, init_sigma(cfg), save_path=save, csv_path=str(tmp_path / "run.csv"))
    ck = torch.load(save, weights_only=True)
    assert ck["epoch"] == 3                                   # the state after epoch 2
    assert len(ck["avg_epoch_loss"]) == 4 and len(ck["avg_val_loss"]) == 3
    _same_calls(step.calls, expected_calls()[:16])
    assert len(list(csv.reader(open(tmp_path / "run.csv")))) == 4


def test_validation_skeleton_term_uses_the_probability_loss(monkeypatch):
    """engine.py:571 of the reference: ``_loss_skeleton = loss_prob(predicted_skeleton, ...)`` in the validation pass."""
    from skoots_amd.train import engine as E
    seen = {}

    class Model:
        released = False

        def forward(self, images):
            return "logits"

        def release(self):
            self.released = True

    def fake_fused_loss(logits, masks, skele_masks, baked, sigma, vector_scale, loss_params, weights, need_grad=True):
        seen.update(logits=logits, loss_params=loss_params, weights=list(weights), need_grad=need_grad, sigma=list(sigma))
        return torch.zeros(4), None

    monkeypatch.setattr(E, "fused_loss", fake_fused_loss)
    step = object.__new__(E.TrainStep)
    step.model, step.vector_scale, step.weights = Model(), [60.0, 60.0, 12.0], [1.0, 1.0, 1.0]
    step.loss_params = [[0.25, 0.75, 1e-8], [0.5, 0.5, 1e-8], [0.5, 1.5, 1e-8]]
    step.evaluate(None, None, None, None, (3.0, 2.0, 1.0), [1.0, 2.0, 0.0])
    assert seen["loss_params"] == [[0.25, 0.75, 1e-8], [0.5, 0.5, 1e-8], [0.5, 0.5, 1e-8]]
    assert seen["need_grad"] is False and seen["weights"] == [1.0, 2.0, 0.0] and seen["sigma"] == [3.0, 2.0, 1.0]
    assert step.model.released and step.loss_params[2] == [0.5, 1.5, 1e-8]


# -- 6. the sampler's partition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", [None, 1])
def test_two_ranks_partition_as_torchs_sampler(epoch):
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from skoots_amd.train.transforms import skeleton_colate
    ds = _Items(5)
    want = {(None, 0): [4, 1, 2], (None, 1): [0, 3, 4], (1, 0): [0, 2, 1], (1, 1): [4, 3, 0]}
    for rank in range(2):
        ours = T.Batches(ds, DistributedSampler(ds, num_replicas=2, rank=rank), 2, skeleton_colate)
        theirs_sampler = DistributedSampler(ds, num_replicas=2, rank=rank)
        if epoch is not None:
            theirs_sampler.set_epoch(epoch)
        theirs = DataLoader(ds, batch_size=2, sampler=theirs_sampler, collate_fn=skeleton_colate)
        got = [b[0].flatten().int().tolist() for b in ours(epoch)]
        assert got == [b[0].flatten().int().tolist() for b in theirs] and len(ours) == len(theirs) == 2
        assert sum(got, []) == want[(epoch, rank)]
