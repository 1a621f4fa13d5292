"""The training loop (reference: skoots/train/engine.py:57-632).

``run_training`` owns the sequence -- warm-up, epochs, loss gates, sigma, learning rate, validation, histories,
saving -- and takes the step object and the batch sources as arguments, so the sequence can be tested without a GPU.
``train`` builds the transform, the datasets, their statistics, the samplers, the model and the :class:`TrainStep`
from a configuration and calls it.  What is kept of the reference's behaviour and what differs is listed in
DESIGN.md section 14.
"""
from __future__ import annotations

import csv
import logging
import os
import random
from statistics import mean
from typing import Callable, Dict, Iterator, List, Optional, Sequence

import torch

from ..config import cfg_to_dict

log = logging.getLogger(__name__)

SENTINEL = 9999999999.9999999999       # first entry of every loss history (engine.py:338-346)
TERMS = ("EMBED", "PROBABILITY", "SKELETON")
HISTORY_KEYS = ("avg_epoch_loss", "avg_epoch_embed_loss", "avg_epoch_prob_loss", "avg_epoch_skele_loss",
                "avg_val_loss", "avg_val_embed_loss", "avg_val_prob_loss", "avg_val_skele_loss")
CSV_COLUMNS = ("epoch", "lr", "sigma_x", "sigma_y", "sigma_z", "train_loss", "train_embed", "train_prob", "train_skele",
               "val_loss", "val_embed", "val_prob", "val_skele")


def relative_weights(cfg) -> List[float]:
    return [float(cfg["TRAIN"][f"LOSS_{t}_RELATIVE_WEIGHT"]) for t in TERMS]


def gated_weights(cfg, epoch: int) -> List[float]:
    """RELATIVE_WEIGHT * (1 if epoch > START_EPOCH else 0) per term: strictly greater (engine.py:480-496)."""
    return [float(cfg["TRAIN"][f"LOSS_{t}_RELATIVE_WEIGHT"]) * (1 if epoch > cfg["TRAIN"][f"LOSS_{t}_START_EPOCH"] else 0)
            for t in TERMS]


def epoch_lr(cfg, epoch: int) -> float:
    """The learning rate of epoch ``epoch``: the scheduler's value after ``epoch`` steps (it is stepped at the end of
    every epoch, engine.py:512)."""
    from .schedule import cosine_annealing_warm_restarts
    return cosine_annealing_warm_restarts(float(cfg["TRAIN"]["LEARNING_RATE"]), int(cfg["TRAIN"]["SCHEDULER_T0"]), epoch)


class Batches:
    """What ``DataLoader(dataset, batch_size, sampler=sampler, collate_fn=collate)`` with no workers yields: batches of
    ``batch_size`` consecutive sampler indices (the last one may be smaller), built lazily.  ``batches(epoch)`` calls
    ``sampler.set_epoch(epoch)`` first unless ``epoch`` is None."""

    def __init__(self, dataset, sampler, batch_size: int, collate: Callable):
        self.dataset, self.sampler, self.batch_size, self.collate = dataset, sampler, int(batch_size), collate

    def __len__(self) -> int:
        return (len(self.sampler) + self.batch_size - 1) // self.batch_size

    def __call__(self, epoch: Optional[int] = None) -> Iterator:
        if epoch is not None:
            self.sampler.set_epoch(epoch)
        indices = list(self.sampler)
        for i in range(0, len(indices), self.batch_size):
            yield self.collate([self.dataset[j] for j in indices[i:i + self.batch_size]])


def _means(losses: Sequence[torch.Tensor]) -> List[float]:
    """(total, embed, prob, skeleton) means of an epoch: the per-batch device values are read once, then averaged with
    ``statistics.mean`` over the fp32 values in batch order, as the reference averages its ``.item()``s."""
    rows = torch.stack([l.detach().reshape(4) for l in losses]).to("cpu", torch.float32).tolist()
    return [mean(r[k] for r in rows) for k in (3, 0, 1, 2)]


def save_checkpoint(path: str, payload: dict) -> None:
    """Atomically: a temporary file next to ``path``, then a rename."""
    tmp = path + ".tmp"
    torch.save(payload, tmp)
    os.replace(tmp, path)


def run_training(step, train_batches, val_batches, cfg, sigma, save_path: Optional[str] = None,
                 csv_path: Optional[str] = None, extra: Optional[dict] = None, rank: int = 0,
                 checkpoint_cfg: Optional[dict] = None) -> Dict[str, List[float]]:
    """The sequence of engine.py:348-631 around ``step``.

    ``step``: a :class:`TrainStep` (or a stand-in with ``lr``, ``__call__``, ``evaluate`` and ``checkpoint``).
    ``train_batches`` / ``val_batches``: :class:`Batches`-like (``len()`` and ``batches(epoch_or_None)`` yielding
    ``(images, masks, skeletons, skele_masks, baked)``); ``val_batches`` may be None.  ``sigma``: ``sigma(e)`` -> three
    floats.  Rank 0 writes ``save_path`` every ``SAVE_INTERVAL`` epochs, at the end and when the loop leaves through an
    exception or Ctrl-C, and one row per epoch to ``csv_path``.  Returns the eight histories."""
    t = cfg["TRAIN"]
    epochs, distributed = int(t["NUM_EPOCHS"]), bool(t["DISTRIBUTED"])
    hist: Dict[str, List[float]] = {k: [SENTINEL] for k in HISTORY_KEYS}
    state = {"epoch": 0}
    cfg_plain = checkpoint_cfg if checkpoint_cfg is not None else cfg_to_dict(cfg)

    def save():
        if save_path is None or rank != 0:
            return
        payload = step.checkpoint(cfg_plain)
        payload.update({k: list(v) for k, v in hist.items()})
        payload.update(extra or {})
        payload["epoch"] = state["epoch"]
        save_checkpoint(save_path, payload)
        log.info("saved %s after %d epochs", save_path, state["epoch"])

    csv_file = open(csv_path, "w", newline="") if (csv_path is not None and rank == 0) else None
    writer = csv.writer(csv_file) if csv_file else None
    if writer:
        writer.writerow(CSV_COLUMNS)
    try:
        # warm-up: the first training batch, N_WARMUP steps on it, sigma(0), no gates, at LEARNING_RATE
        step.lr = float(t["LEARNING_RATE"])
        first = train_batches(None)
        images, masks, _, skele_masks, baked = next(iter(first))
        if hasattr(first, "close"):
            first.close()
        for _ in range(int(t["N_WARMUP"])):
            step(images, masks, skele_masks, baked, sigma(0), relative_weights(cfg))
        del images, masks, skele_masks, baked

        validate = val_batches is not None and len(val_batches) > 0
        for e in range(epochs):
            step.lr = epoch_lr(cfg, e)
            weights, sig = gated_weights(cfg, e), sigma(e)
            losses = [step(images, masks, skele_masks, baked, sig, weights)
                      for images, masks, _, skele_masks, baked in train_batches(e if distributed else None)]
            train_means = _means(losses)
            for k, v in zip(HISTORY_KEYS[:4], train_means):
                hist[k].append(v)
            val_means: List = ["", "", "", ""]
            if validate and e % int(t["VALIDATE_EPOCH_SKIP"]) == 0:
                losses = [step.evaluate(images, masks, skele_masks, baked, sig, weights)
                          for images, masks, _, skele_masks, baked in val_batches(None)]
                val_means = _means(losses)
                for k, v in zip(HISTORY_KEYS[4:], val_means):
                    hist[k].append(v)
            state["epoch"] = e + 1
            if writer:
                writer.writerow([e, step.lr, *sig, *train_means, *val_means])
                csv_file.flush()
            log.info("epoch %d/%d lr=%.3e loss (train | val): %.5f | %.5f", e + 1, epochs, step.lr,
                     hist["avg_epoch_loss"][-1], hist["avg_val_loss"][-1])
            if (e + 1) % int(t["SAVE_INTERVAL"]) == 0 and e + 1 < epochs:
                save()
    except BaseException:
        save()
        raise
    finally:
        if csv_file:
            csv_file.close()
    save()
    return hist


# ----------------------------------------------------------------------------------------------------------------
def checkpoint_cfg(cfg) -> dict:
    """``cfg_to_dict(cfg)`` with the MODEL keys that name the network set to what was trained: this project's
    conv + GroupNorm + SiLU U-Net (``eval()`` refuses a checkpoint that claims another architecture)."""
    from ..unet import SUPPORTED_ARCHITECTURE
    d = cfg_to_dict(cfg)
    d["MODEL"].update({"ARCHITECTURE": SUPPORTED_ARCHITECTURE, "NORMALIZATION": "groupnorm", "ACTIVATION": "silu",
                       "KERNEL_SIZE": 3})
    return d


def resolve_world_size(cfg) -> int:
    """NUM_GPUS if DISTRIBUTED else 1, clamped to the devices present (with a warning)."""
    want = int(cfg["SYSTEM"]["NUM_GPUS"]) if cfg["TRAIN"]["DISTRIBUTED"] else 1
    have = torch.cuda.device_count()
    if want > have:
        log.warning("SYSTEM.NUM_GPUS = %d but %d device(s) present: training on %d", want, have, max(have, 1))
    return max(1, min(want, have))


def build_datasets(cfg, which: str, transform, device):
    from .dataloader import MultiDataset, dataset
    t = cfg["TRAIN"]
    sets = []
    for path, n, on_gpu in zip(t[f"{which}_DATA_DIR"], t[f"{which}_SAMPLE_PER_IMAGE"], t[f"{which}_STORE_DATA_ON_GPU"]):
        sets.append(dataset(path=path, transforms=transform, sample_per_image=n, device=device)
                    .to(device if on_gpu else "cpu"))
    return MultiDataset(*sets)


def train(cfg, precision: str = "bf16", seed: int = 101196, rank: int = 0, world_size: int = 1,
          run_name: Optional[str] = None, on_finish: Optional[Callable] = None) -> str:
    """Train from a validated configuration on device ``rank``; returns the checkpoint path
    ``<SAVE_PATH>/<run_name>.trch`` (``<run_name>.csv`` next to it).  With ``world_size`` > 1 the default
    torch.distributed group must exist (``skoots_amd.train.__main__`` starts the ranks).  ``on_finish(step)`` is called
    on every rank after the last epoch (the two-rank test compares the ranks' parameters with it)."""
    from ..unet import random_state_dict
    from .engine import TrainStep, TrainUNet
    from .loss import loss_from_cfg
    from .sigma import init_sigma
    from .transforms import TransformFromCfg, skeleton_colate
    from torch.utils.data.distributed import DistributedSampler

    t = cfg["TRAIN"]
    if not torch.cuda.is_available():
        raise RuntimeError("skoots_amd.train needs an MI355X: there is no CPU path")
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    random.seed(seed)
    torch.manual_seed(seed)   # the CPU generator and every device generator

    transform = TransformFromCfg(cfg, device).set_dataset_std(255).set_dataset_mean(0)
    merged_train = build_datasets(cfg, "TRAIN", transform, device)
    if len(merged_train) == 0:
        raise ValueError("TRAIN.TRAIN_DATA_DIR holds no training volume (*.labels.tif)")
    dataset_mean = float(merged_train.mean(with_invert=True))
    dataset_std = float(merged_train.std(with_invert=True))
    log.info("Normalizing to dataset: mean->%0.3f, std->%0.3f", dataset_mean, dataset_std)
    transform.set_dataset_mean(dataset_mean).set_dataset_std(dataset_std)   # the validation data shares the object
    merged_val = build_datasets(cfg, "VALIDATION", transform, device)

    bs = int(t["TRAIN_BATCH_SIZE"])   # the validation batches use TRAIN_BATCH_SIZE too (engine.py:243)
    train_batches = Batches(merged_train, DistributedSampler(merged_train, num_replicas=world_size, rank=rank), bs,
                            skeleton_colate)
    val_batches = Batches(merged_val, DistributedSampler(merged_val, num_replicas=world_size, rank=rank), bs,
                          skeleton_colate)

    dims, depths = list(cfg["MODEL"]["DIMS"]), list(cfg["MODEL"]["DEPTHS"])
    pretrained = None
    if t["PRETRAINED_MODEL_PATH"] and t["PRETRAINED_MODEL_PATH"][0]:
        pretrained = torch.load(t["PRETRAINED_MODEL_PATH"][0], map_location="cpu", weights_only=True)
    state_dict = (pretrained.get("model_state_dict", pretrained) if pretrained is not None
                  else random_state_dict(dims, depths, seed))
    model = TrainUNet(state_dict, device, dims, depths, precision=precision)
    kwargs = dict(zip(t["OPTIMIZER_KEYWORD_ARGUMENTS"], t["OPTIMIZER_KEYWORD_VALUES"]))
    losses = [loss_from_cfg(t[f"LOSS_{term}"], t[f"LOSS_{term}_KEYWORDS"], t[f"LOSS_{term}_VALUES"]) for term in TERMS]
    # (the reference's five optimizer steps before any gradient exists change nothing: torch skips parameters
    # without a gradient)
    step = TrainStep(model, lr=t["LEARNING_RATE"], weight_decay=t["WEIGHT_DECAY"], betas=kwargs.get("betas", (0.9, 0.999)),
                     eps=t["OPTIMIZER_EPS"], vector_scale=cfg["SKOOTS"]["VECTOR_SCALING"], loss_embed=losses[0],
                     loss_prob=losses[1], loss_skele=losses[2], weights=relative_weights(cfg),
                     process_group=None if world_size > 1 else False)
    if t["LOAD_PRETRAINED_OPTIMIZER"] and pretrained is not None and "optimizer_state_dict" in pretrained:
        step.load_optimizer_state(pretrained["optimizer_state_dict"])

    run_name = run_name or "skoots_train"
    save_path = os.path.join(t["SAVE_PATH"], run_name + ".trch")
    run_training(step, train_batches, val_batches, cfg, init_sigma(cfg, device), save_path=save_path,
                 csv_path=os.path.join(t["SAVE_PATH"], run_name + ".csv"),
                 extra={"dataset_mean": dataset_mean, "dataset_std": dataset_std, "seed": int(seed),
                        "precision": precision},
                 rank=rank, checkpoint_cfg=checkpoint_cfg(cfg))
    torch.cuda.synchronize(device)
    if on_finish is not None:
        on_finish(step)
    return save_path
