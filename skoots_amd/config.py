"""The training configuration (reference: skoots/config.py) without yacs.

``get_cfg_defaults()`` returns a tree of :class:`CfgNode` (a dict with attribute access) holding the reference's
sections, keys and default values; ``load_cfg_from_file`` merges a YAML file over it; ``validate_cfg`` raises
``ValueError`` naming the offending key; ``cfg_to_dict`` gives plain containers for the checkpoint.

Merge rules (yacs is not a dependency, so these are this project's): a key that the defaults do
not have is an error; a value must have the default's type, except that tuple <-> list and int -> float are accepted.
"""
from __future__ import annotations

import copy
import logging
import os
from typing import Any, Dict

log = logging.getLogger(__name__)


class CfgNode(dict):
    """A dict whose keys are also attributes (``cfg.TRAIN.NUM_EPOCHS`` and ``cfg["TRAIN"]["NUM_EPOCHS"]``)."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value):
        self[key] = value

    def clone(self) -> "CfgNode":
        return copy.deepcopy(self)


def _defaults() -> Dict[str, Dict[str, Any]]:
    return {
        "SYSTEM": {"NUM_GPUS": 2, "NUM_CPUS": 1},
        # only DIMS, DEPTHS and IN_CHANNELS shape this project's network (oracle/unet_spec.py); the rest is accepted
        # and ignored (IGNORED_MODEL_KEYS)
        "MODEL": {
            "ARCHITECTURE": "bism_unext", "IN_CHANNELS": 1, "OUT_CHANNELS": 32,
            "DIMS": [32, 64, 128, 64, 32], "DEPTHS": [2, 2, 2, 2, 2], "KERNEL_SIZE": 7,
            "DROP_PATH_RATE": 0.0, "LAYER_SCALE_INIT_VALUE": 1.0, "ACTIVATION": "gelu", "BLOCK": "block3d",
            "CONCAT_BLOCK": "concatconv3d", "UPSAMPLE_BLOCK": "upsamplelayer3d", "NORMALIZATION": "layernorm",
            "COMPILE": False,
        },
        "TRAIN": {
            "TARGET": "skoots", "DISTRIBUTED": True, "PRETRAINED_MODEL_PATH": [], "LOAD_PRETRAINED_OPTIMIZER": False,
            "TRANSFORM_DEVICE": "default", "DATALOADER_OUTPUT_DEVICE": "default", "DATALOADER_NUM_WORKERS": 0,
            "DATALOADER_PREFETCH_FACTOR": 0,
            "LOSS_EMBED": "tversky", "LOSS_EMBED_KEYWORDS": ["alpha", "beta", "eps"],
            "LOSS_EMBED_VALUES": [0.25, 0.75, 1e-8],
            "LOSS_PROBABILITY": "tversky", "LOSS_PROBABILITY_KEYWORDS": ["alpha", "beta", "eps"],
            "LOSS_PROBABILITY_VALUES": [0.5, 0.5, 1e-8],
            "LOSS_SKELETON": "tversky", "LOSS_SKELETON_KEYWORDS": ["alpha", "beta", "eps"],
            "LOSS_SKELETON_VALUES": [0.5, 1.5, 1e-8],
            "LOSS_EMBED_RELATIVE_WEIGHT": 1.0, "LOSS_PROBABILITY_RELATIVE_WEIGHT": 1.0,
            "LOSS_SKELETON_RELATIVE_WEIGHT": 1.0,
            "LOSS_EMBED_START_EPOCH": -1, "LOSS_PROBABILITY_START_EPOCH": -1, "LOSS_SKELETON_START_EPOCH": 10,
            "TRAIN_DATA_DIR": [], "TRAIN_SAMPLE_PER_IMAGE": [], "TRAIN_BATCH_SIZE": 1,
            "VALIDATION_DATA_DIR": [], "VALIDATION_SAMPLE_PER_IMAGE": [], "VALIDATION_BATCH_SIZE": 1,
            "BACKGROUND_DATA_DIR": [], "BACKGROUND_SAMPLE_PER_IMAGE": [],
            "TRAIN_STORE_DATA_ON_GPU": [], "VALIDATION_STORE_DATA_ON_GPU": [], "BACKGROUND_STORE_DATA_ON_GPU": [],
            "STORE_DATA_ON_GPU": [],
            "INITIAL_SIGMA": [20.0, 20.0, 20.0],
            "SIGMA_DECAY": [[0.66, 200], [0.66, 800], [0.66, 1500], [0.5, 20000], [0.5, 20000]],
            "NUM_EPOCHS": 10000, "LEARNING_RATE": 5e-4, "WEIGHT_DECAY": 1e-6, "OPTIMIZER": "adamw",
            "OPTIMIZER_KEYWORD_ARGUMENTS": [], "OPTIMIZER_KEYWORD_VALUES": [], "OPTIMIZER_EPS": 1e-8,
            "SCHEDULER": "cosine_annealing_warm_restarts", "SCHEDULER_T0": 10001, "MIXED_PRECISION": True,
            "N_WARMUP": 1500,
            "SAVE_PATH": ".",   # the reference's default is its author's home directory
            "SKELETON_MASK_RADIUS": 9, "SKELETON_MASK_FLANK_RADIUS": 3, "SAVE_INTERVAL": 100,
            "VALIDATE_EPOCH_SKIP": 10, "CUDNN_BENCHMARK": True, "AUTOGRAD_PROFILE": False,
            "AUTOGRAD_EMIT_NVTX": False, "AUTOGRAD_DETECT_ANOMALY": False,
        },
        "AUGMENTATION": {
            "CROP_WIDTH": 300, "CROP_HEIGHT": 300, "CROP_DEPTH": 20, "FLIP_RATE": 0.5, "BRIGHTNESS_RATE": 0.4,
            "BRIGHTNESS_RANGE": [-0.1, 0.1], "NOISE_GAMMA": 0.1, "NOISE_RATE": 0.2, "CONTRAST_RATE": 0.33,
            "CONTRAST_RANGE": [0.75, 2.0], "AFFINE_RATE": 0.66, "AFFINE_SCALE": [0.85, 1.1],
            "AFFINE_YAW": [-180, 180], "AFFINE_SHEAR": [-7, 7], "SMOOTH_SKELETON_KERNEL_SIZE": (3, 3, 1),
            "BAKE_SKELETON_ANISOTROPY": (1.0, 1.0, 3.0), "N_SKELETON_MASK_DILATE": 1,
            "ELASTIC_GRID_SHAPE": (6, 6, 2), "ELASTIC_GRID_MAGNITUDE": (0.05, 0.05, 0.01), "ELASTIC_RATE": 0.33,
        },
        "SKOOTS": {"VECTOR_SCALING": (60, 60, 12), "ANISOTROPY": (1.0, 1.0, 3.0), "NOTES": ""},
        "EXPERIMENTAL": {
            "DIST_THR": 10.0, "IS_SPARSE": False, "SPARSE_BACKGROUND_PENALTY_MULTIPLIER": 10,
            "BACKGROUND_N_ERODE": 0.0, "BACKGROUND_SLICE_PERCENTAGE": 1.0,
        },
    }


# MODEL keys that describe the reference's bism network and have no meaning for this project's U-Net
IGNORED_MODEL_KEYS = ("ARCHITECTURE", "OUT_CHANNELS", "KERNEL_SIZE", "DROP_PATH_RATE", "LAYER_SCALE_INIT_VALUE",
                      "ACTIVATION", "BLOCK", "CONCAT_BLOCK", "UPSAMPLE_BLOCK", "NORMALIZATION", "COMPILE")


def _to_node(tree) -> CfgNode:
    return CfgNode({k: _to_node(v) if isinstance(v, dict) else v for k, v in tree.items()})


def get_cfg_defaults() -> CfgNode:
    """A fresh tree with the default values (changing it does not change the defaults)."""
    return _to_node(_defaults())


def _fit(value, default, where: str):
    """``value`` in the type of ``default``, or a ValueError."""
    if isinstance(default, bool) or isinstance(value, bool):
        if isinstance(default, bool) and isinstance(value, bool):
            return value
    elif isinstance(default, float) and isinstance(value, (int, float)):
        return float(value)
    elif isinstance(default, int) and isinstance(value, int):
        return value
    elif isinstance(default, str) and isinstance(value, str):
        return value
    elif isinstance(default, (list, tuple)) and isinstance(value, (list, tuple)):
        return type(default)(value)
    raise ValueError(f"{where}: a {type(value).__name__} ({value!r}) does not fit the default's type "
                     f"{type(default).__name__} ({default!r})")


def merge_cfg(cfg: CfgNode, other: dict, _where: str = "") -> CfgNode:
    """Merge a (nested) dict over ``cfg`` in place, under the rules of the module docstring."""
    if not isinstance(other, dict):
        raise ValueError(f"{_where or 'configuration'}: expected a mapping, got {type(other).__name__}")
    for k, v in other.items():
        where = f"{_where}.{k}" if _where else str(k)
        if k not in cfg:
            raise KeyError(f"{where}: not a configuration key")
        if isinstance(cfg[k], dict):
            merge_cfg(cfg[k], v, where)
        else:
            cfg[k] = _fit(v, cfg[k], where)
    return cfg


def load_cfg_from_file(path: str, validate: bool = True) -> CfgNode:
    """The defaults with the YAML file at ``path`` merged over them (skoots/train/__main__.py:22-34)."""
    import yaml
    if not os.path.exists(path):
        raise ValueError(f"Could not find config file from path: {path}")
    with open(path) as f:
        loaded = yaml.safe_load(f)
    cfg = merge_cfg(get_cfg_defaults(), loaded or {})
    if validate:
        validate_cfg(cfg)
    return cfg


def _same_len(cfg, section: str, *keys: str) -> None:
    lens = [len(cfg[section][k]) for k in keys]
    if len(set(lens)) != 1:
        names = ", ".join(f"{section}.{k} ({n})" for k, n in zip(keys, lens))
        raise ValueError(f"lengths differ: {names}")


def validate_cfg(cfg) -> None:
    """The reference's checks that mean something here (skoots/config.py:157-219) and the things this project does
    not support; every failure is a ValueError that names the key."""
    m, t = cfg["MODEL"], cfg["TRAIN"]
    if len(m["DIMS"]) != len(m["DEPTHS"]):
        raise ValueError(f"MODEL.DIMS ({len(m['DIMS'])}) and MODEL.DEPTHS ({len(m['DEPTHS'])}) differ in length")
    if m["IN_CHANNELS"] != 1:
        raise ValueError(f"MODEL.IN_CHANNELS = {m['IN_CHANNELS']}: only greyscale input images are supported")
    ignored = {k: m[k] for k in IGNORED_MODEL_KEYS if m[k] != _defaults()["MODEL"][k]}
    if ignored:
        log.warning("MODEL keys without effect on this project's U-Net (conv + GroupNorm + SiLU): %s", ignored)
    if t["TARGET"] != "skoots":
        raise ValueError('TRAIN.TARGET must be "skoots"')
    for term in ("EMBED", "PROBABILITY", "SKELETON"):
        _same_len(cfg, "TRAIN", f"LOSS_{term}_KEYWORDS", f"LOSS_{term}_VALUES")
        if t[f"LOSS_{term}_RELATIVE_WEIGHT"] < 0:
            raise ValueError(f"TRAIN.LOSS_{term}_RELATIVE_WEIGHT must be >= 0")
    for src in ("TRAIN", "VALIDATION", "BACKGROUND"):
        _same_len(cfg, "TRAIN", f"{src}_DATA_DIR", f"{src}_SAMPLE_PER_IMAGE", f"{src}_STORE_DATA_ON_GPU")
    _same_len(cfg, "TRAIN", "OPTIMIZER_KEYWORD_ARGUMENTS", "OPTIMIZER_KEYWORD_VALUES")
    for k in ("TRAIN_BATCH_SIZE", "VALIDATION_BATCH_SIZE", "VALIDATE_EPOCH_SKIP"):
        if t[k] < 1:
            raise ValueError(f"TRAIN.{k} must be >= 1")
    if not os.path.exists(t["SAVE_PATH"]):
        raise ValueError(f"TRAIN.SAVE_PATH does not exist: {t['SAVE_PATH']}")
    for p in t["PRETRAINED_MODEL_PATH"]:
        if p and not os.path.exists(p):
            raise ValueError(f"TRAIN.PRETRAINED_MODEL_PATH: {p} does not exist")
    # not supported here
    if t["OPTIMIZER"] != "adamw":
        raise ValueError(f"TRAIN.OPTIMIZER = {t['OPTIMIZER']!r} is not supported: the step's optimizer kernel is AdamW")
    if t["SCHEDULER"] != "cosine_annealing_warm_restarts":
        raise ValueError(f"TRAIN.SCHEDULER = {t['SCHEDULER']!r} is not supported (cosine_annealing_warm_restarts only)")
    if cfg["EXPERIMENTAL"]["IS_SPARSE"]:
        raise ValueError("EXPERIMENTAL.IS_SPARSE is not supported: sparse training is not part of this project")
    if len(t["BACKGROUND_DATA_DIR"]):
        raise ValueError("TRAIN.BACKGROUND_DATA_DIR is not supported: the reference's background transform returns "
                         "None, so that path has never produced a sample")
    for k in ("TRANSFORM_DEVICE", "DATALOADER_OUTPUT_DEVICE"):
        if t[k] != "default":
            raise ValueError(f"TRAIN.{k} = {t[k]!r} is not supported: the transform's kernels run on the device")
    if t["DATALOADER_NUM_WORKERS"] > 0:
        raise ValueError("TRAIN.DATALOADER_NUM_WORKERS > 0 is not supported: the transform launches kernels")
    for k in t["OPTIMIZER_KEYWORD_ARGUMENTS"]:
        if k != "betas":
            raise ValueError(f"TRAIN.OPTIMIZER_KEYWORD_ARGUMENTS: {k!r} is not supported (betas only)")


def cfg_to_dict(cfg):
    """Plain dicts / lists / numbers / strings (a checkpoint's ``cfg`` loads with ``weights_only=True``)."""
    if isinstance(cfg, dict):
        return {str(k): cfg_to_dict(v) for k, v in cfg.items()}
    if isinstance(cfg, (list, tuple)):
        return [cfg_to_dict(v) for v in cfg]
    if isinstance(cfg, (bool, int, float, str)) or cfg is None:
        return cfg
    raise TypeError(f"cannot store a {type(cfg).__name__} in a checkpoint's cfg")
