"""Training-crop augmentation on the MI355X: ``TransformFromCfg`` and ``skeleton_colate``
(reference: skoots/train/merged_transform.py:402-762 and skoots/train/dataloader.py:627-649).

One sample goes crop 1 -> elastic -> affine -> crop 2 -> flips -> invert -> brightness -> contrast -> noise ->
normalise, then the two targets (``bake_skeleton``, ``skeleton_to_mask``).  The random draws of a sample are an
:class:`AugmentPlan`; ``draw_plan`` consumes Python's ``random`` in the reference's order, so a seeded ``random``
takes the reference's decisions.  The voxel work is three HIP launches (csrc/augment.hip): one gather that composes
every geometric stage and applies invert / brightness, then contrast + noise, then the normalisation.  The skeleton
points (N of them, not the hot path) are moved with torch on the device.  The reference's quirks that this port
keeps, and the one it does not raise on, are listed in DESIGN.md section 11.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _ffi
from ..lib.skeleton import bake_skeleton, skeleton_to_mask

# elastic_deform's defaults (merged_transform.py:75-80): TransformFromCfg calls it without the cfg's
# ELASTIC_GRID_SHAPE / ELASTIC_GRID_MAGNITUDE, so these are what the reference uses
ELASTIC_FIELD_SHAPE = (1, 3, 2, 6, 6)            # (1, 3, z, y, x) of displacement_shape (6, 6, 2)
ELASTIC_MAGNITUDE_ZYX = (0.01, 0.05, 0.05)       # displacement_magnitude (0.05, 0.05, 0.01), reversed
CROP1_EXTRA = 300                                # crop 1 is the crop plus 300 voxels in x and y


def _cfg_get(cfg, *path):
    for k in path:
        cfg = cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)
    return cfg


@dataclass
class AugmentPlan:
    """Every random draw of one sample, in the order ``TransformFromCfg.forward`` makes them."""
    key: object                                  # skeleton id that crop 1 centres on
    elastic: bool = False
    elastic_field: Optional[Tensor] = None       # (1, 3, 2, 6, 6) fp32 in [0, 1)
    affine: bool = False
    angle: float = 0.0
    shear: float = 0.0
    scale: float = 1.0
    flip_x: bool = False
    flip_y: bool = False
    flip_z: bool = False
    invert: bool = False
    brightness: bool = False
    brightness_val: float = 0.0
    contrast: bool = False
    contrast_val: float = 1.0
    noise: Optional[Tensor] = None               # (1, w2, h2, d2) fp32 in [0, 1), scaled by NOISE_GAMMA


def draw_plan(transform: "TransformFromCfg", keys: Sequence, image_shape: Sequence[int], device=None) -> AugmentPlan:
    """Draw one sample's plan with Python's ``random`` in the reference's order (forward, merged_transform.py:657-745):
    the crop-1 key, elastic, affine (rate, then angle, shear, scale), three flips, invert, brightness (rate, value),
    contrast (rate, value), noise.  Tensor draws use ``torch.rand`` on ``device``."""
    t = transform
    device = t.DEVICE if device is None else device
    _, (w2, h2, d2) = t.crop_extents(image_shape)
    p = AugmentPlan(key=random.choice(list(keys)))
    if random.random() < t.ELASTIC_RATE:
        p.elastic = True
        p.elastic_field = torch.rand(ELASTIC_FIELD_SHAPE, device=device)
    if random.random() < t.AFFINE_RATE:
        p.affine = True
        p.angle = random.uniform(*t.AFFINE_YAW)
        p.shear = random.uniform(*t.AFFINE_SHEAR)
        p.scale = random.uniform(*t.AFFINE_SCALE)
    p.flip_x = random.random() < t.FLIP_RATE
    p.flip_y = random.random() < t.FLIP_RATE
    p.flip_z = random.random() < t.FLIP_RATE
    p.invert = random.random() < t.BRIGHTNESS_RATE
    if random.random() < t.BRIGHTNESS_RATE:
        p.brightness = True
        p.brightness_val = random.uniform(*t.BRIGHTNESS_RANGE)
    if random.random() < t.CONTRAST_RATE:
        p.contrast = True
        p.contrast_val = random.uniform(*t.CONTRAST_RANGE)
    if random.random() < t.NOISE_RATE:
        p.noise = torch.rand((1, w2, h2, d2), device=device)
    return p


def _rss(angle: float, shear: Tuple[float, float], scale: float) -> Tuple[float, float, float, float]:
    """Rotation-scale-shear entries (a, b, c, d) of torchvision's affine parameterisation, without the scale."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    return a, b, c, d


def _image_theta(angle: float, shear: float, scale: float, w1: int, h1: int) -> List[float]:
    """The grid rows of ``ttf.affine(img [C, Z, H = w1, W = h1], angle, shear=float, scale)`` on a tensor: the inverse
    matrix about centre (0, 0) with shear [shear, 0] (fp32, as F_t.affine builds theta), divided by (W / 2, H / 2) as
    _gen_affine_grid rescales it.  Returned as [x row (3), y row (3)] of the sampling grid."""
    a, b, c, d = _rss(angle, (shear, 0.0), scale)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]   # centre and translation are 0
    theta = torch.tensor(m, dtype=torch.float32).reshape(2, 3)
    div = torch.tensor([0.5 * h1, 0.5 * w1], dtype=torch.float32)
    rescaled = theta / div.view(2, 1)                               # row j of theta over div[j]
    return rescaled.reshape(-1).tolist()


def _mm_fma(A: Tensor, B: Tensor) -> Tensor:
    """fp32 A @ B with each entry an FMA chain over k in ascending order (acc = a0 b0; acc = fma(ak, bk, acc)), the
    inner product of the reference's CPU matmul.  Each step is exact in float64 and rounded once to fp32, so the
    result does not depend on which GEMM the device would pick.  A (M, K), B (K, N)."""
    A64, B64 = A.double(), B.double()
    acc = (A64[:, :1] * B64[:1, :]).float()
    for k in range(1, A.shape[1]):
        acc = (A64[:, k:k + 1] * B64[k:k + 1, :] + acc.double()).float()
    return acc


def _skeleton_affine_matrix(center: Tuple[float, float], angle: float, shear: Tuple[float, float], scale: float,
                            device) -> Tensor:
    """T C RSS C^-1 (translation 0) in fp32 on ``device``: the reference's skeleton matrix (merged_transform.py:
    217-285), with C^-1 written out (the exact inverse of a translation)."""
    a, b, c, d = _rss(angle, shear, scale)
    rss = torch.tensor([[a, b, 0.0], [c, d, 0.0], [0.0, 0.0, 1.0]], device=device) * scale
    rss[2, 2] = 1.0
    C = torch.eye(3, device=device)
    C[0, 2], C[1, 2] = center
    Ci = torch.eye(3, device=device)
    Ci[0, 2], Ci[1, 2] = -center[0], -center[1]
    T = torch.eye(3, device=device)
    return _mm_fma(_mm_fma(_mm_fma(T, C), rss), Ci)


class TransformFromCfg(torch.nn.Module):
    """The reference's training transform (merged_transform.py:402-780) on the HIP kernels.  ``cfg`` is an attribute
    dict or a plain dict with the reference's AUGMENTATION and TRAIN keys.

    ``forward(data_dict, plan=None)`` takes and returns the reference's keys: ``image`` (1, X, Y, Z) uint8 / fp16 /
    fp32 and ``masks`` (1, X, Y, Z) uint8 / int16 / int32, on the CPU or the device; ``skeletons`` {id: (N, 3)}.  It
    adds ``baked_skeleton`` (3, x, y, z) and ``skele_masks`` (1, x, y, z) and replaces ``image`` by the augmented fp32
    crop and ``masks`` by its int32 ids (ids must be below 2^24: the reference's float path is exact up to there).
    A volume on the CPU has only its crop-1 window copied to the device.  ``plan`` fixes the random draws."""

    def __init__(self, cfg, device, scale: float = 255.0):
        super().__init__()
        self.prefix_function = self._identity
        self.posfix_function = self._identity
        self.dataset_mean = 0
        self.dataset_std = 1
        self.cfg = cfg
        self.DEVICE = torch.device(device)
        self.SCALE = scale

        def aug(k):
            return _cfg_get(cfg, "AUGMENTATION", k)

        self.CROP_WIDTH = aug("CROP_WIDTH")
        self.CROP_HEIGHT = aug("CROP_HEIGHT")
        self.CROP_DEPTH = aug("CROP_DEPTH")
        self.FLIP_RATE = aug("FLIP_RATE")
        self.BRIGHTNESS_RATE = aug("BRIGHTNESS_RATE")
        self.BRIGHTNESS_RANGE = aug("BRIGHTNESS_RANGE")
        self.NOISE_GAMMA = aug("NOISE_GAMMA")
        self.NOISE_RATE = aug("NOISE_RATE")
        self.FILTER_RATE = 0.5
        self.CONTRAST_RATE = aug("CONTRAST_RATE")
        self.CONTRAST_RANGE = aug("CONTRAST_RANGE")
        self.AFFINE_RATE = aug("AFFINE_RATE")
        self.AFFINE_SCALE = aug("AFFINE_SCALE")
        self.AFFINE_SHEAR = aug("AFFINE_SHEAR")
        self.AFFINE_YAW = aug("AFFINE_YAW")
        self.ELASTIC_GRID_SHAPE = aug("ELASTIC_GRID_SHAPE")
        self.ELASTIC_GRID_MAGNITUDE = aug("ELASTIC_GRID_MAGNITUDE")
        self.ELASTIC_RATE = aug("ELASTIC_RATE")
        self.BAKE_SKELETON_ANISOTROPY = aug("BAKE_SKELETON_ANISOTROPY")
        self.SKELETON_MASK_RADIUS = _cfg_get(cfg, "TRAIN", "SKELETON_MASK_RADIUS")
        self.SKELETON_MASK_FLANK_RADIUS = _cfg_get(cfg, "TRAIN", "SKELETON_MASK_FLANK_RADIUS")

    @staticmethod
    def _identity(*args):
        return args if len(args) > 1 else args[0]

    def set_dataset_mean(self, mean):
        self.dataset_mean = mean
        return self

    def set_dataset_std(self, std):
        self.dataset_std = std
        return self

    def pre_fn(self, fn: Callable[[Dict[str, Tensor]], Dict[str, Tensor]]):
        self.prefix_function = fn
        return self

    def post_fn(self, fn: Callable[[Dict[str, Tensor]], Dict[str, Tensor]]):
        self.posfix_function = fn
        return self

    def crop_extents(self, image_shape: Sequence[int]):
        """((w1, h1, d1), (w2, h2, d2)): the crop-1 window and the output for an image of shape (C, X, Y, Z)."""
        _, X, Y, Z = (int(s) for s in image_shape)
        w1 = self.CROP_WIDTH + CROP1_EXTRA if self.CROP_WIDTH + CROP1_EXTRA <= X else X
        h1 = self.CROP_HEIGHT + CROP1_EXTRA if self.CROP_HEIGHT + CROP1_EXTRA <= Y else Y
        d1 = self.CROP_DEPTH if self.CROP_DEPTH <= Z else Z
        w2 = self.CROP_WIDTH if self.CROP_WIDTH < w1 else w1
        h2 = self.CROP_HEIGHT if self.CROP_HEIGHT < h1 else h1
        d2 = self.CROP_DEPTH if self.CROP_DEPTH < d1 else d1
        return (w1, h1, d1), (w2, h2, d2)

    def draw_plan(self, data_dict: Dict[str, Tensor]) -> AugmentPlan:
        return draw_plan(self, data_dict["skeletons"].keys(), data_dict["image"].shape, self.DEVICE)

    @torch.no_grad()
    def geometry(self, image_shape: Sequence[int], skeletons: Dict[int, Tensor], plan: AugmentPlan, device=None):
        """Everything of one sample that is not a voxel: the crop-1 origin in the volume, the crop-2 origin in the
        crop-1 window, the image's affine grid rows and the skeleton points in output coordinates (fp32 on
        ``device``; torch, N points).  The crop centre is the fp32 mean of the plan's instance, as in the reference."""
        dev = self.DEVICE if device is None else torch.device(device)
        _, X, Y, Z = (int(s) for s in image_shape)
        (w1, h1, d1), (w2, h2, d2) = self.crop_extents(image_shape)
        center = skeletons[plan.key].float().mean(0).squeeze()
        o1 = torch.stack([center[i].sub(e // 2).long().clamp(min=0, max=n - e)
                          for i, (e, n) in enumerate(((w1, X), (h1, Y), (d1, Z)))])
        x0, y0, z0 = (int(v) for v in o1.tolist())
        keys = list(skeletons.keys())
        counts = [int(skeletons[k].shape[0]) for k in keys]
        shift1 = torch.tensor([x0, y0, z0], device=center.device)
        pts = torch.cat([skeletons[k].to(center.device).sub(shift1).float() for k in keys]).to(dev)

        # elastic: the skeletons stay where they are (the reference's in-bounds test never holds)
        theta = [0.0] * 6
        if plan.affine:
            mat = _skeleton_affine_matrix((w1 / 2, h1 / 2), -plan.angle, (0.0, plan.shear), plan.scale, dev)
            xy1 = torch.cat((pts[:, :2].T, torch.ones((1, pts.shape[0]), device=dev)), 0)
            pts[:, :2] = _mm_fma(mat, xy1)[:2].T
            theta = _image_theta(plan.angle, float(plan.shear), plan.scale, w1, h1)

        # crop 2: centred on the crop-1-relative centre (the rotation is not applied to it)
        center2 = center - shift1
        o2 = torch.stack([center2[i].sub(e // 2).long().clamp(min=0, max=n - e)
                          for i, (e, n) in enumerate(((w2, w1), (h2, h1), (d2, d1)))])
        cx0, cy0, cz0 = (int(v) for v in o2.tolist())
        pts = pts - torch.tensor([cx0, cy0, cz0], device=dev)
        if -1 not in skeletons:
            for axis, (flip, extent) in enumerate(((plan.flip_x, w2), (plan.flip_y, h2), (plan.flip_z, d2))):
                if flip:
                    pts[:, axis] = extent - pts[:, axis]
        return {"crop1": (x0, y0, z0), "crop2": (cx0, cy0, cz0), "theta": theta,
                "skeletons": dict(zip(keys, torch.split(pts, counts)))}

    @torch.no_grad()
    def augment(self, image: Tensor, masks: Tensor, skeletons: Dict[int, Tensor], plan: AugmentPlan,
                intensity: bool = True):
        """The voxel and skeleton stages of one sample: (image (1, w2, h2, d2) fp32, masks (1, w2, h2, d2) int32,
        skeletons {id: (N, 3) fp32} in output coordinates).  ``intensity=False`` stops after the geometric stages
        (no invert, brightness, contrast, noise or normalisation)."""
        if image.ndim != 4 or image.shape[0] != 1 or tuple(masks.shape) != tuple(image.shape):
            raise ValueError(f"image and masks must both be (1, X, Y, Z); got {tuple(image.shape)}, {tuple(masks.shape)}")
        dev = self.DEVICE
        _, X, Y, Z = (int(s) for s in image.shape)
        (w1, h1, d1), (w2, h2, d2) = self.crop_extents(image.shape)
        img_code, msk_code = _ffi.dtype_code(image), _ffi.dtype_code(masks)
        if img_code not in (_ffi.SK_U8, _ffi.SK_F16, _ffi.SK_F32) or msk_code not in (_ffi.SK_U8, _ffi.SK_I16, _ffi.SK_I32):
            raise ValueError(f"image must be uint8 / fp16 / fp32 and masks uint8 / int16 / int32, got {image.dtype}, "
                             f"{masks.dtype}")

        g = self.geometry(image.shape, skeletons, plan, dev)
        (x0, y0, z0), (cx0, cy0, cz0) = g["crop1"], g["crop2"]
        if image.device == dev:
            src_img, src_msk, src_shape, c1 = image.contiguous(), masks.contiguous(), (X, Y, Z), (x0, y0, z0)
        else:  # the reference's layout: the volume on the CPU, only the crop-1 window goes to the device
            win = (slice(None), slice(x0, x0 + w1), slice(y0, y0 + h1), slice(z0, z0 + d1))
            src_img = image[win].contiguous().to(dev)
            src_msk = masks[win].contiguous().to(dev)
            src_shape, c1 = (w1, h1, d1), (0, 0, 0)
        theta = g["theta"]
        out_skel = g["skeletons"]

        p = _ffi.AugParams()
        p.src_x, p.src_y, p.src_z = src_shape
        p.c1_x0, p.c1_y0, p.c1_z0 = c1
        p.w1, p.h1, p.d1 = w1, h1, d1
        p.c2_x0, p.c2_y0, p.c2_z0 = cx0, cy0, cz0
        p.w2, p.h2, p.d2 = w2, h2, d2
        p.flip_x, p.flip_y, p.flip_z = int(plan.flip_x), int(plan.flip_y), int(plan.flip_z)
        p.affine = int(plan.affine)
        p.theta[:] = theta
        field = None
        if plan.elastic:
            field = plan.elastic_field.to(dev, torch.float32).contiguous()
            if tuple(field.shape) != ELASTIC_FIELD_SHAPE:
                raise ValueError(f"elastic_field must be {ELASTIC_FIELD_SHAPE}, got {tuple(field.shape)}")
            p.elastic = 1
            p.field_d, p.field_h, p.field_w = ELASTIC_FIELD_SHAPE[2:]
            p.magnitude[:] = list(ELASTIC_MAGNITUDE_ZYX)
        p.invert = int(intensity and plan.invert)
        p.brightness = int(intensity and plan.brightness)
        p.brightness_val = float(plan.brightness_val)

        out_img = torch.empty((1, w2, h2, d2), dtype=torch.float32, device=dev)
        out_msk = torch.empty((1, w2, h2, d2), dtype=torch.int32, device=dev)
        ws_bytes = int(_ffi.lib.sk_aug_workspace_bytes(w2, h2, d2))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = _ffi.stream_ptr(dev)
        _ffi.check(_ffi.lib.sk_aug_resample(p, _ffi.ptr(src_img), img_code, _ffi.ptr(src_msk), msk_code,
                                            _ffi.ptr(field), _ffi.ptr(out_img), _ffi.ptr(out_msk), _ffi.ptr(ws),
                                            ws_bytes, st))
        if intensity:
            noise = None
            if plan.noise is not None:
                noise = plan.noise.to(dev, torch.float32).contiguous()
                if tuple(noise.shape) != (1, w2, h2, d2):
                    raise ValueError(f"noise must be (1, {w2}, {h2}, {d2}), got {tuple(noise.shape)}")
            own_mean, own_std = not self.dataset_mean, not self.dataset_std
            _ffi.check(_ffi.lib.sk_aug_intensity(_ffi.ptr(out_img), w2, h2, d2, int(plan.contrast),
                                                 float(plan.contrast_val), _ffi.ptr(noise), float(self.NOISE_GAMMA),
                                                 int(own_mean), 0.0 if own_mean else float(self.dataset_mean),
                                                 int(own_std), 0.0 if own_std else float(self.dataset_std),
                                                 _ffi.ptr(ws), ws_bytes, st))
        return out_img, out_msk, out_skel

    @torch.no_grad()
    def forward(self, data_dict: Dict[str, Tensor], plan: Optional[AugmentPlan] = None) -> Dict[str, Tensor]:
        for k in ("masks", "image", "skeletons"):
            if k not in data_dict:
                raise KeyError(f'keyword "{k}" not in data_dict')
        data_dict = self.prefix_function(data_dict)
        if plan is None:
            plan = self.draw_plan(data_dict)
        image, masks, skeletons = self.augment(data_dict["image"], data_dict["masks"], data_dict["skeletons"], plan)
        data_dict["image"] = image
        data_dict["masks"] = masks
        data_dict["baked_skeleton"] = bake_skeleton(masks, skeletons, anisotropy=self.BAKE_SKELETON_ANISOTROPY,
                                                    average=True, device=self.DEVICE)
        _, x, y, z = masks.shape
        data_dict["skele_masks"] = skeleton_to_mask(skeletons, (x, y, z), device=self.DEVICE,
                                                    radius=self.SKELETON_MASK_RADIUS,
                                                    flank_radius=self.SKELETON_MASK_FLANK_RADIUS)
        return self.posfix_function(data_dict)

    def __repr__(self):
        return f"TransformFromCfg[Device:{self.DEVICE}]"


def skeleton_colate(data_dict: List[Dict[str, Tensor]]):
    """Batch augmented samples (dataloader.py:627-649): (images (B, 1, X, Y, Z) fp32, masks (B, 1, X, Y, Z) int32,
    skeletons [dict], skele_masks (B, 1, X, Y, Z) fp32, baked (B, 3, X, Y, Z) fp32 or None) -- the dtypes and layout
    ``TrainStep.__call__(images, masks, skele_masks, baked)`` takes."""
    images = torch.stack([dd.pop("image") for dd in data_dict], dim=0).to(torch.float32).contiguous()
    masks = torch.stack([dd.pop("masks") for dd in data_dict], dim=0).to(torch.int32).contiguous()
    skele_masks = torch.stack([dd.pop("skele_masks") for dd in data_dict], dim=0).to(torch.float32).contiguous()
    baked = [dd.pop("baked_skeleton") for dd in data_dict]
    baked = torch.stack(baked, dim=0).to(torch.float32).contiguous() if baked[0] is not None else None
    skeletons = [dd.pop("skeletons") for dd in data_dict]
    for name, t, c in (("images", images, 1), ("masks", masks, 1), ("skele_masks", skele_masks, 1)):
        if t.ndim != 5 or t.shape[1] != c:
            raise ValueError(f"{name} must batch to (B, {c}, X, Y, Z), got {tuple(t.shape)}")
    if baked is not None and (baked.ndim != 5 or baked.shape[1] != 3):
        raise ValueError(f"baked_skeleton must batch to (B, 3, X, Y, Z), got {tuple(baked.shape)}")
    return images, masks, skeletons, skele_masks, baked
