#!/usr/bin/env python3
"""Generate tests/golden/augment.npz from the REFERENCE's own TransformFromCfg and skeleton_to_mask.

Run where the reference checkout is available (the GPU tests read only the committed .npz), like make_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 PYTORCH_JIT=0 \\
        python tests/golden/make_augment_golden.py

The placeholders for absent third-party modules are make_golden.py's, plus two that the
transform reaches:

  skimage.morphology.disk        x^2 + y^2 <= r^2 over [-r, r]^2, uint8 (skimage's definition)
  torchvision.transforms.functional
                                 a restatement of torchvision's tensor path, which this stage is therefore pinned
                                 to (not torchvision itself):
                                 affine          shear number -> [shear, 0], centre [0, 0], the inverse affine
                                                 matrix, _gen_affine_grid, grid_sample(nearest, zeros,
                                                 align_corners=False)
                                 adjust_contrast per-image mean, blend with the image, clamp to [0, 1]

The reference's _elastic is called with an empty skeleton dict: with real skeletons its in-bounds test raises
(DESIGN.md section 11, quirk 1), and with any skeletons it would leave them unchanged.  bake_skeleton is not called
(the GPU test compares the port's baked target with bake_skeleton on the fixture's own masks and points).  The
reference's skeleton_to_mask returns torch.zeros(shape, device) for a -1 key, which raises a TypeError; the -1 case
records the zeros it means.

Every draw the reference makes (random.choice / random / uniform, torch.rand) is recorded; they become the
AugmentPlan fields of each case.

  augment.npz   per case: the input volume, masks and skeletons, the cfg, the seed, the draws, the image before
                the intensity stages, the final image and masks, the skeleton points handed to skeleton_to_mask, and
                skele_masks; skeleton_to_mask alone for radius 7/3 and 9/3; get_cached_disk_coords tables
"""
import math
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _ident(*a, **k):
    return a[0] if a and callable(a[0]) else (lambda f: f)


def _disk(radius, dtype=np.uint8):
    r = np.arange(-radius, radius + 1)
    xx, yy = np.meshgrid(r, r)
    return (xx ** 2 + yy ** 2 <= radius ** 2).astype(dtype)


# --- torchvision.transforms.functional, tensor path (restated) -------------------------------------------------
def _inverse_affine_matrix(center, angle, translate, scale, shear):
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def _gen_affine_grid(theta, w, h, ow, oh):
    d = 0.5
    base = torch.empty(1, oh, ow, 3, dtype=theta.dtype)
    base[..., 0].copy_(torch.linspace(-ow * 0.5 + d, ow * 0.5 + d - 1, steps=ow))
    base[..., 1].copy_(torch.linspace(-oh * 0.5 + d, oh * 0.5 + d - 1, steps=oh).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype)
    return base.view(1, oh * ow, 3).bmm(rescaled).view(1, oh, ow, 2)


def _tv_affine(img, angle, translate, scale, shear, interpolation=None, fill=None, center=None):
    if isinstance(shear, (int, float)):
        shear = [shear, 0.0]
    matrix = _inverse_affine_matrix([0.0, 0.0], angle, [1.0 * t for t in translate], scale, shear)
    dtype = img.dtype if torch.is_floating_point(img) else torch.float32
    theta = torch.tensor(matrix, dtype=dtype).reshape(1, 2, 3)
    grid = _gen_affine_grid(theta, w=img.shape[-1], h=img.shape[-2], ow=img.shape[-1], oh=img.shape[-2])
    squeeze = img.ndim < 4
    x = img.unsqueeze(0) if squeeze else img
    out = F.grid_sample(x.to(grid.dtype), grid.expand(x.shape[0], -1, -1, -1), mode="nearest", padding_mode="zeros",
                        align_corners=False)
    return out.squeeze(0) if squeeze else out


def _tv_adjust_contrast(img, contrast_factor):
    dtype = img.dtype if torch.is_floating_point(img) else torch.float32
    mean = torch.mean(img.to(dtype), dim=(-3, -2, -1), keepdim=True)
    ratio = float(contrast_factor)
    return (ratio * img + (1.0 - ratio) * mean).clamp(0, 1.0).to(img.dtype)


_stub("numba", njit=_ident, prange=range)
_sk = _stub("skimage")
_sk.morphology = _stub("skimage.morphology", disk=_disk)
_sk.io = _stub("skimage.io")
_stub("bism")
for _s in ("backends", "modules", "models", "models.spatial_embedding"):
    _stub("bism." + _s)
sys.modules["bism.models.spatial_embedding"].SpatialEmbedding = object
_y = _stub("yacs")
_y.config = _stub("yacs.config", CfgNode=dict)
_tv = _stub("torchvision")
_tv.transforms = _stub("torchvision.transforms")
_tv.transforms.functional = _stub("torchvision.transforms.functional", affine=_tv_affine,
                                  adjust_contrast=_tv_adjust_contrast)

import skoots.train.merged_transform as MT  # noqa: E402
from skoots.lib.skeleton import skeleton_to_mask as ref_skeleton_to_mask  # noqa: E402
from skoots.lib.utils import get_cached_disk_coords  # noqa: E402


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def make_cfg(**aug):
    a = dict(CROP_WIDTH=10, CROP_HEIGHT=12, CROP_DEPTH=4, FLIP_RATE=0.5, BRIGHTNESS_RATE=0.4,
             BRIGHTNESS_RANGE=[-0.1, 0.1], NOISE_GAMMA=0.1, NOISE_RATE=0.2, CONTRAST_RATE=0.33,
             CONTRAST_RANGE=[0.75, 2.0], AFFINE_RATE=0.66, AFFINE_SCALE=[0.85, 1.1], AFFINE_YAW=[-180, 180],
             AFFINE_SHEAR=[-7, 7], ELASTIC_GRID_SHAPE=(6, 6, 2), ELASTIC_GRID_MAGNITUDE=(0.05, 0.05, 0.01),
             ELASTIC_RATE=0.33, BAKE_SKELETON_ANISOTROPY=(1.0, 1.0, 3.0))
    radius = aug.pop("RADIUS", 9)
    a.update(aug)
    return AttrDict(AUGMENTATION=AttrDict(a), TRAIN=AttrDict(SKELETON_MASK_RADIUS=radius, SKELETON_MASK_FLANK_RADIUS=3))


ALL_ON = dict(FLIP_RATE=1.0, BRIGHTNESS_RATE=1.0, NOISE_RATE=1.0, CONTRAST_RATE=1.0, AFFINE_RATE=1.0, ELASTIC_RATE=1.0)
ALL_OFF = {k: 0.0 for k in ALL_ON}


def only(**on):
    d = dict(ALL_OFF)
    d.update(on)
    return d


def volume(gen, shape, n_inst, image_dtype, mask_dtype):
    """A structured image (compresses well, no two neighbours alike) and block-shaped instances with skeletons."""
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    img = ((x * 37 + y * 11 + z * 53 + (x * y) % 7) % 256).astype(np.float64)
    if image_dtype == "uint8":
        image = torch.from_numpy(img.astype(np.uint8))
    elif image_dtype == "float32":
        image = torch.from_numpy((img + 0.25).astype(np.float32))
    else:
        image = torch.from_numpy((img / 255.0).astype(np.float16))
    masks = np.zeros(shape, np.int64)
    skeletons = {}
    for k in range(1, n_inst + 1):
        lo = [int(torch.randint(0, max(1, s - 3), (1,), generator=gen)) for s in shape]
        hi = [min(s, l + int(torch.randint(3, max(4, s // 2), (1,), generator=gen))) for s, l in zip(shape, lo)]
        masks[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = k * 7        # ids well apart: 7, 14, ...
        n = int(torch.randint(2, 8, (1,), generator=gen))
        pts = torch.stack([torch.rand(n, generator=gen) * (h - l - 1) + l for l, h in zip(lo, hi)], 1)
        skeletons[k * 7] = pts.float()
    mt = {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32}[mask_dtype]
    return image.unsqueeze(0), torch.from_numpy(masks).to(mt).unsqueeze(0), skeletons


def run_reference(cfg, image, masks, skeletons, seed):
    """One reference forward with its draws and intermediate values recorded."""
    log = []
    rec = {}
    orig = (random.random, random.uniform, random.choice, torch.rand)

    def r_random():
        v = orig[0]()
        log.append(("random", v))
        return v

    def r_uniform(a, b):
        v = orig[1](a, b)
        log.append(("uniform", v))
        return v

    def r_choice(seq):
        v = orig[2](seq)
        log.append(("choice", v))
        return v

    def r_rand(*a, **k):
        v = orig[3](*a, **k)
        log.append(("rand", v.clone()))
        return v

    def elastic(self, image, masks, skeletons):
        i, m, _ = MT.elastic_deform(image.unsqueeze(0), masks.unsqueeze(0), skeleton={})
        return i.squeeze(0), m.squeeze(0), skeletons

    def wrap(name):
        fn = getattr(MT.TransformFromCfg, name)

        def w(self, image, *a):
            if "geom" not in rec:
                rec["geom"] = image.clone().float()
            return fn(self, image, *a)
        return w

    def s2m(skel, shape, device=None, radius=7, flank_radius=3):
        rec["points"] = {k: v.clone() for k, v in skel.items()}
        if -1 in skel:
            return torch.zeros((1,) + tuple(shape))
        return ref_skeleton_to_mask(skel, shape, device=device, radius=radius, flank_radius=flank_radius)

    saved = {n: getattr(MT.TransformFromCfg, n) for n in ("_elastic", "_invert", "_brightness", "_contrast", "_noise",
                                                          "_normalize")}
    saved_mod = (MT.skeleton_to_mask, MT.bake_skeleton)
    try:
        MT.TransformFromCfg._elastic = elastic
        for n in ("_invert", "_brightness", "_contrast", "_noise", "_normalize"):
            setattr(MT.TransformFromCfg, n, wrap(n))
        MT.skeleton_to_mask, MT.bake_skeleton = s2m, (lambda *a, **k: None)
        random.random, random.uniform, random.choice, torch.rand = r_random, r_uniform, r_choice, r_rand
        random.seed(seed)
        torch.manual_seed(seed)
        t = MT.TransformFromCfg(cfg, torch.device("cpu"))
        out = t({"image": image.clone(), "masks": masks.clone(),
                 "skeletons": {k: v.clone() for k, v in skeletons.items()}})
    finally:
        random.random, random.uniform, random.choice, torch.rand = orig
        for n, fn in saved.items():
            setattr(MT.TransformFromCfg, n, fn)
        MT.skeleton_to_mask, MT.bake_skeleton = saved_mod
    return out, rec, log


def plan_fields(cfg, log):
    """The draw log, parsed in forward's order, as AugmentPlan fields."""
    a = cfg.AUGMENTATION
    it = iter(log)
    nxt = lambda kind: (lambda e: e[1] if e[0] == kind else (_ for _ in ()).throw(AssertionError(e[0])))(next(it))  # noqa: E731
    f = {"key": nxt("choice")}
    f["elastic"] = nxt("random") < a.ELASTIC_RATE
    f["elastic_field"] = nxt("rand") if f["elastic"] else None
    f["affine"] = nxt("random") < a.AFFINE_RATE
    f["angle"], f["shear"], f["scale"] = (nxt("uniform"), nxt("uniform"), nxt("uniform")) if f["affine"] else (0.0, 0.0, 1.0)
    for ax in "xyz":
        f["flip_" + ax] = nxt("random") < a.FLIP_RATE
    f["invert"] = nxt("random") < a.BRIGHTNESS_RATE
    f["brightness"] = nxt("random") < a.BRIGHTNESS_RATE
    f["brightness_val"] = nxt("uniform") if f["brightness"] else 0.0
    f["contrast"] = nxt("random") < a.CONTRAST_RATE
    f["contrast_val"] = nxt("uniform") if f["contrast"] else 1.0
    f["noise"] = nxt("rand") if nxt("random") < a.NOISE_RATE else None
    assert next(it, None) is None
    return f


FLAGS = ("elastic", "affine", "flip_x", "flip_y", "flip_z", "invert", "brightness", "contrast")
VALUES = ("angle", "shear", "scale", "brightness_val", "contrast_val")
CFG_KEYS = ("CROP_WIDTH", "CROP_HEIGHT", "CROP_DEPTH", "FLIP_RATE", "BRIGHTNESS_RATE", "NOISE_GAMMA", "NOISE_RATE",
            "CONTRAST_RATE", "AFFINE_RATE", "ELASTIC_RATE")


def main():
    torch.set_num_threads(8)
    gen = torch.Generator().manual_seed(2024)
    vols = {
        "A": volume(gen, (24, 22, 9), 3, "uint8", "int16"),
        "Af32": None, "Af16": None,
        "B": volume(gen, (316, 18, 7), 3, "uint8", "uint8"),       # crop 1 is narrower than the volume in x
        "C": volume(gen, (7, 9, 3), 2, "uint8", "int32"),          # smaller than the crop
        "L": volume(gen, (32, 28, 11), 4, "uint8", "int16"),
    }
    a_img, a_msk, a_sk = vols["A"]
    X, Y, Z = a_img.shape[1:]
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    smooth = torch.from_numpy((x * 37 + y * 11 + z * 53 + (x * y) % 7) % 256).unsqueeze(0)
    vols["Af32"] = ((smooth.float() + 0.25), a_msk.to(torch.int32), a_sk)
    vols["Af16"] = ((smooth.double() / 255.0).half(), a_msk, a_sk)
    big = dict(CROP_WIDTH=24, CROP_HEIGHT=20, CROP_DEPTH=8)
    cases = [  # (volume, cfg overrides, seed)
        ("A", ALL_OFF, 1), ("A", only(ELASTIC_RATE=1.0), 2), ("A", only(AFFINE_RATE=1.0), 3),
        ("A", only(FLIP_RATE=1.0), 4), ("A", only(BRIGHTNESS_RATE=1.0), 5), ("A", only(CONTRAST_RATE=1.0), 6),
        ("A", only(NOISE_RATE=1.0), 7), ("A", ALL_ON, 8), ("A", {}, 11), ("A", {}, 12), ("A", {}, 13),
        ("A", dict(RADIUS=7), 14),
        ("Af32", only(ELASTIC_RATE=1.0, AFFINE_RATE=1.0, FLIP_RATE=1.0, BRIGHTNESS_RATE=1.0), 21),
        ("Af16", only(ELASTIC_RATE=1.0, CONTRAST_RATE=1.0), 22),
        ("B", ALL_ON, 31), ("B", {}, 32),
        ("C", ALL_ON, 41), ("C", only(AFFINE_RATE=1.0, FLIP_RATE=1.0), 42),
        ("L", dict(big, **only(ELASTIC_RATE=1.0)), 51), ("L", dict(big, **only(AFFINE_RATE=1.0)), 52),
        ("L", dict(big, **dict(ALL_ON, NOISE_RATE=0.0)), 53), ("L", dict(big), 54),
        ("A", only(AFFINE_RATE=1.0, FLIP_RATE=1.0, BRIGHTNESS_RATE=1.0), 61),   # the -1 key
    ]
    out = {"n": np.array(len(cases)), "flag_names": np.array(FLAGS), "value_names": np.array(VALUES),
           "cfg_names": np.array(CFG_KEYS)}
    for vname, (image, masks, _) in vols.items():   # each input volume once
        out[f"vol_{vname}_image"], out[f"vol_{vname}_masks"] = image.numpy(), masks.numpy()
    for i, (vname, over, seed) in enumerate(cases):
        image, masks, skel = vols[vname]
        if i == len(cases) - 1:
            skel = {-1: skel[next(iter(skel))].clone()}
        cfg = make_cfg(**over)
        res, rec, log = run_reference(cfg, image, masks, skel, seed)
        f = plan_fields(cfg, log)
        keys = list(skel.keys())
        pts_out = rec["points"]
        pre = f"c{i}_"
        out.update({
            pre + "volume": np.array(vname),
            pre + "keys": np.array(keys, np.int64), pre + "counts": np.array([len(skel[k]) for k in keys]),
            pre + "points_in": torch.cat([skel[k] for k in keys]).numpy(),
            pre + "cfg": np.array([float(cfg.AUGMENTATION[k]) for k in CFG_KEYS]),
            pre + "radius": np.array([cfg.TRAIN.SKELETON_MASK_RADIUS, cfg.TRAIN.SKELETON_MASK_FLANK_RADIUS]),
            pre + "seed": np.array(seed),
            pre + "key": np.array(f["key"]), pre + "flags": np.array([bool(f[k]) for k in FLAGS]),
            pre + "values": np.array([float(f[k]) for k in VALUES]),
            pre + "geom": rec["geom"].numpy(), pre + "image": res["image"].float().numpy(),
            pre + "masks": res["masks"].numpy().astype(np.int32),
            pre + "points": torch.cat([pts_out[k].float() for k in keys]).numpy(),
            pre + "skele_masks": res["skele_masks"].float().numpy(),
        })
        if f["elastic_field"] is not None:
            out[pre + "elastic_field"] = f["elastic_field"].numpy()
        if f["noise"] is not None:
            out[pre + "noise"] = f["noise"].numpy()
        print(i, vname, seed, "flags", [k for k in FLAGS if f[k]], "noise", f["noise"] is not None,
              "out", tuple(res["image"].shape))

    # skeleton_to_mask alone: points near the edges, out of range, negative fractions (truncate to 0)
    g = torch.Generator().manual_seed(77)
    shape = (20, 18, 5)
    pts = {3: torch.tensor([[0.0, 0.0, 0.0], [19.6, 17.2, 4.9], [-0.5, 3.3, 2.0], [10.0, 10.0, 5.0]]),
           5: torch.rand((9, 3), generator=g) * torch.tensor([26.0, 24.0, 7.0]) - torch.tensor([3.0, 3.0, 1.0]),
           8: torch.tensor([[-30.0, 5.0, 2.0], [5.0, 40.0, 2.0], [5.0, 5.0, -2.5], [5.0, 5.0, 6.0]])}
    out["s2m_points"] = torch.cat(list(pts.values())).numpy()
    out["s2m_counts"] = np.array([len(v) for v in pts.values()])
    out["s2m_shape"] = np.array(shape)
    for r, fr in ((7, 3), (9, 3)):
        out[f"s2m_{r}_{fr}"] = ref_skeleton_to_mask(pts, shape, device="cpu", radius=r, flank_radius=fr).numpy()
        out[f"disk_{r}_{fr}"] = get_cached_disk_coords("cpu", r, fr).numpy()

    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(f"augment.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
