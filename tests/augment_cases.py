"""The cases, seeded inputs and references that tests/test_augment_cases_cpu.py and tests/test_hip_augment_cases.py share
(numpy and torch on the CPU only): sk_aug_resample, sk_aug_intensity and sk_skeleton_to_mask (skoots_amd/csrc/augment.hip)
and sk_bake_skeleton / sk_average_baked_skeletons (skoots_amd/csrc/bake.hip).

tests/golden/augment.npz (23 cases, 23 898 voxels, the largest output 24 x 20 x 8) and tests/golden/bake.npz (one
26 x 22 x 12 volume) never reach the second trip of a block-stride loop, more than 16 normalise partials, a crop-1 origin
inside a device-resident volume, five of the nine dtype pairs, a field whose h and w differ, an extent of 1, or the
4096-block cap of the streaming kernels.  The cases here do, at the smallest extents that reach each path.

The references are written from include/skoots_hip.h, DESIGN.md section 11 and the torchvision restatement of
tests/golden/make_augment_golden.py; they never call the library:

    geometry_nominal64   the gather in vectorised float64: flips -> crop-2 origin -> inverse affine per z-slice (nearest,
                         align_corners False) -> elastic map (trilinear field, nearest, align_corners True) -> crop-1 origin;
                         nearest = round-half-even, 0 outside.  Also the voxels where some stage's coordinate lies within EPS
                         of a rounding boundary: only there may fp32 arithmetic pick the other sample.
    voxel_candidates     for ONE voxel, every (image, mask) value it can take when each such coordinate rounds either way
    geometry_torch32     the same chain as torch CPU ops in fp32 (F.interpolate, linspace, grid_sample); it pins the float64
                         reference to the fixture, on the CPU only
    intensity64          invert, brightness, contrast (one mean per z-slice), noise, normalise, all in float64
    skeleton_to_mask_ref fp32 point + offset, truncation toward zero, inside iff -1 < s < extent
    bake_ref / average_ref   oracle/bake.py (float64, first minimal point wins; entries > 0 count)

Every reference takes a ``mut`` naming ONE deliberate error (GEOMETRY_MUTATIONS, INTENSITY_MUTATIONS, "last_wins", "ne0");
tests/test_augment_cases_cpu.py shows that each leaves the GPU test's bound on the case built for it.

EPS and the cap of excused voxels are those of tests/test_hip_augment.py.  EPS has been validated for crop-1 extents up to
316 (the fp32 coordinate error grows with the extent), so no case here has a larger one.
"""
import collections
import functools
import math
from itertools import product

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-4
K_BLOCK, MAX_BLOCKS_PER_Z = 256, 64          # augment.hip: threads per block, partial sums per z-slice
STREAM_GRID_CAP = 4096                       # common.h stream_grid: blocks of 256 threads
MAX_EXTENT = 316
DEFAULT_MAGNITUDE = (0.01, 0.05, 0.05)       # (z, y, x), transforms.ELASTIC_MAGNITUDE_ZYX

GEOMETRY_MUTATIONS = ("field_hw_swapped", "floor_half")
INTENSITY_MUTATIONS = ("std_n", "no_last_partial", "no_second_trip")


def cap(voxels):
    """how many voxels of a case may take the other sample of a rounding boundary"""
    return max(1, int(EPS * voxels))


def blocks_per_z(plane):
    return min(max((plane + K_BLOCK - 1) // K_BLOCK, 1), MAX_BLOCKS_PER_Z)


def r32(x):
    """a host parameter as the library receives it: rounded to a C float"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------ geometry
# src: the source volume (X, Y, Z); o1 / e1: origin and extents of the crop-1 window in it; o2 / e2: origin of the output in
# the crop-1 window and its extents; flips (x, y, z); affine None or (angle, shear, scale); field None or float (3, fd, fh, fw)
# -- fd along x, fh along y, fw along z, channel 0 moves z, 1 y, 2 x; magnitude (z, y, x)
Geo = collections.namedtuple("Geo", "src o1 e1 o2 e2 flips affine field magnitude")


def params_from_plan(t, image_shape, g, plan):
    """the Geo of TransformFromCfg ``t`` for an image (1, X, Y, Z), ``g = t.geometry(...)`` and an AugmentPlan"""
    e1, e2 = t.crop_extents(image_shape)
    field = plan.elastic_field.double().cpu().numpy()[0] if plan.elastic else None
    return Geo(tuple(int(s) for s in image_shape[1:]), tuple(g["crop1"]), e1, tuple(g["crop2"]), e2,
               (bool(plan.flip_x), bool(plan.flip_y), bool(plan.flip_z)),
               (plan.angle, plan.shear, plan.scale) if plan.affine else None, field, DEFAULT_MAGNITUDE)


def _rss(angle, shear, scale):
    """rows [x (3), y (3)] of torchvision's inverse affine matrix about (0, 0), shear [shear, 0], no translation"""
    rot, sx = math.radians(angle), math.radians(shear)
    a = math.cos(rot)
    b = -math.cos(rot) * math.tan(sx) - math.sin(rot)
    c = math.sin(rot)
    d = -math.sin(rot) * math.tan(sx) + math.cos(rot)
    return [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]


def _near(c):
    """the coordinate lies within EPS of a rounding boundary (k + 0.5)"""
    return np.abs(c - np.floor(c) - 0.5) < EPS


def _lin64(dst, n_in, n_out):
    """upsample_trilinear3d, align_corners False, along one axis (vectorised): index, step to the upper sample, weight"""
    src = np.maximum(n_in / n_out * (dst + 0.5) - 0.5, 0.0)
    i0 = src.astype(np.int64)
    return i0, (i0 < n_in - 1).astype(np.int64), src - i0


def _linspace64(i, n):
    return np.full(np.shape(i), -1.0) if n == 1 else -1.0 + 2.0 * i / (n - 1)


def _swap_field_hw(f):
    """what a kernel reads whose h stride is field_h where it should be field_w (past the end it wraps here; a kernel
    would read whatever lies there)"""
    c, fd, fh, fw = f.shape
    a, b, w = np.meshgrid(np.arange(fd), np.arange(fh), np.arange(fw), indexing="ij")
    return np.ascontiguousarray(f).reshape(c, -1)[:, (a * fh * fw + b * fh + w) % (fd * fh * fw)]


Nominal = collections.namedtuple("Nominal", "image masks near inside")


def geometry_nominal64(p, image, masks, mut=None):
    """Nominal(image fp32 (w2, h2, d2), masks int32, near bool, inside bool) of the gather sk_aug_resample documents, every
    coordinate in float64.  image / masks are the source volume (X, Y, Z) of any accepted dtype; values are looked up, so
    they are exact.  ``near``: some stage's coordinate of that voxel lies within EPS of a rounding boundary."""
    rnd = (lambda c: np.floor(c + 0.5)) if mut == "floor_half" else np.rint
    (w1, h1, d1), (w2, h2, d2) = p.e1, p.e2
    x, y, z = np.meshgrid(np.arange(w2), np.arange(h2), np.arange(d2), indexing="ij")
    xa = (w2 - 1 - x if p.flips[0] else x) + p.o2[0]
    ya = (h2 - 1 - y if p.flips[1] else y) + p.o2[1]
    za = (d2 - 1 - z if p.flips[2] else z) + p.o2[2]
    inside = np.ones(x.shape, bool)
    near = np.zeros(x.shape, bool)
    if p.affine is not None:
        m = _rss(*p.affine)
        bx, by = ya - 0.5 * h1 + 0.5, xa - 0.5 * w1 + 0.5
        gx = (bx * m[0] + by * m[1]) / (0.5 * h1)
        gy = (bx * m[3] + by * m[4]) / (0.5 * w1)
        cx, cy = ((gy + 1) * w1 - 1) / 2, ((gx + 1) * h1 - 1) / 2
        near |= _near(cx) | _near(cy)
        xa, ya = rnd(cx).astype(np.int64), rnd(cy).astype(np.int64)
        inside &= (xa >= 0) & (xa < w1) & (ya >= 0) & (ya < h1)
        xa, ya = np.where(inside, xa, 0), np.where(inside, ya, 0)
    if p.field is not None:
        f = np.asarray(p.field, np.float64)
        if mut == "field_hw_swapped":
            f = _swap_field_hw(f)
        _, fd, fh, fw = f.shape
        (a0, ap, la), (b0, bp, lb), (c0, cp, lc) = _lin64(xa, fd, w1), _lin64(ya, fh, h1), _lin64(za, fw, d1)
        off = np.zeros((3,) + x.shape)
        for da, wa in ((0, 1 - la), (ap, la)):
            for db, wb in ((0, 1 - lb), (bp, lb)):
                for dc, wc in ((0, 1 - lc), (cp, lc)):
                    off += wa * wb * wc * f[:, a0 + da, b0 + db, c0 + dc]
        gz = _linspace64(za, d1) + off[0] * p.magnitude[0]
        gy = _linspace64(ya, h1) + off[1] * p.magnitude[1]
        gx = _linspace64(xa, w1) + off[2] * p.magnitude[2]
        cx, cy, cz = (gx + 1) / 2 * (w1 - 1), (gy + 1) / 2 * (h1 - 1), (gz + 1) / 2 * (d1 - 1)
        near |= inside & (_near(cx) | _near(cy) | _near(cz))
        xe, ye, ze = rnd(cx).astype(np.int64), rnd(cy).astype(np.int64), rnd(cz).astype(np.int64)
        inside &= (xe >= 0) & (xe < w1) & (ye >= 0) & (ye < h1) & (ze >= 0) & (ze < d1)
        xa, ya, za = np.where(inside, xe, 0), np.where(inside, ye, 0), np.where(inside, ze, 0)
    s = (xa + p.o1[0], ya + p.o1[1], za + p.o1[2])
    out_i = np.where(inside, np.asarray(image)[s].astype(np.float32), np.float32(0))
    out_m = np.where(inside, np.asarray(masks)[s].astype(np.int32), np.int32(0))
    return Nominal(out_i.astype(np.float32), out_m.astype(np.int32), near, inside)


def _cands(c):
    f = math.floor(c)
    if abs(c - f - 0.5) < EPS:
        return [f, f + 1]
    return [int(np.rint(c))]


def _lin64_scalar(dst, n_in, n_out):
    src = max(n_in / n_out * (dst + 0.5) - 0.5, 0.0)
    i0 = int(src)
    return i0, (1 if i0 < n_in - 1 else 0), src - i0


def voxel_candidates(p, image, masks, x, y, z):
    """Every (image, mask) value the output voxel (x, y, z) can take when each stage's float64 coordinate that lies
    within EPS of a rounding boundary may round either way.  image / masks: the source volume (X, Y, Z)."""
    (w1, h1, d1), (w2, h2, d2) = p.e1, p.e2
    x0, y0, z0 = p.o1
    cx0, cy0, cz0 = p.o2
    xa = (w2 - 1 - x if p.flips[0] else x) + cx0
    ya = (h2 - 1 - y if p.flips[1] else y) + cy0
    za = (d2 - 1 - z if p.flips[2] else z) + cz0
    pos = [(xa, ya, za)]
    if p.affine is not None:
        m = _rss(*p.affine)
        bx, by = ya - 0.5 * h1 + 0.5, xa - 0.5 * w1 + 0.5
        gx = (bx * m[0] + by * m[1]) / (0.5 * h1)
        gy = (bx * m[3] + by * m[4]) / (0.5 * w1)
        pos = [(sx, sy, za) for sx in _cands(((gy + 1) * w1 - 1) / 2) for sy in _cands(((gx + 1) * h1 - 1) / 2)]
    if p.field is not None:
        f = np.asarray(p.field, np.float64)
        _, fd, fh, fw = f.shape
        out = []
        for (xe, ye, ze) in pos:
            if not (0 <= xe < w1 and 0 <= ye < h1):
                out.append(None)
                continue
            (a0, ap, la), (b0, bp, lb), (c0, cp, lc) = (_lin64_scalar(xe, fd, w1), _lin64_scalar(ye, fh, h1),
                                                        _lin64_scalar(ze, fw, d1))
            off = []
            for c in range(3):
                v = 0.0
                for da, wa in ((0, 1 - la), (ap, la)):
                    for db, wb in ((0, 1 - lb), (bp, lb)):
                        for dc, wc in ((0, 1 - lc), (cp, lc)):
                            v += wa * wb * wc * f[c, a0 + da, b0 + db, c0 + dc]
                off.append(v * p.magnitude[c])
            lin = lambda i, n: -1.0 if n == 1 else -1.0 + 2.0 * i / (n - 1)  # noqa: E731
            gz, gy, gx = lin(ze, d1) + off[0], lin(ye, h1) + off[1], lin(xe, w1) + off[2]
            out += list(product(_cands((gx + 1) / 2 * (w1 - 1)), _cands((gy + 1) / 2 * (h1 - 1)),
                                _cands((gz + 1) / 2 * (d1 - 1))))
        pos = out
    vals = set()
    for q in pos:
        if q is None or not (0 <= q[0] < w1 and 0 <= q[1] < h1 and 0 <= q[2] < d1):
            vals.add((0.0, 0))
        else:
            s = (q[0] + x0, q[1] + y0, q[2] + z0)
            vals.add((float(image[s]), int(masks[s])))
    return vals


def excused_voxels(p, image, masks, got_i, got_m, nom):
    """The voxels where (got_i, got_m) differs from the nominal, each checked: it must be flagged near a boundary and its
    pair must be one of voxel_candidates.  Returns their list; the caller holds its length to cap()."""
    bad = np.argwhere((got_i.view(np.int32) != nom.image.view(np.int32)) | (got_m != nom.masks))
    img32 = np.asarray(image).astype(np.float32)
    for x, y, z in bad:
        assert nom.near[x, y, z], f"voxel {(x, y, z)}: {got_i[x, y, z]} / {got_m[x, y, z]} vs nominal " \
                                  f"{nom.image[x, y, z]} / {nom.masks[x, y, z]}, not at a rounding boundary"
        vals = voxel_candidates(p, img32, masks, int(x), int(y), int(z))
        assert (float(got_i[x, y, z]), int(got_m[x, y, z])) in vals, ((x, y, z), got_i[x, y, z], got_m[x, y, z], vals)
    return [tuple(int(v) for v in b) for b in bad]


def image_theta64(p):
    """the six numbers sk_aug_resample takes as theta, from float64 (the library is handed transforms._image_theta)"""
    m = _rss(*p.affine)
    return [m[0] / (0.5 * p.e1[1]), m[1] / (0.5 * p.e1[1]), 0.0, m[3] / (0.5 * p.e1[0]), m[4] / (0.5 * p.e1[0]), 0.0]


def _affine_grid32(affine, w, h):
    """torchvision's tensor path as tests/golden/make_augment_golden.py states it: theta of the inverse matrix in fp32,
    base grid of pixel centres, theta^T over (w / 2, h / 2), bmm -> (1, h, w, 2)"""
    theta = torch.tensor(_rss(*affine), dtype=torch.float32).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32)
    return base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)


def geometry_torch32(p, image, masks):
    """(image fp32, masks int32) of the chain as torch CPU ops in fp32: crop 1; F.interpolate(field, trilinear) * magnitude
    + the linspace grid, grid_sample(nearest, align_corners True); the affine grid per z-slice, grid_sample(nearest,
    align_corners False); crop 2; flips.  The stages gather voxel NUMBERS (exact in fp32 below 2^24, 0 = outside), which are
    then looked up, so every dtype goes through unchanged."""
    (w1, h1, d1), (w2, h2, d2) = p.e1, p.e2
    n1 = w1 * h1 * d1
    assert n1 < (1 << 24)
    idx = torch.arange(1, n1 + 1, dtype=torch.float32).reshape(1, 1, w1, h1, d1)
    if p.field is not None:
        f = torch.from_numpy(np.asarray(p.field, np.float32))[None]
        off = F.interpolate(f, (w1, h1, d1), mode="trilinear").permute(0, 2, 3, 4, 1)
        off = off.mul(torch.tensor(p.magnitude, dtype=torch.float32).view(1, 1, 1, 1, 3))
        mx, my, mz = torch.meshgrid([torch.linspace(-1, 1, n) for n in (w1, h1, d1)], indexing="ij")
        grid = (torch.stack((mz, my, mx), 3).unsqueeze(0) + off).float()
        idx = F.grid_sample(idx, grid, mode="nearest", padding_mode="zeros", align_corners=True)
    if p.affine is not None:
        sl = idx[0].permute(0, 3, 1, 2)                                   # (1, Z, H = X, W = Y)
        sl = F.grid_sample(sl, _affine_grid32(p.affine, h1, w1), mode="nearest", padding_mode="zeros", align_corners=False)
        idx = sl.permute(0, 2, 3, 1).unsqueeze(0)
    idx = idx[0, 0, p.o2[0]:p.o2[0] + w2, p.o2[1]:p.o2[1] + h2, p.o2[2]:p.o2[2] + d2]
    idx = idx.flip([a for a in range(3) if p.flips[a]]) if any(p.flips) else idx
    k = idx.numpy().astype(np.int64)
    inside, k = k > 0, np.maximum(k - 1, 0)
    s = (k // (h1 * d1) + p.o1[0], k // d1 % h1 + p.o1[1], k % d1 + p.o1[2])
    return (np.where(inside, np.asarray(image)[s].astype(np.float32), np.float32(0)).astype(np.float32),
            np.where(inside, np.asarray(masks)[s].astype(np.int32), np.int32(0)).astype(np.int32))


# the geometric cases -----------------------------------------------------------------------------------------------
# name -> dict(src, e1 (default src), o1, e2 (default e1), o2, flips, affine, field (shape), magnitude, img, msk, seed)
_ALL, _NO = (True, True, True), (False, False, False)
_BIG_MAG = (0.3, 0.2, 0.25)     # three distinct values, large enough that a tiny window has zero-filled voxels
_G = collections.OrderedDict()


def _geo(name, src, **kw):
    _G[name] = dict(dict(src=src, e1=src, o1=(0, 0, 0), e2=None, o2=(0, 0, 0), flips=_NO, affine=None, field=None,
                         magnitude=DEFAULT_MAGNITUDE, img="uint8", msk="int16", seed=1), **kw)


# strided planes (crop 1 = volume): 128 x 128 = 64 * 256 columns, exactly one full trip; 129 x 128 a partial second trip;
# 145 x 113 = 16 385 columns, one column in the second trip; 224 x 224 three trips and a partial fourth.
# Stage combinations and the corners of the configured affine ranges are spread over them.  The axis-aligned angles sit on
# odd extents: with an even extent the centre is a half-integer and the rational scales 0.85 and 1.1 put whole rows of
# coordinates exactly on a rounding boundary (42.5 / 0.85 = 50), which is the ties case's business, not theirs.
_geo("128x128x2-elastic", (128, 128, 2), field=(2, 6, 6), seed=2)
_geo("128x128x2-affine", (128, 128, 2), affine=(61.3, 7.0, 0.85), seed=3)
_geo("129x128x3-both", (129, 128, 3), affine=(31.7, -7.0, 1.1), field=(2, 6, 6), seed=4)
_geo("129x128x3-affine", (129, 128, 3), affine=(-61.3, -7.0, 1.1), seed=5)
_geo("145x113x3-affine180", (145, 113, 3), affine=(180.0, 7.0, 0.85), seed=5)
_geo("145x113x3-affine-180", (145, 113, 3), affine=(-180.0, -7.0, 0.85), seed=6)
_geo("145x113x3-affine90", (145, 113, 3), affine=(90.0, 7.0, 0.85), seed=3)
_geo("145x113x3-both-flips", (145, 113, 3), affine=(-123.4, 3.3, 0.85), field=(2, 6, 6), flips=_ALL, seed=7)
_geo("224x224x2-both-flips", (224, 224, 2), affine=(77.7, -4.2, 1.1), field=(2, 6, 6), flips=_ALL, seed=8)
_geo("224x224x2-elastic", (224, 224, 2), field=(2, 6, 6), seed=9)
# a device-resident source with crop 1 at a non-zero origin on all three axes and crop 2 at a non-zero origin in it: what
# TransformFromCfg (crop 8 x 6 x 3) makes of an instance centred at ORIGINS_CENTRE, near the volume's upper x face, so that
# the output lies at the edge of the crop-1 window and the affine stage zero-fills part of it
ORIGINS_CENTRE = (325.0, 164.0, 3.0)
for _fl, _nm in ((_NO, ""), (_ALL, "-flips")):
    _geo("330x320x6-origins" + _nm, (330, 320, 6), o1=(22, 11, 2), e1=(308, 306, 3), o2=(299, 150, 0), e2=(8, 6, 3),
         affine=(12.5, 5.0, 0.95), field=(2, 6, 6), flips=_fl, seed=10)
_geo("330x320x6-origins-plain", (330, 320, 6), o1=(17, 11, 2), e1=(308, 306, 3), o2=(151, 148, 0), e2=(8, 6, 3), seed=11)
# all nine dtype pairs on a (9, 7, 3) output
for _i, _m in product(("uint8", "float16", "float32"), ("uint8", "int16", "int32")):
    _geo(f"9x7x3-{_i}-{_m}", (12, 10, 4), o1=(2, 1, 1), e1=(9, 8, 3), o2=(0, 1, 0), e2=(9, 7, 3), affine=(20.0, 4.0, 0.9),
         field=(2, 6, 6), magnitude=_BIG_MAG, flips=(True, False, True), img=_i, msk=_m, seed=12)
# field shapes: one sample per channel, and h != w (a swap of the two strides shows)
_geo("21x19x6-field111", (21, 19, 6), field=(1, 1, 1), magnitude=_BIG_MAG, seed=18)
_geo("21x19x6-field354", (21, 19, 6), field=(3, 5, 4), magnitude=_BIG_MAG, seed=14)
# degenerate outputs: an extent of 1 (linspace of one point), a plane under 256 columns, each flip combination on odd and
# on even extents
_geo("1x9x4-elastic", (1, 9, 4), field=(2, 6, 6), magnitude=_BIG_MAG, seed=15)
_geo("9x1x4-elastic", (9, 1, 4), field=(2, 6, 6), magnitude=_BIG_MAG, seed=16)
_geo("9x7x1-elastic", (9, 7, 1), field=(2, 6, 6), magnitude=_BIG_MAG, seed=17)
_geo("3x5x2-both", (3, 5, 2), affine=(30.0, 2.0, 0.85), field=(2, 6, 6), magnitude=_BIG_MAG, seed=18)
for _f in product((False, True), repeat=3):
    _tag = "".join(a for a, on in zip("xyz", _f) if on) or "none"
    _geo(f"5x4x3-flip-{_tag}", (5, 4, 3), flips=_f, seed=19)
    _geo(f"4x5x2-flip-{_tag}", (4, 5, 2), flips=_f, seed=20)
# exact ties: scale 1/2 on a 16 x 16 window puts EVERY coordinate at k + 0.5, exactly in fp32 and in float64 (all factors
# are powers of two): round-half-even takes the even sample, floor(c + 0.5) the upper one
_geo("16x16x2-ties", (16, 16, 2), affine=(0.0, 0.0, 0.5), seed=21)

GEO_NAMES = list(_G)
STRIDED = [n for n in GEO_NAMES if n.split("-")[0] in ("128x128x2", "129x128x3", "145x113x3", "224x224x2")]
FLIP_ONLY = [n for n in GEO_NAMES if "-flip-" in n]
_MASK_IDS = {"uint8": (0, 1, 7, 255), "int16": (0, 5, 32767, -3), "int32": (0, 9, (1 << 24) - 1, 70000)}


@functools.lru_cache(maxsize=None)
def geo_case(name):
    """(Geo, image (X, Y, Z), masks (X, Y, Z)) of a geometric case: a random image (no two neighbours alike but by chance;
    fp16 / fp32 hold non-integers) and a random id per voxel, among them the extremes of the dtype"""
    c = _G[name]
    rs = np.random.RandomState(1000 + c["seed"])
    X, Y, Z = c["src"]
    if c["img"] == "uint8":
        image = rs.randint(0, 256, (X, Y, Z)).astype(np.uint8)
    else:
        image = (rs.rand(X, Y, Z) * 255.0).astype(c["img"])
    masks = np.asarray(_MASK_IDS[c["msk"]], c["msk"])[rs.randint(0, 4, (X, Y, Z))]
    field = None if c["field"] is None else rs.rand(3, *c["field"]).astype(np.float32)
    e1 = c["e1"]
    p = Geo(c["src"], c["o1"], e1, c["o2"], c["e2"] or e1, c["flips"], c["affine"], field, c["magnitude"])
    assert max(e1) <= MAX_EXTENT
    image.setflags(write=False)
    masks.setflags(write=False)
    return p, image, masks


@functools.lru_cache(maxsize=None)
def geo_nominal(name):
    p, image, masks = geo_case(name)
    return geometry_nominal64(p, image, masks)


# ------------------------------------------------------------------------------------------------------ intensity
def intensity64(v, invert=False, brightness=None, contrast=None, noise=None, gamma=0.0, own_mean=False, mean=0.0,
                own_std=False, std=1.0, mut=None, upto="end"):
    """The intensity chain on the geometric image ``v`` (w2, h2, d2), all in float64: invert (255 - v), brightness
    (clamp(v + b, 0, 255)), contrast (t = v / 255, one mean of t per z-slice, clamp(r t + (1 - r) mean, 0, 1) * 255),
    + noise * gamma, (v - mean) / std with the image's own mean / unbiased std where asked.  brightness, contrast, gamma,
    mean and std are the C floats the library receives.  ``upto="noise"`` stops before the normalisation."""
    v = np.asarray(v, np.float64).copy()
    w2, h2, d2 = v.shape
    if invert:
        v = 255.0 - v
    if brightness is not None:
        v = np.clip(v + r32(brightness), 0.0, 255.0)
    if contrast is not None:
        r = r32(contrast)
        t = (v / 255.0).reshape(w2 * h2, d2)
        col = np.arange(w2 * h2)
        nb = blocks_per_z(w2 * h2)
        use = np.ones(w2 * h2, bool)
        if mut == "no_last_partial":
            use = (col // K_BLOCK) % nb != nb - 1
        elif mut == "no_second_trip":
            use = col < nb * K_BLOCK
        m = t[use].sum(0) / (w2 * h2)
        u = np.clip(r * t + (1.0 - r) * m[None], 0.0, 1.0) * 255.0
        if mut == "no_second_trip":
            u[~use] = t[~use] * 255.0
        v = u.reshape(w2, h2, d2)
    if noise is not None:
        v = v + np.asarray(noise, np.float64) * r32(gamma)
    if upto == "noise":
        return v
    n = v.size
    mu = v.mean() if own_mean else r32(mean)
    if own_std:
        sd = math.sqrt(((v - v.mean()) ** 2).sum() / (n if mut == "std_n" else n - 1))
    else:
        sd = r32(std)
    return (v - mu) / sd


# fp32 roundings of the kernel's chain, stage by stage (augment.hip); each is at most 2^-24 of the value it rounds, and the
# values are bounded by 255 before the normalisation (t, u and the mean are bounded by 1 and scaled by 255 at the end):
#   invert      v - 255                                      1   (* -1 is exact)
#   brightness  v + b                                        1
#   contrast    t = v / 255; r t; (float)(1 - r); the mean's elements v / 255; (float) mean; (1 - r) mean; the sum; * 255     8
#   noise       noise * gamma; the add                       2
#   normalise   (float) mean; (float) std; v - mean; / std   4, on values of magnitude 255 / std
ROUNDINGS = {"invert": 1, "brightness": 1, "contrast": 8, "noise": 2, "normalise": 4}
U = 2.0 ** -24


def intensity_tolerance(invert=False, brightness=None, contrast=None, noise=None, std_used=1.0, **_):
    """roundings of the stages that run * 2^-24 * the magnitude bound (255 before normalisation, 255 / std after)"""
    n = ROUNDINGS["normalise"] + (ROUNDINGS["invert"] if invert else 0) + (ROUNDINGS["brightness"] if brightness is not None else 0) \
        + (ROUNDINGS["contrast"] if contrast is not None else 0) + (ROUNDINGS["noise"] if noise is not None else 0)
    return n * U * 255.0 / std_used


INTENSITY_SHAPES = {"129x128x5": (129, 128, 5), "4x4x300": (4, 4, 300), "9x7x3": (9, 7, 3)}
# name -> keyword arguments of intensity64 (noise: True = drawn for the shape)
INTENSITY_STAGES = collections.OrderedDict([
    ("none", dict()),
    ("invert", dict(invert=True)),
    ("bright+", dict(brightness=40.0)),                      # clamps at 255
    ("bright-", dict(brightness=-40.0)),                     # clamps at 0
    ("contrast0.75", dict(contrast=0.75)),
    ("contrast2", dict(contrast=2.0)),                       # both clamp ends reached
    ("noise", dict(noise=True, gamma=0.1)),
    ("own-mean", dict(own_mean=True)),
    ("own-std", dict(own_std=True, mean=3.0)),
    ("own-both", dict(own_mean=True, own_std=True)),
    ("given", dict(mean=3.0, std=2.0)),
    ("all", dict(invert=True, brightness=-25.5, contrast=2.0, noise=True, gamma=0.1, own_mean=True, own_std=True)),
    ("all-given", dict(invert=True, brightness=17.25, contrast=0.75, noise=True, gamma=0.1, mean=100.0, std=50.0)),
])
INTENSITY_CASES = [(s, k) for s in INTENSITY_SHAPES for k in INTENSITY_STAGES]


@functools.lru_cache(maxsize=None)
def intensity_inputs(shape_name):
    """(image uint8 (w2, h2, d2), noise fp32 in [0, 1)): the image's slices have different means (a wrong slice shows)"""
    shape = INTENSITY_SHAPES[shape_name]
    rs = np.random.RandomState(77 + shape[2])
    ramp = np.linspace(0.35, 1.0, shape[2])[None, None, :]
    image = (rs.rand(*shape) * 255.999 * ramp).astype(np.uint8)
    noise = rs.rand(*shape).astype(np.float32)
    image.setflags(write=False)
    noise.setflags(write=False)
    return image, noise


def intensity_kwargs(shape_name, stage):
    kw = dict(INTENSITY_STAGES[stage])
    if kw.get("noise"):
        kw["noise"] = intensity_inputs(shape_name)[1]
    return kw


# ------------------------------------------------------------------------------------------------ skeleton_to_mask
def skeleton_to_mask_ref(points, offsets, shape):
    """(X, Y, Z) fp32: 1 at trunc(point + offset), the sum in fp32, for every pair with -1 < s < extent on all three axes"""
    X, Y, Z = shape
    s = np.asarray(points, np.float32)[:, None, :] + np.asarray(offsets).astype(np.float32)[None, :, :]
    ok = ((s > -1) & (s < np.array([X, Y, Z], np.float32))).all(-1)
    k = np.trunc(s[ok]).astype(np.int64)
    out = np.zeros(shape, np.float32)
    out[k[:, 0], k[:, 1], k[:, 2]] = 1.0
    return out


S2M_SHAPE, S2M_POINTS = (60, 50, 12), 13600


def s2m_points(n, shape=S2M_SHAPE, seed=5):
    """n fp32 points around ``shape``: most spread sparsely over a margin that straddles every face, the first ones planted
    in (-1, 0), at the extents and just beyond them"""
    rs = np.random.RandomState(seed)
    ext = np.array(shape, np.float64)
    planted = np.array([[-0.5, 20.3, 5.0], [20.0, -0.999, 5.5], [30.0, 20.0, -0.25], [ext[0] - 0.001, 25.0, 6.0],
                        [25.0, ext[1], 6.0], [25.0, 25.0, ext[2] + 0.5], [-1.0, 10.0, 3.0], [0.0, 0.0, 0.0]])
    pts = rs.rand(n, 3) * (ext + [200.0, 200.0, 138.0]) - [100.0, 100.0, 69.0]
    pts[:min(n, len(planted))] = planted[:n]
    return pts.astype(np.float32)


# ------------------------------------------------------------------------------------------------------ bake
ANISOTROPY = (1.0, 1.0, 3.0)


def bake_ref(masks, skeletons, anisotropy=ANISOTROPY, mut=None):
    """((3, X, Y, Z) fp32 baked, (X, Y, Z) float64 squared distance) of oracle/bake.py; an id that has no skeleton is
    background (include/skoots_hip.h).  mut "last_wins": the last minimal point instead of the first."""
    from oracle import bake as B
    known = np.where(np.isin(masks, list(skeletons)), masks, 0)
    sk = {k: (np.asarray(v)[::-1] if mut == "last_wins" else np.asarray(v)) for k, v in skeletons.items()}
    return B.bake_skeleton(known, sk, anisotropy), B.min_distance2(known, sk, anisotropy)


def bake_blocks(shape=(130, 130, 125), block=(26, 26, 25), seed=3):
    """instances are blocks of ``block`` voxels minus a one-voxel gap, three fractional points each"""
    rs = np.random.RandomState(seed)
    masks = np.zeros(shape, np.int32)
    sk, k = {}, 0
    for bx, by, bz in product(*(range(0, s, b) for s, b in zip(shape, block))):
        k += 1
        hi = [min(o + b - 1, s) for o, b, s in zip((bx, by, bz), block, shape)]
        masks[bx:hi[0], by:hi[1], bz:hi[2]] = k
        lo = np.array([bx, by, bz], np.float64)
        sk[k] = (lo + rs.rand(3, 3) * (np.array(hi) - lo - 1)).astype(np.float32)
    return masks, sk


def bake_edges():
    """A (40, 36, 10) volume of 4 x 4 x 5 blocks and a sparse table of 200 ids 3, 13, 23, ...: blocks carry table ids, and
    ids absent from the table below (1, -4), between (8, 1000) and above it (5000); fractional points; and four designed
    ties under the anisotropy (1, 1, 3): ids 3 / 13 hold two points at x = 1 and x = 3 of their block (every voxel of the
    plane x = 2 is equidistant) in the two orders, ids 23 / 33 three points at distance 2 of one voxel, in two orders."""
    shape, b = (40, 36, 10), (4, 4, 5)
    table = [3 + 10 * i for i in range(200)]
    rs = np.random.RandomState(8)
    masks = np.zeros(shape, np.int32)
    sk = {i: rs.rand(1 + i % 3, 3).astype(np.float32) * 30.0 for i in table}
    blocks = list(product(range(0, 40, 4), range(0, 36, 4), range(0, 10, 5)))           # 180 blocks
    ids = table[:170] + [1, -4, 8, 1000, 5000] + table[195:]
    for (x, y, z), i in zip(blocks, ids):
        masks[x:x + 4, y:y + 4, z:z + 5] = i
    for i, (x, y, z) in zip(table[:4], blocks):
        o = np.array([x, y, z], np.float32)
        two = np.array([[1, 1, 2], [3, 1, 2]], np.float32)
        three = np.array([[0, 1, 2], [2, 3, 2], [4, 1, 2]], np.float32)                   # all at distance 2 of (2, 1, 2)
        sk[i] = o + {3: two, 13: two[::-1], 23: three, 33: three[[2, 0, 1]]}[i]
    return masks, sk


# ------------------------------------------------------------------------------------------------------ average
def average_ref(baked, mut=None):
    from oracle import bake as B
    return _average_ne0(baked) if mut == "ne0" else B.average_baked_skeletons(baked)


def _average_ne0(baked):
    """the 27-term sum over the number of entries != 0"""
    c, X, Y, Z = baked.shape
    pad = np.zeros((c, X + 2, Y + 2, Z + 2))
    pad[:, 1:-1, 1:-1, 1:-1] = baked
    s, n = np.zeros(baked.shape), np.zeros(baked.shape)
    for dx, dy, dz in product(range(3), repeat=3):
        w = pad[:, dx:dx + X, dy:dy + Y, dz:dz + Z]
        s += w
        n += w != 0
    n[n == 0] = 1
    return (s / n).astype(np.float32)


AVERAGE_SHAPES = [(1, 1, 1, 1), (3, 7, 5, 4), (2, 1, 6, 5), (2, 6, 1, 5), (2, 6, 5, 1), (3, 90, 90, 87)]   # the last > 4096*256*2


def average_inputs(shape, seed=2):
    """integer-valued coordinates in [-3, 40] with 30 % exact zeros, everywhere: every face and corner has instances, empty
    voxels and negative values, and the 27-term sums are exact in fp32 and float64 alike"""
    rs = np.random.RandomState(seed + shape[1])
    v = rs.randint(-3, 41, shape).astype(np.float32)
    v[rs.rand(*shape) < 0.3] = 0.0
    return v
