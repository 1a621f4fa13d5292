"""GPU tests of the augmentation and target-baking kernels against the references of tests/augment_cases.py: sk_aug_resample,
sk_aug_intensity and sk_skeleton_to_mask (skoots_amd/csrc/augment.hip), sk_bake_skeleton and sk_average_baked_skeletons
(skoots_amd/csrc/bake.hip), through skoots_amd._ffi and, where a case can be expressed that way, through TransformFromCfg.

The cases reach what the recorded fixtures cannot: the second trip of the column stride loop and the 64-partial mean per
z-slice, more than 256 normalise partials, a crop-1 origin inside a device-resident volume, every dtype pair, fields other
than (2, 6, 6), extents of 1, every flip combination, and more work than the streaming kernels' 4096-block grid covers in
one trip.  tests/test_augment_cases_cpu.py shows that the bounds used here separate the kernels from every error the table
was built for.

Bounds.  Geometry: a voxel may differ from the float64 nominal only where some coordinate lies within 1e-4 voxel of a
rounding boundary and only by a candidate value, at most max(1, 1e-4 voxels) per case (tests/test_hip_augment.py's rule).
Intensity: the fp32 roundings of the stages that run, times 2^-24, times 255 (over std after the normalisation); the
derivation stands at augment_cases.ROUNDINGS.  Integer outputs are exact.  Output buffers hold NaN / -77 before every call
and carry a guard behind them: what is not written, or written past the end, shows.
"""
import numpy as np
import pytest
import torch

from tests import augment_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
_CODES = {"uint8": "SK_U8", "float16": "SK_F16", "float32": "SK_F32", "int16": "SK_I16", "int32": "SK_I32"}


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _resample(ffi, p, image, masks, invert=False, brightness=None):
    """sk_aug_resample on sentinel-filled outputs -> (image (w2, h2, d2) fp32 on the device, masks int32 on the CPU,
    workspace, its bytes)"""
    from skoots_amd.train.transforms import _image_theta
    (w1, h1, d1), (w2, h2, d2) = p.e1, p.e2
    q = ffi.AugParams()
    q.src_x, q.src_y, q.src_z = p.src
    q.c1_x0, q.c1_y0, q.c1_z0 = p.o1
    q.w1, q.h1, q.d1 = w1, h1, d1
    q.c2_x0, q.c2_y0, q.c2_z0 = p.o2
    q.w2, q.h2, q.d2 = w2, h2, d2
    q.flip_x, q.flip_y, q.flip_z = (int(f) for f in p.flips)
    if p.affine is not None:
        q.affine = 1
        q.theta[:] = _image_theta(p.affine[0], float(p.affine[1]), p.affine[2], w1, h1)
    field = None
    if p.field is not None:
        field = torch.from_numpy(np.ascontiguousarray(p.field, np.float32)).to(DEV)
        q.elastic = 1
        q.field_d, q.field_h, q.field_w = p.field.shape[1:]
        q.magnitude[:] = list(p.magnitude)
    q.invert = int(invert)
    q.brightness = int(brightness is not None)
    q.brightness_val = float(brightness or 0.0)
    src_i, src_m = torch.from_numpy(np.array(image)).to(DEV), torch.from_numpy(np.array(masks)).to(DEV)
    n = w2 * h2 * d2
    buf_i = torch.full((n + GUARD,), float("nan"), device=DEV)
    buf_m = torch.full((n + GUARD,), -77, dtype=torch.int32, device=DEV)
    nbytes = int(ffi.lib.sk_aug_workspace_bytes(w2, h2, d2))
    ws = torch.full((nbytes + 8 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    ffi.check(ffi.lib.sk_aug_resample(q, ffi.ptr(src_i), getattr(ffi, _CODES[str(image.dtype)]), ffi.ptr(src_m),
                                      getattr(ffi, _CODES[str(masks.dtype)]), ffi.ptr(field), ffi.ptr(buf_i), ffi.ptr(buf_m),
                                      ffi.ptr(ws), nbytes, ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert torch.isnan(buf_i[n:]).all() and bool((buf_m[n:] == -77).all()) and bool((ws[nbytes:] == 0xFF).all()), \
        "sk_aug_resample wrote behind a buffer"
    return buf_i[:n].reshape(w2, h2, d2), buf_m[:n].reshape(w2, h2, d2).cpu().numpy(), ws, nbytes


def _check_geometry(name, got_i, got_m):
    p, image, masks = K.geo_case(name)
    nom = K.geo_nominal(name)
    assert got_i.dtype == np.float32 and got_m.dtype == np.int32 and got_i.shape == nom.image.shape
    assert not np.isnan(got_i).any() and not (got_m == -77).any(), "voxels left unwritten"
    excused = K.excused_voxels(p, image, masks, got_i, got_m, nom)
    print(f"MEASURED {name}: {len(excused)} voxels took the other sample, cap {K.cap(got_i.size)}, flagged {int(nom.near.sum())}")
    assert len(excused) <= K.cap(got_i.size), excused
    return len(excused)


# ------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("name", K.GEO_NAMES)
def test_resample_vs_float64(ffi, name):
    """Every geometric case through the C ABI, twice (the same bits).  Measured on the MI355X: no voxel took the other
    sample but one in 128x128x2-elastic (cap 3) and one in 224x224x2-both-flips (cap 10)."""
    p, image, masks = K.geo_case(name)
    got_i, got_m, _, _ = _resample(ffi, p, image, masks)
    _check_geometry(name, got_i.cpu().numpy(), got_m)
    again_i, again_m, _, _ = _resample(ffi, p, image, masks)
    assert torch.equal(got_i.view(torch.int32), again_i.view(torch.int32)) and np.array_equal(got_m, again_m)


def _transform(e2):
    from skoots_amd.train import TransformFromCfg
    from tests.test_augment_plan import AttrDict, DEFAULT_AUG
    aug = dict(DEFAULT_AUG, CROP_WIDTH=e2[0], CROP_HEIGHT=e2[1], CROP_DEPTH=e2[2], FLIP_RATE=0.5, BRIGHTNESS_RATE=0.4,
               NOISE_GAMMA=0.1, NOISE_RATE=0.2, CONTRAST_RATE=0.33, AFFINE_RATE=0.66, ELASTIC_RATE=0.33)
    return TransformFromCfg(AttrDict(AUGMENTATION=AttrDict(aug), TRAIN=AttrDict(SKELETON_MASK_RADIUS=9,
                                                                                SKELETON_MASK_FLANK_RADIUS=3)), DEV)


@pytest.mark.parametrize("name", K.STRIDED + ["330x320x6-origins", "330x320x6-origins-flips"])
@pytest.mark.parametrize("where", ["device", "cpu"])
def test_transform_augment_vs_float64(name, where):
    """The same cases through TransformFromCfg.augment: the crop origins come from the instance's centre, theta from
    _image_theta.  A volume on the device is read in place (crop-1 origin in the kernel), one on the CPU has its window
    copied (origin 0): both give the nominal."""
    from skoots_amd.train import AugmentPlan
    p, image, masks = K.geo_case(name)
    t = _transform(p.e2)
    shape = (1,) + tuple(p.src)
    assert t.crop_extents(shape) == (tuple(p.e1), tuple(p.e2))
    centre = K.ORIGINS_CENTRE if "origins" in name else tuple(float(o + e // 2) for o, e in zip(p.o1, p.e1))
    skel = {1: torch.tensor([centre])}
    plan = AugmentPlan(key=1, elastic=p.field is not None,
                       elastic_field=None if p.field is None else torch.from_numpy(np.asarray(p.field, np.float32))[None],
                       affine=p.affine is not None, flip_x=p.flips[0], flip_y=p.flips[1], flip_z=p.flips[2])
    if p.affine is not None:
        plan.angle, plan.shear, plan.scale = p.affine
    g = t.geometry(shape, skel, plan, "cpu")
    assert tuple(g["crop1"]) == tuple(p.o1) and tuple(g["crop2"]) == tuple(p.o2), (g["crop1"], g["crop2"])
    dev = DEV if where == "device" else "cpu"
    img, msk, _ = t.augment(torch.from_numpy(np.array(image))[None].to(dev), torch.from_numpy(np.array(masks))[None].to(dev), skel, plan,
                            intensity=False)
    _check_geometry(name, img[0].cpu().numpy(), msk[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------------ intensity
def _identity(shape):
    return K.Geo(shape, (0, 0, 0), shape, (0, 0, 0), shape, (False, False, False), None, None, K.DEFAULT_MAGNITUDE)


def _run_intensity(ffi, shape_name, kw):
    """sk_aug_resample (identity gather; invert and brightness run there) + sk_aug_intensity -> (w2, h2, d2) fp32, CPU"""
    image, _ = K.intensity_inputs(shape_name)
    w2, h2, d2 = image.shape
    out, _, ws, nbytes = _resample(ffi, _identity(image.shape), image, np.zeros(image.shape, np.uint8),
                                   invert=kw.get("invert", False), brightness=kw.get("brightness"))
    noise = None if kw.get("noise") is None else torch.from_numpy(np.array(kw["noise"])).to(DEV)
    contrast = kw.get("contrast")
    ffi.check(ffi.lib.sk_aug_intensity(ffi.ptr(out), w2, h2, d2, int(contrast is not None), float(contrast or 0.0),
                                       ffi.ptr(noise), float(kw.get("gamma", 0.0)), int(kw.get("own_mean", False)),
                                       float(kw.get("mean", 0.0)), int(kw.get("own_std", False)), float(kw.get("std", 1.0)),
                                       ffi.ptr(ws), nbytes, ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xFF).all()), "sk_aug_intensity wrote behind the workspace"
    return out.cpu().numpy()


@pytest.mark.parametrize("shape_name,stage", K.INTENSITY_CASES)
def test_intensity_vs_float64(ffi, shape_name, stage):
    """Each stage alone and all together, on 320 and 300 normalise partials and on one small output.  Measured on the
    MI355X: at most 0.30 of the tolerance (4x4x300 own-std, 3.1e-7 of 1.05e-6); before the normalisation at most 3.1e-5
    of 1.8e-4 (4x4x300 contrast2)."""
    kw = K.intensity_kwargs(shape_name, stage)
    image, _ = K.intensity_inputs(shape_name)
    got = _run_intensity(ffi, shape_name, kw)
    want = K.intensity64(image, **kw)
    std_used = float(K.intensity64(image, upto="noise", **kw).std(ddof=1)) if kw.get("own_std") else K.r32(kw.get("std", 1.0))
    tol = K.intensity_tolerance(std_used=std_used, **kw)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"MEASURED {shape_name} {stage}: off by {err:.3e}, tolerance {tol:.3e} ({err / tol:.3f} of it)")
    assert np.isfinite(got).all()
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("shape_name", list(K.INTENSITY_SHAPES))
def test_contrast_zero_returns_the_slice_means(ffi, shape_name):
    """contrast_val = 0 blends everything away but the mean: every voxel of a slice is (float) mean * 255, the sum of up
    to 64 partials over the plane.  Held to one ulp of fp32 at 1, times 255 = 3.04e-5: the mean's fp32 rounding and the
    rounding of the product are half an ulp each.  Measured on the MI355X: 5.1e-6, 1.5e-5 and 6.7e-6."""
    image, _ = K.intensity_inputs(shape_name)
    got = _run_intensity(ffi, shape_name, dict(contrast=0.0)).astype(np.float64)
    want = (image.astype(np.float64) / 255.0).mean((0, 1)) * 255.0
    assert (got == got[:1, :1]).all(), "a slice holds more than one value"
    err = float(np.abs(got[0, 0] - want).max())
    print(f"MEASURED {shape_name} contrast 0: slice means off by {err:.3e}, bound {255 * 2.0 ** -23:.3e}")
    assert err <= 255 * 2.0 ** -23, (err, got[0, 0], want)


def test_intensity_is_deterministic(ffi):
    kw = K.intensity_kwargs("129x128x5", "all")
    a, b = _run_intensity(ffi, "129x128x5", kw), _run_intensity(ffi, "129x128x5", kw)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ skeleton_to_mask
@pytest.mark.parametrize("n_points", [1, K.S2M_POINTS])
def test_skeleton_to_mask_vs_reference(n_points):
    """13 600 points x 311 offsets: more pairs than 4096 blocks x 256 threads x 4 cover in one trip."""
    from skoots_amd.lib.skeleton import get_cached_disk_coords, skeleton_to_mask
    pts = K.s2m_points(n_points)
    offs = get_cached_disk_coords("cpu", 9, 3).T.numpy()
    got = skeleton_to_mask({1: torch.from_numpy(pts).to(DEV)}, K.S2M_SHAPE, device=DEV, radius=9, flank_radius=3)
    assert got.shape == (1,) + K.S2M_SHAPE and got.dtype == torch.float32
    np.testing.assert_array_equal(got[0].cpu().numpy(), K.skeleton_to_mask_ref(pts, offs, K.S2M_SHAPE))


# ------------------------------------------------------------------------------------------------------ bake
def _bake(masks, sk):
    from skoots_amd.lib.skeleton import bake_skeleton
    raw, dist = bake_skeleton(torch.from_numpy(masks).to(DEV), {k: torch.from_numpy(np.asarray(v)) for k, v in sk.items()},
                              list(K.ANISOTROPY), average=False, return_distance=True)
    return raw.cpu().numpy(), dist[0].cpu().numpy()


def _check_bake(masks, sk):
    raw, dist = _bake(masks, sk)
    want, d2 = K.bake_ref(masks, sk)
    np.testing.assert_array_equal(raw, want)
    np.testing.assert_allclose(dist, np.sqrt(d2), rtol=1e-6, atol=0)      # one fp32 rounding of a double sqrt


def test_bake_past_the_grid_cap():
    """130 x 130 x 125 voxels: more than 4096 blocks x 256 threads x 2."""
    _check_bake(*K.bake_blocks())


def test_bake_sparse_table_ties_and_absent_ids():
    masks, sk = K.bake_edges()
    _check_bake(masks, sk)
    _check_bake(masks, {23: sk[23]})                                      # K = 1


# ------------------------------------------------------------------------------------------------------ average
@pytest.mark.parametrize("shape", K.AVERAGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_average_is_exact_on_integer_coordinates(shape):
    from skoots_amd.lib.skeleton import average_baked_skeletons
    v = K.average_inputs(shape)
    got = average_baked_skeletons(torch.from_numpy(v)[None].to(DEV))[0].cpu().numpy()
    np.testing.assert_array_equal(got, K.average_ref(v))
