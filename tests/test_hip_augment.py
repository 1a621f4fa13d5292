"""GPU tests of the training-crop augmentation (csrc/augment.hip, skoots_amd/train/transforms.py,
skoots_amd/lib/skeleton.py::skeleton_to_mask) against tests/golden/augment.npz, recorded from the reference's own
TransformFromCfg and skeleton_to_mask (make_augment_golden.py).

The geometric gather is exact up to one thing: a stage whose fp32 source coordinate lies at a rounding boundary can
round either way depending on the order torch's kernels happen to use.  The test computes every stage's coordinate in
float64 itself; a voxel may differ from the fixture only if some coordinate lies within 1e-4 voxel of a boundary,
only if both the port's and the fixture's value are samples the other rounding would give, and at most 1e-4 of all
voxels (at least one) may do so."""
import numpy as np
import pytest
import torch

from tests.augment_cases import EPS, params_from_plan
from tests.augment_cases import voxel_candidates as _voxel_candidates
from tests.test_augment_plan import assert_points_match, case_cfg, case_inputs, case_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def voxel_candidates(image, masks, g, plan, t, x, y, z):
    """Every (image, mask) value the output voxel (x, y, z) can take when each stage's float64 coordinate that lies
    within EPS of a rounding boundary may round either way (tests/augment_cases.py)."""
    p = params_from_plan(t, image.shape, g, plan)
    return _voxel_candidates(p, image[0].numpy(), masks[0].numpy(), int(x), int(y), int(z))


def _transform(d, i):
    from skoots_amd.train import TransformFromCfg
    return TransformFromCfg(case_cfg(d, i), DEV)


def test_geometry_masks_points_and_targets_vs_reference(golden):
    from skoots_amd.lib.skeleton import bake_skeleton
    d = golden("augment.npz")
    excused, total = [], 0
    for i in range(int(d["n"])):
        image, masks, skel = case_inputs(d, i)
        t, plan = _transform(d, i), case_plan(d, i)
        img, msk, pts = t.augment(image, masks, skel, plan, intensity=False)
        got_i, got_m = img[0].cpu().numpy(), msk[0].cpu().numpy()
        want_i, want_m = d[f"c{i}_geom"][0], d[f"c{i}_masks"][0]
        assert got_i.dtype == np.float32 and got_m.dtype == np.int32 and got_i.shape == want_i.shape, i
        total += got_i.size
        bad = np.argwhere((got_i.view(np.int32) != want_i.view(np.int32)) | (got_m != want_m))
        g = t.geometry(image.shape, skel, plan, "cpu")
        for x, y, z in bad:
            vals = voxel_candidates(image.float(), masks, g, plan, t, x, y, z)
            assert len(vals) > 1, f"case {i} voxel {(x, y, z)}: {got_i[x, y, z]} vs {want_i[x, y, z]}, not at a boundary"
            assert (float(got_i[x, y, z]), int(got_m[x, y, z])) in vals and \
                (float(want_i[x, y, z]), int(want_m[x, y, z])) in vals, (i, x, y, z, vals)
            excused.append((i, x, y, z))
        got_pts = torch.cat([pts[k] for k in skel]).cpu().numpy()
        assert_points_match(got_pts, d[f"c{i}_points"], plan.affine, f"case {i}")

        # the whole forward: masks again, skele_masks bit-exact, baked = bake_skeleton on the fixture's own data
        out = t({"image": image, "masks": masks, "skeletons": skel}, plan=plan)
        assert set(out) == {"image", "masks", "skeletons", "baked_skeleton", "skele_masks"}
        assert torch.equal(out["masks"], msk)
        np.testing.assert_array_equal(out["skele_masks"].cpu().numpy(), d[f"c{i}_skele_masks"], err_msg=f"case {i}")
        want_pts = torch.from_numpy(d[f"c{i}_points"])
        counts = [int(c) for c in d[f"c{i}_counts"]]
        fx_skel = dict(zip(skel.keys(), torch.split(want_pts, counts)))
        fx_baked = bake_skeleton(torch.from_numpy(want_m).to(DEV).unsqueeze(0), fx_skel,
                                 anisotropy=t.BAKE_SKELETON_ANISOTROPY, average=True)
        if plan.affine or len(bad):
            torch.testing.assert_close(out["baked_skeleton"], fx_baked, rtol=0, atol=1e-3)
        else:
            assert torch.equal(out["baked_skeleton"], fx_baked), i
    assert len(excused) <= max(1, int(EPS * total)), excused


def test_intensity_stages_vs_reference(golden):
    d = golden("augment.npz")
    for i in range(int(d["n"])):
        image, masks, skel = case_inputs(d, i)
        t, plan = _transform(d, i), case_plan(d, i)
        img, _, _ = t.augment(image, masks, skel, plan)
        want = d[f"c{i}_image"][0]
        # 1e-5 of the intensity range: normalise subtracts a mean of order 100 from values of order 255, so a voxel
        # near the mean keeps the absolute error of the 0..255 values, not a relative one of its own
        scale = max(255.0, float(np.abs(want).max()))
        np.testing.assert_allclose(img[0].cpu().numpy(), want, rtol=0, atol=1e-5 * scale, err_msg=f"case {i}")


def test_dataset_mean_and_std(golden):
    """Normalise: the image's own mean with the default (0, 1); a set mean and std used as given; a std of 0 means
    the image's unbiased std."""
    d = golden("augment.npz")
    i = 7
    image, masks, skel = case_inputs(d, i)
    plan = case_plan(d, i)
    t = _transform(d, i)
    own_mean, _, _ = t.augment(image, masks, skel, plan)
    t.set_dataset_mean(3.0).set_dataset_std(2.0)
    given, _, _ = t.augment(image, masks, skel, plan)
    t.set_dataset_mean(0).set_dataset_std(0)
    own_both, _, _ = t.augment(image, masks, skel, plan)
    v = given.double().cpu() * 2.0 + 3.0            # the image before the normalisation
    np.testing.assert_allclose(own_mean.cpu().numpy(), (v - v.mean()).numpy(), rtol=0, atol=1e-3)
    np.testing.assert_allclose(own_both.cpu().numpy(), ((v - v.mean()) / v.std()).numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("r,fr", [(7, 3), (9, 3)])
def test_skeleton_to_mask_vs_reference(golden, r, fr):
    from skoots_amd.lib.skeleton import skeleton_to_mask
    d = golden("augment.npz")
    pts = torch.from_numpy(d["s2m_points"])
    counts = [int(c) for c in d["s2m_counts"]]
    skel = {k: p.to(DEV) for k, p in zip((3, 5, 8), torch.split(pts, counts))}
    shape = tuple(int(s) for s in d["s2m_shape"])
    got = skeleton_to_mask(skel, shape, device=DEV, radius=r, flank_radius=fr)
    assert got.shape == (1,) + shape and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), d[f"s2m_{r}_{fr}"])
    assert torch.equal(skeleton_to_mask({-1: pts.to(DEV)}, shape, device=DEV), torch.zeros((1,) + shape, device=DEV))
    assert torch.equal(skeleton_to_mask({}, shape, device=DEV), torch.zeros((1,) + shape, device=DEV))


def _synthetic_sample(seed, shape=(44, 40, 14), n=5):
    gen = torch.Generator().manual_seed(seed)
    X, Y, Z = shape
    image = (torch.rand((1,) + shape, generator=gen) * 255).to(torch.uint8)
    masks = torch.zeros((1,) + shape, dtype=torch.int16)
    skel = {}
    for k in range(1, n + 1):
        c = [int(torch.randint(4, s - 4, (1,), generator=gen)) for s in shape]
        masks[0, c[0] - 4:c[0] + 4, c[1] - 4:c[1] + 4, c[2] - 2:c[2] + 2] = k
        skel[k] = torch.tensor([[c[0] - 2.0, c[1], c[2]], [c[0], c[1], c[2]], [c[0] + 2.0, c[1] + 1, c[2]]])
    return {"image": image, "masks": masks, "skeletons": skel}


def _cfg16():
    from tests.test_augment_plan import AttrDict, DEFAULT_AUG
    aug = dict(DEFAULT_AUG, CROP_WIDTH=16, CROP_HEIGHT=16, CROP_DEPTH=8, FLIP_RATE=0.5, BRIGHTNESS_RATE=0.4,
               NOISE_GAMMA=0.1, NOISE_RATE=0.2, CONTRAST_RATE=0.33, AFFINE_RATE=0.66, ELASTIC_RATE=0.33)
    return AttrDict(AUGMENTATION=AttrDict(aug), TRAIN=AttrDict(SKELETON_MASK_RADIUS=9, SKELETON_MASK_FLANK_RADIUS=3))


def test_deterministic_and_volume_on_device():
    """Two runs give identical bits, and a volume already on the device (the gather reads the crop-1 window in place)
    gives what the CPU volume gives."""
    from skoots_amd.train import AugmentPlan, TransformFromCfg
    t = TransformFromCfg(_cfg16(), DEV)
    s = _synthetic_sample(5)
    g = torch.Generator(device=DEV).manual_seed(3)
    plan = AugmentPlan(key=3, elastic=True, elastic_field=torch.rand((1, 3, 2, 6, 6), generator=g, device=DEV),
                       affine=True, angle=31.7, shear=-4.2, scale=0.93, flip_x=True, flip_z=True, invert=True,
                       brightness=True, brightness_val=0.07, contrast=True, contrast_val=1.4,
                       noise=torch.rand((1, 16, 16, 8), generator=g, device=DEV))
    runs = []
    for dev in ("cpu", "cpu", DEV):
        dd = {"image": s["image"].to(dev), "masks": s["masks"].to(dev), "skeletons": dict(s["skeletons"])}
        out = t(dd, plan=plan)
        runs.append([out[k] for k in ("image", "masks", "baked_skeleton", "skele_masks")])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b)


def test_refused_arguments_write_nothing():
    from skoots_amd import _ffi
    w2, h2, d2 = 8, 8, 4
    src = torch.zeros((1, 16, 16, 8), dtype=torch.uint8, device=DEV)
    out_i = torch.full((w2, h2, d2), 7.0, device=DEV)
    out_m = torch.full((w2, h2, d2), 7, dtype=torch.int32, device=DEV)
    nbytes = int(_ffi.lib.sk_aug_workspace_bytes(w2, h2, d2))
    ws = torch.full((nbytes,), 7, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(DEV)

    def params(**over):
        p = _ffi.AugParams()
        p.src_x, p.src_y, p.src_z = 16, 16, 8
        p.w1, p.h1, p.d1 = 16, 16, 8
        p.w2, p.h2, p.d2 = w2, h2, d2
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def resample(p, img_code=_ffi.SK_U8, msk_code=_ffi.SK_U8, field=None, wsb=nbytes):
        return _ffi.lib.sk_aug_resample(p, _ffi.ptr(src), img_code, _ffi.ptr(src), msk_code, _ffi.ptr(field),
                                        _ffi.ptr(out_i), _ffi.ptr(out_m), _ffi.ptr(ws), wsb, st)

    bad = [resample(params(c2_x0=9)),                     # crop 2 leaves crop 1
           resample(params(c1_x0=1)),                     # crop 1 leaves the source
           resample(params(w1=0)),
           resample(params(), img_code=_ffi.SK_I32),      # image dtype
           resample(params(), msk_code=_ffi.SK_F32),      # masks dtype
           resample(params(elastic=1)),                   # elastic without a field
           resample(params(), wsb=nbytes - 1),            # workspace too small
           _ffi.lib.sk_aug_intensity(_ffi.ptr(out_i), w2, h2, 0, 0, 1.0, None, 0.1, 1, 0.0, 1, 0.0, _ffi.ptr(ws),
                                     nbytes, st),
           _ffi.lib.sk_aug_intensity(_ffi.ptr(out_i), w2, h2, d2, 0, 1.0, None, 0.1, 1, 0.0, 1, 0.0, _ffi.ptr(ws),
                                     nbytes - 8, st)]
    pts = torch.zeros((4, 3), device=DEV)
    offs = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    bad += [_ffi.lib.sk_skeleton_to_mask(_ffi.ptr(pts), 1 << 31, _ffi.ptr(offs), 2, w2, h2, d2, _ffi.ptr(out_i), st),
            _ffi.lib.sk_skeleton_to_mask(_ffi.ptr(pts), 4, _ffi.ptr(offs), 0, w2, h2, d2, _ffi.ptr(out_i), st),
            _ffi.lib.sk_skeleton_to_mask(None, 4, _ffi.ptr(offs), 2, w2, h2, d2, _ffi.ptr(out_i), st),
            _ffi.lib.sk_skeleton_to_mask(_ffi.ptr(pts), 4, _ffi.ptr(offs), 2, w2, 0, d2, _ffi.ptr(out_i), st)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad)
    assert bool((out_i == 7.0).all()) and bool((out_m == 7).all()) and bool((ws == 7).all())


def test_augment_collate_train_step_bf16():
    """Augment two samples with drawn plans, collate them, take one bf16 TrainStep: finite losses."""
    import random
    from skoots_amd.train import TrainStep, TrainUNet, TransformFromCfg, skeleton_colate
    from skoots_amd.unet import random_state_dict
    t = TransformFromCfg(_cfg16(), DEV)
    random.seed(4)
    torch.manual_seed(4)
    batch = [t(_synthetic_sample(s)) for s in (11, 12)]
    images, masks, skeletons, skele_masks, baked = skeleton_colate(batch)
    assert images.shape == (2, 1, 16, 16, 8) and images.dtype == torch.float32
    assert masks.shape == (2, 1, 16, 16, 8) and masks.dtype == torch.int32
    assert skele_masks.shape == (2, 1, 16, 16, 8) and baked.shape == (2, 3, 16, 16, 8)
    assert len(skeletons) == 2
    step = TrainStep(TrainUNet(random_state_dict(), DEV, precision="bf16"))
    losses = step(images, masks, skele_masks, baked, [20.0, 20.0, 20.0])
    assert torch.isfinite(losses).all(), losses
