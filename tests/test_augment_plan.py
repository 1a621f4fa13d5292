"""CPU tests of the augmentation's host side (skoots_amd/train/transforms.py, skoots_amd/lib/skeleton.py) against
tests/golden/augment.npz, recorded from the reference's own TransformFromCfg (make_augment_golden.py): the random
draws of a seeded sample, the cfg the constructor reads, the skeleton-mask offset table and the skeleton points."""
import random

import numpy as np
import pytest
import torch

DEFAULT_AUG = dict(BRIGHTNESS_RANGE=[-0.1, 0.1], CONTRAST_RANGE=[0.75, 2.0], AFFINE_SCALE=[0.85, 1.1],
                   AFFINE_YAW=[-180, 180], AFFINE_SHEAR=[-7, 7], ELASTIC_GRID_SHAPE=(6, 6, 2),
                   ELASTIC_GRID_MAGNITUDE=(0.05, 0.05, 0.01), BAKE_SKELETON_ANISOTROPY=(1.0, 1.0, 3.0))


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def case_cfg(d, i, attr=True):
    aug = dict(DEFAULT_AUG)
    for name, v in zip(d["cfg_names"], d[f"c{i}_cfg"]):
        aug[str(name)] = int(v) if str(name).startswith("CROP") else float(v)
    r, fr = (int(v) for v in d[f"c{i}_radius"])
    train = dict(SKELETON_MASK_RADIUS=r, SKELETON_MASK_FLANK_RADIUS=fr)
    if attr:
        return AttrDict(AUGMENTATION=AttrDict(aug), TRAIN=AttrDict(train))
    return {"AUGMENTATION": aug, "TRAIN": train}


def case_inputs(d, i):
    """(image (1, X, Y, Z), masks, skeletons {id: (N, 3) fp32}) of case i, on the CPU as the reference keeps them."""
    v = str(d[f"c{i}_volume"])
    image, masks = torch.from_numpy(d[f"vol_{v}_image"]), torch.from_numpy(d[f"vol_{v}_masks"])
    pts = torch.from_numpy(d[f"c{i}_points_in"])
    keys = [int(k) for k in d[f"c{i}_keys"]]
    skel = dict(zip(keys, torch.split(pts, [int(c) for c in d[f"c{i}_counts"]])))
    return image, masks, {k: p.clone() for k, p in skel.items()}


def case_plan(d, i):
    """The recorded draws of case i as an AugmentPlan."""
    from skoots_amd.train import AugmentPlan
    f = {str(n): bool(v) for n, v in zip(d["flag_names"], d[f"c{i}_flags"])}
    f.update({str(n): float(v) for n, v in zip(d["value_names"], d[f"c{i}_values"])})
    field = d[f"c{i}_elastic_field"] if f"c{i}_elastic_field" in d.files else None
    noise = d[f"c{i}_noise"] if f"c{i}_noise" in d.files else None
    return AugmentPlan(key=int(d[f"c{i}_key"]), elastic_field=None if field is None else torch.from_numpy(field),
                       noise=None if noise is None else torch.from_numpy(noise), **f)


def test_draw_plan_consumes_random_in_the_reference_order(golden):
    from skoots_amd.train import TransformFromCfg, draw_plan
    d = golden("augment.npz")
    for i in range(int(d["n"])):
        image, _, skel = case_inputs(d, i)
        t = TransformFromCfg(case_cfg(d, i), "cpu")
        seed = int(d[f"c{i}_seed"])
        random.seed(seed)
        torch.manual_seed(seed)
        got = draw_plan(t, skel.keys(), image.shape, "cpu")
        want = case_plan(d, i)
        assert got.key == want.key, i
        for name in d["flag_names"]:
            assert getattr(got, str(name)) == getattr(want, str(name)), (i, name)
        for name in d["value_names"]:
            assert getattr(got, str(name)) == getattr(want, str(name)), (i, name)
        for name in ("elastic_field", "noise"):
            g, w = getattr(got, name), getattr(want, name)
            assert (g is None) == (w is None), (i, name)
            if w is not None:
                assert torch.equal(g, w), (i, name)


def test_constructor_reads_the_cfg():
    from skoots_amd.train import TransformFromCfg
    d = {"cfg_names": np.array(["CROP_WIDTH", "CROP_HEIGHT", "CROP_DEPTH", "FLIP_RATE", "BRIGHTNESS_RATE",
                                "NOISE_GAMMA", "NOISE_RATE", "CONTRAST_RATE", "AFFINE_RATE", "ELASTIC_RATE"]),
         "c0_cfg": np.array([300, 280, 20, 0.5, 0.4, 0.1, 0.2, 0.33, 0.66, 0.33]), "c0_radius": np.array([9, 3])}
    for attr in (True, False):
        t = TransformFromCfg(case_cfg(d, 0, attr=attr), "cpu")
        assert (t.CROP_WIDTH, t.CROP_HEIGHT, t.CROP_DEPTH) == (300, 280, 20)
        assert (t.FLIP_RATE, t.BRIGHTNESS_RATE, t.NOISE_GAMMA, t.NOISE_RATE) == (0.5, 0.4, 0.1, 0.2)
        assert (t.CONTRAST_RATE, t.AFFINE_RATE, t.ELASTIC_RATE) == (0.33, 0.66, 0.33)
        assert t.CONTRAST_RANGE == [0.75, 2.0] and t.AFFINE_YAW == [-180, 180] and t.AFFINE_SHEAR == [-7, 7]
        assert t.AFFINE_SCALE == [0.85, 1.1] and t.BRIGHTNESS_RANGE == [-0.1, 0.1]
        assert t.BAKE_SKELETON_ANISOTROPY == (1.0, 1.0, 3.0)
        assert (t.SKELETON_MASK_RADIUS, t.SKELETON_MASK_FLANK_RADIUS) == (9, 3)
        assert (t.dataset_mean, t.dataset_std, t.SCALE) == (0, 1, 255.0)
        assert t.set_dataset_mean(3.5).set_dataset_std(2.0) is t and (t.dataset_mean, t.dataset_std) == (3.5, 2.0)
        # crop 1 = crop + 300 in x, y when the volume allows it; crop 2 never exceeds crop 1
        assert t.crop_extents((1, 700, 500, 64)) == ((600, 500, 20), (300, 280, 20))
        assert t.crop_extents((1, 100, 90, 8)) == ((100, 90, 8), (100, 90, 8))


@pytest.mark.parametrize("r,fr", [(7, 3), (9, 3)])
def test_disk_coords_equal_the_reference_table(golden, r, fr):
    from skoots_amd.lib.skeleton import get_cached_disk_coords
    d = golden("augment.npz")
    got = get_cached_disk_coords("cpu", r, fr)
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.numpy(), d[f"disk_{r}_{fr}"])


def assert_points_match(got, want, affine, msg):
    """Bit for bit, except after the skeleton affine: there the reference's own bits depend on the GEMM torch picks
    for ``mat @ points`` (on the CPU an FMA chain above 44 points per skeleton, separate multiplies and adds below
    that; other kernels on a GPU), so the port's fixed FMA chain is held to 1e-4 voxel."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if affine:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4, err_msg=msg)
    else:
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=msg)


def test_skeleton_points_on_the_host(golden):
    """Crop offsets, the skeleton affine and the flips in torch on the CPU give the reference's points (bit for bit
    without the affine), and the elastic stage leaves them alone."""
    from skoots_amd.train import TransformFromCfg
    d = golden("augment.npz")
    for i in range(int(d["n"])):
        image, _, skel = case_inputs(d, i)
        t = TransformFromCfg(case_cfg(d, i), "cpu")
        g = t.geometry(image.shape, skel, case_plan(d, i), "cpu")
        got = torch.cat([g["skeletons"][k] for k in skel]).numpy()
        assert got.dtype == np.float32
        assert_points_match(got, d[f"c{i}_points"], case_plan(d, i).affine, f"case {i}")
