"""What makes the assertions of tests/test_hip_augment_cases.py mean something, checked on the CPU from the references of
tests/augment_cases.py, tests/golden/augment.npz and the library's host-only size query.

The references: geometry_torch32 (torch's own fp32 ops) reproduces the geometric half of all 23 fixture cases,
geometry_nominal64 agrees with the fixture under the rule the GPU test applies to the kernel, intensity64 agrees with the
fixture's final images.  The table: every case reaches the path it was built for (a second stride trip, more than 256
partials, more pairs / voxels than the streaming kernels' grid cap covers in one trip), zero-fills and samples at least 1 %
of its voxels wherever a stage can leave the window, and lies so far from rounding boundaries that torch's fp32 chain and
the float64 one differ on at most half the cap.  The bounds: each deliberate error of the references leaves the GPU test's
bound on the case built for it.
"""
import numpy as np
import pytest
import torch

from tests import augment_cases as K
from tests.test_augment_plan import case_cfg, case_inputs, case_plan


def _fixture_case(d, i):
    """(Geo, image (X, Y, Z), masks (X, Y, Z), plan, transform) of fixture case i"""
    from skoots_amd.train import TransformFromCfg
    image, masks, skel = case_inputs(d, i)
    t, plan = TransformFromCfg(case_cfg(d, i), "cpu"), case_plan(d, i)
    p = K.params_from_plan(t, image.shape, t.geometry(image.shape, skel, plan, "cpu"), plan)
    return p, image[0].numpy(), masks[0].numpy(), plan, t


def _mismatches(a_i, a_m, b_i, b_m):
    return (a_i.view(np.int32) != b_i.view(np.int32)) | (a_m != b_m)


def _violations(nom, got_i, got_m):
    """(mismatches at voxels that are not flagged near a boundary, all mismatches)"""
    bad = _mismatches(got_i, got_m, nom.image, nom.masks)
    return int((bad & ~nom.near).sum()), int(bad.sum())


# ------------------------------------------------------------------------------------------- references vs the fixture
def test_torch32_reproduces_the_fixture_geometry(golden):
    """Bit for bit on the torch build the fixture was checked with; on another, a voxel may differ only where both values
    are candidates of a rounding boundary, at most 1e-4 of all voxels."""
    d = golden("augment.npz")
    excused, total = [], 0
    for i in range(int(d["n"])):
        p, image, masks, _, _ = _fixture_case(d, i)
        got_i, got_m = K.geometry_torch32(p, image, masks)
        want_i, want_m = d[f"c{i}_geom"][0], d[f"c{i}_masks"][0]
        assert got_i.shape == want_i.shape, i
        total += got_i.size
        for x, y, z in np.argwhere(_mismatches(got_i, got_m, want_i, want_m)):
            vals = K.voxel_candidates(p, image.astype(np.float32), masks, int(x), int(y), int(z))
            assert len(vals) > 1 and (float(got_i[x, y, z]), int(got_m[x, y, z])) in vals and \
                (float(want_i[x, y, z]), int(want_m[x, y, z])) in vals, (i, x, y, z, vals)
            excused.append((i, x, y, z))
    assert total == 23898
    assert len(excused) <= K.cap(total), excused


def test_nominal64_agrees_with_the_fixture_geometry(golden):
    d = golden("augment.npz")
    for i in range(int(d["n"])):
        p, image, masks, _, _ = _fixture_case(d, i)
        nom = K.geometry_nominal64(p, image, masks)
        excused = K.excused_voxels(p, image, masks, d[f"c{i}_geom"][0], d[f"c{i}_masks"][0], nom)
        assert len(excused) <= K.cap(nom.image.size), (i, excused)


def test_intensity64_agrees_with_the_fixture_images(golden):
    d = golden("augment.npz")
    for i in range(int(d["n"])):
        _, _, _, plan, t = _fixture_case(d, i)
        got = K.intensity64(d[f"c{i}_geom"][0], invert=plan.invert, brightness=plan.brightness_val if plan.brightness else None,
                            contrast=plan.contrast_val if plan.contrast else None,
                            noise=None if plan.noise is None else plan.noise[0].numpy(), gamma=t.NOISE_GAMMA, own_mean=True)
        want = d[f"c{i}_image"][0]
        scale = max(255.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * scale, err_msg=f"case {i}")


def test_image_theta_is_the_float64_theta_in_fp32():
    """transforms._image_theta (what the kernel is handed) against the float64 matrix, at the extents of the table"""
    from skoots_amd.train.transforms import _image_theta
    for name in K.GEO_NAMES:
        p = K.geo_case(name)[0]
        if p.affine is not None:
            got, want = _image_theta(*p.affine, p.e1[0], p.e1[1]), K.image_theta64(p)
            np.testing.assert_allclose(got, want, rtol=3 * 2.0 ** -24, atol=1e-18, err_msg=name)   # fp32 theta, one division


# ------------------------------------------------------------------------------------------------- the case conditions
def test_the_table_reaches_the_paths_it_names():
    from skoots_amd import _ffi
    from skoots_amd.lib.skeleton import get_cached_disk_coords
    trips = {}
    for name in K.STRIDED:
        w2, h2, d2 = K.geo_case(name)[0].e2
        assert w2 * h2 >= K.MAX_BLOCKS_PER_Z * K.K_BLOCK and 2 <= d2 <= 3, name
        trips[name.split("-")[0]] = w2 * h2 / (K.MAX_BLOCKS_PER_Z * K.K_BLOCK)
    assert trips["128x128x2"] == 1.0 and 1 < trips["129x128x3"] < 2 and 3 < trips["224x224x2"] < 4
    assert 145 * 113 == K.MAX_BLOCKS_PER_Z * K.K_BLOCK + 1
    for (w2, h2, d2), partials in (((129, 128, 5), 320), ((4, 4, 300), 300)):
        nb = K.blocks_per_z(w2 * h2)
        assert nb * d2 == partials > K.K_BLOCK
        assert int(_ffi.lib.sk_aug_workspace_bytes(w2, h2, d2)) == nb * d2 * 3 * 8     # the library's own count of partials
    for name in K.GEO_NAMES:
        p = K.geo_case(name)[0]
        assert max(p.e1) <= K.MAX_EXTENT
    p = K.geo_case("330x320x6-origins")[0]
    assert min(p.o1) > 0 and max(p.o2[:2]) > 0 and p.e1 == (308, 306, 3) and p.e2 == (8, 6, 3)
    n_off = get_cached_disk_coords("cpu", 9, 3).shape[1]
    assert K.S2M_POINTS * n_off > K.STREAM_GRID_CAP * 256 * 4 >= (K.S2M_POINTS - 200) * n_off      # just past the cap
    assert 130 * 130 * 125 > K.STREAM_GRID_CAP * 256 * 2 and int(np.prod(K.AVERAGE_SHAPES[-1])) > K.STREAM_GRID_CAP * 256 * 2
    pairs = {(K._G[n]["img"], K._G[n]["msk"]) for n in K.GEO_NAMES if n.startswith("9x7x3-")}
    assert len(pairs) == 9


@pytest.mark.parametrize("name", K.GEO_NAMES)
def test_geometric_case_is_well_placed(name):
    """At least 1 % zero-filled and 1 % sampled voxels wherever a stage can leave the window, and torch's own fp32 chain
    differs from the float64 nominal on at most half the cap, only at flagged voxels, only by candidate values."""
    p, image, masks = K.geo_case(name)
    nom = K.geo_nominal(name)
    n = nom.image.size
    if p.affine is not None or p.field is not None:
        assert (~nom.inside).sum() >= 0.01 * n and nom.inside.sum() >= 0.01 * n, (name, int(nom.inside.sum()), n)
    else:
        assert nom.inside.all()
    got_i, got_m = K.geometry_torch32(p, image, masks)
    excused = K.excused_voxels(p, image, masks, got_i, got_m, nom)
    assert len(excused) <= K.cap(n) // 2, (name, excused)
    if "ties" not in name:
        assert nom.near.sum() <= 0.01 * n, (name, int(nom.near.sum()))      # the flagged voxels stay the exception


def test_mask_ids_and_image_values_of_the_dtype_cases():
    seen = set()
    for name in K.GEO_NAMES:
        if name.startswith("9x7x3-"):
            _, image, masks = K.geo_case(name)
            nom = K.geo_nominal(name)
            seen |= set(np.unique(nom.masks).tolist())
            if image.dtype != np.uint8:
                assert (nom.image != np.rint(nom.image)).sum() > 0.5 * nom.inside.sum()      # non-integer values
    assert {255, 32767, -3, (1 << 24) - 1} <= seen


# -------------------------------------------------------------------------------------------------- discrimination
def test_geometry_mutations_leave_the_rule():
    for name, mut in (("21x19x6-field354", "field_hw_swapped"), ("16x16x2-ties", "floor_half")):
        p, image, masks = K.geo_case(name)
        nom = K.geo_nominal(name)
        wrong = K.geometry_nominal64(p, image, masks, mut=mut)
        unflagged, total = _violations(nom, wrong.image, wrong.masks)
        assert total > 10 * K.cap(nom.image.size), (name, mut, unflagged, total)
    # with h == w the swap cannot show: the reason the (3, 5, 4) field is in the table
    p, image, masks = K.geo_case("128x128x2-elastic")
    same = K.geometry_nominal64(p, image, masks, mut="field_hw_swapped")
    nom = K.geo_nominal("128x128x2-elastic")
    assert _violations(nom, same.image, same.masks) == (0, 0)
    # a dropped second stride trip: the columns from 64 * 256 on stay unwritten
    for name in K.STRIDED:
        nom = K.geo_nominal(name)
        w2, h2, d2 = nom.image.shape
        got_i = nom.image.reshape(w2 * h2, d2).copy()
        got_i[K.MAX_BLOCKS_PER_Z * K.K_BLOCK:] = np.float32("nan")
        unflagged, total = _violations(nom, got_i.reshape(w2, h2, d2), nom.masks)
        if w2 * h2 > K.MAX_BLOCKS_PER_Z * K.K_BLOCK:
            assert unflagged > 0 or total > K.cap(nom.image.size), name
        else:
            assert total == 0


@pytest.mark.parametrize("shape_name", ["129x128x5", "4x4x300", "9x7x3"])
def test_intensity_mutations_leave_the_tolerance(shape_name):
    image, _ = K.intensity_inputs(shape_name)
    v = image.astype(np.float64)

    def off(stage, mut):
        kw = K.intensity_kwargs(shape_name, stage)
        ref = K.intensity64(v, **kw)
        std_used = ref_std(kw)
        return np.abs(K.intensity64(v, mut=mut, **kw) - ref).max() / K.intensity_tolerance(std_used=std_used, **kw)

    def ref_std(kw):
        return float(K.intensity64(v, upto="noise", **kw).std(ddof=1)) if kw.get("own_std") else K.r32(kw.get("std", 1.0))

    for stage in ("own-std", "own-both"):
        assert off(stage, "std_n") > 10, (stage, off(stage, "std_n"))
    assert off("all", "std_n") > 2          # 82 560 voxels move the std by 6e-6 of it, and "all" has the widest tolerance
    if shape_name == "129x128x5":
        for stage in ("contrast0.75", "contrast2", "all"):
            assert off(stage, "no_last_partial") > 10 and off(stage, "no_second_trip") > 10, stage
        # contrast_val = 0: the output is the slice mean itself, held to 255 * 2^-23
        want = K.intensity64(v, contrast=0.0, upto="noise")
        for mut in ("no_last_partial", "no_second_trip"):
            assert np.abs(K.intensity64(v, contrast=0.0, upto="noise", mut=mut) - want).max() > 1000 * 255 * 2.0 ** -23


def test_intensity_cases_reach_both_clamps():
    for shape_name in K.INTENSITY_SHAPES:
        image, _ = K.intensity_inputs(shape_name)
        v = image.astype(np.float64)
        n0, n255 = int((v == 0).sum()), int((v == 255).sum())
        up = K.intensity64(v, brightness=40.0, upto="noise")
        down = K.intensity64(v, brightness=-40.0, upto="noise")
        assert (up == 255).sum() > n255 + 0.01 * v.size and (down == 0).sum() > n0 + 0.01 * v.size
        c2 = K.intensity64(v, contrast=2.0, upto="noise")
        assert (c2 == 0).sum() > 0.01 * v.size and (c2 == 255).sum() > 0.01 * v.size
        c0 = K.intensity64(v, contrast=0.0, upto="noise")
        means = (v / 255.0).mean((0, 1)) * 255.0
        assert np.abs(c0 - means[None, None]).max() < 1e-10 and np.ptp(means) > 10       # the slices differ


def test_bake_and_average_mutations_show():
    masks, sk = K.bake_edges()
    right, d2 = K.bake_ref(masks, sk)
    wrong, d2w = K.bake_ref(masks, sk, mut="last_wins")
    assert np.array_equal(d2, d2w)
    tied = (right != wrong).any(0)
    for i in (3, 13, 23, 33):                                            # every designed tie resolves differently
        assert tied[masks == i].any(), i
    # the three-point tie: voxel (2, 1, 2) of blocks 23 / 33 is at distance 2 of all three points
    for i in (23, 33):
        x, y, z = np.argwhere(masks == i).min(0) + (2, 1, 2)
        pts = np.asarray(sk[i], np.float64)
        assert np.array_equal((((np.array([x, y, z]) - pts) * K.ANISOTROPY) ** 2).sum(1), [4.0, 4.0, 4.0])
        assert np.array_equal(right[:, x, y, z], sk[i][0]) and np.array_equal(wrong[:, x, y, z], sk[i][2])
    for absent in (1, -4, 8, 1000, 5000):
        assert (masks == absent).any() and not right[:, masks == absent].any()
    assert len(sk) == 200 and len(set(np.unique(masks)) & set(sk)) >= 170
    for shape in K.AVERAGE_SHAPES[:-1]:
        v = K.average_inputs(shape)
        if v.size > 1:
            assert (v == 0).any() and (v < 0).any()
            assert not np.array_equal(K.average_ref(v), K.average_ref(v, mut="ne0")), shape


def test_skeleton_to_mask_ref_on_the_fixture(golden):
    from skoots_amd.lib.skeleton import get_cached_disk_coords
    d = golden("augment.npz")
    shape = tuple(int(s) for s in d["s2m_shape"])
    for r, fr in ((7, 3), (9, 3)):
        offs = get_cached_disk_coords("cpu", r, fr).T.numpy()
        np.testing.assert_array_equal(K.skeleton_to_mask_ref(d["s2m_points"], offs, shape), d[f"s2m_{r}_{fr}"][0])
    # the large case: points land on every face of the volume, and values in (-1, 0) truncate to voxel 0
    offs = get_cached_disk_coords("cpu", 9, 3).T.numpy()
    m = K.skeleton_to_mask_ref(K.s2m_points(K.S2M_POINTS), offs, K.S2M_SHAPE)
    assert 0.05 < m.mean() < 0.95
    for face in (m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1]):
        assert face.any() and not face.all()
    assert torch.from_numpy(K.s2m_points(K.S2M_POINTS)[:3]).min().item() > -1
