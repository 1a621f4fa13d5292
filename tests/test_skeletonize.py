"""Training skeletons on the CPU (no GPU needed): the sequential Lee thinning restated against fixture (a), the crop
rule and the NaN row of calculate_skeletons, torch's nearest index rule, and the CLI flags.

The shapes that tests/golden/make_skeleton_golden.py and tests/test_hip_skeletonize.py share are defined here."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skeleton.npz")

# (b): scales of the fixture; the last one loses ids and raises
SCALES = [(1.0, 1.0, 1.0), (1.0, 1.0, 3.0), (0.5, 0.5, 2.0), (0.5, 0.5, 0.5)]
DIAGONAL_ID = 77777   # {(x, y + 1, z), (x + 1, y, z)}: its crop holds none of its voxels
SINGLE_ID = 5         # one voxel at odd coordinates: gone after a 0.5 downscale
THIN_AWAY_ID = 88888  # its crop holds 3 of its voxels, which thin away: the fallback row, mean x = 5 / 3 at x0 = 0


def label_volume() -> np.ndarray:
    """(40, 36, 14) int32, ~40 instances: ellipsoids painted over each other (so many touch), two boxes that touch,
    a diagonal two-voxel object, a single voxel, an object that thins away with a mean that is not dyadic, ids above
    65535 (below 2^24, so they survive the fp32 resample)."""
    rng = np.random.default_rng(7)
    v = np.zeros((40, 36, 14), np.int32)
    x, y, z = np.meshgrid(np.arange(40), np.arange(36), np.arange(14), indexing="ij")
    ids = [int(i) for i in rng.choice(np.arange(10, 300), 24, replace=False)] + \
          [65535, 65536, 70001, 123457, 1000003, 16000001] + list(range(300, 306))
    for obj in ids:
        c = rng.uniform((2, 2, 1), (38, 34, 13))
        r = rng.uniform((1.0, 1.0, 0.8), (6.0, 5.0, 3.5))
        v[((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1.0] = obj
    v[28:33, 2:6, 2:7] = 400          # two boxes that touch
    v[33:37, 2:6, 2:7] = 401
    v[0:4, 30:36, 10:14] = 0
    v[1, 32, 11] = DIAGONAL_ID
    v[2, 31, 11] = DIAGONAL_ID
    v[36:40, 30:36, 0:4] = 0
    v[37, 33, 1] = SINGLE_ID
    v[0:5, 12:17, 0:4] = 0
    for p in [(1, 0, 0), (2, 0, 0), (2, 0, 1), (0, 3, 0), (3, 3, 0), (3, 3, 2)]:
        v[p[0], 12 + p[1], p[2]] = THIN_AWAY_ID
    return v


def large_object() -> np.ndarray:
    """(84, 84, 40) bool: a thick torus (radii 30 and 8) crossed by a bar of radius 5 along x, too large for the
    LDS path of the thinning kernel."""
    x, y, z = np.meshgrid(np.arange(84) - 41.7, np.arange(84) - 41.4, np.arange(40) - 19.6, indexing="ij")
    torus = (np.sqrt(x ** 2 + y ** 2) - 30.0) ** 2 + z ** 2 <= 64.0
    bar = (y ** 2 + z ** 2 <= 25.0) & (np.abs(x) <= 32.0)
    return torus | bar


def golden():
    return np.load(GOLDEN)


def fixture_a():
    g = golden()
    out, pos = [], 0
    for shape in g["a_shapes"]:
        n = int(np.prod(shape))
        out.append((g["a_in"][pos:pos + n].reshape(shape).astype(bool), g["a_out"][pos:pos + n].reshape(shape).astype(bool)))
        pos += n
    return out


def fixture_b(si):
    """{id: (K, 3) fp32} of SCALES[si], or None where the reference raised."""
    g = golden()
    if int(g[f"b{si}_raises"]):
        return None
    keys, counts, pts = g[f"b{si}_keys"], g[f"b{si}_counts"], g[f"b{si}_points"]
    out, pos = {}, 0
    for k, c in zip(keys.tolist(), counts.tolist()):
        out[k] = pts[pos:pos + c]
        pos += c
    return out


# ---- the restatement of scikit-image 0.18.3's Lee thinning (sequential, unvectorised) ----
OFF = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


def _chi(cfg):   # Euler characteristic, foreground voxels as closed unit cubes
    pts = set()
    for (i, j, k) in np.argwhere(cfg):
        for a, b, d in itertools.product((0, 1, 2), repeat=3):
            pts.add((2 * i + a, 2 * j + b, 2 * k + d))
    return sum((-1) ** ((p[0] & 1) + (p[1] & 1) + (p[2] & 1)) for p in pts)


def _euler_inv(n):
    m = n.copy()
    m[1, 1, 1] = 0
    return _chi(n) == _chi(m)


def _simple(n):   # foreground 26-neighbours form <= 1 26-component
    fg = [o for o in OFF if o != (0, 0, 0) and n[o[0] + 1, o[1] + 1, o[2] + 1]]
    if not fg:
        return True
    s, seen, st = set(fg), {fg[0]}, [fg[0]]
    while st:
        p = st.pop()
        for q in s:
            if q not in seen and max(abs(p[i] - q[i]) for i in range(3)) <= 1:
                seen.add(q)
                st.append(q)
    return len(seen) == len(s)


def thin(img):
    """== skimage.morphology.skeletonize(img, method="lee") != 0 (scikit-image 0.18.3)."""
    im = np.pad((img != 0).astype(np.uint8), 1)
    dirs = [(0, -1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0)]
    while True:
        unchanged = 0
        for d in dirs:
            cand = []
            for p, r, c in np.argwhere(im[1:-1, 1:-1, 1:-1]) + 1:
                if im[p + d[0], r + d[1], c + d[2]]:
                    continue
                n = im[p - 1:p + 2, r - 1:r + 2, c - 1:c + 2]
                if n.sum() == 2 or not _euler_inv(n) or not _simple(n):
                    continue
                cand.append((p, r, c))
            changed = False
            for p, r, c in cand:
                if _simple(im[p - 1:p + 2, r - 1:r + 2, c - 1:c + 2]):
                    im[p, r, c] = 0
                    changed = True
            unchanged += not changed
        if unchanged == 6:
            return im[1:-1, 1:-1, 1:-1].astype(bool)


def test_restatement_matches_fixture_a():
    cases = fixture_a()
    assert len(cases) >= 100
    small = sorted(range(len(cases)), key=lambda i: cases[i][0].sum())[:40]   # the restatement is slow
    small += [len(cases) - k for k in range(1, 6)]                              # and the last stress shapes
    for i in small:
        src, want = cases[i]
        assert np.array_equal(thin(src), want), f"volume {i} of shape {src.shape}"


def test_fixture_a_skeletons_lie_in_their_volumes():
    emptied = 0
    for src, want in fixture_a():
        assert not (want & ~src).any()
        emptied += bool(src.any() and not want.any())
    # the re-check tests simplicity only, and a lone voxel counts as simple: small pieces can thin away entirely,
    # so calculate_skeletons' fallback (mean of the crop's voxels) does fire
    assert emptied > 0


def test_object_boxes_follow_the_crop_rule():
    from skoots_amd.train.generate_skeletons import _object_boxes
    v = label_volume()
    ids, lower, upper = _object_boxes(torch.from_numpy(v))
    want = [u for u in np.unique(v).tolist() if u != 0]
    assert ids.tolist() == want
    for i, obj in enumerate(want):
        nz = np.argwhere(v == obj)
        assert lower[i].tolist() == nz.min(0).tolist() and upper[i].tolist() == nz.max(0).tolist()


def test_fixture_b_crop_rule_and_nan_row():
    v = label_volume()
    sk = fixture_b(0)
    assert list(sk) == [u for u in np.unique(v).tolist() if u != 0]
    assert np.isnan(sk[DIAGONAL_ID]).all() and sk[DIAGONAL_ID].shape == (1, 3)
    assert all(not np.isnan(p).any() for k, p in sk.items() if k != DIAGONAL_ID)
    # the maximum plane of each axis is left out of the crop; the rest is the restated thinning of the crop
    checked = 0
    for obj in sorted(sk, key=lambda k: (v == k).sum())[:12]:
        if obj == DIAGONAL_ID:
            continue
        nz = np.argwhere(v == obj)
        lo, hi = nz.min(0), nz.max(0)
        hi = np.where(hi - lo == 0, hi + 1, hi)
        crop = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == obj
        skel = thin(crop)
        if skel.any():
            want = (np.argwhere(skel) + lo).astype(np.float32)
        else:   # thinned away: the fallback, the mean of the crop's voxels
            want = torch.nonzero(torch.from_numpy(crop)).float().mean(0).add(torch.from_numpy(lo).float())[None].numpy()
        assert np.array_equal(sk[obj], want), obj
        checked += 1
    assert checked >= 8
    assert fixture_b(3) is None     # the downscale loses SINGLE_ID


def test_fixture_b_thinned_away_row_is_the_cpu_mean():
    """The fallback row of an object that thins away is the reference's CPU mean, sum / n correctly rounded: for
    x = 5 / 3 at offset 0 that is 0x3FD55555, one ulp below 5 * fp32(1 / 3) (a reduction that multiplies by the
    reciprocal, as the device's mean does)."""
    v = label_volume()
    nz = np.argwhere(v == THIN_AWAY_ID)
    lo, hi = nz.min(0), nz.max(0)
    crop = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == THIN_AWAY_ID
    assert crop.sum() == 3 and not thin(crop).any() and lo[0] == 0
    for si in (0, 2):
        row = fixture_b(si)[THIN_AWAY_ID]
        scale = torch.tensor(SCALES[si])
        want = torch.nonzero(torch.from_numpy(crop)).float().mean(0).div(scale).add(torch.from_numpy(lo).div(scale))
        assert row.shape == (1, 3) and np.array_equal(row[0], want.numpy())
    x = fixture_b(0)[THIN_AWAY_ID][0, 0]
    assert x.view(np.uint32) == 0x3FD55555
    assert (np.float32(5) * (np.float32(1) / np.float32(3))).view(np.uint32) != 0x3FD55555


def test_nearest_index_rule_of_the_resample():
    """Documents torch's rule, not project code: F.interpolate(nearest) on the CPU, the reference's resample, is
    src = min(floor(float(i) * (in / out)), in - 1) in fp32, on odd ratios and the 2x / identity special cases.
    test_hip_skeletonize.py pins the device resample that calculate_skeletons uses to this CPU one."""
    rng = np.random.default_rng(3)
    vol = torch.from_numpy(rng.integers(0, 1000, size=(7, 9, 5)).astype(np.float32))
    for size in [(7, 9, 15), (3, 4, 2), (11, 13, 7), (14, 18, 10), (5, 9, 9)]:
        got = F.interpolate(vol[None, None], size=size, mode="nearest")[0, 0]
        idx = []
        for n_in, n_out in zip(vol.shape, size):
            s = np.float32(n_in) / np.float32(n_out)
            idx.append(np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * s).astype(np.int64), n_in - 1))
        want = vol.numpy()[np.ix_(*idx)]
        assert np.array_equal(got.numpy(), want), size


def test_cli_flags():
    from skoots_amd.__main__ import parse_args
    a = parse_args(["--skeletonize-train-data", "d"])
    assert a.skeletonize_train_data == "d" and a.mask_filter == ".labels"
    assert a.anisotropyXY == 1.0 and a.anisotropyZ == 1.0 and a.image is None
    a = parse_args(["--skeletonize-train-data", "f.tif", "--mask-filter", ".m", "--anisotropyXY", "0.5",
                    "--anisotropyZ", "3"])
    assert (a.mask_filter, a.anisotropyXY, a.anisotropyZ) == (".m", 0.5, 3.0)
    a = parse_args(["--image", "x.tif", "--pretrained-checkpoint", "c.trch"])
    assert a.image == "x.tif" and a.skeletonize_train_data is None
    with pytest.raises(SystemExit) as e:
        parse_args(["--pretrained-checkpoint", "c.trch"])    # eval still needs --image
    assert e.value.code == 2
