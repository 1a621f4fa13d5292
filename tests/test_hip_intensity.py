"""``sk_instance_intensity`` (skoots_amd/csrc/instance_intensity.hip) and what stands on it -- ``validate.lib``'s
``instance_intensity`` and ``intensity_ring``, the intensity and ring columns of ``stats_per_instance``, ``--image`` and
its files -- against the numpy restatement of tests/intensity_cases.py.  Every table is an integer table: every
comparison is exact.

The kernel works on tiles of 4 x 16 x 64 voxels (x, y, z), a wave per z row with the lanes along z; (5, 17, 70) and
(11, 19, 150) cross the tile on every axis with remainders and hold runs that go through z = 63 | 64.  The tile's LDS
tables hold 32 rows: ``voxel_ids`` and ``many_ids`` give a tile far more, so the direct path to global memory runs for
moments and histogram.  The image is staged by 32-bit words when Z * bytes per sample is a multiple of 4 and by samples
otherwise; the shapes cover both for both sample widths.  ``many_tiles`` has more tiles than the grid has workgroups."""
import functools

import numpy as np
import pytest
import torch

from tests import intensity_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID = 256 * 8                          # the kernel's grid rule: min(tiles, 2048) workgroups
MANY_TILES = (100, 163, 648)            # 25 x 11 x 11 = 3025 tiles of 4 x 16 x 64, about 10^7 voxels


def _many_tiles():
    rng = np.random.default_rng(77)
    v = np.where(rng.random(MANY_TILES) < 0.02, rng.integers(1, 51, MANY_TILES), 0)
    v[40:60, 30:100, 100:500] = 51      # one large body: long runs through many tiles
    return v


VOLUMES = {
    "one_voxel": lambda: np.full((1, 1, 1), 6, np.int64),
    "line_x": lambda: K.boxes((9, 1, 1), 3, 1),
    "line_y": lambda: K.boxes((1, 20, 1), 3, 2),
    "line_z": lambda: K.boxes((1, 1, 200), 4, 3),
    "below_one_tile": lambda: K.boxes((3, 5, 40), 5, 4),
    "small_crossing": lambda: K.crossing_blobs(K.SMALL_CROSSING, 5),
    "crossing": lambda: K.crossing_blobs(K.CROSSING, 6),
    "voxel_ids": lambda: K.voxel_ids((5, 6, 70)),
    "many_ids": lambda: K.many_ids(K.CROSSING, 400, 10),
    "ids_3_7_300_1000": lambda: K.crossing_blobs(K.SMALL_CROSSING, 7, ids=(3, 7, 300, 1000)),
    "id_int32_max": lambda: K.boxes((12, 13, 9), 5, 8, ids=(1, 2, 2 ** 31 - 1)),
    "all_zero": lambda: np.zeros((5, 9, 66), np.int64),
    "full": lambda: np.full((6, 18, 130), 4, np.int64),
    "many_tiles": _many_tiles,
}

IMAGES = {
    "noise": lambda s: K.noise_u8(s, 21),
    "zeros": lambda s: np.zeros(s, np.uint8),
    "all_255": lambda s: np.full(s, 255, np.uint8),
    "ramp_x": lambda s: K.ramp(s, 0),
    "ramp_y": lambda s: K.ramp(s, 1),
    "ramp_z": lambda s: K.ramp(s, 2),
    "u16": lambda s: K.noise_u16(s, 22),
    "u16_all_65535": lambda s: np.full(s, 65535, np.uint16),
    "u16_top_4000": lambda s: K.noise_u16(s, 23, 4000),
    "u16_top_200": lambda s: K.noise_u16(s, 24, 200),
}


@functools.lru_cache(maxsize=None)
def volume(name):
    v = np.ascontiguousarray(VOLUMES[name]()).astype(np.int64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def image(name, vname):
    v = np.ascontiguousarray(IMAGES[name](volume(vname).shape))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def want(vname, iname, shift):
    out = K.ref_intensity(volume(vname), image(iname, vname), shift)
    for a in out:
        a.setflags(write=False)
    return out


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached arrays are read-only


def image_on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def auto_shift(a):
    return 0 if a.dtype == np.uint8 else max(int(a.max(initial=0)).bit_length() - 8, 0)


def check(vname, iname, shift=None, dtype=None, lead=False, **kw):
    from skoots_amd.validate.lib import instance_intensity
    x, img = on_device(volume(vname), dtype), image_on_device(image(iname, vname))
    if lead:
        x, img = x[None], img[None]
    ids, m, e, h, s = instance_intensity(x, img, shift=shift, **kw)
    assert s == (auto_shift(image(iname, vname)) if shift is None else shift)
    wm, we, wh = want(vname, iname, s)
    assert ids.dtype == torch.int64 and m.dtype == torch.int64 and e.dtype == torch.int32 and m.is_cuda and e.is_cuda
    assert np.array_equal(ids.cpu().numpy(), K.rows_of(volume(vname))[1])
    assert tuple(m.shape) == (ids.numel(), 6) and tuple(e.shape) == (ids.numel(), 2)
    assert np.array_equal(m.cpu().numpy(), wm)
    assert np.array_equal(e.cpu().numpy().astype(np.int64), we)
    if kw.get("want_hist", True):
        assert h.dtype == torch.int64 and h.is_cuda and tuple(h.shape) == (ids.numel(), 256)
        assert np.array_equal(h.cpu().numpy(), wh)
        assert np.array_equal(h.sum(1).cpu().numpy(), wm[:, 0])
    else:
        assert h is None
    return ids, m, e, h, s


SHAPE_CASES = [(v, i) for v in ("one_voxel", "line_x", "line_y", "line_z", "below_one_tile", "small_crossing", "crossing",
                                "full") for i in ("noise", "u16")]
IMAGE_CASES = [("crossing", i) for i in IMAGES if i not in ("noise", "u16")] + \
              [("small_crossing", i) for i in ("all_255", "u16_all_65535", "ramp_x", "ramp_y", "ramp_z")]
ID_CASES = [(v, i) for v in ("voxel_ids", "many_ids", "ids_3_7_300_1000", "id_int32_max")
            for i in ("noise", "all_255", "u16", "u16_top_4000")]


@pytest.mark.parametrize("vname,iname", SHAPE_CASES + IMAGE_CASES + ID_CASES)
def test_tables_match_the_restatement(vname, iname):
    check(vname, iname)


def test_more_tiles_than_workgroups():
    X, Y, Z = MANY_TILES
    assert -(-X // 4) * -(-Y // 16) * -(-Z // 64) > GRID and Z % 4 == 0 and Z % 64 != 0
    ids = check("many_tiles", "noise")[0]
    assert ids.numel() == 51


@pytest.mark.parametrize("iname,shift", [("u16_top_200", 0), ("u16_top_200", 8), ("u16_top_4000", 4), ("u16_top_4000", 8),
                                         ("u16", 8), ("noise", 0)])
def test_forced_shift(iname, shift):
    check("crossing", iname, shift=shift)


def test_a_shift_that_leaves_samples_outside_the_bins_is_refused():
    from skoots_amd.validate.lib import instance_intensity
    x = on_device(volume("small_crossing"))
    for iname, shift in (("u16", 7), ("u16_top_4000", 3), ("noise", 1), ("u16", 9), ("u16", -1), ("u16", 1.5)):
        with pytest.raises(ValueError, match="shift"):
            instance_intensity(x, image_on_device(image(iname, "small_crossing")), shift=shift)


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64])
def test_mask_dtypes(dtype):
    check("small_crossing", "noise", dtype=dtype)


def test_id_int32_max_as_int64_takes_the_relabel_path():
    from skoots_amd.validate.lib import id_rows
    x = on_device(volume("id_int32_max"), torch.int64)
    a, ids, lut, max_id = id_rows(x)[1]
    assert max_id == 3 and ids.tolist() == [1, 2, 2 ** 31 - 1] and int(a.max()) == 3      # rows, not ids, reach the kernel
    check("id_int32_max", "u16", dtype=torch.int64)
    check("id_int32_max", "ramp_y", dtype=torch.int64)


def test_leading_axis_and_zero_and_negative_background():
    assert (volume("crossing") < 0).any() and (volume("crossing") == 0).any()
    check("crossing", "noise", lead=True)
    check("small_crossing", "u16", lead=True)


def test_signed_images():
    from skoots_amd.validate.lib import instance_intensity
    x = on_device(volume("crossing"))
    for iname, dtype in (("u16", torch.int32), ("u16", torch.int64), ("noise", torch.int16), ("u16_top_200", torch.int32)):
        a = image(iname, "crossing")
        got = instance_intensity(x, torch.from_numpy(a.astype(np.int64)).to(dtype).to(DEV))
        s = max(int(a.max()).bit_length() - 8, 0)
        assert got[4] == s
        for g, w in zip(got[1:4], want("crossing", iname, s)):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), w)
    small = (image("noise", "crossing") // 2).astype(np.int8)
    got = instance_intensity(x, torch.from_numpy(small).to(DEV))
    for g, w in zip(got[1:4], K.ref_intensity(volume("crossing"), small, 0)):
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w)
    bad = image("u16", "crossing").astype(np.int32)
    bad[3, 4, 5] = 70000
    with pytest.raises(ValueError, match="70000"):
        instance_intensity(x, torch.from_numpy(bad).to(DEV))
    bad[3, 4, 5] = -1
    with pytest.raises(ValueError, match="-1"):
        instance_intensity(x, torch.from_numpy(bad).to(DEV))
    with pytest.raises(TypeError, match="float16"):
        instance_intensity(x, torch.zeros(tuple(x.shape), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="shape"):
        instance_intensity(x, torch.zeros((11, 19, 149), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="device"):
        instance_intensity(x, torch.zeros(tuple(x.shape), dtype=torch.uint8))


def test_empty_mask_gives_empty_tables():
    ids, m, e, h, s = check("all_zero", "noise")
    assert ids.numel() == 0 and tuple(m.shape) == (0, 6) and tuple(e.shape) == (0, 2) and tuple(h.shape) == (0, 256)
    assert check("all_zero", "u16", want_hist=False)[4] == 8


@pytest.mark.parametrize("vname,iname", [("crossing", "noise"), ("many_ids", "u16"), ("voxel_ids", "all_255")])
def test_without_histogram_and_twice(vname, iname):
    a = check(vname, iname)
    b = check(vname, iname)
    c = check(vname, iname, want_hist=False)
    for p, q in zip(a[:4], b[:4]):
        assert torch.equal(p, q)
    assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]) and c[3] is None


def test_rows_can_be_shared_with_instance_sums():
    from skoots_amd.validate.lib import id_rows, instance_intensity, instance_sums
    x = on_device(volume("ids_3_7_300_1000"))
    rows = id_rows(x)
    ids, sums, _ = instance_sums(x, rows)
    got = instance_intensity(x, image_on_device(image("ramp_z", "ids_3_7_300_1000")), rows)
    assert torch.equal(got[0], ids) and torch.equal(got[1][:, 0], sums[:, 0])
    # the ramp along z is 1 + z here (Z <= 251): S v = S z + n
    assert torch.equal(got[1][:, 1], sums[:, 3] + sums[:, 0])


# ---- the ring ----

def test_ring_of_two_balls_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    from skoots_amd.validate.lib import intensity_ring
    mask = K.two_balls()
    img = K.noise_u8(mask.shape, 31)
    spacing, D = (1.0, 1.0, 3.0), 3.0
    ring = np.zeros(mask.shape, np.int64)
    near_any = ndi.distance_transform_edt(mask == 0, sampling=spacing) <= D
    for row, u in enumerate((5, 10)):
        mine = (mask == 0) & (ndi.distance_transform_edt(mask != u, sampling=spacing) <= D)
        assert not (ring[mine] != 0).any()                                # no voxel is within D of both: no ties
        ring[mine] = row + 1
    assert np.array_equal(ring > 0, near_any & (mask == 0)) and (ring == 1).sum() > 100 and (ring == 2).sum() > 100
    wm, we, _ = K.table_of_rows(ring, 2, img, want_hist=False)
    m, e = intensity_ring(on_device(mask), image_on_device(img), D, spacing)
    assert m.dtype == torch.int64 and e.dtype == torch.int32 and m.is_cuda
    assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(e.cpu().numpy().astype(np.int64), we)
    rm, re_ = K.ref_ring(mask, img, D, spacing)
    assert np.array_equal(rm, wm) and np.array_equal(re_, we)


@pytest.mark.parametrize("vname,iname,D,spacing", [("crossing", "noise", 3.0, (1.0, 1.0, 3.0)),
                                                   ("crossing", "u16", 2.0, (1.0, 1.0, 1.0)),
                                                   ("id_int32_max", "noise", 1.5, (1.0, 0.5, 2.0)),
                                                   ("ids_3_7_300_1000", "u16", 4.0, (2.0, 1.0, 3.0)),
                                                   ("full", "noise", 3.0, (1.0, 1.0, 1.0))])
def test_ring_against_the_restatement(vname, iname, D, spacing):
    from skoots_amd.validate.lib import intensity_ring
    wm, we = K.ref_ring(volume(vname), image(iname, vname), D, spacing)
    m, e = intensity_ring(on_device(volume(vname)), image_on_device(image(iname, vname)), D, spacing)
    assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(e.cpu().numpy().astype(np.int64), we)
    if vname == "full":
        assert (wm == 0).all() and (we == [K.INT32_MAX, -1]).all()       # no background: every ring is empty
    else:
        assert wm[:, 0].sum() > 0
    m2, e2 = intensity_ring(on_device(volume(vname)), image_on_device(image(iname, vname)), D, spacing)
    assert torch.equal(m, m2) and torch.equal(e, e2)


def test_ring_of_an_empty_mask():
    from skoots_amd.validate.lib import intensity_ring
    m, e = intensity_ring(on_device(volume("all_zero")), image_on_device(image("noise", "all_zero")), 2.0)
    assert tuple(m.shape) == (0, 6) and tuple(e.shape) == (0, 2)


# ---- stats_per_instance, get_intensity, the command ----

def test_stats_per_instance_keys_dtypes_and_values():
    from skoots_amd.validate import compare as CMP
    from skoots_amd.validate.stats import get_intensity
    vname, iname, spacing, D = "ids_3_7_300_1000", "u16_top_4000", (1.0, 0.5, 2.0), 2.5
    x, img = on_device(volume(vname)), image_on_device(image(iname, vname))
    plain = CMP.stats_per_instance(x, spacing)
    assert not any("intensity" in k or "ring" in k or k == "contrast" for k in plain)
    got = CMP.stats_per_instance(x, spacing, image=img)
    assert set(got) - set(plain) == {"intensity_moments", "intensity_extrema", "intensity_hist", "intensity_shift",
                                     "intensity_mean", "intensity_std", "intensity_min", "intensity_max",
                                     "intensity_median", "intensity_p05", "intensity_p95", "weighted_centroid"}
    for k in plain:
        assert torch.equal(plain[k], got[k]), k
    both = CMP.stats_per_instance(x, spacing, image=img, intensity_ring=D)
    assert set(both) - set(got) == {"ring_moments", "ring_voxels", "ring_mean", "ring_std", "contrast"}
    shift = 4
    wm, we, wh = want(vname, iname, shift)
    assert both["intensity_shift"] == shift
    assert np.array_equal(both["intensity_moments"].cpu().numpy(), wm) and both["intensity_moments"].dtype == torch.int64
    assert np.array_equal(both["intensity_extrema"].cpu().numpy(), we) and both["intensity_extrema"].dtype == torch.int32
    assert np.array_equal(both["intensity_hist"].cpu().numpy(), wh) and both["intensity_hist"].dtype == torch.int64
    cols = CMP.intensity_columns(wm, we, wh, shift, spacing)
    rm, _ = K.ref_ring(volume(vname), image(iname, vname), D, spacing)
    assert np.array_equal(both["ring_moments"].cpu().numpy(), rm)
    cols.update(CMP.ring_columns(rm, wm))
    for k, v in cols.items():
        assert both[k].is_cuda and both[k].dtype == v.dtype and tuple(both[k].shape) == tuple(v.shape), k
        assert np.array_equal(both[k].cpu().numpy(), v.numpy(), equal_nan=v.dtype == torch.float64), k
    for k in ("intensity_mean", "intensity_std", "ring_mean", "ring_std", "contrast", "weighted_centroid"):
        assert both[k].dtype == torch.float64
    for k in ("intensity_min", "intensity_max", "intensity_median", "intensity_p05", "intensity_p95", "ring_voxels"):
        assert both[k].dtype == torch.int64
    with pytest.raises(ValueError, match="image"):
        CMP.stats_per_instance(x, spacing, intensity_ring=D)
    mean = get_intensity(x, img)
    assert mean.is_cuda and mean.dtype == torch.float64 and torch.equal(mean, both["intensity_mean"])
    assert get_intensity(on_device(volume("all_zero")), image_on_device(image("noise", "all_zero"))).numel() == 0


def test_compare_command_writes_the_intensity_files(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate import compare as CMP
    from skoots_amd.validate.lib import instance_intensity, intensity_ring
    vname, iname = "ids_3_7_300_1000", "u16_top_4000"
    m, a = np.clip(volume(vname), 0, None), image(iname, vname)      # the file holds unsigned labels: no negative ones
    x, img = on_device(m), image_on_device(a)
    path, ipath = str(tmp_path / "mask.tif"), str(tmp_path / "image.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())            # stored [Z, X, Y]
    tiff.write_stack(ipath, image_on_device(np.ascontiguousarray(a.transpose(2, 0, 1))))
    ids = K.rows_of(m)[1]
    base = CMP.stats_per_instance(x, (1.0, 1.0, 3.0))
    plain = open(CMP.main([path, "--spacing", "1", "1", "3", "--out", str(tmp_path / "a.csv")])).read()
    assert plain == CMP.format_csv(path, ids, base["sums"], base["bbox"], m.shape, (1.0, 1.0, 3.0))
    assert not (tmp_path / "mask_histograms.csv").exists()
    out = CMP.main([path, "--spacing", "1", "1", "3", "--image", ipath, "--intensity-ring", "3", "--save-histograms"])
    assert out == str(tmp_path / "mask_instance_stats.csv")
    tables = instance_intensity(x, img)[1:]
    ring = intensity_ring(x, img, 3.0, (1.0, 1.0, 3.0))[0]
    want_text = CMP.format_csv(path, ids, base["sums"], base["bbox"], m.shape, (1.0, 1.0, 3.0), intensity=tables, ring=ring)
    assert open(out).read() == want_text
    assert want_text.splitlines()[2] == CMP.CSV_COLUMNS + "," + CMP.INTENSITY_COLUMNS + "," + CMP.RING_COLUMNS
    assert all(lb.startswith(la + ",") for la, lb in zip(plain.splitlines()[3:], want_text.splitlines()[3:]))
    assert open(tmp_path / "mask_histograms.csv").read() == CMP.format_histograms_csv(path, ids, tables[2], tables[3])
    assert tables[3] == 4
    # an 8-bit .npy image, and the refusals that name both files
    npy = str(tmp_path / "image.npy")
    np.save(npy, np.ascontiguousarray(image("noise", vname).transpose(2, 0, 1)))
    out8 = open(CMP.main([path, "--image", npy, "--out", str(tmp_path / "b.csv")])).read()
    t8 = instance_intensity(x, image_on_device(image("noise", vname)))[1:]
    assert out8 == CMP.format_csv(path, ids, base["sums"], base["bbox"], m.shape, intensity=t8)
    np.save(npy, np.zeros((3, 4, 5), np.uint8))
    with pytest.raises(ValueError, match=r"image\.npy.*mask\.tif"):
        CMP.main([path, "--image", npy])
    np.save(npy, np.zeros(a.transpose(2, 0, 1).shape, np.float32))
    with pytest.raises(ValueError, match=r"float32.*mask\.tif"):
        CMP.main([path, "--image", npy])
    with pytest.raises(SystemExit):
        CMP.main([path, "--intensity-ring", "3"])


# ---- the entry point ----

def test_entry_point_refusals_and_versions():
    from skoots_amd import _ffi
    L = _ffi.lib
    assert L.sk_abi_version() >= 25
    assert [L.sk_instance_intensity_row_values(k) for k in range(3)] == [6, 2, 256]
    x = on_device(volume("below_one_tile"), torch.int32)
    X, Y, Z = x.shape
    lut = torch.arange(8, dtype=torch.int32, device=DEV)
    img = image_on_device(image("noise", "below_one_tile"))
    sentinel = 0x5A5A5A5A5A5A5A5A
    m = torch.full((7, 6), sentinel, dtype=torch.int64, device=DEV)
    e = torch.full((7, 2), 1234567, dtype=torch.int32, device=DEV)
    h = torch.full((7, 256), sentinel, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(x.device)

    def call(X=X, Y=Y, Z=Z, eb=1, shift=0, N=7, labels=x, moments=m, image=img):
        return L.sk_instance_intensity(_ffi.ptr(labels), X, Y, Z, _ffi.ptr(lut), 7, N, _ffi.ptr(image), eb, shift,
                                       _ffi.ptr(moments), _ffi.ptr(e), _ffi.ptr(h), st)

    for kw, word in ((dict(eb=3), "elem_bytes"), (dict(eb=0), "elem_bytes"), (dict(eb=2, shift=9), "shift"),
                     (dict(shift=1), "shift"), (dict(shift=-1), "shift"), (dict(X=-1), "negative"), (dict(N=-1), "negative"),
                     (dict(moments=None), "NULL"), (dict(labels=None), "NULL"), (dict(image=None), "NULL")):
        assert call(**kw) == -1 and word in _ffi.last_error(), kw
    assert L.sk_instance_intensity(None, 2 ** 21, 2 ** 21, 2 ** 21, None, 7, 7, None, 1, 0, None, None, None, st) == -1
    assert "2^63" in _ffi.last_error()
    assert L.sk_instance_intensity(None, 2 ** 14, 2 ** 14, 2 ** 10, None, 7, 7, None, 2, 0, None, None, None, st) == -1
    torch.cuda.synchronize()
    assert bool((m == sentinel).all()) and bool((e == 1234567).all()) and bool((h == sentinel).all())   # nothing was written
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert bool((m == sentinel).all())
    assert call(Z=0) == 0                                                 # an empty volume: the outputs are initialised
    torch.cuda.synchronize()
    assert bool((m == 0).all()) and bool((h == 0).all()) and e.tolist() == [[2 ** 31 - 1, -1]] * 7
    assert call() == 0
    wm, we, wh = K.table_of_rows(np.clip(volume("below_one_tile"), 0, None), 7, image("noise", "below_one_tile"))
    assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(e.cpu().numpy(), we) and np.array_equal(h.cpu().numpy(), wh)
