"""``sk_label_edt`` (skoots_amd/csrc/edt.hip) and everything on top of it -- ``lib.morphology.label_edt``,
``validate.lib.instance_thickness``, ``stats_per_instance(thickness=...)``, ``get_inscribed_radius`` and
``python -m skoots_amd.validate.compare --thickness / --save-distance`` -- against the numpy oracle of
tests/edt_cases.py, which tests/test_edt_cpu.py holds against the pairwise brute force and against scipy.  The kernel
computes a defined sequence of roundings, so every comparison of its output is equality of bits.

The shapes (tests/edt_cases.py) have extents of 1 in every axis, lines that are no multiple of the 64 lanes, more than
one workgroup, walks of 13 steps, instances that touch each other and every face of the volume, and an instance that is
alone in the volume."""
import os

import numpy as np
import pytest
import torch

from tests.edt_cases import BALL, BLOBS, INF, MODES, SPACINGS, cases, expected, row_max, weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = cases()
SMALL_IDS = "cross (9, 11, 37)"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(name, x, spacing, closed):
    from skoots_amd.lib.morphology import label_edt
    ids, rows, want = expected(name, spacing, closed)
    d2, mx = label_edt(x, spacing, closed)
    assert d2.dtype == torch.float64 and mx.dtype == torch.float64 and d2.is_cuda and mx.is_cuda
    assert tuple(d2.shape) == rows.shape and tuple(mx.shape) == (len(ids),)
    got = d2.cpu().numpy()
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{name} {spacing} closed={closed}: {len(bad)} voxels differ, first {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert np.array_equal(bits(mx.cpu().numpy()), bits(row_max(rows, want))), (name, spacing, closed)
    return d2, mx


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_every_spacing_both_modes(name):
    lab = CASES[name]
    x = torch.from_numpy(lab).to(DEV)
    assert x.dtype == (torch.int64 if "int64" in name else torch.int32)
    for spacing in SPACINGS:
        for closed in MODES:
            check(name, x, spacing, closed)


def test_scipy_as_a_second_witness():
    from scipy import ndimage
    from skoots_amd.lib.morphology import label_edt
    x = torch.from_numpy(CASES[BALL]).to(DEV)
    got = np.sqrt(label_edt(x, (1.0, 1.0, 3.0))[0].cpu().numpy())
    assert np.array_equal(got, ndimage.distance_transform_edt(CASES[BALL] > 0, sampling=(1.0, 1.0, 3.0)))
    lab = CASES[BLOBS]
    got = np.sqrt(label_edt(torch.from_numpy(lab).to(DEV), (2.0, 1.0, 5.0), closed=True)[0].cpu().numpy())
    for u in np.unique(lab[lab > 0])[:8]:
        ref = ndimage.distance_transform_edt(np.pad(lab == u, 1), sampling=(2.0, 1.0, 5.0))[1:-1, 1:-1, 1:-1]
        assert np.array_equal(got[lab == u], ref[lab == u]), u


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64])
def test_integer_dtypes_and_a_view(dtype):
    lab = CASES[SMALL_IDS]
    x = torch.from_numpy(lab).to(dtype).to(DEV)
    check(SMALL_IDS, x, SPACINGS[3], False)
    check(SMALL_IDS, x[None], SPACINGS[1], True)                       # (1, X, Y, Z)
    view = torch.from_numpy(np.ascontiguousarray(lab.transpose(2, 0, 1))).to(dtype).to(DEV).permute(1, 2, 0)
    assert not view.is_contiguous() and tuple(view.shape) == lab.shape
    check(SMALL_IDS, view, SPACINGS[3], True)


def test_huge_ids_take_the_relabel_route(monkeypatch):
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.lib import instance_thickness
    monkeypatch.setattr(VL, "_lut", lambda m: pytest.fail("the max id + 1 table was built for a huge id"))
    for name in ("huge int32 (4, 5, 36)", "huge int64 (4, 5, 36)"):
        x = torch.from_numpy(CASES[name]).to(DEV)
        check(name, x, SPACINGS[3], False)
        ids, mx, d2 = instance_thickness(x, SPACINGS[1], closed=True)
        want = expected(name, SPACINGS[1], True)
        assert ids.tolist() == want[0].tolist() and np.array_equal(bits(d2.cpu().numpy()), bits(want[2]))
    assert ids.tolist() == [70000, 2 ** 30, 2 ** 40]


def test_two_runs_give_identical_bits():
    from skoots_amd.lib.morphology import label_edt
    x = torch.from_numpy(CASES[BLOBS]).to(DEV)
    a = label_edt(x, SPACINGS[3], True)
    b = label_edt(x, SPACINGS[3], True)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_passes_one_by_one_and_without_row_max():
    """sk_label_edt is sk_label_edt_pass for z, y and x; row_max may be NULL"""
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    x = torch.from_numpy(CASES[BLOBS]).to(DEV)
    _, (a, ids, lut, max_id) = id_rows(x)
    X, Y, Z = a.shape
    N = int(ids.numel())
    wx, wy, wz = weights(SPACINGS[3])
    want = expected(BLOBS, SPACINGS[3], False)
    one = torch.full((X, Y, Z), -1.0, dtype=torch.float64, device=DEV)
    two = torch.full((X, Y, Z), -1.0, dtype=torch.float64, device=DEV)
    mx = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(a.device)
    args = (_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N)
    _ffi.check(_ffi.lib.sk_label_edt_pass(*args, 2, wz, 0, None, _ffi.ptr(one), None, st))
    _ffi.check(_ffi.lib.sk_label_edt_pass(*args, 1, wy, 0, _ffi.ptr(one), _ffi.ptr(two), None, st))
    _ffi.check(_ffi.lib.sk_label_edt_pass(*args, 0, wx, 0, _ffi.ptr(two), _ffi.ptr(one), _ffi.ptr(mx), st))
    assert np.array_equal(bits(one.cpu().numpy()), bits(want[2]))
    assert np.array_equal(mx.cpu().numpy().view(np.uint64), bits(row_max(want[1], want[2])))
    one.fill_(-1.0)
    _ffi.check(_ffi.lib.sk_label_edt(*args, wx, wy, wz, 0, _ffi.ptr(one), _ffi.ptr(two), None, st))
    assert np.array_equal(bits(one.cpu().numpy()), bits(want[2]))


def test_c_abi_guards_write_nothing():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 17
    X, Y, Z, N, max_id = 4, 5, 6, 2, 9
    lab = torch.zeros((X, Y, Z), dtype=torch.int32, device=DEV)
    lab[1:3, 1:4, 1:5] = 9
    lab[0, 0, 0] = 3
    lut = torch.zeros(max_id + 1, dtype=torch.int32, device=DEV)
    lut[3], lut[9] = 1, 2
    d2 = torch.full((X * Y * Z + 1,), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((X * Y * Z + 1,), -7.0, dtype=torch.float64, device=DEV)
    mx = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    base = dict(labels=_ffi.ptr(lab), X=X, Y=Y, Z=Z, lut=_ffi.ptr(lut), max_id=max_id, N=N, wx=1.0, wy=0.25, wz=9.0,
                closed=0, dist2=_ffi.ptr(d2), scratch=_ffi.ptr(scratch), row_max=_ffi.ptr(mx))

    def call(**kw):
        a = dict(base, **kw)
        rc = _ffi.lib.sk_label_edt(*(a[k] for k in base), _ffi.stream_ptr(lab.device))
        torch.cuda.synchronize()
        return rc

    for null in ("labels", "lut", "dist2", "scratch"):
        assert call(**{null: None}) == -1 and "sk_label_edt: NULL" in _ffi.last_error(), null
    assert call(dist2=d2.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert call(scratch=scratch.data_ptr() + 4) == -1 and call(row_max=mx.data_ptr() + 4) == -1
    assert call(labels=lab.data_ptr() + 2) == -1 and call(lut=lut.data_ptr() + 2) == -1
    for k in ("X", "Y", "Z", "N", "max_id"):
        assert call(**{k: -1}) == -1 and "negative" in _ffi.last_error(), k
    assert call(X=2 ** 26 + 1, Y=1, Z=1) == -1 and "2^26" in _ffi.last_error()
    assert call(X=2 ** 26, Y=2 ** 26, Z=2 ** 26) == -1 and "2^62" in _ffi.last_error()
    assert call(closed=2) == -1 and call(closed=-1) == -1 and "closed" in _ffi.last_error()
    for k in ("wx", "wy", "wz"):
        for v in (0.0, -1.0, INF, float("nan")):
            assert call(**{k: v}) == -1 and "weights" in _ffi.last_error(), (k, v)
    assert call(scratch=_ffi.ptr(d2)) == -1 and "in place" in _ffi.last_error()
    assert _ffi.lib.sk_label_edt_pass(_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), max_id, N, 3, 1.0, 0, _ffi.ptr(scratch),
                                      _ffi.ptr(d2), _ffi.ptr(mx), _ffi.stream_ptr(lab.device)) == -1
    assert "axis" in _ffi.last_error()
    assert _ffi.lib.sk_label_edt_pass(_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), max_id, N, 1, 1.0, 0, None,
                                      _ffi.ptr(d2), _ffi.ptr(mx), _ffi.stream_ptr(lab.device)) == -1
    # an empty volume and N == 0 are not errors, and write nothing either
    assert call(X=0) == 0 and call(Y=0) == 0 and call(Z=0) == 0 and call(N=0) == 0
    assert call(X=0, labels=None, dist2=None, scratch=None) == 0
    assert bool((d2 == -7.0).all()) and bool((scratch == -7.0).all()) and bool((mx == -7).all())
    # and the same buffers take a real run: nothing is written behind their ends
    assert call(closed=1) == 0
    assert bool(d2[-1] == -7.0) and bool(scratch[-1] == -7.0) and bool(mx[-1] == -7)
    got = d2[:-1].view(X, Y, Z)
    assert got[0, 0, 0].item() == 0.25 and got[1, 1, 1].item() == 0.25 and got[2, 2, 2].item() == 1.0
    assert mx[:2].view(torch.float64).tolist() == [0.25, 1.0]


def test_host_guards_and_empty_masks():
    from skoots_amd.lib.morphology import label_edt
    from skoots_amd.validate.lib import instance_thickness
    for x in (torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV), torch.full((3, 3, 3), -5, dtype=torch.int32,
                                                                                   device=DEV),
              torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV)):
        ids, mx, d2 = instance_thickness(x, (1.0, 2.0, 3.0))
        assert tuple(ids.shape) == (0,) and tuple(mx.shape) == (0,) and mx.dtype == torch.float64 and mx.is_cuda
        assert tuple(d2.shape) == tuple(x.shape) and d2.dtype == torch.float64 and not bool(d2.any())
    x = torch.ones((3, 3, 3), dtype=torch.int32, device=DEV)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, INF, 1.0), (1e200, 1.0, 1.0), (1e-200, 1.0, 1.0)):
        with pytest.raises(ValueError):
            label_edt(x, bad)
    with pytest.raises(TypeError):
        label_edt(torch.zeros((3, 3, 3), device=DEV))
    with pytest.raises(ValueError):
        label_edt(torch.zeros((3, 3, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        instance_thickness(x, skeleton=torch.zeros((3, 3, 4), dtype=torch.int32, device=DEV))
    # alone in the volume: inf in open mode, the faces in closed mode
    assert label_edt(x)[1].tolist() == [INF] and label_edt(x, closed=True)[1].tolist() == [4.0]


def _skeleton_stats(rows, d2, skel):
    """(N, 3): mean, min, max of sqrt(d2) over the voxels of each row of the skeleton volume, summed in raster order;
    the rounded mean is kept inside [min, max]"""
    out = np.zeros((int(rows.max()), 3))
    for r in range(1, out.shape[0] + 1):
        v = np.sqrt(d2[skel == r]).tolist()
        if v:
            total = 0.0
            for t in v:
                total += t
            out[r - 1] = (min(max(total / len(v), min(v)), max(v)), min(v), max(v))
    return out


def test_skeleton_radius_columns():
    from skoots_amd.validate.lib import id_rows, instance_skeleton_graph, instance_thickness
    x = torch.from_numpy(CASES[BLOBS]).to(DEV)
    rows = id_rows(x)
    _, graph, skel = instance_skeleton_graph(x, rows, want_volume=True)
    empty = (graph[:, 0] == 0).cpu().numpy()
    assert empty.sum() == 6                                            # instances that thin away
    for spacing, closed in ((SPACINGS[1], False), (SPACINGS[3], True)):
        ids, rws, want = expected(BLOBS, spacing, closed)
        got_ids, mx, d2, st = instance_thickness(x, spacing, closed, rows, skel)
        assert got_ids.tolist() == ids.tolist() and not st.is_cuda and st.dtype == torch.float64
        assert tuple(st.shape) == (len(ids), 3)
        ref = _skeleton_stats(rws, want, skel.cpu().numpy())
        assert np.array_equal(bits(st.numpy()), bits(ref))
        assert (st.numpy()[empty] == 0.0).all() and (st.numpy()[~empty] > 0.0).all()
        assert (st.numpy()[:, 1] <= st.numpy()[:, 0]).all() and (st.numpy()[:, 0] <= st.numpy()[:, 2]).all()
        assert (st.numpy()[:, 2] <= np.sqrt(mx.cpu().numpy())).all()
        again = instance_thickness(x, spacing, closed, skeleton=skel)
        assert torch.equal(again[3], st) and torch.equal(again[1], mx)


def test_stats_per_instance_and_get_inscribed_radius():
    from skoots_amd.validate.compare import stats_per_instance, thickness_columns
    from skoots_amd.validate.stats import get_inscribed_radius
    lab = CASES[BLOBS]
    x = torch.from_numpy(lab).to(DEV)
    spacing = SPACINGS[1]
    plain = stats_per_instance(x, spacing)
    assert set(plain) == {"id", "voxels", "volume", "bbox", "touches_border", "centroid", "face_area", "faces",
                          "axis_lengths", "sums"}
    assert set(stats_per_instance(x, spacing, thickness=None)) == set(plain)
    with_skeleton = stats_per_instance(x, spacing, skeleton=True)
    for mode in ("open", "closed"):
        ids, rows, want = expected(BLOBS, spacing, mode == "closed")
        st = stats_per_instance(x[None], spacing, thickness=mode)
        assert set(st) - set(plain) == {"inscribed_radius", "max_dist2", "dist2"}
        assert all(torch.equal(st[k], plain[k]) for k in plain)
        assert st["id"].tolist() == ids.tolist() and st["dist2"].is_cuda and st["inscribed_radius"].is_cuda
        assert np.array_equal(bits(st["dist2"].cpu().numpy()), bits(want))
        assert np.array_equal(bits(st["max_dist2"].cpu().numpy()), bits(row_max(rows, want)))
        assert np.array_equal(bits(st["inscribed_radius"].cpu().numpy()), bits(np.sqrt(row_max(rows, want))))
        both = stats_per_instance(x, spacing, surface="closed", skeleton=True, thickness=mode)
        assert set(both) - set(with_skeleton) == {"mesh_cells", "surface_area", "surface_to_volume", "inscribed_radius",
                                                  "max_dist2", "dist2", "skeleton_radius_mean", "skeleton_radius_min",
                                                  "skeleton_radius_max"}
        assert all(torch.equal(both[k], with_skeleton[k]) for k in with_skeleton)
        assert torch.equal(both["inscribed_radius"], st["inscribed_radius"])
        col = thickness_columns(both["max_dist2"], torch.stack([both[f"skeleton_radius_{k}"] for k in
                                                                ("mean", "min", "max")], dim=1))
        assert all(torch.equal(both[k].cpu(), v) for k, v in col.items())
        assert bool((both["skeleton_radius_max"] <= both["inscribed_radius"]).all())
    with pytest.raises(ValueError):
        stats_per_instance(x, spacing, thickness="yes")
    u = int(np.unique(lab[lab > 0])[3])
    i = ids.tolist().index(u)
    for closed in MODES:
        one = get_inscribed_radius(x == u, spacing, closed)
        ref = np.sqrt(expected(BLOBS, spacing, closed)[2][lab == u].max())
        # one id alone: the other instances are background here too, so the value is the all-instances one
        assert one.dtype == torch.float64 and one.is_cuda and one.item() == ref
    assert one.item() == st["inscribed_radius"][i].item()
    assert get_inscribed_radius(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]).item() == 0.0
    assert get_inscribed_radius(torch.ones((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]).item() == INF


def test_command_end_to_end(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import main
    from tests.test_edt_cpu import read_float_tiff
    lab = CASES[BLOBS]
    spacing = SPACINGS[1]
    ids, rows, want = expected(BLOBS, spacing, False)
    x = torch.from_numpy(lab).to(DEV)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read().splitlines()
    assert not os.path.exists(os.path.join(tmp_path, "mito_distance.tif"))
    assert plain[2].count(",") == 16 and "radius" not in plain[2]
    with_s = open(main(args + ["--skeleton", "--out", os.path.join(tmp_path, "s.csv")])).read().splitlines()
    out = main(args + ["--skeleton", "--thickness", "open", "--save-distance"])
    assert out == os.path.join(tmp_path, "mito_instance_stats.csv")
    lines = open(out).read().splitlines()
    assert lines[:2] == with_s[:2] and lines[2] == with_s[2] + ",inscribed_radius,skeleton_radius_mean," \
        "skeleton_radius_min,skeleton_radius_max"
    assert [ln.split(",")[:22] for ln in lines[3:]] == [ln.split(",") for ln in with_s[3:]]
    keep = np.array([(lab == u).sum() >= 2 for u in ids])
    assert keep.any() and [int(ln.split(",")[0]) for ln in lines[3:]] == ids[keep].tolist()
    radius = [float(ln.split(",")[22]) for ln in lines[3:]]
    assert radius == np.sqrt(row_max(rows, want))[keep].tolist()
    from skoots_amd.validate.lib import instance_skeleton_graph
    skel = instance_skeleton_graph(x, want_volume=True)[2].cpu().numpy()
    ref = _skeleton_stats(rows, want, skel)[keep]
    assert [[float(v) for v in ln.split(",")[23:]] for ln in lines[3:]] == ref.tolist()
    # --save-distance alone implies --thickness open; closed differs where an instance touches a face
    only = open(main(args + ["--save-distance", "--out", os.path.join(tmp_path, "only.csv")])).read().splitlines()
    assert only[2] == plain[2] + ",inscribed_radius" and [float(ln.split(",")[17]) for ln in only[3:]] == radius
    closed = open(main(args + ["--thickness", "closed", "--out", os.path.join(tmp_path, "c.csv")])).read().splitlines()
    want_closed = np.sqrt(row_max(rows, expected(BLOBS, spacing, True)[2]))[keep].tolist()
    assert [float(ln.split(",")[17]) for ln in closed[3:]] == want_closed and want_closed != radius
    # the distance map: float32 sqrt(D2), background 0, stored [Z, X, Y] like the mask
    dist = read_float_tiff(os.path.join(tmp_path, "mito_distance.tif"))
    assert dist.dtype == np.float32 and dist.shape == (lab.shape[2], lab.shape[0], lab.shape[1])
    ref = np.sqrt(want).astype(np.float32)
    got = dist.transpose(1, 2, 0)
    print("distance map: voxels that differ from float32(sqrt(oracle)):", int((got != ref).sum()))
    assert np.array_equal(got, ref) and (got[lab <= 0] == 0).all() and (got[lab > 0] >= 1).all()
