"""``sk_local_thickness_paint`` (skoots_amd/csrc/local_thickness.hip) and everything on top of it --
``lib.morphology.local_thickness``, ``validate.lib.instance_local_thickness``, ``stats_per_instance(local_thickness=...)``,
``get_local_thickness`` and ``python -m skoots_amd.validate.compare --local-thickness / --save-thickness`` -- against the
numpy statements of tests/local_thickness_cases.py, which tests/test_local_thickness_cpu.py holds against the pairwise
definition.  The kernel computes a defined sequence of roundings and an order-independent maximum, so every comparison
of its output is equality of bits.

The shapes (tests/local_thickness_cases.py) have extents of 1 in every axis, boxes narrower and wider than the 64 lanes,
boxes clipped by every face, more centres than one grid of waves holds, instances that touch each other, a ball that is
open at 3-4-5, a voxel that the rounding form decides, and an instance that is alone in the volume."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests.edt_cases import BLOBS, oracle, row_max
from tests.local_thickness_cases import INF, MODES, NECK_345, SPACINGS, TUBE, cases, expected, paint, table_of, weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_mask(name):
    return torch.from_numpy(CASES[name].copy()).to(DEV)                # the cases are read-only


def read_float_tiff(path):
    """(Z, H, W) float32 of a stack ``write_float_stack`` wrote, by parsing the directories with struct and inflating
    the strips with zlib; asserts the tags a reader of 32-bit float pages goes by (as tests/test_edt_cpu.py reads them)"""
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:4] == b"II*\0"
    ifd = struct.unpack_from("<I", buf, 4)[0]
    pages = []
    while ifd:
        n = struct.unpack_from("<H", buf, ifd)[0]
        tags = {}
        for k in range(n):
            tag, typ, count, val = struct.unpack_from("<HHII", buf, ifd + 2 + 12 * k)
            assert count == 1 and typ in (3, 4)
            tags[tag] = val & 0xFFFF if typ == 3 else val
        assert tags[258] == 32 and tags[339] == 3 and tags[259] == 8 and tags[262] == 1 and tags[277] == 1
        assert tags[278] == tags[257]                                  # one strip per page
        raw = zlib.decompress(buf[tags[273]:tags[273] + tags[279]])
        pages.append(np.frombuffer(raw, "<f4").reshape(tags[257], tags[256]))
        ifd = struct.unpack_from("<I", buf, ifd + 2 + 12 * n)[0]
    return np.stack(pages)


def check(name, x, spacing, closed, **kw):
    from skoots_amd.lib.morphology import local_thickness
    ids, rows, d2, want = expected(name, spacing, closed)
    t2, got_d2, mx = local_thickness(x, spacing, closed, **kw)
    assert t2.dtype == torch.float64 and t2.is_cuda and tuple(t2.shape) == rows.shape
    assert np.array_equal(bits(got_d2.cpu().numpy()), bits(d2)) and tuple(mx.shape) == (len(ids),)
    got = t2.cpu().numpy()
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{name} {spacing} closed={closed} {kw}: {len(bad)} voxels differ, first {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert np.array_equal(bits(mx.cpu().numpy()), bits(row_max(rows, want)))     # per row max T2 = max D2
    return t2


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_every_spacing_both_modes(name):
    x = device_mask(name)
    for spacing in SPACINGS:
        for closed in MODES:
            check(name, x, spacing, closed)


@pytest.mark.parametrize("name", [NECK_345, "diagonal (8, 8, 8)"])
def test_every_centre_its_own_launch(name, monkeypatch):
    """budget = 1: no two centres share a launch, and the result is the same"""
    from skoots_amd import _ffi
    from skoots_amd.lib import morphology as M
    x = device_mask(name)
    calls = []
    real = _ffi.lib

    class Counting:
        def __getattr__(self, k):
            return getattr(real, k)

        @staticmethod
        def sk_local_thickness_paint(*a):
            calls.append(a[8])                                         # n_centres
            return real.sk_local_thickness_paint(*a)

    monkeypatch.setattr(_ffi, "lib", Counting())
    for spacing, closed in ((SPACINGS[0], False), (SPACINGS[3], True)):
        d2 = expected(name, spacing, closed)[2]
        n = int((np.isfinite(d2) & (d2 > min(weights(spacing)))).sum())
        del calls[:]
        check(name, x, spacing, closed, budget=1)
        assert n > 1 and calls == [1] * n
        del calls[:]
        check(name, x, spacing, closed)
        assert calls == [n]                                            # the default budget: one launch
    boxes = M.paint_centres(torch.from_numpy(d2.copy()).to(DEV), weights(spacing))[1]
    del calls[:]
    check(name, x, spacing, closed, budget=3 * int(boxes.max().item()))   # three centres or more a launch
    assert 1 < len(calls) < n and sum(calls) == n and min(calls[:-1]) >= 3


def test_two_runs_give_identical_bits_and_a_given_transform_is_used():
    from skoots_amd.lib.morphology import label_edt, local_thickness
    x = device_mask(BLOBS)
    a = local_thickness(x, SPACINGS[3], True)
    b = local_thickness(x, SPACINGS[3], True)
    assert all(torch.equal(u.view(torch.int64), v.view(torch.int64)) for u, v in zip(a, b))
    pair = label_edt(x, SPACINGS[3], True)
    before = pair[0].clone()
    c = local_thickness(x, SPACINGS[3], True, dist2=pair)
    assert torch.equal(c[0].view(torch.int64), a[0].view(torch.int64)) and c[1].data_ptr() == pair[0].data_ptr()
    assert torch.equal(pair[0].view(torch.int64), before.view(torch.int64))          # the transform is not modified
    assert c[0].data_ptr() != pair[0].data_ptr()


def test_table_and_columns():
    from skoots_amd.validate.compare import local_thickness_columns
    from skoots_amd.validate.lib import instance_local_thickness
    for name, spacing, closed in ((BLOBS, SPACINGS[1], False), (BLOBS, SPACINGS[3], True),
                                  ("huge int64 (4, 5, 36)", SPACINGS[2], True), ("one label (8, 9, 10)", SPACINGS[1], False),
                                  (TUBE, SPACINGS[0], False)):
        ids, rows, d2, want = expected(name, spacing, closed)
        x = device_mask(name)
        got_ids, table, t2, mx = instance_local_thickness(x, spacing, closed)
        assert got_ids.tolist() == ids.tolist() and isinstance(table, np.ndarray) and table.dtype == np.int64
        assert np.array_equal(table, table_of(rows, want)), name
        assert np.array_equal(bits(t2.cpu().numpy()), bits(want))
        assert np.array_equal(bits(mx.cpu().numpy()), bits(row_max(rows, d2)))
        assert table[:, 2].sum() == (rows > 0).sum()
        col = local_thickness_columns(table, len(ids))
        for r in range(len(ids)):
            v = np.sqrt(want[rows == r + 1])
            assert col["local_radius_min"][r].item() == v.min()
            if np.isfinite(v).all():
                # against numpy's own sums: a sum of n terms, each at most max(v), is off by at most n units of 2^-53
                # of n max(v) whatever its order, the mean by 1 / n of that, and there are two sums; the squared
                # deviations are at most max(v)^2 each and carry the mean's error twice over
                eps = 2.0 ** -53 * v.size * v.max()
                assert v.min() <= col["local_radius_mean"][r].item() <= v.max()
                assert abs(col["local_radius_mean"][r].item() - v.mean()) <= 2 * eps
                assert abs(col["local_radius_std"][r].item() ** 2 - v.var()) <= 8 * eps * v.max()
    assert col["local_radius_min"].tolist() == [1.0]                   # the tube: its constriction
    empty = instance_local_thickness(torch.zeros((3, 4, 5), dtype=torch.int32, device=DEV), (1.0, 1.0, 1.0))
    assert empty[0].numel() == 0 and empty[1].shape == (0, 3) and not bool(empty[2].any()) and empty[3].numel() == 0


def test_stats_per_instance_and_get_local_thickness():
    from skoots_amd.validate.compare import local_thickness_columns, stats_per_instance
    from skoots_amd.validate.stats import get_local_thickness
    lab = CASES[BLOBS]
    x = device_mask(BLOBS)
    spacing = SPACINGS[1]
    plain = stats_per_instance(x, spacing)
    assert set(plain) == {"id", "voxels", "volume", "bbox", "touches_border", "centroid", "face_area", "faces",
                          "axis_lengths", "sums"}
    assert set(stats_per_instance(x, spacing, local_thickness=None)) == set(plain)
    for mode in ("open", "closed"):
        ids, rows, d2, want = expected(BLOBS, spacing, mode == "closed")
        st = stats_per_instance(x[None], spacing, local_thickness=mode)
        assert set(st) - set(plain) == {"thick2", "max_dist2", "local_radius_mean", "local_radius_std",
                                        "local_radius_min"}
        assert all(torch.equal(st[k], plain[k]) for k in plain)
        assert np.array_equal(bits(st["thick2"].cpu().numpy()), bits(want)) and st["local_radius_min"].is_cuda
        assert np.array_equal(bits(st["max_dist2"].cpu().numpy()), bits(row_max(rows, d2)))
        col = local_thickness_columns(table_of(rows, want), len(ids))
        assert all(np.array_equal(bits(st[k].cpu().numpy()), bits(v.numpy())) for k, v in col.items())
        both = stats_per_instance(x, spacing, thickness=mode, local_thickness=mode)
        width = stats_per_instance(x, spacing, thickness=mode)
        assert set(both) - set(width) == {"thick2", "local_radius_mean", "local_radius_std", "local_radius_min"}
        assert all(torch.equal(both[k], width[k]) for k in width)
        assert all(torch.equal(both[k], st[k]) for k in set(st) - set(plain))
        other = "closed" if mode == "open" else "open"
        mixed = stats_per_instance(x, spacing, thickness=other, local_thickness=mode)
        assert torch.equal(mixed["thick2"], st["thick2"])
        assert torch.equal(mixed["max_dist2"], stats_per_instance(x, spacing, thickness=other)["max_dist2"])
        assert bool((st["local_radius_min"] <= st["local_radius_mean"]).all())
        assert bool((st["local_radius_mean"].cpu() <= torch.from_numpy(np.sqrt(row_max(rows, d2)))).all())
    with pytest.raises(ValueError):
        stats_per_instance(x, spacing, local_thickness="yes")
    u = int(np.unique(lab[lab > 0])[3])
    for closed in MODES:
        one = get_local_thickness(x == u, spacing, closed)
        assert one.dtype == torch.float64 and one.is_cuda and tuple(one.shape) == lab.shape
        m = (lab == u).astype(np.int64)
        ref = paint(m, oracle(m, weights(spacing), closed), weights(spacing))
        # the square root is the device's own: the same function of the same bits
        assert torch.equal(one.view(torch.int64), torch.sqrt(torch.from_numpy(ref.copy()).to(DEV)).view(torch.int64))
        assert np.array_equal(one.cpu().numpy().astype(np.float32), np.sqrt(ref).astype(np.float32))
    assert not bool(get_local_thickness(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]).any())
    assert bool((get_local_thickness(torch.ones((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]) == INF).all())


def test_command_end_to_end(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import local_thickness_columns, main
    lab = CASES[BLOBS]
    spacing = SPACINGS[1]
    ids, rows, d2, want = expected(BLOBS, spacing, False)
    x = device_mask(BLOBS)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read().splitlines()
    assert not os.path.exists(os.path.join(tmp_path, "mito_thickness.tif")) and "local_radius" not in plain[2]
    width = open(main(args + ["--thickness", "open", "--out", os.path.join(tmp_path, "w.csv")])).read().splitlines()
    out = main(args + ["--thickness", "open", "--local-thickness", "open", "--save-thickness"])
    assert out == os.path.join(tmp_path, "mito_instance_stats.csv")
    lines = open(out).read().splitlines()
    assert lines[:2] == width[:2] and lines[2] == width[2] + ",local_radius_mean,local_radius_std,local_radius_min"
    assert [ln.split(",")[:18] for ln in lines[3:]] == [ln.split(",") for ln in width[3:]]
    keep = np.array([(lab == u).sum() >= 2 for u in ids])
    assert keep.any() and [int(ln.split(",")[0]) for ln in lines[3:]] == ids[keep].tolist()
    col = local_thickness_columns(table_of(rows, want), len(ids))
    ref = np.stack([col[k].numpy() for k in ("local_radius_mean", "local_radius_std", "local_radius_min")], 1)[keep]
    assert [[float(v) for v in ln.split(",")[18:]] for ln in lines[3:]] == ref.tolist()
    # --save-thickness alone implies --local-thickness open; closed differs where an instance touches a face
    only = open(main(args + ["--save-thickness", "--out", os.path.join(tmp_path, "only.csv")])).read().splitlines()
    assert only[2] == plain[2] + ",local_radius_mean,local_radius_std,local_radius_min"
    assert [[float(v) for v in ln.split(",")[17:]] for ln in only[3:]] == ref.tolist()
    closed = open(main(args + ["--local-thickness", "closed", "--out", os.path.join(tmp_path, "c.csv")])).read().splitlines()
    want_c = expected(BLOBS, spacing, True)[3]
    col_c = local_thickness_columns(table_of(rows, want_c), len(ids))
    ref_c = np.stack([col_c[k].numpy() for k in ("local_radius_mean", "local_radius_std", "local_radius_min")], 1)[keep]
    assert [[float(v) for v in ln.split(",")[17:]] for ln in closed[3:]] == ref_c.tolist() and ref_c.tolist() != ref.tolist()
    # the map: float32 sqrt(T2), background 0, stored [Z, X, Y] like the mask
    thick = read_float_tiff(os.path.join(tmp_path, "mito_thickness.tif"))
    assert thick.dtype == np.float32 and thick.shape == (lab.shape[2], lab.shape[0], lab.shape[1])
    got = thick.transpose(1, 2, 0)
    assert np.array_equal(got, np.sqrt(want).astype(np.float32))
    assert (got[lab <= 0] == 0).all() and (got[lab > 0] >= 1).all()
    assert not os.path.exists(os.path.join(tmp_path, "mito_distance.tif"))


def test_c_abi_guards_write_nothing():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 22
    X, Y, Z = 4, 5, 6
    d2 = torch.zeros((X, Y, Z), dtype=torch.float64, device=DEV)
    d2[1:3, 1:4, 1:5] = 1.0
    d2[2, 2, 2] = 4.0
    d2 = torch.cat((d2.reshape(-1), d2.new_full((1,), -7.0)))
    t2 = torch.full((X * Y * Z + 1,), -7.0, dtype=torch.float64, device=DEV)
    centres = torch.tensor([(2 * Y + 2) * Z + 2, 0, (1 * Y + 1) * Z + 1, -7], dtype=torch.int64, device=DEV)
    base = dict(dist2=_ffi.ptr(d2), X=X, Y=Y, Z=Z, wx=1.0, wy=1.0, wz=1.0, centres=_ffi.ptr(centres), n=3,
                thick2=_ffi.ptr(t2))

    def call(**kw):
        a = dict(base, **kw)
        rc = _ffi.lib.sk_local_thickness_paint(*(a[k] for k in base), _ffi.stream_ptr(d2.device))
        torch.cuda.synchronize()
        return rc

    for null in ("dist2", "centres", "thick2"):
        assert call(**{null: None}) == -1 and "sk_local_thickness_paint: NULL" in _ffi.last_error(), null
    assert call(thick2=_ffi.ptr(d2)) == -1 and "sk_local_thickness_paint: thick2 and dist2 are one buffer" in _ffi.last_error()
    for k in ("dist2", "centres", "thick2"):
        assert call(**{k: base[k].value + 4}) == -1 and "sk_local_thickness_paint" in _ffi.last_error() \
            and "aligned" in _ffi.last_error(), k
    assert call(n=-1) == -1 and "sk_local_thickness_paint: n_centres" in _ffi.last_error()
    for k in ("X", "Y", "Z"):
        assert call(**{k: -1}) == -1 and "negative" in _ffi.last_error(), k
    assert call(X=2 ** 26 + 1, Y=1, Z=1) == -1 and "sk_local_thickness_paint" in _ffi.last_error() \
        and "2^26" in _ffi.last_error()
    assert call(X=2 ** 26, Y=2 ** 26, Z=2 ** 26) == -1 and "2^62" in _ffi.last_error()
    for k in ("wx", "wy", "wz"):
        for v in (0.0, -1.0, INF, float("nan")):
            assert call(**{k: v}) == -1 and "weights" in _ffi.last_error(), (k, v)
    # no centre and an empty volume are not errors, and write nothing either
    assert call(n=0) == 0 and call(X=0) == 0 and call(Y=0) == 0 and call(Z=0) == 0
    assert call(n=0, dist2=None, centres=None, thick2=None) == 0
    assert bool((t2 == -7.0).all())
    # and the same buffers take a real run: nothing is written behind their ends, the background centre paints nothing
    t2[:-1] = d2[:-1]
    assert call() == 0
    assert t2[-1].item() == -7.0
    want = d2[:-1].clone().view(X, Y, Z)
    want[1:4, 1:4, 1:4] = 4.0        # the open ball of squared radius 4 holds the offsets of squared length 1, 2 and 3
    assert torch.equal(t2[:-1].view(X, Y, Z), want)


def test_host_guards():
    from skoots_amd.lib.morphology import local_thickness
    x = torch.ones((3, 3, 3), dtype=torch.int32, device=DEV)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, INF, 1.0), (1e200, 1.0, 1.0)):
        with pytest.raises(ValueError):
            local_thickness(x, bad)
    with pytest.raises(ValueError):
        local_thickness(x, budget=0)
    with pytest.raises(ValueError):
        local_thickness(torch.zeros((3, 3, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        local_thickness(x, dist2=(torch.zeros((3, 3, 3), device=DEV), None))       # float32
    t2, d2, mx = local_thickness(torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV))
    assert tuple(t2.shape) == (0, 4, 4) and mx.numel() == 0
    assert local_thickness(x)[2].tolist() == [INF] and bool((local_thickness(x)[0] == INF).all())
    assert local_thickness(x, closed=True)[0].max().item() == 4.0
