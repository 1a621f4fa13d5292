"""``sk_nearest_label`` (skoots_amd/csrc/nearest_label.hip) and what is built on it -- ``lib.morphology.nearest_label``,
``utils.grow.grow`` and ``python -m skoots_amd.utils.grow`` -- against the numpy oracle of tests/nearest_label_cases.py,
which tests/test_nearest_label_cpu.py holds against the pairwise brute force and against scipy.  The kernel computes a
defined sequence of roundings and a defined choice among ties, so every comparison is equality of bits or of integers.

The shapes (tests/nearest_label_cases.py) have extents of 1 in every axis, lines that are no multiple of the 64 lanes,
more than one workgroup, ties on the low side, between the sides and at the reach, and walks that cross a wave's line."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import edt_cases
from tests.nearest_label_cases import (BALL, BLOBS, INF, SPACINGS, STRETCH, WHERE_CASE, cases, expected, grow_rule,
                                       ids_of, limits, report_counts, shrink_rule, weights, where_cases)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = cases()
SMALL_IDS = "cross (9, 11, 37)"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def distance_of(limit2):
    """a max_distance whose square is limit2 in float64, or None; None too where no float squares to it"""
    if limit2 == INF:
        return None
    d = float(np.sqrt(limit2))
    for c in (d, float(np.nextafter(d, 0.0)), float(np.nextafter(d, INF))):
        if c * c == limit2:
            return c
    return NotImplemented


def check_call(name, x, spacing, limit2, where=None):
    """the C entry point at any limit2, through the buffers ``nearest_label`` would hand it"""
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    ids, rows, want_d2, want_near = expected(name, spacing, limit2, where)
    vol, r = id_rows(x)
    X, Y, Z = rows.shape
    d2 = torch.full((X, Y, Z), -1.0, dtype=torch.float64, device=DEV)
    near = torch.full((X, Y, Z), -1, dtype=torch.int32, device=DEV)
    if r is None:
        assert len(ids) == 0
        lab, lut, max_id, N = torch.zeros((X, Y, Z), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32,
                                                                                                 device=DEV), 0, 0
    else:
        lab, got_ids, lut, max_id = r
        N = int(got_ids.numel())
        assert got_ids.tolist() == ids.tolist()
    s2, sr = torch.empty_like(d2), torch.empty_like(near)
    wh = None if where is None else torch.from_numpy(where).to(DEV)
    wx, wy, wz = weights(spacing)
    _ffi.check(_ffi.lib.sk_nearest_label(_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), max_id, N, wx, wy, wz, float(limit2),
                                         _ffi.ptr(wh), _ffi.ptr(d2), _ffi.ptr(near), _ffi.ptr(s2), _ffi.ptr(sr),
                                         _ffi.stream_ptr(lab.device)))
    got = d2.cpu().numpy()
    bad = np.argwhere(bits(got) != bits(want_d2))
    assert bad.size == 0, f"{name} {spacing} limit2={limit2}: {len(bad)} voxels differ, first {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} != {want_d2[tuple(bad[0])]!r}"
    bad = np.argwhere(near.cpu().numpy() != want_near)
    assert bad.size == 0, f"{name} {spacing} limit2={limit2}: {len(bad)} rows differ, first {bad[0]}"


def check(name, x, spacing, max_distance=None, where=None):
    """``nearest_label``: ids, not rows"""
    from skoots_amd.lib.morphology import nearest_label
    limit2 = INF if max_distance is None else float(max_distance) * float(max_distance)
    wh = None if where is None else np.asarray(where.cpu().numpy() if isinstance(where, torch.Tensor) else where)
    ids, rows, want_d2, want_near = expected(name, spacing, limit2, None if wh is None else wh.reshape(rows_shape(name)))
    near, d2 = nearest_label(x, spacing, max_distance, where)
    assert near.dtype == torch.int64 and d2.dtype == torch.float64 and near.is_cuda and d2.is_cuda
    assert tuple(near.shape) == rows.shape and tuple(d2.shape) == rows.shape
    assert np.array_equal(bits(d2.cpu().numpy()), bits(want_d2)), (name, spacing, max_distance)
    assert np.array_equal(near.cpu().numpy(), ids_of(ids, want_near)), (name, spacing, max_distance)
    return near, d2


def rows_shape(name):
    return CASES[name].shape


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_every_spacing_every_limit(name):
    lab = CASES[name]
    x = torch.from_numpy(lab).to(DEV)
    for spacing in SPACINGS:
        for limit2 in limits(name, spacing):
            check_call(name, x, spacing, limit2)
            d = distance_of(limit2)
            if d is not NotImplemented:
                check(name, x, spacing, d)
    assert distance_of(limits(name, SPACINGS[1])[1]) == 6.0 and distance_of(0.0) == 0.0 and distance_of(INF) is None


def test_where_cases():
    lab = CASES[WHERE_CASE]
    x = torch.from_numpy(lab).to(DEV)
    for spacing in SPACINGS:
        for limit2 in limits(WHERE_CASE, spacing):
            for wname, where in where_cases(lab).items():
                check_call(WHERE_CASE, x, spacing, limit2, where)
    for wname, where in where_cases(lab).items():
        for wh in (torch.from_numpy(where).to(DEV), torch.from_numpy(where != 0).to(DEV),
                   torch.from_numpy(where.astype(np.int64) * -3).to(DEV)[None]):
            check(WHERE_CASE, x, SPACINGS[1], 6.0, wh)
            check(WHERE_CASE, x, SPACINGS[3], None, wh)
    from skoots_amd.lib.morphology import nearest_label
    for bad in (torch.ones((8, 8, 7), dtype=torch.uint8, device=DEV), torch.ones((8, 8, 8), dtype=torch.uint8),
                torch.ones((8, 8, 8), device=DEV), np.ones((8, 8, 8), np.uint8)):
        with pytest.raises(ValueError):
            nearest_label(x, where=bad)


def test_passes_one_by_one_equal_the_fused_call():
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    for name, spacing, limit2, where in ((BLOBS, SPACINGS[3], INF, None), (BLOBS, SPACINGS[1], 36.0, None),
                                         (STRETCH, SPACINGS[1], limits(STRETCH, SPACINGS[1])[-2], None),
                                         (WHERE_CASE, SPACINGS[2], 100.0, where_cases(CASES[WHERE_CASE])["checkerboard"])):
        x = torch.from_numpy(CASES[name]).to(DEV)
        _, (a, ids, lut, max_id) = id_rows(x)
        X, Y, Z = a.shape
        N = int(ids.numel())
        wx, wy, wz = weights(spacing)
        want = expected(name, spacing, limit2, where)
        wh = None if where is None else torch.from_numpy(where).to(DEV)
        d = [torch.full((X, Y, Z), -1.0, dtype=torch.float64, device=DEV) for _ in range(2)]
        r = [torch.full((X, Y, Z), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
        st = _ffi.stream_ptr(a.device)
        args = (_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, N)
        P = _ffi.lib.sk_nearest_label_pass
        _ffi.check(P(*args, 2, wz, limit2, None, None, None, _ffi.ptr(d[0]), _ffi.ptr(r[0]), st))
        _ffi.check(P(*args, 1, wy, limit2, _ffi.ptr(d[0]), _ffi.ptr(r[0]), None, _ffi.ptr(d[1]), _ffi.ptr(r[1]), st))
        _ffi.check(P(*args, 0, wx, limit2, _ffi.ptr(d[1]), _ffi.ptr(r[1]), _ffi.ptr(wh), _ffi.ptr(d[0]), _ffi.ptr(r[0]),
                     st))
        assert np.array_equal(bits(d[0].cpu().numpy()), bits(want[2])) and np.array_equal(r[0].cpu().numpy(), want[3])
        d[1].fill_(-1.0)
        r[1].fill_(-1)
        one, row = torch.empty_like(d[0]), torch.empty_like(r[0])
        _ffi.check(_ffi.lib.sk_nearest_label(*args, wx, wy, wz, limit2, _ffi.ptr(wh), _ffi.ptr(one), _ffi.ptr(row),
                                             _ffi.ptr(d[1]), _ffi.ptr(r[1]), st))
        assert torch.equal(one.view(torch.int64), d[0].view(torch.int64)) and torch.equal(row, r[0])


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64])
def test_integer_dtypes_and_a_view(dtype):
    lab = CASES[SMALL_IDS]
    x = torch.from_numpy(lab).to(dtype).to(DEV)
    check(SMALL_IDS, x, SPACINGS[3])
    check(SMALL_IDS, x[None], SPACINGS[1], 6.0)                       # (1, X, Y, Z)
    view = torch.from_numpy(np.ascontiguousarray(lab.transpose(2, 0, 1))).to(dtype).to(DEV).permute(1, 2, 0)
    assert not view.is_contiguous() and tuple(view.shape) == lab.shape
    check(SMALL_IDS, view, SPACINGS[3], 2.5)


def test_huge_ids_take_the_relabel_route(monkeypatch):
    from skoots_amd.validate import lib as VL
    monkeypatch.setattr(VL, "_lut", lambda m: pytest.fail("the max id + 1 table was built for a huge id"))
    for name in ("huge int32 (4, 5, 36)", "huge int64 (4, 5, 36)"):
        x = torch.from_numpy(CASES[name]).to(DEV)
        near, _ = check(name, x, SPACINGS[3])
        check(name, x, SPACINGS[1], 6.0)
        assert sorted(set(near.cpu().numpy().reshape(-1).tolist())) == [70000, 2 ** 30,
                                                                        2 ** 40 if "int64" in name else 2 ** 31 - 1]


def test_two_runs_give_identical_bits():
    from skoots_amd.lib.morphology import nearest_label
    from skoots_amd.utils.grow import grow
    x = torch.from_numpy(CASES[BLOBS]).to(DEV)
    a = nearest_label(x, SPACINGS[3], 1.9)
    b = nearest_label(x, SPACINGS[3], 1.9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    for d in (2.0, -2.0):
        a, b = grow(x, d, SPACINGS[1]), grow(x, d, SPACINGS[1])
        assert torch.equal(a[0], b[0]) and a[1] == b[1]


def test_c_abi_guards_write_nothing():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 21
    X, Y, Z, N, max_id = 4, 5, 6, 2, 9
    n = X * Y * Z
    lab = torch.zeros((X, Y, Z), dtype=torch.int32, device=DEV)
    lab[1:3, 1:4, 1:5] = 9
    lab[0, 0, 0] = 3
    lut = torch.zeros(max_id + 1, dtype=torch.int32, device=DEV)
    lut[3], lut[9] = 1, 2
    where = torch.ones(n, dtype=torch.uint8, device=DEV)
    d2 = torch.full((n + 1,), -7.0, dtype=torch.float64, device=DEV)
    s2 = torch.full((n + 1,), -7.0, dtype=torch.float64, device=DEV)
    nr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    sr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    base = dict(labels=_ffi.ptr(lab), X=X, Y=Y, Z=Z, lut=_ffi.ptr(lut), max_id=max_id, N=N, wx=1.0, wy=0.25, wz=9.0,
                limit2=INF, where=_ffi.ptr(where), dist2=_ffi.ptr(d2), nearest=_ffi.ptr(nr), scratch_d2=_ffi.ptr(s2),
                scratch_row=_ffi.ptr(sr))
    st = _ffi.stream_ptr(lab.device)

    def call(**kw):
        a = dict(base, **kw)
        rc = _ffi.lib.sk_nearest_label(*(a[k] for k in base), st)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((d2 == -7.0).all()) and bool((s2 == -7.0).all()) and bool((nr == -7).all()) and bool((sr == -7).all())

    for null in ("labels", "lut", "dist2", "nearest", "scratch_d2", "scratch_row"):
        assert call(**{null: None}) == -1 and "sk_nearest_label: NULL" in _ffi.last_error(), null
    assert call(dist2=d2.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert call(scratch_d2=s2.data_ptr() + 4) == -1 and call(nearest=nr.data_ptr() + 2) == -1
    assert call(scratch_row=sr.data_ptr() + 2) == -1 and call(labels=lab.data_ptr() + 2) == -1
    assert call(lut=lut.data_ptr() + 2) == -1 and "aligned" in _ffi.last_error()
    for k in ("X", "Y", "Z", "N", "max_id"):
        assert call(**{k: -1}) == -1 and "negative" in _ffi.last_error(), k
    assert call(X=2 ** 26 + 1, Y=1, Z=1) == -1 and "2^26" in _ffi.last_error()
    assert call(X=2 ** 26, Y=2 ** 26, Z=2 ** 26) == -1 and "2^62" in _ffi.last_error()
    for k in ("wx", "wy", "wz"):
        for v in (0.0, -1.0, INF, float("nan")):
            assert call(**{k: v}) == -1 and "weights" in _ffi.last_error(), (k, v)
    for v in (float("nan"), -1.0, -INF, -1e-300):
        assert call(limit2=v) == -1 and "limit2" in _ffi.last_error(), v
    for a, b in (("scratch_d2", d2), ("scratch_row", nr), ("nearest", d2), ("scratch_row", s2), ("scratch_d2", nr),
                 ("dist2", sr)):
        assert call(**{a: _ffi.ptr(b)}) == -1 and "distinct" in _ffi.last_error(), a
    P = _ffi.lib.sk_nearest_label_pass
    head = (_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), max_id, N)
    src, dst = (_ffi.ptr(s2), _ffi.ptr(sr)), (_ffi.ptr(d2), _ffi.ptr(nr))
    for axis in (3, -1):
        assert P(*head, axis, 1.0, INF, *src, None, *dst, st) == -1 and "axis" in _ffi.last_error()
    assert P(*head, 1, 1.0, INF, None, None, None, *dst, st) == -1 and "NULL" in _ffi.last_error()
    assert P(*head, 0, 1.0, INF, src[0], None, None, *dst, st) == -1
    assert P(*head, 2, 1.0, INF, None, None, None, None, dst[1], st) == -1
    assert P(*head, 0, 1.0, INF, dst[0], src[1], None, *dst, st) == -1 and "distinct" in _ffi.last_error()
    assert P(*head, 1, 1.0, INF, src[0], dst[1], None, *dst, st) == -1
    assert P(*head, 1, 0.0, INF, *src, None, *dst, st) == -1 and P(*head, 1, 1.0, float("nan"), *src, None, *dst, st) == -1
    torch.cuda.synchronize()
    assert untouched()
    # an empty volume is not an error and writes nothing
    assert call(X=0) == 0 and call(Y=0) == 0 and call(Z=0) == 0
    assert call(X=0, labels=None, dist2=None, nearest=None, scratch_d2=None, scratch_row=None) == 0
    assert untouched()
    # N == 0 fills the outputs, not the scratch, and nothing behind their ends
    assert call(N=0) == 0
    assert bool((d2[:-1] == INF).all()) and bool((nr[:-1] == 0).all()) and bool(d2[-1] == -7.0) and bool(nr[-1] == -7)
    assert bool((s2 == -7.0).all()) and bool((sr == -7).all())
    # and the same buffers take a real run, where = NULL
    assert call(where=None, limit2=9.0) == 0
    assert bool(d2[-1] == -7.0) and bool(s2[-1] == -7.0) and bool(nr[-1] == -7) and bool(sr[-1] == -7)
    got, row = d2[:-1].view(X, Y, Z), nr[:-1].view(X, Y, Z)
    assert got[0, 0, 0].item() == 0.0 and row[0, 0, 0].item() == 1 and got[1, 1, 1].item() == 0.0
    assert got[0, 1, 0].item() == 0.25 and row[0, 1, 0].item() == 1 and got[0, 0, 1].item() == 1.25 and row[0, 0, 1].item() == 2
    assert got[3, 2, 2].item() == 1.0 and row[3, 2, 2].item() == 2 and got[3, 4, 5].item() == INF and row[3, 4, 5].item() == 0


def test_host_guards_and_empty_masks():
    from skoots_amd.lib.morphology import nearest_label
    for x in (torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV), torch.full((3, 3, 3), -5, dtype=torch.int32,
                                                                                   device=DEV),
              torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV)):
        near, d2 = nearest_label(x, (1.0, 2.0, 3.0), 4.0)
        assert tuple(near.shape) == tuple(x.shape) and near.dtype == torch.int64 and not bool(near.any())
        assert tuple(d2.shape) == tuple(x.shape) and d2.dtype == torch.float64 and bool((d2 == INF).all())
    x = torch.ones((3, 3, 3), dtype=torch.int32, device=DEV)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, INF, 1.0), (1e200, 1.0, 1.0), (1e-200, 1.0, 1.0)):
        with pytest.raises(ValueError):
            nearest_label(x, bad)
    for bad in (float("nan"), -1.0, INF, "1"):
        with pytest.raises(ValueError):
            nearest_label(x, max_distance=bad)
    with pytest.raises(TypeError):
        nearest_label(torch.zeros((3, 3, 3), device=DEV))
    with pytest.raises(ValueError):
        nearest_label(torch.zeros((3, 3, 3), dtype=torch.int32))
    near, d2 = nearest_label(x * 5)
    assert bool((near == 5).all()) and not bool(d2.any())


# ---------------------------------------------------------------------------------------------------------- utils.grow

GROW_DISTANCES = {edt_cases.BLOBS: (1.0, 3.0, 7.5)}


@pytest.mark.parametrize("name", list(CASES))
def test_grow_equals_the_numpy_rule(name):
    from skoots_amd.utils.grow import grow
    lab = CASES[name]
    x = torch.from_numpy(lab).to(DEV)
    spacing = SPACINGS[1]
    ids, rows, d2, near = expected(name, spacing)
    clean = np.where(lab > 0, lab, 0)
    if (lab < 0).any():
        with pytest.raises(ValueError, match="negative"):
            grow(x, 1.0, spacing)
        x, lab = torch.from_numpy(clean).to(DEV), clean
    for d in GROW_DISTANCES.get(name, (3.0,)):
        out, rep = grow(x, d, spacing)
        want = grow_rule(lab, d2, ids_of(ids, near), d)
        got = out.cpu().numpy()
        assert out.dtype == x.dtype and out.is_cuda and np.array_equal(got, want), (name, d)
        assert (got[lab != 0] == lab[lab != 0]).all()                      # no voxel with an id changes
        assert set(np.unique(got).tolist()) <= set(np.unique(lab).tolist()) | {0}    # no id appears
        assert dataclasses.asdict(rep) == report_counts(lab, want)
        assert rep.instances_in == rep.instances_out == len(ids) and rep.voxels_removed == 0 and rep.ids_removed == 0
    out, rep = grow(x, 0, spacing)
    assert torch.equal(out, x) and out.data_ptr() != x.data_ptr() and rep.voxels_added == 0 and rep.instances_in == len(ids)


def test_grow_within_and_dtypes():
    from skoots_amd.utils.grow import grow
    for name, dtypes in ((BLOBS, (torch.int32, torch.int64)), (SMALL_IDS, (torch.uint8, torch.int16, torch.int32))):
        lab = CASES[name]
        spacing = SPACINGS[1]
        ids, rows, d2, near = expected(name, spacing)
        within = (np.indices(lab.shape).sum(0) % 3 != 0)
        want = grow_rule(lab, d2, ids_of(ids, near), 4.0, within)
        assert (want[~within] == lab[~within]).all() and (want != lab).any()
        for dtype in dtypes:
            x = torch.from_numpy(lab).to(dtype).to(DEV)
            for wi in (torch.from_numpy(within).to(DEV), torch.from_numpy(within.astype(np.uint8) * 7).to(DEV)[None]):
                out, rep = grow(x[None], 4.0, spacing, within=wi)
                assert out.dtype == dtype and tuple(out.shape) == lab.shape and np.array_equal(out.cpu().numpy(), want)
                assert dataclasses.asdict(rep) == report_counts(lab, want)
    with pytest.raises(ValueError):
        grow(x, 4.0, spacing, within=torch.ones((2, 2, 2), dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        grow(x, 4.0, spacing, within=torch.from_numpy(within))
    with pytest.raises(ValueError):
        grow(x, -4.0, spacing, within=torch.from_numpy(within).to(DEV))


@pytest.mark.parametrize("name", [BLOBS, BALL, "shared plane (6, 7, 8)", "one label (8, 9, 10)", "huge int64 (4, 5, 36)"])
def test_shrink_against_the_distance_transforms_oracle(name):
    from skoots_amd.utils.grow import grow
    lab = np.where(CASES[name] > 0, CASES[name], 0)
    x = torch.from_numpy(lab).to(DEV)
    for spacing, d in ((SPACINGS[1], 3.0), (SPACINGS[3], 0.8)):
        for closed in (False, True):
            edt = edt_cases.expected(name, spacing, closed)[2]
            out, rep = grow(x, -d, spacing, closed=closed)
            want = shrink_rule(lab, edt, -d)
            assert out.dtype == x.dtype and np.array_equal(out.cpu().numpy(), want), (name, spacing, closed)
            assert dataclasses.asdict(rep) == report_counts(lab, want)
            assert rep.voxels_added == 0 and rep.ids_grown == 0


def test_growing_a_shrunk_ball_never_exceeds_it():
    from skoots_amd.utils.grow import grow
    lab = CASES[BALL]
    x = torch.from_numpy(lab).to(DEV)
    for spacing in (SPACINGS[0], SPACINGS[1], SPACINGS[3]):
        for d in (1.0, 2.5, 4.0):
            small, r1 = grow(x, -d, spacing)
            back, r2 = grow(small, d, spacing)
            assert bool((small > 0).any()) and bool(((back > 0) <= (x > 0)).all()), (spacing, d)
            assert bool(((small > 0) <= (back > 0)).all()) and r2.voxels_added <= r1.voxels_removed


def _orphans():
    """a mask with unassigned foreground, as eval() leaves it, and the gated vectors that tell the foreground"""
    lab = CASES[BLOBS].copy()
    fg = lab > 0
    rng = np.random.default_rng(11)
    lab[fg & (rng.random(lab.shape) < 0.2)] = 0            # foreground voxels whose embedding found no skeleton
    vec = (rng.standard_normal((3,) + lab.shape) * fg).astype(np.float16)
    vec[0][fg & (vec == 0).all(0)] = np.float16(0.5)
    return lab, fg, vec


def test_command_end_to_end(tmp_path, capsys):
    from skoots_amd.lib import tiff, zarr_store
    from skoots_amd.utils import grow as G
    lab, fg, vec = _orphans()
    spacing = SPACINGS[1]
    x = torch.from_numpy(lab).to(DEV)
    path = str(tmp_path / "I_instance_mask.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())                     # stored [Z, X, Y]
    before = open(path, "rb").read()
    store = str(tmp_path / "I_skoots_vectors.zarr")
    zarr_store.save(store, vec)
    within_tif = str(tmp_path / "fg.tif")
    tiff.write_label_stack(within_tif, torch.from_numpy(fg.astype(np.int32) * 3).to(DEV).permute(2, 0, 1).contiguous())
    args = [path, "--distance", "3", "--spacing", *(str(v) for v in spacing)]
    want, report = G.grow(x, 3.0, spacing, within=torch.from_numpy(fg).to(DEV))
    assert report.voxels_added > 0 and bool((want[torch.from_numpy(~fg).to(DEV)] == 0).all())
    for within in (store, within_tif):
        for on_device in (False, True):
            G.READ_ON_DEVICE = on_device
            try:
                capsys.readouterr()
                out_path = G.main(args + ["--within", within])
            finally:
                G.READ_ON_DEVICE = False
            assert out_path == str(tmp_path / "I_instance_mask_grown.tif") and open(path, "rb").read() == before
            back = tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32)
            assert torch.equal(back, want)
            lines = capsys.readouterr().out.splitlines()
            assert lines[:6] == [f"{k}: {v}" for k, v in dataclasses.asdict(report).items()]
            assert lines[6] == f"File Written: {out_path}"
    # without --within the background grows too; a negative distance writes *_shrunk.tif; -o overwrites
    out_path = G.main(args)
    assert torch.equal(tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32), G.grow(x, 3.0, spacing)[0])
    out_path = G.main([path, "--distance", "-2", "--spacing", *(str(v) for v in spacing), "--closed"])
    assert out_path == str(tmp_path / "I_instance_mask_shrunk.tif") and open(path, "rb").read() == before
    shrunk = G.grow(x, -2.0, spacing, closed=True)[0]
    assert torch.equal(tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32), shrunk)
    with pytest.raises(SystemExit):
        G.main([path, "--distance", "-2", "--within", store])
    with pytest.raises(FileNotFoundError):
        G.main(args + ["--within", str(tmp_path / "missing.zarr")])
    assert open(path, "rb").read() == before
    assert G.main(args + ["--within", store, "-o"]) == path
    assert torch.equal(tiff.read_stack(path, DEV).permute(1, 2, 0).to(torch.int32), want)
