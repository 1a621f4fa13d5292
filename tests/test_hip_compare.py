"""``sk_instance_surface_count`` / ``_emit`` / ``sk_surface_distances`` (skoots_amd/csrc/surface_distance.hip) and
everything on top of them -- ``instance_surfaces``, ``surface_distances``, ``compare``, ``--ground-truth`` -- against the
numpy oracle of tests/surface_distance_cases.py (which tests/test_surface_distance_cpu.py holds against scipy).  Every
kernel output is defined bit for bit, so every comparison is exact equality.

The distance kernel gives a workgroup 256 consecutive outputs and stages a pair's target segment through LDS in tiles of
``sk_surface_distance_tile()`` voxels; the synthetic key lists sit on both sides of both sizes, share target segments
between pairs, and hold a segment whose far tiles are prunable and one that is not sorted."""
import os

import numpy as np
import pytest
import torch

from tests import surface_distance_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # a copy: the oracle's arrays are read-only


def offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


@pytest.fixture(scope="module")
def volumes():
    return S.cases()


def test_surfaces_equal_the_oracle(volumes):
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows, instance_surfaces
    for name, pair in volumes.items():
        ids_g, _, counts_g, keys_g, ids_p, _, counts_p, keys_p = S.surfaces_of(name)
        for lab, ids, counts, keys in ((pair[0], ids_g, counts_g, keys_g), (pair[1], ids_p, counts_p, keys_p)):
            got = instance_surfaces(dev(lab))
            assert all(t.is_cuda and t.dtype == torch.int64 for t in got)
            assert got[0].tolist() == ids.tolist(), name
            assert got[1].tolist() == offsets(counts).tolist(), name
            assert np.array_equal(got[2].cpu().numpy(), keys), name
    # the raw passes: a capacity one short leaves the slot past the end untouched and still reports the true total
    x, rows = id_rows(dev(volumes[S.BALL][0][None]))
    a, ids, lut, max_id = rows
    X, Y, Z = x.shape
    want = S.surfaces_of(S.BALL)[3]
    K = int(want.size)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(x.device)
    assert _ffi.lib.sk_instance_surface_count(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, 1, _ffi.ptr(counts), st) == 0
    assert counts.tolist() == [K, -7]
    for cap in (K, K - 1, 0):
        keys = torch.full((K + 1,), -7, dtype=torch.int64, device=DEV)
        produced = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        assert _ffi.lib.sk_instance_surface_emit(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, 1, cap,
                                                 _ffi.ptr(keys) if cap else None, _ffi.ptr(produced), st) == 0
        assert produced.tolist() == [K, -7]
        assert bool((keys[cap:] == -7).all()) and bool((keys[:cap] != -7).all())
        got = keys[:cap].cpu().numpy()
        assert np.unique(got).size == cap and np.isin(got, want).all()
        if cap == K:
            assert np.array_equal(np.sort(got), want)


@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_distances_equal_the_oracle(spacing, volumes):
    from skoots_amd.validate.lib import surface_distances
    for name, (gt, _) in volumes.items():
        e = S.expected(name, spacing)
        _, _, counts_g, keys_g, _, _, counts_p, keys_p = S.surfaces_of(name)
        sg, sp = (dev(offsets(counts_g)), dev(keys_g)), (dev(offsets(counts_p)), dev(keys_p))
        rows = [a for a, _ in e["pairs"].tolist()]
        for k, (q, t, pairs) in enumerate(((sg, sp, e["pairs"]), (sp, sg, e["pairs"][:, ::-1]))):
            off, d2 = surface_distances(q, t, dev(pairs), gt.shape, spacing)
            want = [e["d2"][a][k] for a in rows]
            assert d2.dtype == torch.float64 and d2.is_cuda and off.dtype == torch.int64
            assert off.tolist() == offsets([w.size for w in want]).tolist(), name
            got = d2.cpu().numpy()
            mine = np.concatenate(want) if want else np.zeros(0)
            assert np.array_equal(got, mine), (name, k, int(np.sum(got != mine)))


def test_synthetic_key_lists_around_the_tile_and_the_workgroup():
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import surface_distances
    tile = int(_ffi.lib.sk_surface_distance_tile())
    assert tile >= 64
    shape, q_off, q_keys, t_off, t_keys, pairs = S.synthetic(tile)
    assert sorted(np.diff(t_off).tolist()) == sorted([tile - 1, tile, tile + 1, 2 * tile + 1, 4 * tile + 3, tile + 7])
    assert sorted(np.diff(q_off).tolist()) == [1, 40, 255, 256, 257]
    q, t = (dev(q_off), dev(q_keys)), (dev(t_off), dev(t_keys))
    for spacing in (S.SPACINGS[0], S.SPACINGS[2], S.SPACINGS[3]):
        want_off, want = S.pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, S.weights(spacing))
        off, d2 = surface_distances(q, t, dev(pairs), shape, spacing)
        assert off.tolist() == want_off.tolist()
        got = d2.cpu().numpy()
        assert np.array_equal(got, want), int(np.sum(got != want))
        again = surface_distances(q, t, pairs, shape, spacing)[1]                 # pairs from the host; a second run
        assert torch.equal(again, d2)
    off, d2 = surface_distances(q, t, np.zeros((0, 2), np.int32), shape)          # P = 0
    assert off.tolist() == [0] and d2.shape == (0,)
    # an empty target segment: inf; an empty query segment: no output
    empty = (dev(np.array([0, 0], np.int64)), dev(np.zeros(0, np.int64)))
    off, d2 = surface_distances(q, empty, [[0, 0], [2, 0]], shape)
    assert off.tolist() == [0, 1, 257] and bool(torch.isinf(d2).all())
    off, d2 = surface_distances(empty, t, [[0, 1]], shape)
    assert off.tolist() == [0, 0] and d2.numel() == 0


def test_launch_budget_splits_without_changing_a_bit(monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    shape, q_off, q_keys, t_off, t_keys, pairs = S.synthetic(int(_ffi.lib.sk_surface_distance_tile()))
    q, t = (dev(q_off), dev(q_keys)), (dev(t_off), dev(t_keys))
    real = _ffi.lib.sk_surface_distances
    calls = []
    monkeypatch.setattr(_ffi.lib, "sk_surface_distances", lambda *a: calls.append(1) or real(*a))
    spacing = S.SPACINGS[3]
    off, whole = VL.surface_distances(q, t, pairs, shape, spacing)
    assert len(calls) == 1
    evaluations = int((np.diff(q_off)[pairs[:, 0]] * np.diff(t_off)[pairs[:, 1]]).sum())
    # a budget below the largest pair: the pair list is cut and the queries of the large pairs are
    budget = 257 * 1024 // 3
    assert budget < evaluations // 8
    monkeypatch.setattr(VL, "LAUNCH_BUDGET", budget)
    del calls[:]
    off2, parts = VL.surface_distances(q, t, pairs, shape, spacing)
    assert len(calls) >= evaluations // budget > 8
    assert torch.equal(off, off2) and torch.equal(whole, parts)
    launches = VL._launches(q_off, t_off, pairs.astype(np.int64), budget)
    assert len(launches) == len(calls)
    assert all(int(((qe - qb) * np.diff(t_off)[ts]).sum()) <= budget for qb, qe, ts in launches)
    # one query against more targets than the budget is a launch of its own
    assert [tuple(int(v[0]) for v in l) for l in VL._launches(np.array([0, 2]), np.array([0, 10]), np.array([[0, 0]]), 5)] \
        == [(0, 1, 0), (1, 2, 0)]


@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_compare_equals_the_oracle(spacing, volumes):
    from skoots_amd.validate.compare import compare
    for name, (gt, pred) in volumes.items():
        want = S.expected(name, spacing)["table"]
        got = compare(dev(gt), dev(pred), spacing)
        assert set(got) == set(S.COLUMNS + S.UNMATCHED), name
        for k, w in want.items():
            assert got[k].is_cuda and got[k].dtype == (torch.float64 if w.dtype == np.float64 else torch.int64), (name, k)
            g = got[k].cpu().numpy()
            assert g.shape == w.shape and np.array_equal(g, w, equal_nan=w.dtype == np.float64), (name, k, g, w)
    # (1, X, Y, Z), another dtype, a tolerance and a threshold of its own; two runs give the same bits
    gt, pred = volumes[S.BALL]
    want = S.expected(S.BALL, spacing, threshold=0.3, tolerance=1.5)["table"]
    a = compare(dev(gt[None].astype(np.int64)), dev(pred[None].astype(np.int16)), spacing, 0.3, 1.5)
    b = compare(dev(gt), dev(pred), spacing, 0.3, 1.5)
    for k, w in want.items():
        assert np.array_equal(a[k].cpu().numpy(), w, equal_nan=w.dtype == np.float64), k
        assert torch.equal(a[k], b[k]) or bool(torch.isnan(a[k]).all()), k


def test_compare_degenerate_and_refusals(volumes):
    from skoots_amd.validate.compare import compare
    gt = dev(volumes[S.SHIFTED][0])
    none = torch.zeros_like(gt)
    r = compare(gt, none)                                   # nothing predicted: every row unmatched
    assert r["gt_id"].tolist() == [1] and r["pred_id"].tolist() == [0] and bool(torch.isnan(r["hausdorff"]).all())
    assert r["unmatched_pred_id"].numel() == 0 and r["gt_surface_voxels"].tolist() == [int(S.surfaces_of(S.SHIFTED)[2][0])]
    r = compare(none, gt)                                   # nothing to find: every prediction unmatched
    assert r["gt_id"].numel() == 0 and r["unmatched_pred_id"].tolist() == [1]
    assert r["unmatched_pred_best_iou"].tolist() == [0.0]
    assert compare(none, none)["gt_id"].numel() == 0
    with pytest.raises(ValueError, match="one shape"):
        compare(gt, gt[:, :, :-1])
    with pytest.raises(TypeError):
        compare(gt.float(), gt)
    with pytest.raises(ValueError, match="tolerance"):
        compare(gt, gt, tolerance=-1.0)


def test_argument_checks_leave_the_outputs_untouched():
    from skoots_amd import _ffi
    shape, q_off, q_keys, t_off, t_keys, pairs = S.synthetic(int(_ffi.lib.sk_surface_distance_tile()))
    pairs = pairs[:3]
    out_off = offsets(np.diff(q_off)[pairs[:, 0]])
    t = {k: dev(v) for k, v in dict(qk=q_keys, qo=q_off, tk=t_keys, to=t_off, pr=pairs, oo=out_off).items()}
    d2 = torch.full((int(out_off[-1]) + 1,), -7.0, dtype=torch.float64, device=DEV)
    odd = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(d2.device)
    X, Y, Z = shape

    def call(X=X, Y=Y, Z=Z, P=len(pairs), qs=len(q_off) - 1, ts=len(t_off) - 1, w=(1.0, 1.0, 1.0), d2_p=_ffi.ptr(d2), **p):
        ptrs = {k: _ffi.ptr(v) for k, v in t.items()}
        ptrs.update(p)
        rc = _ffi.lib.sk_surface_distances(ptrs["qk"], ptrs["qo"], qs, ptrs["tk"], ptrs["to"], ts, ptrs["pr"], P,
                                           ptrs["oo"], X, Y, Z, *w, d2_p, st)
        torch.cuda.synchronize()
        return rc

    assert call(X=-1) == -1 and "negative" in _ffi.last_error()
    assert call(Z=2 ** 26 + 1) == -1 and "2^26" in _ffi.last_error()
    assert call(P=-1) == -1 and call(qs=-1) == -1 and call(ts=-1) == -1
    for w in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert call(w=w) == -1 and "finite" in _ffi.last_error()
    for null in ("qk", "qo", "tk", "to", "pr", "oo"):
        assert call(**{null: None}) == -1 and "NULL" in _ffi.last_error(), null
    assert call(d2_p=None) == -1 and "NULL" in _ffi.last_error()
    assert call(d2_p=d2.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert call(qo=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert call(pr=odd.data_ptr() + 2) == -1 and "aligned" in _ffi.last_error()
    down, flat, wrong, wild = q_off.copy(), t_off.copy(), out_off.copy(), pairs.copy()
    down[2], flat[-1], wild[1, 1] = down[1] - 1, 0, len(t_off) - 1
    wrong[-1] += 1
    bad = {k: dev(v) for k, v in dict(down=down, flat=flat, shifted=out_off + 1, wrong=wrong, wild=wild).items()}
    assert call(qo=_ffi.ptr(bad["down"])) == -1 and "monotone" in _ffi.last_error()
    assert call(to=_ffi.ptr(bad["flat"])) == -1 and "monotone" in _ffi.last_error()
    assert call(oo=_ffi.ptr(bad["shifted"])) == -1 and "start at 0" in _ffi.last_error()
    assert call(oo=_ffi.ptr(bad["wrong"])) == -1 and "outputs" in _ffi.last_error()
    assert call(pr=_ffi.ptr(bad["wild"])) == -1 and "segments" in _ffi.last_error()
    assert bool((d2 == -7.0).all())
    assert call(P=0) == 0 and bool((d2 == -7.0).all())      # nothing to do: success, nothing written
    assert call() == 0 and bool((d2[:-1] >= 0).all()) and float(d2[-1]) == -7.0
    # the surface passes
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    lut = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    keys = torch.full((65,), -7, dtype=torch.int64, device=DEV)
    produced = torch.full((2,), -7, dtype=torch.int64, device=DEV)

    def count(X, Y, Z, N=1, max_id=1, lab_p=_ffi.ptr(lab), lut_p=_ffi.ptr(lut), counts_p=_ffi.ptr(counts)):
        rc = _ffi.lib.sk_instance_surface_count(lab_p, X, Y, Z, lut_p, max_id, N, counts_p, st)
        torch.cuda.synchronize()
        return rc

    def emit(X, Y, Z, N=1, max_id=1, cap=64, lab_p=_ffi.ptr(lab), lut_p=_ffi.ptr(lut), keys_p=_ffi.ptr(keys),
             produced_p=_ffi.ptr(produced)):
        rc = _ffi.lib.sk_instance_surface_emit(lab_p, X, Y, Z, lut_p, max_id, N, cap, keys_p, produced_p, st)
        torch.cuda.synchronize()
        return rc

    for fn in (count, emit):
        assert fn(-1, 4, 4) == -1 and "negative" in _ffi.last_error()
        assert fn(4, 2 ** 26 + 1, 1) == -1 and "2^26" in _ffi.last_error()
        assert fn(2 ** 26, 2 ** 26, 2 ** 11) == -1 and "2^63" in _ffi.last_error()
        assert fn(4, 4, 4, N=-1) == -1 and fn(4, 4, 4, max_id=-1) == -1
        assert fn(4, 4, 4, lab_p=None) == -1 and fn(4, 4, 4, lut_p=None) == -1 and "NULL" in _ffi.last_error()
        assert fn(4, 4, 4, lab_p=odd.data_ptr() + 2) == -1 and "aligned" in _ffi.last_error()
        assert fn(0, 4, 4) == 0 and fn(4, 4, 4, N=0) == 0
    assert count(4, 4, 4, counts_p=None) == -1 and count(4, 4, 4, counts_p=odd.data_ptr() + 4) == -1
    assert emit(4, 4, 4, cap=-1) == -1 and emit(4, 4, 4, keys_p=None) == -1 and emit(4, 4, 4, produced_p=None) == -1
    assert emit(4, 4, 4, keys_p=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    for x in (counts, keys, produced):
        assert bool((x == -7).all())
    assert count(4, 4, 4) == 0 and counts.tolist() == [56, -7]                  # a 4 x 4 x 4 box: all but the 8 inside
    assert emit(4, 4, 4) == 0 and produced.tolist() == [56, -7] and bool((keys[56:] == -7).all())
    assert _ffi.lib.sk_abi_version() >= 19


def _table_tensors(table):
    return {k: torch.from_numpy(np.array(v)) for k, v in table.items()}


def test_command_end_to_end(tmp_path, volumes, capsys):
    from skoots_amd.validate.compare import format_compare_csv, format_csv, main
    from skoots_amd.validate.lib import instance_sums
    gt, pred = volumes[S.UNMATCHED_CASE]
    gt_path, pred_path = os.path.join(tmp_path, "truth.npy"), os.path.join(tmp_path, "pred.npy")
    np.save(gt_path, np.ascontiguousarray(gt.transpose(2, 0, 1)))               # stored [Z, X, Y]
    np.save(pred_path, np.ascontiguousarray(pred.transpose(2, 0, 1)))
    spacing = (0.5, 0.25, 3.0)
    args = [pred_path, "--spacing", *(str(v) for v in spacing)]
    # without --ground-truth: the instance statistics alone, as before
    out = main(args)
    assert out == os.path.join(tmp_path, "pred_instance_stats.csv")
    assert not os.path.exists(os.path.join(tmp_path, "pred_compare.csv"))
    ids, sums, boxes = instance_sums(dev(pred))
    plain = open(out).read()
    assert plain == format_csv(pred_path, ids, sums, boxes, pred.shape, spacing)
    assert capsys.readouterr().out == f"File Written: {out}\n"
    # with it: the same file again, and the comparison
    assert main(args + ["--ground-truth", gt_path, "--tolerance", "2.0"]) == out
    assert open(out).read() == plain
    text = open(os.path.join(tmp_path, "pred_compare.csv")).read()
    want = S.expected(S.UNMATCHED_CASE, spacing, tolerance=2.0)["table"]
    assert text == format_compare_csv(pred_path, gt_path, _table_tensors(want), spacing, 0.1, 2.0)
    rows = text.splitlines()
    assert len(rows) == 3 + 2 + 2 and rows[3].startswith("4,0,0.0,0.0,0,27,0,nan,nan,") and rows[5].startswith("0,9,0.0,nan,")
    os.remove(os.path.join(tmp_path, "pred_compare.csv"))
    main(args + ["--ground-truth", gt_path, "--tolerance", "2.0"])
    assert open(os.path.join(tmp_path, "pred_compare.csv")).read() == text      # a second run: byte-identical
    main(args + ["--ground-truth", gt_path, "--iou-threshold", "0.9"])
    want = S.expected(S.UNMATCHED_CASE, spacing, threshold=0.9)["table"]
    assert want["pred_id"].tolist() == [0, 0]
    assert open(os.path.join(tmp_path, "pred_compare.csv")).read() == \
        format_compare_csv(pred_path, gt_path, _table_tensors(want), spacing, 0.9, None)
    np.save(gt_path, np.ascontiguousarray(gt[:, :, :-1].transpose(2, 0, 1)))
    with pytest.raises(ValueError, match="one shape"):
        main(args + ["--ground-truth", gt_path])


def test_launch_budget_with_a_query_segment_shared_by_a_cut_and_an_uncut_pair(monkeypatch):
    """The prediction -> ground truth direction of an under-segmentation: one query segment in two pairs.  The budget cuts
    the first pair; its tail and the whole second pair land in one launch, whose query segments are refined by both."""
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    tile = int(_ffi.lib.sk_surface_distance_tile())
    shape, q_off, q_keys, t_off, t_keys, _ = S.synthetic(tile)
    nq, nt = np.diff(q_off), np.diff(t_off)
    qs, big, small = int(np.argmax(nq)), int(np.argmax(nt)), int(np.argmin(nt))
    assert (nq[qs], nt[big], nt[small]) == (257, 4 * tile + 3, tile - 1)
    pairs = np.array([[qs, big], [qs, small]], np.int64)
    budget = 120 * int(nt[big])                              # runs of 120 queries: 120, 120 and a tail of 17
    launches = VL._launches(q_off, t_off, pairs, budget)
    b0 = int(q_off[qs])
    # the last launch holds the tail (240, 257) and the whole second pair, split at the tail's cut
    assert [(l[0] - b0).tolist() for l in launches] == [[0], [120], [240, 0, 240]]
    assert (launches[2][1] - b0).tolist() == [257, 240, 257] and launches[2][2].tolist() == [big, small, small]
    q, t = (dev(q_off), dev(q_keys)), (dev(t_off), dev(t_keys))
    spacing = S.SPACINGS[3]
    off, whole = VL.surface_distances(q, t, pairs, shape, spacing)
    monkeypatch.setattr(VL, "LAUNCH_BUDGET", budget)
    off2, parts = VL.surface_distances(q, t, pairs, shape, spacing)
    want_off, want = S.pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, S.weights(spacing))
    assert off.tolist() == off2.tolist() == want_off.tolist()
    assert torch.equal(whole, parts) and np.array_equal(parts.cpu().numpy(), want)


def test_compare_splits_an_under_segmentation(monkeypatch, volumes):
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.compare import compare
    gt, pred = volumes[S.TWO_TO_ONE]
    want = S.expected(S.TWO_TO_ONE, S.SPACINGS[1])["table"]
    assert want["pred_shared"].tolist() == [2, 2]
    for budget in (5000, 1237):                              # below one pair; runs of a few queries
        monkeypatch.setattr(VL, "LAUNCH_BUDGET", budget)
        got = compare(dev(gt), dev(pred), S.SPACINGS[1])
        for k, w in want.items():
            assert np.array_equal(got[k].cpu().numpy(), w, equal_nan=w.dtype == np.float64), (budget, k)


def test_keys_of_a_volume_beyond_2_32_voxels_take_the_64_bit_decode():
    from skoots_amd.validate.lib import surface_distances
    shape, q_off, q_keys, t_off, t_keys, pairs = S.synthetic_wide()
    assert shape[0] * shape[1] * shape[2] == 2 ** 54
    q, t = (dev(q_off), dev(q_keys)), (dev(t_off), dev(t_keys))
    for spacing in (S.SPACINGS[0], S.SPACINGS[3]):
        want_off, want = S.pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, S.weights(spacing))
        off, d2 = surface_distances(q, t, pairs, shape, spacing)
        got = d2.cpu().numpy()
        assert off.tolist() == want_off.tolist() and np.array_equal(got, want), int(np.sum(got != want))
    # differences near 2^26 occur (at unit spacing the largest D2 is near 2^52): the squares are still exact
    assert S.pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, S.weights(S.SPACINGS[0]))[1].max() > 2.0 ** 50


def test_surfaces_of_a_mask_beyond_2_32_voxels():
    """The surface passes decode with 64-bit divisions from 2^32 voxels on, which only a mask of that size reaches: 1028
    x 2048 x 2048 int32, empty but for a 3 x 3 x 3 box and two single voxels, all at linear indices beyond 2^32 but one."""
    from skoots_amd import _ffi
    X, Y, Z = 1028, 2048, 2048
    V = X * Y * Z
    assert V >= 2 ** 32 and 1024 * Y * Z == 2 ** 32
    lab = torch.zeros((X, Y, Z), dtype=torch.int32, device=DEV)
    lab[1024:1027, 10:13, 2040:2043] = 1
    lab[0, 0, 0] = lab[X - 1, Y - 1, Z - 1] = 2
    lut = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    box = np.stack(np.meshgrid(np.arange(1024, 1027), np.arange(10, 13), np.arange(2040, 2043), indexing="ij"), -1)
    box = box.reshape(-1, 3)[np.arange(27) != 13]            # all but the centre
    want = np.sort(np.concatenate(((box[:, 0] * Y + box[:, 1]) * Z + box[:, 2], [V, V + V - 1]))).astype(np.int64)
    counts = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    keys = torch.full((want.size + 1,), -7, dtype=torch.int64, device=DEV)
    produced = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    st = _ffi.stream_ptr(lab.device)
    assert _ffi.lib.sk_instance_surface_count(_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), 2, 2, _ffi.ptr(counts), st) == 0
    assert counts.tolist() == [26, 2, -7]
    assert _ffi.lib.sk_instance_surface_emit(_ffi.ptr(lab), X, Y, Z, _ffi.ptr(lut), 2, 2, want.size, _ffi.ptr(keys),
                                             _ffi.ptr(produced), st) == 0
    assert produced.tolist() == [28, -7] and int(keys[-1]) == -7
    assert np.array_equal(np.sort(keys[:-1].cpu().numpy()), want)
