"""The definitions under ``compare()`` without a GPU: the numpy oracle of
tests/surface_distance_cases.py against scipy -- surfaces against ``m & ~binary_erosion(m)``, distances against
``distance_transform_edt`` -- and in closed form, and the host-side pieces of the feature (``match_instances``,
``pair_summaries``, ``format_compare_csv``, the command's parser) against the oracle and literal expectations."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import surface_distance_cases as S


@pytest.fixture(scope="module")
def volumes():
    return S.cases()


def test_surfaces_equal_scipy_erosion(volumes):
    for name, pair in volumes.items():
        for lab in pair:
            ids, rows = S.rows_of(lab)
            surf = S.surface(rows)
            counts, keys = S.surface_keys(rows)
            assert counts.sum() == surf.sum() == keys.size and np.all(counts > 0), name
            assert np.all(np.diff(keys) > 0)
            for r in range(1, ids.size + 1):
                m = rows == r
                want = m & ~ndimage.binary_erosion(m, border_value=0)
                assert np.array_equal(surf & m, want), (name, int(ids[r - 1]))
                mine = keys[(keys // rows.size) == r - 1] % rows.size
                assert np.array_equal(mine, np.flatnonzero(want.reshape(-1))), (name, int(ids[r - 1]))


@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_distances_equal_scipy_edt(spacing, volumes):
    exact = spacing in S.INTEGER_SPACINGS
    worst = 0.0
    for name in volumes:
        e = S.expected(name, spacing)
        _, rows_g, _, _, _, rows_p, _, _ = S.surfaces_of(name)
        for a, b in e["pairs"].tolist():
            sg, sp = S.surface(rows_g) & (rows_g == a + 1), S.surface(rows_p) & (rows_p == b + 1)
            for mine, query, target in ((e["d2"][a][0], sg, sp), (e["d2"][a][1], sp, sg)):
                want = ndimage.distance_transform_edt(~target, sampling=spacing)[query]     # raster order = key order
                got = np.sqrt(mine)
                if exact:
                    assert np.array_equal(got, want), (name, a, b)
                else:
                    rel = np.abs(got - want) / np.maximum(want, 1e-300)
                    worst = max(worst, float(rel.max(initial=0.0)))
                    assert np.all((got == want) | (rel <= 1e-12)), (name, a, b, float(rel.max()))
    print(f"spacing {spacing}: largest relative deviation from scipy {worst:.3g}")


@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_closed_forms(spacing):
    sx, sy, sz = spacing
    wx, wy, wz = S.weights(spacing)
    t = S.expected(S.IDENTICAL, spacing)["table"]
    assert t["pred_id"].tolist() == t["gt_id"].tolist() == [3, 7, 12]
    for k in ("hausdorff", "hausdorff95", "assd"):
        assert np.all(t[k] == 0.0)
    assert np.all(t["nsd"] == 1.0) and np.all(t["iou"] == 1.0) and np.all(t["dice"] == 1.0)
    assert np.all(t["pred_shared"] == 1) and t["unmatched_pred_id"].size == 0
    t = S.expected(S.SHIFTED, spacing)["table"]
    assert t["pred_id"].tolist() == [5] and t["hausdorff"][0] == math.sqrt(wx * 4.0) == 2.0 * sx
    assert t["intersection_voxels"].tolist() == [60] and t["iou"][0] == 60 / 140 and t["dice"][0] == 120 / 200
    # the centroids are fl(6 sx) and fl(4 sx): their difference is 2 sx up to the rounding of the first
    assert t["volume_difference"][0] == 0.0 and abs(t["centroid_distance"][0] - 2.0 * sx) <= 6.0 * sx * 2.0 ** -52
    if spacing in S.INTEGER_SPACINGS:
        assert t["centroid_distance"][0] == 2.0 * sx
    t = S.expected(S.CONCENTRIC, spacing)["table"]
    assert t["hausdorff"][0] == math.sqrt(wx + (wy + wz))             # corner to corner
    assert t["volume_difference"][0] == float(125 - 343) * (sx * sy * sz) and t["centroid_distance"][0] == 0.0
    t = S.expected(S.TWO_TO_ONE, spacing)["table"]
    assert t["pred_id"].tolist() == [6, 6] and t["pred_shared"].tolist() == [2, 2]
    assert t["hausdorff"].tolist() == [4.0 * sx, 4.0 * sx]            # the far face of the merged box
    t = S.expected(S.UNMATCHED_CASE, spacing)["table"]
    assert t["pred_id"].tolist() == [0, 3] and math.isnan(t["hausdorff"][0]) and t["iou"][0] == 0.0
    assert t["unmatched_pred_id"].tolist() == [9, 11] and t["pred_surface_voxels"].tolist()[0] == 0
    assert t["unmatched_pred_best_iou"].tolist() == [0.0, float(np.float32(1) / np.float32(27))]
    t = S.expected(S.TIE, spacing)["table"]
    assert t["pred_id"].tolist() == [3] and t["unmatched_pred_id"].tolist() == [8]
    t = S.expected(S.HUGE, spacing)["table"]
    assert t["gt_id"].tolist() == [2 ** 31 - 1, 2 ** 40] and t["pred_id"].tolist() == [2 ** 40, 5]
    assert t["unmatched_pred_id"].tolist() == [2 ** 31 - 1]
    counts = S.surfaces_of(S.BALL)[2]
    assert counts[0] > 1024                                           # more than one LDS tile of the kernel


def test_match_instances():
    from skoots_amd.validate.lib import match_instances
    iou = torch.tensor([[0.0, 0.5, 0.5, 0.2],      # a tie: the lowest column
                        [0.1, 0.0, 0.0, 0.0],      # exactly the threshold: strict, no match
                        [0.0, 0.0, 0.0, 0.0],
                        [0.3, 0.9, 0.0, 0.9],
                        [0.0, 0.7, 0.0, 0.0]], dtype=torch.float32)
    got = match_instances(iou, 0.1)
    assert got.dtype == torch.int64 and got.tolist() == [1, -1, -1, 1, 1]
    assert got.tolist() == S.match(iou.numpy(), np.float32(0.1)).tolist()
    assert match_instances(iou).tolist() == got.tolist()                              # 0.1 is the default
    assert match_instances(iou, 0.5).tolist() == [-1, -1, -1, 1, 1]
    assert match_instances(iou, 0.0).tolist() == [1, 0, -1, 1, 1]
    assert match_instances(torch.zeros((0, 3))).tolist() == [] and match_instances(torch.zeros((0, 3))).dtype == torch.int64
    assert match_instances(torch.zeros((2, 0))).tolist() == [-1, -1]
    assert match_instances(torch.zeros((0, 0))).shape == (0,)
    rng = np.random.default_rng(3)
    m = (rng.integers(0, 6, (40, 17)) / np.float32(5)).astype(np.float32)             # many ties
    assert match_instances(torch.from_numpy(m), 0.3).tolist() == S.match(m, 0.3).tolist()


@pytest.mark.parametrize("spacing", [S.SPACINGS[0], S.SPACINGS[3]])
def test_pair_summaries_equal_the_oracle(spacing, volumes):
    from skoots_amd.validate.lib import nearest_rank, pair_summaries
    assert [nearest_rank(n) for n in (1, 2, 19, 20, 21, 100, 101)] == [S.nearest_rank(n) for n in (1, 2, 19, 20, 21, 100, 101)]
    assert [S.nearest_rank(n) for n in (1, 20, 21, 100, 101)] == [0, 18, 19, 94, 95]
    tau2 = max(spacing) * max(spacing)
    for name in volumes:
        e = S.expected(name, spacing)
        rows = [a for a, _ in e["pairs"].tolist()]
        # the segments in a scrambled order inside: the reduction sorts them
        rng = np.random.default_rng(len(name))
        seg = [rng.permutation(e["d2"][a][0]) for a in rows] + [rng.permutation(e["d2"][a][1]) for a in rows]
        off = np.concatenate(([0], np.cumsum([s.size for s in seg]))).astype(np.int64)
        d2 = np.concatenate(seg) if seg else np.zeros(0)
        s = pair_summaries(torch.from_numpy(off), torch.from_numpy(d2), len(rows), tau2)
        t = e["table"]
        for k in ("hausdorff", "hausdorff95", "assd", "nsd"):
            assert s[k].dtype == torch.float64
            assert np.array_equal(s[k].numpy(), t[k][rows]), (name, k)
        assert s["gt_surface_voxels"].tolist() == t["gt_surface_voxels"][rows].tolist()
        assert s["pred_surface_voxels"].tolist() == t["pred_surface_voxels"][rows].tolist()
    with pytest.raises(ValueError, match="entries"):
        pair_summaries(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.float64), 1, 1.0)
    s = pair_summaries(torch.tensor([0, 2, 2]), torch.tensor([1.0, 4.0], dtype=torch.float64), 1, 1.0)
    assert math.isnan(s["hausdorff"][0]) and math.isnan(s["nsd"][0])               # an empty direction


def test_format_compare_csv_literal():
    from skoots_amd.validate.compare import COMPARE_COLUMNS, format_compare_csv
    nan = float("nan")
    result = {"gt_id": torch.tensor([4, 2 ** 40]), "pred_id": torch.tensor([0, 7]),
              "iou": torch.tensor([0.0, 0.5], dtype=torch.float64), "dice": torch.tensor([0.0, 2 / 3], dtype=torch.float64),
              "intersection_voxels": torch.tensor([0, 10]), "gt_voxels": torch.tensor([27, 15]),
              "pred_voxels": torch.tensor([0, 15]), "volume_difference": torch.tensor([nan, 0.0], dtype=torch.float64),
              "centroid_distance": torch.tensor([nan, 1.5], dtype=torch.float64),
              "gt_surface_voxels": torch.tensor([26, 15]), "pred_surface_voxels": torch.tensor([0, 14]),
              "hausdorff": torch.tensor([nan, 3.0], dtype=torch.float64),
              "hausdorff95": torch.tensor([nan, math.sqrt(2.0)], dtype=torch.float64),
              "assd": torch.tensor([nan, 0.1], dtype=torch.float64), "nsd": torch.tensor([nan, 0.75], dtype=torch.float64),
              "pred_shared": torch.tensor([0, 1]), "unmatched_pred_id": torch.tensor([9]),
              "unmatched_pred_best_iou": torch.tensor([0.03703703731298447], dtype=torch.float64),
              "unmatched_pred_voxels": torch.tensor([8]), "unmatched_pred_surface_voxels": torch.tensor([8])}
    text = format_compare_csv("pred.tif", "truth.tif", result, (1.0, 0.5, 3.0), 0.1, None)
    assert text == (
        "Mask File: pred.tif Ground Truth File: truth.tif\n"
        "Spacing: 1.0 0.5 3.0 IoU Threshold: 0.1 Tolerance: 3.0\n"
        "gt_id,pred_id,iou,dice,intersection_voxels,gt_voxels,pred_voxels,volume_difference,centroid_distance,"
        "gt_surface_voxels,pred_surface_voxels,hausdorff,hausdorff95,assd,nsd,pred_shared\n"
        "4,0,0.0,0.0,0,27,0,nan,nan,26,0,nan,nan,nan,nan,0\n"
        "1099511627776,7,0.5,0.6666666666666666,10,15,15,0.0,1.5,15,14,3.0,1.4142135623730951,0.1,0.75,1\n"
        "0,9,0.03703703731298447,nan,0,0,8,nan,nan,0,8,nan,nan,nan,nan,0\n")
    assert text.splitlines()[2] == COMPARE_COLUMNS == ",".join(S.COLUMNS)
    assert format_compare_csv("a", "b", result, (1.0, 0.5, 3.0), 0.25, 2.0).splitlines()[1] == \
        "Spacing: 1.0 0.5 3.0 IoU Threshold: 0.25 Tolerance: 2.0"


def test_parser_wants_ground_truth_for_its_switches(capsys):
    from skoots_amd.validate.compare import parse_args
    for extra in (["--tolerance", "2.0"], ["--iou-threshold", "0.3"]):
        with pytest.raises(SystemExit):
            parse_args(["mask.tif", *extra])
        assert "--ground-truth" in capsys.readouterr().err
    args = parse_args(["mask.tif", "--ground-truth", "gt.tif", "--tolerance", "2.0"])
    assert args.ground_truth == "gt.tif" and args.tolerance == 2.0 and args.iou_threshold == 0.1
    args = parse_args(["mask.tif"])
    assert args.ground_truth is None and args.tolerance is None


def test_library_functions_have_no_cpu_fallback():
    from skoots_amd.validate.compare import compare
    from skoots_amd.validate.lib import instance_surfaces, surface_distances
    x = torch.ones((3, 3, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_surfaces(x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        compare(x, x)
    off, keys = torch.tensor([0, 1]), torch.tensor([0])
    with pytest.raises(ValueError, match="no CPU fallback"):
        surface_distances((off, keys), (off, keys), [[0, 0]], (3, 3, 3))


def _check_launches(qo, to, pairs, budget):
    """every item of a launch is one of the launch's query segments (the offsets refined by the launch's cuts), a launch
    of several items stays within the budget, and the items in order are the pairs' queries in order"""
    from skoots_amd.validate.lib import _launches
    qo, to, pairs = np.asarray(qo, np.int64), np.asarray(to, np.int64), np.asarray(pairs, np.int64).reshape(-1, 2)
    launches = _launches(qo, to, pairs, budget)
    items = []
    for qb, qe, ts in launches:
        breaks = np.unique(np.concatenate((qo, qb, qe)))
        assert np.array_equal(breaks[np.searchsorted(breaks, qb) + 1], qe), (qb, qe, breaks)
        assert np.all(qe > qb)
        cost = int(((qe - qb) * np.maximum(np.diff(to)[ts], 1)).sum())
        assert cost <= budget or (len(np.unique(ts)) == 1 and qe.max() - qb.min() == 1), (cost, budget)
        items += list(zip(qb.tolist(), qe.tolist(), ts.tolist()))
    k = 0
    for qs, t in pairs.tolist():
        at = int(qo[qs])
        while at < int(qo[qs + 1]):
            b, e, tt = items[k]
            assert (b, tt) == (at, t) and e <= qo[qs + 1]
            at, k = e, k + 1
    assert k == len(items)
    return launches


def test_launches_split_a_query_segment_that_pairs_share():
    # one query segment of 105 voxels against targets of 10 and of 1 voxel, 1000 evaluations a launch: the first pair is
    # cut at 100, and its tail shares the second launch with the second pair, which is not cut by itself
    launches = _check_launches([0, 105], [0, 10, 11], [[0, 0], [0, 1]], 1000)
    assert [[v.tolist() for v in launch] for launch in launches] == \
        [[[0], [100], [0]], [[100, 0, 100], [105, 100, 105], [0, 1, 1]]]
    # the sizes at which the real budget meets it: a surface of 10^6 voxels that two ground truths chose
    _check_launches([0, 10 ** 6], [0, 5 * 10 ** 5, 5 * 10 ** 5 + 10 ** 4], [[0, 0], [0, 1]], 1 << 36)
    # two cut pairs over one segment with different runs, then the segment whole
    _check_launches([0, 7, 7, 400], [0, 13, 13, 50, 51], [[2, 0], [0, 3], [2, 2], [2, 3], [1, 0]], 900)
    rng = np.random.default_rng(1)
    for _ in range(300):
        nq, nt = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        qo = np.concatenate(([0], np.cumsum(rng.integers(0, 200, nq))))
        to = np.concatenate(([0], np.cumsum(rng.integers(0, 60, nt))))
        pairs = np.stack((rng.integers(0, nq, 8), rng.integers(0, nt, 8)), 1)
        _check_launches(qo, to, pairs, int(rng.integers(50, 3000)))
