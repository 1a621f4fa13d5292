"""The nearest-instance transform on the CPU (no GPU needed): the three numpy statements of the definition in
tests/nearest_label_cases.py held against each other bit for bit and against scipy, the hand-computed ties, and the
pure parts of ``utils.grow``: the grow and shrink rules, the report, the refusals, the command's flags and file names.

tests/test_hip_nearest_label.py compares the device with the same oracle."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import edt_cases
from tests.nearest_label_cases import (INF, INTEGER_SPACINGS, NO_SITES, REACH, REACH_SITE, REACH_VOXEL, SIDES, SPACINGS,
                                       STRETCH, TIE_X, TIE_Y, TIE_Z, WHERE_CASE, brute_force, cases, expected, grow_rule,
                                       ids_of, limits, oracle, report_counts, restrict, shrink_rule, value, walk, weights,
                                       where_cases)

CASES = cases()
SAMPLE = 200          # voxels per (case, spacing) the pairwise brute force takes on the volumes it cannot take whole
WHOLE = 3000          # voxels up to which it takes every voxel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_cases_are_small_and_hold_those_of_the_distance_transform():
    assert set(edt_cases.cases()) < set(CASES)
    assert all(lab.size <= 40 * 40 * 70 for lab in CASES.values())
    assert CASES[STRETCH].shape[2] > 2 * 64 and not CASES[NO_SITES].any()
    assert CASES["corner site (13, 1, 1)"].shape == (13, 1, 1) and CASES["corner site (1, 17, 9)"].shape == (1, 17, 9)


@pytest.mark.parametrize("name", list(CASES))
def test_the_three_statements_agree_bit_for_bit(name):
    """the pairwise minimum with the global tie rule, the unpruned passes and the kernel's pruned walk are one function,
    at every limit"""
    lab = CASES[name]
    rng = np.random.default_rng(5)
    for spacing in SPACINGS:
        w = weights(spacing)
        ids, rows, d2, near = expected(name, spacing)
        assert d2.dtype == np.float64 and not np.isnan(d2).any()
        assert (d2[rows > 0] == 0).all() and (near[rows > 0] == rows[rows > 0]).all() and (d2[rows == 0] > 0).all()
        assert ((near == 0) == np.isinf(d2)).all()
        pts = np.argwhere(np.ones(lab.shape, bool))
        if lab.size > WHOLE:
            pts = pts[rng.choice(len(pts), SAMPLE, replace=False)]
        bd2, bnear = brute_force(rows, w, pts)
        assert np.array_equal(bits(bd2), bits(d2[tuple(pts.T)])), (name, spacing)
        assert np.array_equal(bnear, near[tuple(pts.T)]), (name, spacing)
        for limit2 in limits(name, spacing):
            want = expected(name, spacing, limit2)
            got = walk(rows, w, limit2)
            assert np.array_equal(bits(got[0]), bits(want[2])) and np.array_equal(got[1], want[3]), (name, spacing, limit2)
            assert ((want[2] <= limit2) | np.isinf(want[2])).all() and ((want[3] == 0) == np.isinf(want[2])).all()
            if limit2 == 0:
                assert ((want[3] > 0) == (rows > 0)).all()


def test_where_restricts_the_answers_never_the_sites():
    lab = CASES[WHERE_CASE]
    for spacing in (SPACINGS[1], SPACINGS[3]):
        w = weights(spacing)
        ids, rows, d2, near = expected(WHERE_CASE, spacing)
        for limit2 in limits(WHERE_CASE, spacing):
            for wname, where in where_cases(lab).items():
                want = oracle(rows, w, limit2, where)
                got = walk(rows, w, limit2, where)
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (wname, limit2)
                cached = expected(WHERE_CASE, spacing, limit2, where)
                assert np.array_equal(bits(cached[2]), bits(want[0])) and np.array_equal(cached[3], want[1])
                off = (where == 0) & (rows == 0)
                assert np.isinf(want[0][off]).all() and (want[1][off] == 0).all()
                assert (want[0][rows > 0] == 0).all() and (want[1][rows > 0] == rows[rows > 0]).all()
                on = where != 0
                plain = restrict(rows, d2, near, limit2)
                assert np.array_equal(bits(want[0][on]), bits(plain[0][on])) and np.array_equal(want[1][on], plain[1][on])
    # the sites are switched off in the last case and still answer their neighbours
    where = where_cases(lab)["off on the sites"]
    assert not where[lab > 0].any() and np.isfinite(oracle(rows, w, INF, where)[0]).all()


def test_the_pruned_walk_reads_no_more_than_its_bound():
    """a pass reads at most 2 floor(sqrt(limit2 / w)) positions per voxel"""
    for name in (edt_cases.BLOBS, STRETCH):
        rows = expected(name, SPACINGS[1])[1]
        w = weights(SPACINGS[1])
        for limit2 in (w[2] * 4.0, 100.0):
            reads = []
            walk(rows, w, limit2, reads=reads)
            for n, wa in zip(reads, (w[2], w[1], w[0])):
                assert n <= 2 * int(np.floor(np.sqrt(limit2 / wa))) * rows.size


@pytest.mark.parametrize("name", list(CASES))
def test_scipy_witnesses_the_distance_and_that_its_site_lies_at_it(name):
    """at integer spacings sqrt(D2) is scipy's distance bit for bit; scipy's nearest voxel is a site at value D2, but on
    ties not always ours, so its label is never compared"""
    for spacing in INTEGER_SPACINGS:
        ids, rows, d2, near = expected(name, spacing)
        if not (rows > 0).any():
            assert np.isinf(d2).all() and not near.any()
            continue
        dist, idx = ndimage.distance_transform_edt(rows == 0, sampling=spacing, return_indices=True)
        assert np.array_equal(bits(np.sqrt(d2)), bits(dist)), (name, spacing)
        assert (rows[tuple(idx)] > 0).all()
        w = weights(spacing)
        p = np.indices(rows.shape).astype(np.float64)
        dx, dy, dz = (p[k] - idx[k] for k in range(3))
        at = w[0] * (dx * dx) + (w[1] * (dy * dy) + w[2] * (dz * dz))
        assert np.array_equal(bits(at), bits(d2)), (name, spacing)


def test_hand_computed_ties():
    one = (1.0, 1.0, 1.0)
    for name, voxel, sites in ((TIE_Y, (0, 6, 0), ((0, 1, 0), (0, 2, 3), (0, 3, 4), (0, 6, 5))),
                               (TIE_X, (6, 0, 0), ((1, 0, 0), (2, 0, 3), (3, 0, 4), (6, 0, 5))),
                               (TIE_Z, (0, 0, 6), ((0, 0, 1), (0, 3, 2), (0, 4, 3), (0, 5, 6)))):
        lab = CASES[name]
        assert [int(lab[s]) for s in sites] == [1, 2, 3, 4] and (lab > 0).sum() == 4
        assert [value(voxel, s, one) for s in sites] == [25.0] * 4
        for statement in (lambda l2: expected(name, one, l2)[2:], lambda l2: walk(expected(name, one)[1], one, l2)):
            d2, near = statement(INF)
            assert d2[voxel] == 25.0 and near[voxel] == 1
            d2, near = statement(25.0)
            assert d2[voxel] == 25.0 and near[voxel] == 1
            d2, near = statement(24.0)
            assert d2[voxel] == INF and near[voxel] == 0
    # the low side wins at equal value, whatever the ids
    for spacing, centre in zip(SPACINGS, (6, 6, 5, 6)):       # x low (id 6) unless y is nearer: then y low (id 5)
        ids, rows, d2, near = expected(SIDES, spacing)
        assert ids_of(ids, near)[3, 3, 3] == centre and d2[3, 3, 3] == 4.0 * min(weights(spacing))
        for k, axis in enumerate("xyz"):
            shape = tuple(7 if a == k else 1 for a in range(3))
            ids, rows, d2, near = expected(f"low and high along {axis} {shape}", spacing)
            assert ids_of(ids, near).reshape(-1).tolist() == [2, 2, 2, 2, 1, 1, 1]
            assert d2.reshape(-1)[3] == weights(spacing)[k] * 4.0
    # the reach: a site exactly at limit2 is in, one float above it is out
    for spacing in SPACINGS:
        w = weights(spacing)
        v = value(REACH_VOXEL, REACH_SITE, w)
        at, below = limits(REACH, spacing)[-2:]
        assert at == v and below < v and np.nextafter(below, INF) == v
        assert expected(REACH, spacing, at)[2][REACH_VOXEL] == v and expected(REACH, spacing, at)[3][REACH_VOXEL] == 1
        assert expected(REACH, spacing, below)[2][REACH_VOXEL] == INF and expected(REACH, spacing, below)[3][REACH_VOXEL] == 0
    # the stretch, one line of it alone: z = 74 is 71 steps from both sites and the low one wins
    w = weights((1.0, 1.0, 3.0))
    rows = CASES[STRETCH][:1, :1, :].astype(np.int64)
    for statement in (oracle, walk):
        d2, near = statement(rows, w)
        assert d2[0, 0, 74] == 9.0 * 71 * 71 and near[0, 0, 74] == 1 and near[0, 0, 75] == 2
        near = statement(rows, w, limits(STRETCH, (1.0, 1.0, 3.0))[-2])[1]
        assert near[0, 0, 33] == 1 and near[0, 0, 34] == 0 and near[0, 0, 115] == 2 and near[0, 0, 114] == 0


def test_w_times_d_squared_and_the_order_of_the_sums():
    """the definition adds wy dy^2 + wz dz^2 first; the other order differs in the last bit somewhere"""
    w = weights((0.37, 0.41, 1.3))
    vals = [(w[0] * a + (w[1] * b + w[2] * c), (w[0] * a + w[1] * b) + w[2] * c)
            for a in (1.0, 4.0, 9.0) for b in (1.0, 4.0, 9.0) for c in (1.0, 4.0, 9.0)]
    assert any(x != y for x, y in vals)


# ---------------------------------------------------------------------------------------------------------- utils.grow

def _small():
    lab = CASES[edt_cases.BLOBS]
    spacing = (1.0, 1.0, 3.0)
    ids, rows, d2, near = expected(edt_cases.BLOBS, spacing)
    return lab, spacing, d2, ids_of(ids, near)


def test_grow_rule_on_the_host():
    from skoots_amd.utils.grow import apply_grow, make_report
    lab, spacing, d2, near_id = _small()
    within = (np.indices(lab.shape).sum(0) % 3 != 0)
    for d, wi in ((2.0, None), (3.5, within), (0.5, None)):
        want = grow_rule(lab, d2, near_id, d, wi)
        got = apply_grow(torch.from_numpy(lab), torch.from_numpy(near_id), torch.from_numpy(d2.copy()), d * d,
                         None if wi is None else torch.from_numpy(wi))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
        assert (want[lab != 0] == lab[lab != 0]).all() and set(np.unique(want)) <= set(np.unique(lab))
        if wi is not None:
            assert (want[~wi] == lab[~wi]).all()
        rep = make_report(torch.from_numpy(lab), got)
        assert {k: getattr(rep, k) for k in report_counts(lab, want)} == report_counts(lab, want)
        assert rep.voxels_removed == 0 and rep.ids_removed == 0 and rep.instances_in == rep.instances_out
        assert (rep.voxels_added > 0) == (d >= 1.0) and (rep.ids_grown > 0) == (d >= 1.0)


def test_shrink_rule_and_report_on_the_host():
    from skoots_amd.utils.grow import GrowReport, apply_shrink, make_report
    lab = CASES[edt_cases.BLOBS]
    spacing = (1.0, 1.0, 3.0)
    for closed in (False, True):
        edt = edt_cases.expected(edt_cases.BLOBS, spacing, closed)[2]
        for d in (1.0, 3.0):
            want = shrink_rule(lab, edt, -d)
            got = apply_shrink(torch.from_numpy(lab), torch.from_numpy(edt.copy()), d * d)
            assert np.array_equal(got.numpy(), want) and (want[want != 0] == lab[want != 0]).all()
            rep = make_report(torch.from_numpy(lab), got)
            counts = report_counts(lab, want)
            assert dataclass_dict(rep) == counts and rep.voxels_added == 0 and rep.ids_grown == 0
            assert rep.ids_removed == rep.instances_in - rep.instances_out and rep.voxels_removed > 0
    assert counts["ids_removed"] > 0                       # the small blobs vanish at 3 units
    assert dataclass_dict(GrowReport()) == dict.fromkeys(counts, 0)


def dataclass_dict(rep):
    import dataclasses
    return dataclasses.asdict(rep)


def test_refusals_need_no_device():
    from skoots_amd.lib.morphology import max_distance_squared
    from skoots_amd.utils.grow import check_distance, grow
    x = torch.zeros((3, 4, 5), dtype=torch.int32)
    for bad in (float("nan"), INF, -INF, "3", None, True):
        with pytest.raises(ValueError):
            grow(x, bad)
        with pytest.raises(ValueError):
            check_distance(bad)
    with pytest.raises(ValueError, match="within"):
        grow(x, -1.0, within=torch.ones((3, 4, 5), dtype=torch.bool))
    with pytest.raises(ValueError, match="MI355X"):
        grow(x, 1.0)                                       # a host tensor: there is no CPU fallback
    assert check_distance(-2) == -2.0 and check_distance(np.float32(1.5)) == 1.5
    assert max_distance_squared(None) == INF and max_distance_squared(0) == 0.0 and max_distance_squared(0.1) == 0.1 * 0.1
    for bad in (float("nan"), -1.0, -0.5, INF, "2", True):
        with pytest.raises(ValueError):
            max_distance_squared(bad)


def test_cli_flags_and_file_names():
    from skoots_amd.utils.grow import output_path, parse_args
    a = parse_args(["m.tif", "--distance", "3"])
    assert a.distance == 3.0 and a.spacing == (1.0, 1.0, 1.0) and a.within is None and not a.closed and not a.overwrite
    a = parse_args(["m.tif", "--distance", "-1.5", "--spacing", "1", "1", "3", "--closed", "-o"])
    assert a.distance == -1.5 and a.spacing == (1.0, 1.0, 3.0) and a.closed and a.overwrite
    a = parse_args(["I_instance_mask.tif", "--distance", "3", "--spacing", "1", "1", "3", "--within",
                    "I_skoots_vectors.zarr"])
    assert a.within == "I_skoots_vectors.zarr"
    for bad in ([], ["--distance"], ["--distance", "nan"], ["--distance", "inf"], ["--distance", "-1", "--within", "w.tif"],
                ["--distance", "1", "--spacing", "1", "1"], ["--distance", "1", "--spacing", "1", "0", "1"]):
        with pytest.raises(SystemExit) as e:
            parse_args(["m.tif"] + bad)
        assert e.value.code == 2
    assert output_path("/a/b.c/mask.tif", 2.0, False) == "/a/b.c/mask_grown.tif"
    assert output_path("/a/b.c/mask.tif", -2.0, False) == "/a/b.c/mask_shrunk.tif"
    assert output_path("/a/mask.tif", 0.0, False) == "/a/mask_grown.tif"
    assert output_path("/a/mask.tif", -2.0, True) == "/a/mask.tif"
