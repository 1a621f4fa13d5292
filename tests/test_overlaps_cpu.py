"""The host side of the overlap table, without a GPU: the numpy oracle of tests/overlap_cases.py
against a plain loop and its own invariants, ``match_instances_sparse`` against ``match_instances``, ``plan_relate`` on
hand-written tables and against plain loops, the CSV texts and the command lines.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import contact_cases as K
from tests import overlap_cases as O

SMALL = ["one_voxel", "line_z", "line_x", "below_one_chunk", "zero_a", "zero_b", "zero_both"]


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_a_plain_loop(name, background):
    a, b = O.PAIRS[name]()
    assert np.array_equal(O.ref_overlaps(a, b, background), O.loop_overlaps(a, b, background))


@pytest.mark.parametrize("name", ["many_ids", "ids_3_7_300_1000", "voxel_ids", "balls", "zero_a"])
def test_oracle_invariants_with_background(name):
    a, b = O.PAIRS[name]()
    t = O.ref_overlaps(a, b, True)
    ra, ids_a = K.rows_of(a)
    n = ids_a.size
    per_child = np.zeros(n + 1, np.int64)
    np.add.at(per_child, t[:, 0], t[:, 2])
    assert np.array_equal(per_child[1:], np.bincount(ra.reshape(-1), minlength=n + 1)[1:])
    assert int(t[:, 2].sum()) == int(((a > 0) | (b > 0)).sum())
    assert not ((t[:, 0] == 0) & (t[:, 1] == 0)).any() and (t[:, 2] > 0).all()
    swapped = O.ref_overlaps(b, a, True)[:, [1, 0, 2]]
    assert np.array_equal(swapped[np.lexsort((swapped[:, 1], swapped[:, 0]))], t)
    inside = t[(t[:, 0] > 0) & (t[:, 1] > 0)]
    assert np.array_equal(inside, O.ref_overlaps(a, b, False))


def test_the_overflow_pair_has_a_pair_per_voxel():
    a, b = O.voxel_ids_pair()
    t = O.ref_overlaps(a, b)
    assert t.shape[0] == a.size > O.LDS_SLOTS and (t[:, 2] == 1).all()
    assert O.many_ids_pair()[0].size % O.CHUNK and O.many_ids_pair()[0].size > 2 * O.CHUNK


# ---- match_instances_sparse ----

def sparse_of(dense):
    """(table (Q, 3), values (Q)) of the nonzero entries of a dense matrix, in (row, column) order"""
    r, c = np.nonzero(dense)
    table = np.stack((r + 1, c + 1, np.ones_like(r)), 1).astype(np.int64)
    return torch.from_numpy(table), torch.from_numpy(dense[r, c])


@pytest.mark.parametrize("threshold", [0.1, 0.0, 0.5, -1.0])
@pytest.mark.parametrize("seed", range(4))
def test_sparse_matching_equals_dense_matching_on_random_tables(seed, threshold):
    from skoots_amd.validate.lib import match_instances, match_instances_sparse
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    # few distinct values: ties inside a row are common, and so are rows without an entry
    dense = (rng.integers(1, 5, (n, m)) / np.float32(4)).astype(np.float32) * (rng.random((n, m)) < 0.15)
    table, values = sparse_of(dense)
    order = torch.from_numpy(rng.permutation(table.shape[0]))          # the order of the pairs does not matter
    want = match_instances(torch.from_numpy(dense), threshold)
    assert torch.equal(match_instances_sparse(table, values, n, m, threshold), want)
    assert torch.equal(match_instances_sparse(table[order], values[order], n, m, threshold), want)
    assert (want >= 0).any() or threshold >= 0.5


def test_sparse_matching_without_rows_or_columns():
    from skoots_amd.validate.lib import match_instances, match_instances_sparse
    none, no_values = torch.zeros((0, 3), dtype=torch.int64), torch.zeros(0)
    for n, m in ((0, 0), (0, 5), (4, 0), (4, 5)):
        want = match_instances(torch.zeros((n, m)), 0.1)
        got = match_instances_sparse(none, no_values, n, m, 0.1)
        assert got.dtype == torch.int64 and torch.equal(got, want)
    # background rows of the table are ignored
    table = torch.tensor([[0, 1, 9], [1, 0, 9], [1, 2, 3]])
    assert match_instances_sparse(table, torch.tensor([9.0, 9.0, 0.5]), 1, 2).tolist() == [1]


def test_sparse_matching_on_a_constructed_tie():
    from skoots_amd.validate.lib import match_instances, match_instances_sparse, overlap_ious
    g, p = O.tie_pair()
    iou = O.dense_iou(g, p)
    assert iou.shape == (1, 2) and iou[0, 0] == iou[0, 1] > 0.1         # first: the two fp32 values are equal
    pairs, values = overlap_ious(torch.from_numpy(O.ref_overlaps(g, p, True)), 1, 2)
    assert np.array_equal(values.numpy().view(np.uint32), iou[0].view(np.uint32))
    assert match_instances_sparse(pairs, values, 1, 2).tolist() == match_instances(torch.from_numpy(iou)).tolist() == [0]
    assert match_instances_sparse(pairs.flip(0), values.flip(0), 1, 2).tolist() == [0]


@pytest.mark.parametrize("name", ["many_ids", "ids_3_7_300_1000", "balls", "shared_and_unmatched"])
def test_overlap_ious_and_matching_on_the_case_volumes(name):
    from skoots_amd.validate.lib import match_instances, match_instances_sparse, overlap_ious
    a, b = O.PAIRS[name]()
    iou = O.dense_iou(a, b)
    n, m = iou.shape
    pairs, values = overlap_ious(torch.from_numpy(O.ref_overlaps(a, b, True)), n, m)
    assert values.dtype == torch.float32 and np.array_equal(pairs.numpy(), O.ref_overlaps(a, b, False))
    got = np.zeros_like(iou)
    got[pairs[:, 0].numpy() - 1, pairs[:, 1].numpy() - 1] = values.numpy()
    assert np.array_equal(got.view(np.uint32), iou.view(np.uint32))
    for threshold in (0.1, 0.0):
        assert torch.equal(match_instances_sparse(pairs, values, n, m, threshold),
                           match_instances(torch.from_numpy(iou), threshold))


def test_the_noise_volumes_have_no_tie():
    """no row of the noise pair has its largest IoU twice: a tie has to be constructed (``tie_pair``)"""
    iou = O.dense_iou(*O.noise_pair((12, 13, 9), 3, (0, 3, 7, 300, 1000)))
    best = iou.max(1)
    assert (best > 0).all() and ((iou == best[:, None]).sum(1) == 1).all()


# ---- plan_relate ----

CHILD_KEYS = ("voxels", "parent_row", "inside_voxels", "inside_fraction", "parents_touched", "outside_voxels")
PARENT_KEYS = ("voxels", "children", "children_voxels", "occupied_voxels", "occupancy")


def as_rows(d, keys):
    return [tuple(v) for v in zip(*(d[k].tolist() for k in keys))]


def test_plan_relate_on_a_hand_written_table():
    from skoots_amd.utils.relate import plan_relate
    table = np.array([[0, 1, 50], [0, 3, 7],             # parents' voxels under no child; parent 3 holds nobody
                      [1, 1, 4], [1, 2, 4], [1, 0, 2],   # child 1: a tie between parents 1 and 2 -> the lower row
                      [2, 0, 9],                         # child 2: wholly outside
                      [3, 2, 3], [3, 0, 1],              # child 3: 3 of 4 voxels inside parent 2
                      [4, 2, 6]], np.int64)
    c, p = plan_relate(table, 4, 3)
    assert as_rows(c, CHILD_KEYS) == [(10, 1, 4, 0.4, 2, 2), (9, 0, 0, 0.0, 0, 9), (4, 2, 3, 0.75, 1, 1), (6, 2, 6, 1.0, 1, 0)]
    assert as_rows(p, PARENT_KEYS) == [(54, 1, 10, 4, 4 / 54), (13, 2, 10, 13, 1.0), (7, 0, 0, 0, 0.0)]
    assert all(c[k].dtype == (np.float64 if k == "inside_fraction" else np.int64) for k in CHILD_KEYS)
    assert all(p[k].dtype == (np.float64 if k == "occupancy" else np.int64) for k in PARENT_KEYS)
    # the order of the rows does not matter, and torch tensors are taken
    c2, p2 = plan_relate(torch.from_numpy(table[::-1].copy()), 4, 3)
    assert as_rows(c2, CHILD_KEYS) == as_rows(c, CHILD_KEYS) and as_rows(p2, PARENT_KEYS) == as_rows(p, PARENT_KEYS)


def test_plan_relate_min_fraction_at_the_boundary():
    from skoots_amd.utils.relate import plan_relate
    table = np.array([[1, 1, 3], [1, 0, 1], [2, 1, 1], [2, 0, 9]], np.int64)
    at = plan_relate(table, 2, 1, 0.75)[0]                # 3 / 4 == 0.75 exactly: not below it
    assert at["parent_row"].tolist() == [1, 0] and at["inside_voxels"].tolist() == [3, 0]
    assert at["inside_fraction"].tolist() == [0.75, 0.0]
    above = plan_relate(table, 2, 1, float(np.nextafter(0.75, 1.0)))
    assert above[0]["parent_row"].tolist() == [0, 0] and above[1]["children"].tolist() == [0]
    assert above[1]["occupied_voxels"].tolist() == [4]    # what lies under a child does not depend on the assignment
    below = plan_relate(table, 2, 1, 0.1)[0]
    assert below["parent_row"].tolist() == [1, 1] and below["inside_fraction"].tolist() == [0.75, 0.1]
    for bad in (-0.1, 1.5, float("nan"), True, "0.5"):
        with pytest.raises(ValueError, match="min_fraction"):
            plan_relate(table, 2, 1, bad)
    with pytest.raises(ValueError, match="outside"):
        plan_relate(np.array([[3, 1, 1]]), 2, 1)
    with pytest.raises(ValueError, match="outside"):
        plan_relate(np.array([[0, 0, 1]]), 2, 1)


def test_plan_relate_without_children_or_parents():
    from skoots_amd.utils.relate import plan_relate
    c, p = plan_relate(np.zeros((0, 3), np.int64), 0, 0)
    assert all(v.shape == (0,) for v in c.values()) and all(v.shape == (0,) for v in p.values())
    c, p = plan_relate(np.array([[0, 1, 5], [0, 2, 6]]), 0, 2)
    assert p["voxels"].tolist() == [5, 6] and p["children"].tolist() == [0, 0] and p["occupancy"].tolist() == [0.0, 0.0]
    c, p = plan_relate(np.array([[1, 0, 5]]), 1, 0)
    assert as_rows(c, CHILD_KEYS) == [(5, 0, 0, 0.0, 0, 5)] and p["voxels"].shape == (0,)


@pytest.mark.parametrize("min_fraction", [0.0, 0.3])
@pytest.mark.parametrize("name", ["ids_3_7_300_1000", "balls", "many_ids", "zero_a", "zero_b"])
def test_plan_relate_equals_plain_loops(name, min_fraction):
    from skoots_amd.utils.relate import plan_relate
    a, b = O.PAIRS[name]()
    n, m = K.rows_of(a)[1].size, K.rows_of(b)[1].size
    if name == "many_ids":                                # the plain loops are quadratic: a corner of the pair
        a, b = a[:4, :6, :40], b[:4, :6, :40]
        n, m = K.rows_of(a)[1].size, K.rows_of(b)[1].size
    table = O.ref_overlaps(a, b, True)
    c, p = plan_relate(table, n, m, min_fraction)
    want_c, want_p = O.ref_relate(table, n, m, min_fraction)
    assert as_rows(c, CHILD_KEYS) == want_c and as_rows(p, PARENT_KEYS) == want_p


# ---- texts and command lines ----

def test_relate_csv_texts():
    from skoots_amd.utils import relate as R
    child = {"id": torch.tensor([3, 2 ** 40]), "voxels": torch.tensor([10, 9]), "parent_id": torch.tensor([7, 0]),
             "inside_voxels": torch.tensor([4, 0]), "inside_fraction": torch.tensor([0.4, 0.0], dtype=torch.float64),
             "parents_touched": torch.tensor([2, 0]), "outside_voxels": torch.tensor([2, 9])}
    assert R.format_parents_csv("c.tif", "p.tif", child, (1.0, 0.5, 2.0), 0.25) == (
        "Children File: c.tif Parents File: p.tif\n"
        "Spacing: 1.0 0.5 2.0 Min Fraction: 0.25\n"
        "id,voxels,parent_id,inside_voxels,inside_fraction,parents_touched,outside_voxels\n"
        "3,10,7,4,0.4,2,2\n"
        "1099511627776,9,0,0,0.0,0,9\n")
    parent = {"id": np.array([7]), "voxels": np.array([54]), "children": np.array([1]), "children_voxels": np.array([10]),
              "occupied_voxels": np.array([4]), "occupancy": np.array([4 / 54]), "children_volume": np.array([10.0])}
    assert R.format_children_csv("c.tif", "p.tif", parent) == (
        "Children File: c.tif Parents File: p.tif\n"
        "Spacing: 1.0 1.0 1.0 Min Fraction: 0.0\n"
        "id,voxels,children,children_voxels,occupied_voxels,occupancy,children_volume\n"
        "7,54,1,10,4,0.07407407407407407,10.0\n")


def test_instance_stats_csv_with_parents():
    from skoots_amd.validate import compare as CMP
    sums = torch.tensor([[8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 8, 8, 8]], dtype=torch.int64)      # a 2 x 2 x 2 cube at the origin
    boxes = torch.tensor([[0, 0, 0, 1, 1, 1]], dtype=torch.int32)
    plain = CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4))
    got = CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), parent_table=(torch.tensor([12]), torch.tensor([0.625])))
    a, b = plain.splitlines(), got.splitlines()
    assert a[:2] == b[:2] and b[2] == a[2] + ",parent,inside_fraction" and b[3] == a[3] + ",12,0.625" and len(b) == 4
    assert CMP.PARENT_COLUMNS == "parent,inside_fraction"
    with pytest.raises(ValueError, match="parent_table"):
        CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), parent_table=(torch.tensor([12, 3]), torch.tensor([0.5])))


def test_relate_parse_args():
    from skoots_amd.utils.relate import parse_args
    args = parse_args(["c.tif", "p.tif"])
    assert (args.children, args.parents, args.min_fraction, tuple(args.spacing)) == ("c.tif", "p.tif", 0.0, (1.0, 1.0, 1.0))
    assert not args.save_relabelled and not args.overwrite
    args = parse_args(["c.tif", "p.tif", "--min-fraction", "0.5", "--spacing", "1", "2", "3", "--save-relabelled", "-o"])
    assert args.min_fraction == 0.5 and list(args.spacing) == [1.0, 2.0, 3.0] and args.save_relabelled and args.overwrite
    for bad in (["c.tif"], ["c.tif", "p.tif", "--min-fraction", "1.5"], ["c.tif", "p.tif", "--min-fraction", "nan"],
                ["c.tif", "p.tif", "-o"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_compare_parse_args_of_the_new_switches():
    from skoots_amd.validate.compare import parse_args
    args = parse_args(["m.tif"])
    assert args.sparse_matching is False and args.parents is None and args.parent_min_fraction == 0.0
    args = parse_args(["m.tif", "--ground-truth", "g.tif", "--sparse-matching", "--parents", "p.tif",
                       "--parent-min-fraction", "0.5"])
    assert args.sparse_matching is True and args.parents == "p.tif" and args.parent_min_fraction == 0.5
    for bad in (["m.tif", "--sparse-matching"], ["m.tif", "--parent-min-fraction", "0.5"],
                ["m.tif", "--parents", "p.tif", "--parent-min-fraction", "2"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
