"""CPU tests of the contact feature: the numpy restatement of ``sk_instance_contacts`` in
tests/contact_cases.py against a plain loop and against the invariants of the definition, and the pure host functions
on top of the table -- ``contact_columns``, the two CSV texts, ``plan_merge`` and both commands' ``parse_args``."""
import numpy as np
import pytest
import torch

from tests import contact_cases as K

MODES = [(c, b) for c in (6, 18, 26) for b in (False, True)]


def shared_volumes():
    return {"noise": K.sparse_noise((12, 13, 9), 1), "crossing": K.sparse_noise(K.CROSSING, 2),
            "edge": K.edge_contact((7, 8, 9)), "corner": K.corner_contact((7, 8, 9)),
            "checker": K.checkerboard((6, 7, 8), 4), "blob": K.blob(), "voxels": K.voxel_ids((3, 4, 5)),
            "many": K.many_ids((9, 10, 11), 40, 3), "split": K.split_blob()}


@pytest.mark.parametrize("connectivity,background", MODES)
def test_ref_contacts_equals_a_plain_loop(connectivity, background):
    for v in (K.sparse_noise((5, 6, 7), 5), K.many_ids((4, 5, 6), 9, 6), K.voxel_ids((2, 3, 4)), K.edge_contact((3, 4, 5)),
              np.zeros((2, 2, 2), np.int64), K.sparse_noise((1, 1, 9), 7), K.sparse_noise((1, 6, 1), 8)):
        got, want = K.ref_contacts(v, connectivity, background), K.loop_contacts(v, connectivity, background)
        assert np.array_equal(got, want)
        assert (got[:, 0] < got[:, 1]).all() and (got[:, 2:].sum(1) > 0).all()
        assert (got[:, 2 + K.CLASSES_AT[connectivity]:] == 0).all()
        assert background or (got[:, 0] > 0).all()


@pytest.mark.parametrize("name", sorted(shared_volumes()))
def test_contacts_plus_border_voxels_are_the_exposed_faces(name):
    """connectivity 6 with background: per id and axis, the contacts over all partners plus the id's voxels in the two
    border planes equal the exposed faces counted for that id alone"""
    v = shared_volumes()[name]
    n = K.rows_of(v)[1].size
    t = K.ref_contacts(v, 6, True)
    assert np.array_equal(K.face_contacts_per_row(t, n) + K.border_voxels(v), K.exposed_faces(v))


@pytest.mark.parametrize("perm", [(1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0)])
def test_transposing_the_volume_permutes_the_classes(perm):
    v = K.sparse_noise((6, 7, 8), 11)
    t, u = K.ref_contacts(v, 26, True), K.ref_contacts(np.transpose(v, perm), 26, True)
    # axis k of the transposed volume is axis perm[k] of the original
    face = [2 + perm[k] for k in range(3)]
    pair = {(0, 1): 5, (0, 2): 6, (1, 2): 7}
    edge = [pair[tuple(sorted((perm[a], perm[b])))] for a, b in ((0, 1), (0, 2), (1, 2))]
    assert np.array_equal(u, t[:, [0, 1, *face, *edge, 8]])


def test_relabelling_the_ids_keeps_the_counts():
    v = K.sparse_noise((7, 8, 9), 12, ids=(0, 1, 2, 3, 4))
    lut = np.array([0, 30, 7, 2 ** 31 - 1, 1000], np.int64)      # row order changes: 1 -> 30, 2 -> 7, ...
    t, u = K.ref_contacts(v, 26, False), K.ref_contacts(lut[v], 26, False)
    a, b = K.with_ids(t, [1, 2, 3, 4]), K.with_ids(u, sorted(lut[1:].tolist()))
    a[:, :2] = np.sort(lut[a[:, :2]], 1)
    assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b)


# ---- contact_columns and the CSV texts ----

TABLE = np.array([[2, 5, 4, 0, 2, 1, 0, 0, 3],       # ids 2-5: area 4 sy sz + 2 sx sy
                  [2, 9, 0, 6, 0, 0, 0, 0, 0],       # 2-9: 6 sx sz
                  [5, 9, 0, 0, 0, 2, 0, 1, 0],       # 5-9: edges only, no area
                  [0, 2, 9, 9, 9, 0, 0, 0, 0]], np.int64)      # background row: ignored
IDS = np.array([2, 5, 9, 11], np.int64)
FACE_AREA = np.array([24.0, 12.0, 6.0, 6.0])


def test_contact_area_is_the_face_area_expression():
    from skoots_amd.validate.compare import contact_area
    sx, sy, sz = 0.5, 2.0, 3.0
    assert contact_area(TABLE, (sx, sy, sz)).tolist() == [4 * (sy * sz) + 0 * (sx * sz) + 2 * (sx * sy), 6 * (sx * sz), 0.0,
                                                          9 * (sy * sz) + 9 * (sx * sz) + 9 * (sx * sy)]
    assert contact_area(np.zeros((0, 9), np.int64)).shape == (0,)


def test_contact_columns_partners_ties_and_none():
    from skoots_amd.validate.compare import contact_columns
    c = {k: v.tolist() for k, v in contact_columns(torch.from_numpy(TABLE), IDS, FACE_AREA).items()}
    assert c["neighbours"] == [2, 2, 2, 0]
    assert c["contact_area"] == [12.0, 6.0, 6.0, 0.0]
    assert c["contact_fraction"] == [0.5, 0.5, 1.0, 0.0]
    # id 2: 6.0 with 5 and 6.0 with 9 -- the smaller id; id 5: its edge-only partner 9 has no area; id 11: nobody
    assert c["largest_contact_id"] == [5, 2, 2, 0]
    assert c["largest_contact_area"] == [6.0, 6.0, 6.0, 0.0]
    assert all(v.dtype == (torch.int64 if k in ("neighbours", "largest_contact_id") else torch.float64)
               for k, v in contact_columns(TABLE, IDS, FACE_AREA).items())
    empty = contact_columns(np.zeros((0, 9), np.int64), IDS, FACE_AREA)
    assert empty["neighbours"].tolist() == [0] * 4 and empty["largest_contact_area"].tolist() == [0.0] * 4
    with pytest.raises(ValueError, match="not among ids"):
        contact_columns(np.array([[2, 6, 1, 0, 0, 0, 0, 0, 0]]), IDS, FACE_AREA)
    with pytest.raises(ValueError, match="face_area"):
        contact_columns(TABLE, IDS, FACE_AREA[:3])


def test_format_contacts_csv_text():
    from skoots_amd.validate.compare import CONTACT_CSV_COLUMNS, format_contacts_csv
    text = format_contacts_csv("m.tif", TABLE[::-1], IDS, FACE_AREA, (1.0, 1.0, 2.0), 18)
    assert text.splitlines() == ["Mask File: m.tif", "Spacing: 1.0 1.0 2.0 Connectivity: 18", CONTACT_CSV_COLUMNS,
                                 "2,5,4,0,2,1,0,0,3,10.0," + repr(10.0 / 24.0) + "," + repr(10.0 / 12.0),
                                 "2,9,0,6,0,0,0,0,0,12.0,0.5,2.0",
                                 "5,9,0,0,0,2,0,1,0,0.0,0.0,0.0"]
    assert CONTACT_CSV_COLUMNS == ("id_a,id_b,faces_x,faces_y,faces_z,edges_xy,edges_xz,edges_yz,corners,contact_area,"
                                   "fraction_a,fraction_b")
    assert format_contacts_csv("m.tif", np.zeros((0, 9), np.int64), IDS, FACE_AREA).count("\n") == 3


def test_format_csv_appends_the_contact_columns_last_and_only_on_request():
    from skoots_amd.validate.compare import CONTACT_COLUMNS, CSV_COLUMNS, derive, format_csv
    sums = torch.zeros((4, 13), dtype=torch.int64)
    sums[:, 0] = 1
    sums[:, 10:13] = 2                                  # one voxel each: 6 faces, face_area 6
    boxes = torch.zeros((4, 6), dtype=torch.int32)
    plain = format_csv("m.tif", IDS, sums, boxes, (3, 3, 3))
    text = format_csv("m.tif", IDS, sums, boxes, (3, 3, 3), contact_table=TABLE)
    assert plain.splitlines()[2] == CSV_COLUMNS and text.splitlines()[2] == CSV_COLUMNS + "," + CONTACT_COLUMNS
    assert float(derive(sums, boxes, (3, 3, 3))["face_area"][0]) == 6.0
    for a, b, tail in zip(plain.splitlines()[3:], text.splitlines()[3:],
                          ("2,12.0,2.0,5,6.0", "2,6.0,1.0,2,6.0", "2,6.0,1.0,2,6.0", "0,0.0,0.0,0,0.0")):
        assert b == a + "," + tail


# ---- plan_merge ----

def chain_table():
    """ids 3 - 4 - 7 in a row, and 7 - 20 by an edge only; face areas chosen so that the fractions are round"""
    ids = np.array([3, 4, 7, 20], np.int64)
    table = np.array([[3, 4, 8, 0, 0, 0, 0, 0, 0],       # area 8: fractions 8/16 and 8/32
                      [4, 7, 0, 2, 0, 0, 0, 0, 0],       # area 2: fractions 2/32 and 2/4
                      [7, 20, 0, 0, 0, 1, 0, 0, 0]], np.int64)
    return table, ids, np.array([16.0, 32.0, 4.0, 100.0])


def test_plan_merge_each_criterion_alone_and_both():
    from skoots_amd.utils.merge import plan_merge
    table, ids, fa = chain_table()
    lut, f = plan_merge(table, ids, fa, min_contact_area=8)
    assert lut.tolist() == [0, 3, 3, 7, 20]
    assert f == dict(instances_in=4, pairs_touching=3, pairs_merged=1, pairs_explicit=0, pairs_explicit_not_touching=0,
                     groups=1, instances_out=3)
    # the larger of the two fractions: 4-7 passes on the side of the small id 7 (2 / 4), 3-4 on the side of 3 (8 / 16)
    lut, f = plan_merge(table, ids, fa, min_contact_fraction=0.5)
    assert lut.tolist() == [0, 3, 3, 3, 20] and f["pairs_merged"] == 2 and f["groups"] == 1 and f["instances_out"] == 2
    lut, f = plan_merge(table, ids, fa, min_contact_fraction=0.51)
    assert lut.tolist() == [0, 3, 4, 7, 20] and f["pairs_merged"] == 0 and f["groups"] == 0 and f["instances_out"] == 4
    lut, f = plan_merge(table, ids, fa, min_contact_area=3, min_contact_fraction=0.5)
    assert lut.tolist() == [0, 3, 3, 7, 20] and f["pairs_merged"] == 1
    # area 0 admits the edge-only pair too: everything touching becomes one
    lut, f = plan_merge(table, ids, fa, min_contact_area=0)
    assert lut.tolist() == [0, 3, 3, 3, 3] and f["pairs_merged"] == 3 and f["instances_out"] == 1
    # the spacing enters the area: faces along y at (2, 1, 3) have area 6 each
    lut, _ = plan_merge(table, ids, fa, spacing=(2.0, 1.0, 3.0), min_contact_area=12)
    assert lut.tolist() == [0, 3, 3, 3, 20]


def test_plan_merge_is_transitive_and_the_smallest_id_wins():
    from skoots_amd.utils.merge import plan_merge
    table, ids, fa = chain_table()
    lut, f = plan_merge(table, ids, fa, pairs=[(20, 7), (7, 4)])
    assert lut.tolist() == [0, 3, 4, 4, 4] and f["groups"] == 1 and f["pairs_explicit"] == 2
    lut, f = plan_merge(table, ids, fa, min_contact_area=8, pairs=[(20, 7)])
    assert lut.tolist() == [0, 3, 3, 7, 7] and f["groups"] == 2 and f["instances_out"] == 2
    lut, f = plan_merge(torch.from_numpy(table), torch.from_numpy(ids), torch.from_numpy(fa), min_contact_area=1,
                        pairs=np.array([[20, 3]]))
    assert lut.tolist() == [0, 3, 3, 3, 3] and lut.dtype == np.int64


def test_plan_merge_explicit_pairs():
    from skoots_amd.utils.merge import plan_merge
    table, ids, fa = chain_table()
    lut, f = plan_merge(table, ids, fa, pairs=[(20, 3), (3, 20), (4, 3)])
    assert lut.tolist() == [0, 3, 3, 7, 3]
    assert f["pairs_explicit"] == 2 and f["pairs_explicit_not_touching"] == 1 and f["pairs_merged"] == 0
    with pytest.raises(ValueError, match=r"\[5, 99\]"):
        plan_merge(table, ids, fa, pairs=[(3, 99), (5, 4)])
    with pytest.raises(ValueError, match="twice"):
        plan_merge(table, ids, fa, pairs=[(3, 3)])
    with pytest.raises(ValueError, match="pairs of integer ids"):
        plan_merge(table, ids, fa, pairs=[(3, 4, 7)])
    with pytest.raises(ValueError, match="nothing to decide"):
        plan_merge(table, ids, fa)
    for bad in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="min_contact_area"):
            plan_merge(table, ids, fa, min_contact_area=bad)
        with pytest.raises(ValueError, match="min_contact_fraction"):
            plan_merge(table, ids, fa, min_contact_fraction=bad)


def test_plan_merge_on_the_split_blob():
    """the two halves share a wall that is a large share of either's surface; the small ball is far away"""
    from skoots_amd.utils.merge import plan_merge
    from skoots_amd.validate.compare import contact_area
    v = K.split_blob()
    _, ids = K.rows_of(v)
    table = K.with_ids(K.ref_contacts(v, 6, False), ids)
    fa = K.exposed_faces(v).sum(1).astype(np.float64)
    assert table[:, :2].tolist() == [[2, 5]] and table[0, 3] > 100 and table[0, 2] == table[0, 4] == 0
    assert contact_area(table)[0] / fa[:2].max() > 0.15
    lut, f = plan_merge(table, ids, fa, min_contact_fraction=0.15)
    assert lut.tolist() == [0, 2, 2, 9] and f["instances_out"] == 2


# ---- the commands' arguments ----

def test_merge_parse_args(capsys):
    from skoots_amd.utils.merge import parse_args
    a = parse_args(["m.tif", "--pairs", "3", "4", "9", "2", "--min-contact-area", "5", "--spacing", "1", "2", "3",
                    "--connectivity", "26", "--renumber", "-o"])
    assert a.pairs == ((3, 4), (9, 2)) and a.min_contact_area == 5.0 and a.min_contact_fraction is None
    assert tuple(a.spacing) == (1.0, 2.0, 3.0) and a.connectivity == 26 and a.renumber and a.overwrite
    a = parse_args(["m.tif", "--min-contact-fraction", "0.3"])
    assert a.pairs == () and a.connectivity == 6 and not a.renumber and not a.overwrite and a.min_contact_fraction == 0.3
    for bad in (["m.tif"], ["m.tif", "--pairs", "3", "4", "9"], ["m.tif", "--connectivity", "8", "--pairs", "1", "2"],
                ["m.tif", "--min-contact-area", "-1"], ["m.tif", "--min-contact-fraction", "nan"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert "even number" in capsys.readouterr().err


def test_compare_parse_args_contacts():
    from skoots_amd.validate.compare import parse_args
    assert parse_args(["m.tif"]).contacts is None
    assert parse_args(["m.tif", "--contacts", "18"]).contacts == 18
    with pytest.raises(SystemExit):
        parse_args(["m.tif", "--contacts", "7"])


def test_stats_per_instance_refuses_a_bad_contacts_value_before_the_device():
    from skoots_amd.validate.compare import stats_per_instance
    for bad in (True, 8, "6"):
        with pytest.raises(ValueError, match="contacts must be one of"):
            stats_per_instance(torch.zeros((2, 2, 2), dtype=torch.int32), contacts=bad)
