"""CPU tests of the mask clean-up: the scipy restatement of tests/clean_cases.py against scipy's
own functions, the pure planning functions of skoots_amd/utils/clean.py on hand-written tables and against the
restatement, the step order, the command's argument errors and the opt-in piece columns of the instance CSV.  No GPU."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from skoots_amd.utils import clean as CL
from skoots_amd.validate import compare as CMP
from tests import clean_cases as CC
from tests.test_instance_stats_cpu import _CSV_BOXES, _CSV_HEAD, _CSV_ROW_5, _CSV_ROW_9, _CSV_SUMS

MULTI = {
    "noise_small": lambda: CC.sparse_noise((12, 13, 9), 1),
    "noise_sparse_ids": lambda: CC.sparse_noise((12, 13, 9), 2, ids=(0, 3, 7, 300, 1000)),
    "two_blobs": lambda: CC.blob(seed=3, value=2) + CC.blob(seed=4, value=5) * (CC.blob(seed=3) == 0),
    "nested_shells": CC.nested_shells,
    "cavity_with_speck": CC.cavity_with_speck,
    "border_bodies": CC.border_bodies,
    "tie": lambda: CC.TIE,
}


def emulate_clean(mask, components="keep", connectivity=6, min_voxels=0, clear_border=False, fill_holes=False,
                  renumber=False):
    """``clean`` with the device work replaced by the restatement's tables: what plan_relabel / plan_fill decide"""
    mask = np.asarray(mask).astype(np.int64)
    piece, table = CC.ref_label_components(mask, connectivity)
    top = int(mask.max())
    lut, fields = CL.plan_relabel(table, top, components, min_voxels, clear_border, renumber)
    out = lut[piece]
    if fill_holes:
        zero_piece, zero_table = CC.ref_label_components(out, background=True)
        zero_lut, zero_fields = CL.plan_fill(zero_table)
        fields.update(zero_fields)
        out = np.where(zero_piece > 0, zero_lut[zero_piece], out)
    report = dict.fromkeys(CC.REPORT_FIELDS, 0)
    report.update(fields)
    return out, report


@pytest.mark.parametrize("seed", range(20))
def test_restated_fill_is_binary_fill_holes(seed):
    m = CC.blob(seed=seed, value=7)
    out, rep = CC.ref_clean(m, fill_holes=True)
    assert np.array_equal(out, ndi.binary_fill_holes(m > 0) * 7)
    assert rep["voxels_filled"] == int((out > 0).sum() - (m > 0).sum()) and rep["holes_ambiguous"] == 0
    got, got_rep = emulate_clean(m, fill_holes=True)
    assert np.array_equal(got, out) and got_rep == rep


@pytest.mark.parametrize("connectivity", (6, 18, 26))
@pytest.mark.parametrize("name", ("noise_small", "noise_sparse_ids", "two_blobs"))
def test_split_and_largest_leave_one_piece_per_id(name, connectivity):
    m = MULTI[name]()
    s = CC.structure(connectivity)
    split, rep = CC.ref_clean(m, components="split", connectivity=connectivity)
    assert np.array_equal(split > 0, m > 0)
    assert rep["ids_added"] == rep["pieces"] - rep["instances_in"] and rep["instances_out"] == rep["pieces"]
    largest, rep_l = CC.ref_clean(m, components="largest", connectivity=connectivity)
    assert rep_l["instances_out"] == rep_l["instances_in"] and rep_l["pieces_removed"] == rep["ids_added"]
    for out in (split, largest):
        for u in np.unique(out[out > 0]):
            assert ndi.label(out == u, s)[1] == 1
    for u in np.unique(m[m > 0]):                                # the piece an id keeps is its largest one
        lab, n = ndi.label(m == u, s)
        assert (largest == u).sum() == (split == u).sum() == np.bincount(lab.reshape(-1))[1:].max()


@pytest.mark.parametrize("name", list(MULTI))
@pytest.mark.parametrize("kwargs", [
    dict(), dict(components="largest"), dict(components="split", connectivity=18), dict(components="split", min_voxels=3),
    dict(min_voxels=30, fill_holes=True), dict(clear_border=True), dict(clear_border=(True, False, False), fill_holes=True),
    dict(components="largest", connectivity=26, min_voxels=2, clear_border=(False, False, True), fill_holes=True, renumber=True),
], ids=str)
def test_plans_agree_with_the_restatement(name, kwargs):
    m = MULTI[name]()
    want, want_rep = CC.ref_clean(m, **kwargs)
    got, got_rep = emulate_clean(m, **kwargs)
    assert got_rep == want_rep
    if kwargs.get("renumber"):                                   # the plan leaves ranks; first-seen order is the device's step
        _, first = np.unique(got.reshape(-1), return_index=True)
        lut = np.zeros(int(got.max()) + 1, np.int64)
        ids = np.unique(got)
        order = ids[np.argsort(first)]
        order = order[order > 0]
        lut[order] = np.arange(1, order.size + 1)
        got = lut[got]
    assert np.array_equal(got, want)


def _rows(*rows):
    return np.array([r + (0, 0) for r in rows], np.int64).reshape(-1, 6)


def test_plan_relabel_tie_and_new_ids():
    # value, voxels, first voxel, border bits: id 4 twice with 3 voxels, id 2 in three pieces, id 9 alone
    t = _rows((4, 3, 0, 0), (2, 1, 5, 0), (4, 3, 7, 0), (2, 6, 9, 0), (9, 2, 11, 0), (2, 6, 20, 0))
    lut, f = CL.plan_relabel(t, 9, "largest")
    assert lut.tolist() == [0, 4, 0, 0, 2, 9, 0]                 # the tie goes to the first voxel, twice
    assert (f["pieces"], f["instances_in"], f["ids_in_pieces"], f["pieces_removed"], f["voxels_cleared"]) == (6, 3, 2, 3, 10)
    lut, f = CL.plan_relabel(t, 9, "split")
    assert lut.tolist() == [0, 4, 10, 11, 2, 9, 12]              # new ids in the order of the pieces' first voxels
    assert f["ids_added"] == 3 and f["instances_out"] == 6 and f["voxels_cleared"] == 0
    lut, f = CL.plan_relabel(t, 9, "keep")
    assert lut.tolist() == [0, 4, 2, 4, 2, 9, 2] and f["instances_out"] == 3
    lut, f = CL.plan_relabel(torch.from_numpy(t), 9, "keep")     # CPU torch in
    assert lut.tolist() == [0, 4, 2, 4, 2, 9, 2] and lut.dtype == np.int64


def test_plan_relabel_min_voxels_counts_the_id_as_it_stands():
    t = _rows((4, 3, 0, 0), (4, 3, 7, 0), (5, 5, 9, 0))
    assert CL.plan_relabel(t, 5, "keep", min_voxels=6)[0].tolist() == [0, 4, 4, 0]      # 3 + 3 voxels: id 4 stays
    lut, f = CL.plan_relabel(t, 5, "split", min_voxels=5)
    assert lut.tolist() == [0, 0, 0, 5] and f["ids_removed_small"] == 2 and f["ids_added"] == 1
    assert CL.plan_relabel(t, 5, "largest", min_voxels=4)[0].tolist() == [0, 0, 0, 5]


def test_plan_relabel_border_bits_per_axis():
    t = _rows((1, 9, 0, 1), (2, 9, 1, 8), (3, 9, 2, 32), (4, 9, 3, 0), (4, 1, 4, 2))
    assert CL.plan_relabel(t, 4, clear_border=True)[0].tolist() == [0, 0, 0, 0, 0, 0]
    assert CL.plan_relabel(t, 4, clear_border=(True, True, False))[0].tolist() == [0, 0, 0, 3, 0, 0]
    assert CL.plan_relabel(t, 4, clear_border=(False, False, True))[0].tolist() == [0, 1, 2, 0, 4, 4]
    lut, f = CL.plan_relabel(t, 4, "largest", clear_border=(True, False, False))
    assert lut.tolist() == [0, 0, 2, 3, 4, 0] and f["ids_removed_border"] == 1   # 4's speck on the face went in step 1
    lut, f = CL.plan_relabel(t, 4, "keep", min_voxels=10, clear_border=True)
    assert f["ids_removed_small"] == 3 and f["ids_removed_border"] == 1          # an id is counted where it is cleared first


def test_plan_relabel_int32_overflow_names_renumber():
    t = _rows((2 ** 31 - 1, 3, 0, 0), (1, 2, 4, 0), (1, 1, 9, 0))
    assert CL.plan_relabel(t, 2 ** 31 - 1, "keep")[0].max() == 2 ** 31 - 1
    with pytest.raises(ValueError, match="renumber=True"):
        CL.plan_relabel(t, 2 ** 31 - 1, "split")
    lut, _ = CL.plan_relabel(t, 2 ** 31 - 1, "split", renumber=True)
    assert lut.tolist() == [0, 2 ** 31 - 1, 1, 2 ** 31]
    with pytest.raises(ValueError, match="renumber=True"):
        CL.plan_relabel(_rows((2 ** 40, 3, 0, 0)), 2 ** 40, "keep")


def test_plan_argument_errors():
    t = _rows((1, 1, 0, 0))
    for kw in (dict(components="all"), dict(min_voxels=-1), dict(min_voxels=1.5), dict(clear_border=(True, False)),
               dict(clear_border="xy"), dict(clear_border=(1, 0, 0))):
        with pytest.raises(ValueError):
            CL.plan_relabel(t, 1, **kw)
    with pytest.raises(ValueError, match="positive"):
        CL.plan_relabel(_rows((0, 1, 0, 0)), 1)
    with pytest.raises(ValueError, match="zero"):
        CL.plan_fill(t)
    lut, f = CL.plan_relabel(np.zeros((0, 6), np.int64), 0, "split")
    assert lut.tolist() == [0] and f["pieces"] == 0 and f["instances_out"] == 0


def test_plan_fill():
    # value, voxels, first voxel, border bits, min and max neighbour id
    t = np.array([[0, 100, 0, 63, 1, 9], [0, 4, 50, 0, 5, 5], [0, 2, 60, 0, 5, 9], [0, 1, 70, 4, 9, 9], [0, 3, 80, 0, 9, 9]])
    lut, f = CL.plan_fill(t)
    assert lut.tolist() == [0, 0, 5, 0, 0, 9]                    # min != max is left, a face is left
    assert f == dict(holes_filled=2, holes_ambiguous=1, voxels_filled=7)
    assert CL.plan_fill(np.zeros((0, 6), np.int64))[0].tolist() == [0]


def test_step_order_speck_in_a_cavity():
    m = CC.cavity_with_speck()
    assert (m == 3).sum() == 124
    solid = np.zeros_like(m)
    solid[1:13, 1:13, 1:13] = 2
    for run in (CC.ref_clean, emulate_clean):
        out, rep = run(m, min_voxels=200, fill_holes=True)
        assert np.array_equal(out, solid) and rep["ids_removed_small"] == 1 and rep["voxels_filled"] == 343
        out, rep = run(m, fill_holes=True)                           # filling alone: the pocket touches two ids
        assert np.array_equal(out, m) and rep["holes_ambiguous"] == 1 and rep["holes_filled"] == 0


def test_restated_cases_are_what_their_names_say():
    assert [ndi.label(CC.serpentine() > 0, CC.structure(k))[1] for k in (6, 18, 26)] == [1, 1, 1]
    assert [ndi.label(CC.checkerboard((5, 6, 7)), CC.structure(k))[1] for k in (6, 18, 26)] == [105, 1, 1]
    piece, table = CC.ref_label_components(CC.u_shape())
    assert table[:, 1].tolist()[1] == 1 and table.shape[0] == 2 and table[0, 2] < table[1, 2]
    assert [CC.ref_label_components(CC.edge_contact((5, 9, 66)), k)[1].shape[0] for k in (6, 18, 26)] == [5 * 9 * 66, 2, 2]
    ones = [int((CC.ref_label_components(CC.corner_contact((5, 9, 66)), k)[1][:, 0] == 1).sum()) for k in (6, 18, 26)]
    assert ones[0] == ones[1] > 1 and ones[2] == 1
    out, _ = CC.ref_clean(CC.diagonal_pocket(), fill_holes=True)
    assert out[2, 2, 2] == 4 and out[1, 1, 2] == 0
    out, _ = CC.ref_clean(CC.border_pocket(), fill_holes=True)
    assert out[0, 3, 3] == 0 and out[3, 3, 3] == 6
    out, _ = CC.ref_clean(CC.border_bodies(), clear_border=(True, True, False))
    assert np.unique(out).tolist() == [0, 1, 4]
    assert CC.ref_clean(CC.TIE, components="largest")[0].ravel().tolist() == [4, 4, 4, 0, 0, 0, 0, 0, 0]
    assert CC.ref_clean(CC.TIE, components="split")[0].ravel().tolist() == [4, 4, 4, 0, 0, 5, 5, 5, 0]


def test_command_argument_errors(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        CL.main([str(tmp_path / "mask.tif")])
    assert e.value.code == 2 and "nothing was asked for" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        CL.main([str(tmp_path / "mask.tif"), "--components", "keep"])          # keep alone asks for nothing either
    with pytest.raises(SystemExit):
        CL.main([str(tmp_path / "mask.tif"), "--connectivity", "7", "--fill-holes"])
    with pytest.raises(SystemExit):
        CL.main([str(tmp_path / "mask.tif"), "--min-voxels", "-2"])
    with pytest.raises(FileNotFoundError):
        CL.main([str(tmp_path / "mask.tif"), "--fill-holes"])
    a = CL.parse_args(["m.tif", "--clear-border"])
    assert a.clear_border is True and a.components == "keep" and a.min_voxels == 0
    a = CL.parse_args(["m.tif", "--clear-border", "x", "y", "--components", "split", "--connectivity", "26", "-o"])
    assert a.clear_border == (True, True, False) and a.components == "split" and a.connectivity == 26 and a.overwrite
    assert CL.parse_args(["m.tif", "--renumber"]).clear_border is False


def test_csv_without_pieces_is_unchanged_and_with_them_gains_two_columns():
    args = ("dir/mask.tif", [5, 9], _CSV_SUMS, _CSV_BOXES, (4, 5, 6), (0.5, 0.5, 3.0))
    assert CMP.format_csv(*args) == CMP.format_csv(*args, piece_table=None) == _CSV_HEAD + _CSV_ROW_5 + _CSV_ROW_9
    table = torch.tensor([[5, 6, 0, 1, 0, 0], [9, 1, 119, 42, 0, 0], [5, 2, 7, 0, 0, 0]])
    text = CMP.format_csv(*args, piece_table=table)
    assert text == (_CSV_HEAD[:-1] + ",pieces,largest_piece_voxels\n" + _CSV_ROW_5[:-1] + ",2,6\n" + _CSV_ROW_9[:-1] + ",1,1\n")
    cols = CMP.pieces_columns(table, torch.tensor([5, 9]))
    assert cols["pieces"].tolist() == [2, 1] and cols["largest_piece_voxels"].tolist() == [6, 1]
    with pytest.raises(ValueError, match="not among"):
        CMP.pieces_columns(table, [5])
    assert CMP.parse_args(["m.tif"]).pieces is None and CMP.parse_args(["m.tif", "--pieces", "18"]).pieces == 18
    with pytest.raises(SystemExit):
        CMP.parse_args(["m.tif", "--pieces", "7"])
