"""The local thickness on the CPU (no GPU needed): the two numpy statements of the definition in
tests/local_thickness_cases.py held against each other bit for bit, the facts that follow from the definition, the pinned
voxels of the special cases, the host columns of ``validate.compare.local_thickness_columns``, the CSV text and the
command's flags.

tests/test_hip_local_thickness.py compares the device with the same statements."""
import math

import numpy as np
import pytest
import torch

from tests.edt_cases import row_max
from tests.local_thickness_cases import (BRUTE_SAMPLE, FORMS, FORMS_CENTRE, FORMS_OFFSET, FORMS_SPACING, HALF, INF, LARGE,
                                         MODES, NECK_345, NECK_345_CENTRE, NECK_345_OFFSET, SPACINGS, THIN, TUBE,
                                         brute_force, cases, d2_of, expected, half_extent, table_of, weights)
from tests.test_edt_cpu import PLAIN, _measured

CASES = cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_cases_are_small_and_cover_the_shapes():
    assert all(lab.size <= 40 * 40 * 70 for lab in CASES.values())
    shapes = [lab.shape for lab in CASES.values()]
    assert all(any(s[k] == 1 for s in shapes) for k in range(3))           # an extent of 1 in every axis
    assert all(n in CASES for n in (HALF, NECK_345, FORMS, TUBE) + THIN)
    assert "shared plane (6, 7, 8)" in CASES and "diagonal (8, 8, 8)" in CASES and "blobs (24, 40, 70)" in CASES
    assert (CASES[HALF][:, :, :8] == 2).all() and not CASES[HALF][:, :, 8:].any()


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_statements_agree_and_the_facts_hold(name):
    lab = CASES[name]
    for spacing in SPACINGS:
        w = weights(spacing)
        for closed in MODES:
            ids, rows, d2, t2 = expected(name, spacing, closed)
            fg = rows > 0
            points = np.argwhere(fg)
            if points.shape[0] > LARGE:                                     # a sample: the pairwise form costs fg x volume
                rng = np.random.default_rng(points.shape[0])
                points = points[np.sort(rng.choice(points.shape[0], BRUTE_SAMPLE, replace=False))]
            brute, cross = brute_force(rows, d2, w, points)
            at = tuple(points.T)
            assert np.array_equal(bits(brute), bits(t2[at])), (name, spacing, closed)
            assert cross == 0, (name, spacing, closed)                      # no ball reaches another row
            assert (t2[fg] >= d2[fg]).all() and (t2[fg] > 0).all() and not t2[~fg].any()
            assert np.array_equal(bits(row_max(rows, t2)), bits(row_max(rows, d2)))
            assert t2.shape == lab.shape and t2.dtype == np.float64


def test_an_instance_alone_in_the_volume_is_inf_in_open_mode_only():
    ids, rows, d2, t2 = expected("one label (8, 9, 10)", SPACINGS[1], False)
    assert (d2 == INF).all() and (t2 == INF).all()
    ids, rows, d2, t2 = expected("one label (8, 9, 10)", SPACINGS[1], True)
    assert np.isfinite(t2).all() and t2.max() == d2.max() and t2.min() >= 1.0


def test_half_is_clipped_by_five_faces():
    spacing = SPACINGS[1]
    ids, rows, d2, t2 = expected(HALF, spacing, False)
    sz2 = weights(spacing)[2]
    assert d2[0, 0, 0] == 64.0 * sz2 and d2.max() == 64.0 * sz2            # the only outside voxels are those of z >= 8
    assert (t2[:, :, 0] == 64.0 * sz2).all()
    # a voxel of the last layer is inside the ball of (x, y, 0) only where the lateral offset keeps d2 below 64 sz^2
    assert t2[5, 5, 7] == d2[5, 5, 0] and half_extent(d2[0, 0, 0], 1.0, 10) == 10


def test_the_ball_is_open_at_3_4_5():
    ids, rows, d2, t2 = expected(NECK_345, (1.0, 1.0, 1.0), False)
    c = np.array(NECK_345_CENTRE)
    p = tuple(c + NECK_345_OFFSET)
    assert d2[tuple(c)] == 25.0 and rows[tuple(c + (3, 4, 0))] == 0       # the nearest outside voxel, at 5 exactly
    assert rows[p] > 0 and d2_of((1.0, 1.0, 1.0), 5.0, 0.0, 0.0) == 25.0   # the neck voxel lies at 5 exactly as well
    assert t2[p] == 17.0 < 25.0                                           # <= in place of < would give 25
    assert t2[tuple(c + (4, 0, 0))] == 25.0 and t2[tuple(c + (6, 0, 0))] == 1.0


def test_the_rounding_form_decides_a_voxel_at_spacing_037():
    w = weights(FORMS_SPACING)
    dx, dy, dz = (float(v) for v in FORMS_OFFSET)
    D = w[1] * 25.0
    defined = d2_of(w, dx, dy, dz)
    other = (w[0] * dx) * dx + ((w[1] * dy) * dy + (w[2] * dz) * dz)         # (w d) d
    assert defined == D and other < D                                       # the forms decide membership differently
    ids, rows, d2, t2 = expected(FORMS, FORMS_SPACING, False)
    c = np.array(FORMS_CENTRE)
    p = tuple(c + FORMS_OFFSET)
    assert d2[tuple(c)] == D and rows[tuple(c - FORMS_OFFSET)] == 0 and rows[p] > 0
    assert t2[p] < D and t2[tuple(c + (0, 4, 0))] == D                      # (w d) d would paint p with D


def test_the_thinnest_place_of_a_tube_is_its_constriction():
    from skoots_amd.validate.compare import local_thickness_columns
    for closed in MODES:
        ids, rows, d2, t2 = expected(TUBE, (1.0, 1.0, 1.0), closed)
        col = local_thickness_columns(table_of(rows, t2), 1)
        assert col["local_radius_min"].tolist() == [1.0]                    # one voxel across: a radius of one spacing
        assert t2[11, 4, 4] == 1.0 and t2[12, 4, 4] == 1.0 and t2[3, 4, 4] == 9.0 and t2[3, 6, 4] == 9.0
        assert 1.0 < col["local_radius_mean"].item() < 3.0 and col["local_radius_std"].item() > 0.0
        assert math.sqrt(row_max(rows, d2)[0]) == 3.0                       # the inscribed radius sees the tube only


def test_table_of():
    rows = np.array([[[0, 1, 1, 2, 2, 2, 0]]])
    t2 = np.array([[[0.0, 4.0, 1.0, INF, 2.0, 2.0, 0.0]]])
    want = [[1, bits(1.0).item(), 1], [1, bits(4.0).item(), 1], [2, bits(2.0).item(), 2], [2, bits(INF).item(), 1]]
    assert table_of(rows, t2).tolist() == want and table_of(rows * 0, t2).shape == (0, 3)


def _table(*entries):
    return np.array([[r, bits(v).item(), n] for r, v, n in entries], np.int64).reshape(-1, 3)


def test_local_thickness_columns():
    from skoots_amd.validate.compare import LOCAL_THICKNESS_COLUMNS, local_thickness_columns
    assert LOCAL_THICKNESS_COLUMNS == "local_radius_mean,local_radius_std,local_radius_min"
    # row 1: a single value; row 2: inf; row 3: empty; row 4: two values; row 5: a value whose mean needs the clamp
    third = 0.1369
    table = _table((1, 2.0, 7), (2, INF, 5), (4, 1.0, 3), (4, 9.0, 1), (5, third, 3))
    col = local_thickness_columns(table, 5)
    assert list(col) == LOCAL_THICKNESS_COLUMNS.split(",")
    assert all(v.dtype == torch.float64 and not v.is_cuda and tuple(v.shape) == (5,) for v in col.values())
    r = float(np.sqrt(np.float64(third)))
    assert col["local_radius_min"].tolist() == [float(np.sqrt(2.0)), INF, 0.0, 1.0, r]
    mean4 = (3 * 1.0 + 1 * 3.0) / 4
    std4 = float(np.sqrt(np.float64((3 * (1.0 - mean4) ** 2 + 1 * (3.0 - mean4) ** 2) / 4)))
    assert col["local_radius_mean"].tolist() == [float(np.sqrt(2.0)), INF, 0.0, mean4, r]
    assert col["local_radius_std"].tolist() == [0.0, 0.0, 0.0, std4, 0.0]
    # the clamp: the rounded mean of equal values can fall a unit outside them; find such a value and count
    found = None
    for k in range(1, 4000):
        v = float(np.sqrt(np.float64(k * 0.1369)))
        for n in (3, 5, 6, 7, 10):
            if (0.0 + n * v) / n != v:
                found = (k * 0.1369, n, v)
                break
        if found:
            break
    assert found is not None, "no value whose plain mean leaves [min, max]: the clamp is untested"
    col = local_thickness_columns(_table((1, found[0], found[1])), 1)
    assert col["local_radius_mean"].tolist() == [found[2]] and col["local_radius_std"].tolist() == [0.0]
    # sorted by row, then value; tensors and arrays alike; N = 0
    assert all(torch.equal(a, b) for a, b in zip(local_thickness_columns(torch.from_numpy(table), 5).values(),
                                                 local_thickness_columns(table, 5).values()))
    assert local_thickness_columns(np.zeros((0, 3), np.int64), 0)["local_radius_min"].shape == (0,)


def test_format_csv_columns():
    from skoots_amd.validate.compare import format_csv
    ids, sums, boxes, graph, max_d2, radius = _measured()
    shape, spacing = (8, 8, 8), (0.5, 0.7, 3.0)
    plain = format_csv("m.tif", ids, sums, boxes, shape, spacing)
    assert plain.startswith(PLAIN) and len(plain.splitlines()) == 5
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, thickness_table=None) == plain
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, 1, None, None, None, None, None, False, None, None) == plain
    table = _table((1, 1.0, 3), (1, 4.0, 1), (2, INF, 1))
    old = plain.splitlines()
    new = format_csv("m.tif", ids, sums, boxes, shape, spacing, thickness_table=table).splitlines()
    assert new[:2] == old[:2] and new[2] == old[2] + ",local_radius_mean,local_radius_std,local_radius_min"
    std = float(np.sqrt(np.float64((3 * 0.25 ** 2 + 0.75 ** 2) / 4)))
    assert new[3] == old[3] + f",1.25,{std!r},1.0" and new[4] == old[4] + ",inf,0.0,inf"
    # behind everything else
    pieces = torch.tensor([[3, 4, 0, 0, 0, 0], [70000, 1, 0, 0, 0, 0]])
    with_all = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph, max_dist2=max_d2,
                          skeleton_radius=radius, piece_table=pieces).splitlines()
    both = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph, max_dist2=max_d2,
                      skeleton_radius=radius, piece_table=pieces, thickness_table=table).splitlines()
    assert both[2] == with_all[2] + ",local_radius_mean,local_radius_std,local_radius_min"
    assert both[3] == with_all[3] + f",1.25,{std!r},1.0" and both[4] == with_all[4] + ",inf,0.0,inf"
    assert len(format_csv("m.tif", ids, sums, boxes, shape, spacing, 2, thickness_table=table).splitlines()) == 4


def test_cli_flags():
    from skoots_amd.validate.compare import parse_args
    a = parse_args(["m.tif"])
    assert a.local_thickness is None and a.save_thickness is False and a.thickness is None
    a = parse_args(["m.tif", "--local-thickness", "closed"])
    assert a.local_thickness == "closed" and a.save_thickness is False and a.thickness is None
    a = parse_args(["m.tif", "--save-thickness"])
    assert a.local_thickness == "open" and a.save_thickness is True and a.thickness is None   # implies open
    assert a.save_distance is False
    a = parse_args(["m.tif", "--save-thickness", "--local-thickness", "closed"])
    assert a.local_thickness == "closed" and a.save_thickness is True
    for bad in (["--local-thickness"], ["--local-thickness", "yes"], ["--save-thickness", "1"],
                ["--local-thickness", "open", "closed"]):
        with pytest.raises(SystemExit) as e:
            parse_args(["m.tif"] + bad)
        assert e.value.code == 2
    # --thickness and --save-distance behave as before, alone and next to the new switches
    a = parse_args(["m.tif", "--thickness", "closed", "--skeleton"])
    assert a.thickness == "closed" and a.save_distance is False and a.skeleton is True and a.local_thickness is None
    a = parse_args(["m.tif", "--save-distance"])
    assert a.thickness == "open" and a.save_distance is True and a.local_thickness is None and a.save_thickness is False
    a = parse_args(["m.tif", "--save-distance", "--local-thickness", "closed"])
    assert a.thickness == "open" and a.local_thickness == "closed"
    for bad in (["--thickness"], ["--thickness", "yes"]):
        with pytest.raises(SystemExit) as e:
            parse_args(["m.tif"] + bad)
        assert e.value.code == 2


def test_stats_per_instance_refuses_a_bad_mode_before_touching_the_device():
    from skoots_amd.validate.compare import stats_per_instance
    with pytest.raises(ValueError, match="local_thickness"):
        stats_per_instance(torch.zeros((2, 2, 2), dtype=torch.int32), local_thickness="yes")
