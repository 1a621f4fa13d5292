"""The labelled Euclidean distance transform on the CPU (no GPU needed): the three numpy statements of the definition in
tests/edt_cases.py held against each other bit for bit and against scipy, the host columns of
``validate.compare.thickness_columns``, the CSV text, the command's flags and ``lib.tiff.write_float_stack`` on the host.

tests/test_hip_edt.py compares the device with the same oracle."""
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.edt_cases import (BALL, INF, INTEGER_SPACINGS, MODES, SPACINGS, brute_force, cases, expected, row_max,
                             rows_of, walk, weights)

CASES = cases()
SAMPLE = 200          # voxels per (case, spacing, mode) the pairwise brute force takes on the volumes it cannot take whole
WHOLE = 3000          # voxels up to which it takes every voxel


def test_the_cases_are_small_and_cover_the_shapes():
    assert all(lab.size <= 2e5 for lab in CASES.values())
    shapes = [lab.shape for lab in CASES.values()]
    assert all(any(s[k] == 1 for s in shapes) for k in range(3))           # an extent of 1 in every axis
    assert (1, 17, 9) in shapes and (13, 1, 1) in shapes and (40, 40, 70) in shapes
    assert max(int(lab.max()) for lab in CASES.values()) == 2 ** 40
    one = CASES["one label (8, 9, 10)"]
    assert (one == one.flat[0]).all() and one.flat[0] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_walk_equals_the_oracle_and_the_brute_force_bit_for_bit(name):
    """the pruned three-pass walk, the line-first minimum and the pairwise minimum are one function"""
    lab = CASES[name]
    rng = np.random.default_rng(5)
    for spacing in SPACINGS:
        for closed in MODES:
            ids, rows, want = expected(name, spacing, closed)
            w = weights(spacing)
            got = walk(rows, w, closed)
            assert got.dtype == np.float64 and np.array_equal(got, want), (name, spacing, closed)
            assert not np.isnan(want).any() and (want[rows == 0] == 0).all() and (want[rows > 0] > 0).all()
            pts = np.argwhere(rows > 0)
            if lab.size > WHOLE:
                pts = pts[rng.choice(len(pts), min(SAMPLE, len(pts)), replace=False)]
            assert np.array_equal(brute_force(rows, w, closed, pts), want[tuple(pts.T)]), (name, spacing, closed)


def _scipy(rows, r, spacing, closed):
    m = rows == r
    if closed:
        return ndimage.distance_transform_edt(np.pad(m, 1), sampling=spacing)[1:-1, 1:-1, 1:-1]
    return ndimage.distance_transform_edt(m, sampling=spacing)


@pytest.mark.parametrize("name", list(CASES))
def test_sqrt_of_the_oracle_is_scipy_at_integer_spacings(name):
    checked = 0
    for spacing in INTEGER_SPACINGS:
        for closed in MODES:
            ids, rows, want = expected(name, spacing, closed)
            for r in range(1, len(ids) + 1):
                m = rows == r
                if not closed and m.all():                    # no other voxel: scipy has no answer, the oracle has inf
                    assert (want == INF).all()
                    continue
                assert np.array_equal(np.sqrt(want[m]), _scipy(rows, r, spacing, closed)[m]), (name, spacing, closed, r)
                checked += 1
    assert checked or name.startswith("one label")


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_agrees_with_scipy_at_a_non_integer_spacing(name):
    """1e-14 relative: both sides make at most about 6.5 double roundings of relative error between them (1.4e-15);
    2e-16 was measured.  Only this comparison has a tolerance."""
    spacing = SPACINGS[3]
    assert spacing == (0.37, 0.41, 1.3)
    for closed in MODES:
        ids, rows, want = expected(name, spacing, closed)
        for r in range(1, len(ids) + 1):
            m = rows == r
            if not closed and m.all():
                assert (want == INF).all()
                continue
            ref = _scipy(rows, r, spacing, closed)[m]
            assert (np.abs(np.sqrt(want[m]) - ref) <= 1e-14 * ref).all(), (name, closed, r)


def test_known_values():
    # a sheet one voxel thick has a radius of one spacing; a slab k voxels across (k + 1) / 2 spacings, rounded down
    lab = np.zeros((7, 9, 11), np.int32)
    lab[3] = 1
    lab[:, :, 0] = 0
    ids, rows = rows_of(lab)
    assert walk(rows, weights((2.0, 1.0, 5.0)), False).max() == 4.0
    lab[2:5] = 1                                              # three voxels across x
    lab[:, :, 0] = 0
    assert walk(rows_of(lab)[1], weights((2.0, 1.0, 5.0)), False).max() == 16.0
    # the ball |v|^2 <= 144: the nearest outside voxel of its centre is (12, 1, 0), 145 = 12^2 + 1^2
    for closed in MODES:
        assert expected(BALL, (1, 1, 1), closed)[2][20, 20, 56] == 145.0
    assert expected(BALL, (2, 1, 5), False)[2][20, 20, 56] == 148.0      # (1, 12, 0): 4 + 144; x and z cost more
    # the shared plane bounds both ids, and closed mode adds the volume's faces
    ids, rows, d2 = expected("shared plane (6, 7, 8)", (1, 1, 1), False)
    assert d2[0, 0, 0] == 9.0 and d2[2, 3, 3] == 1.0 and d2[3, 3, 3] == 1.0 and d2[5, 6, 7] == 9.0
    d2 = expected("shared plane (6, 7, 8)", (1, 1, 1), True)[2]
    assert d2[0, 0, 0] == 1.0 and d2[2, 3, 3] == 1.0 and d2[1, 3, 3] == 4.0
    # the slab through the whole x extent gets nothing from x in open mode and the faces in closed mode
    assert expected("slab (9, 12, 10)", (0.37, 0.41, 1.3), False)[2][0, 5, 4] == min(weights((0.37, 0.41, 1.3))[1] * 9.0,
                                                                                    weights((0.37, 0.41, 1.3))[2] * 9.0)
    assert expected("slab (9, 12, 10)", (0.37, 0.41, 1.3), True)[2][0, 5, 4] == weights((0.37, 0.41, 1.3))[0]
    # beside the slot of the U the nearest outside voxel lies across x
    assert expected("U (12, 16, 30)", (1, 1, 3), False)[2][4, 8, 20] == 1.0
    # one label alone in the volume
    assert (expected("one label (8, 9, 10)", (1, 1, 1), False)[2] == INF).all()
    assert expected("one label (8, 9, 10)", (1, 1, 1), True)[2].max() == 16.0
    assert row_max(*expected("one label (8, 9, 10)", (1, 1, 1), False)[1:]).tolist() == [INF]


def test_w_times_d_squared_is_not_w_d_times_d():
    """the definition multiplies the weight by the exact square; the other grouping differs in the last bit"""
    w = weights((0.37, 0.41, 1.3))
    assert any(wk * (d * d) != (wk * d) * d for wk in w for d in (3.0, 5.0, 7.0, 11.0, 13.0))


def test_thickness_columns():
    from skoots_amd.validate.compare import SKELETON_RADIUS_COLUMNS, THICKNESS_COLUMNS, thickness_columns
    assert THICKNESS_COLUMNS == "inscribed_radius"
    assert SKELETON_RADIUS_COLUMNS == "skeleton_radius_mean,skeleton_radius_min,skeleton_radius_max"
    max_d2 = torch.tensor([169.0, 0.1369, INF, 2.0], dtype=torch.float64)
    col = thickness_columns(max_d2)
    assert list(col) == ["inscribed_radius"] and col["inscribed_radius"].dtype == torch.float64
    assert col["inscribed_radius"].tolist() == [13.0, math.sqrt(0.1369), INF, math.sqrt(2.0)]
    st = torch.tensor([[1.5, 1.0, 2.0], [0.0, 0.0, 0.0], [INF, INF, INF], [1.0, 1.0, 1.0]], dtype=torch.float64)
    col = thickness_columns(max_d2, st)
    assert list(col) == ["inscribed_radius"] + SKELETON_RADIUS_COLUMNS.split(",")
    assert col["skeleton_radius_mean"].tolist() == [1.5, 0.0, INF, 1.0]
    assert col["skeleton_radius_min"].tolist() == [1.0, 0.0, INF, 1.0]
    assert col["skeleton_radius_max"].tolist() == [2.0, 0.0, INF, 1.0]
    assert thickness_columns(torch.zeros(0, dtype=torch.float64))["inscribed_radius"].shape == (0,)


def _measured():
    """ids, sums, boxes (host tensors, made by hand) of two instances, a graph, and width results for them"""
    ids = torch.tensor([3, 70000])
    sums = torch.tensor([[4, 6, 4, 4, 14, 4, 4, 6, 6, 4, 2, 8, 8], [1, 5, 5, 5, 25, 25, 25, 25, 25, 25, 2, 2, 2]])
    boxes = torch.tensor([[0, 1, 1, 3, 1, 1], [5, 5, 5, 5, 5, 5]], dtype=torch.int32)
    graph = torch.tensor([[4, 0, 2, 2, 0, 3, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]])
    max_d2 = torch.tensor([0.1369, INF], dtype=torch.float64)
    radius = torch.tensor([[0.37, 0.25, 0.5], [0.0, 0.0, 0.0]], dtype=torch.float64)
    return ids, sums, boxes, graph, max_d2, radius


# what format_csv returns for _measured() without the new arguments, as it did before they existed
PLAIN = ("Mask File: m.tif\n"
         "Spacing: 0.5 0.7 3.0\n"
         "id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,axis_minor\n")


def test_format_csv_columns():
    from skoots_amd.validate.compare import format_csv
    ids, sums, boxes, graph, max_d2, radius = _measured()
    shape, spacing = (8, 8, 8), (0.5, 0.7, 3.0)
    plain = format_csv("m.tif", ids, sums, boxes, shape, spacing)
    assert plain.startswith(PLAIN) and len(plain.splitlines()) == 5
    assert [len(ln.split(",")) for ln in plain.splitlines()[2:]] == [17, 17, 17]
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, max_dist2=None, skeleton_radius=None) == plain
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, 1, None, None, None, None) == plain
    old = plain.splitlines()
    width = format_csv("m.tif", ids, sums, boxes, shape, spacing, max_dist2=max_d2).splitlines()
    assert width[:2] == old[:2] and width[2] == old[2] + ",inscribed_radius"
    assert width[3] == old[3] + "," + repr(math.sqrt(0.1369)) and width[4] == old[4] + ",inf"
    with_s = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph).splitlines()
    both = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph, max_dist2=max_d2,
                      skeleton_radius=radius).splitlines()
    assert both[2] == with_s[2] + ",inscribed_radius,skeleton_radius_mean,skeleton_radius_min,skeleton_radius_max"
    assert both[3] == with_s[3] + "," + repr(math.sqrt(0.1369)) + ",0.37,0.25,0.5"
    assert both[4] == with_s[4] + ",inf,0.0,0.0,0.0"
    assert len(format_csv("m.tif", ids, sums, boxes, shape, spacing, 2, max_dist2=max_d2).splitlines()) == 4
    with pytest.raises(ValueError):
        format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_radius=radius)


def test_cli_flags():
    from skoots_amd.validate.compare import parse_args
    a = parse_args(["m.tif"])
    assert a.thickness is None and a.save_distance is False
    a = parse_args(["m.tif", "--thickness", "closed", "--skeleton"])
    assert a.thickness == "closed" and a.save_distance is False and a.skeleton is True
    a = parse_args(["m.tif", "--save-distance"])
    assert a.thickness == "open" and a.save_distance is True and a.skeleton is False     # implies --thickness open
    a = parse_args(["m.tif", "--save-distance", "--thickness", "closed"])
    assert a.thickness == "closed" and a.save_distance is True
    for bad in (["--thickness"], ["--thickness", "yes"], ["--save-distance", "1"]):
        with pytest.raises(SystemExit) as e:
            parse_args(["m.tif"] + bad)
        assert e.value.code == 2


def read_float_tiff(path):
    """(Z, H, W) float32 of a stack ``write_float_stack`` wrote, by parsing the directories with struct and inflating
    the strips with zlib; asserts the tags a reader of 32-bit float pages goes by"""
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


def test_write_float_stack_on_the_host(tmp_path):
    from skoots_amd.lib import tiff
    rng = np.random.default_rng(3)
    pages = rng.standard_normal((3, 5, 7)).astype(np.float32)
    pages[0, 0, :3] = (0.0, INF, 1e-30)
    for k, src in enumerate((pages, torch.from_numpy(pages), torch.from_numpy(pages).permute(0, 2, 1))):
        path = os.path.join(tmp_path, f"f{k}.tif")
        tiff.write_float_stack(path, src)
        got = read_float_tiff(path)
        want = pages if k < 2 else pages.transpose(0, 2, 1)
        assert got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(want).tobytes()
        assert tiff.scan(path) is None                                  # the integer readers leave such a file alone
    for bad in (pages.astype(np.float64), pages[0], np.zeros((2, 2, 2), np.int32), torch.zeros((2, 2, 2), dtype=torch.float16)):
        with pytest.raises(ValueError):
            tiff.write_float_stack(os.path.join(tmp_path, "bad.tif"), bad)
    with pytest.raises(ValueError):                                     # write_stack still refuses float32
        tiff.write_stack(os.path.join(tmp_path, "bad.tif"), pages)
    with pytest.raises(ValueError):
        tiff.write_stack(os.path.join(tmp_path, "bad.tif"), torch.from_numpy(pages))
    assert not os.path.exists(os.path.join(tmp_path, "bad.tif"))
