"""Host side of the marching-cubes surface area: the class table
(skoots_amd/validate/mc_table.py), ``class_areas`` and the CSV text, without a GPU.  ``mesh_cells_oracle`` below is the
numpy statement of what ``sk_instance_mesh_cells`` counts; tests/test_hip_surface_area.py and
tools/instance_mesh_host_check.py compare the kernel with it, and here it is compared with the reference's own areas
(tests/golden/surface_area.npz, made by scikit-image's marching cubes through the reference's ``get_surface_area``)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from skoots_amd.validate import compare as CMP
from skoots_amd.validate.mc_table import CLASS_OF, CLASS_TRIANGLES, NO_CLASS, TRIANGLE_TYPES

N_CLASSES = len(CLASS_TRIANGLES)

# Largest relative deviation of the float64 oracle from the fixture, measured over every input, id and mode:
#   unit spacing       1.355e-07  scikit-image keeps float32 vertices and sums the triangle areas in float32 there
#   the other spacings 3.417e-16  float64 throughout; what is left is the order of the summation
# The bounds are 10 x the measured values: room for another scikit-image build's summation order.
MEASURED_UNIT, MEASURED_OTHER = 1.355e-07, 3.417e-16
RTOL_UNIT, RTOL_OTHER = 10 * MEASURED_UNIT, 10 * MEASURED_OTHER


def rtol_for(spacing):
    return RTOL_UNIT if tuple(float(v) for v in spacing) == (1.0, 1.0, 1.0) else RTOL_OTHER


def config_volume(m):
    """(X - 1, Y - 1, Z - 1) uint8 configurations of a boolean (X, Y, Z) array: bit b of cell (x, y, z) is the corner
    (x + (b & 1), y + ((b >> 1) & 1), z + ((b >> 2) & 1))"""
    X, Y, Z = m.shape
    cfg = np.zeros((X - 1, Y - 1, Z - 1), np.uint8)
    for b in range(8):
        dx, dy, dz = b & 1, (b >> 1) & 1, (b >> 2) & 1
        cfg |= m[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.uint8) << b
    return cfg


def mesh_cells_oracle(lab, closed):
    """(ids, cells (N, 30) int64) of an (X, Y, Z) integer array: per positive id the configuration volume of
    ``lab == id`` (padded with one layer of background when ``closed``), then CLASS_OF, then bincount.  Only the box of
    the id, grown by one voxel, is looked at: no other cell can hold a corner of it."""
    lab = np.asarray(lab).astype(np.int64)
    if closed:
        lab = np.pad(lab, 1)
    ids = np.unique(lab)
    ids = ids[ids > 0]
    class_of = np.array(CLASS_OF, np.int64)
    cells = np.zeros((len(ids), N_CLASSES), np.int64)
    if len(ids) == 0 or min(lab.shape) < 2:
        return ids, cells
    order = np.argsort(lab, axis=None, kind="stable")
    flat = lab.ravel()[order]
    coords = np.stack(np.unravel_index(order, lab.shape), 1)
    starts, ends = np.searchsorted(flat, ids, "left"), np.searchsorted(flat, ids, "right")
    for i, (u, s, e) in enumerate(zip(ids, starts, ends)):
        lo = np.maximum(coords[s:e].min(0) - 1, 0)
        hi = np.minimum(coords[s:e].max(0) + 2, lab.shape)
        crop = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == u
        if min(crop.shape) < 2:
            continue
        cls = class_of[config_volume(crop)]
        cells[i] = np.bincount(cls[cls != NO_CLASS], minlength=N_CLASSES)
    return ids, cells


def oracle_area(lab, closed, spacing):
    ids, cells = mesh_cells_oracle(lab, closed)
    return ids, cells.astype(np.float64) @ CMP.class_areas(spacing).numpy()


def fixture_cases(g):
    """(name, mask (X, Y, Z), ids, area (ids, spacings, 2)) of tests/golden/surface_area.npz"""
    inst = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_stats.npz"))
    for name in g["names"].tolist():
        mask = inst["mask"][0] if name == "instance_stats" else g[name + "_mask"]
        yield name, mask, g[name + "_ids"], g[name + "_area"]


def test_oracle_matches_the_reference(golden):
    g = golden("surface_area.npz")
    spacings = g["spacings"]
    assert [tuple(s) for s in spacings.tolist()] == [(1.0, 1.0, 1.0), (1.0, 1.0, 3.0), (0.5, 2.0, 3.0)]
    worst = {"unit": 0.0, "other": 0.0}
    names = []
    for name, mask, ids, area in fixture_cases(g):
        names.append(name)
        for m, closed in enumerate((False, True)):
            for s, spacing in enumerate(spacings.tolist()):
                got_ids, got = oracle_area(mask, closed, spacing)
                assert np.array_equal(got_ids, ids)
                rel = np.abs(got - area[:, s, m]) / area[:, s, m]
                key = "unit" if s == 0 else "other"
                worst[key] = max(worst[key], float(rel.max()))
                print(f"{name} closed={closed} spacing={spacing}: largest relative deviation {rel.max():.3e}")
                assert rel.max() <= rtol_for(spacing), (name, closed, spacing, rel)
    print("largest relative deviation:", worst)
    assert names == ["instance_stats", "noise", "ellipsoids"]
    ids = g["instance_stats_ids"].tolist()
    assert ids == [3, 7, 300, 1000]
    # one voxel in the corner of the volume: one corner cell when open, all eight when closed
    one = g["instance_stats_area"][ids.index(1000), 0]
    assert one[0] == pytest.approx(math.sqrt(3) / 8, rel=1e-6) and one[1] == pytest.approx(math.sqrt(3), rel=1e-6)


def test_table_invariants():
    assert len(TRIANGLE_TYPES) == 12 and len(set(TRIANGLE_TYPES)) == 12
    assert N_CLASSES == 30 and all(len(row) == 12 for row in CLASS_TRIANGLES)
    assert len(set(CLASS_TRIANGLES)) == 30
    assert all(sum(row) >= 1 and sum(row) <= 5 and min(row) >= 0 for row in CLASS_TRIANGLES)
    assert len(CLASS_OF) == 256 and CLASS_OF[0] == CLASS_OF[255] == NO_CLASS and NO_CLASS >= 32
    assert sorted(set(CLASS_OF[1:255])) == list(range(30))

    def mirrored(c, axis):
        return sum(((c >> b) & 1) << (b ^ (1 << axis)) for b in range(8))

    for axis in range(3):
        assert all(CLASS_OF[mirrored(c, axis)] == CLASS_OF[c] for c in range(256)), axis
    assert len({CLASS_OF[1 << b] for b in range(8)}) == 1
    unit = CMP.class_areas((1, 1, 1))
    assert unit.dtype == torch.float64 and tuple(unit.shape) == (30,)
    assert unit[CLASS_OF[1]].item() == math.sqrt(3) / 8
    for face in (0x0F, 0xF0, 0x33, 0xCC, 0x55, 0xAA):               # the six faces of the cube
        assert unit[CLASS_OF[face]].item() == 1.0
    # a face cell at spacing (sx, sy, sz): the face normal to z has the area sx sy
    s = CMP.class_areas((0.5, 2.0, 3.0))
    assert s[CLASS_OF[0x0F]].item() == 0.5 * 2.0 and s[CLASS_OF[0x33]].item() == 0.5 * 3.0
    assert s[CLASS_OF[0x55]].item() == 2.0 * 3.0
    with pytest.raises(ValueError):
        CMP.class_areas((1, 0, 1))


def test_class_areas_formula():
    sx, sy, sz = 0.5, 2.0, 3.0
    want = [sum(n * math.sqrt((a * sy * sz) ** 2 + (b * sx * sz) ** 2 + (c * sx * sy) ** 2) / 8
                for n, (a, b, c) in zip(row, TRIANGLE_TYPES)) for row in CLASS_TRIANGLES]
    assert np.allclose(CMP.class_areas((sx, sy, sz)).numpy(), want, rtol=4e-16, atol=0)


def test_oracle_on_a_box_and_shared_cells():
    lab = np.zeros((6, 7, 8), np.int32)
    lab[1:4, 2:6, 1:7] = 2                                            # a 3 x 4 x 6 box inside the volume
    for closed in (False, True):
        ids, a = oracle_area(lab, closed, (1, 1, 1))
        # faces (n - 1 cells per edge), 12 edges of quarter-pipe cells and 8 corners
        want = 2 * (2 * 3 + 2 * 5 + 3 * 5) + 4 * (2 + 3 + 5) * math.sqrt(2) / 2 + 8 * math.sqrt(3) / 8
        assert ids.tolist() == [2] and a[0] == pytest.approx(want, rel=1e-14)
    lab[4:6, 2:6, 1:7] = 9                                            # a neighbour across the x = 3 | 4 face
    ids, cells = mesh_cells_oracle(lab, False)
    _, alone = mesh_cells_oracle(np.where(lab == 2, 2, 0), False)
    assert ids.tolist() == [2, 9] and np.array_equal(cells[0], alone[0])   # a shared cell counts for each instance
    full = np.full((4, 5, 6), 7)
    assert mesh_cells_oracle(full, False)[1].sum() == 0
    assert oracle_area(full, True, (1, 1, 1))[1][0] == pytest.approx(
        2 * (3 * 4 + 3 * 5 + 4 * 5) + 4 * (3 + 4 + 5) * math.sqrt(2) / 2 + math.sqrt(3), rel=1e-14)


def test_csv_without_the_switch_is_unchanged():
    sums = torch.tensor([[8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 8, 8, 8]], dtype=torch.int64)
    boxes = torch.tensor([[0, 0, 0, 1, 1, 1]], dtype=torch.int32)
    text = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0))
    lines = text.splitlines()
    assert lines[2] == ("id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,"
                        "axis_minor")
    assert len(lines) == 4 and len(lines[3].split(",")) == 17
    # the row as the code wrote it before the switch existed; the axes come out of LAPACK and are compared as numbers
    assert lines[3].split(",")[:14] == "4,8,16.0,0,0,0,1,1,1,1,0.5,0.5,1.0,40.0".split(",")
    assert [float(v) for v in lines[3].split(",")[14:]] == pytest.approx(
        [4.47213595499958, 2.23606797749979, 2.23606797749979], rel=1e-13, abs=0)
    _, cells = mesh_cells_oracle(np.pad(np.full((2, 2, 2), 4), ((0, 3), (0, 3), (0, 3))), True)
    with_area = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0),
                               mesh_cells=torch.from_numpy(cells)).splitlines()
    assert with_area[:2] == lines[:2] and with_area[2] == lines[2] + ",surface_area,surface_to_volume"
    row = with_area[3].split(",")
    assert row[:17] == lines[3].split(",") and len(row) == 19
    area = CMP.mesh_area(torch.from_numpy(cells), (1.0, 1.0, 2.0))[0].item()
    by_numpy = float(cells[0].astype(np.float64) @ CMP.class_areas((1.0, 1.0, 2.0)).numpy())
    assert area == pytest.approx(by_numpy, rel=1e-15)
    assert float(row[17]) == area and float(row[18]) == area / 16.0
    assert CMP.parse_args(["m.tif"]).surface_area is None
    assert CMP.parse_args(["m.tif", "--surface-area", "closed"]).surface_area == "closed"
    with pytest.raises(SystemExit):
        CMP.parse_args(["m.tif", "--surface-area", "both"])


def test_surface_argument_is_checked():
    with pytest.raises(ValueError, match="surface"):
        CMP.stats_per_instance(torch.zeros((2, 2, 2), dtype=torch.int32), surface="both")


def test_table_regenerates():
    pytest.importorskip("skimage")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import make_mc_table
    finally:
        sys.path.pop(0)
    types, class_of, class_triangles = make_mc_table.generate()
    assert types == TRIANGLE_TYPES and class_of == CLASS_OF and class_triangles == CLASS_TRIANGLES
    with open(make_mc_table.OUT) as f:
        assert f.read() == make_mc_table.render(types, class_of, class_triangles)
