"""The skeleton graph on the CPU (no GPU needed): the numpy statement of ``sk_skeleton_graph`` checked on shapes whose
answer is known in closed form and on the anchors of tests/golden/skeleton_graph.npz (scikit-image 0.18.3), the host
columns of ``validate.compare.skeleton_columns``, the CSV text and the command's flags.

tests/test_hip_skeleton_graph.py takes the oracle and the golden skeletons from here."""
import math
import os

import numpy as np
import pytest
import torch

from tests.skeleton_graph_cases import (LINE_IDS, LINE_VOXELS, LINK_CLASSES, PAIR_IDS, RING_ID, T_ID, cases, line,
                                        positive_ids)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skeleton_graph.npz")
N_GRAPH = 12
THIN_AWAY = [29410, 42334, 50645, 85386, 98047, 98063]     # of "blobs (24, 40, 70)", under scikit-image 0.18.3
SPACINGS = ((1.0, 1.0, 1.0), (0.5, 0.7, 3.0))


def skeleton_graph_oracle(skel_labels):
    """(labels (N) int64 ascending, graph (N, 12) int64) of the positive labels of a skeleton label volume: what
    ``sk_skeleton_graph`` counts, stated with shifted comparisons.  Pad by one voxel; a voxel's degree is the number
    of its 26 neighbours with its own label; a link is counted from the voxel that has it among its 13
    raster-following neighbours and binned by (|dx|, |dy|, |dz|)."""
    lab = np.asarray(skel_labels)
    ids = positive_ids(lab)
    row = np.searchsorted(ids, lab.clip(min=0)) * (lab > 0)          # 0-based row where lab > 0
    X, Y, Z = lab.shape
    p = np.pad(lab, 1)
    fg = lab > 0
    degree = np.zeros(lab.shape, np.int64)
    graph = np.zeros((len(ids), N_GRAPH), np.int64)
    offsets = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    for k, (a, b, c) in enumerate(offsets):
        if k == 13:
            continue
        same = fg & (p[1 + a:1 + a + X, 1 + b:1 + b + Y, 1 + c:1 + c + Z] == lab)
        degree += same
        if k > 13:                                                   # the 13 raster-following neighbours
            cls = LINK_CLASSES.index((abs(a), abs(b), abs(c)))
            graph[:, 5 + cls] += np.bincount(row[same], minlength=len(ids))
    graph[:, 0] = np.bincount(row[fg], minlength=len(ids))
    for col, pick in ((1, degree == 0), (2, degree == 1), (3, degree == 2), (4, degree >= 3)):
        graph[:, col] = np.bincount(row[fg & pick], minlength=len(ids))
    graph_degree_sum = np.bincount(row[fg], weights=degree[fg], minlength=len(ids)).astype(np.int64)
    assert np.array_equal(graph_degree_sum, 2 * graph[:, 5:].sum(1))  # every link has two ends
    return ids, graph


_golden = {}


def golden_rows(name):
    """the golden skeleton of a case: (X, Y, Z) int32, 0 or the row (1 .. N) of the instance, read-only"""
    if not _golden:
        g = np.load(GOLDEN)
        pos = 0
        for n, shape in zip(g["names"].tolist(), g["shapes"].tolist()):
            size = int(np.prod(shape))
            _golden[n] = g["rows"][pos:pos + size].reshape(shape)
            _golden[n].setflags(write=False)
            pos += size
    return _golden[name]


_want = {}


def want_graph(name, lab):
    """(ids (N) int64, graph (N, 12) int64) a case must give: the oracle on its golden skeleton, with a row of zeros
    for every instance that thinned away; computed once per case"""
    if name not in _want:
        ids = positive_ids(lab)
        rows, g = skeleton_graph_oracle(golden_rows(name))
        graph = np.zeros((len(ids), N_GRAPH), np.int64)
        graph[rows - 1] = g
        _want[name] = (ids, graph)
    return _want[name]


def test_the_golden_file_covers_the_cases():
    vols = cases()
    g = np.load(GOLDEN)
    assert g["names"].tolist() == list(vols) and g["rows"].dtype == np.int32
    assert os.path.getsize(GOLDEN) < 64 * 1024
    for name, lab in vols.items():
        r = golden_rows(name)
        ids = positive_ids(lab)
        assert r.shape == lab.shape and r.max() <= len(ids)
        assert not ((r > 0) & (lab != np.concatenate(([0], ids))[r])).any()      # a skeleton lies in its instance


def test_oracle_on_lines_of_every_class():
    lab = cases()["lines"]
    ids, graph = skeleton_graph_oracle(lab)                          # a one-voxel line is its own skeleton
    assert ids.tolist() == list(LINE_IDS) + list(PAIR_IDS)
    for k, obj in enumerate(LINE_IDS):
        links = [0] * 7
        links[k] = LINE_VOXELS - 1
        assert graph[k].tolist() == [LINE_VOXELS, 0, 2, LINE_VOXELS - 2, 0] + links, obj
    for k in (7, 8):                                                 # no link crosses ids
        assert graph[k].tolist() == [9, 0, 2, 7, 0, 0, 0, 0, 0, 8, 0, 0]
    both = np.where(lab >= PAIR_IDS[0], 1, 0)                        # as one object the pair is a ladder
    assert skeleton_graph_oracle(both)[1][0, 5:].sum() > 16


def test_oracle_on_hand_built_ring_corner_and_dots():
    lab = np.zeros((8, 8, 40), np.int32)
    for y, z in [(1, 30), (1, 31), (1, 32), (2, 33), (3, 33), (4, 32), (4, 31), (4, 30), (3, 29), (2, 29)]:
        lab[2, y, z] = 5                                             # a ring of ten chain voxels across z = 31 | 32
    lab[5, 1, 1] = lab[5, 2, 1] = lab[5, 1, 2] = 6                   # a corner triangle: three links, all counted
    lab[7, 7, 39] = lab[0, 0, 0] = lab[7, 0, 5] = 9                  # three isolated voxels of one id
    ids, graph = skeleton_graph_oracle(lab)
    assert ids.tolist() == [5, 6, 9]
    assert graph[0].tolist() == [10, 0, 0, 10, 0, 0, 2, 4, 0, 0, 4, 0]
    assert graph[1].tolist() == [3, 0, 0, 3, 0, 0, 1, 1, 0, 0, 1, 0]
    assert graph[2].tolist() == [3, 3, 0, 0, 0] + [0] * 7
    assert skeleton_graph_oracle(np.zeros((3, 3, 3), np.int32))[1].shape == (0, N_GRAPH)


def test_anchors_of_the_golden_skeletons():
    vols = cases()
    name = "blobs (24, 40, 70)"
    ids, graph = want_graph(name, vols[name])
    ids = ids.tolist()
    ring, tee = graph[ids.index(RING_ID)], graph[ids.index(T_ID)]
    assert ring[:5].tolist() == [60, 0, 0, 60, 0] and ring[5:].sum() == 60
    assert tee[0] == 32 and tee[2] == 3 and tee[4] == 1 and tee[5:].sum() - tee[3] == 3
    assert [u for u, g in zip(ids, graph) if g[0] == 0] == THIN_AWAY
    assert sum(1 for g in graph if g[0] == 1 and g[1] == 1) == 3     # a single voxel of degree 0
    assert max(ids) > 65535 and len(ids) == 32
    # the lines are their own skeletons, also under scikit-image
    assert np.array_equal(golden_rows("lines") > 0, vols["lines"] > 0)
    assert np.array_equal(want_graph("lines", vols["lines"])[1], skeleton_graph_oracle(vols["lines"])[1])
    # one label filling the volume thins to something; two corner voxels stay
    assert want_graph("one label (8, 9, 10)", vols["one label (8, 9, 10)"])[1][0, 0] > 0
    assert want_graph("corners (5, 6, 34)", vols["corners (5, 6, 34)"])[1][:, :2].tolist() == [[1, 1], [1, 1]]
    assert want_graph("huge int64 (4, 5, 36)", vols["huge int64 (4, 5, 36)"])[0].tolist() == [70000, 2 ** 30, 2 ** 40]


def test_degree_identity_on_every_row():
    """col2 + 2 col3 + (degree sum of the junction voxels) = 2 links; the junction sum is at least 3 col4"""
    for name, lab in cases().items():
        _, graph = want_graph(name, lab)
        links = graph[:, 5:].sum(1)
        junction_degrees = 2 * links - graph[:, 2] - 2 * graph[:, 3]
        assert (junction_degrees >= 3 * graph[:, 4]).all() and (junction_degrees <= 26 * graph[:, 4]).all(), name
        assert np.array_equal(graph[:, 1:5].sum(1), graph[:, 0]), name


def test_lee_thinning_restated_gives_the_golden_lines():
    from tests.test_skeletonize import thin
    lab = cases()["lines"]
    rows = golden_rows("lines")
    for r, obj in enumerate(positive_ids(lab).tolist()):
        assert np.array_equal(thin(lab == obj), rows == r + 1), obj


def test_skeleton_columns():
    from skoots_amd.validate.compare import skeleton_columns
    vols = cases()
    name = "blobs (24, 40, 70)"
    ids, graph = want_graph(name, vols[name])
    g = np.concatenate([graph, want_graph("lines", vols["lines"])[1], np.zeros((2, N_GRAPH), np.int64)])
    for spacing in SPACINGS:
        col = skeleton_columns(torch.from_numpy(g), spacing)
        assert col["skeleton_length"].dtype == torch.float64
        assert all(col[k].dtype == torch.int64 for k in col if k != "skeleton_length")
        assert col["skeleton_voxels"].tolist() == g[:, 0].tolist()
        assert col["skeleton_endpoints"].tolist() == g[:, 2].tolist()
        assert col["skeleton_junctions"].tolist() == g[:, 4].tolist()
        assert col["skeleton_links"].tolist() == g[:, 5:].sum(1).tolist()
        assert col["skeleton_branches"].tolist() == (g[:, 5:].sum(1) - g[:, 3]).tolist()
        step = [math.sqrt(sum((d * s) ** 2 for d, s in zip(c, spacing))) for c in LINK_CLASSES]
        for row, got in zip(g.tolist(), col["skeleton_length"].tolist()):
            want = math.fsum(n * s for n, s in zip(row[5:], step))
            assert not math.isnan(got) and abs(got - want) <= 1e-12 * want
        assert col["skeleton_length"][-2:].tolist() == [0.0, 0.0] and col["skeleton_branches"][-1].item() == 0
    i = ids.tolist()
    col = skeleton_columns(torch.from_numpy(graph))
    assert col["skeleton_branches"][i.index(RING_ID)].item() == 0 and col["skeleton_branches"][i.index(T_ID)].item() == 3
    lines = skeleton_columns(torch.from_numpy(want_graph("lines", vols["lines"])[1]), (0.5, 0.7, 3.0))
    assert lines["skeleton_branches"].tolist() == [1] * 9            # a rod is one branch
    assert lines["skeleton_length"][2].item() == 8 * 3.0 and lines["skeleton_length"][0].item() == 8 * 0.5
    assert skeleton_columns(torch.zeros((0, N_GRAPH), dtype=torch.int64))["skeleton_length"].shape == (0,)
    with pytest.raises(ValueError):
        skeleton_columns(torch.from_numpy(graph), (1.0, 0.0, 1.0))


def _measured():
    """ids, sums, boxes (host tensors, made by hand) of two instances, and a graph for them"""
    ids = torch.tensor([3, 70000])
    sums = torch.tensor([[4, 6, 4, 4, 14, 4, 4, 6, 6, 4, 2, 8, 8], [1, 5, 5, 5, 25, 25, 25, 25, 25, 25, 2, 2, 2]])
    boxes = torch.tensor([[0, 1, 1, 3, 1, 1], [5, 5, 5, 5, 5, 5]], dtype=torch.int32)
    graph = torch.tensor([[4, 0, 2, 2, 0, 3, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]])
    return ids, sums, boxes, graph


def test_format_csv_columns():
    from skoots_amd.validate.compare import format_csv
    ids, sums, boxes, graph = _measured()
    shape, spacing = (8, 8, 8), (0.5, 0.7, 3.0)
    plain = format_csv("m.tif", ids, sums, boxes, shape, spacing)
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=None) == plain
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, 1, None, None) == plain
    with_s = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph).splitlines()
    old = plain.splitlines()
    new = "skeleton_voxels,skeleton_length,skeleton_endpoints,skeleton_junctions,skeleton_branches"
    assert with_s[:2] == old[:2] and with_s[2] == old[2] + "," + new
    assert [ln.split(",")[:17] for ln in with_s[3:]] == [ln.split(",") for ln in old[3:]]
    assert with_s[3].split(",")[17:] == ["4", "1.5", "2", "0", "1"]
    assert with_s[4].split(",")[17:] == ["1", "0.0", "0", "0", "0"]
    # after the surface columns when both are asked for
    cells = torch.zeros((2, 30), dtype=torch.int64)
    cells[:, 1] = 8
    both = format_csv("m.tif", ids, sums, boxes, shape, spacing, mesh_cells=cells, skeleton_graph=graph).splitlines()
    surface = format_csv("m.tif", ids, sums, boxes, shape, spacing, mesh_cells=cells).splitlines()
    assert both[2] == old[2] + ",surface_area,surface_to_volume," + new
    assert [ln.split(",")[:19] for ln in both[3:]] == [ln.split(",") for ln in surface[3:]]
    assert [ln.split(",")[19:] for ln in both[3:]] == [ln.split(",")[17:] for ln in with_s[3:]]
    # min_voxels leaves rows out of every column alike
    assert len(format_csv("m.tif", ids, sums, boxes, shape, spacing, 2, skeleton_graph=graph).splitlines()) == 4


def test_cli_flags():
    from skoots_amd.validate.compare import parse_args
    a = parse_args(["m.tif"])
    assert a.skeleton is False and a.save_skeletons is False
    a = parse_args(["m.tif", "--skeleton", "--surface-area", "open"])
    assert a.skeleton is True and a.save_skeletons is False and a.surface_area == "open"
    a = parse_args(["m.tif", "--save-skeletons"])
    assert a.skeleton is True and a.save_skeletons is True           # --save-skeletons implies --skeleton
    with pytest.raises(SystemExit) as e:
        parse_args(["m.tif", "--skeleton", "yes"])
    assert e.value.code == 2
