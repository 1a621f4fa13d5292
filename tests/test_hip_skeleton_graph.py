"""``sk_skeleton_graph`` (skoots_amd/csrc/skeletonize.hip) and everything on top of it -- ``lib.morphology.skeleton_graph``,
``validate.lib.instance_skeleton_graph``, ``stats_per_instance(skeleton=True)``, ``get_skeleton_length`` and
``python -m skoots_amd.validate.compare --skeleton / --save-skeletons`` -- against the golden skeletons of scikit-image
0.18.3 (tests/golden/skeleton_graph.npz) and the numpy oracle of tests/test_skeleton_graph_cpu.py on them.  Every
output of the kernels is an integer, so every comparison of it is exact equality.

The shapes (tests/skeleton_graph_cases.py) have rows of one, two and three 32-voxel words, extents of 1 in every axis,
objects in the LDS of the thinning kernel and one outside it, and more instances than one batch when the budget says so."""
import os

import numpy as np
import pytest
import torch

from tests.skeleton_graph_cases import RING_ID, T_ID, cases, positive_ids
from tests.test_skeleton_graph_cpu import N_GRAPH, SPACINGS, golden_rows, skeleton_graph_oracle, want_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOBS = "blobs (24, 40, 70)"
CASES = cases()


def _ffi_workspace_bytes(boxes):
    from skoots_amd import _ffi
    return int(_ffi.lib.sk_skeletonize_workspace_bytes(boxes.ctypes.data_as(_ffi.ip), boxes.shape[0]))


def check(name, lab, dtype, **kw):
    from skoots_amd.validate.lib import instance_skeleton_graph
    ids, graph = want_graph(name, lab)
    x = torch.from_numpy(lab).to(dtype).to(DEV)
    got_ids, got, vol = instance_skeleton_graph(x, want_volume=True, **kw)
    assert got_ids.dtype == torch.int64 and got.dtype == torch.int64 and got.is_cuda and vol.dtype == torch.int32
    assert tuple(got.shape) == (len(ids), N_GRAPH) and tuple(vol.shape) == lab.shape
    assert np.array_equal(got_ids.cpu().numpy(), ids) and np.array_equal(ids, positive_ids(lab))
    g = got.cpu().numpy()
    bad = np.argwhere(g != graph)
    assert bad.size == 0, f"{name}: {len(bad)} values differ, first (row, column) {bad[0]}: " \
                          f"{g[tuple(bad[0])]} != {graph[tuple(bad[0])]}"
    assert np.array_equal(vol.cpu().numpy(), golden_rows(name)), name
    two = instance_skeleton_graph(x, **kw)
    assert len(two) == 2 and torch.equal(two[0], got_ids) and torch.equal(two[1], got)
    return got_ids, got, vol


@pytest.mark.parametrize("name", [n for n in CASES if "int64" not in n])
def test_every_case_int32(name):
    check(name, CASES[name], torch.int32)


@pytest.mark.parametrize("name", [n for n in CASES if "huge" not in n and int(CASES[n].max()) < 256])
def test_every_small_id_case_uint8(name):
    check(name, CASES[name], torch.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_int64(name):
    check(name, CASES[name].astype(np.int64), torch.int64)


def test_blobs_as_uint8_ranks():
    """the blobs volume has ids above 255: its instances renumbered 1 .. N fit uint8 and thin alike"""
    lab = CASES[BLOBS]
    ranks = (np.searchsorted(positive_ids(lab), lab) + 1) * (lab > 0)
    from skoots_amd.validate.lib import instance_skeleton_graph
    ids, got, vol = instance_skeleton_graph(torch.from_numpy(ranks.astype(np.uint8)).to(DEV), want_volume=True)
    assert ids.tolist() == list(range(1, 33))
    assert np.array_equal(got.cpu().numpy(), want_graph(BLOBS, lab)[1])
    assert np.array_equal(vol.cpu().numpy(), golden_rows(BLOBS))


def test_huge_ids_take_the_relabel_route(monkeypatch):
    from skoots_amd.validate import lib as VL
    monkeypatch.setattr(VL, "_lut", lambda m: pytest.fail("the max id + 1 table was built for a huge id"))
    for name, dtype in (("huge int32 (4, 5, 36)", torch.int32), ("huge int64 (4, 5, 36)", torch.int64)):
        ids, _, _ = check(name, CASES[name], dtype)
    assert ids.tolist() == [70000, 2 ** 30, 2 ** 40]


def test_anchors_on_the_device():
    ids, got, _ = check(BLOBS, CASES[BLOBS], torch.int32)
    ids = ids.tolist()
    ring, tee = got[ids.index(RING_ID)].tolist(), got[ids.index(T_ID)].tolist()
    assert ring[:5] == [60, 0, 0, 60, 0] and sum(ring[5:]) == 60
    assert tee[0] == 32 and tee[2] == 3 and tee[4] == 1
    assert int((got[:, 0] == 0).sum()) == 6                          # instances that thin away: rows of zeros
    assert bool((got[got[:, 0] == 0] == 0).all())


def test_large_object_outside_lds():
    """(84, 84, 40): thinned in the whole volume, the six planes of its padded crop do not fit the thinning kernel's
    LDS, so the skeleton the graph kernel reads is the workspace's own image plane; in its own box they just fit"""
    from skoots_amd.lib.morphology import skeleton_graph
    from skoots_amd.validate.lib import instance_skeleton_graph
    from tests.test_skeletonize import golden, large_object
    big = large_object()
    skel = np.zeros(big.shape, np.int32)
    skel[tuple(golden()["c_points"].astype(np.int64).T)] = 1
    _, want = skeleton_graph_oracle(skel)
    x = torch.from_numpy(big.astype(np.int32)).to(DEV)
    whole = np.array([[0, 0, 0, 84, 84, 40]], np.int32)
    assert _ffi_workspace_bytes(whole) > 6 * 4 * 86 * 86 * 2 > 152 * 1024
    graph, counts, points = skeleton_graph(x, [1], whole, want_points=True)
    assert graph.cpu().numpy().tolist() == want.tolist() and counts.tolist() == [want[0, 0]]
    assert np.array_equal(points.cpu().numpy(), np.argwhere(skel))
    for boxes in (None, torch.tensor([[0, 0, 0, 83, 83, 39]], dtype=torch.int32, device=DEV)):
        ids, got, vol = instance_skeleton_graph(x, boxes=boxes, want_volume=True)
        assert ids.tolist() == [1] and got.cpu().numpy().tolist() == want.tolist()
        assert np.array_equal(vol.cpu().numpy(), skel)
    assert want[0, 4] > 0 and want[0, 0] > 100                       # a ring crossed by a bar: junctions


def test_the_budget_does_not_change_the_result(monkeypatch):
    from skoots_amd.lib import morphology
    from skoots_amd.validate import lib as VL
    x = torch.from_numpy(CASES[BLOBS]).to(DEV)
    sizes = []
    real = morphology.skeleton_graph
    monkeypatch.setattr(morphology, "skeleton_graph", lambda a, ids, boxes, **kw: sizes.append(len(ids)) or
                        real(a, ids, boxes, **kw))
    default = VL.instance_skeleton_graph(x, want_volume=True)
    assert sizes == [32] and VL.SKELETON_BUDGET == 1 << 30
    del sizes[:]
    single = VL.instance_skeleton_graph(x, budget_bytes=1, want_volume=True)
    assert sizes == [1] * 32
    del sizes[:]
    some = VL.instance_skeleton_graph(x, budget_bytes=4096, want_volume=True)
    assert 1 < len(sizes) < 32 and sum(sizes) == 32
    for other in (single, some):
        assert all(torch.equal(a, b) for a, b in zip(default, other))
    # rows and boxes handed in give the same again
    rows = VL.id_rows(x)
    boxes = VL.instance_sums(x, rows)[2]
    again = VL.instance_skeleton_graph(x, rows, boxes)
    assert torch.equal(again[1], default[1])


def test_morphology_skeleton_graph_shares_the_workspace_with_emit():
    from skoots_amd.lib.morphology import skeleton_graph, thin_objects
    lab = CASES[BLOBS]
    ids = positive_ids(lab)
    boxes = []
    for u in ids:
        nz = np.argwhere(lab == u)
        boxes.append(np.concatenate((nz.min(0), nz.max(0) + 1)))
    x = torch.from_numpy(lab).to(DEV)
    points, counts, _ = thin_objects(x, ids, boxes)
    graph, g_counts, g_points = skeleton_graph(x, ids, boxes, want_points=True)
    assert graph.dtype == torch.int64 and graph.is_cuda and tuple(graph.shape) == (len(ids), N_GRAPH)
    assert np.array_equal(g_counts, counts) and g_counts.dtype == np.int64 and torch.equal(g_points, points)
    assert graph[:, 0].cpu().numpy().tolist() == counts.tolist()
    assert np.array_equal(graph.cpu().numpy(), want_graph(BLOBS, lab)[1])
    graph2, _, none = skeleton_graph(x, ids, boxes)
    assert none is None and torch.equal(graph2, graph)
    empty = skeleton_graph(x, [], np.zeros((0, 6), np.int32), want_points=True)
    assert tuple(empty[0].shape) == (0, N_GRAPH) and empty[1].shape == (0,) and tuple(empty[2].shape) == (0, 3)


def test_c_abi_guards_launch_nothing():
    import ctypes as C
    from skoots_amd import _ffi
    assert _ffi.lib.sk_skeleton_graph_row_values() == 12 and _ffi.lib.sk_abi_version() >= 16
    boxes = np.array([[0, 0, 0, 4, 5, 40], [1, 1, 1, 3, 3, 3]], np.int32)
    boxes_p = boxes.ctypes.data_as(_ffi.ip)
    nbytes = _ffi.lib.sk_skeletonize_workspace_bytes(boxes_p, 2)
    assert nbytes > 0
    work = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    graph = torch.full((2, N_GRAPH), -7, dtype=torch.int64, device=DEV)

    def call(boxes_p=boxes_p, n=2, work_p=_ffi.ptr(work), size=nbytes, graph_p=_ffi.ptr(graph)):
        rc = _ffi.lib.sk_skeleton_graph(boxes_p, n, work_p, C.c_size_t(size), graph_p, _ffi.stream_ptr(work.device))
        torch.cuda.synchronize()
        return rc

    for null in ("boxes_p", "work_p", "graph_p"):
        assert call(**{null: None}) == -1 and "sk_skeleton_graph" in _ffi.last_error()
    assert call(n=0) == -1 and call(n=-1) == -1
    assert call(size=nbytes - 1) == -1 and "workspace" in _ffi.last_error() and str(nbytes) in _ffi.last_error()
    assert call(size=0) == -1
    bad = np.array([[0, 0, 0, 4, 0, 4], [1, 1, 1, 3, 3, 3]], np.int32)          # an empty box
    assert call(boxes_p=bad.ctypes.data_as(_ffi.ip)) == -1 and "empty" in _ffi.last_error()
    assert call(graph_p=graph.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert bool((graph == -7).all())                                 # nothing ran


def test_refuses_a_box_too_large_before_any_launch(monkeypatch):
    from skoots_amd.lib import morphology
    from skoots_amd.validate import lib as VL
    monkeypatch.setattr(morphology, "skeleton_graph", lambda *a, **k: pytest.fail("a batch was launched"))
    x = torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV)
    x[0, 0, 0], x[1, 1, 1] = 5, 77
    rows = VL.id_rows(x)
    boxes = torch.tensor([[0, 0, 0, 0, 0, 0], [0, 0, 0, 1023, 1023, 1023]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="instance 77 "):
        VL.instance_skeleton_graph(x, rows, boxes)
    # 4.0e8 voxels, below 2^30, in one word per row: 20002^2 words of padded plane, and 6 of them reach 2^31
    boxes[1] = torch.tensor([0, 0, 0, 19999, 19999, 0])
    with pytest.raises(ValueError, match="instance 77 "):
        VL.instance_skeleton_graph(x, rows, boxes)


def test_empty_masks():
    from skoots_amd.validate.lib import instance_skeleton_graph
    for x in (torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV), torch.full((3, 3, 3), -5, dtype=torch.int32,
                                                                                   device=DEV)):
        ids, graph = instance_skeleton_graph(x)
        assert tuple(ids.shape) == (0,) and tuple(graph.shape) == (0, N_GRAPH)
        assert ids.dtype == torch.int64 and graph.dtype == torch.int64 and graph.is_cuda
        vol = instance_skeleton_graph(x, want_volume=True)[2]
        assert tuple(vol.shape) == tuple(x.shape) and vol.dtype == torch.int32 and not bool(vol.any())
    with pytest.raises(TypeError):
        instance_skeleton_graph(torch.zeros((3, 3, 3), device=DEV))
    with pytest.raises(ValueError):
        instance_skeleton_graph(torch.zeros((3, 3, 3), dtype=torch.int32))


def test_stats_per_instance_and_get_skeleton_length():
    from skoots_amd.validate.compare import skeleton_columns, stats_per_instance
    from skoots_amd.validate.stats import get_skeleton_length
    lab = CASES[BLOBS]
    x = torch.from_numpy(lab).to(DEV)
    ids, graph = want_graph(BLOBS, lab)
    plain = stats_per_instance(x, SPACINGS[1])
    assert set(plain) == {"id", "voxels", "volume", "bbox", "touches_border", "centroid", "face_area", "faces",
                          "axis_lengths", "sums"}
    for spacing in SPACINGS:
        st = stats_per_instance(x[None], spacing, skeleton=True)
        assert set(st) - set(plain) == {"skeleton_graph", "skeleton_voxels", "skeleton_length", "skeleton_endpoints",
                                        "skeleton_junctions", "skeleton_links", "skeleton_branches"}
        assert st["id"].tolist() == ids.tolist() and st["skeleton_graph"].dtype == torch.int64
        assert np.array_equal(st["skeleton_graph"].cpu().numpy(), graph)
        for k, v in skeleton_columns(torch.from_numpy(graph), spacing).items():
            assert st[k].is_cuda and st[k].dtype == v.dtype and torch.equal(st[k].cpu(), v), k
        assert all(torch.equal(st[k], plain[k]) for k in plain if spacing == SPACINGS[1])
    both = stats_per_instance(x, SPACINGS[1], surface="closed", skeleton=True)
    assert "surface_area" in both and torch.equal(both["skeleton_length"], st["skeleton_length"])
    i = ids.tolist().index(T_ID)
    one = get_skeleton_length(x == T_ID, SPACINGS[1])
    assert one.dtype == torch.float64 and one.is_cuda and one.item() == st["skeleton_length"][i].item()
    assert get_skeleton_length(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]).item() == 0.0


def test_command_end_to_end(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import main, skeleton_columns
    lab = CASES[BLOBS]
    ids, graph = want_graph(BLOBS, lab)
    x = torch.from_numpy(lab).to(DEV)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    spacing = SPACINGS[1]
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read().splitlines()
    assert not os.path.exists(os.path.join(tmp_path, "mito_skeletons.tif"))
    out = main(args + ["--save-skeletons", "--surface-area", "open"])
    assert out == os.path.join(tmp_path, "mito_instance_stats.csv")
    lines = open(out).read().splitlines()
    assert lines[:2] == plain[:2] and lines[2] == plain[2] + ",surface_area,surface_to_volume,skeleton_voxels," \
        "skeleton_length,skeleton_endpoints,skeleton_junctions,skeleton_branches"
    assert [ln.split(",")[:17] for ln in lines[3:]] == [ln.split(",") for ln in plain[3:]]
    col = skeleton_columns(torch.from_numpy(graph), spacing)
    keep = np.array([(lab == u).sum() >= 2 for u in ids])
    assert keep.any() and [int(ln.split(",")[0]) for ln in lines[3:]] == ids[keep].tolist()
    rows = [ln.split(",")[19:] for ln in lines[3:]]
    for j, k in enumerate(("skeleton_voxels", "skeleton_length", "skeleton_endpoints", "skeleton_junctions",
                           "skeleton_branches")):
        want = col[k].numpy()[keep].tolist()
        assert [float(r[j]) if k == "skeleton_length" else int(r[j]) for r in rows] == want, k
    only = open(main(args + ["--skeleton", "--out", os.path.join(tmp_path, "only.csv")])).read().splitlines()
    assert [ln.split(",")[17:] for ln in only[3:]] == rows
    # the skeletons, each voxel its instance id, stored [Z, X, Y] like the mask
    skel = tiff.read_image(os.path.join(tmp_path, "mito_skeletons.tif"))
    want = np.concatenate(([0], ids))[golden_rows(BLOBS)]
    assert skel.shape == (lab.shape[2], lab.shape[0], lab.shape[1])
    assert np.array_equal(skel.astype(np.int64).transpose(1, 2, 0), want)
