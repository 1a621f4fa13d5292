"""The branch tracing on the device (skoots_amd/csrc/skeletonize.hip: ``sk_skeleton_pack``,
``sk_skeleton_branches_count``, ``sk_skeleton_branches_emit``) and everything on top of it --
``lib.morphology.skeleton_branches``, ``validate.lib.instance_skeleton_branches``, ``stats_per_instance(branches=True)``,
``get_branches`` and ``python -m skoots_amd.validate.compare --branches`` -- against the python oracle of
tests/test_skeleton_branches_cpu.py.  Every output of the kernels is an integer: every comparison is exact equality.

Three settings: the cases of tests/skeleton_graph_cases.py thinned on the device (the oracle reads the skeleton the
device emitted), the hand-built skeletons of tests/skeleton_branch_cases.py packed without thinning, and one object
thinned in the whole volume, whose planes do not fit the thinning kernel's LDS."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.skeleton_branch_cases import cases as branch_cases
from tests.skeleton_graph_cases import cases as graph_cases, positive_ids
from tests.test_skeleton_branches_cpu import N_BRANCH, N_NODE, skeleton_branches_oracle
from tests.test_skeleton_graph_cpu import N_GRAPH, SPACINGS, golden_rows, skeleton_graph_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOBS = "blobs (24, 40, 70)"
GRAPH_CASES = graph_cases()
BRANCH_CASES = branch_cases()


_wanted = {}


def want_for(skeleton_rows, n, key=None):
    """(graph (n, 12), nodes, branches, points, owner) for a skeleton volume labelled with the instances' rows 1 .. n:
    the oracles, column 0 of the tables the instance's index (an instance without skeleton has no rows)"""
    if key is not None and key in _wanted:
        return _wanted[key]
    rows, nodes, branches, points, owner = skeleton_branches_oracle(skeleton_rows)
    nodes, branches = nodes.copy(), branches.copy()
    if len(rows):
        nodes[:, 0], branches[:, 0] = rows[nodes[:, 0]] - 1, rows[branches[:, 0]] - 1
    graph = np.zeros((n, N_GRAPH), np.int64)
    grows, g = skeleton_graph_oracle(skeleton_rows)
    graph[grows - 1] = g
    if key is not None:
        _wanted[key] = (graph, nodes, branches, points, owner)
    return graph, nodes, branches, points, owner


def check_tables(got, want, name):
    ids, graph, nodes, branches, points, owner = got
    assert graph.dtype == torch.int64 and all(t.dtype == torch.int32 and t.is_cuda for t in (nodes, branches, points, owner))
    for what, a, b in zip(("graph", "nodes", "branches", "points", "owner"), (graph, nodes, branches, points, owner), want):
        a = a.cpu().numpy()
        assert a.shape == b.shape, f"{name}: {what} has the shape {a.shape}, the oracle's {b.shape}"
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{name}: {len(bad)} values of {what} differ, first at {bad[0]}: " \
                              f"{a[tuple(bad[0])]} != {b[tuple(bad[0])]}"


def rows_volume(points, graph, shape):
    vol = np.zeros(shape, np.int32)
    row = np.repeat(np.arange(1, graph.shape[0] + 1), graph[:, 0].cpu().numpy())
    vol[tuple(points.cpu().numpy().T)] = row
    return vol


@pytest.mark.parametrize("name", list(GRAPH_CASES))
def test_thinned_on_the_device(name):
    """every case thinned on the device; the oracle runs on the skeleton the device emitted, which is the golden one"""
    from skoots_amd.validate.lib import instance_skeleton_branches
    lab = GRAPH_CASES[name]
    x = torch.from_numpy(lab).to(DEV)
    got = instance_skeleton_branches(x)
    assert np.array_equal(got[0].cpu().numpy(), positive_ids(lab))
    emitted = rows_volume(got[4], got[1], lab.shape)
    assert np.array_equal(emitted, golden_rows(name))
    check_tables(got, want_for(emitted, len(got[0]), name), name)


@pytest.mark.parametrize("name", list(BRANCH_CASES))
def test_hand_built_through_pack(name):
    """every hand-built skeleton as its own mask, packed without thinning; the graph rows of the packed planes too"""
    from skoots_amd.validate.lib import instance_skeleton_branches
    lab = BRANCH_CASES[name]
    ids = positive_ids(lab)
    x = torch.from_numpy(lab).to(DEV)
    got = instance_skeleton_branches(x, skeleton=x)
    assert np.array_equal(got[0].cpu().numpy(), ids)
    rows = ((np.searchsorted(ids, lab.clip(min=0)) + 1) * (lab > 0)).astype(np.int32)
    want = want_for(rows, len(ids))
    check_tables(got, want, name)
    assert np.array_equal(got[1].cpu().numpy(), skeleton_graph_oracle(lab)[1])
    assert np.array_equal(rows_volume(got[4], got[1], lab.shape), rows)          # nothing was thinned
    # owner against the tables: every chain voxel names a branch of its instance, every node voxel a node of it
    owner, nodes, branches = (t.cpu().numpy().astype(np.int64) for t in (got[5], got[2], got[3]))
    assert np.array_equal(np.bincount(owner[owner >= 0], minlength=len(branches)), branches[:, 3])
    assert np.array_equal(np.bincount(-1 - owner[owner < 0], minlength=len(nodes)), nodes[:, 2])
    inst = np.repeat(np.arange(len(ids)), got[1][:, 0].cpu().numpy())
    assert np.array_equal(np.where(owner >= 0, branches[owner.clip(min=0), 0] if len(branches) else -1,
                                   nodes[(-1 - owner).clip(min=0), 0]), inst)


def test_large_object_outside_lds():
    """(84, 84, 40) thinned in the whole volume: the planes live in the global workspace, not in LDS"""
    from skoots_amd.lib.morphology import skeleton_branches
    from tests.test_skeletonize import golden, large_object
    big = large_object()
    skel = np.zeros(big.shape, np.int32)
    skel[tuple(golden()["c_points"].astype(np.int64).T)] = 1
    want = want_for(skel, 1)
    x = torch.from_numpy(big.astype(np.int32)).to(DEV)
    whole = np.array([[0, 0, 0, 84, 84, 40]], np.int32)
    graph, counts, points, nodes, branches, owner = skeleton_branches(x, [1], whole)
    assert counts.tolist() == [226] and counts.dtype == np.int64
    check_tables((None, graph, nodes, branches, points, owner), want, "large object")
    assert nodes[:, 1].tolist() == [2, 2] and branches.shape[0] == 3
    pairs = branches[:, 1:3].tolist()
    assert pairs.count([0, 1]) >= 2                              # two of the three are parallel
    packed = skeleton_branches(torch.from_numpy(skel).to(DEV), [1], whole, thin=False)
    assert all(torch.equal(a, b) for a, b in zip(packed[2:], (points, nodes, branches, owner)))
    assert torch.equal(packed[0], graph)


def test_the_budget_does_not_change_the_result_and_runs_are_identical(monkeypatch):
    from skoots_amd.lib import morphology
    from skoots_amd.validate import lib as VL
    x = torch.from_numpy(GRAPH_CASES[BLOBS]).to(DEV)
    sizes = []
    real = morphology.skeleton_branches
    monkeypatch.setattr(morphology, "skeleton_branches", lambda a, ids, boxes, **kw: sizes.append(len(ids)) or
                        real(a, ids, boxes, **kw))
    default = VL.instance_skeleton_branches(x)
    assert sizes == [32]
    del sizes[:]
    single = VL.instance_skeleton_branches(x, budget_bytes=1)
    assert sizes == [1] * 32
    del sizes[:]
    some = VL.instance_skeleton_branches(x, budget_bytes=4096)
    assert 1 < len(sizes) < 32 and sum(sizes) == 32
    again = VL.instance_skeleton_branches(x)
    for other in (single, some, again):
        assert all(torch.equal(a, b) for a, b in zip(default, other))
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(default, other))
    rows = VL.id_rows(x)
    boxes = VL.instance_sums(x, rows)[2]
    assert all(torch.equal(a, b) for a, b in zip(default, VL.instance_skeleton_branches(x, rows, boxes)))
    # the saved skeletons traced without thinning give the same again
    skeleton = torch.cat((default[0].new_zeros(1), default[0]))[torch.from_numpy(golden_rows(BLOBS).copy()).long().to(DEV)]
    assert all(torch.equal(a, b) for a, b in zip(default, VL.instance_skeleton_branches(x, skeleton=skeleton)))


def _packed(lab):
    """the C-ABI state after sk_skeleton_pack on a one-id volume: everything the branch calls take"""
    from skoots_amd import _ffi
    x = torch.from_numpy(lab).to(torch.int32).to(DEV)
    X, Y, Z = lab.shape
    boxes = np.array([[0, 0, 0, X, Y, Z]], np.int32)
    boxes_p = boxes.ctypes.data_as(_ffi.ip)
    nbytes = int(_ffi.lib.sk_skeletonize_workspace_bytes(boxes_p, 1))
    work = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    ids = torch.tensor([int(lab.max())], dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    err = torch.ones(1, dtype=torch.int32, device=DEV)
    stream = _ffi.stream_ptr(torch.device(DEV))
    _ffi.check(_ffi.lib.sk_skeleton_pack(_ffi.ptr(x), X, Y, Z, _ffi.ptr(ids), boxes_p, 1, _ffi.ptr(work),
                                         C.c_size_t(nbytes), _ffi.ptr(counts), _ffi.ptr(stats), _ffi.ptr(err), stream))
    assert err.item() == 0
    counts_host = counts.cpu().numpy()
    sbytes = int(_ffi.lib.sk_skeleton_branches_scratch_bytes(boxes_p, counts_host.ctypes.data_as(_ffi.ip), 1))
    assert sbytes == 16 + 44 * int(counts_host[0])
    offsets = torch.tensor([0, int(counts_host[0])], dtype=torch.int32, device=DEV)
    scratch = torch.zeros(sbytes, dtype=torch.uint8, device=DEV)
    return dict(x=x, boxes=boxes, boxes_p=boxes_p, nbytes=nbytes, work=work, ids=ids, counts=counts, stats=stats,
                err=err, stream=stream, sbytes=sbytes, offsets=offsets, scratch=scratch, n_points=int(counts_host[0]))


def test_canary_rows_past_the_totals_stay_untouched():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 26
    assert (_ffi.lib.sk_skeleton_nodes_row_values(), _ffi.lib.sk_skeleton_branches_row_values()) == (N_NODE, N_BRANCH)
    lab = BRANCH_CASES["theta"]
    s = _packed(lab)
    _, want_nodes, want_branches, _, want_owner = skeleton_branches_oracle((lab > 0).astype(np.int32))
    per = torch.full((1, 2), -9, dtype=torch.int32, device=DEV)
    common = (s["boxes_p"], 1, _ffi.ptr(s["work"]), C.c_size_t(s["nbytes"]), _ffi.ptr(s["offsets"]), s["n_points"],
              _ffi.ptr(s["scratch"]), C.c_size_t(s["sbytes"]))
    _ffi.check(_ffi.lib.sk_skeleton_branches_count(*common, _ffi.ptr(per), s["stream"]))
    assert per.tolist() == [[2, 3]]
    for n_nodes, n_branches in ((2, 3), (1, 2), (0, 0)):
        nodes = torch.full((4, N_NODE), -7, dtype=torch.int32, device=DEV)
        branches = torch.full((5, N_BRANCH), -7, dtype=torch.int32, device=DEV)
        owner = torch.full((s["n_points"] + 3,), -7, dtype=torch.int32, device=DEV)
        noff = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
        boff = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
        _ffi.check(_ffi.lib.sk_skeleton_branches_emit(*common, _ffi.ptr(noff), _ffi.ptr(boff), n_nodes, n_branches,
                                                      _ffi.ptr(nodes), _ffi.ptr(branches), _ffi.ptr(owner), s["stream"]))
        assert np.array_equal(nodes[:n_nodes].cpu().numpy(), want_nodes[:n_nodes])
        assert np.array_equal(branches[:n_branches].cpu().numpy(), want_branches[:n_branches])
        assert bool((nodes[n_nodes:] == -7).all()) and bool((branches[n_branches:] == -7).all())
        assert bool((owner[s["n_points"]:] == -7).all())
        if n_branches == 3:
            assert np.array_equal(owner[:s["n_points"]].cpu().numpy(), want_owner)
    # offsets that do not match the plane: the object is refused, nothing else happens
    wrong = torch.tensor([0, s["n_points"] - 1], dtype=torch.int32, device=DEV)
    _ffi.check(_ffi.lib.sk_skeleton_branches_count(common[0], 1, common[2], common[3], _ffi.ptr(wrong), s["n_points"],
                                                   common[6], common[7], _ffi.ptr(per), s["stream"]))
    assert per.tolist() == [[-1, -1]]


def test_c_abi_guards_launch_nothing():
    from skoots_amd import _ffi
    L = _ffi.lib
    s = _packed(BRANCH_CASES["lollipop"])
    per = torch.full((1, 2), -9, dtype=torch.int32, device=DEV)
    nodes = torch.full((2, N_NODE), -7, dtype=torch.int32, device=DEV)
    branches = torch.full((2, N_BRANCH), -7, dtype=torch.int32, device=DEV)
    owner = torch.full((s["n_points"],), -7, dtype=torch.int32, device=DEV)
    noff = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    base = dict(boxes_p=s["boxes_p"], n=1, work=s["work"].data_ptr(), nbytes=s["nbytes"], offsets=s["offsets"].data_ptr(),
                n_points=s["n_points"], scratch=s["scratch"].data_ptr(), sbytes=s["sbytes"])

    def count(per_p=per.data_ptr(), **kw):
        a = {**base, **kw}
        rc = L.sk_skeleton_branches_count(a["boxes_p"], a["n"], a["work"], C.c_size_t(a["nbytes"]), a["offsets"],
                                          a["n_points"], a["scratch"], C.c_size_t(a["sbytes"]), per_p, s["stream"])
        torch.cuda.synchronize()
        return rc

    def emit(noff_p=noff.data_ptr(), boff_p=boff.data_ptr(), n_nodes=2, n_branches=2, nodes_p=nodes.data_ptr(),
             branches_p=branches.data_ptr(), owner_p=owner.data_ptr(), **kw):
        a = {**base, **kw}
        rc = L.sk_skeleton_branches_emit(a["boxes_p"], a["n"], a["work"], C.c_size_t(a["nbytes"]), a["offsets"],
                                         a["n_points"], a["scratch"], C.c_size_t(a["sbytes"]), noff_p, boff_p, n_nodes,
                                         n_branches, nodes_p, branches_p, owner_p, s["stream"])
        torch.cuda.synchronize()
        return rc

    empty_box = np.array([[0, 0, 0, 4, 0, 4]], np.int32)
    shared = (dict(boxes_p=None), dict(n=0), dict(n=-1), dict(work=None), dict(nbytes=s["nbytes"] - 1), dict(nbytes=0),
              dict(offsets=None), dict(n_points=-1), dict(n_points=2 ** 31), dict(scratch=None),
              dict(sbytes=s["sbytes"] - 1), dict(sbytes=0), dict(work=s["work"].data_ptr() + 4),
              dict(scratch=s["scratch"].data_ptr() + 2), dict(offsets=s["offsets"].data_ptr() + 1),
              dict(boxes_p=empty_box.ctypes.data_as(_ffi.ip)))
    for call, what in ((count, "sk_skeleton_branches_count"), (emit, "sk_skeleton_branches_emit")):
        for kw in shared:
            assert call(**kw) == -1, kw
            assert what in _ffi.last_error() or "sk_skeletonize" in _ffi.last_error(), kw
    assert count(per_p=None) == -1 and count(per_p=per.data_ptr() + 2) == -1
    for kw in (dict(noff_p=None), dict(boff_p=None), dict(n_nodes=-1), dict(n_branches=-1), dict(n_nodes=2 ** 31),
               dict(nodes_p=None), dict(branches_p=None), dict(owner_p=None), dict(nodes_p=nodes.data_ptr() + 2),
               dict(owner_p=owner.data_ptr() + 1), dict(noff_p=noff.data_ptr() + 2)):
        assert emit(**kw) == -1, kw
    assert bool((per == -9).all()) and bool((nodes == -7).all()) and bool((branches == -7).all())
    assert bool((owner == -7).all())                             # nothing ran
    # sk_skeleton_pack: the checks of sk_skeletonize
    x, X, Y, Z = s["x"], *s["x"].shape

    def pack(x_p=x.data_ptr(), n=1, work_p=s["work"].data_ptr(), nbytes=s["nbytes"], counts_p=s["counts"].data_ptr(),
             boxes_p=s["boxes_p"], dims=(X, Y, Z)):
        return L.sk_skeleton_pack(x_p, *dims, s["ids"].data_ptr(), boxes_p, n, work_p, C.c_size_t(nbytes), counts_p,
                                  s["stats"].data_ptr(), s["err"].data_ptr(), s["stream"])

    outside = np.array([[0, 0, 0, X + 1, Y, Z]], np.int32)
    for kw in (dict(x_p=None), dict(n=0), dict(work_p=None), dict(nbytes=s["nbytes"] - 1), dict(counts_p=None),
               dict(work_p=s["work"].data_ptr() + 4), dict(dims=(0, Y, Z)), dict(boxes_p=outside.ctypes.data_as(_ffi.ip)),
               dict(boxes_p=empty_box.ctypes.data_as(_ffi.ip))):
        assert pack(**kw) == -1, kw
    bad_counts = np.array([-1], np.int32)
    assert L.sk_skeleton_branches_scratch_bytes(s["boxes_p"], bad_counts.ctypes.data_as(_ffi.ip), 1) == 0
    bad_counts[0] = int(np.prod(s["x"].shape)) + 1
    assert L.sk_skeleton_branches_scratch_bytes(s["boxes_p"], bad_counts.ctypes.data_as(_ffi.ip), 1) == 0
    assert L.sk_skeleton_branches_scratch_bytes(s["boxes_p"], None, 1) == 0


def test_empty_inputs():
    from skoots_amd.lib.morphology import skeleton_branches
    from skoots_amd.validate.lib import instance_skeleton_branches
    x = torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV)
    ids, graph, nodes, branches, points, owner = instance_skeleton_branches(x)
    assert tuple(ids.shape) == (0,) and tuple(graph.shape) == (0, N_GRAPH) and tuple(nodes.shape) == (0, N_NODE)
    assert tuple(branches.shape) == (0, N_BRANCH) and tuple(points.shape) == (0, 3) and tuple(owner.shape) == (0,)
    out = skeleton_branches(x, [], np.zeros((0, 6), np.int32))
    assert tuple(out[3].shape) == (0, N_NODE) and tuple(out[4].shape) == (0, N_BRANCH) and out[1].shape == (0,)
    # a mask whose saved skeleton is empty: every instance an empty object
    x[1:4, 1:4, 1:4] = 5
    ids, graph, nodes, branches, points, owner = instance_skeleton_branches(x, skeleton=torch.zeros_like(x))
    assert ids.tolist() == [5] and graph.tolist() == [[0] * N_GRAPH] and nodes.shape[0] == branches.shape[0] == 0
    with pytest.raises(ValueError):
        instance_skeleton_branches(x, skeleton=torch.zeros((3, 3, 3), dtype=torch.int32, device=DEV))


def test_stats_per_instance_and_get_branches():
    from skoots_amd.validate.compare import BRANCH_COLUMNS, branch_columns, stats_per_instance
    from skoots_amd.validate.stats import get_branches
    lab = GRAPH_CASES[BLOBS]
    x = torch.from_numpy(lab).to(DEV)
    n = len(positive_ids(lab))
    _, want_nodes, want_branches, _, _ = want_for(golden_rows(BLOBS), n, BLOBS)
    spacing = SPACINGS[1]
    plain = stats_per_instance(x, spacing, skeleton=True)
    st = stats_per_instance(x, spacing, branches=True)
    assert set(st) - set(plain) == set(BRANCH_COLUMNS.split(",")) | {"skeleton_nodes", "skeleton_branch_table",
                                                                     "skeleton_points", "skeleton_owner"}
    assert all(torch.equal(st[k], plain[k]) for k in plain)
    assert np.array_equal(st["skeleton_nodes"].cpu().numpy(), want_nodes)
    assert np.array_equal(st["skeleton_branch_table"].cpu().numpy(), want_branches)
    for k, v in branch_columns(torch.from_numpy(want_nodes), torch.from_numpy(want_branches), n, spacing).items():
        assert st[k].is_cuda and st[k].dtype == v.dtype and torch.equal(st[k].cpu(), v), k
    both = stats_per_instance(x, spacing, branches=True, thickness="closed")
    ref = stats_per_instance(x, spacing, skeleton=True, thickness="closed")
    assert all(torch.equal(both[k], ref[k]) for k in ("skeleton_radius_mean", "skeleton_radius_min", "skeleton_radius_max"))
    with pytest.raises(ValueError):
        stats_per_instance(x, spacing, skeleton_volume=x)
    from tests.skeleton_graph_cases import T_ID
    i = positive_ids(lab).tolist().index(T_ID)
    one = get_branches(x == T_ID, spacing)
    assert one["graph_branches"] == 3 and one["graph_junctions"] == 1 and one["graph_endpoints"] == 3
    assert one["graph_cycles"] == 0 and one["graph_length"] == st["graph_length"][i].item()
    assert tuple(one["nodes"].shape) == (4, N_NODE) and one["lengths"].dtype == torch.float64 and one["lengths"].is_cuda
    none = get_branches(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1])
    assert none["graph_branches"] == 0 and none["graph_length"] == 0.0 and none["nodes"].shape[0] == 0


def test_command_end_to_end(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import (BRANCH_COLUMNS, BRANCH_CSV_COLUMNS, BRANCH_RADIUS_COLUMNS, branch_columns,
                                             format_branches_csv, format_nodes_csv, main)
    lab = GRAPH_CASES[BLOBS]
    ids = positive_ids(lab)
    _, want_nodes, want_branches, _, _ = want_for(golden_rows(BLOBS), len(ids), BLOBS)
    nodes, branches = torch.from_numpy(want_nodes), torch.from_numpy(want_branches)
    x = torch.from_numpy(lab).to(DEV)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    spacing = SPACINGS[1]
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    old = open(main(args + ["--skeleton", "--save-skeletons", "--out", os.path.join(tmp_path, "old.csv")])).read()
    for suffix in ("branches", "nodes"):
        assert not os.path.exists(os.path.join(tmp_path, f"mito_{suffix}.csv"))
    out = main(args + ["--branches"])
    lines, old_lines = open(out).read().splitlines(), old.splitlines()
    assert lines[2] == old_lines[2] + "," + BRANCH_COLUMNS
    assert [ln.split(",")[:22] for ln in lines[3:]] == [ln.split(",") for ln in old_lines[3:]]
    keep = [(lab == u).sum() >= 2 for u in ids]
    col = branch_columns(nodes, branches, len(ids), spacing)
    names = BRANCH_COLUMNS.split(",")
    want_rows = [[str(col[k][i].item()) if k in names[:7] else repr(col[k][i].item()) for k in names]
                 for i in range(len(ids)) if keep[i]]
    assert [ln.split(",")[22:] for ln in lines[3:]] == want_rows
    btext = open(os.path.join(tmp_path, "mito_branches.csv")).read()
    assert btext == format_branches_csv(path, ids, nodes, branches, spacing, keep)
    assert btext.splitlines()[2] == BRANCH_CSV_COLUMNS and len(btext.splitlines()) > 10
    ntext = open(os.path.join(tmp_path, "mito_nodes.csv")).read()
    assert ntext == format_nodes_csv(path, ids, nodes, keep)
    # the saved skeletons give the same three files without thinning, and --thickness adds the radii along the branches
    again = main(args + ["--branches", "--skeleton-from", os.path.join(tmp_path, "mito_skeletons.tif"), "--out",
                         os.path.join(tmp_path, "again.csv")])
    assert open(again).read() == open(out).read()
    assert open(os.path.join(tmp_path, "mito_branches.csv")).read() == btext
    main(args + ["--branches", "--thickness", "closed", "--out", os.path.join(tmp_path, "thick.csv")])
    thick = open(os.path.join(tmp_path, "mito_branches.csv")).read().splitlines()
    assert thick[2] == BRANCH_CSV_COLUMNS + "," + BRANCH_RADIUS_COLUMNS
    assert [ln.split(",")[:15] for ln in thick[3:]] == [ln.split(",") for ln in btext.splitlines()[3:]]
    from scipy import ndimage
    skel = golden_rows(BLOBS)
    for ln in thick[3:]:
        cells = ln.split(",")
        r = int(cells[1])
        row = want_branches[r]
        dist = ndimage.distance_transform_edt(np.pad(lab == int(cells[0]), 1), sampling=spacing)[1:-1, 1:-1, 1:-1]
        mean, low, high = (float(v) for v in cells[15:])
        inst = skeleton_branches_oracle(skel, ("golden", BLOBS))
        chain = inst[3][inst[4] == r]
        voxels = {tuple(row[11:14]), tuple(row[14:17])} | {tuple(v) for v in chain.tolist()}
        values = [dist[v] for v in voxels]
        # scipy forms the same float64 sums of squares in another order: a few units in the last place
        assert abs(low - min(values)) <= 1e-12 * high and abs(high - max(values)) <= 1e-12 * high
        assert abs(mean - np.mean(values)) <= 1e-12 * high
