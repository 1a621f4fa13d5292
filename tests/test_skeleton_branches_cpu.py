"""The branch tracing on the CPU (no GPU needed): an independent numpy / scipy statement of the definitions of DESIGN.md
section 32 (``skeleton_branches_oracle``: a python walk over dictionaries, junctions and rings from ``scipy.ndimage.label``),
the closed forms of the hand-built skeletons of tests/skeleton_branch_cases.py, the invariants against the rows of the
skeleton-graph oracle on them and on every golden skeleton of tests/golden/skeleton_graph.npz, the golden anchors, and
the host columns of ``validate.compare.branch_columns`` with both CSV texts and the command's flags.

tests/test_hip_skeleton_branches.py and tools/skeleton_branches_host_check.py take the oracle from here."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.skeleton_branch_cases import ROD_VOXELS, cases as branch_cases
from tests.skeleton_graph_cases import LINK_CLASSES, RING_ID, T_ID, cases as graph_cases, positive_ids
from tests.test_skeleton_graph_cpu import golden_rows, skeleton_graph_oracle

N_NODE, N_BRANCH = 8, 18
FULL = np.ones((3, 3, 3), bool)
OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]     # direction code -> (dx, dy, dz)


def _trace(vox):
    """nodes, branches (object-local node rows, object column 0) and owner of ONE object; vox (n, 3) in (x, y, z) order"""
    at = {tuple(v): k for k, v in enumerate(vox.tolist())}
    assert len(at) == len(vox) and vox.tolist() == sorted(vox.tolist())
    links = []                                                   # per voxel: [(code, neighbour)] by ascending code
    for v in vox.tolist():
        links.append([(c, at[(v[0] + d[0], v[1] + d[1], v[2] + d[2])]) for c, d in enumerate(OFFSETS)
                      if c != 13 and (v[0] + d[0], v[1] + d[1], v[2] + d[2]) in at])
    degree = [len(ln) for ln in links]
    lo = vox.min(0) if len(vox) else np.zeros(3, np.int64)
    shape = (vox.max(0) - lo + 1) if len(vox) else (1, 1, 1)

    def components(members):
        """the 26-connected pieces of a set of voxel numbers, each sorted, by scipy"""
        grid = np.zeros(shape, bool)
        grid[tuple((vox[members] - lo).T)] = True
        lab, k = ndimage.label(grid, FULL)
        which = lab[tuple((vox[members] - lo).T)]
        return [sorted(np.asarray(members)[which == j].tolist()) for j in range(1, k + 1)]

    node_of = {}                                                 # node voxel -> first voxel of its node
    members = {}                                                 # first voxel -> voxels of the node
    for k, d in enumerate(degree):
        if d < 2:
            node_of[k], members[k] = k, [k]
    junction_voxels = [k for k, d in enumerate(degree) if d >= 3]
    if junction_voxels:
        for piece in components(junction_voxels):
            members[piece[0]] = piece
            node_of.update({k: piece[0] for k in piece})
    # every walk from a node voxel along a link that is not internal to its node
    walks, visited = [], set()
    for p in sorted(node_of):
        for c, q in links[p]:
            if q in node_of and node_of[q] == node_of[p]:
                continue
            path, codes, prev, cur = [], [c], p, q
            while cur not in node_of:
                path.append(cur)
                (c0, n0), (c1, n1) = links[cur]
                step, nxt = (c1, n1) if n0 == prev else (c0, n0)
                codes.append(step)
                prev, cur = cur, nxt
            visited.update(path)
            walks.append(((p, c), (cur, 26 - codes[-1]), path, codes))
    rings = [k for k, d in enumerate(degree) if d == 2 and k not in visited]
    n_rings = 0
    if rings:
        for piece in components(rings):
            n_rings += 1
            a = piece[0]
            node_of[a], members[a] = a, [a]
            c, q = links[a][0]
            path, codes, prev, cur = [], [c], a, q
            while cur != a:
                path.append(cur)
                (c0, n0), (c1, n1) = links[cur]
                step, nxt = (c1, n1) if n0 == prev else (c0, n0)
                codes.append(step)
                prev, cur = cur, nxt
            assert sorted(path + [a]) == piece and 26 - codes[-1] == links[a][1][0]
            walks.append(((a, c), (a, 26 - codes[-1]), path, codes))
    firsts = sorted(members)
    row_of = {f: r for r, f in enumerate(firsts)}
    kept = sorted((w for w in walks if w[0] < w[1]), key=lambda w: w[0])
    assert 2 * len(kept) == len(walks) + n_rings                       # every branch is walked from both ends
    nodes = np.zeros((len(firsts), N_NODE), np.int64)
    ends = {f: 0 for f in firsts}
    branches = np.zeros((len(kept), N_BRANCH), np.int64)
    owner = np.zeros(len(vox), np.int64)
    for k in node_of:
        owner[k] = -1 - row_of[node_of[k]]
    for r, ((a, c), (b, _), path, codes) in enumerate(kept):
        ends[node_of[a]] += 1
        ends[node_of[b]] += 1
        owner[path] = r
        by_class = [0] * 7
        for code in codes:
            by_class[LINK_CLASSES.index(tuple(abs(d) for d in OFFSETS[code]))] += 1
        branches[r] = [0, row_of[node_of[a]], row_of[node_of[b]], len(path)] + by_class + vox[a].tolist() + \
            vox[b].tolist() + [c]
    for r, f in enumerate(firsts):
        mine = set(members[f])
        internal = sum(1 for k in mine for _, q in links[k] if q in mine and q > k)
        kind = degree[f] if degree[f] < 2 else 3 if degree[f] == 2 else 2
        nodes[r] = [0, kind, len(mine), internal] + vox[f].tolist() + [ends[f]]
    return nodes, branches, owner


_cache = {}


def skeleton_branches_oracle(skel_labels, key=None):
    """(ids (N) int64 ascending, nodes (Nn, 8), branches (Nb, 18), points (P, 3), owner (P)), all int64, of the positive
    labels of a skeleton label volume: the tables of include/skoots_hip.h with the object index = the label's place in
    ``ids``, the points object by object in (x, y, z) order and in volume coordinates.  ``key`` caches the result."""
    if key is not None and key in _cache:
        return _cache[key]
    lab = np.asarray(skel_labels)
    ids = positive_ids(lab)
    nodes, branches, points, owner = [], [], [], []
    n_nodes = n_branches = 0
    for i, obj in enumerate(ids.tolist()):
        vox = np.argwhere(lab == obj)
        nd, br, ow = _trace(vox)
        nd[:, 0], br[:, 0] = i, i
        br[:, 1:3] += n_nodes
        ow = np.where(ow >= 0, ow + n_branches, ow - n_nodes)
        n_nodes, n_branches = n_nodes + len(nd), n_branches + len(br)
        nodes.append(nd), branches.append(br), points.append(vox), owner.append(ow)
    cat = lambda parts, width: np.concatenate(parts) if parts else np.zeros((0, width), np.int64)  # noqa: E731
    out = (ids, cat(nodes, N_NODE), cat(branches, N_BRANCH), cat(points, 3),
           np.concatenate(owner) if owner else np.zeros(0, np.int64))
    for a in out:
        a.setflags(write=False)
    if key is not None:
        _cache[key] = out
    return out


def golden_skeleton(name):
    """the golden skeleton of a case of tests/skeleton_graph_cases.py with the instances' rows 1 .. N as labels"""
    return golden_rows(name)


def branch_summary(nodes, branches):
    """(nodes by type 0..3, branches, self-loops, corner loops, rings) of one object's rows"""
    self_loops = branches[branches[:, 1] == branches[:, 2]]
    gap = np.abs(self_loops[:, 11:14] - self_loops[:, 14:17]).max(1) if len(self_loops) else np.zeros(0)
    corner = int(((self_loops[:, 3] == 1) & (gap == 1)).sum())
    rings = int((nodes[:, 1] == 3).sum())
    return [int((nodes[:, 1] == t).sum()) for t in range(4)], len(branches), len(self_loops), corner, rings


def check_invariants(lab, name, key="inv"):
    """the invariants of DESIGN.md section 32 on every object of a skeleton label volume, against the graph oracle"""
    ids, nodes, branches, points, owner = skeleton_branches_oracle(lab, (key, name))
    gids, graph = skeleton_graph_oracle(lab)
    assert np.array_equal(ids, gids)
    offsets = np.concatenate(([0], np.cumsum(graph[:, 0])))
    assert len(points) == offsets[-1] == len(owner)
    for i, obj in enumerate(ids.tolist()):
        nd, br, g = nodes[nodes[:, 0] == i], branches[branches[:, 0] == i], graph[i]
        assert br[:, 4:11].sum() + nd[:, 3].sum() == g[5:].sum(), (name, obj)
        assert br[:, 3].sum() + nd[:, 2].sum() == g[0], (name, obj)
        assert nd[nd[:, 1] == 2][:, 2].sum() == g[4] and (nd[:, 1] == 1).sum() == g[2] and (nd[:, 1] == 0).sum() == g[1]
        assert 2 * len(br) == nd[:, 7].sum()
        components = ndimage.label(np.asarray(lab) == obj, FULL)[1]
        junctions = nd[nd[:, 1] == 2]
        assert g[5:].sum() - g[0] + components == \
            len(br) - len(nd) + components + (junctions[:, 3] - junctions[:, 2] + 1).sum(), (name, obj)
        # the order of the rows, and what the owner says
        assert nd[:, 4:7].tolist() == sorted(nd[:, 4:7].tolist())
        keys = [tuple(r[11:14]) + (r[17],) for r in br.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        ow = owner[offsets[i]:offsets[i + 1]]
        first_branch = int((branches[:, 0] < i).sum())
        assert np.array_equal(np.bincount(ow[ow >= 0] - first_branch, minlength=len(br)), br[:, 3])
        first_node = int((nodes[:, 0] < i).sum())
        assert np.array_equal(np.bincount(-1 - ow[ow < 0] - first_node, minlength=len(nd)), nd[:, 2])


def _one(name, obj=None):
    """(nodes, branches) of one object of a hand-built case"""
    lab = branch_cases()[name]
    ids, nodes, branches, _, _ = skeleton_branches_oracle(lab, ("case", name))
    i = 0 if obj is None else ids.tolist().index(obj)
    return nodes[nodes[:, 0] == i], branches[branches[:, 0] == i]


def test_rods_pairs_and_single_voxels():
    for obj, cls in ((3, 6), (4, 2)):
        nd, br = _one("rods", obj)
        assert nd[:, 1].tolist() == [1, 1] and nd[:, 2:4].tolist() == [[1, 0], [1, 0]] and nd[:, 7].tolist() == [1, 1]
        links = [0] * 7
        links[cls] = ROD_VOXELS - 1
        assert br[:, 3].tolist() == [ROD_VOXELS - 2] and br[0, 4:11].tolist() == links
        assert br[0, 1] + 1 == br[0, 2] and br[0, 11:14].tolist() == nd[0, 4:7].tolist()
    nd, br = _one("two voxels")
    assert nd[:, 1].tolist() == [1, 1] and br[:, 3].tolist() == [0] and br[0, 4:11].sum() == 1 and br[0, 17] == 26
    nd, br = _one("one voxel")
    assert nd.tolist() == [[0, 0, 1, 0, 0, 2, 1, 0]] and len(br) == 0
    for name in ("extent one (1, 1, 9)", "extent one (6, 1, 1)", "extent one (1, 7, 1)"):
        nd, br = _one(name)
        n = max(branch_cases()[name].shape)
        assert nd[:, 1].tolist() == [1, 1] and br[:, 3].tolist() == [n - 2] and br[0, 4:11].sum() == n - 1


def test_rings():
    nd, br = _one("ring of ten")
    assert nd.tolist() == [[0, 3, 1, 0, 2, 1, 30, 2]]
    assert br[:, 3].tolist() == [9] and br[0, 4:11].sum() == 10 and br[0, 1] == br[0, 2]
    assert br[0, 11:14].tolist() == br[0, 14:17].tolist() == [2, 1, 30]
    assert br[0, 17] == 9 + 3 * 1 + 2                            # of (0, 0, +1) and (0, +1, -1) the smaller code
    nd, br = _one("triangle")
    assert nd[:, 1].tolist() == [3] and br[:, 3].tolist() == [2] and br[0, 4:11].sum() == 3
    assert branch_summary(nd, br)[2:] == (1, 0, 1)               # a self-loop of two chain voxels: no corner loop


def test_junctions_of_several_voxels():
    nd, br = _one("jog")
    assert sorted(nd[:, 1].tolist()) == [1, 1, 2] and nd[nd[:, 1] == 2][0, 2:4].tolist() == [4, 5]
    assert br[:, 3].tolist() == [3, 3] and br[:, 4:11].sum(1).tolist() == [4, 4]
    nd, br = _one("spur")
    assert sorted(nd[:, 1].tolist()) == [1, 1, 2] and nd[nd[:, 1] == 2][0, 2:4].tolist() == [4, 5]
    assert sorted(br[:, 3].tolist()) == [3, 4]
    # the plain corner: its two neighbours of the corner voxel are the junction, the corner voxel a corner loop
    nd, br = _one("corner")
    assert sorted(nd[:, 1].tolist()) == [1, 1, 2] and nd[nd[:, 1] == 2][0, 2:4].tolist() == [2, 1]
    assert sorted(br[:, 3].tolist()) == [1, 3, 4] and branch_summary(nd, br)[2:] == (1, 1, 0)
    nd, br = _one("solid 5")
    assert nd.tolist() == [[0, 2, 125, 1036, 0, 0, 0, 0]] and len(br) == 0
    nd, br = _one("solid 5 with an arm")
    assert nd[:, 1:4].tolist() == [[2, 126, 1045], [1, 1, 0]] and br[:, 3].tolist() == [3]
    assert br[0, 1:3].tolist() == [0, 1] and br[0, 4:11].tolist() == [0, 0, 4, 0, 0, 0, 0]


def test_theta_lollipop_and_self_loops():
    nd, br = _one("theta")
    assert nd[:, 1:4].tolist() == [[2, 1, 0], [2, 1, 0]] and nd[:, 7].tolist() == [3, 3]
    assert br[:, 1:3].tolist() == [[0, 1]] * 3                   # three parallel branches between the same two nodes
    codes = br[:, 17].tolist()
    assert codes == sorted(codes) and len(set(codes)) == 3 and (br[:, 11:14] == br[0, 11:14]).all()
    assert br[:, 3].tolist() == [15, 9, 15]                      # by direction code: y - 1 first, then z + 1, then y + 1
    nd, br = _one("lollipop")
    assert nd[:, 1].tolist() == [1, 2] and nd[:, 7].tolist() == [1, 3]
    loop = br[br[:, 1] == br[:, 2]]
    assert len(br) == 2 and len(loop) == 1 and loop[0, 3] == 9 and loop[0, 4:11].sum() == 10
    assert loop[0, 11:14].tolist() == loop[0, 14:17].tolist()    # it leaves and re-enters the same junction voxel
    assert branch_summary(nd, br)[2:] == (1, 0, 0)


def test_ids_do_not_link_and_pieces_of_one_id():
    lab = branch_cases()["lines"]
    ids, nodes, branches, _, _ = skeleton_branches_oracle(lab, ("case", "lines"))
    assert len(ids) == 9 and len(branches) == 9 and (nodes[:, 1] == 1).all() and len(nodes) == 18
    assert branches[:, 3].tolist() == [7] * 9                    # also the two that touch diagonally all along
    nd, br = _one("rings and pieces", 7)
    assert branch_summary(nd, br) == ([1, 4, 0, 2], 4, 2, 0, 2)
    assert sorted(br[:, 3].tolist()) == [0, 5, 9, 9]
    ids = skeleton_branches_oracle(branch_cases()["huge ids"], ("case", "huge ids"))[0]
    assert ids.tolist() == [70000, 2 ** 31 - 1, 2 ** 40]
    nd, br = _one("huge ids", 2 ** 40)
    assert br[:, 3].tolist() == [32]


def test_invariants_on_every_hand_built_case():
    for name, lab in branch_cases().items():
        check_invariants(lab, name)


def test_invariants_on_every_golden_skeleton():
    total = 0
    for name in graph_cases():
        skel = golden_skeleton(name)
        check_invariants(skel, name, "golden")
        total += len(positive_ids(skel))
    assert total == 54


def _golden_object(name, obj):
    lab = graph_cases()[name]
    row = positive_ids(lab).tolist().index(obj) + 1
    skel = golden_skeleton(name)
    ids, nodes, branches, _, _ = skeleton_branches_oracle(skel, ("golden", name))
    i = ids.tolist().index(row)
    return nodes[nodes[:, 0] == i], branches[branches[:, 0] == i], skeleton_graph_oracle(skel)[1][i]


def test_golden_anchors():
    nd, br, _ = _golden_object("blobs (24, 40, 70)", T_ID)
    assert len(nd) == 4 and len(br) == 3 and len(br) - len(nd) + 1 == 0
    nd, br, _ = _golden_object("blobs (24, 40, 70)", RING_ID)
    assert nd[:, 1].tolist() == [3] and br[:, 3].tolist() == [59] and br[0, 4:11].sum() == 60
    nd, br, g = _golden_object("cross (9, 11, 37)", 4)
    assert g[0] == 51 and g[4] == 7
    assert len(nd) == 7 and nd[nd[:, 1] == 2][:, 2].tolist() == [7] and len(br) == 6 and len(br) - len(nd) + 1 == 0
    links = g[5:].sum()
    assert links - g[3] == 24 and links - g[0] + 1 == 12         # what the counts alone say: 24 branches, 12 loops


# ---- the host layers: validate.compare.branch_columns, the CSV texts, the flags ----

SPACINGS = ((1.0, 1.0, 1.0), (0.5, 0.7, 3.0))


def _tables(name, golden=False):
    """(lab, ids, nodes, branches) of a case as torch tensors, column 0 the object's index"""
    lab = golden_skeleton(name) if golden else branch_cases()[name]
    ids, nodes, branches, _, _ = skeleton_branches_oracle(lab, ("golden" if golden else "case", name))
    return lab, ids, torch.from_numpy(nodes.astype(np.int32)), torch.from_numpy(branches.astype(np.int32))


def test_branch_columns_closed_forms():
    from skoots_amd.validate.compare import BRANCH_COLUMNS, branch_columns
    want = {"corner": (1, 2, 1, 3, 0, 1, 0), "theta": (1, 0, 2, 3, 0, 0, 2), "lollipop": (1, 1, 1, 2, 0, 0, 1),
            "triangle": (1, 0, 0, 1, 1, 0, 1), "one voxel": (1, 0, 0, 0, 0, 0, 0), "solid 5": (1, 0, 1, 0, 0, 0, 0),
            "jog": (1, 2, 1, 2, 0, 0, 0)}
    names = BRANCH_COLUMNS.split(",")
    for name, numbers in want.items():
        _, ids, nodes, branches = _tables(name)
        col = branch_columns(nodes, branches, len(ids))
        assert list(col) == names and all(col[k].dtype == torch.int64 for k in names[:7])
        assert all(col[k].dtype == torch.float64 for k in names[7:])
        assert tuple(col[k][0].item() for k in names[:7]) == numbers, name
    _, ids, nodes, branches = _tables("rings and pieces")
    col = branch_columns(nodes, branches, len(ids))
    assert [col[k][0].item() for k in names[:7]] == [5, 4, 0, 4, 2, 0, 2]
    assert [col[k][1].item() for k in names[:7]] == [1, 2, 0, 1, 0, 0, 0]
    nd, br, _ = _golden_object("cross (9, 11, 37)", 4)
    col = branch_columns(torch.from_numpy(nd), torch.from_numpy(br), 1)
    assert [col[k][0].item() for k in names[:7]] == [1, 6, 1, 6, 0, 0, 0]


def test_graph_components_against_scipy():
    from skoots_amd.validate.compare import branch_columns
    for golden, names in ((False, branch_cases()), (True, graph_cases())):
        for name in names:
            lab, ids, nodes, branches = _tables(name, golden)
            got = branch_columns(nodes, branches, len(ids))["graph_components"].tolist()
            assert got == [ndimage.label(np.asarray(lab) == obj, FULL)[1] for obj in ids.tolist()], name


def test_branch_lengths_and_empty_rows():
    from skoots_amd.validate.compare import branch_columns, branch_lengths
    _, ids, nodes, branches = _tables("rods")
    for spacing in SPACINGS:
        step = [math.sqrt(sum((d * s) ** 2 for d, s in zip(c, spacing))) for c in LINK_CLASSES]
        lengths = branch_lengths(branches, spacing)
        assert lengths.dtype == torch.float64
        assert lengths.tolist() == [(ROD_VOXELS - 1) * step[6], (ROD_VOXELS - 1) * step[2]]
        col = branch_columns(nodes, branches, 4, spacing)        # two more instances whose skeletons are empty
        assert col["graph_length"].tolist() == lengths.tolist() + [0.0, 0.0]
        assert col["branch_length_mean"].tolist() == lengths.tolist() + [0.0, 0.0]
        assert col["longest_branch"].tolist() == lengths.tolist() + [0.0, 0.0]
        assert col["graph_branches"].tolist() == [1, 1, 0, 0] and col["graph_cycles"].tolist() == [0, 0, 0, 0]
    _, ids, nodes, branches = _tables("theta")
    col = branch_columns(nodes, branches, 1, (0.5, 0.7, 3.0))
    each = branch_lengths(branches, (0.5, 0.7, 3.0))
    assert col["longest_branch"][0].item() == each.max().item() and each[0].item() == each[2].item() > each[1].item()
    assert abs(col["graph_length"][0].item() - each.sum().item()) <= 1e-12 * each.sum().item()
    assert col["branch_length_mean"][0].item() == col["graph_length"][0].item() / 3
    empty = branch_columns(torch.zeros((0, 8), dtype=torch.int32), torch.zeros((0, 18), dtype=torch.int32), 2)
    assert all(v.tolist() == [0, 0] for v in empty.values())
    with pytest.raises(ValueError):
        branch_columns(nodes, branches, 1, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        branch_columns(nodes, branches, 0)


def test_branch_and_node_csv_texts():
    from skoots_amd.validate.compare import (BRANCH_CSV_COLUMNS, BRANCH_KINDS, NODE_CSV_COLUMNS, branch_kinds,
                                             format_branches_csv, format_nodes_csv)
    _, ids, nodes, branches = _tables("rings and pieces")
    text = format_branches_csv("m.tif", ids, nodes, branches, (0.5, 0.7, 3.0)).splitlines()
    assert text[0] == "Mask File: m.tif" and text[1] == "Spacing: 0.5 0.7 3.0" and text[2] == BRANCH_CSV_COLUMNS
    assert len(text) == 3 + 5
    rows = [ln.split(",") for ln in text[3:]]
    assert [r[0] for r in rows] == ["7"] * 4 + ["13"] and [r[1] for r in rows] == [str(k) for k in range(5)]
    assert sorted(r[2] for r in rows) == ["endpoint-endpoint"] * 3 + ["ring"] * 2
    ring = next(r for r in rows if r[2] == "ring")
    assert ring[3] == ring[4] and ring[5] == "9" and ring[7] == "0.0" and ring[8] == "" and ring[9:12] == ring[12:15]
    rod = rows[-1]                                               # id 13: four voxels along z
    assert rod[5:9] == ["2", "9.0", "9.0", "1.0"] and rod[9:] == ["3", "5", "20", "3", "5", "23"]
    kept = format_branches_csv("m.tif", ids, nodes, branches, (0.5, 0.7, 3.0), keep=[False, True]).splitlines()
    assert kept[:3] == text[:3] and kept[3:] == text[-1:]
    radius = np.arange(15, dtype=np.float64).reshape(5, 3) / 4
    with_r = format_branches_csv("m.tif", ids, nodes, branches, (0.5, 0.7, 3.0), radius=radius).splitlines()
    assert with_r[2] == BRANCH_CSV_COLUMNS + ",radius_mean,radius_min,radius_max"
    assert [ln.split(",")[:15] for ln in with_r[3:]] == rows and with_r[4].split(",")[15:] == ["0.75", "1.0", "1.25"]
    ntext = format_nodes_csv("m.tif", ids, nodes).splitlines()
    assert ntext[0] == "Mask File: m.tif" and ntext[1] == NODE_CSV_COLUMNS and len(ntext) == 2 + 9
    assert ntext[2].split(",") == ["7", "0", "ring-anchor", "1", "0", "1", "1", "30", "2"]
    assert sorted(ln.split(",")[2] for ln in ntext[2:]) == ["endpoint"] * 6 + ["isolated"] + ["ring-anchor"] * 2
    assert format_nodes_csv("m.tif", ids, nodes, keep=[False, True]).splitlines()[2:] == ntext[-2:]
    # every kind once
    kinds = {}
    for name in ("corner", "lollipop", "theta", "solid 5 with an arm", "ring of ten", "two voxels"):
        _, _, nd, br = _tables(name)
        kinds[name] = sorted(BRANCH_KINDS[k] for k in branch_kinds(nd, br).tolist())
    assert kinds == {"corner": ["corner-loop", "endpoint-junction", "endpoint-junction"],
                     "lollipop": ["endpoint-junction", "self-loop"], "theta": ["junction-junction"] * 3,
                     "solid 5 with an arm": ["endpoint-junction"], "ring of ten": ["ring"],
                     "two voxels": ["endpoint-endpoint"]}


def test_format_csv_with_and_without_the_branch_columns():
    from skoots_amd.validate.compare import BRANCH_COLUMNS, format_csv
    from tests.test_skeleton_graph_cpu import _measured
    ids, sums, boxes, graph = _measured()
    shape, spacing = (8, 8, 8), (0.5, 0.7, 3.0)
    plain = format_csv("m.tif", ids, sums, boxes, shape, spacing)
    assert format_csv("m.tif", ids, sums, boxes, shape, spacing, branch_tables=None) == plain
    nodes = torch.tensor([[0, 1, 1, 0, 0, 1, 1, 1], [0, 1, 1, 0, 3, 1, 1, 1], [1, 0, 1, 0, 5, 5, 5, 0]], dtype=torch.int32)
    branches = torch.tensor([[0, 0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 1, 1, 3, 1, 1, 22]], dtype=torch.int32)
    old = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph).splitlines()
    new = format_csv("m.tif", ids, sums, boxes, shape, spacing, skeleton_graph=graph,
                     branch_tables=(nodes, branches)).splitlines()
    assert new[:2] == old[:2] and new[2] == old[2] + "," + BRANCH_COLUMNS
    assert [ln.split(",")[:22] for ln in new[3:]] == [ln.split(",") for ln in old[3:]]
    assert new[3].split(",")[22:] == ["1", "2", "0", "1", "0", "0", "0", "1.5", "1.5", "1.5"]
    assert new[4].split(",")[22:] == ["1", "0", "0", "0", "0", "0", "0", "0.0", "0.0", "0.0"]


def test_cli_flags():
    from skoots_amd.validate.compare import parse_args
    a = parse_args(["m.tif"])
    assert a.branches is False and a.skeleton_from is None and a.skeleton is False
    a = parse_args(["m.tif", "--skeleton"])
    assert a.branches is False and a.skeleton is True
    a = parse_args(["m.tif", "--branches"])
    assert a.branches is True and a.skeleton is True and a.save_skeletons is False   # --branches implies --skeleton
    a = parse_args(["m.tif", "--branches", "--skeleton-from", "s.tif", "--thickness", "closed"])
    assert a.skeleton_from == "s.tif" and a.thickness == "closed"
    for bad in (["m.tif", "--skeleton-from", "s.tif"], ["m.tif", "--branches", "yes"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2
