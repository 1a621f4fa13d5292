"""The numpy statement of what ``sk_instance_mesh_count`` / ``sk_instance_mesh_emit`` and ``instance_meshes`` give
(DESIGN.md section 24), and the shapes they are checked on.  tests/test_mesh_cpu.py compares the oracle
with scikit-image's own meshes (tests/golden/mesh.npz), tests/test_hip_mesh.py and
tools/instance_mesh_emit_host_check.py compare the kernels with the oracle.

``mesh_oracle(mask, id, closed)`` applies ``mc_triangles.TRIANGLES`` cell by cell to ``mask == id`` and returns the
mesh in the library's canonical order: vertices (V, 3) int32 in DOUBLED index coordinates, ascending by edge key;
faces (F, 3) int32 indices into them, ascending by order key, each in scikit-image's vertex order."""
import os

import numpy as np

from skoots_amd.validate.mc_triangles import EDGES, TRIANGLES
from tests.test_hip_surface_area import cases as surface_cases
from tests.test_surface_area_cpu import config_volume

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

N_TRI = np.array([len(t) for t in TRIANGLES], np.int64)
TRI = np.zeros((256, 5, 3), np.int64)
for _c, _t in enumerate(TRIANGLES):
    if _t:
        TRI[_c, :len(_t)] = _t
EDGE_AXIS = np.array([a for a, _ in EDGES], np.int64)
EDGE_LOW = np.array([[(b >> k) & 1 for k in range(3)] for _, b in EDGES], np.int64)    # the low corner's offset


def edge_keys(doubled, shape):
    """edge key of vertices given as (..., 3) doubled coordinates in a volume of ``shape``: the linear index of the
    edge's low voxel in the volume padded by one layer, times 3, plus the axis"""
    d = np.asarray(doubled).astype(np.int64)
    axis = np.argmax(d & 1, axis=-1)
    v = (d >> 1) + 1                                         # floor: -1 / 2 -> -1, the layer before the volume
    _, Y, Z = (int(s) for s in shape)
    return ((v[..., 0] * (Y + 2) + v[..., 1]) * (Z + 2) + v[..., 2]) * 3 + axis


def _cell_triangles(lab, u, closed):
    """(doubled (F, 3, 3), edge keys (F, 3), order keys (F)) of the triangles of ``lab == u``, ascending by order key.
    Only the box of the id, grown by one voxel, is looked at: no other cell can hold a corner of it."""
    lab = np.asarray(lab)
    shape = lab.shape
    empty = np.zeros((0, 3, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    at = np.argwhere(lab == u)
    if at.size == 0:
        return empty
    # the corner voxels that exist: 0 .. extent - 1 (open) or -1 .. extent (closed)
    first, last = (-1, np.array(shape)) if closed else (0, np.array(shape) - 1)
    lo, hi = np.maximum(at.min(0) - 1, first), np.minimum(at.max(0) + 1, last)
    m = np.zeros(hi - lo + 1, bool)
    a, b = np.maximum(lo, 0), np.minimum(hi, np.array(shape) - 1)
    m[a[0] - lo[0]:b[0] - lo[0] + 1, a[1] - lo[1]:b[1] - lo[1] + 1, a[2] - lo[2]:b[2] - lo[2] + 1] = \
        lab[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1] == u
    if min(m.shape) < 2:
        return empty
    cfg = config_volume(m)
    cells = np.argwhere((cfg != 0) & (cfg != 255))           # ascending (x, y, z): ascending order key
    c = cfg[tuple(cells.T)].astype(np.int64)
    n = N_TRI[c]
    rep = np.repeat(np.arange(len(cells)), n)
    j = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    e = TRI[c[rep], j]                                       # (F, 3) edge numbers
    corner = cells[rep] + lo                                 # (F, 3) the cell's low corner voxel
    vox = corner[:, None, :] + EDGE_LOW[e]                   # (F, 3, 3) low voxel of every vertex's edge
    doubled = 2 * vox + np.eye(3, dtype=np.int64)[EDGE_AXIS[e]]
    _, Y, Z = (int(v) for v in shape)
    order = (((corner[:, 0] + 1) * (Y + 2) + corner[:, 1] + 1) * (Z + 2) + corner[:, 2] + 1) * 8 + j
    return doubled, edge_keys(doubled, shape), order


def mesh_oracle(lab, u, closed):
    """(vertices (V, 3) int32 doubled, faces (F, 3) int32 local) of ``lab == u`` in the canonical order"""
    doubled, keys, _ = _cell_triangles(lab, u, closed)
    if len(keys) == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32)
    _, first_at, inverse = np.unique(keys.reshape(-1), return_index=True, return_inverse=True)
    vertices = doubled.reshape(-1, 3)[first_at].astype(np.int32)
    return vertices, inverse.reshape(-1, 3).astype(np.int32)


def record_oracle(lab, closed):
    """(ids, counts (N, 2), vertex records (V, 2), triangle records (F, 5)) int64: what ``sk_instance_mesh_count`` and
    ``sk_instance_mesh_emit`` give a volume, the records sorted by (row, edge key) and by (row, order key).  The vertex
    records come from the crossing edges themselves, not from the triangles."""
    lab = np.asarray(lab)
    ids = np.unique(lab)
    ids = ids[ids > 0].astype(np.int64)
    X, Y, Z = lab.shape
    padded = np.zeros((X + 2, Y + 2, Z + 2), np.int64)
    padded[1:-1, 1:-1, 1:-1] = np.searchsorted(ids, lab) + 1
    padded[1:-1, 1:-1, 1:-1][lab <= 0] = 0
    inside = np.zeros(padded.shape, bool)                    # the corner voxels of the cell range
    inside[...] = True if closed else False
    inside[1:-1, 1:-1, 1:-1] = True
    index = np.arange(padded.size, dtype=np.int64).reshape(padded.shape)
    vrec = [np.zeros((0, 2), np.int64)]
    for axis in range(3):
        lo_sl = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        hi_sl = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        r0, r1 = padded[lo_sl], padded[hi_sl]
        ok = inside[lo_sl] & inside[hi_sl] & (r0 != r1)
        for r in (r0, r1):
            sel = ok & (r > 0)
            vrec.append(np.stack((r[sel], index[lo_sl][sel] * 3 + axis), 1))
    vrec = np.concatenate(vrec)
    if min(X, Y, Z) < 2 and not closed:
        vrec = vrec[:0]                                      # no cell: no mesh
    vrec = vrec[np.lexsort((vrec[:, 1], vrec[:, 0]))]
    trec = [np.zeros((0, 5), np.int64)]
    for row, u in enumerate(ids, 1):
        _, keys, order = _cell_triangles(lab, u, closed)
        trec.append(np.concatenate((np.full((len(keys), 1), row), keys, order[:, None]), 1))
    trec = np.concatenate(trec)
    counts = np.stack((np.bincount(vrec[:, 0], minlength=len(ids) + 1)[1:],
                       np.bincount(trec[:, 0], minlength=len(ids) + 1)[1:]), 1).astype(np.int64)
    return ids, counts, vrec, trec


def canonical_triangles(vertices, faces):
    """(F, 3, 3) int64: the triangles as doubled coordinates, each rotated so that its smallest vertex (x, then y,
    then z) comes first -- the orientation stays -- and the rows sorted: the form tests/golden/mesh.npz stores"""
    t = np.asarray(vertices).astype(np.int64)[np.asarray(faces).astype(np.int64)].reshape(-1, 3, 3)
    if len(t) == 0:
        return t
    rank = (t[..., 0] * 2 ** 20 + t[..., 1]) * 2 ** 20 + t[..., 2]
    k = np.argmin(rank, axis=1)
    t = t[np.arange(len(t))[:, None], (k[:, None] + np.arange(3)) % 3]
    flat = t.reshape(len(t), 9)
    return t[np.lexsort(flat.T[::-1])]


def crossing_edges(lab, u, closed):
    """number of axis-neighbour voxel pairs with exactly one voxel of ``u``, the mask padded when ``closed``"""
    m = np.asarray(lab) == u
    if closed:
        m = np.pad(m, 1)
    if min(m.shape) < 2:
        return 0
    return int(sum((np.diff(m.astype(np.int8), axis=a) != 0).sum() for a in range(3)))


def euler_characteristic(vertices, faces):
    assert len(faces) % 2 == 0
    return len(vertices) - len(faces) // 2


def signed_volume6(vertices, faces):
    """sum of det(v0, v1, v2) in doubled coordinates: 48 times the enclosed volume, by sign of the winding"""
    t = np.asarray(vertices).astype(np.int64)[np.asarray(faces).astype(np.int64)].reshape(-1, 3, 3)
    return int(np.linalg.det(t.astype(np.float64)).round().astype(np.int64).sum()) if len(t) else 0


def directed_edges_pair_up(faces):
    """every directed edge of the triangles has its reverse exactly once, and itself exactly once"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 1
    fwd, rev = np.sort(a[:, 0] * n + a[:, 1]), np.sort(a[:, 1] * n + a[:, 0])
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(fwd, rev)


# ---- the fixture ----

def fixture_cases(g):
    """(name, mask (X, Y, Z), ids) of tests/golden/mesh.npz; the meshes are g[f"{name}_{id}_{open|closed}_tri"] and
    g[f"{name}_{id}_{open|closed}_v"]"""
    inst = np.load(os.path.join(GOLDEN, "instance_stats.npz"))
    area = np.load(os.path.join(GOLDEN, "surface_area.npz"))
    for name in g["names"].tolist():
        if name == "instance_stats":
            mask = inst["mask"][0]
        elif name == "ellipsoids":
            mask = area["ellipsoids_mask"]
        else:
            mask = g[name + "_mask"]
        yield name, mask, g[name + "_ids"].tolist()


# ---- the shapes of the device tests ----

def cases():
    """name -> (X, Y, Z) int32 array: the shapes of tests/test_hip_surface_area.py, which straddle the 4 x 16 x 64 tile,
    and one more whose cell range in closed mode ends exactly on a tile (3 + 1, 15 + 1 and 63 + 1 cells), so that the
    positions on the high faces are tiles of their own"""
    out = dict(surface_cases())
    out["checkerboard (3, 15, 63)"] = (np.indices((3, 15, 63)).sum(0) % 2 + 1).astype(np.int32)
    return out


def oracle_all(lab, closed):
    """(ids, vertices, faces, vertex_offsets, face_offsets) as ``instance_meshes`` returns them, from ``mesh_oracle``"""
    lab = np.asarray(lab)
    ids = np.unique(lab)
    ids = ids[ids > 0].astype(np.int64)
    vs, fs = [np.zeros((0, 3), np.int32)], [np.zeros((0, 3), np.int32)]
    vo, fo = [0], [0]
    for u in ids:
        v, f = mesh_oracle(lab, u, closed)
        vs.append(v)
        fs.append(f)
        vo.append(vo[-1] + len(v))
        fo.append(fo[-1] + len(f))
    return ids, np.concatenate(vs), np.concatenate(fs), np.array(vo, np.int64), np.array(fo, np.int64)
