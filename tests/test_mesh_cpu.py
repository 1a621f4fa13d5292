"""Host side of the per-instance meshes, without a GPU: the triangle table
(skoots_amd/validate/mc_triangles.py), the numpy oracle of tests/mesh_cases.py against scikit-image's own meshes
(tests/golden/mesh.npz, exactly), the PLY writer and the CSV text."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from skoots_amd.validate.mc_table import CLASS_OF, CLASS_TRIANGLES, NO_CLASS, TRIANGLE_TYPES
from skoots_amd.validate.mc_triangles import EDGES, TRIANGLES
from tests import mesh_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("open", False), ("closed", True))


def read_ply(path):
    """A parser of exactly the layout ``write_ply`` promises: (header lines, x y z float32 (V, 3), vertex instance (V),
    faces (F, 3) global int32, face instance (F))."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0" and header[-1] == "end_header"
    body = [ln for ln in header[2:-1] if not ln.startswith("comment ")]
    V, F = int(body[0].split()[-1]), int(body[5].split()[-1])
    assert body == [f"element vertex {V}", "property float x", "property float y", "property float z",
                    "property int instance", f"element face {F}", "property list uchar int vertex_indices",
                    "property int instance"]
    assert len(data) == end + 16 * V + 17 * F
    xyz, vid = np.zeros((V, 3), np.float32), np.zeros(V, np.int64)
    for i in range(V):
        *xyz[i], vid[i] = struct.unpack_from("<fffi", data, end + 16 * i)
    faces, fid = np.zeros((F, 3), np.int64), np.zeros(F, np.int64)
    for i in range(F):
        n, *faces[i], fid[i] = struct.unpack_from("<Biiii", data, end + 16 * V + 17 * i)
        assert n == 3
    return header, xyz, vid, faces, fid


def test_table_shape_and_tool_assertions():
    assert len(EDGES) == 12 and len(set(EDGES)) == 12
    assert EDGES == tuple((axis, b) for axis in range(3) for b in range(8) if not (b >> axis) & 1)
    assert len(TRIANGLES) == 256 and TRIANGLES[0] == () and TRIANGLES[255] == ()
    for c in range(1, 255):
        tris = TRIANGLES[c]
        assert 1 <= len(tris) <= 5, c
        for t in tris:
            assert len(t) == 3 and len(set(t)) == 3 and all(0 <= e < 12 for e in t), (c, t)
            for e in t:                                       # a vertex lies between a corner inside and one outside
                axis, low = EDGES[e]
                assert ((c >> low) & 1) != ((c >> (low | 1 << axis)) & 1), (c, t)
        used = {e for t in tris for e in t}                   # every crossing edge of the cell carries a vertex
        crossing = {e for e, (axis, low) in enumerate(EDGES) if ((c >> low) & 1) != ((c >> (low | 1 << axis)) & 1)}
        assert used == crossing, c


def test_table_reproduces_the_classes():
    """4 |cross product| of every triangle, as the integer triples of mc_table.py: per configuration the multiset is
    that of its class"""
    mid = np.array([[2 * ((low >> k) & 1) + (k == axis) for k in range(3)] for axis, low in EDGES], np.int64)
    for c in range(256):
        counts = [0] * len(TRIANGLE_TYPES)
        for t in TRIANGLES[c]:
            p, q, r = mid[list(t)]                            # doubled coordinates: the cross product is 4 x
            cross = tuple(int(v) for v in np.abs(np.cross(q - p, r - p)))
            assert cross != (0, 0, 0), (c, t)
            counts[TRIANGLE_TYPES.index(cross)] += 1
        if c in (0, 255):
            assert CLASS_OF[c] == NO_CLASS and sum(counts) == 0
        else:
            assert tuple(counts) == CLASS_TRIANGLES[CLASS_OF[c]], c


def _boundary(tris):
    """directed edges of the patch that no neighbouring triangle takes back: its oriented rim"""
    d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(d)) == len(d)
    return sorted(e for e in d if (e[1], e[0]) not in d)


def test_table_is_mirror_consistent():
    """The mirror image of a configuration along x, y or z has the mirror image of its surface patch with the
    orientation reversed: as many triangles, and the patch's oriented rim (the directed edges no second triangle takes
    back) is the mirrored rim run backwards.  Inside the rim scikit-image may cut a polygon along another diagonal,
    so the triangles themselves are not compared; test_table_reproduces_the_classes pins their areas."""
    def mirrored(c, axis):
        return sum(((c >> b) & 1) << (b ^ (1 << axis)) for b in range(8))

    def mirror_edge(e, axis):
        a, low = EDGES[e]
        return e if a == axis else EDGES.index((a, low ^ (1 << axis)))

    for axis in range(3):
        for c in range(256):
            m = TRIANGLES[mirrored(c, axis)]
            want = sorted((mirror_edge(b, axis), mirror_edge(a, axis)) for a, b in _boundary(TRIANGLES[c]))
            assert len(m) == len(TRIANGLES[c]) and _boundary(m) == want, (axis, c)


def test_packed_table():
    from skoots_amd.validate.lib import packed_triangle_table
    t = packed_triangle_table()
    assert t.dtype == np.uint64 and t.shape == (256,)
    for c in range(256):
        v = int(t[c])
        assert v >> 60 == len(TRIANGLES[c])
        got = tuple(tuple((v >> (4 * (3 * j + i))) & 15 for i in range(3)) for j in range(len(TRIANGLES[c])))
        assert got == TRIANGLES[c]
        assert (v & ((1 << 60) - 1)) >> (12 * len(TRIANGLES[c])) == 0


def test_oracle_equals_scikit_image_exactly(golden):
    g = golden("mesh.npz")
    names = []
    for name, mask, ids in M.fixture_cases(g):
        names.append(name)
        for u in ids:
            for mode, closed in MODES:
                v, f = M.mesh_oracle(mask, u, closed)
                want = g[f"{name}_{u}_{mode}_tri"]
                assert want.dtype == np.int16
                got = M.canonical_triangles(v, f)
                assert got.shape == want.shape and np.array_equal(got, want), (name, u, mode)
                assert len(v) == int(g[f"{name}_{u}_{mode}_v"]) == M.crossing_edges(mask, u, closed), (name, u, mode)
                # the canonical order: vertices ascending by edge key, every one referenced
                keys = M.edge_keys(v, mask.shape)
                assert np.all(np.diff(keys) > 0) and np.array_equal(np.unique(f), np.arange(len(v)))
    assert names == ["instance_stats", "noise", "ellipsoids", "ball", "hollow_ball", "torus"]
    assert os.path.getsize(os.path.join(M.GOLDEN, "mesh.npz")) < os.path.getsize(os.path.join(M.GOLDEN, "augment.npz"))


def test_closed_meshes_are_manifold_with_known_euler_characteristic(golden):
    g = golden("mesh.npz")
    chi = {}
    for name, mask, ids in M.fixture_cases(g):
        for u in ids:
            v, f = M.mesh_oracle(mask, u, True)
            assert M.directed_edges_pair_up(f), (name, u)
            assert M.signed_volume6(v, f) < 0, (name, u)      # scikit-image's winding: normals point inwards
            chi[name, u] = M.euler_characteristic(v, f)
    assert chi["ball", 2] == 2 and chi["hollow_ball", 2] == 4 and chi["torus", 2] == 0
    assert chi["instance_stats", 1000] == 2
    one = np.zeros((3, 3, 3), np.int32)
    one[1, 1, 1] = 5
    v, f = M.mesh_oracle(one, 5, False)
    assert len(v) == 6 and len(f) == 8 and M.signed_volume6(v, f) == -8        # a volume of -1 / 6
    assert M.signed_volume6(*M.mesh_oracle(g["ball_mask"], 2, True)) == -8168
    edge = np.zeros((4, 4, 3), np.int32)                      # two cubes that share an edge; a corner
    edge[1, 1, 1] = edge[2, 2, 1] = 1
    corner = np.zeros((4, 4, 4), np.int32)
    corner[1, 1, 1] = corner[2, 2, 2] = 1
    assert M.euler_characteristic(*M.mesh_oracle(edge, 1, True)) == 2
    assert M.euler_characteristic(*M.mesh_oracle(corner, 1, True)) == 4


def test_record_oracle_agrees_with_the_mesh_oracle():
    """the vertex records come from the crossing edges, the meshes from the table: V is the same, key by key"""
    lab = M.cases()["all configurations (12, 24, 24)"]
    for closed in (False, True):
        ids, counts, vrec, trec = M.record_oracle(lab, closed)
        _, v, f, vo, fo = M.oracle_all(lab, closed)
        assert np.array_equal(counts[:, 0], np.diff(vo)) and np.array_equal(counts[:, 1], np.diff(fo))
        assert np.array_equal(vrec[:, 1], M.edge_keys(v, lab.shape))
        assert np.array_equal(vrec[:, 0], np.repeat(np.arange(1, len(ids) + 1), np.diff(vo)))
        assert len(trec) == len(f) and np.all(np.diff(trec[:, 0] * 2 ** 40 + trec[:, 4]) > 0)


def test_write_ply_round_trip(tmp_path, golden):
    from skoots_amd.lib.ply import write_ply
    g = golden("mesh.npz")
    inst = np.load(os.path.join(M.GOLDEN, "instance_stats.npz"))["mask"][0]
    ids, v, f, vo, fo = M.oracle_all(inst, True)
    spacing = (0.5, 0.25, 3.0)
    path = os.path.join(tmp_path, "m.ply")
    for flip in (True, False):
        assert write_ply(path, torch.from_numpy(ids), torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(vo),
                         torch.from_numpy(fo), spacing, flip=flip, comment="four instances") == path
        header, xyz, vid, faces, fid = read_ply(path)
        assert header[2] == "comment four instances"
        assert len(xyz) == len(v) and len(faces) == len(f)
        want = (v.astype(np.float64) * np.array(spacing) / 2.0).astype(np.float32)
        assert xyz.dtype == np.float32 and np.array_equal(xyz, want)
        assert np.array_equal(vid, np.repeat(ids, np.diff(vo))) and np.array_equal(fid, np.repeat(ids, np.diff(fo)))
        glob = f.astype(np.int64) + np.repeat(vo[:-1], np.diff(fo))[:, None]
        assert np.array_equal(faces, glob[:, ::-1] if flip else glob)
        assert np.array_equal(vid[faces], np.repeat(fid[:, None], 3, 1))       # a face stays inside its instance
        tri = xyz.astype(np.float64)[faces]
        volume = np.linalg.det(tri).sum() / 6.0
        assert (volume > 0) == flip
    assert ids.tolist() == [3, 7, 300, 1000] and g["instance_stats_ids"].tolist() == ids.tolist()
    # numpy arrays and an empty set of meshes go through as well
    write_ply(path, np.zeros(0, np.int64), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), [0], [0])
    header, xyz, _, faces, _ = read_ply(path)
    assert len(xyz) == 0 and len(faces) == 0 and not any(ln.startswith("comment") for ln in header)


def test_write_ply_refuses(tmp_path):
    from skoots_amd.lib.ply import write_ply
    path = os.path.join(tmp_path, "m.ply")
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.int32)
    f = np.array([[0, 1, 2]], np.int32)
    write_ply(path, [2 ** 31 - 1], v, f, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="int32"):
        write_ply(path, [2 ** 31], v, f, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="outside its instance"):
        write_ply(path, [1], v, f + 1, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="offsets"):
        write_ply(path, [1, 2], v, f, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="spacing"):
        write_ply(path, [1], v, f, [0, 3], [0, 1], spacing=(1, 0, 1))
    with pytest.raises(ValueError, match="comment"):
        write_ply(path, [1], v, f, [0, 3], [0, 1], comment="two\nlines")

    # 2^31 vertices without the memory: every row is the same 24 bytes
    big = np.lib.stride_tricks.as_strided(np.zeros(3, np.int64), shape=(2 ** 31, 3), strides=(0, 8))
    with pytest.raises(ValueError, match="vertices do not fit"):
        write_ply(path, [1], big, f, [0, 2 ** 31], [0, 1])


def test_csv_without_the_new_arguments_is_unchanged():
    from skoots_amd.validate import compare as CMP
    sums = torch.tensor([[8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 8, 8, 8]], dtype=torch.int64)
    boxes = torch.tensor([[0, 0, 0, 1, 1, 1]], dtype=torch.int32)
    text = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0))
    lines = text.splitlines()
    assert lines[2] == ("id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,"
                        "axis_minor")
    assert len(lines) == 4 and lines[3].split(",")[:14] == "4,8,16.0,0,0,0,1,1,1,1,0.5,0.5,1.0,40.0".split(",")
    counts = torch.tensor([[24, 44]], dtype=torch.int64)
    closed = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0), mesh_counts=counts,
                            mesh_closed=True).splitlines()
    assert closed[:2] == lines[:2] and closed[2] == lines[2] + ",mesh_vertices,mesh_triangles,euler_characteristic"
    assert closed[3] == lines[3] + ",24,44,2"
    opened = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0), mesh_counts=counts).splitlines()
    assert opened[2] == lines[2] + ",mesh_vertices,mesh_triangles" and opened[3] == lines[3] + ",24,44"
    # behind every other optional column
    full = CMP.format_csv("m.tif", [4], sums, boxes, (5, 5, 5), (1.0, 1.0, 2.0), max_dist2=torch.tensor([4.0]),
                          mesh_counts=counts, mesh_closed=True).splitlines()
    assert full[2] == lines[2] + ",inscribed_radius,mesh_vertices,mesh_triangles,euler_characteristic"
    assert full[3] == lines[3] + ",2.0,24,44,2"
    with pytest.raises(RuntimeError, match="odd"):
        CMP.mesh_columns(torch.tensor([[3, 1]]), True)
    assert set(CMP.mesh_columns(torch.tensor([[3, 1]]), False)) == {"mesh_vertices", "mesh_triangles"}


def test_arguments_are_checked():
    from skoots_amd.validate import compare as CMP
    a = CMP.parse_args(["m.tif"])
    assert a.mesh is None and a.save_meshes is False and a.mesh_ids is None
    assert CMP.parse_args(["m.tif", "--mesh", "open"]).mesh == "open"
    assert CMP.parse_args(["m.tif", "--save-meshes"]).mesh == "closed"
    assert CMP.parse_args(["m.tif", "--save-meshes", "--mesh", "open"]).mesh == "open"
    assert CMP.parse_args(["m.tif", "--save-meshes", "--mesh-ids", "3", "7"]).mesh_ids == [3, 7]
    for bad in (["--mesh", "both"], ["--mesh-ids", "3"]):
        with pytest.raises(SystemExit):
            CMP.parse_args(["m.tif"] + bad)
    with pytest.raises(ValueError, match="mesh"):
        CMP.stats_per_instance(torch.zeros((2, 2, 2), dtype=torch.int32), mesh="both")
    from skoots_amd.validate.lib import instance_meshes
    from skoots_amd.validate.stats import get_mesh
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_meshes(torch.zeros((2, 2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        get_mesh(torch.zeros((2, 2, 2), dtype=torch.int32), [1, 1, 1])


def test_table_tool_check_mode():
    pytest.importorskip("skimage")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_mc_triangles.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "up to date" in r.stdout
