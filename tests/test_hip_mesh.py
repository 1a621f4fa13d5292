"""``sk_instance_mesh_count`` / ``sk_instance_mesh_emit`` (skoots_amd/csrc/instance_mesh_emit.hip) and everything on top
of them -- ``instance_meshes``, ``stats_per_instance(mesh=...)``, ``get_mesh``, ``--mesh`` / ``--save-meshes`` -- against
scikit-image's own meshes (tests/golden/mesh.npz) and the numpy oracle of tests/mesh_cases.py.  Every output is an
integer, so every comparison is exact equality.

The kernels work on tiles of 4 x 16 x 64 positions (z along the 64 lanes of a wave; in closed mode the grid starts at
-1; a position is a cell or, on the high faces, only the start of edges); the shapes are no multiples of these, end
exactly on them, exceed the LDS table of the count pass, and degenerate in every axis."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import mesh_cases as M
from tests.test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = (("open", False), ("closed", True))
KEYS = ("ids", "vertices", "faces", "vertex_offsets", "face_offsets")


@pytest.fixture(scope="module")
def volumes():
    return M.cases()


@pytest.fixture(scope="module")
def want():
    """the oracle's (ids, vertices, faces, vertex_offsets, face_offsets) per (case name, closed), computed once"""
    cache = {}

    def get(name, lab, closed):
        if (name, closed) not in cache:
            cache[name, closed] = M.oracle_all(lab, closed)
        return cache[name, closed]

    return get


def meshes(lab, closed, **kw):
    from skoots_amd.validate.lib import instance_meshes
    x = lab if isinstance(lab, torch.Tensor) else torch.from_numpy(np.asarray(lab)).to(DEV)
    m = instance_meshes(x, closed=closed, **kw)
    assert set(m) == set(KEYS) and all(m[k].is_cuda for k in KEYS)
    assert m["vertices"].dtype == torch.int32 and m["faces"].dtype == torch.int32
    assert all(m[k].dtype == torch.int64 for k in ("ids", "vertex_offsets", "face_offsets"))
    return {k: v.cpu().numpy() for k, v in m.items()}


def check_structure(m, closed):
    """indices lie in [0, V_a), every vertex is referenced, and closed meshes are edge-manifold"""
    vo, fo, f = m["vertex_offsets"], m["face_offsets"], m["faces"].astype(np.int64)
    N = len(m["ids"])
    assert vo.shape == (N + 1,) and fo.shape == (N + 1,) and vo[0] == 0 and fo[0] == 0
    assert vo[-1] == len(m["vertices"]) and fo[-1] == len(f)
    assert np.all(np.diff(vo) >= 0) and np.all(np.diff(fo) >= 0)
    nv = np.repeat(np.diff(vo), np.diff(fo))
    assert len(f) == 0 or (f.min() >= 0 and np.all(f < nv[:, None]))
    glob = f + np.repeat(vo[:-1], np.diff(fo))[:, None]       # the instances' index ranges are disjoint
    assert np.array_equal(np.unique(glob), np.arange(len(m["vertices"])))
    if closed:
        assert M.directed_edges_pair_up(glob)
        assert np.all(np.diff(fo) % 2 == 0)


def check_case(name, lab, want, closed):
    ids, v, f, vo, fo = want(name, lab, closed)
    m = meshes(lab, closed)
    assert np.array_equal(m["ids"], ids)
    assert np.array_equal(m["vertex_offsets"], vo) and np.array_equal(m["face_offsets"], fo)
    bad = np.argwhere(m["vertices"] != v)
    assert bad.size == 0, f"{name}, closed={closed}: {len(bad)} coordinates differ, first {bad[0]}"
    bad = np.argwhere(m["faces"] != f)
    assert bad.size == 0, f"{name}, closed={closed}: {len(bad)} indices differ, first {bad[0]}"
    check_structure(m, closed)
    return m


def test_fixture_meshes_equal_scikit_image(golden):
    g = golden("mesh.npz")
    for name, mask, ids in M.fixture_cases(g):
        for mode, closed in MODES:
            m = meshes(mask, closed)
            assert m["ids"].tolist() == ids
            check_structure(m, closed)
            for k, u in enumerate(ids):
                v = m["vertices"][m["vertex_offsets"][k]:m["vertex_offsets"][k + 1]]
                f = m["faces"][m["face_offsets"][k]:m["face_offsets"][k + 1]]
                got, fixture = M.canonical_triangles(v, f), g[f"{name}_{u}_{mode}_tri"]
                assert got.shape == fixture.shape and np.array_equal(got, fixture), (name, u, mode)
                assert len(v) == int(g[f"{name}_{u}_{mode}_v"]), (name, u, mode)
                if closed:
                    assert M.signed_volume6(v, f) < 0, (name, u)
            if closed and name in ("ball", "hollow_ball", "torus"):
                chi = {"ball": 2, "hollow_ball": 4, "torus": 0}[name]
                assert len(m["vertices"]) - len(m["faces"]) // 2 == chi


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", ["blobs (9, 35, 70)", "own label per voxel (6, 18, 66)", "checkerboard (5, 17, 65)",
                                  "all configurations (12, 24, 24)", "checkerboard (3, 15, 63)",
                                  "one label (8, 9, 10)"])
def test_shapes_equal_the_oracle(name, closed, volumes, want):
    m = check_case(name, volumes[name], want, closed)
    if name.startswith("own label") and closed:               # a voxel alone: 6 vertices, 8 triangles
        assert np.all(np.diff(m["vertex_offsets"]) == 6) and np.all(np.diff(m["face_offsets"]) == 8)
    if name.startswith("one label") and not closed:
        assert len(m["vertices"]) == 0 and len(m["faces"]) == 0 and m["ids"].tolist() == [12]


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 1, 1), (1, 1, 70), (3, 70, 1)])
def test_degenerate_extents(shape, volumes, want):
    for kind in ("random", "one label"):
        name = f"{kind} {shape}"
        assert len(check_case(name, volumes[name], want, False)["vertices"]) == 0
        assert len(check_case(name, volumes[name], want, True)["vertices"]) > 0


def test_nothing_to_mesh():
    for closed in (False, True):
        for x in (torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV),
                  torch.full((3, 3, 3), -5, dtype=torch.int32, device=DEV),
                  torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV)):
            m = meshes(x, closed)
            assert m["ids"].shape == (0,) and m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3)
            assert m["vertex_offsets"].tolist() == [0] and m["face_offsets"].tolist() == [0]


def _tri_terms(v, f, spacing):
    """the area of every triangle, from its exact integer cross product, as compare.class_areas computes a type's"""
    sx, sy, sz = spacing
    t = v.astype(np.int64)[f.astype(np.int64)]
    a, b, c = np.abs(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])).T          # 4 x the unit cross product, exact
    return [math.sqrt((int(p) * sy * sz) ** 2 + (int(q) * sx * sz) ** 2 + (int(r) * sx * sy) ** 2) / 8.0
            for p, q, r in zip(a, b, c)]


def test_cross_checks_against_the_other_kernels(volumes):
    from skoots_amd.validate.compare import stats_per_instance
    from skoots_amd.validate.mc_table import CLASS_TRIANGLES
    per_class = torch.tensor([sum(row) for row in CLASS_TRIANGLES], dtype=torch.int64, device=DEV)
    lab = volumes["blobs (9, 35, 70)"]
    x = torch.from_numpy(lab).to(DEV)
    spacing = (0.5, 0.25, 3.0)
    for mode, closed in MODES:
        st = stats_per_instance(x, spacing, surface=mode, mesh=mode)
        assert st["mesh_vertices"].dtype == torch.int64 and st["mesh_vertices"].is_cuda
        assert torch.equal(st["mesh_triangles"], (st["mesh_cells"] * per_class).sum(1))
        m = meshes(x, closed)
        assert np.array_equal(st["mesh_vertices"].cpu().numpy(), np.diff(m["vertex_offsets"]))
        assert np.array_equal(st["mesh_triangles"].cpu().numpy(), np.diff(m["face_offsets"]))
        if closed:
            assert torch.equal(st["mesh_vertices"], st["faces"].sum(1))          # V = the exposed voxel faces
            assert torch.equal(st["euler_characteristic"], st["mesh_vertices"] - st["mesh_triangles"] // 2)
            assert st["euler_characteristic"].dtype == torch.int64
        else:
            assert "euler_characteristic" not in st
        # both are sums of the same F positive terms, in different orders: within F 2^-52, relatively
        area = st["surface_area"].cpu().numpy()
        worst = 0.0
        for k in range(len(m["ids"])):
            v = m["vertices"][m["vertex_offsets"][k]:m["vertex_offsets"][k + 1]]
            f = m["faces"][m["face_offsets"][k]:m["face_offsets"][k + 1]]
            if len(f) == 0:
                assert area[k] == 0.0
                continue
            mine = math.fsum(_tri_terms(v, f, spacing))
            rel = abs(mine - area[k]) / area[k]
            worst = max(worst, rel / (len(f) * 2.0 ** -52))
            assert rel <= len(f) * 2.0 ** -52, (mode, int(m["ids"][k]), mine, area[k], len(f))
        print(f"{mode}: largest deviation of the areas, in units of F 2^-52: {worst:.3f}")
    assert "mesh_vertices" not in stats_per_instance(x, spacing)


def test_closed_instances_have_negative_signed_volume(volumes):
    for name in ("blobs (9, 35, 70)", "all configurations (12, 24, 24)"):
        m = meshes(volumes[name], True)
        t = m["vertices"].astype(np.int64)[m["faces"].astype(np.int64) +
                                           np.repeat(m["vertex_offsets"][:-1], np.diff(m["face_offsets"]))[:, None]]
        det = np.einsum("ni,ni->n", t[:, 0], np.cross(t[:, 1], t[:, 2]))          # exact in int64
        per = np.add.reduceat(det, m["face_offsets"][:-1])
        assert np.all(np.diff(m["face_offsets"]) > 0) and np.all(per < 0), name


def test_two_runs_are_byte_identical_and_non_default_stream(volumes):
    from skoots_amd.validate.lib import instance_meshes
    x = torch.from_numpy(volumes["blobs (9, 35, 70)"]).to(DEV)
    for closed in (False, True):
        a, b = instance_meshes(x, closed), instance_meshes(x, closed)
        assert all(torch.equal(a[k], b[k]) for k in KEYS)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            c = instance_meshes(x, closed)
        s.synchronize()
        assert all(torch.equal(a[k], c[k]) for k in KEYS)
        d = instance_meshes(x[None].to(torch.int64), closed)                       # (1, X, Y, Z), another dtype
        assert all(torch.equal(a[k], d[k]) for k in KEYS)
    with pytest.raises(TypeError):
        instance_meshes(x.float())


def test_ids_select_slices_of_the_full_result(volumes):
    from skoots_amd.validate.lib import id_rows, instance_meshes
    lab = volumes["blobs (9, 35, 70)"]
    x = torch.from_numpy(lab).to(DEV)
    for closed in (False, True):
        full = meshes(x, closed)
        ids = full["ids"].tolist()
        pick = [ids[-1], ids[0], 41001, 41000, ids[0]]        # any order, a repeat: ascending and unique in the result
        part = meshes(x, closed, ids=pick)
        assert part["ids"].tolist() == sorted(set(pick))
        check_structure(part, closed)
        for k, u in enumerate(part["ids"].tolist()):
            j = ids.index(u)
            for key, off in (("vertices", "vertex_offsets"), ("faces", "face_offsets")):
                assert np.array_equal(part[key][part[off][k]:part[off][k + 1]], full[key][full[off][j]:full[off][j + 1]])
        one = instance_meshes(x, closed, rows=id_rows(x), ids=torch.tensor([41000]))
        assert one["ids"].tolist() == [41000] and one["vertices"].shape[0] == np.diff(full["vertex_offsets"])[ids.index(41000)]
    with pytest.raises(ValueError, match="not in the mask"):
        instance_meshes(x, ids=[ids[0], 7777777])
    assert meshes(x, True, ids=[])["ids"].shape == (0,)
    # ids far beyond the voxel count take the relabel route of the prologue
    big = np.zeros((4, 4, 4), np.int64)
    big[0, 0, :3], big[1:3, 1:3, 1:3], big[3, 3, 3] = 2 ** 40, 2 ** 30, 5
    full = meshes(torch.from_numpy(big).to(DEV), True)
    assert full["ids"].tolist() == [5, 2 ** 30, 2 ** 40]
    want_ids, v, f, vo, fo = M.oracle_all(big, True)
    assert np.array_equal(full["vertices"], v) and np.array_equal(full["faces"], f)
    part = meshes(torch.from_numpy(big).to(DEV), True, ids=[2 ** 40])
    assert np.array_equal(part["vertices"], v[vo[2]:vo[3]]) and np.array_equal(part["faces"], f[fo[2]:fo[3]])


def test_budget_refuses_before_allocation(volumes, monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.validate import lib as VL
    x = torch.from_numpy(volumes["blobs (9, 35, 70)"]).to(DEV)
    rows = VL.id_rows(x)
    counts = VL.instance_mesh_counts(x, True, rows)[1].sum(0).tolist()
    need = 16 * counts[0] + 40 * counts[1]
    assert need > 2 ** 19
    assert VL.instance_meshes(x, True, rows, budget_bytes=need)["vertices"].shape[0] == counts[0]
    real = VL._ffi.lib.sk_instance_mesh_emit
    called = []
    monkeypatch.setattr(_ffi.lib, "sk_instance_mesh_emit", lambda *a: called.append(1) or real(*a))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=rf"{need} bytes.*ids="):
        VL.instance_meshes(x, True, rows, budget_bytes=need - 1)
    assert not called
    # the count pass has its (N, 2) counts and the 2 KiB table; the records, `need` bytes, were never allocated
    assert torch.cuda.max_memory_allocated() - before < 2 ** 16 < need
    # the sort keys must fit int64: refused from the shape and the row count alone
    many = types.SimpleNamespace(numel=lambda: 2 ** 40)
    monkeypatch.setattr(VL, "_mesh_prologue", lambda x, rows, ids: (x, (None, many, None, 0), (2 ** 10,) * 3))
    with pytest.raises(ValueError, match=r"2\^63"):
        VL.instance_meshes(x, True)


def test_get_mesh(golden):
    from skoots_amd.validate.stats import get_mesh
    g = golden("mesh.npz")
    x = torch.from_numpy(g["noise_mask"]).to(DEV)
    spacing = [1.0, 0.5, 3.0]
    for mode, closed in MODES:
        verts, faces = get_mesh(x, spacing, closed=closed)
        assert verts.dtype == torch.float64 and faces.dtype == torch.int64 and verts.is_cuda and faces.is_cuda
        doubled = (verts.cpu().numpy() / np.array(spacing) * 2.0)
        assert np.array_equal(doubled, np.round(doubled))
        got = M.canonical_triangles(doubled.astype(np.int64), faces.cpu().numpy())
        assert np.array_equal(got, g[f"noise_4_{mode}_tri"])
    assert torch.equal(get_mesh(x.float(), spacing, closed=True)[0], verts)    # x > 0 is the meaning: any dtype
    v, f = get_mesh(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), spacing, closed=True)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_command_end_to_end(tmp_path, volumes):
    from skoots_amd.validate.compare import main
    lab = volumes["blobs (9, 35, 70)"][:, :, :40].copy()
    path = os.path.join(tmp_path, "mito.npy")
    np.save(path, np.ascontiguousarray(lab.transpose(2, 0, 1)))                 # stored [Z, X, Y]
    spacing = (0.5, 0.25, 3.0)
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read().splitlines()
    assert not os.path.exists(os.path.join(tmp_path, "mito_meshes.ply"))
    out = main(args + ["--mesh", "closed", "--save-meshes"])
    lines = open(out).read().splitlines()
    assert lines[:2] == plain[:2] and lines[2] == plain[2] + ",mesh_vertices,mesh_triangles,euler_characteristic"
    assert [ln.split(",")[:-3] for ln in lines[3:]] == [ln.split(",") for ln in plain[3:]]
    listed = [int(ln.split(",")[0]) for ln in lines[3:]]
    ids, v, f, vo, fo = M.oracle_all(lab, True)
    assert set(listed) < set(ids.tolist())                    # --min-voxels leaves the single voxels out
    header, xyz, vid, faces, fid = read_ply(os.path.join(tmp_path, "mito_meshes.ply"))
    assert header[2].startswith("comment skoots_amd marching-cubes meshes (closed) of mito.npy")
    assert sorted(set(fid.tolist())) == listed
    for row in lines[3:]:
        cells = row.split(",")
        u, k = int(cells[0]), ids.tolist().index(int(cells[0]))
        assert [int(c) for c in cells[-3:]] == [vo[k + 1] - vo[k], fo[k + 1] - fo[k],
                                                (vo[k + 1] - vo[k]) - (fo[k + 1] - fo[k]) // 2]
        want_xyz = (v[vo[k]:vo[k + 1]].astype(np.float64) * np.array(spacing) / 2.0).astype(np.float32)
        mine = np.flatnonzero(vid == u)
        assert np.array_equal(xyz[mine], want_xyz)
        tri = faces[fid == u] - mine[0]                       # global -> local; written reversed: normals point out
        assert np.array_equal(tri[:, ::-1], f[fo[k]:fo[k + 1]])
    assert np.linalg.det(xyz.astype(np.float64)[faces]).sum() > 0
    # --mesh-ids, open mode, and the refusals
    main(args + ["--save-meshes", "--mesh", "open", "--mesh-ids", str(listed[-1]), str(listed[0]), "--out",
                 os.path.join(tmp_path, "two.csv")])
    two = open(os.path.join(tmp_path, "two.csv")).read().splitlines()
    assert two[2] == plain[2] + ",mesh_vertices,mesh_triangles" and len(two) == len(plain)
    _, xyz, vid, faces, fid = read_ply(os.path.join(tmp_path, "mito_meshes.ply"))
    assert sorted(set(vid.tolist())) == [listed[0], listed[-1]] == sorted(set(fid.tolist()))
    with pytest.raises(ValueError, match="mesh-ids"):
        main(args + ["--save-meshes", "--mesh-ids", "90001"])                   # one voxel: below --min-voxels


def test_c_abi_guards_and_capacities():
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import packed_triangle_table
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    lut = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    table = torch.from_numpy(packed_triangle_table().view(np.int64)).to(DEV)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    vrec = torch.full((200, 2), -7, dtype=torch.int64, device=DEV)
    trec = torch.full((300, 5), -7, dtype=torch.int64, device=DEV)
    produced = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    odd = torch.zeros(80, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(lab.device)

    def count(X, Y, Z, N=1, max_id=1, closed=0, lab_p=_ffi.ptr(lab), lut_p=_ffi.ptr(lut), table_p=_ffi.ptr(table),
              counts_p=_ffi.ptr(counts)):
        rc = _ffi.lib.sk_instance_mesh_count(lab_p, X, Y, Z, lut_p, max_id, N, table_p, closed, counts_p, st)
        torch.cuda.synchronize()
        return rc

    def emit(X, Y, Z, N=1, max_id=1, closed=0, cv=200, ct=300, lab_p=_ffi.ptr(lab), lut_p=_ffi.ptr(lut),
             table_p=_ffi.ptr(table), vrec_p=_ffi.ptr(vrec), trec_p=_ffi.ptr(trec), produced_p=_ffi.ptr(produced)):
        rc = _ffi.lib.sk_instance_mesh_emit(lab_p, X, Y, Z, lut_p, max_id, N, table_p, closed, vrec_p, cv, trec_p, ct,
                                            produced_p, st)
        torch.cuda.synchronize()
        return rc

    for call in (count, emit):
        assert call(3000000, 3000000, 3000000) == -1 and "2^62" in _ffi.last_error()
        assert call(2 ** 31 - 1, 2 ** 31 - 1, 1) == -1 and "2^60" in _ffi.last_error()
        assert call(-1, 4, 4) == -1 and "negative" in _ffi.last_error()
        assert call(4, -1, 4) == -1 and call(4, 4, -1) == -1
        assert call(4, 4, 4, N=-1) == -1 and call(4, 4, 4, max_id=-1) == -1
        assert call(4, 4, 4, closed=2) == -1 and "closed" in _ffi.last_error()
        assert call(4, 4, 4, closed=-1) == -1
        for null in ("lab_p", "lut_p", "table_p"):
            assert call(4, 4, 4, **{null: None}) == -1 and "NULL" in _ffi.last_error()
        assert call(4, 4, 4, lab_p=odd.data_ptr() + 1) == -1 and "aligned" in _ffi.last_error()
        assert call(4, 4, 4, lut_p=odd.data_ptr() + 2) == -1 and "aligned" in _ffi.last_error()
        assert call(4, 4, 4, table_p=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
        assert call(0, 4, 4) == 0 and call(4, 4, 4, N=0) == 0                   # nothing to do: success, nothing written
    assert count(4, 4, 4, counts_p=None) == -1 and "NULL" in _ffi.last_error()
    assert count(4, 4, 4, counts_p=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert emit(4, 4, 4, produced_p=None) == -1 and emit(4, 4, 4, vrec_p=None) == -1 and emit(4, 4, 4, trec_p=None) == -1
    assert emit(4, 4, 4, vrec_p=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert emit(4, 4, 4, cv=-1) == -1 and emit(4, 4, 4, ct=-1) == -1 and emit(4, 4, 4, cv=2 ** 58) == -1
    for t in (counts, vrec, trec, produced):
        assert bool((t == -7).all())
    assert count(4, 4, 1) == 0 and counts.tolist() == [0, 0, -7, -7]            # open, an extent of 1: no cell, zeros
    assert emit(4, 4, 1) == 0 and produced.tolist() == [0, 0] and bool((vrec == -7).all())
    # a 4 x 4 x 4 box, closed: 6 x 16 crossing edges
    assert count(4, 4, 4, closed=1) == 0
    V, F = counts[:2].tolist()
    assert [[V, F]] == M.record_oracle(np.ones((4, 4, 4), np.int32), True)[1].tolist() and V == 96
    assert counts[2:].tolist() == [-7, -7]
    assert emit(4, 4, 4, closed=1) == 0 and produced.tolist() == [V, F]
    assert bool((vrec[:V] != -7).all()) and bool((vrec[V:] == -7).all())
    assert bool((trec[:F] != -7).all()) and bool((trec[F:] == -7).all())
    assert bool((vrec[:V, 0] == 1).all()) and vrec[:V, 1].unique().numel() == V
    full_v, full_t = vrec[:V].clone(), trec[:F].clone()
    # capacities below the need: nothing beyond them is written, the counters say what was needed, and what is
    # written is part of the full result
    vrec.fill_(-7), trec.fill_(-7)
    assert emit(4, 4, 4, closed=1, cv=40, ct=50) == 0 and produced.tolist() == [V, F]
    assert bool((vrec[40:] == -7).all()) and bool((trec[50:] == -7).all())
    assert set(vrec[:40, 1].tolist()) <= set(full_v[:, 1].tolist()) and bool((vrec[:40] != -7).all())
    assert set(trec[:50, 4].tolist()) <= set(full_t[:, 4].tolist())
    vrec.fill_(-7), trec.fill_(-7)
    assert emit(4, 4, 4, closed=1, cv=0, ct=0, vrec_p=None, trec_p=None) == 0 and produced.tolist() == [V, F]
    assert bool((vrec == -7).all()) and bool((trec == -7).all())
    # a look-up table that names rows outside 1..N: background, nothing leaves the outputs
    wild = torch.tensor([0, 9], dtype=torch.int32, device=DEV)
    counts.fill_(-7)
    assert count(4, 4, 4, closed=1, lut_p=_ffi.ptr(wild)) == 0 and counts.tolist() == [0, 0, -7, -7]
    assert _ffi.lib.sk_abi_version() >= 18
