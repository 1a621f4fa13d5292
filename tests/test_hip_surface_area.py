"""``sk_instance_mesh_cells`` (skoots_amd/csrc/instance_mesh.hip) and everything on top of it --
``instance_mesh_cells``, ``get_surface_area``, ``stats_per_instance(surface=...)`` and ``python -m skoots_amd.validate.compare --surface-area``
-- against the numpy oracle of tests/test_surface_area_cpu.py.  Every output of the kernel is an integer, so every
comparison of it is exact equality; areas are compared with the reference's (tests/golden/surface_area.npz) at the
tolerance measured there.

The kernel works on tiles of 4 x 16 x 64 cells (z along the 64 lanes of a wave; in closed mode the tile grid starts at
cell -1) and keeps 32 rows per tile in LDS; the shapes below are no multiples of any of these, exceed the table, and
degenerate in every axis."""
import os

import numpy as np
import pytest
import torch

from tests.test_surface_area_cpu import N_CLASSES, fixture_cases, mesh_cells_oracle, rtol_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = (False, True)


def blobs(shape, n, seed, id_max=100000, rmax=6.0):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32)
    g = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1)
    for i in rng.choice(np.arange(1, id_max), n, replace=False):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        rad = rng.uniform(1.5, rmax, 3)
        lab[(((g - c) / rad) ** 2).sum(-1) <= 1] = i
    return lab


def all_configurations():
    """(12, 24, 24): configuration c = 1..254 as a 2 x 2 x 2 block of label c, one background voxel between blocks"""
    lab = np.zeros((12, 24, 24), np.int32)
    for c in range(1, 255):
        i = c - 1
        x0, y0, z0 = 3 * (i // 64), 3 * (i // 8 % 8), 3 * (i % 8)
        for b in range(8):
            if (c >> b) & 1:
                lab[x0 + (b & 1), y0 + ((b >> 1) & 1), z0 + ((b >> 2) & 1)] = c
    return lab


def cases():
    """name -> (X, Y, Z) int32 array: the shapes the kernel is checked on, on the device and by
    tools/instance_mesh_host_check.py on the CPU"""
    out = {}
    lab = blobs((9, 35, 70), 40, seed=21)                 # two tiles in x, three in y, the 64-lane row in z
    lab[2:7, 14:16, 60:68] = 41000                        # two boxes sharing the y = 15 | 16 face, across the tile
    lab[2:7, 16:19, 60:68] = 41001                        # seams in y and z
    lab[0, 0, 0], lab[8, 34, 69] = 90001, 90002           # single voxels in two opposite corners
    out["blobs (9, 35, 70)"] = lab
    rng = np.random.default_rng(5)
    out["own label per voxel (6, 18, 66)"] = (rng.permutation(6 * 18 * 66) + 1).astype(np.int32).reshape(6, 18, 66)
    out["checkerboard (5, 17, 65)"] = (np.indices((5, 17, 65)).sum(0) % 2 + 1).astype(np.int32)
    out["all configurations (12, 24, 24)"] = all_configurations()
    for shape in ((1, 1, 1), (5, 1, 1), (1, 1, 70), (3, 70, 1)):
        lab = np.random.default_rng(sum(shape)).integers(0, 4, shape).astype(np.int32) * 7
        lab.flat[0] = 7
        out[f"random {shape}"] = lab
        out[f"one label {shape}"] = np.full(shape, 3, np.int32)
    out["one label (8, 9, 10)"] = np.full((8, 9, 10), 12, np.int32)
    return out


@pytest.fixture(scope="module")
def volumes():
    return cases()


@pytest.fixture(scope="module")
def want():
    """the oracle's (ids, cells) per (case name, closed), computed once"""
    cache = {}

    def get(name, lab, closed):
        if (name, closed) not in cache:
            cache[name, closed] = mesh_cells_oracle(lab, closed)
        return cache[name, closed]

    return get


def check(name, lab, want, dtype=torch.int32, x=None):
    from skoots_amd.validate.lib import instance_mesh_cells
    x = torch.from_numpy(np.asarray(lab)).to(dtype).to(DEV) if x is None else x
    out = {}
    for closed in MODES:
        ids, cells = want(name, lab, closed)
        got_ids, got = instance_mesh_cells(x, closed=closed)
        assert got_ids.dtype == torch.int64 and got.dtype == torch.int64 and got.is_cuda
        assert tuple(got.shape) == (len(ids), N_CLASSES)
        assert np.array_equal(got_ids.cpu().numpy(), ids)
        g = got.cpu().numpy()
        bad = np.argwhere(g != cells)
        assert bad.size == 0, f"{name}, closed={closed}: {len(bad)} counts differ, first (row, class) {bad[0]}: " \
                              f"{g[tuple(bad[0])]} != {cells[tuple(bad[0])]}"
        out[closed] = got
    return out


def test_blobs_sparse_ids(volumes, want):
    name = "blobs (9, 35, 70)"
    got = check(name, volumes[name], want)
    ids = want(name, volumes[name], False)[0].tolist()
    assert {41000, 41001, 90001, 90002} <= set(ids) and len(ids) > 30
    # one voxel in a corner of the volume: one single-corner cell when open, eight when closed
    assert got[False][ids.index(90002)].sum().item() == 1 and got[True][ids.index(90002)].sum().item() == 8
    assert not torch.equal(got[False], got[True])


def test_every_voxel_its_own_label(volumes, want):
    """7 128 rows in at most four tiles, eight rows per cell: far more than the LDS table holds, so the
    direct-to-global path carries the result."""
    name = "own label per voxel (6, 18, 66)"
    got = check(name, volumes[name], want)
    assert bool((got[True].sum(1) == 8).all())                       # every voxel is a corner of eight cells


def test_checkerboard(volumes, want):
    """every cell is the ambiguous configuration 0x69 or 0x96 for both labels"""
    name = "checkerboard (5, 17, 65)"
    got = check(name, volumes[name], want)
    assert got[False].sum().item() == 2 * 4 * 16 * 64


def test_all_configurations(volumes, want):
    name = "all configurations (12, 24, 24)"
    got = check(name, volumes[name], want)
    assert bool((got[False].sum(0) > 0).all())                       # every class occurs


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 1, 1), (1, 1, 70), (3, 70, 1)])
def test_degenerate_extents(shape, volumes, want):
    for kind in ("random", "one label"):
        name = f"{kind} {shape}"
        got = check(name, volumes[name], want)
        assert got[False].sum().item() == 0 and got[True].sum().item() > 0


def test_all_background_and_one_label(volumes, want):
    from skoots_amd.validate.compare import mesh_area
    from skoots_amd.validate.lib import instance_mesh_cells
    for closed in MODES:
        ids, cells = instance_mesh_cells(torch.zeros((8, 9, 10), dtype=torch.int32, device=DEV), closed=closed)
        assert tuple(ids.shape) == (0,) and tuple(cells.shape) == (0, N_CLASSES) and cells.dtype == torch.int64
        assert instance_mesh_cells(torch.full((3, 3, 3), -5, dtype=torch.int32, device=DEV), closed)[0].numel() == 0
        assert instance_mesh_cells(torch.zeros((0, 4, 4), dtype=torch.int32, device=DEV), closed)[0].numel() == 0
    name = "one label (8, 9, 10)"
    got = check(name, volumes[name], want)
    assert got[False].sum().item() == 0
    area = mesh_area(got[True], (1, 1, 1))[0].item()
    assert area == mesh_area(torch.from_numpy(want(name, volumes[name], True)[1]), (1, 1, 1))[0].item()
    assert area == pytest.approx(2 * (7 * 8 + 7 * 9 + 8 * 9) + 4 * (7 + 8 + 9) * 2 ** 0.5 / 2 + 3 ** 0.5, rel=1e-14)


def test_huge_ids_take_the_relabel_route(monkeypatch, want):
    from skoots_amd.validate import lib as VL
    lab = np.zeros((4, 4, 4), np.int32)
    lab[0, 0, :3] = 2 ** 31 - 1
    lab[1:3, 1:3, 1:3] = 2 ** 30
    lab[3, 3, 3] = 5
    lab[3, 0, 0] = -9
    monkeypatch.setattr(VL, "_lut", lambda m: pytest.fail("the max id + 1 table was built for a 2^31 - 1 id"))
    check("huge int32", lab, want)
    big = lab.astype(np.int64)
    big[0, 0, :3] = 2 ** 40                           # beyond int32 altogether
    check("huge int64", big, want, dtype=torch.int64)
    assert want("huge int64", big, False)[0].tolist() == [5, 2 ** 30, 2 ** 40]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int64])
def test_integer_dtypes_and_4d(dtype, volumes, want):
    from skoots_amd.validate.lib import instance_mesh_cells
    lab = (volumes["blobs (9, 35, 70)"][:7, :20, :66] % 120).astype(np.int32)
    x = torch.from_numpy(lab).to(dtype).to(DEV)
    check("blobs mod 120", lab, want, x=x[None])
    with pytest.raises(TypeError):
        instance_mesh_cells(x.float())


def test_two_runs_are_bit_identical_and_non_default_stream(volumes, want):
    from skoots_amd.validate.lib import instance_mesh_cells
    name = "blobs (9, 35, 70)"
    x = torch.from_numpy(volumes[name]).to(DEV)
    for closed in MODES:
        a, b = instance_mesh_cells(x, closed), instance_mesh_cells(x, closed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        check(name, volumes[name], want, x=x)
    s.synchronize()


def test_guards_launch_nothing():
    from skoots_amd import _ffi
    from skoots_amd.validate.mc_table import CLASS_OF
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    lut = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    class_of = torch.tensor(CLASS_OF, dtype=torch.uint8, device=DEV)
    cells = torch.full((1, 32), -7, dtype=torch.int64, device=DEV)
    odd = torch.zeros(80, dtype=torch.uint8, device=DEV)

    def call(X, Y, Z, N=1, max_id=1, n_classes=N_CLASSES, closed=0, lab_p=_ffi.ptr(lab), lut_p=_ffi.ptr(lut),
             class_p=_ffi.ptr(class_of), cells_p=_ffi.ptr(cells)):
        rc = _ffi.lib.sk_instance_mesh_cells(lab_p, X, Y, Z, lut_p, max_id, N, class_p, n_classes, closed, cells_p,
                                             _ffi.stream_ptr(lab.device))
        torch.cuda.synchronize()
        return rc

    for shape in [(3000000, 3000000, 3000000), (2 ** 31 - 1, 2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert call(*shape) == -1 and "2^62" in _ffi.last_error()
    assert call(4, 4, 4, N=-1) == -1 and call(4, 4, 4, max_id=-1) == -1
    assert call(-1, 4, 4) == -1 and call(4, -1, 4) == -1 and call(4, 4, -1) == -1
    for n in (0, -1, 33):
        assert call(4, 4, 4, n_classes=n) == -1 and "n_classes" in _ffi.last_error()
    assert call(4, 4, 4, closed=2) == -1 and call(4, 4, 4, closed=-1) == -1
    for null in ("lab_p", "lut_p", "class_p", "cells_p"):
        assert call(4, 4, 4, **{null: None}) == -1 and "NULL" in _ffi.last_error()
    assert call(4, 4, 4, lab_p=odd.data_ptr() + 1) == -1 and "aligned" in _ffi.last_error()
    assert call(4, 4, 4, lut_p=odd.data_ptr() + 2) == -1 and "aligned" in _ffi.last_error()
    assert call(4, 4, 4, cells_p=odd.data_ptr() + 4) == -1 and "aligned" in _ffi.last_error()
    assert call(0, 4, 4) == 0 and call(4, 4, 4, N=0) == 0           # nothing to do: success, nothing written
    assert bool((cells == -7).all())
    assert call(4, 4, 1) == 0                                       # open, an extent of 1: no cell, zeros
    assert bool((cells[0, :N_CLASSES] == 0).all()) and bool((cells[0, N_CLASSES:] == -7).all())
    assert call(4, 4, 4, closed=1) == 0                             # the same buffers, now measured: a 4^3 box
    assert cells[0, :N_CLASSES].sum().item() == 5 ** 3 - 3 ** 3 and bool((cells[0, N_CLASSES:] == -7).all())
    # a table that names classes the row does not have: those cells are skipped, nothing leaves the row
    want = cells[0, :7].clone()
    cells.fill_(-7)
    assert call(4, 4, 4, n_classes=7, closed=1) == 0
    assert torch.equal(cells[0, :7], want) and bool((cells[0, 7:] == -7).all())
    assert _ffi.lib.sk_abi_version() >= 15


def test_areas_against_the_reference(golden):
    from skoots_amd.validate.compare import stats_per_instance
    from skoots_amd.validate.stats import get_surface_area
    g = golden("surface_area.npz")
    spacings = g["spacings"].tolist()
    for name, mask, ids, area in fixture_cases(g):
        x = torch.from_numpy(mask).to(DEV)
        for m, mode in enumerate(("open", "closed")):
            for s, spacing in enumerate(spacings):
                st = stats_per_instance(x, spacing, surface=mode)
                assert st["id"].tolist() == ids.tolist()
                assert st["surface_area"].dtype == torch.float64 and st["surface_area"].is_cuda
                assert st["mesh_cells"].dtype == torch.int64 and tuple(st["mesh_cells"].shape) == (len(ids), 30)
                got = st["surface_area"].cpu().numpy()
                rel = np.abs(got - area[:, s, m]) / area[:, s, m]
                print(f"{name} {mode} {spacing}: largest relative deviation {rel.max():.3e}")
                assert rel.max() <= rtol_for(spacing), (name, mode, spacing, rel)
                assert torch.equal(st["surface_to_volume"], st["surface_area"] / st["volume"])
                one = get_surface_area(x == int(ids[-1]), spacing, closed=mode == "closed")
                assert one.dtype == torch.float64 and one.is_cuda and one.item() == got[-1]
    # the reference's meaning of the mask is x > 0: every instance of the noise volume together
    x = torch.from_numpy(g["noise_mask"]).to(DEV)
    assert get_surface_area(x.float(), [1.0, 1.0, 3.0]).item() == get_surface_area(x, [1.0, 1.0, 3.0]).item()
    assert abs(get_surface_area(x, [1.0, 1.0, 3.0]).item() / g["noise_area"][0, 1, 0] - 1) <= rtol_for((1, 1, 3))
    # stated difference: no surface inside the volume gives 0 where scikit-image raises
    assert get_surface_area(torch.ones((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1]).item() == 0.0
    assert get_surface_area(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV), [1, 1, 1], closed=True).item() == 0.0
    # without the switch the dict is what it was
    assert set(stats_per_instance(x)) == {"id", "voxels", "volume", "bbox", "touches_border", "centroid", "face_area",
                                          "faces", "axis_lengths", "sums"}


def test_command_end_to_end(tmp_path, volumes):
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import format_csv, main, stats_per_instance
    from skoots_amd.validate.lib import instance_sums
    lab = volumes["blobs (9, 35, 70)"][:, :, :40].copy()
    x = torch.from_numpy(lab).to(DEV)
    path = os.path.join(tmp_path, "mito.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    spacing = (0.5, 0.25, 3.0)
    args = [path, "--spacing", *(str(v) for v in spacing), "--min-voxels", "2"]
    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read()
    # the text of the code path as it was before the switch existed
    assert plain == format_csv(path, *instance_sums(x), lab.shape, spacing, 2)
    assert plain.splitlines()[2] == ("id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,"
                                     "axis_mid,axis_minor")
    out = main(args + ["--surface-area", "closed"])
    assert out == os.path.join(tmp_path, "mito_instance_stats.csv")
    lines, old = open(out).read().splitlines(), plain.splitlines()
    assert lines[:2] == old[:2] and lines[2] == old[2] + ",surface_area,surface_to_volume"
    assert [ln.split(",")[:17] for ln in lines[3:]] == [ln.split(",") for ln in old[3:]]
    st = stats_per_instance(x, spacing, surface="closed")
    keep = (st["voxels"] >= 2).cpu().numpy()
    assert not keep.all() and keep.any()
    rows = [ln.split(",") for ln in lines[3:]]
    assert [float(r[17]) for r in rows] == st["surface_area"].cpu().numpy()[keep].tolist()
    assert [float(r[18]) for r in rows] == st["surface_to_volume"].cpu().numpy()[keep].tolist()
    open_rows = open(main(args + ["--surface-area", "open", "--out", os.path.join(tmp_path, "open.csv")])).read()
    st = stats_per_instance(x, spacing, surface="open")
    assert [float(ln.split(",")[17]) for ln in open_rows.splitlines()[3:]] == \
        st["surface_area"].cpu().numpy()[keep].tolist()


def test_command_rows_are_pinned(tmp_path):
    """The file the command writes for a small mask, as literals taken from the code before the switch existed (the
    17 columns) and from the numpy oracle (the two new ones): a change of the row text cannot pass unnoticed.  The
    axes of the two boxes come out of LAPACK and are compared as numbers; every other field is compared as text."""
    from skoots_amd.lib import tiff
    from skoots_amd.validate.compare import main
    lab = np.zeros((6, 7, 8), np.int32)
    lab[1:4, 2:6, 1:7] = 2
    lab[4:6, 2:6, 1:7] = 9                                            # shares the x = 3 | 4 face with 2
    lab[0, 0, 0] = 40
    path = os.path.join(tmp_path, "m.tif")
    tiff.write_label_stack(path, torch.from_numpy(lab).to(DEV).permute(2, 0, 1).contiguous())
    args = [path, "--spacing", "0.5", "0.25", "3.0"]
    header = "id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,axis_minor"
    rows = ["2,72,27.0,1,2,1,3,5,6,0,1.0,0.875,10.5,93.0,22.9128784747792,1.825741858350554,1.25",
            "9,48,18.0,4,2,1,5,5,6,1,2.25,0.875,10.5,74.0,22.9128784747792,1.25,1.118033988749895",
            "40,1,0.375,0,0,0,0,0,0,1,0.0,0.0,0.0,4.75,0.0,0.0,0.0"]
    surface = {"open": [["83.03508202425246", "3.0753734083056465"], ["41.51754101212623", "2.306530056229235"],
                        ["0.21021287573552672", "0.5605676686280713"]],
               "closed": [["83.03508202425246", "3.0753734083056465"], ["64.27468337955438", "3.5708157433085765"],
                          ["1.6817030058842137", "4.48454134902457"]]}

    def same(got, want_row):
        g, w = got.split(","), want_row.split(",")
        assert g[:14] == w[:14], (got, want_row)
        assert [float(v) for v in g[14:17]] == pytest.approx([float(v) for v in w[14:17]], rel=1e-13, abs=0)

    plain = open(main(args + ["--out", os.path.join(tmp_path, "plain.csv")])).read().splitlines()
    assert plain[:3] == [f"Mask File: {path}", "Spacing: 0.5 0.25 3.0", header] and len(plain) == 6
    for got, want_row in zip(plain[3:], rows):
        same(got, want_row)
    assert plain[5] == rows[2]                                        # one voxel: no field comes out of LAPACK
    for mode, cols in surface.items():
        lines = open(main(args + ["--surface-area", mode])).read().splitlines()
        assert lines[:2] == plain[:2] and lines[2] == header + ",surface_area,surface_to_volume"
        assert [ln.split(",")[:17] for ln in lines[3:]] == [ln.split(",") for ln in plain[3:]]
        assert [ln.split(",")[17:] for ln in lines[3:]] == cols


def test_both_kernels_share_one_prologue(monkeypatch, volumes):
    from skoots_amd.validate import lib as VL
    from skoots_amd.validate.compare import stats_per_instance
    calls = []
    real = VL._id_rows
    monkeypatch.setattr(VL, "_id_rows", lambda x: calls.append(1) or real(x))
    st = stats_per_instance(torch.from_numpy(volumes["blobs (9, 35, 70)"]).to(DEV), surface="open")
    assert len(calls) == 1 and st["mesh_cells"].shape[0] == st["id"].numel()

