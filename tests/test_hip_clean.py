"""``sk_label_components`` / ``sk_component_table`` / ``sk_apply_piece_lut`` (skoots_amd/csrc/components.hip) and what
stands on them -- ``lib.morphology.label_components``, ``utils.clean.clean`` and its command, the ``pieces`` columns of
``stats_per_instance`` -- against the scipy restatement of tests/clean_cases.py.  Everything is an integer: every
comparison is exact, the piece map number for number and every column of the table.

The labelling works on tiles of 4 x 8 x 64 voxels (x, y, z); (11, 19, 150) crosses tile faces, edges and corners at
least twice on every axis with a remainder.  Also extents of 1 and volumes smaller than one tile."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from tests import clean_cases as CC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

VOLUMES = {
    "serpentine": CC.serpentine,
    "u_shape": CC.u_shape,
    "checkerboard_5x6x7": lambda: CC.checkerboard((5, 6, 7)),
    "checkerboard_crossing": lambda: CC.checkerboard(CC.CROSSING),
    "edge_contact": CC.edge_contact,
    "corner_contact": CC.corner_contact,
    "noise_12x13x9": lambda: CC.sparse_noise((12, 13, 9), 1),
    "noise_crossing": lambda: CC.sparse_noise(CC.CROSSING, 2),
    "noise_ids_3_7_300_1000": lambda: CC.sparse_noise((12, 13, 9), 3, ids=(0, 3, 7, 300, 1000)),
    "noise_id_int32_max": lambda: CC.sparse_noise((12, 13, 9), 4, ids=(0, 1, 2 ** 31 - 1)),
    "one_voxel": lambda: np.full((1, 1, 1), 6, np.int32),
    "line_z": lambda: CC.sparse_noise((1, 1, 200), 5, ids=(0, 1, 1, 2)),
    "line_y": lambda: CC.sparse_noise((1, 20, 1), 6, ids=(0, 1, 1, 2)),
    "line_x": lambda: CC.sparse_noise((9, 1, 1), 7, ids=(0, 1, 1, 2)),
    "plane_xz": lambda: CC.sparse_noise((9, 1, 70), 8, ids=(0, 1, 1, 2)),
    "below_one_tile": lambda: CC.sparse_noise((3, 5, 40), 9),
    "all_zero": lambda: np.zeros((5, 9, 66), np.int32),
    "two_blobs": lambda: CC.blob(seed=3, value=2) + CC.blob(seed=4, value=5) * (CC.blob(seed=3) == 0),
    "nested_shells": CC.nested_shells,
    "cavity_with_speck": CC.cavity_with_speck,
    "diagonal_pocket": CC.diagonal_pocket,
    "border_pocket": CC.border_pocket,
    "border_bodies": CC.border_bodies,
    "tie": lambda: CC.TIE,
}


@functools.lru_cache(maxsize=None)
def volume(name):
    if name.startswith("golden:"):
        _, file, key = name.split(":")
        v = np.load(os.path.join(GOLDEN, file))[key]
        v = v[0] if v.ndim == 4 else v                                # (1, X, Y, Z) -> (X, Y, Z)
    else:
        v = VOLUMES[name]()
    v = np.ascontiguousarray(v).astype(np.int64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def want_components(name, connectivity, background):
    return CC.ref_label_components(volume(name), connectivity, background)


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached volumes are read-only


def check_components(name, connectivity, background=False):
    from skoots_amd.lib.morphology import label_components
    want_piece, want_table = want_components(name, connectivity, background)
    piece, table = label_components(on_device(volume(name)), connectivity, background)
    assert piece.dtype == torch.int32 and table.dtype == torch.int64 and piece.is_cuda and table.is_cuda
    assert tuple(piece.shape) == volume(name).shape and tuple(table.shape) == want_table.shape, (table.shape, want_table.shape)
    got = piece.cpu().numpy()
    bad = np.argwhere(got != want_piece)
    assert bad.size == 0, f"{len(bad)} voxels differ, first {bad[0]}: {got[tuple(bad[0])]} != {want_piece[tuple(bad[0])]}"
    t = table.cpu().numpy()
    for k, column in enumerate(CC.COLUMNS):
        assert np.array_equal(t[:, k], want_table[:, k]), column


@pytest.mark.parametrize("connectivity", (6, 18, 26))
@pytest.mark.parametrize("name", list(VOLUMES))
def test_label_components(name, connectivity):
    check_components(name, connectivity)


@pytest.mark.parametrize("name", list(VOLUMES))
def test_label_background(name):
    check_components(name, 26, background=True)     # the background is 6-connected whatever the connectivity says


def test_the_cases_test_what_they_are_for():
    assert [want_components("checkerboard_5x6x7", k, False)[1].shape[0] for k in (6, 18, 26)] == [105, 1, 1]
    assert [want_components("checkerboard_crossing", k, False)[1].shape[0] for k in (18, 26)] == [1, 1]
    assert [want_components("serpentine", k, False)[1].shape[0] for k in (6, 26)] == [1, 1]
    assert [want_components("edge_contact", k, False)[1].shape[0] for k in (18, 26)] == [2, 2]
    ones = [int((want_components("corner_contact", k, False)[1][:, 0] == 1).sum()) for k in (18, 26)]
    assert ones[0] > 1000 and ones[1] == 1
    t = want_components("u_shape", 6, False)[1]
    assert t[:, 1].tolist() == [t[0, 1], 1] and t[0, 1] > 1000   # the lone voxel is number 2
    assert want_components("noise_crossing", 6, False)[1].shape[0] > 300


CLEAN_OPTIONS = [
    dict(components="split"),
    dict(components="largest", fill_holes=True),
    dict(components="split", connectivity=18, min_voxels=3),
    dict(components="largest", connectivity=26, min_voxels=2, clear_border=(False, False, True), fill_holes=True),
    dict(min_voxels=30, fill_holes=True),
    dict(clear_border=True, fill_holes=True),
    dict(fill_holes=True),
]
CLEAN_VOLUMES = ["noise_12x13x9", "noise_crossing", "noise_ids_3_7_300_1000", "two_blobs", "nested_shells",
                 "cavity_with_speck", "diagonal_pocket", "border_pocket", "border_bodies", "tie", "checkerboard_5x6x7",
                 "serpentine", "line_z", "all_zero"]


def check_clean(name, **kwargs):
    from skoots_amd.utils.clean import clean
    want, want_report = CC.ref_clean(volume(name), **kwargs)
    got, report = clean(on_device(volume(name)), **kwargs)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == volume(name).shape
    assert dataclasses.asdict(report) == want_report
    assert all(type(v) is int for v in dataclasses.asdict(report).values())
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"{len(bad)} voxels differ, first {bad[0]}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    return g, report


@pytest.mark.parametrize("kwargs", CLEAN_OPTIONS, ids=str)
@pytest.mark.parametrize("name", CLEAN_VOLUMES)
def test_clean_against_the_restatement(name, kwargs):
    check_clean(name, **kwargs)


def test_tie():
    g, _ = check_clean("tie", components="largest")
    assert g.ravel().tolist() == [4, 4, 4, 0, 0, 0, 0, 0, 0]
    g, report = check_clean("tie", components="split")
    assert g.ravel().tolist() == [4, 4, 4, 0, 0, 5, 5, 5, 0] and report.ids_added == 1


def test_nested_shells():
    g, report = check_clean("nested_shells", fill_holes=True)
    assert g[6, 6, 6] == 9 and g[4, 4, 4] == 0 and (report.holes_filled, report.holes_ambiguous) == (1, 1)
    g, report = check_clean("nested_shells", min_voxels=27, fill_holes=True)      # the shell of 9 has 26 voxels
    assert (g[1:12, 1:12, 1:12] == 5).all() and (g > 0).sum() == 11 ** 3 and report.ids_removed_small == 1


def test_step_order_speck_in_a_cavity():
    g, report = check_clean("cavity_with_speck", min_voxels=200, fill_holes=True)
    assert (g[1:13, 1:13, 1:13] == 2).all() and report.voxels_filled == 343
    g, report = check_clean("cavity_with_speck", fill_holes=True)
    assert np.array_equal(g, volume("cavity_with_speck")) and report.holes_ambiguous == 1


def test_pockets():
    g, _ = check_clean("diagonal_pocket", fill_holes=True)
    assert g[2, 2, 2] == 4 and g[1, 1, 2] == 0
    g, _ = check_clean("diagonal_pocket", connectivity=26, fill_holes=True)      # the background stays 6-connected
    assert g[2, 2, 2] == 4 and g[1, 1, 2] == 0
    g, _ = check_clean("border_pocket", fill_holes=True)
    assert g[0, 3, 3] == 0 and g[3, 3, 3] == 6


def test_clear_border_per_axis():
    g, report = check_clean("border_bodies", clear_border=(True, True, False))
    assert np.unique(g).tolist() == [0, 1, 4] and report.ids_removed_border == 2
    g, _ = check_clean("border_bodies", clear_border=True)
    assert np.unique(g).tolist() == [0, 4]


@pytest.mark.parametrize("name", ["golden:instance_stats.npz:mask", "golden:flood_and_stitch.npz:labels_field21_d0",
                                  "golden:flood_and_stitch.npz:labels_field11_d1",
                                  "golden:flood_and_stitch.npz:labels_field41_d0"])
def test_fixtures(name):
    _, report = check_clean(name, components="split")
    assert report.ids_in_pieces > 0 and report.instances_out == report.pieces
    check_clean(name, components="largest", fill_holes=True)


def test_single_id_fill_is_binary_fill_holes():
    from scipy import ndimage as ndi
    from skoots_amd.utils.clean import clean
    for seed in range(3):
        m = CC.blob(seed=seed, value=7)
        got, _ = clean(on_device(m, torch.uint8), fill_holes=True)
        assert np.array_equal(got.cpu().numpy(), ndi.binary_fill_holes(m > 0) * 7)


def test_repeatable_and_renumbered():
    from skoots_amd.utils.clean import clean
    x = on_device(volume("noise_crossing"))
    kwargs = dict(components="split", connectivity=18, min_voxels=2, fill_holes=True)
    a, ra = clean(x, **kwargs)
    b, rb = clean(x[None], **kwargs)                                  # (1, X, Y, Z) is the same volume
    assert torch.equal(a, b) and ra == rb
    want, want_report = CC.ref_clean(volume("noise_crossing"), renumber=True, **kwargs)
    got, report = clean(x, renumber=True, **kwargs)
    assert np.array_equal(got.cpu().numpy(), want) and dataclasses.asdict(report) == want_report
    flat = got.cpu().numpy().reshape(-1)
    ids, first = np.unique(flat[flat > 0], return_index=True)
    assert ids.tolist() == list(range(1, report.instances_out + 1)) and (np.diff(first) > 0).all()


def test_ids_beyond_int32():
    from skoots_amd.utils.clean import clean
    m = volume("noise_id_int32_max")
    got, _ = clean(on_device(m), components="largest")                # the id itself still fits
    assert np.array_equal(got.cpu().numpy(), CC.ref_clean(m, components="largest")[0])
    with pytest.raises(ValueError, match="renumber=True"):
        clean(on_device(m), components="split")
    want, want_report = CC.ref_clean(m, components="split", renumber=True)
    got, report = clean(on_device(m), components="split", renumber=True)
    assert np.array_equal(got.cpu().numpy(), want) and dataclasses.asdict(report) == want_report
    huge = np.where(m == 1, 2 ** 40, m)                               # an int64 mask
    with pytest.raises(ValueError, match="renumber=True"):
        clean(on_device(huge))
    got, _ = clean(on_device(huge), renumber=True)
    assert np.array_equal(got.cpu().numpy(), CC.ref_clean(huge, renumber=True)[0])


def test_errors_come_before_any_launch(monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import label_components
    from skoots_amd.utils.clean import clean

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    for fn in ("sk_label_components", "sk_component_table", "sk_apply_piece_lut"):
        monkeypatch.setattr(_ffi.lib, fn, refuse, raising=False)
    good = on_device(volume("tie"))
    for run in (label_components, clean):
        with pytest.raises(ValueError, match="no CPU fallback"):
            run(torch.from_numpy(np.array(volume("tie"))))
        with pytest.raises(TypeError, match="integer dtype"):
            run(good.float())
        with pytest.raises(ValueError, match="negative value -7"):
            run(good - 7)
        with pytest.raises(ValueError, match="connectivity"):
            run(good, connectivity=7)
        with pytest.raises(ValueError, match="2\\^31"):
            run(torch.zeros(1, dtype=torch.uint8, device=DEV).expand(2048, 1024, 1024))
    with pytest.raises(ValueError, match="components"):
        clean(good, components="all")
    with pytest.raises(ValueError, match="min_voxels"):
        clean(good, min_voxels=-1)
    with pytest.raises(ValueError, match="clear_border"):
        clean(good, clear_border=(True, False))


def test_c_abi_guards():
    import ctypes as C

    from skoots_amd import _ffi
    L = _ffi.lib
    assert L.sk_abi_version() >= 20 and L.sk_component_table_row_values() == 6
    assert L.sk_label_components_workspace_bytes(2048, 1024, 1024) == 0 and L.sk_label_components_workspace_bytes(0, 4, 4) == 0
    a = torch.full((4, 4, 4), 3, dtype=torch.int32, device=DEV)
    parent, ranks = torch.full_like(a, -7), torch.full_like(a, -7)
    n = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    nbytes = L.sk_label_components_workspace_bytes(4, 4, 4)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = _ffi.stream_ptr(a.device)

    def call(X=4, Y=4, Z=4, connectivity=6, which=1, labels=a, ws=nbytes):
        return L.sk_label_components(_ffi.ptr(labels), X, Y, Z, connectivity, which, _ffi.ptr(parent), _ffi.ptr(ranks),
                                     _ffi.ptr(n), _ffi.ptr(work), C.c_size_t(ws), s)

    assert call(X=2048, Y=1024, Z=1024) == -1 and "2^31" in _ffi.last_error()
    assert call(connectivity=7) == -1 and call(which=2) == -1 and call(Z=0) == -1 and call(ws=nbytes - 1) == -1
    assert call(labels=None) == -1
    rows = torch.full((2, 6), -7, dtype=torch.int64, device=DEV)
    assert L.sk_component_table(_ffi.ptr(a), _ffi.ptr(ranks), 4, 4, 4, -1, _ffi.ptr(rows), s) == -1
    assert L.sk_component_table(_ffi.ptr(a), None, 4, 4, 4, 2, _ffi.ptr(rows), s) == -1
    assert L.sk_apply_piece_lut(_ffi.ptr(ranks), None, 3, _ffi.ptr(parent), 64, 0, s) == -1
    torch.cuda.synchronize()
    assert int(n.item()) == -7 and bool((parent == -7).all()) and bool((ranks == -7).all()) and bool((rows == -7).all())
    assert call() == 0                                               # and the same arguments unbroken do run
    assert int(n.item()) == 1 and bool((ranks == 1).all()) and bool((parent == 0).all())
    # pieces the table was not sized for are skipped, never written out of bounds
    ranks[0, 0, 0] = 9
    assert L.sk_component_table(_ffi.ptr(a), _ffi.ptr(ranks), 4, 4, 4, 1, _ffi.ptr(rows), s) == 0
    assert rows.cpu().tolist() == [[3, 63, 1, 63, 0, 0], [-7] * 6]
    out = torch.full_like(a, -7)
    lut = torch.tensor([5, 8], dtype=torch.int32, device=DEV)
    assert L.sk_apply_piece_lut(_ffi.ptr(ranks), _ffi.ptr(lut), 2, _ffi.ptr(out), 64, 0, s) == 0
    assert out[0, 0, 0].item() == 0 and bool((out.reshape(-1)[1:] == 8).all())


def test_command(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import clean as CL
    m = volume("two_blobs")
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, on_device(m).permute(2, 0, 1).contiguous())          # stored [Z, X, Y]
    before = open(path, "rb").read()
    out_path = CL.main([path, "--components", "split", "--min-voxels", "4", "--clear-border", "x", "y", "--fill-holes"])
    assert out_path == str(tmp_path / "mask_cleaned.tif") and open(path, "rb").read() == before
    want, report = CL.clean(on_device(m), components="split", min_voxels=4, clear_border=(True, True, False),
                            fill_holes=True)
    back = tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32)
    assert torch.equal(back, want)
    assert np.array_equal(want.cpu().numpy(), CC.ref_clean(m, components="split", min_voxels=4,
                                                           clear_border=(True, True, False), fill_holes=True)[0])
    lines = capsys.readouterr().out.splitlines()
    assert lines[:12] == [f"{k}: {v}" for k, v in dataclasses.asdict(report).items()]
    assert lines[12] == f"File Written: {out_path}"
    with pytest.raises(SystemExit):
        CL.main([path])
    assert open(path, "rb").read() == before
    assert CL.main([path, "--renumber", "-o"]) == path
    assert torch.equal(tiff.read_stack(path, DEV).permute(1, 2, 0).to(torch.int32), CL.clean(on_device(m), renumber=True)[0])


def test_pieces_columns_of_stats_per_instance(tmp_path):
    from scipy import ndimage as ndi
    from skoots_amd.validate import compare as CMP
    m = volume("golden:instance_stats.npz:mask")
    x = on_device(m)
    plain = CMP.stats_per_instance(x, (1.0, 1.0, 2.0))
    assert "pieces" not in plain
    for k in (26, 6):
        got = CMP.stats_per_instance(x, (1.0, 1.0, 2.0), pieces=k)
        ids = got["id"].cpu().tolist()
        labelled = [ndi.label(m == u, CC.structure(k)) for u in ids]
        assert got["pieces"].cpu().tolist() == [n for _, n in labelled]
        assert got["largest_piece_voxels"].cpu().tolist() == [int(np.bincount(lab.reshape(-1))[1:].max()) for lab, _ in labelled]
        assert all(torch.equal(got[c], plain[c]) for c in plain)
    assert max(got["pieces"].cpu().tolist()) > 1
    with pytest.raises(ValueError, match="pieces"):
        CMP.stats_per_instance(x, pieces=8)
    # the command: the same file with and without the option differs by the two columns only
    from skoots_amd.lib import tiff
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    text = open(CMP.main([path, "--out", str(tmp_path / "a.csv")])).read()
    with_pieces = open(CMP.main([path, "--pieces", "6", "--out", str(tmp_path / "b.csv")])).read()
    a, b = text.splitlines(), with_pieces.splitlines()
    assert a[:2] == b[:2] and b[2] == a[2] + ",pieces,largest_piece_voxels"
    got = CMP.stats_per_instance(x, pieces=6)
    for i, (la, lb) in enumerate(zip(a[3:], b[3:])):
        assert lb == f"{la},{got['pieces'][i].item()},{got['largest_piece_voxels'][i].item()}"
