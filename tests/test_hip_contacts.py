"""``sk_instance_contacts`` (skoots_amd/csrc/contacts.hip) and what stands on it -- ``validate.lib.instance_contacts``, the
contact columns of ``stats_per_instance`` and the ``--contacts`` files, ``utils.merge.merge`` and its command -- against
the numpy restatement of tests/contact_cases.py.  Everything is an integer: every comparison is exact, row for row.

The kernel works on tiles of 4 x 16 x 64 voxels (x, y, z) with a forward halo; (11, 19, 150) crosses the tile at least
twice on every axis with a remainder, so contacts across tile faces, edges and corners all occur.  The tile's LDS table
holds 256 pairs: ``voxel_ids`` and ``many_ids`` give a tile thousands, so the direct path to the global table runs."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import contact_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = [(c, b) for c in (6, 18, 26) for b in (False, True)]

VOLUMES = {
    "noise_12x13x9": lambda: K.sparse_noise((12, 13, 9), 1),
    "noise_crossing": lambda: K.sparse_noise(K.CROSSING, 2),
    "edge_contact": K.edge_contact,
    "corner_contact": K.corner_contact,
    "noise_ids_3_7_300_1000": lambda: K.sparse_noise((12, 13, 9), 3, ids=(0, 3, 7, 300, 1000)),
    "noise_id_int32_max": lambda: K.sparse_noise((12, 13, 9), 4, ids=(0, 1, 2 ** 31 - 1)),
    "line_z": lambda: K.sparse_noise((1, 1, 200), 5, ids=(0, 1, 1, 2)),
    "line_y": lambda: K.sparse_noise((1, 20, 1), 6, ids=(0, 1, 1, 2)),
    "line_x": lambda: K.sparse_noise((9, 1, 1), 7, ids=(0, 1, 1, 2)),
    "plane_xz": lambda: K.sparse_noise((9, 1, 70), 8, ids=(0, 1, 1, 2)),
    "one_voxel": lambda: np.full((1, 1, 1), 6, np.int32),
    "all_zero": lambda: np.zeros((5, 9, 66), np.int32),
    "below_one_tile": lambda: K.sparse_noise((3, 5, 40), 9),
    "voxel_ids": lambda: K.voxel_ids((5, 6, 70)),
    "many_ids": lambda: K.many_ids(K.CROSSING, 400, 10),
    "split_blob": K.split_blob,
}


@functools.lru_cache(maxsize=None)
def volume(name):
    v = np.ascontiguousarray(VOLUMES[name]()).astype(np.int64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def want_contacts(name, connectivity, background):
    t = K.ref_contacts(volume(name), connectivity, background)
    t.setflags(write=False)
    return t


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached volumes are read-only


def check_contacts(name, connectivity, background, dtype=None, **kw):
    from skoots_amd.validate.lib import instance_contacts
    ids, table = instance_contacts(on_device(volume(name), dtype), connectivity, background, **kw)
    assert ids.dtype == torch.int64 and table.dtype == torch.int64 and table.is_cuda and table.ndim == 2
    assert np.array_equal(ids.cpu().numpy(), K.rows_of(volume(name))[1])
    assert np.array_equal(table.cpu().numpy(), want_contacts(name, connectivity, background))
    return table


@pytest.mark.parametrize("connectivity,background", MODES)
@pytest.mark.parametrize("name", sorted(set(VOLUMES) - {"voxel_ids", "many_ids"}))
def test_table_equals_the_definition(name, connectivity, background):
    check_contacts(name, connectivity, background)


@pytest.mark.parametrize("connectivity,background", MODES)
@pytest.mark.parametrize("name", ["voxel_ids", "many_ids"])
def test_more_pairs_than_the_tile_table_holds(name, connectivity, background):
    table = check_contacts(name, connectivity, background)
    # more than twice as many distinct pairs as all its tiles' LDS tables hold together: some tile overflows
    tiles = int(np.prod([-(-n // t) for n, t in zip(volume(name).shape, K.TILE)]))
    assert table.shape[0] > 2 * 256 * tiles


def test_pair_counts_of_the_overflow_volumes():
    """every pair of neighbouring voxels of ``voxel_ids`` is a key of its own: their number is that of the grid"""
    X, Y, Z = volume("voxel_ids").shape
    pairs = sum((X - abs(a)) * (Y - abs(b)) * (Z - abs(c)) for a, b, c in K.FORWARD)
    assert want_contacts("voxel_ids", 26, False).shape[0] == pairs == 20582
    assert (want_contacts("voxel_ids", 26, False)[:, 2:].sum(1) == 1).all()


@pytest.mark.parametrize("connectivity,background", [(6, False), (26, True)])
def test_int64_mask(connectivity, background):
    check_contacts("noise_ids_3_7_300_1000", connectivity, background, dtype=torch.int64)
    v = volume("noise_12x13x9") * (2 ** 40)               # ids beyond int32: the relabel path of the prologue
    from skoots_amd.validate.lib import instance_contacts
    ids, table = instance_contacts(on_device(v), connectivity, background)
    assert ids.cpu().tolist() == [2 ** 40, 2 ** 41, 3 * 2 ** 40]
    assert np.array_equal(table.cpu().numpy(), want_contacts("noise_12x13x9", connectivity, background))


def test_rows_argument_and_four_dimensions():
    from skoots_amd.validate.lib import id_rows, instance_contacts
    x = on_device(volume("noise_crossing"))
    a = instance_contacts(x, 18, True)[1]
    b = instance_contacts(x[None], 18, True, rows=id_rows(x[None]))[1]
    assert torch.equal(a, b)


# ---- capacity and the retry ----

def raw_call(v, connectivity, background, capacity, guard=8):
    """sk_instance_contacts through the C ABI on sentinel-filled buffers: (status, rows with the guard tail, counts)"""
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    x, (a, ids, lut, max_id) = id_rows(on_device(v))
    L = _ffi.lib
    rows = torch.full((capacity + guard, 9), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(L.sk_instance_contacts_workspace_bytes(capacity))
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    X, Y, Z = (int(n) for n in a.shape)
    status = L.sk_instance_contacts(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut), max_id, int(ids.numel()), connectivity,
                                    int(background), _ffi.ptr(rows), capacity, _ffi.ptr(counts), _ffi.ptr(work),
                                    C.c_size_t(nbytes), _ffi.stream_ptr(a.device))
    torch.cuda.synchronize()
    return status, rows.cpu().numpy(), counts.cpu().tolist()


def test_a_small_capacity_is_refused_then_retried():
    status, rows, (stored, refused) = raw_call(volume("voxel_ids"), 26, False, 64)
    assert status == 0 and refused > 0 and 0 < stored <= 64          # a handled path, not a fault
    assert stored + refused >= want_contacts("voxel_ids", 26, False).shape[0]
    assert (rows[stored:] == -7).all()                               # nothing behind the rows, nothing in the guard
    # what was stored is exact: a key is stored for the whole launch or not at all
    want = {tuple(r[:2]): tuple(r[2:]) for r in want_contacts("voxel_ids", 26, False).tolist()}
    assert len({tuple(r[:2]) for r in rows[:stored].tolist()}) == stored
    assert all(want[tuple(r[:2])] == tuple(r[2:]) for r in rows[:stored].tolist())
    check_contacts("voxel_ids", 26, False, capacity=64)              # the library call retries to the same table
    check_contacts("many_ids", 18, True, capacity=1)


def test_capacity_argument_of_the_library():
    from skoots_amd.validate.lib import instance_contacts
    x = on_device(volume("noise_12x13x9"))
    for bad in (0, 3, -4):
        with pytest.raises(ValueError, match="power of two"):
            instance_contacts(x, capacity=bad)
    with pytest.raises(ValueError, match="connectivity"):
        instance_contacts(x, connectivity=8)
    with pytest.raises(ValueError, match="connectivity"):
        instance_contacts(x, connectivity=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_contacts(x.cpu())


@pytest.mark.parametrize("connectivity,background", [(6, True), (26, False)])
def test_buffers_beyond_the_rows_stay_untouched_and_runs_agree(connectivity, background):
    want = want_contacts("noise_crossing", connectivity, background)
    tables = []
    for _ in range(2):
        status, rows, (stored, refused) = raw_call(volume("noise_crossing"), connectivity, background, 32)
        assert status == 0 and refused == 0 and stored == want.shape[0]
        assert (rows[stored:] == -7).all()
        t = rows[:stored]
        tables.append(t[np.lexsort((t[:, 1], t[:, 0]))])
    assert np.array_equal(tables[0], want) and np.array_equal(tables[1], want)


def test_c_abi_guards():
    from skoots_amd import _ffi
    L = _ffi.lib
    assert L.sk_abi_version() >= 23 and L.sk_instance_contacts_row_values() == 9
    assert L.sk_instance_contacts_workspace_bytes(0) == 0 and L.sk_instance_contacts_workspace_bytes(-8) == 0
    assert L.sk_instance_contacts_workspace_bytes(16) >= 16 * 8 * 8
    a = torch.tensor([1, 2], dtype=torch.int32, device=DEV).repeat(4, 4, 2)          # (4, 4, 4): z alternates 1, 2
    lut = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    rows = torch.full((16 + 4, 9), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(L.sk_instance_contacts_workspace_bytes(16))
    work = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=DEV)
    s = _ffi.stream_ptr(a.device)
    P = _ffi.ptr

    def call(X=4, Y=4, Z=4, N=2, max_id=2, connectivity=6, background=0, capacity=16, ws=nbytes, labels=P(a), table=P(lut),
             out=P(rows), cnt=P(counts), wsp=P(work)):
        return L.sk_instance_contacts(labels, X, Y, Z, table, max_id, N, connectivity, background, out, capacity, cnt, wsp,
                                      C.c_size_t(ws), s)

    assert call(X=-1) == -1 and "negative" in _ffi.last_error()
    assert call(Y=-1) == -1 and call(Z=-1) == -1 and call(N=-1) == -1 and call(max_id=-1) == -1
    assert call(connectivity=7) == -1 and "connectivity" in _ffi.last_error()
    assert call(connectivity=0) == -1 and call(background=2) == -1 and call(background=-1) == -1
    assert call(capacity=0) == -1 and "power of two" in _ffi.last_error()
    assert call(capacity=12) == -1 and call(capacity=-16) == -1
    assert call(ws=nbytes - 1) == -1 and "workspace" in _ffi.last_error()
    assert call(capacity=32) == -1                                   # the workspace is that of 16
    for name in ("labels", "table", "out", "cnt", "wsp"):
        assert call(**{name: None}) == -1 and "NULL" in _ffi.last_error()
    assert call(labels=C.c_void_p(a.data_ptr() + 2)) == -1 and "aligned" in _ffi.last_error()
    assert call(table=C.c_void_p(lut.data_ptr() + 1)) == -1 and call(out=C.c_void_p(rows.data_ptr() + 4)) == -1
    assert call(cnt=C.c_void_p(counts.data_ptr() + 4)) == -1 and call(wsp=C.c_void_p(work.data_ptr() + 4)) == -1
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((counts == -7).all()) and bool((work == 0x55).all())
    # an empty volume or no rows: counts = {0, 0}, nothing else, the mask is not looked at
    assert call(Z=0, labels=None, table=None) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and bool((rows == -7).all())
    counts.fill_(-7)
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and bool((rows == -7).all())
    assert call() == 0                                               # and the same arguments unbroken do run
    torch.cuda.synchronize()
    assert counts.tolist() == [1, 0] and rows[0].tolist() == [1, 2, 0, 0, 48, 0, 0, 0, 0] and bool((rows[1:] == -7).all())
    assert bool((work[nbytes:] == 0x55).all())


# ---- stats_per_instance(contacts=...) ----

@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_contact_columns_of_stats_per_instance(connectivity):
    from skoots_amd.validate import compare as CMP
    m = volume("noise_ids_3_7_300_1000")
    x = on_device(m)
    spacing = (1.0, 0.5, 2.0)
    plain = CMP.stats_per_instance(x, spacing)
    assert "neighbours" not in plain and "contact_table" not in plain
    got = CMP.stats_per_instance(x, spacing, contacts=connectivity)
    assert all(torch.equal(got[c], plain[c]) for c in plain)
    ids = K.rows_of(m)[1]
    want_table = K.with_ids(want_contacts("noise_ids_3_7_300_1000", connectivity, False), ids)
    assert got["contact_table"].is_cuda and np.array_equal(got["contact_table"].cpu().numpy(), want_table)
    assert np.array_equal(got["faces"].cpu().numpy(), K.exposed_faces(m))
    face_area = got["face_area"].cpu().numpy()            # derive's value of those faces, an existing column
    want = CMP.contact_columns(want_table, ids, face_area, spacing)
    for k in CMP.CONTACT_COLUMNS.split(","):
        assert got[k].is_cuda and got[k].dtype == want[k].dtype and got[k].cpu().tolist() == want[k].tolist(), k
    assert got["neighbours"].cpu().tolist() == [3, 3, 3, 3] and float(got["contact_fraction"].min()) > 0


@pytest.mark.parametrize("name", ["noise_crossing", "many_ids", "split_blob", "edge_contact"])
def test_faces_are_contacts_plus_border_voxels_on_the_device(name):
    """connectivity 6 with background: the contacts of an id over all partners plus its voxels in the border planes are
    the exposed faces that ``sk_instance_stats`` counts for it, per axis"""
    from skoots_amd.validate.lib import id_rows, instance_contacts, instance_sums
    x = on_device(volume(name))
    rows = id_rows(x)
    ids, table = instance_contacts(x, 6, True, rows)
    faces = instance_sums(x, rows)[1][:, 10:13].cpu().numpy()
    t = table.cpu().numpy()
    assert np.array_equal(K.face_contacts_per_row(t, int(ids.numel())) + K.border_voxels(volume(name)), faces)


# ---- merge ----

def test_merge_joins_the_halves_and_leaves_the_third():
    from skoots_amd.utils.merge import MergeReport, merge
    m = volume("split_blob")
    x = on_device(m)
    out, report = merge(x, min_contact_fraction=0.15)
    assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == m.shape
    assert np.array_equal(out.cpu().numpy(), K.ref_merge(m, [(2, 5)]))
    assert report == MergeReport(instances_in=3, pairs_touching=1, pairs_merged=1, pairs_explicit=0,
                                 pairs_explicit_not_touching=0, groups=1, voxels_relabelled=int((m == 5).sum()),
                                 instances_out=2)
    again, report2 = merge(x[None].to(torch.int64), min_contact_fraction=0.15)
    assert torch.equal(again, out) and report2 == report
    # the wall has about 150 faces along y: at this spacing its area is 150 sx sz
    wall = int(want_contacts("split_blob", 6, False)[0, 3])
    assert torch.equal(merge(x, spacing=(2.0, 1.0, 0.5), min_contact_area=wall)[0], out)
    same, none = merge(x, spacing=(2.0, 1.0, 0.5), min_contact_area=wall + 1)
    assert torch.equal(same, x) and none.pairs_merged == 0 and none.groups == 0 and none.voxels_relabelled == 0
    assert none.instances_out == 3


def test_merge_explicit_pairs_and_renumber():
    from skoots_amd.utils.merge import merge
    m = volume("split_blob")
    x = on_device(m)
    out, report = merge(x, pairs=[(9, 5)])
    assert np.array_equal(out.cpu().numpy(), K.ref_merge(m, [(5, 9)]))
    assert report.pairs_explicit == 1 and report.pairs_explicit_not_touching == 1 and report.pairs_merged == 0
    assert report.voxels_relabelled == int((m == 9).sum()) and report.instances_out == 2
    out, report = merge(x, pairs=[(9, 5)], min_contact_fraction=0.15, renumber=True)
    assert np.array_equal(out.cpu().numpy(), (m > 0).astype(np.int64)) and report.instances_out == 1 and report.groups == 1
    out, _ = merge(x, pairs=[(9, 2)], renumber=True)
    assert np.array_equal(out.cpu().numpy(), K.ref_renumber(K.ref_merge(m, [(2, 9)])))
    # two voxels that share an edge only: not touching at 6; touching at 18, without area
    e = np.zeros((3, 3, 3), np.int32)
    e[0, 0, 0], e[1, 1, 0] = 4, 6
    got, report = merge(on_device(e), connectivity=6, min_contact_area=0)
    assert report.pairs_touching == 0 and torch.equal(got, on_device(e))
    got, report = merge(on_device(e), connectivity=18, min_contact_area=0)
    assert report.pairs_touching == 1 and report.pairs_merged == 1 and np.array_equal(got.cpu().numpy(), 4 * (e > 0))
    assert merge(on_device(e), connectivity=18, min_contact_fraction=0.01)[1].pairs_merged == 0
    huge = volume("noise_12x13x9") * (2 ** 40)
    with pytest.raises(ValueError, match="beyond int32"):
        merge(on_device(huge), pairs=[(2 ** 40, 2 ** 41)])
    out, _ = merge(on_device(huge), pairs=[(2 ** 40, 2 ** 41)], renumber=True)
    assert np.array_equal(out.cpu().numpy(), K.ref_renumber(K.ref_merge(huge, [(2 ** 40, 2 ** 41)])))


def test_merge_errors_come_before_any_launch(monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.utils.merge import merge

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    good = on_device(volume("split_blob"))
    monkeypatch.setattr(_ffi.lib, "sk_instance_contacts", refuse, raising=False)
    with pytest.raises(ValueError, match="no CPU fallback"):
        merge(good.cpu(), min_contact_area=1)
    with pytest.raises(TypeError, match="integer dtype"):
        merge(good.float(), min_contact_area=1)
    with pytest.raises(ValueError, match="negative value -3"):
        merge(good - 3, min_contact_area=1)
    with pytest.raises(ValueError, match="nothing to decide"):
        merge(good)
    with pytest.raises(ValueError, match="min_contact_fraction"):
        merge(good, min_contact_fraction=-0.5)
    with pytest.raises(ValueError, match="connectivity"):
        merge(good, connectivity=7, min_contact_area=1)
    monkeypatch.undo()
    with pytest.raises(ValueError, match=r"\[4\]"):
        merge(good, pairs=[(2, 4)])
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        merge(torch.zeros_like(good), pairs=[(1, 2)])
    out, report = merge(torch.zeros_like(good), min_contact_area=1)
    assert not bool(out.any()) and report.instances_in == 0


# ---- both commands on files ----

def test_compare_command_writes_the_contact_files(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate import compare as CMP
    m = volume("noise_ids_3_7_300_1000")
    x = on_device(m)
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())            # stored [Z, X, Y]
    spacing = (1.0, 0.5, 2.0)
    plain = open(CMP.main([path, "--spacing", "1", "0.5", "2", "--out", str(tmp_path / "a.csv")])).read()
    assert not (tmp_path / "mask_contacts.csv").exists()
    stats_path = CMP.main([path, "--spacing", "1", "0.5", "2", "--contacts", "18"])
    assert stats_path == str(tmp_path / "mask_instance_stats.csv")
    ids = K.rows_of(m)[1]
    table = K.with_ids(want_contacts("noise_ids_3_7_300_1000", 18, False), ids)
    got = CMP.stats_per_instance(x, spacing)
    want_stats = CMP.format_csv(path, ids, got["sums"], got["bbox"], m.shape, spacing, contact_table=table)
    want_pairs = CMP.format_contacts_csv(path, table, ids, got["face_area"], spacing, 18)
    stats, pairs = open(stats_path, "rb").read(), open(tmp_path / "mask_contacts.csv", "rb").read()
    assert stats.decode() == want_stats and pairs.decode() == want_pairs
    a, b = plain.splitlines(), want_stats.splitlines()
    assert a[:2] == b[:2] and b[2] == a[2] + "," + CMP.CONTACT_COLUMNS and all(lb.startswith(la + ",") for la, lb in
                                                                               zip(a[3:], b[3:]))
    assert len(pairs.decode().splitlines()) == 3 + table.shape[0] and table.shape[0] == 6
    CMP.main([path, "--spacing", "1", "0.5", "2", "--contacts", "18"])
    assert open(stats_path, "rb").read() == stats and open(tmp_path / "mask_contacts.csv", "rb").read() == pairs


def test_merge_command(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import merge as MG
    m = volume("split_blob")
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, on_device(m).permute(2, 0, 1).contiguous())          # stored [Z, X, Y]
    before = open(path, "rb").read()
    out_path = MG.main([path, "--min-contact-fraction", "0.15", "--pairs", "9", "2"])
    assert out_path == str(tmp_path / "mask_merged.tif") and open(path, "rb").read() == before
    want, report = MG.merge(on_device(m), min_contact_fraction=0.15, pairs=[(9, 2)])
    back = tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32)
    assert torch.equal(back, want) and np.array_equal(want.cpu().numpy(), 2 * (m > 0))
    lines = capsys.readouterr().out.splitlines()
    assert lines[:8] == [f"{k}: {v}" for k, v in dataclasses.asdict(report).items()]
    assert lines[8] == f"File Written: {out_path}"
    first = open(out_path, "rb").read()
    MG.main([path, "--min-contact-fraction", "0.15", "--pairs", "9", "2"])
    assert open(out_path, "rb").read() == first
    with pytest.raises(SystemExit):
        MG.main([path])
    with pytest.raises(SystemExit):
        MG.main([path, "--pairs", "2", "5", "9"])
    assert open(path, "rb").read() == before
    assert MG.main([path, "--min-contact-area", "100", "--renumber", "-o"]) == path
    assert torch.equal(tiff.read_stack(path, DEV).permute(1, 2, 0).to(torch.int32),
                       MG.merge(on_device(m), min_contact_area=100, renumber=True)[0])
