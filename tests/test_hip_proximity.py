"""``sk_instance_proximity`` (skoots_amd/csrc/proximity.hip) and what stands on it -- ``validate.lib.instance_proximity``,
``utils.proximity.proximity`` and its command, the near columns of ``stats_per_instance`` -- against the numpy
restatement of tests/proximity_cases.py.  Everything is an integer or an fp64 bit pattern: every comparison is exact,
row for row, and a second call gives the same tensors.

The kernel takes tiles of 4 x 16 x 64 voxels, lanes along z, and stages the rows of B of the tile grown by the reach;
``K.CROSSING`` = (11, 19, 150) crosses a tile at least twice per axis with a remainder.  A lane keeps 4 partners in
registers and a tile 256 keys in LDS: ``voxel_ids`` gives a voxel dozens of partners and a tile thousands of keys, so the
rescan, the overflow of the LDS table and the direct path to the global table run."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from tests import contact_cases as K
from tests import proximity_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = (1.0, 1.0, 1.0)


def frozen(*arrays):
    out = tuple(np.ascontiguousarray(v).astype(np.int64) for v in arrays)
    for v in out:
        v.setflags(write=False)
    return out


PAIRS = {
    "noise": lambda: P.noise_pair(K.CROSSING, 5),
    "reach5": lambda: P.noise_pair((7, 7, 70), 6, (0,) * 300 + (1, 2, 3)),
    "faces": P.faces_pair,
    "line_z": lambda: P.noise_pair((1, 1, 200), 7),
    "line_y": lambda: P.noise_pair((1, 20, 1), 8, (0, 1, 2)),
    "line_x": lambda: P.noise_pair((9, 1, 1), 9, (0, 1, 2)),
    "sheet_xz": lambda: P.noise_pair((9, 1, 70), 10),
    "voxel_ids": P.voxel_ids_pair,
    "many_ids": P.many_ids_pair,
    "balls": P.balls_pair,
    "zero_a": lambda: (np.zeros((5, 9, 66), np.int64), K.sparse_noise((5, 9, 66), 12)),
    "zero_b": lambda: (K.sparse_noise((5, 9, 66), 13), np.zeros((5, 9, 66), np.int64)),
    "ids_3_7_300_1000": lambda: P.noise_pair((12, 13, 9), 3, (0, 0, 0, 3, 7, 300, 1000)),
    "id_int32_max": lambda: P.noise_pair((12, 13, 9), 4, (0, 0, 1, 2 ** 31 - 1)),
}


@functools.lru_cache(maxsize=None)
def pair(name):
    return frozen(*PAIRS[name]())


@functools.lru_cache(maxsize=None)
def want(name, distance, spacing=UNIT, same=False):
    a, b = pair(name)
    pairs, gap2 = P.ref_proximity(a, None if same else b, distance, spacing)
    pairs.setflags(write=False)
    gap2.setflags(write=False)
    return pairs, gap2


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached volumes are read-only


def bits(t):
    return torch.as_tensor(t).cpu().contiguous().numpy().view(np.int64)


def assert_equals(got, expected):
    ids_a, ids_b, pairs, gap2 = got
    assert pairs.dtype == torch.int64 and gap2.dtype == torch.float64 and pairs.is_cuda and gap2.is_cuda
    assert tuple(pairs.shape) == expected[0].shape and tuple(gap2.shape) == expected[1].shape
    assert np.array_equal(pairs.cpu().numpy(), expected[0])
    assert np.array_equal(bits(gap2), expected[1].view(np.int64))


def check(name, distance, spacing=UNIT, same=False, dtype=None, **kw):
    from skoots_amd.validate.lib import instance_proximity
    a, b = pair(name)
    xa, xb = on_device(a, dtype), (None if same else on_device(b, dtype))
    got = instance_proximity(xa, xb, distance, spacing, **kw)
    assert np.array_equal(got[0].cpu().numpy(), K.rows_of(a)[1])
    assert np.array_equal(got[1].cpu().numpy(), K.rows_of(a if same else b)[1])
    assert_equals(got, want(name, distance, spacing, same))
    again = instance_proximity(xa, xb, distance, spacing, **kw)
    assert torch.equal(got[2], again[2]) and torch.equal(bits_t(got[3]), bits_t(again[3]))
    return got


def bits_t(t):
    return t.view(torch.int64)


# ---- the table against the definition ----

@pytest.mark.parametrize("spacing, distance", [(UNIT, 2.0), ((1.0, 1.0, 3.0), 3.0), ((0.5, 0.7, 1.3), 1.5)])
def test_noise_pairs_equal_the_definition(spacing, distance):
    got = check("noise", distance, spacing)
    assert got[2].shape[0] == 9 + 3                       # every pair of 3 x 3 instances and the union rows


def test_distance_zero_is_the_overlap_table():
    from skoots_amd.validate.lib import instance_overlaps
    ids_a, ids_b, pairs, gap2 = check("noise", 0.0, (1.0, 1.0, 3.0))
    a, b = (on_device(v) for v in pair("noise"))
    table = instance_overlaps(a, b)[2]
    assert torch.equal(pairs[pairs[:, 1] > 0], table) and bool((gap2 == 0).all())
    union = torch.zeros(4, dtype=torch.int64, device=DEV).index_add_(0, table[:, 0], table[:, 2])[1:]
    assert torch.equal(pairs[pairs[:, 1] == 0][:, 2], union)


@pytest.mark.parametrize("spacing, distance", [(UNIT, 0.0), ((1.0, 1.0, 3.0), 2.0), ((1.0, 1.0, 3.0), 3.0), (UNIT, 3.0),
                                               ((1.0, 1.0, 3.0), 5.0), (UNIT, 5.0)])
def test_workgroups_per_cu_are_what_the_runtime_says(spacing, distance):
    """the reach query's residency -- LDS, wave slots and the registers the kernel is compiled for -- against the
    runtime's occupancy query for the kernel and the dynamic LDS that are launched at that reach"""
    from skoots_amd import _ffi
    w, limit2 = P.metric(distance, spacing)
    out, n = np.zeros(8, np.int32), np.zeros(1, np.int32)
    _ffi.check(_ffi.lib.sk_instance_proximity_reach(*w, limit2, out.ctypes.data))
    _ffi.check(_ffi.lib.sk_instance_proximity_resident(*w, limit2, n.ctypes.data))
    assert out[3] == 1 and out[5] == n[0] >= 1 and out[6] in (512, 1024)
    assert (out[6] == 512) == (2 * out[4] <= 160 * 1024) and (out[5] >= 2) == (out[6] == 512)


def test_the_largest_reach():
    from skoots_amd.validate.lib import proximity_reach
    assert proximity_reach(5.0) == (5, 5, 5)
    got = check("reach5", 5.0)
    assert got[2].shape[0] == 12 and float(got[3].max()) >= 5.0   # partners found only voxels away, off every axis


@pytest.mark.parametrize("name, a_at, b_at, beyond, distance", [
    ("face_x", (3, 8, 30), (5, 8, 30), (6, 8, 30), 2.0),
    ("face_y", (1, 15, 30), (1, 17, 30), (1, 18, 30), 2.0),
    ("face_z", (1, 8, 63), (1, 8, 65), (1, 8, 66), 2.0),
    ("face_z_far_tile", (9, 33, 126), (9, 33, 129), (9, 33, 130), 3.0),
    ("edge_xy", (2, 14, 30), (5, 18, 30), (5, 19, 30), 5.0),      # 3-4-5 across the x and y faces of a tile
    ("edge_xz", (7, 3, 61), (11, 3, 64), (11, 3, 65), 5.0),
    ("corner", (3, 15, 63), (4, 17, 65), (4, 17, 66), 3.0),       # 1-2-2 across the corner (4, 16, 64)
    ("corner_back", (4, 16, 64), (3, 14, 62), (3, 14, 61), 3.0)])
def test_two_voxels_at_the_distance_and_one_beyond(name, a_at, b_at, beyond, distance):
    from skoots_amd.validate.lib import instance_proximity
    shape = (12, 35, 134)
    for q, rows in ((b_at, 2), (beyond, 0)):
        a, b = P.two_voxels(shape, a_at, q)
        expected = P.ref_proximity(a, b, distance)
        assert expected[0].shape[0] == rows                # at the distance counts (<=): a pair row and the union row
        for x, y in ((a, b), (b, a)):
            assert_equals(instance_proximity(on_device(x), on_device(y), distance), P.ref_proximity(x, y, distance))
    if rows == 2:
        assert expected[1].tolist() == [distance * distance] * 2


def test_instances_on_every_face_of_the_volume():
    check("faces", 2.0)
    check("faces", 3.0, (1.0, 1.0, 3.0), same=True)


@pytest.mark.parametrize("name", ["line_z", "line_y", "line_x", "sheet_xz"])
def test_degenerate_shapes(name):
    check(name, 2.0)
    check(name, 3.0, (1.0, 1.0, 3.0), same=True)


def test_a_voxel_with_dozens_of_partners():
    """b holds one id per voxel: the seen list overflows into the rescan, the tile's table into the global one"""
    ids_a, ids_b, pairs, gap2 = check("voxel_ids", 2.0)
    assert pairs.shape[0] > 4 * P.LDS_SLOTS and int(pairs[pairs[:, 1] > 0, 2].max()) > 2 * P.SEEN
    check("voxel_ids", 2.0, same=False, capacity=1 << 15)
    # and the other direction: every voxel of a has few partners, every row of a thousands
    from skoots_amd.validate.lib import instance_proximity
    a, b = pair("voxel_ids")
    assert_equals(instance_proximity(on_device(b), on_device(a), 2.0), P.ref_proximity(b, a, 2.0))


@pytest.mark.parametrize("capacity", [1, 64])
def test_a_small_capacity_is_retried(capacity, monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import instance_proximity
    calls = []
    real = _ffi.lib.sk_instance_proximity
    monkeypatch.setattr(_ffi.lib, "sk_instance_proximity", lambda *args: (calls.append(int(args[17])), real(*args))[1])
    a, b = (on_device(v) for v in pair("many_ids"))
    got = instance_proximity(a, b, 1.0, capacity=capacity)
    assert_equals(got, want("many_ids", 1.0))
    assert len(calls) > 1 and calls[0] == capacity and calls == sorted(set(calls))
    assert calls[-1] >= want("many_ids", 1.0)[0].shape[0]


def test_the_retry_stops_at_the_largest_table(monkeypatch):
    from skoots_amd.validate import lib
    monkeypatch.setattr(lib, "MAX_PROXIMITY_CAPACITY", 4)
    a, b = (on_device(v) for v in pair("many_ids"))
    with pytest.raises(RuntimeError, match="more than 4"):
        lib.instance_proximity(a, b, 1.0, capacity=1)


@pytest.mark.parametrize("spacing, distance", [(UNIT, 2.0), ((1.0, 1.0, 3.0), 3.0)])
def test_one_mask_mode(spacing, distance):
    ids_a, ids_b, pairs, gap2 = check("noise", distance, spacing, same=True)
    assert torch.equal(ids_a, ids_b) and not bool((pairs[:, 0] == pairs[:, 1]).any())
    table = {(r[0], r[1]): g for r, g in zip(pairs.tolist(), bits(gap2).tolist())}
    assert len(table) == 6 + 3 and all(table[(k[1], k[0])] == g for k, g in table.items() if k[1])
    check("balls", 5.0, (1.0, 1.0, 3.0), same=True)


@pytest.mark.parametrize("name", ["zero_a", "zero_b"])
def test_a_side_without_instances(name):
    for same in (False, True):
        got = check(name, 2.0, same=same)
        assert (got[2].shape[0] == 0) == (not same or name == "zero_a")


def test_an_empty_volume():
    from skoots_amd.validate.lib import instance_proximity
    empty = torch.zeros((4, 0, 9), dtype=torch.int32, device=DEV)
    ids_a, ids_b, pairs, gap2 = instance_proximity(empty, empty, 2.0)
    assert ids_a.numel() == ids_b.numel() == 0 and tuple(pairs.shape) == (0, 3) and tuple(gap2.shape) == (0,)
    assert instance_proximity(empty, None, 2.0)[2].shape == (0, 3)


def test_sparse_and_huge_ids():
    from skoots_amd.validate.lib import instance_proximity
    check("ids_3_7_300_1000", 2.0)
    check("ids_3_7_300_1000", 2.0, dtype=torch.int64)
    check("id_int32_max", 1.5, (0.5, 0.7, 1.3))
    a, b = pair("ids_3_7_300_1000")
    got = instance_proximity(on_device(a * 2 ** 40), on_device(b * 2 ** 33), 2.0)
    assert got[0].tolist() == [3 * 2 ** 40, 7 * 2 ** 40, 300 * 2 ** 40, 1000 * 2 ** 40] and int(got[1][0]) == 3 * 2 ** 33
    assert_equals(got, want("ids_3_7_300_1000", 2.0))
    assert_equals(instance_proximity(on_device(a * 2 ** 40), None, 2.0), want("ids_3_7_300_1000", 2.0, UNIT, True))


def test_four_dimensions_views_and_rows():
    from skoots_amd.validate.lib import id_rows, instance_proximity
    a, b = (on_device(v) for v in pair("balls"))
    expected = want("balls", 3.0, (1.0, 1.0, 3.0))
    spacing = (1.0, 1.0, 3.0)
    assert_equals(instance_proximity(a[None], b[None], 3.0, spacing), expected)
    assert_equals(instance_proximity(a, b[None], 3.0, spacing, rows_a=id_rows(a), rows_b=id_rows(b[None])), expected)
    # non-contiguous views: a transposed buffer and every second plane of a larger one
    at = a.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    wide = torch.zeros((b.shape[0], b.shape[1], 2 * b.shape[2]), dtype=b.dtype, device=DEV)
    wide[:, :, ::2] = b
    assert not at.is_contiguous() and not wide[:, :, ::2].is_contiguous()
    assert_equals(instance_proximity(at, wide[:, :, ::2], 3.0, spacing), expected)


def test_refusals_come_before_any_launch(monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import instance_proximity
    a, b = (on_device(v) for v in pair("ids_3_7_300_1000"))
    launched = []
    real = _ffi.lib.sk_instance_proximity
    monkeypatch.setattr(_ffi.lib, "sk_instance_proximity", lambda *args: (launched.append(1), real(*args))[1])
    with pytest.raises(ValueError, match="one shape"):
        instance_proximity(a, b[:, :, :8], 2.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_proximity(a, b.cpu(), 2.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_proximity(a.cpu(), None, 2.0)
    with pytest.raises(TypeError, match="integer"):
        instance_proximity(a, b.float(), 2.0)
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="distance"):
            instance_proximity(a, b, bad)
    with pytest.raises(ValueError, match="beyond the window"):
        instance_proximity(a, b, 40.0)
    with pytest.raises(ValueError, match="beyond the window"):
        instance_proximity(a, None, 8.0, (1.0, 0.5, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        instance_proximity(a, b, 2.0, (1.0, 0.0, 1.0))
    for bad in (0, 3, -4):
        with pytest.raises(ValueError, match="power of two"):
            instance_proximity(a, b, 2.0, capacity=bad)
    assert not launched
    instance_proximity(a, b, 2.0)
    assert launched


def test_a_refusal_writes_nothing_else():
    """the C ABI on sentinel-filled buffers with a table far too small: a handled path, and what is stored is exact"""
    import ctypes as C
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    (_, (a, ids_a, lut_a, max_a)), (_, (b, ids_b, lut_b, max_b)) = (id_rows(on_device(v)) for v in pair("voxel_ids"))
    L, capacity = _ffi.lib, 64
    rows = torch.full((capacity + 8, 4), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(L.sk_instance_proximity_workspace_bytes(capacity))
    work = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=DEV)
    X, Y, Z = (int(n) for n in a.shape)
    status = L.sk_instance_proximity(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut_a), max_a, int(ids_a.numel()), _ffi.ptr(b),
                                     _ffi.ptr(lut_b), max_b, int(ids_b.numel()), 1.0, 1.0, 1.0, 4.0, 0, _ffi.ptr(rows),
                                     capacity, _ffi.ptr(counts), _ffi.ptr(work), C.c_size_t(nbytes), _ffi.stream_ptr(a.device))
    torch.cuda.synchronize()
    stored, refused = counts.tolist()
    expected = want("voxel_ids", 2.0)
    assert status == 0 and refused > 0 and 0 < stored <= capacity and stored + refused >= expected[0].shape[0]
    out = rows.cpu().numpy()
    assert (out[stored:] == -7).all() and bool((work[nbytes:] == 0x55).all())
    exact = {(r[0], r[1]): (r[2], g) for r, g in zip(expected[0].tolist(), expected[1].view(np.int64).tolist())}
    assert len({(r[0], r[1]) for r in out[:stored].tolist()}) == stored
    assert all(exact[(r[0], r[1])] == (r[2], r[3]) for r in out[:stored].tolist())


# ---- proximity(), its command, and the near columns ----

def test_proximity_joins_both_directions():
    from skoots_amd.utils.proximity import ProximityReport, proximity, sites
    from skoots_amd.validate.lib import instance_sums, plan_proximity
    a, b = pair("balls")
    spacing, distance = (1.0, 1.0, 3.0), 5.0
    ab, ba = want("balls", distance, spacing), P.ref_proximity(b, a, distance, spacing)
    ids_a, ids_b = K.rows_of(a)[1], K.rows_of(b)[1]
    xa, xb = on_device(a), on_device(b)
    pair_table, a_table, b_table, report = proximity(xa, xb, distance, spacing)
    q = ab[0][ab[0][:, 1] > 0]
    assert q.shape[0] >= 3 and q.shape[0] < ids_a.size * ids_b.size        # some pairs are within the distance, some not
    assert np.array_equal(pair_table["a_id"].cpu().numpy(), ids_a[q[:, 0] - 1])
    assert np.array_equal(pair_table["b_id"].cpu().numpy(), ids_b[q[:, 1] - 1])
    assert np.array_equal(bits(pair_table["gap"]), np.sqrt(ab[1][ab[0][:, 1] > 0]).view(np.int64))
    other = {(r[1], r[0]): (r[2], g) for r, g in zip(ba[0].tolist(), ba[1].tolist()) if r[1]}
    assert pair_table["b_near_voxels"].tolist() == [other[(r[0], r[1])][0] for r in q.tolist()]
    assert pair_table["gap"].tolist() == [float(np.sqrt(other[(r[0], r[1])][1])) for r in q.tolist()]
    assert np.array_equal(pair_table["a_near_voxels"].cpu().numpy(), q[:, 2])
    vox_a, vox_b = instance_sums(xa)[1][:, 0], instance_sums(xb)[1][:, 0]
    assert torch.equal(a_table["voxels"], vox_a) and torch.equal(b_table["voxels"], vox_b)
    assert pair_table["a_near_fraction"].tolist() == [v / vox_a[r - 1].item() for r, v in zip(q[:, 0].tolist(), q[:, 2].tolist())]
    for table, (pairs, gap2), n, m, other_ids in ((a_table, ab, ids_a.size, ids_b.size, ids_b),
                                                  (b_table, ba, ids_b.size, ids_a.size, ids_a)):
        plan = plan_proximity(pairs, gap2, n, m)
        assert np.array_equal(table["partners"].cpu().numpy(), plan["partners"])
        assert np.array_equal(table["nearest_id"].cpu().numpy(), np.concatenate(([0], other_ids))[plan["nearest_row"]])
        assert np.array_equal(bits(table["nearest_gap"]), np.sqrt(plan["nearest_gap2"]).view(np.int64))
        assert np.array_equal(table["near_voxels"].cpu().numpy(), plan["near_voxels"])
        assert table["near_fraction"].tolist() == (plan["near_voxels"] / table["voxels"].cpu().numpy()).tolist()
    assert int((a_table["partners"] == 0).sum()) > 0 and float(a_table["nearest_gap"].max()) == float("inf")
    assert report == ProximityReport(ids_a.size, ids_b.size, q.shape[0], int((a_table["partners"] > 0).sum()),
                                     int((b_table["partners"] > 0).sum()), int(a_table["near_voxels"].sum()),
                                     int(b_table["near_voxels"].sum()), float(pair_table["gap"].min()))
    # the sites volume comes from nearest_label, a kernel of its own: per id it has the union row's voxels
    volume = sites(xa, xb, distance, spacing)
    per_id = torch.bincount(volume.reshape(-1), minlength=int(ids_a[-1]) + 1)[torch.from_numpy(ids_a).to(DEV)]
    assert torch.equal(per_id, a_table["near_voxels"]) and bool(((volume == 0) | (volume == xa)).all())
    assert torch.equal(sites(xa[None], xb[None], distance, spacing), volume) and torch.equal(sites(xa, xb[None], distance, spacing), volume)
    with pytest.raises(ValueError, match="one shape"):
        sites(xa, xb[:, :, :9], distance, spacing)
    # voxel counts handed in are used as they are
    given = proximity(xa, xb, distance, spacing, voxels_a=vox_a, voxels_b=vox_b)
    assert all(torch.equal(pair_table[k], given[0][k]) for k in pair_table) and torch.equal(given[1]["voxels"], vox_a)
    with pytest.raises(ValueError, match="voxel counts"):
        proximity(xa, xb, distance, spacing, voxels_a=vox_a[:-1])
    again = proximity(xa, xb, distance, spacing)
    assert all(torch.equal(pair_table[k], again[0][k]) for k in pair_table)
    assert dataclasses.asdict(again[3]) == dataclasses.asdict(report)
    # one mask: b_table is None and the pair table holds both orders
    pt, at, bt, rep = proximity(xa, None, distance, spacing)
    assert bt is None and rep.instances_b == rep.instances_a and rep.b_near_voxels == rep.a_near_voxels
    both = set(zip(pt["a_id"].tolist(), pt["b_id"].tolist()))
    assert both == {(j, i) for i, j in both} and all(i != j for i, j in both)


def test_proximity_command_twice(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import proximity as X
    a, b = pair("balls")
    files = []
    for k in range(2):
        d = tmp_path / str(k)
        d.mkdir()
        for name, v in (("mito.tif", a), ("er.tif", b)):
            tiff.write_label_stack(str(d / name), on_device(v).permute(2, 0, 1).contiguous())
        out = X.main([str(d / "mito.tif"), str(d / "er.tif"), "--distance", "5", "--spacing", "1", "1", "3", "--save-sites"])
        assert out == (str(d / "mito_proximity.csv"), str(d / "mito_near.csv"), str(d / "er_near.csv"))
        files.append([(d / n).read_bytes().replace(str(d).encode(), b"D")
                      for n in ("mito_proximity.csv", "mito_near.csv", "er_near.csv", "mito_sites.tif")])
    assert files[0] == files[1]
    assert "a_with_partner:" in capsys.readouterr().out
    xa, xb = on_device(a), on_device(b)
    pair_table, a_table, b_table, _ = X.proximity(xa, xb, 5.0, (1.0, 1.0, 3.0))
    assert files[0][0].decode() == X.format_pairs_csv("D/mito.tif", "D/er.tif", pair_table, 5.0, (1.0, 1.0, 3.0))
    assert files[0][1].decode() == X.format_near_csv("D/mito.tif", "D/er.tif", a_table, 5.0, (1.0, 1.0, 3.0))
    assert files[0][2].decode() == X.format_near_csv("D/mito.tif", "D/er.tif", b_table, 5.0, (1.0, 1.0, 3.0))
    d = tmp_path / "0"
    back = tiff.read_stack(str(d / "mito_sites.tif"), DEV).permute(1, 2, 0)
    assert torch.equal(back.to(torch.int64), X.sites(xa, xb, 5.0, (1.0, 1.0, 3.0)))
    # one mask: two files, and --save-sites is refused
    out = X.main([str(d / "mito.tif"), "--distance", "5", "--spacing", "1", "1", "3"])
    assert out == (str(d / "mito_proximity.csv"), str(d / "mito_near.csv"))
    assert (d / "mito_near.csv").read_text().splitlines()[0] == f"A File: {d / 'mito.tif'} B File: {d / 'mito.tif'}"
    with pytest.raises(SystemExit):
        X.main([str(d / "mito.tif"), "--distance", "5", "--save-sites"])


def test_near_columns_of_stats_per_instance(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate import compare as CMP
    from skoots_amd.validate.lib import plan_proximity
    a, b = pair("balls")
    xa, xb = on_device(a), on_device(b)
    spacing, distance = (1.0, 1.0, 3.0), 5.0
    plain = CMP.stats_per_instance(xa, spacing)
    new = {"near_partners", "nearest_id", "nearest_gap", "near_voxels", "near_fraction"}
    ids_a, ids_b = K.rows_of(a)[1], K.rows_of(b)[1]
    for near, same, other_ids in ((xb, False, ids_b), ("self", True, ids_a)):
        got = CMP.stats_per_instance(xa, spacing, near=near, near_distance=distance)
        assert set(got) - set(plain) == new and list(got)[:len(plain)] == list(plain)
        # without the new arguments nothing changed: every earlier output is the same tensor, bit for bit
        assert all(torch.equal(got[k], plain[k]) for k in plain if got[k].dtype != torch.float64)
        assert all(np.array_equal(bits(got[k]), bits(plain[k])) for k in plain if got[k].dtype == torch.float64)
        plan = plan_proximity(*want("balls", distance, spacing, same), ids_a.size, other_ids.size)
        assert np.array_equal(got["near_partners"].cpu().numpy(), plan["partners"])
        assert np.array_equal(got["nearest_id"].cpu().numpy(), np.concatenate(([0], other_ids))[plan["nearest_row"]])
        assert np.array_equal(bits(got["nearest_gap"]), np.sqrt(plan["nearest_gap2"]).view(np.int64))
        assert np.array_equal(got["near_voxels"].cpu().numpy(), plan["near_voxels"])
        assert got["near_fraction"].tolist() == (plan["near_voxels"] / got["voxels"].cpu().numpy()).tolist()
    with pytest.raises(ValueError, match="together"):
        CMP.stats_per_instance(xa, spacing, near=xb)
    with pytest.raises(ValueError, match="together"):
        CMP.stats_per_instance(xa, spacing, near_distance=2.0)
    # the command: the same file as before without --near, five more columns with it
    for name, v in (("m.tif", a), ("er.tif", b)):
        tiff.write_label_stack(str(tmp_path / name), on_device(v).permute(2, 0, 1).contiguous())
    before = CMP.format_csv(str(tmp_path / "m.tif"), plain["id"], plain["sums"], plain["bbox"], a.shape, spacing)
    CMP.main([str(tmp_path / "m.tif"), "--spacing", "1", "1", "3"])
    assert (tmp_path / "m_instance_stats.csv").read_text() == before
    # ... and "as before" is a file the command wrote before it knew --near (tests/golden, other switches included)
    CMP.main([str(tmp_path / "m.tif"), "--spacing", "1", "1", "3", "--surface-area", "closed", "--contacts", "26"])
    stored = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proximity_balls_instance_stats.csv")
    with open(stored) as f:
        assert (tmp_path / "m_instance_stats.csv").read_text().replace(str(tmp_path), "D") == f.read()
    for k, column in (("id", 0), ("voxels", 1)):
        with open(stored) as f:
            assert plain[k].tolist() == [int(line.split(",")[column]) for line in f.read().splitlines()[3:]]
    got = CMP.stats_per_instance(xa, spacing, near=xb, near_distance=distance)
    CMP.main([str(tmp_path / "m.tif"), "--spacing", "1", "1", "3", "--near", str(tmp_path / "er.tif"), "--near-distance", "5"])
    lines, old = (tmp_path / "m_instance_stats.csv").read_text().splitlines(), before.splitlines()
    assert lines[:2] == old[:2] and lines[2] == old[2] + "," + CMP.NEAR_COLUMNS and len(lines) == len(old)
    cols = [got[k].tolist() for k in ("near_partners", "nearest_id", "nearest_gap", "near_voxels", "near_fraction")]
    for line, was, (n, u, g, v, f) in zip(lines[3:], old[3:], zip(*cols)):
        assert line == f"{was},{n},{u},{g!r},{v},{f!r}"
    with pytest.raises(SystemExit):
        CMP.parse_args([str(tmp_path / "m.tif"), "--near", "self"])
