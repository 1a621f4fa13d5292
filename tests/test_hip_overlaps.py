"""``sk_instance_overlaps`` (skoots_amd/csrc/overlaps.hip) and what stands on it -- ``validate.lib.instance_overlaps``,
``sparse_mask_iou``, ``compare(sparse=True)``, ``utils.relate.relate`` and its command, the parent columns of
``stats_per_instance`` -- against the numpy restatement of tests/overlap_cases.py.  Everything is an integer or an fp32 /
fp64 bit pattern: every comparison is exact, row for row.

The kernel reads the volumes as one line in chunks of 4096 voxels, 16 bytes per lane and load, with a scalar head and
tail; a chunk's LDS table holds 256 pairs.  ``many_ids`` (31 350 voxels) is several chunks and no multiple of one, and
it and ``voxel_ids`` give a chunk more pairs than the table holds, so the direct path to the global table runs."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import contact_cases as K
from tests import overlap_cases as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def pair(name):
    a, b = (np.ascontiguousarray(v).astype(np.int64) for v in O.PAIRS[name]())
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def want_overlaps(name, background):
    t = O.ref_overlaps(*pair(name), background)
    t.setflags(write=False)
    return t


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached volumes are read-only


def check_overlaps(name, background, dtype=None, **kw):
    from skoots_amd.validate.lib import instance_overlaps
    a, b = pair(name)
    xa, xb = on_device(a, dtype), on_device(b, dtype)
    ids_a, ids_b, table = instance_overlaps(xa, xb, background, **kw)
    assert ids_a.dtype == ids_b.dtype == table.dtype == torch.int64 and table.is_cuda and table.ndim == 2
    assert np.array_equal(ids_a.cpu().numpy(), K.rows_of(a)[1]) and np.array_equal(ids_b.cpu().numpy(), K.rows_of(b)[1])
    assert np.array_equal(table.cpu().numpy(), want_overlaps(name, background))
    again = instance_overlaps(xa, xb, background, **kw)[2]
    assert torch.equal(table, again)
    return table


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("name", sorted(set(O.PAIRS) - {"voxel_ids"}))
def test_table_equals_the_definition(name, background):
    check_overlaps(name, background)


@pytest.mark.parametrize("background", [False, True])
def test_more_pairs_than_the_chunk_table_holds(background):
    table = check_overlaps("voxel_ids", background)
    assert table.shape[0] >= pair("voxel_ids")[0].size > O.LDS_SLOTS
    chunks = -(-pair("many_ids")[0].size // O.CHUNK)
    assert want_overlaps("many_ids", background).shape[0] > 2 * O.LDS_SLOTS * chunks


@pytest.mark.parametrize("background", [False, True])
def test_int64_masks(background):
    check_overlaps("ids_3_7_300_1000", background, dtype=torch.int64)
    from skoots_amd.validate.lib import instance_overlaps
    a, b = pair("below_one_chunk")
    ids_a, ids_b, table = instance_overlaps(on_device(a * 2 ** 40), on_device(b * 2 ** 33), background)
    assert ids_a.cpu().tolist() == [2 ** 40, 2 ** 41, 3 * 2 ** 40] and ids_b.cpu().tolist() == [2 ** 33, 2 ** 34, 3 * 2 ** 33]
    assert np.array_equal(table.cpu().numpy(), want_overlaps("below_one_chunk", background))
    # one side relabelled, the other through its table
    table = instance_overlaps(on_device(a * 2 ** 40), on_device(b), background)[2]
    assert np.array_equal(table.cpu().numpy(), want_overlaps("below_one_chunk", background))


def test_rows_arguments_and_four_dimensions():
    from skoots_amd.validate.lib import id_rows, instance_overlaps
    a, b = (on_device(v) for v in pair("ids_3_7_300_1000"))
    want = instance_overlaps(a, b, True)[2]
    got = instance_overlaps(a[None], b[None], True, rows_a=id_rows(a[None]), rows_b=id_rows(b))[2]
    assert torch.equal(got, want) and torch.equal(instance_overlaps(a[None], b, True)[2], want)


@pytest.mark.parametrize("offsets", [(1, 1), (3, 3), (1, 0), (2, 3)])
@pytest.mark.parametrize("name", ["many_ids", "line_z", "one_voxel"])
def test_views_that_are_only_4_byte_aligned(name, offsets):
    """the volumes start `offsets` elements into their buffers: the same misalignment on both sides is a scalar head and
    16-byte loads, a different one on each side is read voxel by voxel"""
    from skoots_amd.validate.lib import instance_overlaps
    a, b = pair(name)
    views = []
    for v, off in zip((a, b), offsets):
        buf = torch.full((v.size + off + 5,), 77, dtype=torch.int32, device=DEV)        # 77: an id outside the view
        buf[off:off + v.size] = on_device(v).reshape(-1)
        views.append(buf[off:off + v.size].view(v.shape))
        assert views[-1].is_contiguous() and views[-1].data_ptr() % 16 == 4 * off % 16
    for background in (False, True):
        table = instance_overlaps(*views, background)[2]
        assert np.array_equal(table.cpu().numpy(), want_overlaps(name, background))


def test_shape_device_and_dtype_errors():
    from skoots_amd.validate.lib import instance_overlaps
    a, b = (on_device(v) for v in pair("below_one_chunk"))
    with pytest.raises(ValueError, match="one shape"):
        instance_overlaps(a, b[:, :, :39])
    with pytest.raises(ValueError, match="no CPU fallback"):
        instance_overlaps(a, b.cpu())
    with pytest.raises(TypeError, match="integer"):
        instance_overlaps(a, b.float())
    for bad in (0, 3, -4):
        with pytest.raises(ValueError, match="power of two"):
            instance_overlaps(a, b, capacity=bad)


# ---- capacity and the retry ----

@pytest.mark.parametrize("capacity", [1, 2])
def test_a_small_capacity_is_retried(capacity, monkeypatch):
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import instance_overlaps
    calls = []
    real = _ffi.lib.sk_instance_overlaps
    monkeypatch.setattr(_ffi.lib, "sk_instance_overlaps", lambda *args: (calls.append(int(args[13])), real(*args))[1])
    a, b = (on_device(v) for v in pair("many_ids"))
    table = instance_overlaps(a, b, True, capacity=capacity)[2]
    assert np.array_equal(table.cpu().numpy(), want_overlaps("many_ids", True))
    assert len(calls) > 1 and calls[0] == capacity and calls == sorted(set(calls))
    assert calls[-1] >= want_overlaps("many_ids", True).shape[0]


def test_the_retry_stops_at_the_largest_table(monkeypatch):
    from skoots_amd.validate import lib
    monkeypatch.setattr(lib, "MAX_OVERLAP_CAPACITY", 4)
    a, b = (on_device(v) for v in pair("many_ids"))
    with pytest.raises(RuntimeError, match="more than 4"):
        lib.instance_overlaps(a, b, capacity=1)
    with pytest.raises(RuntimeError, match="more than 4"):
        lib.instance_overlaps(a, b)


def raw_call(name, background, capacity, guard=8):
    """sk_instance_overlaps through the C ABI on sentinel-filled buffers: (status, rows with the guard tail, counts)"""
    from skoots_amd import _ffi
    from skoots_amd.validate.lib import id_rows
    (_, (a, ids_a, lut_a, max_a)), (_, (b, ids_b, lut_b, max_b)) = (id_rows(on_device(v)) for v in pair(name))
    L = _ffi.lib
    rows = torch.full((capacity + guard, 3), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(L.sk_instance_overlaps_workspace_bytes(capacity))
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    X, Y, Z = (int(n) for n in a.shape)
    status = L.sk_instance_overlaps(_ffi.ptr(a), X, Y, Z, _ffi.ptr(lut_a), max_a, int(ids_a.numel()), _ffi.ptr(b),
                                    _ffi.ptr(lut_b), max_b, int(ids_b.numel()), int(background), _ffi.ptr(rows), capacity,
                                    _ffi.ptr(counts), _ffi.ptr(work), C.c_size_t(nbytes), _ffi.stream_ptr(a.device))
    torch.cuda.synchronize()
    return status, rows.cpu().numpy(), counts.cpu().tolist()


def test_a_refusal_writes_nothing_else():
    status, rows, (stored, refused) = raw_call("voxel_ids", False, 64)
    want = want_overlaps("voxel_ids", False)
    assert status == 0 and refused > 0 and 0 < stored <= 64          # a handled path, not a fault
    assert stored + refused >= want.shape[0]
    assert (rows[stored:] == -7).all()                               # nothing behind the rows, nothing in the guard
    # what was stored is exact: a key is stored for the whole launch or not at all
    exact = {tuple(r[:2]): r[2] for r in want.tolist()}
    assert len({tuple(r[:2]) for r in rows[:stored].tolist()}) == stored
    assert all(exact[tuple(r[:2])] == r[2] for r in rows[:stored].tolist())


@pytest.mark.parametrize("background", [False, True])
def test_buffers_beyond_the_rows_stay_untouched(background):
    want = want_overlaps("ids_3_7_300_1000", background)
    status, rows, (stored, refused) = raw_call("ids_3_7_300_1000", background, 32)
    assert status == 0 and refused == 0 and stored == want.shape[0] and (rows[stored:] == -7).all()
    t = rows[:stored]
    assert np.array_equal(t[np.lexsort((t[:, 1], t[:, 0]))], want)


def test_c_abi_guards():
    from skoots_amd import _ffi
    L = _ffi.lib
    assert L.sk_abi_version() >= 28 and L.sk_instance_overlaps_row_values() == 3
    assert L.sk_instance_overlaps_workspace_bytes(0) == 0 and L.sk_instance_overlaps_workspace_bytes(-8) == 0
    assert L.sk_instance_overlaps_workspace_bytes(16) >= 16 * 2 * 8
    a = torch.tensor([1, 2], dtype=torch.int32, device=DEV).repeat(4, 4, 2)          # (4, 4, 4): z alternates 1, 2
    b = torch.ones((4, 4, 4), dtype=torch.int32, device=DEV)
    lut = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    rows = torch.full((16 + 4, 3), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(L.sk_instance_overlaps_workspace_bytes(16))
    work = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=DEV)
    s = _ffi.stream_ptr(a.device)
    P = _ffi.ptr

    def call(X=4, Y=4, Z=4, N=2, max_a=2, M=1, max_b=1, background=0, capacity=16, ws=nbytes, la=P(a), ta=P(lut), lb=P(b),
             tb=P(lut), out=P(rows), cnt=P(counts), wsp=P(work)):
        return L.sk_instance_overlaps(la, X, Y, Z, ta, max_a, N, lb, tb, max_b, M, background, out, capacity, cnt, wsp,
                                      C.c_size_t(ws), s)

    assert call(X=-1) == -1 and "negative" in _ffi.last_error()
    assert call(Y=-1) == -1 and call(Z=-1) == -1 and call(N=-1) == -1 and call(max_a=-1) == -1
    assert call(M=-1) == -1 and "negative" in _ffi.last_error() and call(max_b=-1) == -1
    assert call(background=2) == -1 and "background" in _ffi.last_error() and call(background=-1) == -1
    assert call(capacity=0) == -1 and "power of two" in _ffi.last_error()
    assert call(capacity=12) == -1 and call(capacity=-16) == -1
    assert call(ws=nbytes - 1) == -1 and "workspace" in _ffi.last_error()
    assert call(capacity=32) == -1                                   # the workspace is that of 16
    for name in ("la", "ta", "lb", "tb", "out", "cnt", "wsp"):
        assert call(**{name: None}) == -1 and "NULL" in _ffi.last_error(), name
    assert call(la=C.c_void_p(a.data_ptr() + 2)) == -1 and "aligned" in _ffi.last_error()
    assert call(tb=C.c_void_p(lut.data_ptr() + 1)) == -1 and call(out=C.c_void_p(rows.data_ptr() + 4)) == -1
    assert call(cnt=C.c_void_p(counts.data_ptr() + 4)) == -1 and call(wsp=C.c_void_p(work.data_ptr() + 4)) == -1
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((counts == -7).all()) and bool((work == 0x55).all())
    # the empty calls: counts = {0, 0}, nothing else, no mask pointer is looked at
    nothing = dict(la=None, ta=None, lb=None, tb=None)
    for empty in (dict(Z=0), dict(N=0, M=0), dict(N=0, M=0, background=1), dict(N=0), dict(M=0)):
        counts.fill_(-7)
        assert call(**empty, **nothing) == 0, empty
        torch.cuda.synchronize()
        assert counts.tolist() == [0, 0] and bool((rows == -7).all()), empty
    # a side without instances is background and is not looked at; the other one is
    counts.fill_(-7)
    assert call(M=0, background=1, lb=None, tb=None) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [2, 0] and sorted(rows[:2].tolist()) == [[1, 0, 32], [2, 0, 32]] and bool((rows[2:] == -7).all())
    assert call(M=0, background=1, la=None) == -1 and "NULL" in _ffi.last_error()
    rows.fill_(-7)
    assert call() == 0                                               # and the same arguments unbroken do run
    torch.cuda.synchronize()
    assert counts.tolist() == [2, 0] and sorted(rows[:2].tolist()) == [[1, 1, 32], [2, 1, 32]] and bool((rows[2:] == -7).all())
    assert bool((work[nbytes:] == 0x55).all())


# ---- scale: what the dense path cannot hold ----

def test_sixty_four_thousand_instances_a_side():
    """64 000 x 64 000 instances: the dense table alone would be 16 GB.  256 MiB is a condition, not a measurement: the
    inputs and the pair table are a few MB."""
    from skoots_amd.validate.lib import instance_overlaps, sparse_mask_iou
    a, b = O.voxel_ids_pair((40, 40, 40))
    want = O.ref_overlaps(a, b, True)
    assert want.shape[0] == 64000
    xa, xb = on_device(a), on_device(b)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids_a, ids_b, table = instance_overlaps(xa, xb, True)
    iou = sparse_mask_iou(xa, xb)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 256 << 20
    assert ids_a.numel() == ids_b.numel() == 64000 and np.array_equal(table.cpu().numpy(), want)
    assert iou.shape == (64000, 64000) and iou.is_coalesced() and iou._nnz() == 64000
    assert np.array_equal(iou.indices().cpu().numpy(), want[:, :2].T - 1)
    assert bool((iou.values() == 1.0).all())                       # every voxel of a is one voxel of b


# ---- sparse_mask_iou ----

def bits(t, kind):
    return torch.as_tensor(t).cpu().contiguous().numpy().view(kind)


@pytest.mark.parametrize("name", ["zero_a", "zero_b", "zero_both", "id_int32_max"])
def test_sparse_mask_iou_of_empty_sides_and_huge_ids(name):
    """what ``mask_iou`` is not asked for: a side without instances, and an id that would make its table 8 GB"""
    from skoots_amd.validate.lib import sparse_mask_iou
    a, b = pair(name)
    sparse = sparse_mask_iou(on_device(a), on_device(b))
    want = O.dense_iou(a, b)
    assert sparse.is_sparse and sparse.is_coalesced() and sparse.dtype == torch.float32 and sparse.is_cuda
    assert tuple(sparse.shape) == want.shape and sparse._nnz() == int((want > 0).sum())
    assert np.array_equal(bits(sparse.to_dense(), np.uint32).reshape(want.shape), want.view(np.uint32))


@pytest.mark.parametrize("name", ["many_ids", "balls", "tie", "ids_3_7_300_1000", "shared_and_unmatched"])
def test_sparse_mask_iou_is_mask_iou(name):
    from skoots_amd.validate.lib import mask_iou, sparse_mask_iou
    a, b = (on_device(v) for v in pair(name))
    dense = mask_iou(a, b)
    sparse = sparse_mask_iou(a, b)
    assert sparse.is_sparse and sparse.is_coalesced() and sparse.dtype == torch.float32 and sparse.is_cuda
    assert tuple(sparse.shape) == tuple(dense.shape)
    assert np.array_equal(bits(sparse.to_dense(), np.uint32), bits(dense, np.uint32))
    assert sparse._nnz() == want_overlaps(name, False).shape[0] == int((dense > 0).sum())
    assert np.array_equal(bits(dense, np.uint32), O.dense_iou(*pair(name)).view(np.uint32))


# ---- compare(sparse=True) ----

@pytest.mark.parametrize("threshold", [0.1, 0.6])
@pytest.mark.parametrize("name", ["many_ids", "tie", "shared_and_unmatched", "zero_a", "zero_b"])
def test_sparse_compare_is_compare(name, threshold):
    from skoots_amd.validate import compare as CMP
    g, p = (on_device(v) for v in pair(name))
    spacing = (1.0, 0.5, 2.0)
    dense = CMP.compare(g, p, spacing, threshold)
    sparse = CMP.compare(g, p, spacing, threshold, sparse=True)
    assert list(dense) == list(sparse)
    for k in dense:
        assert dense[k].dtype == sparse[k].dtype and dense[k].device == sparse[k].device, k
        if dense[k].dtype == torch.float64:
            assert np.array_equal(bits(dense[k], np.uint64), bits(sparse[k], np.uint64)), k
        else:
            assert not dense[k].is_floating_point() and torch.equal(dense[k], sparse[k]), k
    texts = [CMP.format_compare_csv("p.tif", "g.tif", r, spacing, threshold) for r in (dense, sparse)]
    assert texts[0] == texts[1]
    if name == "tie":
        assert dense["pred_id"].tolist() == ([1] if threshold < 0.4 else [0])
    if name == "shared_and_unmatched" and threshold == 0.1:
        assert dense["pred_id"].tolist() == [5, 5, 8, 0] and dense["pred_shared"].tolist() == [2, 2, 1, 0]
        assert dense["unmatched_pred_id"].tolist() == [7, 9] and dense["unmatched_pred_best_iou"][1] == 0
        assert dense["unmatched_pred_best_iou"][0] > 0


def test_sparse_compare_command(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.validate import compare as CMP
    g, p = pair("shared_and_unmatched")
    texts = []
    for k, extra in enumerate(([], ["--sparse-matching"])):
        d = tmp_path / str(k)
        d.mkdir()
        for name, v in (("g.tif", g), ("p.tif", p)):
            tiff.write_label_stack(str(d / name), on_device(v).permute(2, 0, 1).contiguous())
        CMP.main([str(d / "p.tif"), "--ground-truth", str(d / "g.tif"), *extra])
        texts.append((d / "p_compare.csv").read_text().replace(str(d), "D"))
    assert texts[0] == texts[1] and texts[0].count("\n") == 3 + 4 + 2


# ---- relate ----

RELATE_CASES = ["ids_3_7_300_1000", "balls", "many_ids", "zero_a", "zero_b", "id_int32_max"]


@pytest.mark.parametrize("min_fraction", [0.0, 0.3])
@pytest.mark.parametrize("name", RELATE_CASES)
def test_relate_equals_the_plan_of_the_oracle_table(name, min_fraction):
    from skoots_amd.utils.relate import RelateReport, plan_relate, relate
    from skoots_amd.validate.lib import instance_sums
    a, b = pair(name)
    spacing = (1.0, 0.5, 2.0)
    ids_a, ids_b = K.rows_of(a)[1], K.rows_of(b)[1]
    want_c, want_p = plan_relate(want_overlaps(name, True), ids_a.size, ids_b.size, min_fraction)
    xa, xb = on_device(a), on_device(b)
    child, parent, report = relate(xa, xb, min_fraction, spacing, relabel=True)
    assert all(v.is_cuda for v in child.values()) and all(v.is_cuda for v in parent.values())
    assert np.array_equal(child["id"].cpu().numpy(), ids_a) and np.array_equal(parent["id"].cpu().numpy(), ids_b)
    parent_id = np.concatenate(([0], ids_b))[want_c["parent_row"]]
    assert np.array_equal(child["parent_id"].cpu().numpy(), parent_id)
    for k in ("voxels", "inside_voxels", "parents_touched", "outside_voxels"):
        assert child[k].dtype == torch.int64 and np.array_equal(child[k].cpu().numpy(), want_c[k]), k
    assert np.array_equal(bits(child["inside_fraction"], np.uint64), want_c["inside_fraction"].view(np.uint64))
    for k in ("voxels", "children", "children_voxels", "occupied_voxels"):
        assert parent[k].dtype == torch.int64 and np.array_equal(parent[k].cpu().numpy(), want_p[k]), k
    assert np.array_equal(bits(parent["occupancy"], np.uint64), want_p["occupancy"].view(np.uint64))
    assert parent["children_volume"].cpu().tolist() == [float(v) * (1.0 * 0.5 * 2.0) for v in want_p["children_voxels"]]
    # against the measurements that exist
    assert torch.equal(child["voxels"], instance_sums(xa)[1][:, 0]) and torch.equal(parent["voxels"], instance_sums(xb)[1][:, 0])
    # the relabelled volume against numpy
    want_volume = np.concatenate(([0], parent_id))[K.rows_of(a)[0]]
    assert child["by_parent"].dtype == torch.int32 and np.array_equal(child["by_parent"].cpu().numpy(), want_volume)
    assigned = int((want_c["parent_row"] > 0).sum())
    assert report == RelateReport(ids_a.size, ids_b.size, assigned, ids_a.size - assigned,
                                  int((want_c["parents_touched"] > 1).sum()), int((want_p["children"] == 0).sum()),
                                  int((a > 0).sum()), int(want_c["inside_voxels"].sum()), int(((a > 0) & (b == 0)).sum()))
    again = relate(xa, xb, min_fraction, spacing, relabel=True)
    assert all(torch.equal(child[k], again[0][k]) for k in child) and dataclasses.asdict(again[2]) == dataclasses.asdict(report)
    assert "by_parent" not in relate(xa, xb, min_fraction, spacing)[0]


def test_relate_argument_errors():
    from skoots_amd.utils.relate import relate
    a, b = (on_device(v) for v in pair("below_one_chunk"))
    with pytest.raises(ValueError, match="min_fraction"):
        relate(a, b, 1.5)
    with pytest.raises(ValueError, match="spacing"):
        relate(a, b, 0.0, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="one shape"):
        relate(a, b[:2])
    with pytest.raises(ValueError, match="negative"):
        relate(a - 1, b, relabel=True)
    with pytest.raises(ValueError, match="beyond int32"):
        relate(a, b.long() * 2 ** 40, relabel=True)
    assert relate(a, b.long() * 2 ** 40)[0]["parent_id"].max() >= 2 ** 40


def test_relate_command_twice(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import relate as R
    a, b = pair("balls")
    files = []
    for k in range(2):
        d = tmp_path / str(k)
        d.mkdir()
        for name, v in (("mito.tif", a), ("cells.tif", b)):
            tiff.write_label_stack(str(d / name), on_device(v).permute(2, 0, 1).contiguous())
        out = R.main([str(d / "mito.tif"), str(d / "cells.tif"), "--min-fraction", "0.25", "--spacing", "1", "0.5", "2",
                      "--save-relabelled"])
        assert out == (str(d / "mito_parents.csv"), str(d / "cells_children.csv"))
        files.append([(d / n).read_bytes().replace(str(d).encode(), b"D")
                      for n in ("mito_parents.csv", "cells_children.csv", "mito_by_parent.tif")])
    assert files[0] == files[1]
    assert "children_assigned:" in capsys.readouterr().out
    child, parent, _ = R.relate(on_device(a), on_device(b), 0.25, (1.0, 0.5, 2.0), relabel=True)
    d = tmp_path / "0"
    assert files[0][0].decode() == R.format_parents_csv("D/mito.tif", "D/cells.tif", child, (1.0, 0.5, 2.0), 0.25)
    assert files[0][1].decode() == R.format_children_csv("D/mito.tif", "D/cells.tif", parent, (1.0, 0.5, 2.0), 0.25)
    back = tiff.read_stack(str(d / "mito_by_parent.tif"), DEV).permute(1, 2, 0)
    assert torch.equal(back.to(torch.int32), child["by_parent"])
    # -o writes the volume over the children file
    R.main([str(d / "mito.tif"), str(d / "cells.tif"), "--min-fraction", "0.25", "--save-relabelled", "-o"])
    assert torch.equal(tiff.read_stack(str(d / "mito.tif"), DEV).permute(1, 2, 0).to(torch.int32), child["by_parent"])


# ---- stats_per_instance(parents=...) ----

def test_parent_columns_of_stats_per_instance(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.utils.relate import relate
    from skoots_amd.validate import compare as CMP
    a, b = pair("balls")
    xa, xb = on_device(a), on_device(b)
    spacing = (1.0, 0.5, 2.0)
    plain = CMP.stats_per_instance(xa, spacing)
    got = CMP.stats_per_instance(xa, spacing, parents=xb, parent_min_fraction=0.3)
    assert set(got) - set(plain) == {"parent", "inside_fraction"} and list(got)[:len(plain)] == list(plain)
    assert all(torch.equal(got[k], plain[k]) for k in plain if got[k].dtype != torch.float64)
    assert all(np.array_equal(bits(got[k], np.uint64), bits(plain[k], np.uint64)) for k in plain
               if got[k].dtype == torch.float64)
    child = relate(xa, xb, 0.3)[0]
    assert torch.equal(got["parent"], child["parent_id"]) and got["parent"].dtype == torch.int64
    assert np.array_equal(bits(got["inside_fraction"], np.uint64), bits(child["inside_fraction"], np.uint64))
    assert 0 < int((got["parent"] > 0).sum()) and int((child["parent_id"] == 0).sum()) > 0
    # the command: the same file as before without --parents, two more columns with it
    for name, v in (("m.tif", a), ("cells.tif", b)):
        tiff.write_label_stack(str(tmp_path / name), on_device(v).permute(2, 0, 1).contiguous())
    before = CMP.format_csv(str(tmp_path / "m.tif"), plain["id"], plain["sums"], plain["bbox"], a.shape, spacing)
    CMP.main([str(tmp_path / "m.tif"), "--spacing", "1", "0.5", "2"])
    assert (tmp_path / "m_instance_stats.csv").read_text() == before
    CMP.main([str(tmp_path / "m.tif"), "--spacing", "1", "0.5", "2", "--parents", str(tmp_path / "cells.tif"),
              "--parent-min-fraction", "0.3"])
    lines, old = (tmp_path / "m_instance_stats.csv").read_text().splitlines(), before.splitlines()
    assert lines[:2] == old[:2] and lines[2] == old[2] + ",parent,inside_fraction" and len(lines) == len(old)
    for line, was, u, f in zip(lines[3:], old[3:], got["parent"].tolist(), got["inside_fraction"].tolist()):
        assert line == f"{was},{u},{f!r}"
