"""``sk_pool_volume`` (skoots_amd/csrc/pyramid.hip) on the device against the block-by-block numpy oracle of
tests/pool_cases.py: every reduction and dtype, clipped edges, z extents around a lane's 16-byte vector and a wave, rows
that take the scalar path, a volume of many workgroups; then ``pyramid()`` and ``write_ome_zarr`` from device tensors.
Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests import pool_cases as PC

from skoots_amd.lib import zarr_store
from skoots_amd.lib.morphology import pool
from skoots_amd.utils import pyramid as PY

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(how, dtype, shape, factors, sparse):
    src = PC.to_torch(PC.source(how, dtype, shape)).to(DEV)
    got = pool(src, factors, how, sparse)
    want = PC.expected(how, dtype, shape, factors, sparse)
    assert got.dtype == src.dtype and got.device == src.device and tuple(got.shape) == want.shape
    assert np.array_equal(PC.to_numpy(got), want)


@pytest.mark.parametrize("shape", PC.SMALL_SHAPES + (PC.PLANTED_SHAPE,), ids=lambda s: "x".join(str(i) for i in s))
@pytest.mark.parametrize("factors", PC.FACTORS, ids=lambda f: "f" + "".join(str(i) for i in f))
def test_small_volumes_equal_the_oracle(shape, factors):
    """every reduction, dtype and sparse setting of one extent and factor set"""
    for how, dtype, s, f, sparse in PC.small_cases():
        if s == shape and f == factors:
            _run(how, dtype, s, f, sparse)


@pytest.mark.parametrize("factors", PC.FACTORS, ids=lambda f: "f" + "".join(str(i) for i in f))
def test_mode_cases_contain_the_blocks_they_are_for(factors):
    """from the oracle's side: ties, ties with zero among the tied values, all-distinct blocks -- otherwise the equality
    above shows nothing about the tie rules"""
    for dtype in PC.MODE_DTYPES:
        tied, zero_tied, distinct = PC.block_census(PC.mode_volume(dtype, PC.PLANTED_SHAPE), factors)
        assert tied > 0 and zero_tied > 0 and distinct > 0
        assert (PC.expected("mode", dtype, PC.PLANTED_SHAPE, factors, False) !=
                PC.expected("mode", dtype, PC.PLANTED_SHAPE, factors, True)).any()


@pytest.mark.parametrize("case", PC.BIG_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_many_workgroups(case):
    _run(*case)


def test_two_runs_are_identical_and_a_side_stream_works():
    src = PC.to_torch(PC.source("mode", "int32", PC.BIG_SHAPE)).to(DEV)
    a = pool(src, (2, 2, 2), "mode")
    b = pool(src, (2, 2, 2), "mode")
    assert torch.equal(a, b)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        c = pool(src, (2, 2, 2), "mode")
    stream.synchronize()
    assert torch.equal(a, c)
    assert np.array_equal(a.cpu().numpy(), PC.expected("mode", "int32", PC.BIG_SHAPE, (2, 2, 2), False))


def test_unaligned_views_take_the_scalar_path():
    """a volume that starts one element into its storage: rows are not dword aligned for the 8- and 16-bit dtypes"""
    for how, dtype in (("mode", "uint8"), ("mode", "int16"), ("mean", "uint16"), ("max", "uint8")):
        a = PC.source(how, dtype, (3, 4, 16))
        store = torch.zeros(a.size + 1, dtype=PC.to_torch(a).dtype, device=DEV)
        store[1:].copy_(PC.to_torch(a).to(DEV).reshape(-1))
        view = store[1:].view(3, 4, 16)
        assert view.is_contiguous() and view.data_ptr() % 4 != 0
        got = pool(view, (2, 2, 2), how)
        assert np.array_equal(PC.to_numpy(got), PC.expected(how, dtype, (3, 4, 16), (2, 2, 2)))


def test_library_refuses_by_name():
    from skoots_amd import _ffi
    v = torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV)
    out = torch.zeros((2, 2, 2), dtype=torch.int32, device=DEV)
    st = _ffi.stream_ptr(v.device)
    for args, word in (((3, 4, 4, 4, 2, 2, 3, 0, 0), "factors"), ((3, 4, 4, 4, 1, 1, 1, 0, 0), "factors"),
                       ((3, 4, 4, 4, 2, 2, 2, 1, 0), "dtype"), ((1, 4, 4, 4, 2, 2, 2, 0, 0), "dtype"),
                       ((3, 4, 0, 4, 2, 2, 2, 0, 0), "extents"), ((3, 4, 4, 4, 2, 2, 2, 3, 0), "how")):
        with pytest.raises(ValueError, match="sk_pool_volume.*" + word):
            _ffi.check(_ffi.lib.sk_pool_volume(_ffi.ptr(v), *args, _ffi.ptr(out), st))
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


SHAPE, SPACING = (40, 36, 24), (1.0, 1.0, 3.0)


def _oracle_levels(how, dtype, plan, sparse=False):
    levels = [PC.source(how, dtype, SHAPE)]
    for lv in plan[1:]:
        levels.append(PC.oracle_pool(levels[-1], lv.factors, how, sparse))
    return levels


def test_three_level_pyramid():
    mask = PC.to_torch(PC.source("mode", "int32", SHAPE)).to(DEV)
    tensors, plan = PY.pyramid(mask, SPACING, "mode", levels=3)
    assert [lv.factors for lv in plan] == [(1, 1, 1), (2, 2, 1), (2, 2, 2)]
    assert tensors[0].data_ptr() == mask.data_ptr()
    for t, want in zip(tensors, _oracle_levels("mode", "int32", plan)):
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)


@pytest.mark.parametrize("huffman", ("fixed", "dynamic"))
def test_write_ome_zarr_from_device_tensors(tmp_path, huffman):
    image = PC.to_torch(PC.source("mean", "uint16", SHAPE)).to(DEV)
    mask = PC.to_torch(PC.source("mode", "int32", SHAPE)).to(DEV)
    skel = PC.to_torch(PC.source("max", "uint8", SHAPE)).to(DEV)
    path = str(tmp_path / "vol.ome.zarr")
    timings = {}
    report = PY.write_ome_zarr(path, SPACING, image=image, labels={"instances": mask, "skeleton": (skel, "max")},
                               huffman=huffman, levels=3, timings=timings)
    assert timings["pool_s"] > 0 and timings["kernel_s"] > 0 and report["bytes_written"] > 0
    plan = report["plan"]
    for group, how, dtype in ((path, "mean", "uint16"), (os.path.join(path, "labels", "instances"), "mode", "int32"),
                              (os.path.join(path, "labels", "skeleton"), "max", "uint8")):
        pairs = PY.read_multiscales(group)
        assert [s for _, s in pairs] == [[3.0, 1.0, 1.0], [3.0, 2.0, 2.0], [6.0, 4.0, 4.0]]
        for (array_path, _), level in zip(pairs, _oracle_levels(how, dtype, plan)):
            assert np.array_equal(zarr_store.load(array_path), level.transpose(2, 0, 1))
    back = zarr_store.load_device(os.path.join(path, "labels", "instances", "1"), DEV)
    assert np.array_equal(back.cpu().numpy(), _oracle_levels("mode", "int32", plan)[1].transpose(2, 0, 1))
