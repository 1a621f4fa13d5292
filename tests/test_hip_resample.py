"""``sk_resample_volume`` (skoots_amd/csrc/resample.hip) on the device against the integer oracle of
tests/resample_cases.py: z extents around a lane's 16-byte unit and around a wave at seven ratios, extents of 1 at both
ends of the ratio limit, mixed operators, every dtype per operator, rows that take the scalar path, a volume of many
workgroups and its way back, both accumulator widths, and the C ABI on sentinel-filled buffers.  Every comparison is
exact."""
import numpy as np
import pytest
import torch

from tests import resample_cases as RC

from skoots_amd import _ffi
from skoots_amd.lib import morphology as M
from skoots_amd.lib.morphology import resample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(how, dtype, shape, out_shape):
    src = RC.to_torch(RC.source(how, dtype, shape)).to(DEV)
    got = resample(src, shape=out_shape, how=how)
    want = RC.expected(how, dtype, tuple(shape), tuple(out_shape))
    assert got.dtype == src.dtype and got.device == src.device and tuple(got.shape) == want.shape
    assert np.array_equal(RC.to_numpy(got), want), (how, dtype, shape, out_shape)


@pytest.mark.parametrize("z", RC.Z_EXTENTS)
def test_z_around_a_lane_and_a_wave(z):
    """source (3, 4, z) to every z target: the same, 2x, 3/2, 1/2, 2/3, 8x, 1/8"""
    cases = [c for c in RC.z_cases() if c[2][2] == z]
    assert {c[3][2] for c in cases} == set(RC.z_targets(z)) and len(RC.z_targets(z)) == 7
    for case in cases:
        _run(*case)


def test_extents_of_one_at_both_ends_of_the_ratio_limit():
    for case in RC.UNIT_CASES:
        _run(*case)


def test_mixed_operators_under_auto():
    assert RC.operators((6, 9, 40), (9, 6, 60), "auto") == ("linear", "area", "linear")
    assert RC.operators((6, 9, 40), (3, 18, 13), "auto") == ("area", "linear", "area")
    for case in RC.MIXED_CASES:
        _run(*case)


@pytest.mark.parametrize("case", RC.DTYPE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_every_dtype_per_operator(case):
    _run(*case)


def test_rows_that_are_no_dword_multiple():
    for case in RC.ODD_ROW_CASES:
        assert (case[2][2] * np.dtype(case[1]).itemsize) % 4 or (case[3][2] * np.dtype(case[1]).itemsize) % 4
        _run(*case)


def test_non_contiguous_and_unaligned_inputs():
    how, dtype, shape, out_shape = "auto", "uint8", (5, 7, 24), (7, 5, 36)
    a = RC.source(how, dtype, shape)
    want = RC.expected(how, dtype, shape, out_shape)
    t = RC.to_torch(np.ascontiguousarray(a.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)     # (X, Y, Z) with Z outermost
    assert not t.is_contiguous()
    assert np.array_equal(RC.to_numpy(resample(t, shape=out_shape, how=how)), want)
    # a volume that starts one element into its storage: rows are not dword aligned
    store = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    store[1:].copy_(RC.to_torch(a).to(DEV).reshape(-1))
    view = store[1:].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 4 != 0
    assert np.array_equal(RC.to_numpy(resample(view, shape=out_shape, how=how)), want)
    lead = RC.to_torch(a).to(DEV).unsqueeze(0)
    got = resample(lead, factors=(1.4, 0.7, 1.5), how=how)                                    # the leading 1 is kept
    assert tuple(got.shape) == (1,) + out_shape and np.array_equal(RC.to_numpy(got[0]), want)


@pytest.mark.parametrize("case", RC.BIG_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_many_workgroups(case):
    _run(*case)


def test_many_workgroups_and_back_with_nearest():
    """(70, 66, 300) -> (105, 44, 450) -> (70, 66, 300) on int32 labels, each way equal to the oracle; two runs and a
    side stream give the same bits"""
    src = RC.to_torch(RC.source("nearest", "int32", RC.BIG_SHAPE)).to(DEV)
    there = resample(src, shape=RC.BIG_OUT, how="nearest")
    back = resample(there, shape=RC.BIG_SHAPE, how="nearest")
    want_there = RC.expected("nearest", "int32", RC.BIG_SHAPE, RC.BIG_OUT)
    assert np.array_equal(there.cpu().numpy(), want_there)
    assert np.array_equal(back.cpu().numpy(), RC.oracle_resample(want_there, RC.BIG_SHAPE, "nearest"))
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        again = resample(src, shape=RC.BIG_OUT, how="nearest")
    stream.synchronize()
    assert torch.equal(there, again)


def test_up_by_integer_factors_and_back_is_the_identity():
    for dtype in RC.LABEL_DTYPES:
        src = RC.to_torch(RC.source("nearest", dtype, (5, 7, 24))).to(DEV)
        up = resample(src, factors=(2, 3, 4), how="nearest")
        assert tuple(up.shape) == (10, 21, 96)
        assert torch.equal(resample(up, shape=(5, 7, 24), how="nearest"), src)


@pytest.mark.parametrize("case", RC.ACC_CASES, ids=lambda c: f"{c[1]}-{c[4]}")
def test_both_accumulator_widths(case):
    how, dtype, shape, out_shape, path = case
    ops = RC.operators(shape, out_shape, how)
    product = RC.reduced_total(shape, out_shape, ops) * int(np.iinfo(dtype).max)
    assert (product < 2 ** 32) == (path == "acc32") and 0.99 < product / 2 ** 32 < 1.07     # just below, just above
    assert M.resample_path(getattr(torch, dtype), shape, out_shape, ops) == path
    _run(how, dtype, shape, out_shape)


def _abi_call(src, dst, code, n, m, ops, workspace, nbytes):
    return _ffi.lib.sk_resample_volume(_ffi.ptr(src), _ffi.ptr(dst), code, *n, *m, *ops, _ffi.ptr(workspace), nbytes,
                                       _ffi.stream_ptr(torch.device(DEV)))


def test_c_abi_writes_nothing_outside_dst_and_refuses_by_name():
    how, dtype, shape, out_shape = "auto", "uint8", (5, 7, 24), (7, 5, 37)
    a = RC.source(how, dtype, shape)
    ops = tuple(M.RESAMPLE_OP[o] for o in RC.operators(shape, out_shape, how))
    n_out, pad = int(np.prod(out_shape)), 256
    nbytes = int(_ffi.lib.sk_resample_workspace_bytes(4, *shape, *out_shape, *ops))
    assert nbytes > 0
    src = RC.to_torch(a).to(DEV)
    store = torch.full((pad + n_out + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_store = torch.full((pad + nbytes + pad,), 0x5A, dtype=torch.uint8, device=DEV)
    dst, ws = store[pad:pad + n_out], ws_store[pad:pad + nbytes]
    _ffi.check(_abi_call(src, dst, 4, shape, out_shape, ops, ws, nbytes))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(out_shape), RC.expected(how, dtype, shape, out_shape))
    assert bool((store[:pad] == 0xA5).all()) and bool((store[pad + n_out:] == 0xA5).all())
    assert bool((ws_store[:pad] == 0x5A).all()) and bool((ws_store[pad + nbytes:] == 0x5A).all())

    # every bad argument: SK_ERR_ARG with a message, nothing launched
    store.fill_(0xA5)
    ws_store.fill_(0x5A)
    torch.cuda.synchronize()
    lab = torch.zeros(shape, dtype=torch.int32, device=DEV)
    bad = ((src, dst, 4, (5, 0, 24), out_shape, ops, ws, nbytes, "extents"),
           (src, dst, 4, shape, (7, 5, -1), ops, ws, nbytes, "extents"),
           (src, dst, 4, shape, (41, 5, 37), ops, ws, nbytes, "ratio"),
           (src, dst, 4, (5, 57, 24), (7, 7, 37), ops, ws, nbytes, "ratio"),
           (src, dst, 4, shape, out_shape, (1, 3, 1), ws, nbytes, "operator"),
           (src, dst, 1, shape, out_shape, ops, ws, nbytes, "dtype"),
           (lab, dst, 3, shape, out_shape, ops, ws, nbytes, "dtype"),
           (src, dst, 4, shape, out_shape, ops, ws, nbytes - 1, "workspace"),
           (None, dst, 4, shape, out_shape, ops, ws, nbytes, "NULL"),
           (src, None, 4, shape, out_shape, ops, ws, nbytes, "NULL"),
           (src, dst, 4, shape, out_shape, ops, None, nbytes, "NULL"),
           (src, dst, 4, (2 ** 30 + 1, 7, 24), (2 ** 30 + 1, 5, 37), ops, ws, nbytes, "2\\^30"),
           (src, dst, 5, (2 ** 28, 2 ** 28, 24), (2 ** 28, 2 ** 28, 37), (1, 1, 1), ws, nbytes, "2\\^63"),
           (src, dst, 4, (2 ** 20, 2 ** 20, 24), (2 ** 20, 2 ** 20, 37), (0, 0, 0), ws, nbytes, "rows"))
    for *args, word in bad:
        rc = _abi_call(*args)
        assert rc == -1, (args[2:6], word)
        with pytest.raises(ValueError, match="sk_resample_volume.*" + word):
            _ffi.check(rc)
    assert _ffi.lib.sk_resample_workspace_bytes(4, *shape, 41, 5, 37, *ops) == 0
    torch.cuda.synchronize()
    assert bool((store == 0xA5).all()) and bool((ws_store == 0x5A).all())
