"""``sk_convert_pages_u8`` (skoots_amd/csrc/convert.hip) and ``--convert`` on the device: against what the reference's own
``convert`` produced (tests/golden/convert.npz, every fp16 value with |x| <= 1 among it) and against the reference's
chain of torch operations run on the same device.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests.convert_cases import CASE_NAMES, expected_pages, load_cases, write_case

from skoots_amd import _ffi
from skoots_amd.lib import tiff
from skoots_amd.utils import convert_trch_to_tif as CV
from skoots_amd.utils import renumber as RN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _plan(case, x):
    vmax = x.max().item() if case.kind == "zarr" and x.ndim == 4 else None
    vmin = x.min().item() if case.kind == "trch" else None
    return CV.plan_conversion(case.kind, x.ndim, x.dtype, vmin, vmax)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_cases(name):
    case = load_cases()[name]
    x = torch.from_numpy(case.array.copy()).to(DEV)
    plan = _plan(case, x)
    want = torch.from_numpy(case.out)
    got = CV.make_pages(x, plan)
    assert got.dtype == want.dtype and torch.equal(got.cpu().reshape(want.shape), want)
    assert torch.equal(CV.pages_torch(x, plan.mode).cpu().reshape(want.shape), want)      # the other route, same device
    if x.ndim == 4:                                                                         # and the kernel itself
        assert plan.mode is not None
        assert torch.equal(CV.pages_kernel(x, plan.mode).cpu(), want)
    elif plan.mode is not None:
        assert torch.equal(CV.pages_kernel(x.unsqueeze(0), plan.mode).cpu()[..., 0], want)


@pytest.mark.parametrize("mode,name", ((CV.MODE_TRUNC, "every_fp16_store"), (CV.MODE_ROUND, "every_fp16_trch")))
def test_every_fp16_value_up_to_one(mode, name):
    """fp32 arithmetic would give another byte for 1 002 (mode 1) / 3 822 (mode 2) of the 30 722 values."""
    case = load_cases()[name]
    x = torch.from_numpy(case.array.copy()).to(DEV)
    got = CV.pages_kernel(x, mode).cpu()
    want = torch.from_numpy(case.out)
    assert torch.equal(got, want), int((got != want).sum())
    wide = CV.pages_torch(x.float(), mode).cpu()
    assert int((wide != want).sum()) == {CV.MODE_TRUNC: 1002, CV.MODE_ROUND: 3822}[mode]


def _values(shape, dtype, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        return torch.randint(0, 256 if mode == CV.MODE_CAST else 2 + 254 * (seed % 2), shape, generator=gen,
                             dtype=torch.uint8)
    if mode == CV.MODE_CAST:
        x = torch.rand(shape, generator=gen) * 255.99
    else:
        x = torch.rand(shape, generator=gen) * 2 - 1
        flat = x.reshape(-1)
        flat[torch.randperm(n, generator=gen)[: max(1, n // 7)]] = 0.0
        flat[torch.randperm(n, generator=gen)[: max(1, n // 11)]] = -0.0
        wide = torch.randperm(n, generator=gen)[: n // 5]
        flat[wide] = flat[wide] * 3        # t outside [0, 256) too: unpinned in the reference, equal on both routes
    return x.to(dtype)


SHAPES = ((3, 5, 7, 9), (1, 33, 70, 65), (4, 2, 129, 3), (3, 1, 1, 1), (2, 3, 5, 1), (3, 64, 64, 64))


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_torch_route(shape):
    for dtype in (torch.uint8, torch.float16, torch.float32):
        for mode in (CV.MODE_CAST, CV.MODE_TRUNC, CV.MODE_ROUND):
            x = _values(shape, dtype, mode, seed=sum(shape) + mode).to(DEV)
            got = CV.pages_kernel(x, mode)
            want = CV.pages_torch(x, mode)
            assert got.shape == (shape[3], shape[1], shape[2], shape[0]) and got.dtype == torch.uint8
            assert torch.equal(got, want), (shape, dtype, mode, int((got != want).sum()))
            if mode == CV.MODE_CAST and dtype == torch.uint8:
                assert torch.equal(got, x.permute(3, 1, 2, 0))                              # a pure transpose


def test_sixteen_byte_and_bytewise_stores_agree():
    """Y * C a multiple of 16 takes 16-byte stores, anything else (and a destination off a 16-byte boundary) single
    bytes: the same pages either way."""
    x = _values((3, 3, 80, 70), torch.float16, CV.MODE_TRUNC, seed=9).to(DEV)              # Y * C = 240
    want = CV.pages_torch(x, CV.MODE_TRUNC)
    assert torch.equal(CV.pages_kernel(x, CV.MODE_TRUNC), want)
    buf = torch.zeros(want.numel() + 16, dtype=torch.uint8, device=DEV)
    out = buf[1:1 + want.numel()]
    _ffi.check(_ffi.lib.sk_convert_pages_u8(_ffi.ptr(x), 1, CV.MODE_TRUNC, 3, 3, 80, 70, _ffi.ptr(out),
                                            _ffi.stream_ptr(x.device)))
    assert torch.equal(out.view(want.shape), want) and int(buf[0]) == 0 and int(buf[1 + want.numel():].sum()) == 0


@pytest.mark.parametrize("read_on_device", (False, True))
@pytest.mark.parametrize("name", ("vectors_store", "skeleton_store"))
def test_convert_end_to_end(name, read_on_device, tmp_path):
    case = load_cases()[name]
    path = write_case(case, str(tmp_path))
    (out,) = CV.convert(path, device=DEV, read_on_device=read_on_device)
    assert out == os.path.join(str(tmp_path), case.out_name)
    want = expected_pages(case)
    assert np.array_equal(tiff.read_image(out), want)                                       # Pillow opens it
    assert np.array_equal(tiff.read_stack(out, DEV).cpu().numpy(), want)


def test_renumber_on_device_matches_cpu(tmp_path):
    rng = np.random.default_rng(4)
    ids = np.concatenate([[0], rng.choice(np.arange(1, 200000), 400, replace=False)])
    vol = rng.choice(ids, (6, 40, 37)).astype(np.int32)
    path = str(tmp_path / "m.tif")
    tiff.write_stack(path, vol)
    cpu = tiff.read_image(RN.load_renumber_save(path, False, device="cpu"))
    os.rename(str(tmp_path / "m_remapped.tif"), str(tmp_path / "cpu.tif"))
    gpu = tiff.read_image(RN.load_renumber_save(path, False, device=DEV))
    assert gpu.dtype == cpu.dtype == np.uint16 and np.array_equal(gpu, cpu)


def test_bad_arguments_are_refused_before_a_launch():
    x = torch.zeros((3, 4, 5, 6), dtype=torch.float16, device=DEV)
    out = torch.full((6 * 4 * 5 * 3,), 7, dtype=torch.uint8, device=DEV)
    s = _ffi.stream_ptr(x.device)
    call = _ffi.lib.sk_convert_pages_u8
    assert call(_ffi.ptr(x), 1, 1, 5, 4, 5, 6, _ffi.ptr(out), s) == -1 and "C = 5" in _ffi.last_error()
    assert call(None, 1, 1, 3, 4, 5, 6, _ffi.ptr(out), s) == -1 and "NULL" in _ffi.last_error()
    assert call(_ffi.ptr(x), 1, 1, 3, 4, 5, 6, None, s) == -1
    assert call(_ffi.ptr(x), 3, 1, 3, 4, 5, 6, _ffi.ptr(out), s) == -1
    assert call(_ffi.ptr(x), 1, 3, 3, 4, 5, 6, _ffi.ptr(out), s) == -1
    assert call(_ffi.ptr(x), 1, 1, 3, 0, 5, 6, _ffi.ptr(out), s) == -1
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    assert _ffi.lib.sk_abi_version() >= 11
