"""``lib.morphology.pool`` on CPU tensors against the block-by-block oracle of tests/pool_cases.py, ``plan_pyramid``, the
OME-Zarr layout ``write_ome_zarr`` leaves (NGFF 0.4 on zarr v2: every JSON file with exactly its keys and values, since no
third-party reader is available to open it), the command, and the refusals.  Nothing here needs a GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests import pool_cases as PC

from skoots_amd import _ffi
from skoots_amd.lib import ome_zarr, tiff, zarr_store
from skoots_amd.lib.morphology import pool
from skoots_amd.utils import pyramid as PY


def test_abi():
    assert _ffi.lib.sk_abi_version() >= 31 and "sk_pool_volume" in _ffi.EXPORTS


@pytest.mark.parametrize("how,dtype,shape,factors,sparse", PC.small_cases(),
                         ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_pool_cpu_equals_the_oracle(how, dtype, shape, factors, sparse):
    src = PC.to_torch(PC.source(how, dtype, shape))
    got = pool(src, factors, how, sparse)
    want = PC.expected(how, dtype, shape, factors, sparse)
    assert got.dtype == src.dtype and tuple(got.shape) == want.shape
    assert np.array_equal(PC.to_numpy(got), want)


def test_pool_keeps_the_rank_and_takes_a_signed_image():
    a = PC.source("mean", "uint16", (5, 7, 9))
    want = PC.expected("mean", "uint16", (5, 7, 9), (2, 2, 2))
    got = pool(torch.from_numpy(a.astype(np.int32)).unsqueeze(0), (2, 2, 2), "mean")
    assert got.dtype == torch.uint16 and tuple(got.shape) == (1,) + want.shape
    assert np.array_equal(PC.to_numpy(got[0]), want)
    with pytest.raises(ValueError, match="volume"):
        pool(torch.full((2, 2, 2), -1, dtype=torch.int32), (2, 2, 2), "mean")


@pytest.mark.parametrize("dtype", PC.MODE_DTYPES)
@pytest.mark.parametrize("factors", PC.FACTORS)
def test_mode_cases_hold_what_they_are_for(dtype, factors):
    """Ties, ties with zero among the tied values and all-distinct blocks really occur, and the planted blocks of a
    (2, 2, 2) pooling come out by the rules."""
    a = PC.mode_volume(dtype, PC.PLANTED_SHAPE)
    tied, zero_tied, distinct = PC.block_census(a, factors)
    assert tied > 0 and zero_tied > 0 and distinct > 0
    dense = PC.expected("mode", dtype, PC.PLANTED_SHAPE, factors, False)
    sparse = PC.expected("mode", dtype, PC.PLANTED_SHAPE, factors, True)
    assert (dense != sparse).any()
    if factors == (2, 2, 2):
        assert (dense[0, 0, 0:4] == 3).all()                                     # 4 + 4: the smaller value
        assert (dense[0, 0, 4:8] == 0).all() and (sparse[0, 0, 4:8] == 4).all()  # 4 + 4 with zero
        assert (dense[1, 0, :] == 20).all() and (dense[2, 0, :] == 40).all()     # 2 + 2 + 2 + 2, 8 distinct
        info = np.iinfo(dtype)
        assert (dense[3] == info.min).any() and (dense[3] >= info.max - 1).any() and a.max() == info.max


@pytest.mark.parametrize("dtype", PC.IMAGE_DTYPES)
def test_mean_cases_hold_what_they_are_for(dtype):
    a = PC.image_volume(dtype, (5, 7, 9)).astype(np.int64)
    top = np.iinfo(dtype).max
    full = half = 0
    for i, j, k in np.ndindex(2, 3, 4):                       # the unclipped (2, 2, 2) blocks
        s = int(a[2 * i:2 * i + 2, 2 * j:2 * j + 2, 2 * k:2 * k + 2].sum())
        full += s == 8 * top
        half += s % 8 == 4
    assert full > 0 and half > 0


# ---- plan_pyramid ----

def test_plan_anisotropic():
    plan = PY.plan_pyramid((64, 64, 16), (1, 1, 3), levels=5)
    assert [lv.factors for lv in plan] == [(1, 1, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)]
    assert [lv.shape for lv in plan] == [(64, 64, 16), (32, 32, 16), (16, 16, 8), (8, 8, 4), (4, 4, 2)]
    assert [lv.spacing for lv in plan] == [(1, 1, 3), (2, 2, 3), (4, 4, 6), (8, 8, 12), (16, 16, 24)]
    assert all(isinstance(v, float) for lv in plan for v in lv.spacing)


def test_plan_isotropic_and_odd_extents():
    plan = PY.plan_pyramid((70, 33, 9), (0.5, 0.5, 0.5), levels=4)
    assert [lv.factors for lv in plan[1:]] == [(2, 2, 2)] * 3
    assert [lv.shape for lv in plan] == [(70, 33, 9), (35, 17, 5), (18, 9, 3), (9, 5, 2)]


def test_plan_never_halves_an_extent_of_one():
    plan = PY.plan_pyramid((16, 1, 4), (1, 1, 1), levels=6)
    assert [lv.factors for lv in plan[1:]] == [(2, 1, 2), (2, 1, 2), (2, 1, 1), (2, 1, 1)]   # ends when all are 1
    assert plan[-1].shape == (1, 1, 1)
    # an axis of one voxel does not set the finest spacing either
    assert PY.plan_pyramid((8, 8, 1), (1, 1, 0.1), levels=2)[1].factors == (2, 2, 1)


def test_plan_stops():
    assert len(PY.plan_pyramid((64, 64, 16), (1, 1, 3))) == 1                   # already within until = 64
    plan = PY.plan_pyramid((1024, 1024, 256), (1, 1, 3))
    assert max(plan[-1].shape) <= 64 < max(plan[-2].shape) and len(plan) == 5
    assert len(PY.plan_pyramid((1024, 1024, 256), (1, 1, 3), until=300)) == 3
    assert len(PY.plan_pyramid((1024, 1024, 256), (1, 1, 3), levels=2, until=1)) == 2   # levels wins
    assert len(PY.plan_pyramid((9, 9, 9), (1, 1, 1), levels=1)) == 1


def test_plan_touches_no_tensor(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("plan_pyramid made a tensor")
    for name in ("empty", "zeros", "tensor", "as_tensor", "from_numpy"):
        monkeypatch.setattr(torch, name, boom)
    assert len(PY.plan_pyramid((40, 36, 24), (1, 1, 3), levels=3)) == 3


@pytest.mark.parametrize("kwargs", ({"shape": (4, 4), "spacing": (1, 1, 1)}, {"shape": (4, 0, 4), "spacing": (1, 1, 1)},
                                    {"shape": (4, 4, 4), "spacing": (1, 0, 1)}, {"shape": (4, 4, 4), "spacing": (1, 1)},
                                    {"shape": (4, 4, 4), "spacing": (1, 1, 1), "levels": 0},
                                    {"shape": (4, 4, 4), "spacing": (1, 1, 1), "until": 0}))
def test_plan_refusals(kwargs):
    with pytest.raises(ValueError, match="shape|spacing|levels|until"):
        PY.plan_pyramid(**kwargs)


# ---- write_ome_zarr ----

SHAPE, SPACING = (40, 36, 24), (1.0, 1.0, 3.0)


def _volumes():
    return (PC.to_torch(PC.source("mean", "uint16", SHAPE)), PC.to_torch(PC.source("mode", "int32", SHAPE)),
            PC.to_torch(PC.source("max", "uint8", SHAPE)))


def _json(*parts):
    with open(os.path.join(*parts)) as f:
        return json.load(f)


def _oracle_levels(how, dtype, plan, sparse=False):
    levels = [PC.source(how, dtype, SHAPE)]
    for lv in plan[1:]:
        levels.append(PC.oracle_pool(levels[-1], lv.factors, how, sparse))
    return levels


def _check_multiscales(group, name, how, plan, unit=None):
    attrs = _json(group, ".zattrs")
    ms = attrs["multiscales"]
    assert len(ms) == 1 and set(ms[0]) == {"version", "name", "axes", "datasets", "type"}
    assert ms[0]["version"] == "0.4" and ms[0]["name"] == name and ms[0]["type"] == how
    want_axes = [dict({"name": n, "type": "space"}, **({"unit": unit} if unit else {})) for n in ("z", "y", "x")]
    assert ms[0]["axes"] == want_axes
    assert ms[0]["datasets"] == [
        {"path": str(k), "coordinateTransformations": [{"type": "scale", "scale": [lv.spacing[2], lv.spacing[0], lv.spacing[1]]}]}
        for k, lv in enumerate(plan)]
    assert _json(group, ".zgroup") == {"zarr_format": 2}
    return attrs


def test_write_ome_zarr_layout_and_levels(tmp_path):
    image, mask, skel = _volumes()
    path = str(tmp_path / "vol.ome.zarr")
    report = PY.write_ome_zarr(path, SPACING, image=image, labels={"instances": mask, "skeleton": (skel, "max")},
                               levels=3, unit="micrometer")
    plan = report["plan"]
    assert [lv.factors for lv in plan] == [(1, 1, 1), (2, 2, 1), (2, 2, 2)] and report["levels"] == 3
    assert report["bytes_written"] > 0

    root = _check_multiscales(path, "vol", "mean", plan, "micrometer")
    assert set(root) == {"multiscales"}
    assert _json(path, "labels", ".zgroup") == {"zarr_format": 2}
    assert _json(path, "labels", ".zattrs") == {"labels": ["instances", "skeleton"]}
    for name, how in (("instances", "mode"), ("skeleton", "max")):
        attrs = _check_multiscales(os.path.join(path, "labels", name), name, how, plan, "micrometer")
        assert set(attrs) == {"multiscales", "image-label"}
        assert attrs["image-label"] == {"version": "0.4", "source": {"image": "../../"}}
    assert sorted(os.listdir(path)) == [".zattrs", ".zgroup", "0", "1", "2", "labels"]
    assert sorted(os.listdir(os.path.join(path, "labels"))) == [".zattrs", ".zgroup", "instances", "skeleton"]

    for group, how, dtype in ((path, "mean", "uint16"), (os.path.join(path, "labels", "instances"), "mode", "int32"),
                              (os.path.join(path, "labels", "skeleton"), "max", "uint8")):
        pairs = PY.read_multiscales(group)
        want = _oracle_levels(how, dtype, plan)
        assert [p for p, _ in pairs] == [os.path.join(group, str(k)) for k in range(3)]
        assert [s for _, s in pairs] == [[3.0, 1.0, 1.0], [3.0, 2.0, 2.0], [6.0, 4.0, 4.0]]   # doubled where halved
        for (array_path, _), level in zip(pairs, want):
            meta = _json(array_path, ".zarray")
            zxy = level.transpose(2, 0, 1)
            assert meta["shape"] == list(zxy.shape) and meta["chunks"] == [min(s, c) for s, c in zip(zxy.shape, (32, 256, 256))]
            assert meta["compressor"] == {"id": "zlib", "level": 1} and meta["zarr_format"] == 2 and meta["order"] == "C"
            got = zarr_store.load(array_path)
            assert got.dtype == level.dtype and np.array_equal(got, zxy)
            assert all("/" not in fn for fn in os.listdir(array_path))            # "."-separated chunk keys
    assert ome_zarr.read_labels(path) == ["instances", "skeleton"]


def test_write_ome_zarr_labels_only_sparse_and_rewrite(tmp_path):
    _, mask, _ = _volumes()
    path = str(tmp_path / "masks.ome.zarr")
    for _ in range(2):                                         # the second call replaces the first group
        report = PY.write_ome_zarr(path, SPACING, labels={"instances": mask}, levels=2, sparse=True)
    assert sorted(os.listdir(path)) == [".zgroup", "labels"]   # no multiscales at the root
    assert _json(path, ".zgroup") == {"zarr_format": 2}
    with pytest.raises(ValueError, match="multiscales"):
        PY.read_multiscales(path)
    group = os.path.join(path, "labels", "instances")
    attrs = _check_multiscales(group, "instances", "mode", report["plan"])
    assert attrs["image-label"] == {"version": "0.4"}
    want = _oracle_levels("mode", "int32", report["plan"], sparse=True)
    for (array_path, _), level in zip(PY.read_multiscales(group), want):
        assert np.array_equal(zarr_store.load(array_path), level.transpose(2, 0, 1))
    assert not np.array_equal(want[1], _oracle_levels("mode", "int32", report["plan"])[1])


def test_pyramid_returns_the_input_as_level_zero():
    _, mask, _ = _volumes()
    tensors, plan = PY.pyramid(mask, SPACING, "mode", levels=3)
    assert tensors[0].data_ptr() == mask.data_ptr() and len(tensors) == len(plan) == 3
    for t, lv, want in zip(tensors, plan, _oracle_levels("mode", "int32", plan)):
        assert tuple(t.shape) == lv.shape and np.array_equal(t.numpy(), want)


def test_command_end_to_end(tmp_path, capsys):
    image, mask, _ = _volumes()
    tiff.write_stack(str(tmp_path / "I.tif"), image.permute(2, 0, 1).contiguous())
    tiff.write_stack(str(tmp_path / "I_instance_mask.tif"), mask.permute(2, 0, 1).contiguous())
    zarr_store.save(str(tmp_path / "I_skoots_skeleton.zarr"), PC.source("max", "uint8", SHAPE)[None])
    out = PY.main(["--image", str(tmp_path / "I.tif"), "--labels", str(tmp_path / "I_instance_mask.tif"),
                   "--skeleton", str(tmp_path / "I_skoots_skeleton.zarr"), "--spacing", "1", "1", "3", "--levels", "3",
                   "--device", "cpu"])
    assert out == str(tmp_path / "I.ome.zarr")
    text = capsys.readouterr().out
    assert "level 2: factors (2, 2, 2) shape (X, Y, Z) (10, 9, 12) scale (z, y, x) [6.0, 4.0, 4.0]" in text
    assert "bytes written:" in text and "seconds:" in text and f"File Written: {out}" in text
    assert _json(out, "labels", ".zattrs") == {"labels": ["I_instance_mask", "skeleton"]}
    plan = PY.plan_pyramid(SHAPE, SPACING, levels=3)
    for group, how, dtype in ((out, "mean", "uint16"), (os.path.join(out, "labels", "I_instance_mask"), "mode", "int32"),
                              (os.path.join(out, "labels", "skeleton"), "max", "uint8")):
        for (array_path, _), level in zip(PY.read_multiscales(group), _oracle_levels(how, dtype, plan)):
            assert np.array_equal(zarr_store.load(array_path), level.transpose(2, 0, 1))
    out2 = PY.main(["--labels", str(tmp_path / "I_instance_mask.tif"), "--spacing", "1", "1", "1", "--until", "20",
                    "--sparse", "-o", str(tmp_path / "m.ome.zarr"), "--device", "cpu"])
    assert out2 == str(tmp_path / "m.ome.zarr") and len(PY.read_multiscales(os.path.join(out2, "labels", "I_instance_mask"))) == 2


# ---- refusals: by name, before anything is written ----

def test_pool_refusals(monkeypatch):
    monkeypatch.setattr(_ffi.lib, "sk_pool_volume", None)      # nothing below may reach the library
    v = torch.zeros((4, 4, 4), dtype=torch.int32)
    with pytest.raises(TypeError, match="volume.*float"):
        pool(v.float(), (2, 2, 2))
    with pytest.raises(TypeError, match="volume.*int64"):
        pool(v.long(), (2, 2, 2), "mode")
    with pytest.raises(TypeError, match="volume.*int32"):
        pool(v, (2, 2, 2), "max")
    with pytest.raises(TypeError, match="volume"):
        pool(v.numpy(), (2, 2, 2))
    for bad in ((3, 2, 2), (2, 2), (2, 2.0, 2), (0, 1, 2), 2):
        with pytest.raises(ValueError, match="factors"):
            pool(v, bad)
    with pytest.raises(ValueError, match=r"factors \(1, 1, 1\)"):
        pool(v, (1, 1, 1))
    with pytest.raises(ValueError, match="how"):
        pool(v, (2, 2, 2), "median")
    with pytest.raises(ValueError, match="sparse"):
        pool(v.to(torch.uint8), (2, 2, 2), "max", sparse=True)
    with pytest.raises(ValueError, match="volume.*shape"):
        pool(v[0], (2, 2, 2))


def test_write_refusals_leave_nothing(tmp_path):
    image, mask, _ = _volumes()
    path = str(tmp_path / "no.ome.zarr")
    with pytest.raises(TypeError, match="image.*float"):
        PY.write_ome_zarr(path, SPACING, image=image.float(), labels={"instances": mask})
    with pytest.raises(TypeError, match=r"labels\['instances'\].*float"):
        PY.write_ome_zarr(path, SPACING, image=image, labels={"instances": mask.float()})
    with pytest.raises(ValueError, match=r"labels\['instances'\].*shape"):
        PY.write_ome_zarr(path, SPACING, image=image, labels={"instances": mask[:-1]})
    with pytest.raises(ValueError, match="huffman"):
        PY.write_ome_zarr(path, SPACING, image=image, huffman="best")
    with pytest.raises(ValueError, match="spacing"):
        PY.write_ome_zarr(path, (1, 1), image=image)
    with pytest.raises(ValueError, match="how"):
        PY.write_ome_zarr(path, SPACING, labels={"instances": (mask, "mean")})
    with pytest.raises(ValueError, match="nothing to write"):
        PY.write_ome_zarr(path, SPACING)
    assert not os.path.exists(path)
    os.makedirs(tmp_path / "mine")
    (tmp_path / "mine" / "notes.txt").write_text("keep")
    with pytest.raises(FileExistsError):
        PY.write_ome_zarr(str(tmp_path / "mine"), SPACING, image=image)
    assert (tmp_path / "mine" / "notes.txt").read_text() == "keep"


def test_eval_signature():
    from skoots_amd.lib.eval import eval as sk_eval
    p = inspect.signature(sk_eval).parameters["pyramid"]
    assert p.default is False
    from skoots_amd.__main__ import build_parser
    assert build_parser().parse_args(["--pyramid"]).pyramid is True
    assert build_parser().parse_args([]).pyramid is False
