"""``skoots_amd.utils.flood_and_stitch`` without a GPU: the reference's own results (tests/golden/flood_and_stitch.npz, made
by tests/golden/make_flood_and_stitch_golden.py: the stitched volume BEFORE the final renumbering, for dim 0, 1, 2)
against a voxel-level restatement, against the host table walk ``sk_stitch_walk_host`` on scipy-made tables, and against
the whole CPU route; the table walk against a naive one on random tables; the errors; the command.  All exact."""
import os
import struct

import numpy as np
import pytest
import torch

from tests import stitch_reference as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "flood_and_stitch.npz")


def _cases():
    g = np.load(GOLDEN)
    return g, [str(n) for n in g["names"]]


_G, NAMES = _cases()
CASES = [(n, d) for n in NAMES for d in range(3)]


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 256 << 10
    assert len([n for n in NAMES if n.startswith("field")]) == 15
    assert {"tie", "newind_taken", "same_number", "split_rejoin", "single_slice", "empty"} <= set(NAMES)


def test_abi():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 14


@pytest.mark.parametrize("name,dim", CASES)
def test_voxel_restatement_equals_reference(name, dim):
    assert np.array_equal(R.voxel_stitch(_G[f"mask_{name}"], dim), _G[f"labels_{name}_d{dim}"])


@pytest.mark.parametrize("name,dim", CASES)
def test_stitch_tables_equals_reference(name, dim):
    from skoots_amd.utils import flood_and_stitch as F
    labels, offsets, rows = R.plane_tables(_G[f"mask_{name}"], dim)
    lut, mx = F.stitch_tables(offsets, rows)
    want = _G[f"labels_{name}_d{dim}"]
    assert lut.dtype == torch.int32 and lut.numel() == offsets[-1] + 1 and int(lut[0]) == 0
    assert np.array_equal(lut.numpy()[labels], want)
    assert mx == int(want.max())


@pytest.mark.parametrize("quirk,name", [("tie", "tie"), ("newind", "newind_taken"), ("same", "same_number"),
                                        ("same", "split_rejoin")])
def test_hand_cases_depend_on_the_quirks(quirk, name):
    """Each of the reference's three quirks decides a hand-made case: the walk without it gives another partition."""
    labels, offsets, rows = R.plane_tables(_G[f"mask_{name}"], 0)
    want = R.first_seen(_G[f"labels_{name}_d0"])
    assert np.array_equal(R.first_seen(R.naive_table_walk(offsets, rows)[labels]), want)
    assert not np.array_equal(R.first_seen(R.naive_table_walk(offsets, rows, without=quirk)[labels]), want)


def _random_tables(rng):
    P = int(rng.integers(1, 13))
    counts = rng.integers(0, 10, size=P)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = []
    for p in range(P - 1):
        for a in range(offsets[p] + 1, offsets[p + 1] + 1):
            for b in range(offsets[p + 1] + 1, offsets[p + 2] + 1):
                if rng.random() < 0.3:
                    rows.append((a, b, int(rng.integers(1, 4))))   # few distinct counts: many ties
    return offsets, np.array(rows, dtype=np.int32).reshape(-1, 3)


def test_stitch_tables_equals_naive_walk_on_random_tables():
    from skoots_amd.utils import flood_and_stitch as F
    rng = np.random.default_rng(20)
    renamed = 0
    for _ in range(200):
        offsets, rows = _random_tables(rng)
        lut, mx = F.stitch_tables(offsets, rows)
        want = R.naive_table_walk(offsets, rows)
        assert np.array_equal(lut.numpy(), want), (offsets.tolist(), rows.tolist())
        assert mx == int(want.max())
        renamed += int(want.max() > offsets[-1])
    assert renamed > 100


def test_stitch_tables_refuses_malformed_tables():
    from skoots_amd.utils import flood_and_stitch as F
    off = np.array([0, 2, 4], dtype=np.int32)
    F.stitch_tables(off, np.array([[1, 3, 1], [1, 4, 2]], dtype=np.int32))
    for rows in ([[1, 4, 2], [1, 3, 1]],      # not sorted
                 [[1, 2, 1]],                 # both in plane 0
                 [[3, 1, 1]],                 # backwards
                 [[1, 5, 1]],                 # id past the total
                 [[1, 3, 0]]):                # empty overlap
        with pytest.raises(ValueError):
            F.stitch_tables(off, np.array(rows, dtype=np.int32))
    with pytest.raises(ValueError):
        F.stitch_tables(np.array([1, 2], dtype=np.int32), np.zeros((0, 3), dtype=np.int32))


@pytest.mark.parametrize("name,dim", CASES)
def test_cpu_route_equals_renumbered_reference(name, dim):
    from skoots_amd.utils import flood_and_stitch as F
    from skoots_amd.utils.renumber import compact_by_rank, renumber_first_seen
    mask = _G[f"mask_{name}"]
    got = F.watershed_and_stitch(torch.from_numpy(mask), dim)
    assert got.dtype == torch.int32 and got.shape == mask.shape and got.device.type == "cpu"
    compact, k = compact_by_rank(torch.from_numpy(_G[f"labels_{name}_d{dim}"]))
    want = renumber_first_seen(compact, k)
    assert torch.equal(got, want)
    assert np.array_equal(got.numpy(), R.first_seen(_G[f"labels_{name}_d{dim}"]))


def test_stages_on_cpu_tensors():
    from skoots_amd.utils import flood_and_stitch as F
    mask = _G["mask_field21"]
    for dim in range(3):
        labels, offsets = F.label_planes(torch.from_numpy(mask), dim)
        want_labels, want_offsets, want_rows = R.plane_tables(mask, dim)
        assert labels.dtype == torch.int32 and np.array_equal(labels.numpy(), want_labels)
        assert offsets.dtype == torch.int32 and np.array_equal(offsets.numpy(), want_offsets)
        rows = F.plane_overlaps(labels, offsets, dim)
        assert rows.dtype == torch.int32 and np.array_equal(rows.numpy(), want_rows)


def test_accepts_numpy_and_bool():
    from skoots_amd.utils import flood_and_stitch as F
    mask = _G["mask_split_rejoin"]
    want = F.watershed_and_stitch(torch.from_numpy(mask), 0)
    assert torch.equal(F.watershed_and_stitch(mask, 0), want)
    assert torch.equal(F.watershed_and_stitch(mask.astype(bool), 0), want)
    assert torch.equal(F.watershed_and_stitch(torch.from_numpy(mask * 200), 0), want)   # anything nonzero is foreground


def test_single_slice_and_empty():
    from skoots_amd.utils import flood_and_stitch as F
    one = _G["mask_single_slice"]
    import scipy.ndimage
    assert np.array_equal(F.watershed_and_stitch(one, 0).numpy()[0], scipy.ndimage.label(one[0])[0])
    assert not F.watershed_and_stitch(np.zeros((3, 4, 5), dtype=np.uint8), 1).any()
    assert F.watershed_and_stitch(np.zeros((0, 4, 5), dtype=np.uint8), 0).shape == (0, 4, 5)


def test_value_errors():
    from skoots_amd.utils import flood_and_stitch as F
    good = np.zeros((2, 3, 4), dtype=np.uint8)
    for mask, dim in ((np.zeros((3, 4), dtype=np.uint8), 0), (np.zeros((1, 2, 3, 4), dtype=np.uint8), 0),
                      (good.astype(np.int32), 0), (good.astype(np.float32), 0), (torch.zeros((2, 3, 4), dtype=torch.int64), 0),
                      (good, 3), (good, -1), (good, 1.0)):
        with pytest.raises(ValueError):
            F.watershed_and_stitch(mask, dim)
    huge = torch.zeros(1, dtype=torch.uint8).expand(2048, 1024, 1024)    # no storage behind it: refused by its shape
    with pytest.raises(ValueError, match=r"\(2048, 1024, 1024\)"):
        F.watershed_and_stitch(huge, 0)


def test_command_writes_replaced_tif(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import flood_and_stitch as F
    mask = _G["mask_field11"]
    path = str(tmp_path / "stack.tif")
    tiff.write_stack(path, torch.from_numpy(mask * 255))
    with pytest.warns(UserWarning, match="--distance"):
        out = F.main([path, "-d", "1", "--distance", "--log", "4"])
    assert out == str(tmp_path / "stack_replaced.tif") and os.path.exists(out)
    want = F.watershed_and_stitch(torch.from_numpy(mask), 1)
    back = tiff.read_stack(out, "cpu")
    assert int(want.max()) <= 255 and back.dtype == torch.uint8
    assert torch.equal(back.to(torch.int32), want)
    with pytest.raises(ValueError):
        F.flood_stitch_save(out, 5)


def test_wide_label_counts_are_written_as_uint16(tmp_path):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import flood_and_stitch as F
    mask = np.zeros((2, 40, 40), dtype=np.uint8)
    mask[0, ::2, ::2] = 1                        # 400 one-voxel objects in slice 0, none below them
    path = str(tmp_path / "many.tif")
    tiff.write_stack(path, torch.from_numpy(mask))
    out = F.flood_stitch_save(path, 0, device="cpu")
    back = tiff.read_stack(out, "cpu")
    assert back.dtype == torch.uint16 and int(back.to(torch.int32).max()) == 400


def write_host_check_tables(path):
    """The file tools/stitch_host_check.cpp reads: int32 n, then per case int32 P, int64 R, P + 1 offsets, R x 3 rows,
    T + 1 expected lut entries (T = offsets[P]).  Every fixture case and the random tables of the test above."""
    tables = []
    for name, dim in CASES:
        _, offsets, rows = R.plane_tables(_G[f"mask_{name}"], dim)
        tables.append((offsets, rows))
    rng = np.random.default_rng(20)
    tables += [_random_tables(rng) for _ in range(200)]
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(tables)))
        for offsets, rows in tables:
            f.write(struct.pack("<iq", len(offsets) - 1, len(rows)))
            f.write(np.asarray(offsets, dtype="<i4").tobytes())
            f.write(np.asarray(rows, dtype="<i4").tobytes())
            f.write(R.naive_table_walk(offsets, rows).astype("<i4").tobytes())
    return len(tables)


def test_host_check_tables_file(tmp_path):
    path = str(tmp_path / "stitch_tables.bin")
    n = write_host_check_tables(path)
    assert n == len(CASES) + 200 and os.path.getsize(path) > 4
