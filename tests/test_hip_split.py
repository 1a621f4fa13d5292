"""``sk_geodesic_init`` / ``sk_geodesic_rounds`` / ``sk_geodesic_finish`` (skoots_amd/csrc/geodesic.hip) and what stands on
them -- ``lib.morphology.geodesic_assign``, ``utils.split.split`` and its command, the ``cores`` column of
``stats_per_instance`` -- against the numpy oracle and the scipy restatement of tests/split_cases.py.  Everything is an
integer: every comparison is exact, owner and cost number for number.

The relaxation works on tiles of 4 x 8 x 64 voxels (x, y, z); (11, 19, 150) is two tiles and a remainder on every axis.
Also extents of 1, a volume below one tile, one voxel, no label, no seed."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import clean_cases as CC
from tests import split_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COSTS = ((1, 1, 1), (1, 1, 3))
SERPENTINE = (5, 11, 130)             # 2 x 2 x 3 tiles with a remainder on every axis; the oracle sweeps once per voxel of it


def _u_shape():
    return SC.issue_u_shape()[:2]


def _serpentine():
    m = CC.serpentine(SERPENTINE)
    s = np.zeros_like(m)
    s[0, 0, 0] = 5
    return m, s


CASES = {
    "u_shape": _u_shape,
    "serpentine": _serpentine,
    "crossing_one_face": SC.corridor_crossing_one_face,
    "shared_wall": SC.shared_wall,
    "seeds_on_tile_borders": SC.seeds_on_tile_borders,
    "tie_across_face": SC.tie_across_face,
    "noise_crossing": lambda: SC.noise(SC.CROSSING, 2),
    "noise_sparse_ids": lambda: SC.noise(SC.CROSSING, 3, ids=(0, 3, 7, 300, 2 ** 31 - 1)),
    "noise_uint8": lambda: SC.noise(SC.CROSSING, 12, seed_ids=(5, 6, 9, 200)),
    "dense_noise_crossing": lambda: SC.dense_noise(SC.CROSSING, 4),
    "line_z": lambda: SC.noise((1, 1, 200), 5, ids=(0, 1, 1, 2), seed_rate=0.05),
    "line_x": lambda: SC.noise((9, 1, 1), 6, ids=(1, 1, 1, 2), seed_rate=0.3),
    "line_y": lambda: SC.noise((1, 20, 1), 7, ids=(0, 1, 1, 2), seed_rate=0.2),
    "below_one_tile": lambda: SC.noise((3, 5, 40), 8, seed_rate=0.03),
    "one_voxel": lambda: (np.full((1, 1, 1), 6, np.int64), np.full((1, 1, 1), 4, np.int64)),
    "one_voxel_unseeded": lambda: (np.full((1, 1, 1), 6, np.int64), np.zeros((1, 1, 1), np.int64)),
    "all_zero": lambda: (np.zeros((5, 9, 66), np.int64), SC.noise((5, 9, 66), 9)[1]),
    "no_seeds": lambda: (SC.noise((5, 9, 66), 10)[0], np.zeros((5, 9, 66), np.int64)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    m, s = CASES[name]()
    m, s = np.ascontiguousarray(m).astype(np.int64), np.ascontiguousarray(s).astype(np.int64)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


@functools.lru_cache(maxsize=None)
def want(name, costs, max_cost=None):
    owner, cost, _ = SC.ref_geodesic(*case(name), costs, max_cost)
    owner.setflags(write=False)
    cost.setflags(write=False)
    return owner, cost


def on_device(v, dtype=None):
    v = np.asarray(v)
    if dtype is None:
        dtype = torch.int32 if v.max(initial=0) <= 2 ** 31 - 1 else torch.int64
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)        # a copy: the cached volumes are read-only


def assign(name, costs=(1, 1, 1), max_cost=None, dtype=None, stats=None):
    from skoots_amd.lib.morphology import geodesic_assign
    m, s = case(name)
    return geodesic_assign(on_device(m, dtype), on_device(s, dtype), costs, max_cost, stats=stats)


def check(name, costs=(1, 1, 1), max_cost=None, dtype=None, stats=None):
    owner, cost = assign(name, costs, max_cost, dtype, stats)
    want_owner, want_cost = want(name, costs, max_cost)
    assert owner.dtype == torch.int32 and cost.dtype == torch.int32 and owner.is_cuda and cost.is_cuda
    assert tuple(owner.shape) == want_owner.shape == tuple(cost.shape)
    for got, ref, what in ((owner.cpu().numpy(), want_owner, "owner"), (cost.cpu().numpy(), want_cost, "cost")):
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{what}: {len(bad)} voxels differ, first {bad[0]}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    return owner, cost


def test_abi():
    from skoots_amd import _ffi
    assert _ffi.lib.sk_abi_version() >= 27
    assert _ffi.lib.sk_geodesic_tiles(11, 19, 150) == 27 and _ffi.lib.sk_geodesic_max_rounds() >= 8


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("name", list(CASES))
def test_geodesic_assign(name, costs):
    check(name, costs)


def test_the_cases_test_what_they_are_for():
    owner, cost = want("u_shape", (1, 1, 3))
    assert set(np.unique(owner)) == {0, 5, 9} and cost.max() > 200
    owner, _ = want("shared_wall", (1, 1, 1))
    m, _ = case("shared_wall")
    assert (owner[m == 8] == 0).all() and (owner[m == 3] > 0).all() and set(np.unique(owner)) == {0, 11, 12}
    owner, cost = want("tie_across_face", (1, 1, 1))
    assert owner[3, 2, 5] == 4 and cost[3, 2, 5] == 3 and owner[1, 5, 64] == 2 and cost[1, 5, 64] == 20
    assert owner[2, 2, 5] == 9 and owner[1, 5, 65] == 3
    owner, _ = want("seeds_on_tile_borders", (1, 1, 3))
    assert set(np.unique(owner)) == set(range(21, 28))
    owner, _ = want("noise_sparse_ids", (1, 1, 1))
    assert (owner > 0).sum() > 100 and ((owner == 0) & (case("noise_sparse_ids")[0] > 0)).sum() > 100
    owner, cost = want("dense_noise_crossing", (1, 1, 1))
    assert cost.max() >= 12 and np.unique(owner).size > 20


def test_u_shape_owners_are_one_piece_each():
    from skoots_amd.lib.morphology import label_components
    owner, _ = check("u_shape", (1, 1, 3))
    table = label_components(owner)[1].cpu().numpy()
    assert sorted(table[:, 0].tolist()) == [5, 9]


def test_rounds_of_a_serpentine():
    """a one-voxel corridor through all 12 tiles, over and over: tiles that went idle are woken again"""
    from skoots_amd.lib.morphology import geodesic_round_bound
    stats = {}
    check("serpentine", (1, 1, 1), stats=stats)
    assert stats["tiles"] == 12 and stats["bound"] == geodesic_round_bound(SERPENTINE)
    assert 12 < stats["rounds"] <= stats["bound"] and stats["rounds"] < stats["launched"] <= stats["rounds"] + 8
    # the crossings a path makes decide, not the tiles: two tiles, nine crossings of the face between them
    stats = {}
    check("crossing_one_face", (1, 1, 1), stats=stats)
    assert stats["tiles"] == 2 and 9 <= stats["rounds"] <= 10 and stats["rounds"] <= stats["bound"]
    # a body inside one tile needs one round that changes something
    stats = {}
    check("below_one_tile", stats=stats)
    assert stats["rounds"] == 1
    stats = {}
    check("no_seeds", stats=stats)
    assert stats["rounds"] == 0 and stats["launched"] == 0


def test_max_cost_cuts_a_corridor():
    stats, free = {}, {}
    owner, cost = check("serpentine", (1, 1, 2), max_cost=400, stats=stats)
    assert int(cost.max().item()) in (399, 400) and int((owner > 0).sum().item()) < int((case("serpentine")[0] > 0).sum())
    check("serpentine", (1, 1, 2), stats=free)
    assert stats["rounds"] < free["rounds"]                   # what lies beyond the limit costs no round
    check("tie_across_face", (1, 1, 1), max_cost=0)
    check("tie_across_face", (1, 1, 1), max_cost=19)          # the middle voxel, at 20, is left out
    check("u_shape", (1, 1, 3), max_cost=2 ** 40)


@pytest.mark.parametrize("name, dtype", (("noise_sparse_ids", torch.int64), ("noise_uint8", torch.uint8),
                                         ("noise_uint8", torch.int16)))
def test_dtypes(name, dtype):
    check(name, (1, 1, 3), dtype=dtype)


def test_four_dimensions():
    from skoots_amd.lib.morphology import geodesic_assign
    m, s = case("noise_uint8")
    owner, cost = geodesic_assign(on_device(m)[None], on_device(s)[None], (1, 1, 3))
    assert owner.shape == m.shape and np.array_equal(owner.cpu().numpy(), want("noise_uint8", (1, 1, 3))[0])


def test_two_runs_are_identical():
    a = assign("dense_noise_crossing", (1, 1, 3))
    b = assign("dense_noise_crossing", (1, 1, 3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rows_are_taken():
    from skoots_amd.lib.morphology import geodesic_assign
    from skoots_amd.validate.lib import id_rows
    m, s = case("noise_sparse_ids")
    x = on_device(m)
    owner, cost = geodesic_assign(x, on_device(s), (1, 1, 3), rows=id_rows(x))
    assert np.array_equal(owner.cpu().numpy(), want("noise_sparse_ids", (1, 1, 3))[0])
    assert np.array_equal(cost.cpu().numpy(), want("noise_sparse_ids", (1, 1, 3))[1])


def test_refusals():
    from skoots_amd import _ffi
    from skoots_amd.lib.morphology import geodesic_assign
    m, s = (on_device(v) for v in case("below_one_tile"))
    with pytest.raises(ValueError, match="negative"):
        geodesic_assign(-m, s)
    with pytest.raises(ValueError, match="seeds"):
        geodesic_assign(m, -s)
    with pytest.raises(ValueError, match="seeds"):
        geodesic_assign(m, s.long() + 2 ** 31)
    with pytest.raises(ValueError, match="shape"):
        geodesic_assign(m, s[:, :, :-1])
    with pytest.raises(TypeError):
        geodesic_assign(m, s.float())
    with pytest.raises(ValueError, match="costs"):
        geodesic_assign(m, s, (1, 1, 256))
    with pytest.raises(ValueError, match="max_cost"):
        geodesic_assign(m, s, max_cost=-2)
    # the library's own guards: an error code and a message, nothing launched
    lib, p = _ffi.lib, _ffi.ptr
    keys = torch.zeros((2, m.numel()), dtype=torch.int64, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    words = torch.zeros(9, dtype=torch.int32, device=DEV)
    X, Y, Z = m.shape
    stream = _ffi.stream_ptr(m.device)
    a = m.to(torch.int32).contiguous()

    def rounds(X=X, Y=Y, Z=Z, costs=(1, 1, 1), max_cost=-1, ka=keys[0], kb=keys[1], first=0, n=1):
        return lib.sk_geodesic_rounds(p(a), X, Y, Z, *costs, max_cost, p(ka), p(kb), p(flags), first, n, p(words[1:]), stream)

    for bad in (dict(X=0), dict(costs=(0, 1, 1)), dict(costs=(1, 256, 1)), dict(max_cost=-2), dict(kb=keys[0]), dict(n=0),
                dict(n=lib.sk_geodesic_max_rounds() + 1), dict(first=-1), dict(X=2048, Y=1024, Z=1024),
                dict(X=1024, Y=1024, Z=256, costs=(1, 1, 8))):
        assert rounds(**bad) == -1 and _ffi.last_error().startswith("sk_geodesic_rounds"), bad
    assert lib.sk_geodesic_init(p(a), None, X, Y, Z, p(keys[0]), p(flags), p(words), stream) == -1
    assert lib.sk_geodesic_init(p(a), p(a), X, -1, Z, p(keys[0]), p(flags), p(words), stream) == -1
    assert lib.sk_geodesic_finish(p(keys[0]), -1, p(a), p(a), stream) == -1
    assert lib.sk_geodesic_tiles(0, 1, 1) == 0 and lib.sk_geodesic_tiles(2048, 1024, 1024) == 0
    # a negative value that reaches the library is reported through its error word, not ignored
    neg = a.clone()
    neg[0, 0, 0] = -3
    assert lib.sk_geodesic_init(p(neg), p(a), X, Y, Z, p(keys[0]), p(flags), p(words), stream) == 0
    assert int(words[0].item()) == 1
    assert lib.sk_geodesic_init(p(a), p(a), X, Y, Z, p(keys[0]), p(flags), p(words), stream) == 0
    assert int(words[0].item()) == 0


# ---- split ----

MASKS = {"dumbbell": SC.dumbbell, "blobs": SC.blobs_some_fused}


@functools.lru_cache(maxsize=None)
def mask(name):
    m = np.ascontiguousarray(MASKS[name]()).astype(np.int64)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def want_split(name, radius):
    return SC.ref_split(mask(name), radius)


def report_of(report):
    d = dataclasses.asdict(report)
    rounds = d.pop("rounds")
    return d, rounds


def test_split_dumbbell():
    from skoots_amd.lib.morphology import label_components
    from skoots_amd.utils.split import split
    out, report = split(on_device(mask("dumbbell")), 3.5)
    ref, rep = want_split("dumbbell", 3.5)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), ref)
    got, rounds = report_of(report)
    assert got == rep and rounds >= 1 and rep["instances_out"] == 2 and rep["instances_split"] == 1
    table = label_components(out)[1].cpu().numpy()
    assert sorted(table[:, 0].tolist()) == [6, 7]                             # two ids, each one piece
    assert table[table[:, 0] == 6, 1].item() > table[table[:, 0] == 7, 1].item()      # the larger side keeps the id
    assert int(out[9, 9, 33].item()) == 6 and int(out[9, 9, 8].item()) == 7
    again, report_again = split(on_device(mask("dumbbell")), 3.5)
    assert torch.equal(out, again) and report == report_again


@pytest.mark.parametrize("options", [dict(), dict(spacing=(1, 1, 2)), dict(spacing=(1, 1, 2), closed=True),
                                     dict(min_seed_voxels=100), dict(ids=(40,)), dict(ids=(7, 9)), dict(renumber=True),
                                     dict(spacing=(2, 2, 2), costs=(1, 1, 1))],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()).replace(" ", "") or "plain")
def test_split_blobs(options):
    from skoots_amd.utils.split import split
    radius = 3.5 * options.get("spacing", (1, 1, 1))[0]
    out, report = split(on_device(mask("blobs")), radius, **options)
    ref, rep = SC.ref_split(mask("blobs"), radius, **options)
    assert np.array_equal(out.cpu().numpy(), ref)
    got, rounds = report_of(report)
    assert got == rep, (got, rep)
    assert (rounds >= 1) == (rep["instances_split"] > 0)
    for u in np.unique(ref[ref > 0]):
        assert SC.pieces_of(ref, u) == 1


def test_the_masks_test_what_they_are_for():
    rep = want_split("blobs", 3.5)[1]
    assert rep["instances_in"] == 5 and rep["instances_split"] == 2 and rep["instances_out"] == 7 and rep["cores_found"] == 6
    assert SC.ref_split(mask("blobs"), 3.5, ids=(40,))[1]["instances_out"] == 6
    assert SC.ref_split(mask("blobs"), 3.5, ids=(7, 9))[1]["instances_split"] == 0
    assert SC.ref_split(mask("blobs"), 3.5, min_seed_voxels=100)[1]["cores_dropped"] > 0


def test_split_leaves_other_inputs_alone():
    from skoots_amd.utils.split import SplitReport, split
    zero = torch.zeros((5, 6, 7), dtype=torch.int32, device=DEV)
    out, report = split(zero, 2.0)
    assert torch.equal(out, zero) and report == SplitReport()
    out, report = split(torch.zeros((0, 6, 7), dtype=torch.int64, device=DEV), 2.0)
    assert out.shape == (0, 6, 7) and report == SplitReport()
    m = on_device(mask("dumbbell"), torch.int64)[None]                        # (1, X, Y, Z), int64
    out, report = split(m, 3.5)
    assert np.array_equal(out.cpu().numpy(), want_split("dumbbell", 3.5)[0])
    out, report = split(m, 9.0)                                                # no core: nothing happens
    assert np.array_equal(out.cpu().numpy(), mask("dumbbell")) and report.cores_found == 0 and report.rounds == 0
    big = m[0] * (2 ** 31 // 6 + 1)                                            # the id does not fit int32
    with pytest.raises(ValueError, match="beyond int32"):
        split(big, 3.5)
    out, report = split(big, 3.5, renumber=True)
    assert np.array_equal(out.cpu().numpy(), SC.ref_split(mask("dumbbell"), 3.5, renumber=True)[0])
    top = m[0] * 0 + torch.where(m[0] > 0, 2 ** 31 - 1, 0)                     # the new id does not
    with pytest.raises(ValueError, match="beyond int32"):
        split(top, 3.5)
    with pytest.raises(ValueError, match="not in the mask"):
        split(m, 3.5, ids=(5,))
    with pytest.raises(ValueError, match="costs"):
        split(m, 3.5, spacing=(0.5, 0.5, 1.0))
    with pytest.raises(ValueError, match="negative"):
        split(-m, 3.5)
    with pytest.raises(ValueError, match="radius"):
        split(m, -1.0)
    with pytest.raises(ValueError, match="min_seed_voxels"):
        split(m, 3.5, min_seed_voxels=0)


def test_command(tmp_path, capsys):
    from skoots_amd.lib import tiff
    from skoots_amd.utils import split as SP
    m = mask("blobs")
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, on_device(m).permute(2, 0, 1).contiguous())          # stored [Z, X, Y]
    before = open(path, "rb").read()
    out_path = SP.main([path, "--radius", "7", "--spacing", "2", "2", "2", "--costs", "1", "1", "1", "--ids", "40", "2"])
    assert out_path == str(tmp_path / "mask_split.tif") and open(path, "rb").read() == before
    want, report = SP.split(on_device(m), 7.0, spacing=(2.0, 2.0, 2.0), costs=(1, 1, 1), ids=(40, 2))
    back = tiff.read_stack(out_path, DEV).permute(1, 2, 0).to(torch.int32)
    assert torch.equal(back, want)
    assert np.array_equal(want.cpu().numpy(), SC.ref_split(m, 7.0, (2, 2, 2), costs=(1, 1, 1))[0])
    lines = capsys.readouterr().out.splitlines()
    assert lines[:7] == [f"{k}: {v}" for k, v in dataclasses.asdict(report).items()]
    assert lines[7] == f"File Written: {out_path}"
    with pytest.raises(SystemExit):
        SP.main([path])
    assert open(path, "rb").read() == before
    assert SP.main([path, "--radius", "3.5", "--renumber", "-o"]) == path
    assert torch.equal(tiff.read_stack(path, DEV).permute(1, 2, 0).to(torch.int32),
                       SP.split(on_device(m), 3.5, renumber=True)[0])


def test_cores_column_of_stats_per_instance(tmp_path):
    from skoots_amd.validate import compare as CMP
    m = mask("blobs")
    x = on_device(m)
    plain = CMP.stats_per_instance(x, (1.0, 1.0, 1.0))
    assert "cores" not in plain
    got = CMP.stats_per_instance(x, (1.0, 1.0, 1.0), cores=3.5)
    assert got["id"].cpu().tolist() == [2, 7, 9, 12, 40] and got["cores"].cpu().tolist() == [2, 1, 1, 0, 2]
    ids = got["id"].cpu().tolist()
    assert got["cores"].cpu().tolist() == [sum(c[0] == u for c in SC.ref_cores(m, 3.5)) for u in ids]
    assert all(torch.equal(got[c], plain[c]) for c in plain)
    wide = CMP.stats_per_instance(x, (1.0, 1.0, 2.0), cores=4.0, thickness="closed")
    assert wide["cores"].cpu().tolist() == [sum(c[0] == u for c in SC.ref_cores(m, 4.0, (1, 1, 2), True)) for u in ids]
    with pytest.raises(ValueError, match="cores"):
        CMP.stats_per_instance(x, cores=-1.0)
    # the command: the same file with and without the option differs by the one column only
    from skoots_amd.lib import tiff
    path = str(tmp_path / "mask.tif")
    tiff.write_label_stack(path, x.permute(2, 0, 1).contiguous())
    a = open(CMP.main([path, "--out", str(tmp_path / "a.csv")])).read().splitlines()
    b = open(CMP.main([path, "--cores", "3.5", "--out", str(tmp_path / "b.csv")])).read().splitlines()
    assert a[:2] == b[:2] and b[2] == a[2] + ",cores"
    assert b[3:] == [f"{line},{n}" for line, n in zip(a[3:], got["cores"].cpu().tolist())]
