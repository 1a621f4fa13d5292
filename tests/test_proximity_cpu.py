"""The numpy restatement of ``sk_instance_proximity`` (tests/proximity_cases.py) against a plain loop and against scipy's
distance transform, and the host side of ``proximity``: the reach, ``plan_proximity``, the CSV texts, the command line,
and the entry point's argument refusals, which need no device."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import contact_cases as K
from tests import proximity_cases as P

NOISE = [((1.0, 1.0, 1.0), 2.0), ((1.0, 1.0, 3.0), 3.0), ((0.5, 0.7, 1.3), 1.5)]


@functools.lru_cache(maxsize=None)
def noise():
    a, b = P.noise_pair(K.CROSSING, 5)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("spacing, distance", [((1.0, 1.0, 1.0), 1.5), ((1.0, 2.0, 3.0), 3.0), ((0.5, 0.7, 1.3), 1.0)])
@pytest.mark.parametrize("same", [False, True])
def test_oracle_equals_a_plain_loop(spacing, distance, same):
    a, b = P.noise_pair((3, 4, 9), 2)
    want = P.loop_proximity(a, None if same else b, distance, spacing)
    got = P.ref_proximity(a, None if same else b, distance, spacing)
    assert want[0].shape[0] > 3 and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


@pytest.mark.parametrize("spacing, distance", NOISE[:2])
def test_oracle_equals_scipy_at_integer_spacings(spacing, distance):
    from scipy import ndimage as ndi
    a, b = noise()
    ra, rb = K.rows_of(a)[0], K.rows_of(b)[0]
    pairs, gap2 = P.ref_proximity(a, b, distance, spacing)
    want, any_b = {}, ndi.distance_transform_edt(rb == 0, sampling=spacing)
    for r_a in range(1, int(ra.max()) + 1):
        for r_b in range(0, int(rb.max()) + 1):
            d = (any_b if r_b == 0 else ndi.distance_transform_edt(rb != r_b, sampling=spacing))[ra == r_a]
            if (d <= distance).any():
                want[(r_a, r_b)] = (int((d <= distance).sum()), float(d.min()))
    assert sorted(want) == [tuple(r[:2]) for r in pairs.tolist()]
    assert [want[k][0] for k in sorted(want)] == pairs[:, 2].tolist()
    assert [want[k][1] for k in sorted(want)] == np.sqrt(gap2).tolist()


@pytest.mark.parametrize("spacing, distance", NOISE)
def test_gap2_is_symmetric_between_the_directions(spacing, distance):
    a, b = noise()
    (ab, g_ab), (ba, g_ba) = P.ref_proximity(a, b, distance, spacing), P.ref_proximity(b, a, distance, spacing)
    one = {(r[0], r[1]): g for r, g in zip(ab.tolist(), g_ab.tolist()) if r[1]}
    other = {(r[1], r[0]): g for r, g in zip(ba.tolist(), g_ba.tolist()) if r[1]}
    assert one == other and len(one) == 9
    same, g = P.ref_proximity(a, None, distance, spacing)
    table = {(r[0], r[1]): v for r, v in zip(same.tolist(), g.tolist())}
    assert all(r[0] != r[1] for r in same.tolist()) and all(table[(k[1], k[0])] == v for k, v in table.items() if k[1])


def test_distance_zero_is_the_overlap_table():
    from tests import overlap_cases as O
    a, b = noise()
    pairs, gap2 = P.ref_proximity(a, b, 0.0, (1.0, 1.0, 3.0))
    assert np.array_equal(pairs[pairs[:, 1] > 0], O.ref_overlaps(a, b)) and (gap2 == 0).all()


def test_the_overflow_pair_overflows():
    """one voxel of a sees more rows of b than a lane keeps, and a tile more keys than its table holds"""
    a, b = P.voxel_ids_pair()
    pairs, _ = P.ref_proximity(a, b, 2.0)
    per_voxel_most = 33                                   # offsets within 2 voxels
    assert pairs.shape[0] > 4 * P.LDS_SLOTS and per_voxel_most > P.SEEN
    # an interior voxel of a meets every one of the 33 offsets as a row of its own
    assert pairs[pairs[:, 1] > 0, 2].max() > 2 * P.SEEN and pairs[pairs[:, 1] > 0, 2].sum() > 33 * a.size // 4


# ---- the reach ----

def test_reach_at_the_boundary():
    from skoots_amd.validate.lib import proximity_reach
    assert proximity_reach(0.0) == (0, 0, 0) and proximity_reach(0.999) == (0, 0, 0) and proximity_reach(1.0) == (1, 1, 1)
    assert proximity_reach(3.0, (1.0, 1.0, 3.0)) == (3, 3, 1) and proximity_reach(2.999, (1.0, 1.0, 3.0)) == (2, 2, 0)
    assert proximity_reach(5.0) == (5, 5, 5) and proximity_reach(5.99) == (5, 5, 5)
    # fl(w k^2) == limit2 exactly counts: 0.1^2 * 9 against (0.1 * 3)^2 differ in the last bit, found by search
    for s, k in ((0.1, 3), (0.7, 3), (1.3, 2), (0.3, 5)):
        w = s * s
        d = math.sqrt(w * float(k * k))
        if d * d == w * float(k * k):
            assert proximity_reach(d, (s, 1e6, 1e6)) == (k, 0, 0)
        below = math.nextafter(w * float(k * k), 0.0)
        d = math.sqrt(below)
        d = d if d * d <= below else math.nextafter(d, 0.0)
        assert d * d < w * float(k * k) and proximity_reach(d, (s, 1e6, 1e6)) == (k - 1, 0, 0)
    for spacing, distance in NOISE:
        assert proximity_reach(distance, spacing) == P.reach(*P.metric(distance, spacing))


def test_reach_refusals_name_the_largest_distance():
    from skoots_amd.validate.lib import proximity_reach
    with pytest.raises(ValueError, match="below"):
        proximity_reach(40.0)
    with pytest.raises(ValueError) as e:
        proximity_reach(100.0, (1.0, 1.0, 3.0))
    limit = float(str(e.value).rsplit("below ", 1)[1])
    assert proximity_reach(math.nextafter(limit, 0.0), (1.0, 1.0, 3.0))
    with pytest.raises(ValueError):
        proximity_reach(limit, (1.0, 1.0, 3.0))
    for bad in (-1.0, float("nan"), float("inf"), None, "3", True, 1e200):
        with pytest.raises(ValueError, match="distance"):
            proximity_reach(bad)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            proximity_reach(1.0, bad)


# ---- plan_proximity ----

def test_plan_proximity_on_a_hand_written_table():
    from skoots_amd.validate.lib import plan_proximity
    pairs = np.array([[1, 0, 9], [1, 2, 4], [1, 3, 7], [1, 5, 1],       # row 1: a tie between 3 and 5 -> the lower row
                      [2, 0, 2], [2, 4, 2],                               # row 2: one partner
                      [4, 0, 1], [4, 1, 1]], np.int64)                    # row 3 has none; row 4 overlaps (gap 0)
    gap2 = np.array([1.0, 4.0, 1.0, 1.0, 2.25, 2.25, 0.0, 0.0])
    p = plan_proximity(pairs, gap2, 4, 5)
    assert p["partners"].tolist() == [3, 1, 0, 1] and p["nearest_row"].tolist() == [3, 4, 0, 1]
    assert p["nearest_gap2"].tolist() == [1.0, 2.25, np.inf, 0.0] and p["near_voxels"].tolist() == [9, 2, 0, 1]
    assert all(v.dtype == (np.float64 if k == "nearest_gap2" else np.int64) for k, v in p.items())
    shuffled = np.random.default_rng(0).permutation(8)
    q = plan_proximity(pairs[shuffled], gap2[shuffled], 4, 5)
    assert all(np.array_equal(p[k], q[k]) for k in p)


def test_plan_proximity_without_rows():
    from skoots_amd.validate.lib import plan_proximity
    for n, m in ((0, 0), (0, 3), (4, 0), (4, 3)):
        p = plan_proximity(np.zeros((0, 3), np.int64), np.zeros(0), n, m)
        assert all(v.shape == (n,) for v in p.values()) and (p["nearest_gap2"] == np.inf).all()
        assert not p["partners"].any() and not p["nearest_row"].any() and not p["near_voxels"].any()
    with pytest.raises(ValueError, match="rows"):
        plan_proximity(np.array([[1, 0, 1]]), np.zeros(2), 1, 1)
    with pytest.raises(ValueError, match="outside"):
        plan_proximity(np.array([[2, 0, 1]]), np.zeros(1), 1, 1)


@pytest.mark.parametrize("spacing, distance", NOISE)
def test_plan_proximity_equals_plain_loops(spacing, distance):
    from skoots_amd.validate.lib import plan_proximity
    a, b = P.many_ids_pair()
    a, b = a[:5, :6, :20], b[:5, :6, :20]
    pairs, gap2 = P.ref_proximity(a, b, distance, spacing)
    n, m = K.rows_of(a)[1].size, K.rows_of(b)[1].size
    p = plan_proximity(pairs, gap2, n, m)
    want = P.ref_plan(pairs, gap2, n)
    got = list(zip(p["partners"].tolist(), p["nearest_row"].tolist(), p["nearest_gap2"].tolist(), p["near_voxels"].tolist()))
    assert got == want and max(w[0] for w in want) > 1


# ---- texts and the command line ----

def test_proximity_csv_texts():
    from skoots_amd.utils import proximity as X
    pair = {"a_id": torch.tensor([3, 2 ** 40]), "b_id": torch.tensor([7, 7]),
            "gap": torch.tensor([0.0, 2.5], dtype=torch.float64), "a_near_voxels": torch.tensor([4, 1]),
            "a_near_fraction": torch.tensor([0.4, 0.1], dtype=torch.float64), "b_near_voxels": torch.tensor([5, 2]),
            "b_near_fraction": torch.tensor([0.25, 1 / 3], dtype=torch.float64)}
    text = X.format_pairs_csv("a.tif", "b.tif", pair, 3, (1, 1, 3))
    assert text == ("A File: a.tif B File: b.tif\nSpacing: 1.0 1.0 3.0 Distance: 3.0\n" + X.PAIR_CSV_COLUMNS + "\n"
                    "3,7,0.0,4,0.4,5,0.25\n" + f"{2 ** 40},7,2.5,1,0.1,2,{1 / 3!r}\n")
    near = {"id": torch.tensor([3, 9]), "voxels": torch.tensor([10, 6]), "partners": torch.tensor([2, 0]),
            "nearest_id": torch.tensor([7, 0]), "nearest_gap": torch.tensor([1.5, math.inf], dtype=torch.float64),
            "near_voxels": torch.tensor([4, 0]), "near_fraction": torch.tensor([0.4, 0.0], dtype=torch.float64)}
    text = X.format_near_csv("a.tif", None, near, 0.5)
    assert text == ("A File: a.tif B File: a.tif\nSpacing: 1.0 1.0 1.0 Distance: 0.5\n" + X.NEAR_CSV_COLUMNS + "\n"
                    "3,10,2,7,1.5,4,0.4\n9,6,0,0,inf,0,0.0\n")
    assert X.format_near_csv("a.tif", None, near, 0.5) == text
    assert X.PAIR_CSV_COLUMNS == "a_id,b_id,gap,a_near_voxels,a_near_fraction,b_near_voxels,b_near_fraction"
    assert X.NEAR_CSV_COLUMNS == "id,voxels,partners,nearest_id,nearest_gap,near_voxels,near_fraction"


def test_proximity_parse_args():
    from skoots_amd.utils.proximity import parse_args
    args = parse_args(["a.tif", "--distance", "2"])
    assert (args.a, args.b, args.distance, tuple(args.spacing)) == ("a.tif", None, 2.0, (1.0, 1.0, 1.0))
    assert not args.save_sites and not args.overwrite
    args = parse_args(["a.tif", "b.tif", "--distance", "0.03", "--spacing", "0.01", "0.01", "0.03", "--save-sites", "-o"])
    assert (args.b, args.distance, tuple(args.spacing)) == ("b.tif", 0.03, (0.01, 0.01, 0.03))
    assert args.save_sites and args.overwrite
    for bad in (["a.tif"], ["a.tif", "--distance", "-1"], ["a.tif", "--distance", "nan"], ["a.tif", "--distance", "inf"],
                ["a.tif", "--distance", "1", "--save-sites"], ["a.tif", "b.tif", "--distance", "1", "-o"],
                ["--distance", "1"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_instance_stats_csv_with_the_near_columns():
    from skoots_amd.validate import compare as CMP
    sums = torch.tensor([[8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 8, 8, 8]], dtype=torch.int64)      # a 2 x 2 x 2 cube at the origin
    boxes = torch.tensor([[0, 0, 0, 1, 1, 1]], dtype=torch.int32)
    near = {"id": torch.tensor([5]), "voxels": torch.tensor([8]), "partners": torch.tensor([2]),
            "nearest_id": torch.tensor([9]), "nearest_gap": torch.tensor([1.5], dtype=torch.float64),
            "near_voxels": torch.tensor([6]), "near_fraction": torch.tensor([0.75], dtype=torch.float64)}
    plain = CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4))
    got = CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), near_table=near)
    a, b = plain.splitlines(), got.splitlines()
    assert a[:2] == b[:2] and b[2] == a[2] + "," + CMP.NEAR_COLUMNS and b[3] == a[3] + ",2,9,1.5,6,0.75" and len(b) == 4
    assert CMP.NEAR_COLUMNS == "near_partners,nearest_id,nearest_gap,near_voxels,near_fraction"
    both = CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), parent_table=(torch.tensor([12]), torch.tensor([0.625])),
                          near_table=near)
    assert both.splitlines()[3] == a[3] + ",12,0.625,2,9,1.5,6,0.75"
    none = dict(near, nearest_id=torch.tensor([0]), nearest_gap=torch.tensor([math.inf], dtype=torch.float64))
    assert CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), near_table=none).splitlines()[3] == a[3] + ",2,0,inf,6,0.75"
    with pytest.raises(ValueError, match="near_table"):
        CMP.format_csv("m.tif", [5], sums, boxes, (4, 4, 4), near_table={k: torch.cat((v, v)) for k, v in near.items()})


def test_compare_parse_args_of_the_near_switches():
    from skoots_amd.validate.compare import parse_args
    args = parse_args(["m.tif"])
    assert args.near is None and args.near_distance is None
    args = parse_args(["m.tif", "--near", "self", "--near-distance", "2.5"])
    assert args.near == "self" and args.near_distance == 2.5
    assert parse_args(["m.tif", "--near", "er.tif", "--near-distance", "0"]).near == "er.tif"
    for bad in (["m.tif", "--near", "self"], ["m.tif", "--near-distance", "2"],
                ["m.tif", "--near", "self", "--near-distance", "-1"], ["m.tif", "--near", "self", "--near-distance", "inf"],
                ["m.tif", "--near", "self", "--near-distance", "nan"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


# ---- the entry point without a device ----

def test_abi_and_argument_refusals():
    from skoots_amd import _ffi
    L = _ffi.lib
    assert L.sk_abi_version() >= 29 and L.sk_instance_proximity_row_values() == 4
    assert L.sk_instance_proximity_workspace_bytes(0) == 0 and L.sk_instance_proximity_workspace_bytes(48) == 0
    assert L.sk_instance_proximity_workspace_bytes(64) == 64 * 3 * 8

    out = np.full(8, -7, np.int32)
    assert L.sk_instance_proximity_reach(1.0, 1.0, 9.0, 9.0, out.ctypes.data) == 0
    assert out[:4].tolist() == [3, 3, 1, 1] and 0 < out[4] <= 80 * 1024     # two windows fit a CU:
    assert out[5:].tolist() == [2, 512, 0]                                   # 512 threads, and two of them resident
    assert L.sk_instance_proximity_reach(1.0, 1.0, 1.0, 0.0, out.ctypes.data) == 0
    assert out[:4].tolist() == [0, 0, 0, 1] and 160 * 1024 // out[4] > 2    # LDS would allow more; the registers do not
    assert out[5:].tolist() == [2, 512, 0]
    assert L.sk_instance_proximity_reach(1.0, 1.0, 1.0, 25.0, out.ctypes.data) == 0
    assert out[:4].tolist() == [5, 5, 5, 1] and 80 * 1024 < out[4] <= 160 * 1024   # every reach up to 5 is taken
    assert out[5:].tolist() == [1, 1024, 0]
    assert L.sk_instance_proximity_reach(1.0, 1.0, 1.0, 1e6, out.ctypes.data) == 0
    assert out.tolist() == [1000, 1000, 1000, 0, 0, 0, 0, 0]
    assert L.sk_instance_proximity_reach(1.0, 0.0, 1.0, 1.0, out.ctypes.data) == -1
    assert L.sk_instance_proximity_reach(1.0, 1.0, 1.0, float("inf"), out.ctypes.data) == -1
    assert L.sk_instance_proximity_reach(1.0, 1.0, 1.0, 1.0, None) == -1

    p8, p4 = 4096, 4100                                   # aligned to 8, and to 4 only: never dereferenced

    def call(X=4, Y=4, Z=4, max_a=1, N=1, max_b=1, M=1, w=(1.0, 1.0, 1.0), limit2=1.0, same=0, capacity=16, nbytes=None,
             a=p8, lut_a=p8, b=p8, lut_b=p8, rows=p8, counts=p8, work=p8):
        nbytes = 16 * 3 * 8 if nbytes is None else nbytes
        return L.sk_instance_proximity(a, X, Y, Z, lut_a, max_a, N, b, lut_b, max_b, M, *w, limit2, same, rows, capacity,
                                       counts, work, nbytes, None)

    for kw, word in (({"X": -1}, "negative"), ({"N": -1}, "negative"), ({"max_b": -1}, "negative"), ({"M": -2}, "negative"),
                     ({"X": 2 ** 21, "Y": 2 ** 21, "Z": 2 ** 21}, "2^62"),
                     ({"w": (1.0, 0.0, 1.0)}, "weights"), ({"w": (1.0, float("inf"), 1.0)}, "weights"),
                     ({"w": (float("nan"), 1.0, 1.0)}, "weights"),
                     ({"limit2": -1.0}, "limit2"), ({"limit2": float("nan")}, "limit2"), ({"limit2": float("inf")}, "limit2"),
                     ({"same": 2}, "exclude_same"), ({"same": -1}, "exclude_same"),
                     ({"limit2": 49.0}, "beyond what the kernel stages"), ({"limit2": 1e12}, "not truncated"),
                     ({"capacity": 0}, "power of two"), ({"capacity": 24}, "power of two"), ({"capacity": 2 ** 41}, "power"),
                     ({"nbytes": 16 * 3 * 8 - 1}, "workspace too small"),
                     ({"rows": None}, "NULL"), ({"counts": None}, "NULL"), ({"work": None}, "NULL"),
                     ({"rows": p4}, "aligned"), ({"counts": p4}, "aligned"),
                     ({"a": None}, "NULL"), ({"lut_b": None}, "NULL"), ({"b": 4098}, "aligned"), ({"lut_a": 4097}, "aligned")):
        assert call(**kw) == -1, kw
        assert word in _ffi.last_error(), (kw, _ffi.last_error())
