"""CPU tests of the neck cut: the numpy oracle of tests/split_cases.py on hand-made cases whose
answer is written out here, the pure ``plan_split`` of skoots_amd/utils/split.py on hand-written tables and against the
restatement, and every refusal that is decided before the device is touched.  No GPU."""
import numpy as np
import pytest
import torch

from skoots_amd.utils import split as SP
from tests import split_cases as SC


def test_oracle_corridor_with_two_seeds():
    m = np.ones((1, 1, 9), np.int32)
    s = np.zeros_like(m)
    s[0, 0, 1], s[0, 0, 6] = 8, 3
    owner, cost, _ = SC.ref_geodesic(m, s, (1, 1, 2))
    assert owner[0, 0].tolist() == [8, 8, 8, 8, 3, 3, 3, 3, 3]      # z = 3: cost 4 from 8, 6 from 3
    assert cost[0, 0].tolist() == [2, 0, 2, 4, 4, 2, 0, 2, 4]


def test_oracle_tie_goes_to_the_smaller_seed():
    m = np.ones((5, 1, 1), np.int32)
    s = np.zeros_like(m)
    s[0, 0, 0], s[4, 0, 0] = 9, 4
    owner, cost, _ = SC.ref_geodesic(m, s)
    assert owner[:, 0, 0].tolist() == [9, 9, 4, 4, 4] and cost[:, 0, 0].tolist() == [0, 1, 2, 1, 0]
    owner, _, _ = SC.ref_geodesic(m, np.where(s == 9, 2, s))
    assert owner[:, 0, 0].tolist() == [2, 2, 2, 4, 4]


def test_oracle_wall_of_another_id_leaves_the_voxel_unreached():
    m = np.array([1, 1, 2, 1, 0, 1], np.int32).reshape(1, 6, 1)
    s = np.zeros_like(m)
    s[0, 0, 0] = 5
    owner, cost, _ = SC.ref_geodesic(m, s, (1, 7, 1))
    assert owner[0, :, 0].tolist() == [5, 5, 0, 0, 0, 0] and cost[0, :, 0].tolist() == [0, 7, -1, -1, -1, -1]


def test_oracle_seed_on_background_and_max_cost():
    m = np.ones((1, 1, 8), np.int32)
    m[0, 0, 7] = 0
    s = np.zeros_like(m)
    s[0, 0, 0], s[0, 0, 7] = 2, 1            # the seed 1 lies on the background: it seeds nothing
    owner, cost, _ = SC.ref_geodesic(m, s, max_cost=3)
    assert owner[0, 0].tolist() == [2, 2, 2, 2, 0, 0, 0, 0] and cost[0, 0].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]


def test_oracle_u_shape_of_the_issue():
    """nearest by straight line cuts id 5 in two; along paths inside the instance both owners are one piece"""
    m, s, costs = SC.issue_u_shape()
    owner, cost, sweeps = SC.ref_geodesic(m, s, costs)
    assert (owner > 0).sum() == (m > 0).sum() == 6680 and set(np.unique(owner)) == {0, 5, 9}
    assert SC.pieces_of(owner, 5) == 1 and SC.pieces_of(owner, 9) == 1
    x, y, z = np.indices(m.shape)
    d5 = (x - 4) ** 2 + (y - 6) ** 2 + 9 * (z - 4) ** 2
    d9 = (x - 4) ** 2 + (y - 6) ** 2 + 9 * (z - 50) ** 2
    straight = np.where(m > 0, np.where(d5 <= d9, 5, 9), 0)
    assert SC.pieces_of(straight, 5) == 2 and int(((straight != owner) & (m > 0)).sum()) == 1300
    assert cost[4, 6, 4] == 0 and cost[4, 18, 4] == 3 * 56 + 12 + 3 * 10      # round the bend from the seed 9


def test_corridor_crossing_one_face_is_one_path():
    m, s = SC.corridor_crossing_one_face()
    owner, cost, _ = SC.ref_geodesic(m, s)
    assert SC.pieces_of(m, 4) == 1 and ((owner == 7) == (m > 0)).all()
    assert cost.max() == (m > 0).sum() - 1                                     # one voxel wide: the path is the corridor


def table_of(rows):
    """(value, voxels, first_voxel) -> the six columns of label_components"""
    return np.array([[v, n, f, 0, 0, 0] for v, n, f in rows], np.int64).reshape(-1, 6)


def test_plan_split_ordering_and_new_ids():
    #                  id voxels first         piece
    t = table_of([(7, 10, 0),              # 1   id 7: second largest -> new id
                  (3, 5, 4),               # 2   id 3: tie on voxels, first voxel first -> keeps 3
                  (7, 30, 9),              # 3   id 7: the largest keeps 7
                  (3, 5, 11),              # 4   id 3: tie, later -> new id
                  (7, 2, 20),              # 5   id 7: the smallest -> new id
                  (9, 50, 30)])            # 6   id 9: one core, left alone
    lut, f = SP.plan_split(t, [3, 7, 9], 9)
    # new ids over the ids ascending: id 3's second core first, then id 7's in order of size
    assert lut.tolist() == [0, 11, 3, 7, 10, 12, 0]
    assert f == dict(instances_in=3, instances_split=2, cores_found=6, cores_dropped=0, instances_out=6)


def test_plan_split_min_seed_voxels_and_only_ids():
    t = table_of([(7, 10, 0), (3, 5, 4), (7, 30, 9), (3, 5, 11), (7, 2, 20), (9, 50, 30)])
    lut, f = SP.plan_split(t, [3, 7, 9], 9, min_seed_voxels=3)
    assert lut.tolist() == [0, 11, 3, 7, 10, 0, 0] and f["cores_dropped"] == 1 and f["instances_out"] == 5
    lut, f = SP.plan_split(t, [3, 7, 9], 9, min_seed_voxels=6)        # id 3 loses both cores, id 7 keeps two
    assert lut.tolist() == [0, 10, 0, 7, 0, 0, 0] and f["cores_dropped"] == 3 and f["instances_split"] == 1
    lut, f = SP.plan_split(t, [3, 7, 9], 9, min_seed_voxels=11)       # one core left of id 7: nothing to split
    assert not lut.any() and f["instances_split"] == 0 and f["instances_out"] == 3 and f["cores_dropped"] == 4
    lut, f = SP.plan_split(t, [3, 7, 9], 9, only_ids=[3, 9])
    assert lut.tolist() == [0, 0, 3, 0, 10, 0, 0] and f["instances_split"] == 1 and f["cores_dropped"] == 0
    lut, f = SP.plan_split(t, [3, 7, 9], 9, only_ids=[])
    assert not lut.any() and f["instances_out"] == 3
    with pytest.raises(ValueError, match="not in the mask"):
        SP.plan_split(t, [3, 7, 9], 9, only_ids=[3, 8])


def test_plan_split_empty_and_torch_tables():
    lut, f = SP.plan_split(np.zeros((0, 6), np.int64), [4], 4)
    assert lut.tolist() == [0] and f == dict(instances_in=1, instances_split=0, cores_found=0, cores_dropped=0,
                                              instances_out=1)
    t = torch.from_numpy(table_of([(2, 4, 0), (2, 4, 9)]))
    lut, f = SP.plan_split(t, torch.tensor([2]), 2)
    assert lut.tolist() == [0, 2, 3] and f["instances_out"] == 2


def test_plan_split_int32_overflow():
    top = 2 ** 31 - 1
    t = table_of([(top, 4, 0), (top, 3, 9)])
    with pytest.raises(ValueError, match="beyond int32"):
        SP.plan_split(t, [top], top)
    lut, _ = SP.plan_split(t, [top], top, renumber=True)
    assert lut.tolist() == [0, top, top + 1]
    lut, _ = SP.plan_split(table_of([(top, 4, 0)]), [top], top)       # nothing new is needed: no overflow
    assert not lut.any()


@pytest.mark.parametrize("bad", [dict(min_seed_voxels=0), dict(min_seed_voxels=2.5), dict(min_seed_voxels=True),
                                 dict(only_ids=[0]), dict(only_ids=[1.5]), dict(only_ids=[[1, 2]])])
def test_plan_split_refuses(bad):
    with pytest.raises(ValueError):
        SP.plan_split(table_of([(2, 4, 0)]), [2], 2, **bad)
    with pytest.raises(ValueError, match="positive values"):
        SP.plan_split(table_of([(0, 4, 0)]), [2], 2)


@pytest.mark.parametrize("name", ("dumbbell", "blobs"))
def test_plan_split_agrees_with_the_restatement(name):
    """the table of the restatement's cores through plan_split gives the restatement's seeds and report"""
    m = SC.dumbbell() if name == "dumbbell" else SC.blobs_some_fused()
    cores = sorted(SC.ref_cores(m, 3.5), key=lambda c: c[2])                   # label_components numbers by first voxel
    ids = np.unique(m[m > 0])
    lut, f = SP.plan_split(table_of([c[:3] for c in cores]), ids, int(ids.max()))
    seeds = np.zeros(m.size, np.int64)
    for k, c in enumerate(cores):
        seeds[c[3]] = lut[k + 1]
    owner, _, _ = SC.ref_geodesic(m, seeds.reshape(m.shape))
    out = np.where(owner > 0, owner, m)
    want, rep = SC.ref_split(m, 3.5)
    assert np.array_equal(out, want)
    assert f == {k: rep[k] for k in f}
    assert rep["instances_split"] == (1 if name == "dumbbell" else 2)
    for u in np.unique(want[want > 0]):
        assert SC.pieces_of(want, u) == 1


def test_dumbbell_is_cut_and_the_larger_side_keeps_the_id():
    m = SC.dumbbell()
    out, rep = SC.ref_split(m, 3.5)
    assert rep == dict(instances_in=1, instances_split=1, cores_found=2, cores_dropped=0, instances_out=2,
                       voxels_relabelled=int((out == 7).sum()))
    assert set(np.unique(out)) == {0, 6, 7} and np.array_equal(out > 0, m > 0)
    assert (out[:, :, 30:] == 6).sum() > 0 and (out[:, :, 30:] == 7).sum() == 0     # the ball of radius 7 keeps id 6
    assert (out[:, :, :12] == 6).sum() == 0
    assert SC.ref_split(m, 1.5)[1]["instances_split"] == 0                      # below the neck's radius: one core
    assert SC.ref_split(m, 9)[1]["cores_found"] == 0                            # above the balls': none


def test_costs_default_to_an_integral_spacing():
    assert SP.split_costs(None, (1, 1, 3)) == (1, 1, 3) and SP.split_costs(None, (2.0, 2.0, 5.0)) == (2, 2, 5)
    assert SP.split_costs((1, 2, 3), (0.3, 0.3, 1.1)) == (1, 2, 3)
    with pytest.raises(ValueError, match="costs"):
        SP.split_costs(None, (0.3, 0.3, 1.0))
    with pytest.raises(ValueError, match="costs"):
        SP.split_costs(None, (1, 1, 300))
    for bad in ((1, 1), (0, 1, 1), (1, 256, 1), (1.0, 1, 1), (True, 1, 1), "abc", 3):
        with pytest.raises(ValueError, match="costs"):
            SP.split_costs(bad, (1, 1, 1))


def test_geodesic_guards_before_the_device():
    from skoots_amd.lib import morphology as M
    M.check_geodesic_shape((1024, 1024, 256), (1, 1, 3))
    with pytest.raises(ValueError, match="2\\^31"):
        M.check_geodesic_shape((1024, 1024, 256), (1, 1, 8))
    with pytest.raises(ValueError, match="2\\^31"):
        M.check_geodesic_shape((2048, 1024, 1024))
    assert M.geodesic_max_cost(None) == -1 and M.geodesic_max_cost(7) == 7 and M.geodesic_max_cost(2 ** 40) == 2 ** 31 - 1
    for bad in (-1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="max_cost"):
            M.geodesic_max_cost(bad)
    assert M.geodesic_tiles((11, 19, 150)) == 3 * 3 * 3 and M.geodesic_tiles((1, 1, 1)) == 1
    assert M.geodesic_round_bound((11, 19, 150)) == 11 * 19 * 150 + 1
    # a tensor that is not on the device is refused before anything else is looked at
    with pytest.raises(ValueError, match="MI355X"):
        M.geodesic_assign(torch.zeros((2, 2, 2), dtype=torch.int32), torch.zeros((2, 2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="costs"):
        M.geodesic_assign(torch.zeros((2, 2, 2), dtype=torch.int32), torch.zeros((2, 2, 2), dtype=torch.int32), costs=(0, 1, 1))


def test_split_refuses_before_the_device():
    cpu = torch.zeros((2, 2, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="MI355X"):
        SP.split(cpu, 2.0)
    for bad in (None, -1.0, float("inf"), float("nan"), "2", True):
        with pytest.raises(ValueError, match="radius"):
            SP._radius2(bad)
    assert SP._radius2(2.5) == 6.25 and SP._radius2(0) == 0.0


@pytest.mark.parametrize("argv", [["m.tif"], ["m.tif", "--radius", "-1"], ["m.tif", "--radius", "inf"],
                                  ["m.tif", "--radius", "2", "--min-seed-voxels", "0"],
                                  ["m.tif", "--radius", "2", "--costs", "1", "1"],
                                  ["m.tif", "--radius", "2", "--costs", "1", "1", "0"],
                                  ["m.tif", "--radius", "2", "--costs", "1", "1", "1.5"],
                                  ["m.tif", "--radius", "2", "--ids", "0"]])
def test_command_argument_errors(argv, capsys):
    with pytest.raises(SystemExit):
        SP.parse_args(argv)
    capsys.readouterr()


def test_command_arguments():
    a = SP.parse_args(["m.tif", "--radius", "3.5", "--spacing", "1", "1", "3", "--closed", "--min-seed-voxels", "4",
                       "--costs", "1", "1", "3", "--ids", "5", "9", "--renumber", "-o"])
    assert (a.mask, a.radius, tuple(a.spacing), a.closed, a.min_seed_voxels, a.costs, a.ids, a.renumber, a.overwrite) == \
        ("m.tif", 3.5, (1.0, 1.0, 3.0), True, 4, [1, 1, 3], [5, 9], True, True)
    a = SP.parse_args(["m.tif", "--radius", "2"])
    assert (tuple(a.spacing), a.closed, a.min_seed_voxels, a.costs, a.ids, a.renumber, a.overwrite) == \
        ((1.0, 1.0, 1.0), False, 1, None, None, False, False)
    with pytest.raises(FileNotFoundError):
        SP.main(["/nonexistent/m.tif", "--radius", "2"])
