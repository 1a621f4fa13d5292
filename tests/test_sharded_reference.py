"""CPU tests of what the sharded GPU tests (tests/test_hip_sharded_kernels.py) stand on: the numpy / scipy reference
of the Z-sharded labelling, the preconditions its inputs are built to meet, and the in-process communicator."""
import threading
import time

import numpy as np
import pytest
import torch

from tests import sharded_reference as R
from tests.inproc_comm import run_ranks


def test_constants_restate_the_projects():
    from skoots_amd import parallel as P
    from skoots_amd.lib import flood_fill as F
    assert R.HALO == P.HALO and R.PAIR_CAP == F.PAIR_CAP
    for Z, world in ((256, 8), (90, 3), (128, 2), (512, 8)):
        assert R.slab_bounds(Z, world) == P.slab_bounds(Z, world)
        assert [R.window_of(s, Z, world) for s in R.slab_bounds(Z, world)] == \
               [P.window_of(s, Z, world) for s in P.slab_bounds(Z, world)]
    # label_slab's foreground capacity at the sizes of these cases
    for name, (_, worlds) in R.CASES.items():
        X, Y, Z = R.case_mask(name).shape
        for world in worlds:
            zmax = max(b - a for a, b in R.slab_bounds(Z, world))
            assert max(1 << 16, X * Y * zmax // F.NNZ_DIV) == R.NNZ_CAP


@pytest.mark.parametrize("name,world", R.CASE_IDS)
def test_reference_procedure_and_preconditions(name, world):
    mask = R.case_mask(name)
    whole, counts = R.case_reference(name, world)
    merged, counts2, runs, fg = R.merge_slabs(mask, world)
    # (a) slab labels + prefix-sum offsets + union over the seam pairs IS the whole-volume partition
    assert counts == counts2
    assert R.partition_equal(merged, whole)
    assert sum(counts) > int(whole.max())      # something does merge across a boundary
    # (b) capacities, from the reference alone
    assert len(runs) == world - 1 and max(runs) <= R.PAIR_CAP
    assert max(runs) > 8                       # the PAIR_CAP = 8 test overflows
    if name in R.FG_OVERFLOW:
        assert max(fg) > R.NNZ_CAP
    else:
        assert max(fg) <= R.NNZ_CAP
    # (c) every rank's crop is mask-driven: z0 % 16 == d % 16 == window % 16 == 0
    if name in R.GENERIC_PATH:
        assert not any(R.mask_driven(mask.shape[2], world))
    else:
        assert all(R.mask_driven(mask.shape[2], world))
        slabs = R.slab_bounds(mask.shape[2], world)
        assert any(lo - R.window_of((lo, hi), mask.shape[2], world)[0] == 48 for lo, hi in slabs)   # z0 = 48 occurs


def test_serpentine_is_connected_only_through_the_end_ranks():
    mask = R.case_mask("serpentine")
    whole, counts = R.case_reference("serpentine", 8)
    assert int(whole.max()) == 16 + 8                    # one snake per row + one more per broken bar
    assert all(c >= 256 for c in counts[1:-1])           # a middle rank sees every bar on its own
    assert counts[0] < 256 and counts[-1] < 256
    whole3, counts3 = R.case_reference("serpentine_generic", 3)
    assert int(whole3.max()) == 10 + 3 and counts3[1] >= 90


def test_hollow_field_has_empty_ranks_between_non_empty_ones():
    _, counts = R.case_reference("hollow", 8)
    assert counts[3:7] == [0, 0, 0, 0] and counts[2] > 0 and counts[7] > 0


def test_partition_equal_and_seam_helpers():
    ref = np.array([[[0, 1, 1, 0, 2, 2]]])
    assert R.partition_equal(np.array([[[0, 7, 7, 0, 3, 3]]]), ref)
    assert not R.partition_equal(np.array([[[0, 7, 7, 0, 7, 7]]]), ref)      # merged
    assert not R.partition_equal(np.array([[[0, 7, 8, 0, 3, 3]]]), ref)      # split
    assert not R.partition_equal(np.array([[[1, 7, 7, 0, 3, 3]]]), ref)      # background labelled
    lab = np.zeros((2, 3, 4), dtype=np.int32)
    lab[0, 1, :] = [5, 5, 0, 6]
    lab[1, 1, :] = [9, 9, 9, 9]
    assert R.seam_pair_set(lab, 0, 1) == {(9, 5), (9, 6)}
    assert R.seam_adjacent(lab, 0, 1) == 3 and R.seam_runs(lab, 0, 1) == 2
    assert R.min_of_component(7, [(5, 6), (2, 6), (3, 4)]).tolist() == [0, 1, 2, 3, 3, 2, 2]


# ----------------------------------------------------------------------------- ThreadComm on CPU tensors
def test_thread_comm_collectives():
    world = 4

    def body(comm):
        r = comm.rank
        parts = comm.all_gather(torch.full((3,), r, dtype=torch.int32), what="g")
        red = comm.all_reduce_min(torch.tensor([r + 10, 100 - r, 7], dtype=torch.int64), what="m")
        # ring: every rank sends to the next one, the last to the first; two messages to check their order
        nxt, prv = (r + 1) % world, (r - 1) % world
        got = comm.exchange([(nxt, torch.tensor([r, 1])), (nxt, torch.tensor([r, 2]))],
                            [(prv, torch.empty(2, dtype=torch.int64)), (prv, torch.empty(2, dtype=torch.int64))], what="ring")
        return [p.tolist() for p in parts], red.tolist(), [g.tolist() for g in got], dict(comm.calls)

    for r, (parts, red, got, calls) in enumerate(run_ranks(world, body, timeout=20)):
        assert parts == [[q] * 3 for q in range(world)]
        assert red == [10, 100 - (world - 1), 7]
        assert got == [[(r - 1) % world, 1], [(r - 1) % world, 2]]
        assert calls == {"g": 1, "m": 1, "ring": 1}


def test_thread_comm_single_rank_is_the_identity():
    def body(comm):
        t = torch.arange(4)
        return comm.all_gather(t)[0] is t and comm.all_reduce_min(t) is t and comm.exchange([], []) == []

    assert run_ranks(1, body, timeout=5) == [True]


def test_thread_comm_exception_in_one_rank_surfaces_in_the_driver():
    def body(comm):
        if comm.rank == 2:
            raise ZeroDivisionError("rank 2 fails")
        comm.all_gather(torch.zeros(1), what="never_completes")
        return True

    t0 = time.monotonic()
    with pytest.raises(ZeroDivisionError, match="rank 2 fails"):
        run_ranks(4, body, timeout=20)
    assert time.monotonic() - t0 < 10       # the other ranks were released by the aborted barrier, not by the timeout
    assert not [t for t in threading.enumerate() if t.name.startswith("rank")]


def test_thread_comm_mismatched_collectives_are_an_error():
    def body(comm):
        return comm.all_gather(torch.zeros(1), what="a" if comm.rank else "b")

    with pytest.raises(RuntimeError, match="different collectives"):
        run_ranks(2, body, timeout=10)
