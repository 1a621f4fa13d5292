"""Hand-built skeletons for the branch tracing, shared by tests/test_skeleton_branches_cpu.py,
tests/test_hip_skeleton_branches.py and tools/skeleton_branches_host_check.py (numpy only).

They are fed to the tracing as they are, without thinning (``sk_skeleton_pack``): most of them are shapes that Lee
thinning would alter.  Every case is a label volume; the closed forms that the cases must give are stated in
tests/test_skeleton_branches_cpu.py."""
import numpy as np

from tests.skeleton_graph_cases import line, lines

ROD_VOXELS = 7
# a ring of ten chain voxels across the word boundary z = 31 | 32, as (y, z): that of tests/test_skeleton_graph_cpu.py
RING_YZ = ((1, 30), (1, 31), (1, 32), (2, 33), (3, 33), (4, 32), (4, 31), (4, 30), (3, 29), (2, 29))


def _plane(shape, yz, x=1, value=1, lab=None):
    lab = np.zeros(shape, np.int32) if lab is None else lab
    for y, z in yz:
        assert lab[x, y, z] == 0
        lab[x, y, z] = value
    return lab


def theta_yz():
    """two junction voxels (5, 2) and (5, 12) joined by three paths: through y = 2, straight, and through y = 8"""
    upper = [(4, 1), (3, 1)] + [(2, z) for z in range(2, 13)] + [(3, 13), (4, 13)]
    lower = [(10 - y, z) for y, z in upper]
    return [(5, 2), (5, 12)] + upper + [(5, z) for z in range(3, 12)] + lower


def lollipop_yz():
    """a stem of four voxels to the junction voxel (5, 4), and a loop that leaves it and comes back to it"""
    return [(5, z) for z in range(4)] + [(5, 4), (4, 5), (3, 6), (3, 7), (4, 8), (5, 9), (6, 8), (7, 7), (7, 6), (6, 5)]


def cases():
    """name -> (X, Y, Z) int32 label volume (int64 where the ids need it)"""
    out = {}
    lab = np.zeros((9, 9, 40), np.int32)
    lab[line((1, 1, 28), (1, 1, 1), ROD_VOXELS)] = 3            # a rod across the word boundary
    lab[line((1, 7, 2), (0, 0, 1), ROD_VOXELS)] = 4
    out["rods"] = lab
    lab = np.zeros((3, 3, 3), np.int32)
    lab[1, 1, 1] = lab[2, 2, 2] = 6
    out["two voxels"] = lab
    lab = np.zeros((3, 3, 3), np.int32)
    lab[0, 2, 1] = 6
    out["one voxel"] = lab
    out["ring of ten"] = _plane((4, 6, 40), RING_YZ, x=2, value=5)
    lab = np.zeros((3, 4, 4), np.int32)
    lab[1, 1, 1] = lab[1, 2, 1] = lab[1, 1, 2] = 6
    out["triangle"] = lab
    # a 6-connected path of 12 voxels that steps aside once: the four voxels round the step are one junction
    out["jog"] = _plane((3, 4, 11), [(1, z) for z in range(6)] + [(2, z) for z in range(5, 11)], value=2)
    # a 6-connected path of 12 voxels with one right-angle corner: the corner voxel has two neighbours and is a corner loop
    out["corner"] = _plane((3, 8, 9), [(y, 1) for y in range(1, 7)] + [(6, z) for z in range(2, 8)], value=2)
    # a line of 12 with a one-voxel spur beside its middle
    out["spur"] = _plane((3, 4, 14), [(1, z) for z in range(1, 13)] + [(2, 6)], value=9)
    out["solid 5"] = np.full((5, 5, 5), 8, np.int32)
    lab = np.zeros((5, 5, 10), np.int32)
    lab[:, :, :5] = 8
    lab[2, 2, 5:] = 8
    out["solid 5 with an arm"] = lab
    out["theta"] = _plane((3, 11, 15), theta_yz(), value=11)
    out["lollipop"] = _plane((3, 9, 11), lollipop_yz(), value=12)
    out["lines"] = lines()                                        # every link class, and two ids touching diagonally
    # one id: two rings, a rod, a pair and a single voxel
    lab = _plane((8, 6, 40), RING_YZ, x=1, value=7)
    _plane(None, RING_YZ, x=5, value=7, lab=lab)
    lab[3, 0, 2:9] = 7
    lab[7, 5, 38] = lab[7, 4, 39] = 7
    lab[7, 0, 0] = 7
    lab[3, 5, 20:24] = 13                                         # and another id between them
    out["rings and pieces"] = lab
    lab = np.zeros((4, 5, 36), np.int64)
    lab[1, 1, 1:35] = 2 ** 40
    lab[3, 3, 30:36] = 2 ** 31 - 1
    lab[3, 0, 0] = 70000
    out["huge ids"] = lab
    for shape in ((1, 1, 9), (6, 1, 1), (1, 7, 1)):
        out[f"extent one {shape}"] = np.full(shape, 4, np.int32)
    return out
