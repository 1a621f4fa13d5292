"""The label volumes that tests/golden/make_skeleton_graph_golden.py, tests/test_skeleton_graph_cpu.py and
tests/test_hip_skeleton_graph.py share (numpy only: the generator's interpreter has no torch).

Every instance of every case is thinned on the whole volume, other ids as background; the golden file holds the
result.  The shapes are small and reach every path of the kernels: rows of one, two and three 32-voxel words,
extents of 1 in every axis, objects on every face and in the corners of the volume, skeletons that are empty, a
single voxel, a rod, a ring and a T, and ids that take the relabel route of ``validate.lib._id_rows``."""
import numpy as np

# (|dx|, |dy|, |dz|) of the link classes, columns 5 .. 11 of sk_skeleton_graph
LINK_CLASSES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
LINE_VOXELS = 9
LINE_IDS = tuple(range(11, 11 + len(LINK_CLASSES)))      # one straight line per link class
PAIR_IDS = (101, 102)                                    # two lines of class (1, 0, 1), diagonally adjacent
RING_ID, T_ID = 7, 8


def blobs(shape, n, seed, id_max=100000, rmax=6.0):
    """the generator of tests/test_hip_surface_area.py (which imports torch), restated"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32)
    g = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1)
    for i in rng.choice(np.arange(1, id_max), n, replace=False):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        rad = rng.uniform(1.5, rmax, 3)
        lab[(((g - c) / rad) ** 2).sum(-1) <= 1] = i
    return lab


def line(start, step, n=LINE_VOXELS):
    return tuple(np.array([[s + t * d for s, d in zip(start, step)] for t in range(n)]).T)


def lines():
    """(11, 98, 40): for every link class a straight digital line of nine voxels (z from 28 on, so the lines with a z
    step cross the word boundary at 32), and two more of different ids that touch diagonally all along"""
    lab = np.zeros((11, 12 * len(LINK_CLASSES) + 14, 40), np.int32)
    for k, step in enumerate(LINK_CLASSES):
        lab[line((1, 12 * k + 1, 28), step)] = LINE_IDS[k]
    y0 = 12 * len(LINK_CLASSES) + 2
    lab[line((1, y0, 28), (1, 0, 1))] = PAIR_IDS[0]
    lab[line((1, y0 + 1, 29), (1, 0, 1))] = PAIR_IDS[1]   # every voxel a (0, 1, 1) neighbour of the other line
    return lab


def cases():
    """name -> (X, Y, Z) int32 array (int64 for the one case whose ids need it)"""
    out = {}
    lab = blobs((24, 40, 70), 30, seed=21, rmax=9.0)      # z = 70: rows of three words
    lab[3:6, 5:25, 5:8] = RING_ID                         # a square ring
    lab[3:6, 5:25, 20:23] = RING_ID
    lab[3:6, 5:8, 5:23] = RING_ID
    lab[3:6, 22:25, 5:23] = RING_ID
    lab[12:15, 2:20, 40:43] = T_ID                        # a T
    lab[12:15, 10:13, 40:60] = T_ID
    out["blobs (24, 40, 70)"] = lab
    out["lines"] = lines()
    for shape in ((1, 1, 70), (5, 1, 1), (3, 70, 1)):
        lab = np.random.default_rng(sum(shape)).integers(0, 4, shape).astype(np.int32) * 7
        lab.flat[0] = 7
        out[f"random {shape}"] = lab
    out["one label (8, 9, 10)"] = np.full((8, 9, 10), 12, np.int32)
    lab = np.zeros((5, 6, 34), np.int32)
    lab[0, 0, 0], lab[4, 5, 33] = 3, 9
    out["corners (5, 6, 34)"] = lab
    lab = np.zeros((9, 11, 37), np.int32)                 # three bars through the centre: touches all six faces
    lab[:, 4:7, 17:20] = 4
    lab[3:6, :, 17:20] = 4
    lab[3:6, 4:7, :] = 4
    out["cross (9, 11, 37)"] = lab
    lab = np.zeros((4, 5, 36), np.int32)                  # max id > 4 * voxels: relabelled, no table of 2^31 entries
    lab[0:3, 0:3, 1:35] = 2 ** 31 - 1
    lab[3, 3:5, 30:36] = 2 ** 30
    lab[3, 0, 0] = 70000
    lab[0, 4, 0] = -9
    out["huge int32 (4, 5, 36)"] = lab
    big = lab.astype(np.int64)
    big[big == 2 ** 31 - 1] = 2 ** 40                     # beyond int32 altogether
    out["huge int64 (4, 5, 36)"] = big
    return out


def positive_ids(lab):
    u = np.unique(lab)
    return u[u > 0].astype(np.int64)
