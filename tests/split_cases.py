"""The numpy oracle of ``geodesic_assign``, a numpy / scipy restatement of the whole ``split``,
and the volumes both are tried on.  No torch, no GPU, nothing of the code under test.

The oracle packs ``cost << 32 | seed`` into int64 and takes the minimum with the six shifted copies where ``labels``
agree, until nothing changes: the relaxation whose unique fixed point defines the result."""
import numpy as np
from scipy import ndimage as ndi

from tests import clean_cases as CC

TILE = (4, 8, 64)                     # the relaxation kernel's tile (x, y, z): the labelling kernel's
CROSSING = CC.CROSSING                # (11, 19, 150): two tiles and a remainder on every axis
NONE = np.int64(2 ** 63 - 1)
REPORT_FIELDS = ("instances_in", "instances_split", "cores_found", "cores_dropped", "instances_out", "voxels_relabelled")


def ref_geodesic(labels, seeds, costs=(1, 1, 1), max_cost=None):
    """(owner int32, cost int32, sweeps): the definition, by relaxation to the fixed point."""
    labels = np.asarray(labels).astype(np.int64)
    seeds = np.asarray(seeds).astype(np.int64)
    assert labels.shape == seeds.shape and labels.ndim == 3
    key = np.where((labels > 0) & (seeds > 0), seeds, NONE)
    limit = None if max_cost is None else np.int64(max_cost)
    sweeps = 0
    while True:
        sweeps += 1
        new = key.copy()
        for axis, c in enumerate(costs):
            if labels.shape[axis] < 2:
                continue
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            same = (labels[lo] == labels[hi]) & (labels[lo] > 0)
            for dst, src in ((hi, lo), (lo, hi)):
                cand = np.where(same & (key[src] != NONE), key[src] + (np.int64(c) << 32), NONE)
                if limit is not None:
                    cand = np.where((cand >> 32) > limit, NONE, cand)
                new[dst] = np.minimum(new[dst], cand)
        if np.array_equal(new, key):
            break
        key = new
    reached = key != NONE
    owner = np.where(reached, key & 0xFFFFFFFF, 0).astype(np.int32)
    cost = np.where(reached, key >> 32, -1).astype(np.int32)
    return owner, cost, sweeps


def pieces_of(owner, value):
    """the 6-connected pieces of ``owner == value``"""
    return int(ndi.label(owner == value)[1])


def ref_edt2(mask, spacing=(1, 1, 1), closed=False):
    """exact squared distance of every instance voxel to the nearest voxel outside its instance, at integer spacings,
    as ``label_edt`` defines it: scipy's transform squared and rounded to the integer it is"""
    mask = np.asarray(mask).astype(np.int64)
    assert all(float(s) == int(s) for s in spacing)
    m = np.pad(mask, 1) if closed else mask
    d2 = np.zeros(m.shape, np.float64)
    for u in np.unique(m[m > 0]):
        inside = m == u
        if inside.all():
            d2[inside] = np.inf
            continue
        d2[inside] = np.rint(ndi.distance_transform_edt(inside, sampling=[float(s) for s in spacing]) ** 2)[inside]
    return d2[1:-1, 1:-1, 1:-1] if closed else d2


def ref_cores(mask, radius, spacing=(1, 1, 1), closed=False):
    """[(id, voxels, first voxel, flat indices)] of the cores of every id at depth ``radius``"""
    mask = np.asarray(mask).astype(np.int64)
    core = ref_edt2(mask, spacing, closed) > float(radius) * float(radius)
    out = []
    for u in np.unique(mask[mask > 0]):
        lab, n = ndi.label((mask == u) & core)
        flat = lab.reshape(-1)
        for k in range(1, n + 1):
            idx = np.flatnonzero(flat == k)
            out.append((int(u), int(idx.size), int(idx[0]), idx))
    return out


def ref_split(mask, radius, spacing=(1, 1, 1), closed=False, min_seed_voxels=1, costs=None, ids=None, renumber=False):
    """(mask_out int64, report dict without ``rounds``) by the eight steps of ``split``, one id at a time."""
    mask = np.asarray(mask).astype(np.int64)
    costs = tuple(int(s) for s in spacing) if costs is None else tuple(costs)
    all_ids = np.unique(mask[mask > 0])
    cores = ref_cores(mask, radius, spacing, closed)
    rep = dict.fromkeys(REPORT_FIELDS, 0)
    rep["instances_in"] = int(all_ids.size)
    rep["cores_found"] = len(cores)
    rep["cores_dropped"] = sum(c[1] < min_seed_voxels for c in cores)
    seeds = np.zeros(mask.size, np.int64)
    nxt = int(all_ids.max()) + 1 if all_ids.size else 1
    for u in all_ids:
        mine = sorted((c for c in cores if c[0] == u and c[1] >= min_seed_voxels), key=lambda c: (-c[1], c[2]))
        if len(mine) < 2 or (ids is not None and int(u) not in set(int(i) for i in ids)):
            continue
        rep["instances_split"] += 1
        for k, c in enumerate(mine):
            if k == 0:
                seeds[c[3]] = u
            else:
                seeds[c[3]] = nxt
                nxt += 1
    seeds = seeds.reshape(mask.shape)
    owner, _, _ = ref_geodesic(mask, seeds, costs)
    out = np.where(owner > 0, owner.astype(np.int64), mask)
    rep["voxels_relabelled"] = int((out != mask).sum())
    rep["instances_out"] = int(np.unique(out[out > 0]).size)
    if renumber:
        flat = out.reshape(-1)
        vals, first = np.unique(flat, return_index=True)
        vals, first = vals[vals > 0], first[vals > 0]
        lut = {int(v): k + 1 for k, v in enumerate(vals[np.argsort(first)])}
        lut[0] = 0
        out = np.vectorize(lut.get, otypes=[np.int64])(out)
    return out, rep


# ---- volumes ----

def issue_u_shape():
    """the U of the issue: two arms along z joined at high z; the straight line from the far end of one arm to the seed in
    the other crosses the gap.  (labels, seeds, costs)"""
    m = np.zeros((9, 30, 70), np.int32)
    m[2:7, 2:12, 2:68] = 1
    m[2:7, 14:24, 2:68] = 1
    m[2:7, 2:24, 60:68] = 1
    s = np.zeros_like(m)
    s[4, 6, 4] = 5
    s[4, 6, 50] = 9
    return m, s, (1, 1, 3)


def corridor_crossing_one_face(turns=9):
    """two tiles along x only ((8, 8, 64) is 2 x 1 x 1 tiles): a one-voxel-wide corridor that goes back and forth across
    the face between them ``turns`` times, seeded at its start.  The tile that holds the front changes with every
    crossing, so the rounds grow with the crossings while the tiles stay two."""
    m = np.zeros((8, 8, 64), np.int32)
    z = 0
    for k in range(turns):
        m[2:6, 3, z] = 4                              # across the face between x = 3 and x = 4
        if k + 1 < turns:
            m[5 if k % 2 == 0 else 2, 3, z:z + 3] = 4   # on to the next crossing, inside one tile
        z += 2
    s = np.zeros_like(m)
    s[2, 3, 0] = 7
    return m, s


def shared_wall(shape=CROSSING):
    """two ids that share a long wall through many tiles, seeds in one of them only"""
    m = np.zeros(shape, np.int32)
    m[:, :9, :] = 3
    m[:, 9:, :] = 8
    s = np.zeros(shape, np.int32)
    s[1, 2, 5] = 11
    s[9, 7, 140] = 12
    return m, s


def seeds_on_tile_borders(shape=CROSSING):
    """one solid id; seeds on a tile face, on a tile edge, in a tile corner (both sides of each) and inside a tile"""
    m = np.full(shape, 2, np.int32)
    s = np.zeros(shape, np.int32)
    s[3, 3, 30] = 21      # x face (x = 3 | 4)
    s[4, 12, 100] = 22    # the other side of an x face
    s[7, 7, 20] = 23      # x-y edge
    s[8, 16, 64] = 24     # corner: first voxel of tile (2, 2, 1)
    s[7, 15, 63] = 25     # corner: last voxel of tile (1, 1, 0)
    s[1, 1, 128] = 26     # z face
    s[5, 10, 90] = 27     # inside
    return m, s


def tie_across_face():
    """a straight corridor along x through the face x = 3 | 4 and one along z through z = 63 | 64, with equidistant seeds
    on both sides: the voxels in the middle tie, and the smaller seed wins"""
    m = np.zeros((8, 8, 128), np.int32)
    m[:, 2, 5] = 1
    m[1, 5, 44:85] = 6
    s = np.zeros_like(m)
    s[0, 2, 5], s[6, 2, 5] = 9, 4          # x = 3 is the middle: cost 3 from both
    s[1, 5, 44], s[1, 5, 84] = 2, 3        # z = 64 is the middle
    return m, s


def noise(shape, seed, ids=(0, 1, 2, 3), seed_rate=0.01, seed_ids=(5, 6, 9, 1000)):
    m = CC.sparse_noise(shape, seed, ids)
    rng = np.random.default_rng(seed + 1000)
    s = np.where(rng.random(shape) < seed_rate, np.asarray(seed_ids, np.int64)[rng.integers(0, len(seed_ids), shape)], 0)
    return m, s


def dense_noise(shape, seed, ids=(3, 7, 300, 2 ** 31 - 1), holes=0.15):
    """mostly foreground, in blocks of 3 x 3 x 5 voxels of one id with holes: paths that are many steps long"""
    rng = np.random.default_rng(seed)
    coarse = np.asarray(ids, np.int64)[rng.integers(0, len(ids), tuple(-(-n // b) for n, b in zip(shape, (3, 3, 5))))]
    m = np.kron(coarse, np.ones((3, 3, 5), np.int64))[:shape[0], :shape[1], :shape[2]]
    m = np.where(rng.random(shape) < holes, 0, m)
    s = np.where(rng.random(shape) < 0.002, rng.integers(1, 2 ** 31 - 1, shape), 0)
    return m, s


def ball(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


def dumbbell(value=6):
    """two balls of radius 7 and 6 joined by a neck of radius 2 along z; the larger ball comes second in raster order"""
    shape = (18, 18, 44)
    m = ball(shape, (9, 9, 8), 6) | ball(shape, (9, 9, 33), 7)
    x, y, z = np.indices(shape)
    m |= ((x - 9) ** 2 + (y - 9) ** 2 <= 4) & (z >= 8) & (z <= 33)
    return (m * value).astype(np.int32)


def blobs_some_fused():
    """five ids: two dumbbells (ids 2 and 40), two plain balls and a thin rod; only the dumbbells split at radius 3.5"""
    m = np.zeros((40, 36, 90), np.int32)
    d = dumbbell(1)
    m[1:19, 1:19, 1:45] = d * 2
    m[20:38, 17:35, 45:89] = d[:, :, ::-1] * 40
    m[21:39, 1:17, 2:20][ball((18, 16, 18), (9, 8, 9), 7)] = 7
    m[2:16, 20:34, 60:76][ball((14, 14, 16), (7, 7, 8), 6)] = 9
    m[30, 5, 30:44] = 12
    return m
