"""The mask pairs and the numpy oracle that tests/test_surface_distance_cpu.py, tests/test_hip_compare.py and
tools/surface_distance_host_check.py share (numpy only).

The definitions (include/skoots_hip.h: sk_instance_surface_count, sk_surface_distances).  ``r(v)``
is the row of voxel v (1 .. N, 0 for background and outside the volume).  A surface voxel of row a is a voxel of row a
with a face neighbour of another row; its key is ``(a - 1) X Y Z + ((x Y + y) Z + z)``.  With
``(wx, wy, wz) = (fl(sx sx), fl(sy sy), fl(sz sz))``

    D2(q, T) = min over t in T of  fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),

every square an exact integer, every product and sum rounded once.  Here the surfaces come from shifted comparisons on
the padded row volume and D2 from chunked brute force, one term per pair of voxels, exactly as written.
"""
import functools
import math

import numpy as np

from tests.edt_cases import INTEGER_SPACINGS, SPACINGS, rows_of, weights  # noqa: F401  (re-exported)

IOU_THRESHOLD = 0.1
COLUMNS = ("gt_id", "pred_id", "iou", "dice", "intersection_voxels", "gt_voxels", "pred_voxels", "volume_difference",
           "centroid_distance", "gt_surface_voxels", "pred_surface_voxels", "hausdorff", "hausdorff95", "assd", "nsd",
           "pred_shared")
UNMATCHED = ("unmatched_pred_id", "unmatched_pred_best_iou", "unmatched_pred_voxels", "unmatched_pred_surface_voxels")
SHIFTED, CONCENTRIC, IDENTICAL, TWO_TO_ONE, UNMATCHED_CASE, TIE, HUGE, BALL = (
    "box shifted by (2, 0, 0) (12, 9, 8)", "concentric boxes (11, 11, 11)", "identical (10, 12, 14)",
    "two to one (10, 10, 12)", "unmatched (12, 10, 8)", "tie (4, 4, 8)", "ids 2^31 - 1 and 2^40 (8, 8, 8)",
    "ball (30, 30, 30)")


def cases():
    """name -> (ground truth, prediction), two (X, Y, Z) integer arrays of one shape"""
    out = {}
    g = np.zeros((10, 12, 14), np.int32)
    g[1:5, 2:9, 3:11], g[6:9, 1:4, 1:13], g[7, 8, 9] = 3, 7, 12
    out[IDENTICAL] = (g, g.copy())
    g, p = np.zeros((12, 9, 8), np.int32), np.zeros((12, 9, 8), np.int32)
    g[2:7, 2:7, 2:6], p[4:9, 2:7, 2:6] = 1, 5
    out[SHIFTED] = (g, p)
    g, p = np.zeros((11, 11, 11), np.int32), np.zeros((11, 11, 11), np.int32)
    g[2:9, 2:9, 2:9], p[3:8, 3:8, 3:8] = 2, 2
    out[CONCENTRIC] = (g, p)
    g, p = np.zeros((5, 6, 7), np.int32), np.zeros((5, 6, 7), np.int32)   # one-voxel instances: found, beside, missed
    g[0, 0, 0], g[2, 3, 4], g[4, 5, 6], g[1, 1, 5] = 1, 2, 3, 4
    p[0, 0, 0], p[2, 3, 5], p[4, 5, 6], p[3, 0, 2] = 9, 8, 7, 6
    out["one-voxel instances (5, 6, 7)"] = (g, p)
    for shape in ((1, 17, 9), (13, 1, 1)):                             # extents of 1
        g = np.random.default_rng(sum(shape)).integers(0, 3, shape).astype(np.int32) * 4
        p = np.where(np.random.default_rng(7).random(shape) < 0.2, 0, g).astype(np.int32)
        out[f"random {shape}"] = (g, p)
    g, p = np.full((6, 5, 4), 9, np.int32), np.full((6, 5, 4), 4, np.int32)   # a surface only because outside is row 0
    p[4:] = 0
    out["filling the volume (6, 5, 4)"] = (g, p)
    g, p = np.zeros((9, 10, 11), np.int32), np.zeros((9, 10, 11), np.int32)
    g[:3, :3, :3], g[-3:, -3:, -3:] = 1, 2
    p[:4, :3, :4], p[-4:, -3:, -2:] = 2, 1
    out["opposite corners (9, 10, 11)"] = (g, p)
    g, p = np.zeros((10, 10, 12), np.int32), np.zeros((10, 10, 12), np.int32)
    g[1:5, 2:8, 2:10], g[5:9, 2:8, 2:10], p[1:9, 2:8, 2:10] = 1, 2, 6
    out[TWO_TO_ONE] = (g, p)
    g, p = np.zeros((12, 10, 8), np.int32), np.zeros((12, 10, 8), np.int32)
    g[1:4, 1:4, 1:4], g[7:11, 5:9, 2:7] = 4, 5                         # 4 has no match; 9 is chosen by nobody
    p[7:11, 5:9, 3:7], p[1:3, 7:9, 5:7] = 3, 9
    p[3, 3, 3] = 11                                                    # IoU 1 / 27 with 4: below the threshold
    out[UNMATCHED_CASE] = (g, p)
    g, p = np.zeros((8, 8, 8), np.int64), np.zeros((8, 8, 8), np.int64)
    g[1:4, 1:4, 1:5], g[4:7, 3:8, 2:7] = 2 ** 31 - 1, 2 ** 40
    p[1:4, 1:4, 2:6], p[4:8, 3:8, 2:7], p[0, 7, 7] = 2 ** 40, 5, 2 ** 31 - 1
    out[HUGE] = (g, p)
    g, p = np.zeros((4, 4, 8), np.int32), np.zeros((4, 4, 8), np.int32)
    g[:, :, 2:6], p[:, :, 2:4], p[:, :, 4:6] = 1, 8, 3                 # IoU 1/2 with both: the lower id, 3
    out[TIE] = (g, p)
    c = np.stack(np.meshgrid(*(np.arange(30),) * 3, indexing="ij"), -1)
    g = (((c - np.array([14, 14, 15])) ** 2).sum(-1) <= 121).astype(np.int32) * 6      # surfaces of two LDS tiles
    p = (((c - np.array([15, 16, 15])) ** 2).sum(-1) <= 100).astype(np.int32) * 2
    p[(c[..., 0] > 20) & (g == 0)] = 0
    out[BALL] = (g, p)
    return out


def surface(rows):
    """(X, Y, Z) bool: the surface voxels, by shifted comparisons on the row volume padded with row 0"""
    rows = np.asarray(rows)
    pad = np.pad(rows, 1)
    inner = (slice(1, -1),) * 3
    out = np.zeros(rows.shape, bool)
    for axis in range(3):
        for shift in (-1, 1):
            out |= np.roll(pad, shift, axis=axis)[inner] != rows
    return out & (rows > 0)


def surface_keys(rows):
    """(counts (N) int64, keys int64 ascending) of a row volume: key = (row - 1) X Y Z + linear voxel index"""
    rows = np.asarray(rows)
    n = int(rows.max(initial=0))
    at = np.flatnonzero(surface(rows).reshape(-1))
    r = rows.reshape(-1)[at]
    keys = np.sort((r - 1) * rows.size + at).astype(np.int64)
    return np.bincount(r, minlength=n + 1)[1:].astype(np.int64), keys


def points(keys, shape):
    """(n, 3) int64 voxel coordinates of surface keys"""
    lin = np.asarray(keys, np.int64) % int(np.prod(shape))
    return np.stack(np.unravel_index(lin, shape), -1).astype(np.int64).reshape(-1, 3)


def brute_d2(q, t, w, chunk=1 << 22):
    """(n) float64: D2 of every point of q ((n, 3) integers) against the set t ((m, 3)); inf for an empty set"""
    wx, wy, wz = w
    q, t = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3)
    out = np.full(q.shape[0], np.inf)
    if t.shape[0] == 0:
        return out
    step = max(1, chunk // t.shape[0])
    for lo in range(0, q.shape[0], step):
        dx, dy, dz = (q[lo:lo + step, None, k] - t[None, :, k] for k in range(3))
        out[lo:lo + step] = (wx * (dx * dx) + (wy * (dy * dy) + wz * (dz * dz))).min(axis=1)
    return out


def synthetic(tile, chunk=256, extent=48, seed=5):
    """Key lists around the kernel's sizes, which need no mask: ``(shape, q_off, q_keys, t_off, t_keys, pairs)``.

    Random distinct voxels of an ``extent``^3 volume.  Query segments of 1, chunk - 1, chunk, chunk + 1 keys (the
    workgroup's queries +- 1) and one of 40 keys that all lie in the planes x <= 1; target segments of tile - 1, tile,
    tile + 1 and 2 tile + 1 keys (the LDS tile +- 1), sorted like real surfaces, one of 4 tile + 3 sorted keys -- for
    the queries at x <= 1 every tile but the first is prunable, for the random ones none is at first -- and one of
    tile + 7 keys in random order, which must give the definition's value all the same.  Every query segment meets every
    target segment, so each target segment is shared by several pairs, and pairs are listed in a scrambled order.
    Segment s carries the row prefix s: only key mod X Y Z is a voxel."""
    rng = np.random.default_rng(seed)
    shape = (extent,) * 3
    V = extent ** 3
    q_sizes = (1, chunk - 1, chunk, chunk + 1)
    t_sizes = (tile - 1, tile, tile + 1, 2 * tile + 1, 4 * tile + 3)
    q = [rng.choice(V, n, replace=False) for n in q_sizes] + [rng.choice(2 * extent * extent, 40, replace=False)]
    t = [np.sort(rng.choice(V, n, replace=False)) for n in t_sizes] + [rng.choice(V, tile + 7, replace=False)]
    q = [np.sort(a) for a in q]

    def pack(segs):
        off = np.concatenate(([0], np.cumsum([a.size for a in segs]))).astype(np.int64)
        return off, np.concatenate([a.astype(np.int64) + k * V for k, a in enumerate(segs)])

    pairs = np.array([(a, b) for a in range(len(q)) for b in range(len(t))], np.int32)
    pairs = pairs[rng.permutation(len(pairs))]
    return (shape, *pack(q), *pack(t), pairs)


def synthetic_wide(seed=11):
    """Key lists in a DECLARED volume of (2^26, 2^26, 4) voxels, X Y Z = 2^54, which need no mask and no memory: the
    kernels decode with 64-bit divisions from X Y Z = 2^32 on, and every extent is the largest the library takes, so the
    largest differences (2^26 - 1, whose square is still exact) occur.  ``(shape, q_off, q_keys, t_off, t_keys, pairs)``
    as ``synthetic``: query segments of 300 voxels at the high end of x and y and of 5 at x < 40; target segments of
    1500 voxels (two LDS tiles) at the high end and of 700 in the middle of x; every query segment meets both."""
    rng = np.random.default_rng(seed)
    E = 1 << 26
    shape = (E, E, 4)
    V = E * E * 4

    def cloud(n, x0):
        x, y, z = x0 + rng.integers(0, 40, n), E - 1 - rng.integers(0, 50, n), rng.integers(0, 4, n)
        return np.unique((x.astype(np.int64) * E + y) * 4 + z)

    q = [cloud(300, E - 40), cloud(5, 0)]
    t = [cloud(1500, E - 40), cloud(700, E // 2)]

    def pack(segs):
        off = np.concatenate(([0], np.cumsum([a.size for a in segs]))).astype(np.int64)
        return off, np.concatenate([a + k * V for k, a in enumerate(segs)])

    pairs = np.array([(1, 0), (0, 0), (0, 1), (1, 1)], np.int32)
    return (shape, *pack(q), *pack(t), pairs)


def pair_d2(shape, q_off, q_keys, t_off, t_keys, pairs, w):
    """(out_offsets (P + 1) int64, d2 float64) of key lists: brute force, pair by pair"""
    out = [brute_d2(points(q_keys[q_off[a]:q_off[a + 1]], shape), points(t_keys[t_off[b]:t_off[b + 1]], shape), w)
           for a, b in np.asarray(pairs).reshape(-1, 2).tolist()]
    off = np.concatenate(([0], np.cumsum([d.size for d in out]))).astype(np.int64)
    return off, np.concatenate(out) if out else np.zeros(0)


def iou_matrix(rows_g, rows_p):
    """(N, M) float32 as sk_mask_iou computes it: float(intersection) / float(union), 0 where they do not touch"""
    n, m = int(rows_g.max(initial=0)), int(rows_p.max(initial=0))
    both = np.bincount((rows_g * (m + 1) + rows_p).reshape(-1), minlength=(n + 1) * (m + 1)).reshape(n + 1, m + 1)
    inter = both[1:, 1:]
    union = both[1:].sum(1)[:, None] + both[:, 1:].sum(0)[None, :] - inter
    iou = np.zeros((n, m), np.float32)
    np.divide(inter.astype(np.float32), union.astype(np.float32), out=iou, where=inter > 0)
    return iou, inter


def match(iou, threshold=IOU_THRESHOLD):
    """(N) int64: the rule, one row at a time -- the first column that holds the row's maximum, if that is > threshold"""
    out = np.full(iou.shape[0], -1, np.int64)
    threshold = np.float32(threshold)                        # the matrix is float32 and is compared as such
    for a in range(iou.shape[0]):
        best, col = -math.inf, -1
        for b in range(iou.shape[1]):
            if iou[a, b] > best:
                best, col = iou[a, b], b
        if col >= 0 and best > threshold:
            out[a] = col
    return out


def nearest_rank(n):
    return -(-95 * n // 100) - 1                             # ceil(0.95 n) - 1 in integers


def summaries(d2_g, d2_p, tolerance2):
    """(hausdorff, hausdorff95, assd, nsd) of one pair from the squared distances of its two directions"""
    dg, dp = np.sqrt(np.sort(d2_g)), np.sqrt(np.sort(d2_p))
    total = 0.0
    sums = []
    for d in (dg, dp):
        total = 0.0
        for v in d.tolist():                                 # left to right over the ascending values
            total += v
        sums.append(total)
    n = dg.size + dp.size
    within = int((d2_g <= tolerance2).sum()) + int((d2_p <= tolerance2).sum())
    return (max(dg[-1], dp[-1]), max(dg[nearest_rank(dg.size)], dp[nearest_rank(dp.size)]), (sums[0] + sums[1]) / n,
            within / n)


def _centroids(rows, spacing):
    n = int(rows.max(initial=0))
    idx = np.argwhere(rows > 0)
    r = rows[rows > 0]
    count = np.bincount(r, minlength=n + 1)[1:].astype(np.float64)
    cen = np.stack([np.bincount(r, weights=idx[:, k], minlength=n + 1)[1:] for k in range(3)], 1)
    return cen / count[:, None] * np.array(spacing, np.float64), count.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _surfaces(name):
    g, p = cases()[name]
    (ids_g, rows_g), (ids_p, rows_p) = rows_of(g), rows_of(p)
    out = (ids_g, rows_g, *surface_keys(rows_g), ids_p, rows_p, *surface_keys(rows_p))
    for a in out:
        a.setflags(write=False)
    return out


def surfaces_of(name):
    """(ids_g, rows_g, counts_g, keys_g, ids_p, rows_p, counts_p, keys_p) of a case, computed once and read-only"""
    return _surfaces(name)


@functools.lru_cache(maxsize=None)
def _expected(name, spacing, threshold, tolerance):
    ids_g, rows_g, counts_g, keys_g, ids_p, rows_p, counts_p, keys_p = _surfaces(name)
    shape = rows_g.shape
    w = weights(spacing)
    tau = max(spacing) if tolerance is None else tolerance
    n, m = ids_g.size, ids_p.size
    iou, inter = iou_matrix(rows_g, rows_p)
    cols = match(iou, threshold)
    off_g = np.concatenate(([0], np.cumsum(counts_g)))
    off_p = np.concatenate(([0], np.cumsum(counts_p)))
    cen_g, vox_g = _centroids(rows_g, spacing)
    cen_p, vox_p = _centroids(rows_p, spacing)
    t = {k: np.zeros(n, np.int64) for k in ("pred_id", "intersection_voxels", "pred_voxels", "pred_surface_voxels",
                                            "pred_shared")}
    t.update({k: np.full(n, np.nan) for k in ("volume_difference", "centroid_distance", "hausdorff", "hausdorff95",
                                              "assd", "nsd")})
    t.update(gt_id=ids_g.copy(), gt_voxels=vox_g, gt_surface_voxels=counts_g.copy())
    pairs, d2 = [], {}
    sx, sy, sz = spacing
    for a in range(n):
        b = int(cols[a])
        if b < 0:
            continue
        pairs.append((a, b))
        sg = points(keys_g[off_g[a]:off_g[a + 1]], shape)
        sp = points(keys_p[off_p[b]:off_p[b + 1]], shape)
        d2[a] = (brute_d2(sg, sp, w), brute_d2(sp, sg, w))
        t["pred_id"][a], t["intersection_voxels"][a], t["pred_voxels"][a] = ids_p[b], inter[a, b], vox_p[b]
        t["pred_surface_voxels"][a], t["pred_shared"][a] = counts_p[b], int((cols == b).sum())
        t["volume_difference"][a] = float(vox_p[b] - vox_g[a]) * (sx * sy * sz)
        d = cen_p[b] - cen_g[a]
        t["centroid_distance"][a] = np.sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]))
        t["hausdorff"][a], t["hausdorff95"][a], t["assd"][a], t["nsd"][a] = summaries(*d2[a], tau * tau)
    i, v = t["intersection_voxels"], t["gt_voxels"] + t["pred_voxels"]
    t["iou"], t["dice"] = i / (v - i).astype(np.float64), (2 * i) / v.astype(np.float64)
    un = np.array([b for b in range(m) if not np.any(cols == b)], np.int64)
    t["unmatched_pred_id"] = ids_p[un]
    t["unmatched_pred_best_iou"] = (iou.max(axis=0)[un] if n else np.zeros(un.size, np.float32)).astype(np.float64)
    t["unmatched_pred_voxels"], t["unmatched_pred_surface_voxels"] = vox_p[un], counts_p[un]
    for a in t.values():
        a.setflags(write=False)
    return {"iou": iou, "match": cols, "pairs": np.array(pairs, np.int64).reshape(-1, 2), "d2": d2, "table": t}


def expected(name, spacing=(1.0, 1.0, 1.0), threshold=IOU_THRESHOLD, tolerance=None):
    """The oracle's results for a case, computed once per process: ``iou`` (N, M) float32, ``match`` (N), ``pairs``
    (K, 2) rows and columns, ``d2`` row -> (ground truth -> prediction, prediction -> ground truth) squared distances in
    key order, and ``table``, the dict of ``compare`` as numpy arrays"""
    return _expected(name, tuple(float(v) for v in spacing), float(threshold), None if tolerance is None else float(tolerance))
