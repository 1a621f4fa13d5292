"""Case volumes and the numpy restatement for ``sk_instance_intensity`` (skoots_amd/csrc/instance_intensity.hip), the image
under every instance.

Definition.  ``r(p)`` is the row of voxel p: the rank 1 .. N of its value among the sorted positive values of the mask,
0 for every value <= 0.  With v(p) the image sample and (x, y, z) the indices of p, row r has

    moments  n, S v, S v^2, S v x, S v y, S v z        summed over the voxels with r(p) = r
    extrema  min v, max v                              INT32_MAX, -1 for a row without voxels
    hist     the voxels per bin min(v >> shift, 255)

The RING of row r is the set of voxels with a mask value <= 0 whose nearest instance, as the nearest-instance transform
decides it within ``distance`` (tests/nearest_label_cases.py restates that, its tie rule included), is r; ``ref_ring``
measures the image over the rings.  Everything is an integer and every sum is formed in int64 or Python integers."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
CROSSING = (11, 19, 150)                # crosses the 4 x 16 x 64 tile at least twice on every axis, with remainders
SMALL_CROSSING = (5, 17, 70)


def rows_of(mask):
    """(rows (X, Y, Z) int64, ids (N) int64 ascending)"""
    v = np.asarray(mask).astype(np.int64)
    ids = np.unique(v[v > 0])
    return np.where(v > 0, np.searchsorted(ids, v) + 1, 0), ids


def _sum_by_row(r, term, n_rows):
    """exact per-row sums of non-negative int64 terms: ``bincount`` adds float64, which is exact while the total stays
    below 2^53; beyond that an unbuffered integer add"""
    if term.size == 0 or int(term.max()) * term.size < 2 ** 53:
        return np.bincount(r, weights=term, minlength=n_rows).astype(np.int64)
    out = np.zeros(n_rows, np.int64)
    np.add.at(out, r, term)
    return out


def table_of_rows(rows, n_rows, image, shift=0, want_hist=True):
    """(moments (N, 6), extrema (N, 2), hist (N, 256) or None), int64, of a row volume (0 = not measured)"""
    rows = np.asarray(rows)
    at = np.flatnonzero(rows.reshape(-1))
    r = rows.reshape(-1)[at].astype(np.int64) - 1
    v = np.asarray(image).reshape(-1)[at].astype(np.int64)
    x, y, z = (c.astype(np.int64) for c in np.unravel_index(at, rows.shape))
    moments = np.stack([_sum_by_row(r, t, n_rows) for t in (np.ones_like(v), v, v * v, v * x, v * y, v * z)], 1)
    extrema = np.empty((n_rows, 2), np.int64)
    extrema[:, 0], extrema[:, 1] = INT32_MAX, -1
    np.minimum.at(extrema[:, 0], r, v)
    np.maximum.at(extrema[:, 1], r, v)
    hist = None
    if want_hist:
        hist = np.bincount(r * 256 + np.minimum(v >> shift, 255), minlength=n_rows * 256).reshape(n_rows, 256)
    return moments, extrema, hist


def ref_intensity(mask, image, shift=0):
    """(moments, extrema, hist) of every positive id of ``mask``, ascending"""
    assert tuple(np.shape(mask)) == tuple(np.shape(image))
    rows, ids = rows_of(mask)
    return table_of_rows(rows, ids.size, image, shift)


def loop_intensity(mask, image, shift=0):
    """the same tables from a plain loop over the voxels, in Python integers"""
    rows, ids = rows_of(mask)
    m = [[0] * 6 for _ in range(ids.size)]
    e = [[INT32_MAX, -1] for _ in range(ids.size)]
    h = [[0] * 256 for _ in range(ids.size)]
    for (x, y, z), r in np.ndenumerate(rows):
        if r:
            v = int(np.asarray(image)[x, y, z])
            for k, t in enumerate((1, v, v * v, v * x, v * y, v * z)):
                m[r - 1][k] += t
            e[r - 1] = [min(e[r - 1][0], v), max(e[r - 1][1], v)]
            h[r - 1][min(v >> shift, 255)] += 1
    return np.array(m, np.int64).reshape(-1, 6), np.array(e, np.int64).reshape(-1, 2), np.array(h, np.int64).reshape(-1, 256)


def ring_rows(mask, distance, spacing):
    """(X, Y, Z) int64: the row whose ring a voxel is in, 0 for instance voxels and for voxels farther than ``distance``
    from every instance"""
    from tests import nearest_label_cases as NL
    rows, _ = rows_of(mask)
    d = float(distance)
    _, near = NL.oracle(rows, NL.weights(spacing), d * d)
    return np.where(np.asarray(mask) <= 0, near, 0)


def ref_ring(mask, image, distance, spacing):
    """(moments (N, 6), extrema (N, 2)) of the image over the ring of every positive id of ``mask``"""
    rows, ids = rows_of(mask)
    return table_of_rows(ring_rows(mask, distance, spacing), ids.size, image, want_hist=False)[:2]


# ---- case volumes ----

def boxes(shape, n, seed, ids=None):
    """n random boxes of up to half the extent per axis (at least 1), painted in order with ``ids`` (default 1 .. n; a
    later box overwrites); a few voxels are set to 0 and to negative values afterwards: both are background"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.int64)
    ids = list(range(1, n + 1)) if ids is None else list(ids)
    for k in range(n):
        ext = [int(rng.integers(1, max(s // 2, 1) + 1)) for s in shape]
        lo = [int(rng.integers(0, s - e + 1)) for s, e in zip(shape, ext)]
        v[tuple(slice(a, a + e) for a, e in zip(lo, ext))] = ids[k % len(ids)]
    holes = rng.random(shape)
    v[holes < 0.05] = 0
    v[holes > 0.97] = -3
    return v


def crossing_blobs(shape, seed, ids=None):
    """``boxes`` plus one box whose z runs go through z = 63 | 64, the seam between two tiles along the lanes"""
    v = boxes(shape, 7, seed, ids)
    X, Y, Z = shape
    assert Z > 66
    v[X // 2:, Y // 3:Y // 3 + 3, 58:min(Z, 69)] = (ids or [9])[-1]
    return v


def voxel_ids(shape):
    """every voxel carries its own id: a tile has thousands of rows, far more than its LDS table holds"""
    return (np.arange(int(np.prod(shape)), dtype=np.int64) + 1).reshape(shape)


def many_ids(shape, k, seed):
    """a random id in 1 .. k per voxel, one voxel in eight zero"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, k + 1, shape)
    v[rng.random(shape) < 0.125] = 0
    return v.astype(np.int64)


def two_balls(shape=(24, 24, 40), radius=5):
    """two balls far enough apart that no voxel within 3 units of one is as near to the other: no ties"""
    g = np.indices(shape)
    v = np.zeros(shape, np.int64)
    for k, c in enumerate(((7, 8, 9), (16, 15, 30))):
        v[sum((g[a] - c[a]) ** 2 for a in range(3)) <= radius * radius] = 5 * (k + 1)
    return v


def noise_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def noise_u16(shape, seed, top=65535):
    """uniform samples in 0 .. top with both ends present"""
    v = np.random.default_rng(seed).integers(0, top + 1, shape).astype(np.uint16)
    flat = v.reshape(-1)
    flat[0], flat[-1] = 0, top
    if flat.size > 2:
        flat[flat.size // 2] = top
        flat[flat.size // 3] = 0
    return v


def ramp(shape, axis):
    """1 + the voxel index along ``axis`` (mod 251): distinguishes the three axes in S v x, S v y, S v z"""
    c = np.arange(shape[axis]).reshape([-1 if k == axis else 1 for k in range(3)])
    return np.broadcast_to((1 + c % 251).astype(np.uint8), shape).copy()
