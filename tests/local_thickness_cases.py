"""The label volumes and the numpy statements of the local thickness that tests/test_local_thickness_cpu.py,
tests/test_hip_local_thickness.py and tools/local_thickness_host_check.py share (numpy only).

The definition (include/skoots_hip.h: sk_local_thickness_paint).  ``r(v)`` is the row of voxel v,
``(wx, wy, wz)`` the float64 squares of the spacing, ``D2`` the labelled distance transform of tests/edt_cases.py (open
or closed), and

    d2(p, c) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),

every square an exact integer, every product and sum rounded once, no fused multiply-add.  For a voxel p with r(p) > 0

    T2(p) = max over voxels c of the volume with d2(p, c) < D2(c) of D2(c),

and T2(p) = 0 where r(p) = 0.  The ball is open: the nearest outside voxel of c lies at D2(c) exactly and is not in it.

Two statements of it, which the CPU tests hold against each other bit for bit:

``brute_force``  the maximum as written, one term per pair (p, c) with c running over every voxel of the volume, background
                 included; nothing is pruned and no box is formed.  It also counts the pairs whose voxels are of
                 different rows (there are none: D2(c) is the minimum of the same expression over the other rows).  It
                 costs voxels(foreground) x voxels(volume), so the tests run it on every voxel of the small volumes and
                 on a sample of the voxels of the large ones.
``paint``        the scatter form of the kernel: T2 starts as a copy of D2; every voxel c with a finite D2(c) > 0 raises T2
                 to D2(c) on the voxels p of its clipped bounding box with d2(p, c) < D2(c).  The half-extents come from
                 an exact search (the largest d with w d^2 < D2(c)), never from a square root.  Centres of one value
                 share their offsets, so the loop runs over the distinct values of D2.
"""
import functools

import numpy as np

from tests import edt_cases
from tests.edt_cases import INF, MODES, SPACINGS, rows_of, weights  # noqa: F401  (re-exported for the tests)

HALF = "half (10, 10, 12)"
NECK_345 = "3-4-5 neck (14, 11, 11)"
FORMS = "rounding forms (13, 19, 5)"
TUBE = "tube (24, 9, 9)"
THIN = ("thin x (1, 9, 8)", "thin y (9, 1, 8)", "thin z (9, 8, 1)")
BRUTE_SAMPLE = 300                                         # voxels of a large volume that brute_force is run on
LARGE = 3000                                               # foreground voxels from which a volume counts as large

# The spacing at which w (d d) and (w d) d differ (DESIGN.md section 23 uses the same one), and the pinned voxel: at the
# offset (0, 5, 0) the defined form gives fl(wy 25) = 4.2025 and (wy 5) 5 gives a smaller number.  FORMS is the open
# ball of that squared radius around its centre, so the nearest outside voxel of the centre is (0, -5, 0), at 4.2025
# exactly, and a neck runs through (0, 5, 0), (0, 6, 0), (0, 7, 0): the first neck voxel lies at 4.2025 exactly, outside
# the open ball, and a kernel that forms (w d) d paints it.  (A search over every offset within 20 voxels finds 725
# offsets at which the forms differ; this is the one with the smallest ball in which the wrong form is the smaller.)
FORMS_SPACING = (0.37, 0.41, 1.3)
FORMS_CENTRE = (6, 6, 2)
FORMS_OFFSET = (0, 5, 0)
NECK_345_CENTRE = (5, 5, 5)
NECK_345_OFFSET = (5, 0, 0)


def d2_of(w, dx, dy, dz):
    """fl(wx dx^2 + fl(wy dy^2 + wz dz^2)) of float64 arrays of integer differences"""
    return w[0] * (dx * dx) + (w[1] * (dy * dy) + w[2] * (dz * dz))


def _ball_with_neck(shape, centre, w, D, axis, first, length, value):
    """The voxels with d2(p, centre) < D and a one-voxel neck of ``length`` voxels from offset ``first`` along ``axis``"""
    g = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), -1) - np.array(centre, float)
    lab = (d2_of(w, g[..., 0], g[..., 1], g[..., 2]) < D).astype(np.int32) * value
    at = list(centre)
    for k in range(length):
        at[axis] = centre[axis] + first + k
        lab[tuple(at)] = value
    return lab


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (X, Y, Z) integer array: the volumes of tests/edt_cases.py and the ones where the painting in particular
    can go wrong.  Built once per process; the arrays are read-only."""
    out = dict(edt_cases.cases())
    lab = np.zeros((10, 10, 12), np.int32)                # open mode: balls of up to 8 sz, clipped by five faces
    lab[:, :, :8] = 2
    out[HALF] = lab
    # an open ball of squared radius 25, the nearest outside voxel at (3, 4, 0) among others, and a neck through
    # (5, 0, 0), (6, 0, 0), (7, 0, 0): with <= in place of < the neck voxel at distance exactly 5 would take 25
    out[NECK_345] = _ball_with_neck((14, 11, 11), NECK_345_CENTRE, (1.0, 1.0, 1.0), 25.0, 0, 5, 3, 7)
    w = weights(FORMS_SPACING)
    out[FORMS] = _ball_with_neck((13, 19, 5), FORMS_CENTRE, w, w[1] * 25.0, 1, 5, 3, 3)
    for name, shape in zip(THIN, ((1, 9, 8), (9, 1, 8), (9, 8, 1))):    # an extent of 1 on each axis: two touching ids, a hole
        flat = np.zeros((9, 8), np.int32)
        flat[1:8, 1:4], flat[1:8, 4:7], flat[4, 2] = 4, 11, 0
        out[name] = flat.reshape(shape)
    # a tube along x five voxels across (radius 3: the nearest outside voxel of the axis lies 3 away) with a
    # constriction one voxel across (radius 1) at x = 10 .. 13
    y, z = np.meshgrid(np.arange(9) - 4, np.arange(9) - 4, indexing="ij")
    lab = np.zeros((24, 9, 9), np.int32)
    lab[:] = (y * y + z * z < 9) * 5
    lab[10:14] = 0
    lab[10:14, 4, 4] = 5
    out[TUBE] = lab
    for lab in out.values():
        lab.setflags(write=False)
    return out


def half_extent(D, w, E):
    """the largest d in [0, E] with w d^2 < D (D > 0), by exact search"""
    d = 0
    while d < E and w * (float(d + 1) * float(d + 1)) < D:
        d += 1
    return d


def brute_force(rows, d2, w, points=None, chunk=1 << 22):
    """(T2 at ``points``, pairs of different rows): ``points`` (n, 3) voxel indices, default every voxel with a row;
    one term per pair (p, c), c over every voxel of the volume"""
    rows, d2 = np.asarray(rows), np.asarray(d2)
    if points is None:
        points = np.argwhere(rows > 0)
    points = np.asarray(points, np.int64).reshape(-1, 3)
    c_all = np.argwhere(np.ones(rows.shape, bool)).astype(np.float64)
    D_all, r_all = d2.reshape(-1), rows.reshape(-1)
    out = np.zeros(points.shape[0], np.float64)
    cross = 0
    step = max(1, chunk // max(1, c_all.shape[0]))
    for lo in range(0, points.shape[0], step):
        p = points[lo:lo + step]
        pf = p.astype(np.float64)
        dx, dy, dz = (pf[:, None, k] - c_all[None, :, k] for k in range(3))
        inside = d2_of(w, dx, dy, dz) < D_all[None, :]
        rp = rows[tuple(p.T)]
        cross += int((inside & (r_all[None, :] != rp[:, None])).sum())
        out[lo:lo + step] = np.where(rp > 0, np.where(inside, D_all[None, :], 0.0).max(axis=1), 0.0)
    return out, cross


def paint(rows, d2, w, chunk=1 << 22):
    """(X, Y, Z) float64 T2: every centre with a finite D2 > 0 raises its clipped box where d2 < D2"""
    d2 = np.asarray(d2)
    shape = d2.shape
    t2 = d2.copy()
    flat = t2.reshape(-1)
    centres = np.argwhere(np.isfinite(d2) & (d2 > 0))
    values = d2[tuple(centres.T)]
    for v in np.unique(values):
        h = [half_extent(v, w[k], shape[k]) for k in range(3)]
        o = np.stack(np.meshgrid(*(np.arange(-n, n + 1) for n in h), indexing="ij"), -1).reshape(-1, 3)
        of = o.astype(np.float64)
        o = o[d2_of(w, of[:, 0], of[:, 1], of[:, 2]) < v]
        c = centres[values == v]
        step = max(1, chunk // o.shape[0])
        for lo in range(0, c.shape[0], step):
            p = (c[lo:lo + step, None, :] + o[None, :, :]).reshape(-1, 3)
            p = p[((p >= 0) & (p < np.array(shape))).all(axis=1)]          # the clip to the volume
            at = np.unique(np.ravel_multi_index(tuple(p.T), shape))
            flat[at] = np.maximum(flat[at], v)
    return t2


def table_of(rows, t2):
    """(K, 3) int64 rows (row, T2 bit pattern, voxels), sorted by row and then value: the table of
    ``validate.lib.instance_local_thickness``"""
    fg = np.asarray(rows) > 0
    keys = np.stack((np.asarray(rows)[fg].astype(np.int64), np.ascontiguousarray(t2)[fg].view(np.int64)), 1)
    if keys.shape[0] == 0:
        return np.zeros((0, 3), np.int64)
    u, n = np.unique(keys, axis=0, return_counts=True)    # lexicographic; the patterns of non-negative doubles are >= 0
    return np.concatenate((u, n[:, None].astype(np.int64)), 1)


@functools.lru_cache(maxsize=None)
def _cached(name, spacing, closed):
    ids, rows = rows_of(cases()[name])
    d2 = edt_cases.oracle(rows, weights(spacing), closed)
    d2.setflags(write=False)
    t2 = paint(rows, d2, weights(spacing))
    t2.setflags(write=False)
    return ids, rows, d2, t2


def expected(name, spacing, closed):
    """(ids, rows, D2, T2) of a case, computed once per process and read-only"""
    return _cached(name, tuple(float(v) for v in spacing), bool(closed))
