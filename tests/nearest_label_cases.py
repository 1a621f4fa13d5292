"""The label volumes and the numpy statements of the nearest-instance transform that tests/test_nearest_label_cpu.py,
tests/test_hip_nearest_label.py and tools/nearest_label_host_check.py share (numpy only).

The definition (include/skoots_hip.h: sk_nearest_label).  ``r(v)`` is the row of voxel v (1 .. N, 0
for background), ``(wx, wy, wz) = (fl(sx sx), fl(sy sy), fl(sz sz))``, a site is a voxel with r > 0, and for a voxel p
and a site q

    value(p, q) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),        D2(p) = min over sites q of value(p, q),

every square an exact integer, every product and sum rounded once, no fused multiply-add.  ``nearest(p)`` is the row of
the site the nested minimum chooses when it is taken as three passes -- z, then y, then x -- each keeping the smallest
coordinate among the positions of equal value.  ``limit2`` and ``where`` then decide what is answered (``restrict``).

Three statements of it, which the CPU tests hold against each other bit for bit:

``brute_force``  the minimum as written, one term per pair (voxel, site), with the tie rule stated globally.
``oracle``       the three passes unpruned: every position of a line is a candidate for every voxel of the line, one
                 ``argmin`` per voxel and pass; numpy's first minimum is the smallest coordinate.
``walk``         the three pruned passes of the kernel, every lane of the kernel an array element.
"""
import functools

import numpy as np

from tests import edt_cases
from tests.edt_cases import BALL, BLOBS, INF, INTEGER_SPACINGS, SPACINGS, rows_of, weights  # noqa: F401

TIE_Y = "3-4-5 tie along y (1, 8, 7)"
TIE_X = "3-4-5 tie along x (8, 1, 7)"
TIE_Z = "3-4-5 tie along z (1, 7, 8)"
SIDES = "low and high ties (7, 7, 7)"
REACH = "reach boundary (9, 9, 9)"
REACH_SITE, REACH_VOXEL = (1, 2, 3), (4, 6, 5)
STRETCH = "site-free stretch (2, 3, 150)"
NO_SITES = "no sites (5, 6, 7)"
WHERE_CASE = "diagonal (8, 8, 8)"


def cases():
    """name -> (X, Y, Z) integer array: every volume of tests/edt_cases.py and the ones where this kernel in particular
    can go wrong"""
    out = dict(edt_cases.cases())
    lab = np.zeros((1, 8, 7), np.int32)                   # four candidates of value 25 for voxel (0, 6, 0): 25 + 0,
    lab[0, 1, 0], lab[0, 2, 3], lab[0, 3, 4], lab[0, 6, 5] = 1, 2, 3, 4     # 16 + 9, 9 + 16, 0 + 25; y' = 1 must win
    out[TIE_Y] = lab
    out[TIE_X] = np.ascontiguousarray(lab.transpose(1, 0, 2))               # voxel (6, 0, 0): x' = 1 must win
    out[TIE_Z] = np.ascontiguousarray(lab.transpose(0, 2, 1))               # voxel (0, 0, 6): the site (0, 0, 1)
    lab = np.zeros((7, 7, 7), np.int32)                   # the centre has six sites at value 4 w: the low x side wins,
    lab[1, 3, 3], lab[5, 3, 3], lab[3, 1, 3], lab[3, 5, 3], lab[3, 3, 1], lab[3, 3, 5] = 6, 1, 5, 2, 4, 3
    out[SIDES] = lab                                      # and it carries the largest id
    for axis, name in enumerate("xyz"):
        shape = [1, 1, 1]
        shape[axis] = 7
        lab = np.zeros(shape, np.int32)
        lab.reshape(-1)[[1, 5]] = (2, 1)                  # voxel 3 is two steps from both: the low side, id 2
        out[f"low and high along {name} {tuple(shape)}"] = lab
    lab = np.zeros((9, 9, 9), np.int32)
    lab[REACH_SITE] = 7
    out[REACH] = lab
    lab = np.zeros((2, 3, 150), np.int32)                 # 141 site-free voxels along z: walks cross a wave's line
    lab[0, 0, 3], lab[0, 0, 145], lab[1, 2, 3], lab[1, 2, 145], lab[1, 1, 70] = 1, 2, 3, 4, 5
    out[STRETCH] = lab
    out[NO_SITES] = np.zeros((5, 6, 7), np.int32)
    lab = np.zeros((13, 1, 1), np.int32)
    lab[12, 0, 0] = 3
    out["corner site (13, 1, 1)"] = lab
    lab = np.zeros((1, 17, 9), np.int32)
    lab[0, 0, 0] = 3
    out["corner site (1, 17, 9)"] = lab
    return out


def value(p, q, w):
    """fl(wx dx^2 + fl(wy dy^2 + wz dz^2)) of two voxels, in Python floats"""
    dx, dy, dz = (float(a - b) for a, b in zip(p, q))
    return w[0] * (dx * dx) + (w[1] * (dy * dy) + w[2] * (dz * dz))


def limits(name, spacing):
    """the values of limit2 a case runs at: no limit, a reach of two voxels along the coarsest axis (more along the
    others, and sites exactly at the reach), 0, and what the case is about"""
    w = weights(spacing)
    out = [INF, 4.0 * max(w), 0.0]
    if name in (TIE_Y, TIE_X, TIE_Z):
        out += [25.0, 24.0]
    if name == REACH:                                     # the site exactly at the reach, and one float above it
        v = value(REACH_VOXEL, REACH_SITE, w)
        out += [v, float(np.nextafter(v, 0.0))]
    if name == STRETCH:                                   # a reach shorter and longer than the stretch
        out += [w[2] * (30.0 * 30.0), w[2] * (145.0 * 145.0)]
    return tuple(out)


def where_cases(lab):
    """name -> (X, Y, Z) uint8: all zero, all one, a checkerboard, and zero exactly on the sites (which still count)"""
    g = np.indices(lab.shape).sum(0)
    return {"zeros": np.zeros(lab.shape, np.uint8), "ones": np.ones(lab.shape, np.uint8),
            "checkerboard": (g % 2).astype(np.uint8) * 255, "off on the sites": (np.asarray(lab) <= 0).astype(np.uint8)}


def restrict(rows, d2, near, limit2=INF, where=None):
    """the last step of the definition: ``(+inf, 0)`` where D2 is above limit2 or not finite, and on the unwanted
    voxels that are no sites"""
    out = ~(d2 <= limit2) | ~np.isfinite(d2)
    if where is not None:
        out |= (np.asarray(where) == 0) & (np.asarray(rows) == 0)
    return np.where(out, INF, d2), np.where(out, 0, near)


def brute_force(rows, w, points=None, chunk=1 << 20):
    """(D2, nearest) at ``points`` ((n, 3) voxel indices; default: every voxel), unrestricted, one term per pair of a
    voxel and a site.  The tie rule, globally: of the sites at value D2 the smallest x'; of the sites of that plane those
    with the smallest fl(wy dy^2 + wz dz^2), and of them the smallest y'; of the sites of that line those with the
    smallest wz dz^2, and of them the smallest z'."""
    wx, wy, wz = w
    rows = np.asarray(rows)
    if points is None:
        points = np.argwhere(np.ones(rows.shape, bool))
    points = np.asarray(points, np.int64).reshape(-1, 3)
    sites = np.argwhere(rows > 0)
    d2 = np.full(points.shape[0], INF)
    near = np.zeros(points.shape[0], np.int64)
    if sites.shape[0] == 0:
        return d2, near
    q = sites.astype(np.float64)
    step = max(1, chunk // sites.shape[0])
    big = np.int64(2 ** 40)
    for lo in range(0, points.shape[0], step):
        p = points[lo:lo + step].astype(np.float64)
        dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
        line = wz * (dz * dz)
        plane = wy * (dy * dy) + line
        val = wx * (dx * dx) + plane
        best = val.min(axis=1)
        m = val == best[:, None]
        for coord, inner in ((0, plane), (1, line), (2, None)):
            c = np.where(m, sites[None, :, coord], big).min(axis=1)
            m &= sites[None, :, coord] == c[:, None]
            if inner is not None:
                m &= inner == np.where(m, inner, INF).min(axis=1)[:, None]
        assert (m.sum(axis=1) == 1).all()
        chosen = sites[m.argmax(axis=1)]
        d2[lo:lo + step] = best
        near[lo:lo + step] = rows[tuple(chosen.T)]
    return d2, near


def _unpruned_pass(g, row, w, axis, chunk=1 << 22):
    """min over the positions c' of a line of fl(w (c - c')^2 + g(c')) and the row at the first minimum"""
    g = np.moveaxis(g, axis, -1)
    row = np.moveaxis(row, axis, -1)
    shape = g.shape
    E = shape[-1]
    g = np.ascontiguousarray(g).reshape(-1, E)
    row = np.ascontiguousarray(row).reshape(-1, E)
    c = np.arange(E)
    d = (c[:, None] - c[None, :]).astype(np.float64)
    cost = w * (d * d)                                      # (c, c')
    out_g = np.empty_like(g)
    out_row = np.empty_like(row)
    step = max(1, chunk // (E * E))
    for lo in range(0, g.shape[0], step):
        val = cost[None] + g[lo:lo + step, None, :]         # (lines, c, c')
        k = val.argmin(axis=2)
        out_g[lo:lo + step] = np.take_along_axis(val, k[:, :, None], axis=2)[:, :, 0]
        out_row[lo:lo + step] = np.take_along_axis(row[lo:lo + step], k, axis=1)
    return np.moveaxis(out_g.reshape(shape), -1, axis), np.moveaxis(out_row.reshape(shape), -1, axis)


def oracle(rows, w, limit2=INF, where=None):
    """(D2 (X, Y, Z) float64, nearest (X, Y, Z) int64 rows): the three passes with nothing pruned, then ``restrict``"""
    rows = np.asarray(rows).astype(np.int64)
    g = np.where(rows > 0, 0.0, INF)
    row = rows
    for axis in (2, 1, 0):
        g, row = _unpruned_pass(g, row, w[axis], axis)
    return restrict(rows, g, row, limit2, where)


def walk(rows, w, limit2=INF, where=None, reads=None):
    """(D2, nearest) as the kernel computes them.  A voxel starts from its own position's offer -- (0, r(p)) on a site,
    else the previous pass's (g, row), (+inf, 0) in the z pass -- and steps outward along the pass's axis, d = 1, 2,
    ..., while a position at d lies inside, ``w d^2 <= best`` and ``w d^2 <= limit2``: the low side first, which wins
    with ``<=``, then the high side, only while ``w d^2 < best``, which wins with ``<``.  The last pass skips the
    unwanted voxels that are no sites and turns what is above limit2 or not finite into (+inf, 0).  ``reads`` (a list)
    receives the positions read in each pass, summed over the voxels."""
    rows = np.asarray(rows).astype(np.int64)
    shape = rows.shape
    site = rows > 0
    g = grow = None
    for axis, wa in ((2, w[2]), (1, w[1]), (0, w[0])):
        first, last = axis == 2, axis == 0
        E = shape[axis]
        coord = np.arange(E).reshape([E if k == axis else 1 for k in range(3)])
        best = np.where(site, 0.0, INF if first else g)
        row = np.where(site, rows, 0 if first else grow)
        walking = ~site
        if last and where is not None:
            skip = ~site & (np.asarray(where) == 0)
            best, row, walking = np.where(skip, INF, best), np.where(skip, 0, row), walking & ~skip
        n_reads = 0
        for d in range(1, E):
            wd = wa * (float(d) * float(d))
            in_lo = np.broadcast_to(coord - d >= 0, shape)
            in_hi = np.broadcast_to(coord + d < E, shape)
            walking = walking & (in_lo | in_hi) & (wd <= best) & ~(wd > limit2)
            if not walking.any():
                break
            for inside, shift, wins in ((in_lo, d, np.less_equal), (in_hi, -d, np.less)):
                go = walking & inside
                if shift < 0:
                    go &= wd < best
                n_reads += int(go.sum())
                if first:
                    rq = np.roll(rows, shift, axis=axis)        # rq[p] = rows[p - shift]
                    take = go & (rq > 0)
                    best, row = np.where(take, wd, best), np.where(take, rq, row)
                else:
                    v = wd + np.roll(g, shift, axis=axis)
                    take = go & wins(v, best)
                    best, row = np.where(take, v, best), np.where(take, np.roll(grow, shift, axis=axis), row)
        if reads is not None:
            reads.append(n_reads)
        if last:
            out = ~((best <= limit2) & (best < INF))
            best, row = np.where(out, INF, best), np.where(out, 0, row)
        g, grow = best, row
    return g, grow


def grow_rule(lab, d2, near_id, distance, within=None):
    """``grow(distance > 0)`` in numpy: a zero voxel, inside ``within`` if given, takes the nearest id when
    ``D2 <= fl(d d)``; every other voxel keeps what it holds"""
    lab = np.asarray(lab)
    take = (lab == 0) & (d2 <= float(distance) * float(distance))
    if within is not None:
        take &= np.asarray(within) != 0
    return np.where(take, near_id, lab).astype(lab.dtype)


def shrink_rule(lab, edt_d2, distance):
    """``grow(distance < 0)`` in numpy: a voxel keeps its id iff its ``label_edt`` value exceeds ``fl(d d)``"""
    lab = np.asarray(lab)
    return np.where(edt_d2 > float(distance) * float(distance), lab, 0).astype(lab.dtype)


def report_counts(before, after):
    """the fields of ``GrowReport`` from the two volumes"""
    a, b = np.asarray(before), np.asarray(after)
    ids_a, ids_b = np.unique(a[a > 0]), np.unique(b[b > 0])
    grown = np.unique(b[(a == 0) & (b > 0)])
    return dict(instances_in=int(ids_a.size), instances_out=int(ids_b.size),
                voxels_added=int(((a == 0) & (b != 0)).sum()), voxels_removed=int(((a != 0) & (b == 0)).sum()),
                ids_removed=int(np.setdiff1d(ids_a, ids_b).size), ids_grown=int(grown.size))


@functools.lru_cache(maxsize=None)
def _cached(name, spacing):
    ids, rows = rows_of(cases()[name])
    d2, near = oracle(rows, weights(spacing))
    for a in (ids, rows, d2, near):
        a.setflags(write=False)
    return ids, rows, d2, near


def expected(name, spacing, limit2=INF, where=None):
    """(ids, rows, D2, nearest rows) of a case: the unrestricted oracle is computed once per process and is read-only,
    ``restrict`` is applied per call"""
    ids, rows, d2, near = _cached(name, tuple(float(v) for v in spacing))
    d2, near = restrict(rows, d2, near, limit2, where)
    return ids, rows, d2, near


def ids_of(ids, near_rows):
    """rows 1 .. N back to ids, 0 staying 0"""
    return np.concatenate((np.zeros(1, np.int64), np.asarray(ids, np.int64)))[near_rows]
