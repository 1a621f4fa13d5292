"""The label volumes and the numpy oracle that tests/test_edt_cpu.py, tests/test_hip_edt.py and tools/edt_host_check.py
share (numpy only).

The definition (include/skoots_hip.h: sk_label_edt).  ``r(v)`` is the row of voxel v (1 .. N, 0 for
background), ``(wx, wy, wz) = (fl(sx sx), fl(sy sy), fl(sz sz))``; for a voxel p with r(p) > 0

    D2(p) = min over voxels q with r(q) != r(p) of  fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),

every square an exact integer, every product and sum rounded once, no fused multiply-add; 0 where r(p) = 0; ``inf`` where
no such q exists.  Open mode has the voxels of the volume only, closed mode the volume padded with one layer of
background.

Three statements of it, which the CPU tests hold against each other bit for bit:

``brute_force``  the minimum as written, one term per pair (p, q), chunked.  It costs voxels(row) x voxels(volume), so the
                 tests run it on every voxel of the small volumes and on a sample of the voxels of the large ones.
``oracle``       the same minimum with the innermost one taken first: rounding is monotone, so
                 ``min_q fl(a + fl(b + c_q)) = fl(a + fl(b + min_q c_q))`` and the minimum over the voxels of a line
                 along z can be taken before the line's (dx, dy) enters.  Still every line of the volume is a candidate
                 for every voxel: nothing is pruned.  Costs voxels(row) x lines(volume).
``walk``         the three pruned passes of the kernel (z, then y, then x), every lane of the kernel an array element.
"""
import functools

import numpy as np

from tests.skeleton_graph_cases import cases as _skeleton_cases

SPACINGS = ((1.0, 1.0, 1.0), (1.0, 1.0, 3.0), (2.0, 1.0, 5.0), (0.37, 0.41, 1.3))
INTEGER_SPACINGS = SPACINGS[:3]
MODES = (False, True)                                      # closed
INF = float("inf")
BALL = "ball (40, 40, 70)"
BLOBS = "blobs (24, 40, 70)"


def cases():
    """name -> (X, Y, Z) integer array: the volumes of tests/skeleton_graph_cases.py (ring and T among blobs, extents of
    1, one label filling the volume, opposite corners, a cross through all six faces, ids 2^31 - 1 and 2^40) and the
    ones where this kernel in particular can go wrong"""
    out = dict(_skeleton_cases())
    lab = np.zeros((6, 7, 8), np.int32)                   # two ids that share a whole plane and fill the volume
    lab[:3], lab[3:] = 1, 2
    out["shared plane (6, 7, 8)"] = lab
    lab = np.zeros((8, 8, 8), np.int32)                   # two cubes that touch in one corner only
    lab[1:4, 1:4, 1:4], lab[4:7, 4:7, 4:7] = 5, 6
    out["diagonal (8, 8, 8)"] = lab
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(70), indexing="ij"), -1)
    lab = (((g - np.array([20, 20, 56])) ** 2).sum(-1) <= 144).astype(np.int32) * 9    # z = 44 .. 68: walks of 13 steps
    out[BALL] = lab
    lab = np.zeros((9, 12, 10), np.int32)                 # fills the whole x extent: open mode gets nothing from x
    lab[:, 3:8, 2:7] = 3
    out["slab (9, 12, 10)"] = lab
    lab = np.zeros((12, 16, 30), np.int32)                # a U in the x-z plane: the slot is one voxel wide in x, so for
    lab[2:10, 2:14, 2:28] = 4                             # the voxels beside it the nearest outside voxel lies across
    lab[5, 2:14, 10:28] = 0                               # x, and the z pass, which runs first, sees far ends only
    out["U (12, 16, 30)"] = lab
    for shape in ((1, 17, 9), (13, 1, 1)):
        out[f"random {shape}"] = np.random.default_rng(sum(shape)).integers(0, 3, shape).astype(np.int32) * 4
    return out


def weights(spacing):
    """(wx, wy, wz): the squares of the spacing, each rounded once in float64"""
    sx, sy, sz = (float(v) for v in spacing)
    return sx * sx, sy * sy, sz * sz


def rows_of(lab):
    """(ids (N) int64 ascending, rows (X, Y, Z) int64): the positive ids and every voxel's row 1 .. N, 0 for the rest"""
    u = np.unique(lab)
    ids = u[u > 0].astype(np.int64)
    rows = (np.searchsorted(ids, lab.clip(min=0)) + 1) * (lab > 0)
    return ids, rows.astype(np.int64)


def _pad(rows, closed):
    return np.pad(rows, 1) if closed else rows


def brute_force(rows, w, closed, points=None, chunk=1 << 22):
    """D2 at ``points`` ((n, 3) voxel indices; default: every voxel with a row), one term per pair of voxels"""
    wx, wy, wz = w
    rows = np.asarray(rows)
    if points is None:
        points = np.argwhere(rows > 0)
    points = np.asarray(points, np.int64).reshape(-1, 3)
    pad = _pad(rows, closed)
    q_all = np.argwhere(np.ones(pad.shape, bool)) - int(closed)
    r_all = pad.reshape(-1)
    out = np.zeros(points.shape[0], np.float64)
    for r in np.unique(rows[tuple(points.T)]):
        sel = np.flatnonzero(rows[tuple(points.T)] == r)
        if r == 0:
            continue
        q = q_all[r_all != r].astype(np.float64)
        if q.shape[0] == 0:
            out[sel] = INF
            continue
        step = max(1, chunk // q.shape[0])
        for lo in range(0, sel.size, step):
            p = points[sel[lo:lo + step]].astype(np.float64)
            dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
            out[sel[lo:lo + step]] = (wx * (dx * dx) + (wy * (dy * dy) + wz * (dz * dz))).min(axis=1)
    return out


def oracle(rows, w, closed, chunk=1 << 22):
    """(X, Y, Z) float64 D2 of every voxel: per row, the minimum over the non-row voxels of every line along z first,
    then over all lines of the volume"""
    wx, wy, wz = w
    rows = np.asarray(rows)
    pad = _pad(rows, closed)
    X, Y, Z = pad.shape
    out = np.zeros(pad.shape, np.float64)
    zz = np.arange(Z, dtype=np.float64)
    cz = wz * ((zz[:, None] - zz[None, :]) ** 2)             # (z, z')
    xs = np.arange(X, dtype=np.float64)
    ys = np.arange(Y, dtype=np.float64)
    for r in range(1, int(rows.max(initial=0)) + 1):
        m = pad == r
        if not m.any():
            continue
        # a[x', y', z] = min over z' with pad[x', y', z'] != r of wz (z - z')^2: 0 on a line without the row
        a = np.zeros(pad.shape, np.float64)
        lines = np.argwhere(m.any(axis=2))
        a[lines[:, 0], lines[:, 1]] = np.where(m[lines[:, 0], lines[:, 1]][:, None, :], INF, cz[None]).min(axis=2)
        p = np.argwhere(m)
        step = max(1, chunk // (X * Y))
        for lo in range(0, p.shape[0], step):
            px, py, pz = p[lo:lo + step].T
            dx = px[:, None].astype(np.float64) - xs[None, :]
            dy = py[:, None].astype(np.float64) - ys[None, :]
            inner = wy * (dy * dy)[:, None, :] + a[:, :, pz].transpose(2, 0, 1)         # (n, X, Y)
            out[px, py, pz] = (wx * (dx * dx)[:, :, None] + inner).min(axis=(1, 2))
    return out[1:-1, 1:-1, 1:-1] if closed else out


def walk(rows, w, closed, steps=None):
    """(X, Y, Z) float64 D2: the kernel's three passes.  A voxel starts from ``best`` (inf in the z pass, the previous
    pass's value after it), steps outward along the pass's axis in both directions, d = 1, 2, ..., while
    ``w d^2 < best``; a voxel of its own row offers ``fl(w d^2 + g_prev(q))`` (nothing in the z pass), a voxel of
    another row offers ``w d^2`` and ends the direction, and so does the end of the volume in closed mode; in open mode
    it ends the direction and offers nothing.  ``steps`` (a list) receives the walk's steps of each pass, summed over
    the voxels."""
    rows = np.asarray(rows)
    shape = rows.shape
    fg = rows > 0
    g = np.where(fg, INF, 0.0)
    for axis, wa, first in ((2, w[2], True), (1, w[1], False), (0, w[0], False)):
        E = shape[axis]
        best = g.copy()
        alive = [fg.copy(), fg.copy()]                       # up, down
        coord = np.arange(E).reshape([E if k == axis else 1 for k in range(3)])
        n_steps = 0
        for d in range(1, E + 1):
            wd = wa * (float(d) * float(d))
            active = fg & (wd < best) & (alive[0] | alive[1])
            if not active.any():
                break
            n_steps += int(active.sum())
            for k, sign in enumerate((1, -1)):
                go = active & alive[k]
                inside = (coord + sign * d >= 0) & (coord + sign * d < E)
                off = go & ~inside
                alive[k] &= ~off
                if closed:
                    best = np.where(off, np.minimum(best, wd), best)
                go &= inside
                rq = np.roll(rows, -sign * d, axis=axis)     # rq[p] = rows[p + sign d] where that lies inside
                gq = np.roll(g, -sign * d, axis=axis)
                same = go & (rq == rows)
                other = go & (rq != rows)
                if not first:
                    best = np.where(same, np.minimum(best, wd + gq), best)
                best = np.where(other, np.minimum(best, wd), best)
                alive[k] &= ~other
        if steps is not None:
            steps.append(n_steps)
        g = best
    return g


def row_max(rows, d2):
    """(N) float64: the largest D2 of every row"""
    n = int(np.asarray(rows).max(initial=0))
    out = np.zeros(n, np.float64)
    np.maximum.at(out, rows[rows > 0] - 1, d2[rows > 0])
    return out


@functools.lru_cache(maxsize=None)
def _cached(name, spacing, closed):
    ids, rows = rows_of(cases()[name])
    d2 = oracle(rows, weights(spacing), closed)
    d2.setflags(write=False)
    return ids, rows, d2


def expected(name, spacing, closed):
    """(ids, rows, D2) of a case, computed once per process and read-only"""
    return _cached(name, tuple(float(v) for v in spacing), bool(closed))
