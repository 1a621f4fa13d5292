"""Not a test: a numpy restatement of ``sk_instance_proximity`` written from the definition -- a
loop over the offsets within the limit, a table (voxel, ra, rb) -> min d2, then the rows -- and the volumes the proximity
tests run it on."""
import itertools

import numpy as np

from tests import contact_cases as K

TILE = (4, 16, 64)                    # the proximity kernel's tile (x, y, z); K.CROSSING crosses it twice per axis
LDS_SLOTS = 256                       # keys the tile's LDS table holds
SEEN = 4                              # partners a lane keeps in registers before it falls back to the rescan


def metric(distance, spacing):
    """((wx, wy, wz), limit2): the spacing squared and fl(d d), python floats (IEEE doubles, one rounding each)"""
    return tuple(float(s) * float(s) for s in spacing), float(distance) * float(distance)


def d2_of(w, d):
    """fl(wx dx^2 + fl(wy dy^2 + wz dz^2)): every product and sum a python float operation, rounded once"""
    return w[0] * float(d[0] * d[0]) + (w[1] * float(d[1] * d[1]) + w[2] * float(d[2] * d[2]))


def reach(w, limit2, most=1 << 20):
    """per axis the largest k >= 0 with fl(w k^2) <= limit2, by counting up"""
    out = []
    for wk in w:
        k = 0
        while k < most and wk * float((k + 1) * (k + 1)) <= limit2:
            k += 1
        out.append(k)
    return tuple(out)


def _views(shape, d):
    """(p, q): slices such that voxel q = p + d, over every p for which both lie inside"""
    p = tuple(slice(max(-k, 0), n - max(k, 0)) for k, n in zip(d, shape))
    q = tuple(slice(max(k, 0), n - max(-k, 0)) for k, n in zip(d, shape))
    return p, q


def ref_proximity(a, b=None, distance=0.0, spacing=(1.0, 1.0, 1.0)):
    """(pairs (P, 3) int64 sorted by (ra, rb), gap2 (P) float64): ``ra, rb, near_voxels`` in ROWS (ranks of the positive
    ids), the union rows at rb = 0; ``b=None`` is the one-mask mode"""
    same = b is None
    ra = K.rows_of(a)[0]
    rb = ra if same else K.rows_of(b)[0]
    assert ra.shape == rb.shape
    w, limit2 = metric(distance, spacing)
    h = tuple(min(k, max(n - 1, 0)) for k, n in zip(reach(w, limit2), ra.shape))   # farther leaves the volume
    m1 = int(rb.max(initial=0)) + 1
    voxel = np.arange(ra.size, dtype=np.int64).reshape(ra.shape)
    keys, vals = [], []
    for d in itertools.product(*(range(-k, k + 1) for k in h)):
        d2 = d2_of(w, d)
        if not d2 <= limit2:
            continue
        # q = p + d: the definition's dx = px - qx is -d, and d2 is even in it
        p, q = _views(ra.shape, d)
        pa, qb = ra[p], rb[q]
        on = (pa > 0) & (qb > 0)
        if same:
            on &= pa != qb
        keys.append(voxel[p][on] * m1 + qb[on])
        vals.append(np.full(int(on.sum()), d2))
    if not keys or not sum(k.size for k in keys):
        return np.zeros((0, 3), np.int64), np.zeros(0, np.float64)
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    order = np.lexsort((vals, keys))
    keys, vals = keys[order], vals[order]
    first = np.concatenate(([True], keys[1:] != keys[:-1]))
    keys, vals = keys[first], vals[first]                  # (voxel, rb) -> min d2
    vox, prb = keys // m1, keys % m1
    pra = ra.reshape(-1)[vox]
    acc = {}
    for r_a, r_b, v in zip(pra.tolist(), prb.tolist(), vals.tolist()):
        n, g = acc.get((r_a, r_b), (0, np.inf))
        acc[(r_a, r_b)] = (n + 1, min(g, v))
    # the union rows: a voxel once, whatever the number of its partners
    uniq_vox, start = np.unique(vox, return_index=True)
    vmin = np.minimum.reduceat(vals, start)
    for r_a, v in zip(ra.reshape(-1)[uniq_vox].tolist(), vmin.tolist()):
        n, g = acc.get((r_a, 0), (0, np.inf))
        acc[(r_a, 0)] = (n + 1, min(g, v))
    ks = sorted(acc)
    return (np.array([[*k, acc[k][0]] for k in ks], np.int64).reshape(-1, 3),
            np.array([acc[k][1] for k in ks], np.float64))


def loop_proximity(a, b=None, distance=0.0, spacing=(1.0, 1.0, 1.0)):
    """the same table from a plain loop over every voxel pair: small volumes only"""
    same = b is None
    ra = K.rows_of(a)[0]
    rb = ra if same else K.rows_of(b)[0]
    w, limit2 = metric(distance, spacing)
    best = {}
    cells = list(itertools.product(*(range(n) for n in ra.shape)))
    for p in cells:
        if ra[p] == 0:
            continue
        for q in cells:
            if rb[q] == 0 or (same and ra[p] == rb[q]):
                continue
            d2 = d2_of(w, tuple(i - j for i, j in zip(p, q)))
            if d2 <= limit2:
                for key in ((p, int(ra[p]), int(rb[q])), (p, int(ra[p]), 0)):
                    best[key] = min(best.get(key, np.inf), d2)
    acc = {}
    for (_, r_a, r_b), v in best.items():
        n, g = acc.get((r_a, r_b), (0, np.inf))
        acc[(r_a, r_b)] = (n + 1, min(g, v))
    ks = sorted(acc)
    return (np.array([[*k, acc[k][0]] for k in ks], np.int64).reshape(-1, 3),
            np.array([acc[k][1] for k in ks], np.float64))


def ref_plan(pairs, gap2, n):
    """``plan_proximity`` in plain loops: per row of a ``(partners, nearest_row, nearest_gap2, near_voxels)``"""
    rows = [(int(r[0]), int(r[1]), int(r[2]), float(g)) for r, g in zip(np.asarray(pairs).reshape(-1, 3), gap2)]
    out = []
    for r in range(1, n + 1):
        mine = sorted((g, rb) for ra, rb, _, g in rows if ra == r and rb > 0)
        union = [v for ra, rb, v, _ in rows if ra == r and rb == 0]
        out.append((len(mine), mine[0][1] if mine else 0, mine[0][0] if mine else np.inf, union[0] if union else 0))
    return out


# ---- case volumes ----

def noise_pair(shape, seed, ids=(0, 0, 0, 0, 0, 1, 2, 3)):
    """two independently seeded sparse noise volumes (five voxels in eight background)"""
    return K.sparse_noise(shape, seed, ids), K.sparse_noise(shape, seed + 100, ids)


def two_voxels(shape, p, q, ids=(4, 9)):
    a, b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    a[p], b[q] = ids
    return a, b


def faces_pair(shape=(6, 18, 70)):
    """instances on every face, edge and corner of the volume, of a and of b: every halo lies outside"""
    a, b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    a[0], a[-1], a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1] = 1, 2, 3, 4, 5, 6
    b[1:-1, 1:-1, 1:-1] = K.sparse_noise(tuple(n - 2 for n in shape), 21, (0, 0, 0, 7, 8))
    b[0, 0, :], b[-1, :, -1], b[:, -1, 0] = 11, 12, 13
    return a, b


def voxel_ids_pair(shape=(5, 6, 70)):
    """b carries one id per voxel: a voxel of a sees dozens of rows of b at D = 2, far more than a lane's list and a
    tile's table hold"""
    return K.sparse_noise(shape, 31, (0, 1, 2)), K.voxel_ids(shape)


def many_ids_pair():
    return K.many_ids(K.CROSSING, 400, 10), K.many_ids(K.CROSSING, 300, 11)


def balls_pair(shape=(20, 40, 72)):
    """a few solid instances per mask with gaps of a few voxels between them"""
    x, y, z = np.indices(shape)
    a, b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    for k, (cx, cy, cz, r) in enumerate([(6, 8, 12, 5), (12, 28, 30, 7), (5, 20, 60, 4), (15, 10, 50, 5), (6, 19, 12, 4),
                                         (14, 2, 60, 3)]):
        a[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = 3 * k + 2
    for k, (cx, cy, cz, r) in enumerate([(8, 15, 14, 4), (10, 22, 42, 5), (16, 33, 20, 4), (3, 3, 70, 3), (17, 5, 38, 3)]):
        b[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = 5 * k + 1
    return a, b
