"""Not a test: a numpy restatement of ``sk_instance_overlaps`` written from the definition, the
pairs of volumes the overlap tests run it on, and host restatements of what is derived from the table."""
import itertools

import numpy as np

from tests import contact_cases as K

CHUNK = 4096                          # voxels the overlap kernel books between two flushes of its LDS table
LDS_SLOTS = 256                       # pairs that table holds
ROLL = (1, 2, 3)


def ref_overlaps(a, b, background=False):
    """(P, 3) int64, sorted by (ra, rb): ``ra, rb, voxels`` in ROWS (ranks of the positive ids, 0 = background)"""
    ra, rb = K.rows_of(a)[0].reshape(-1), K.rows_of(b)[0].reshape(-1)
    m1 = int(rb.max(initial=0)) + 1
    on = ((ra > 0) | (rb > 0)) if background else ((ra > 0) & (rb > 0))
    keys, counts = np.unique(ra[on] * m1 + rb[on], return_counts=True)
    return np.stack((keys // m1, keys % m1, counts), 1).astype(np.int64).reshape(-1, 3)


def loop_overlaps(a, b, background=False):
    """the same table from a plain loop over every voxel"""
    ra, rb = K.rows_of(a)[0], K.rows_of(b)[0]
    acc = {}
    for x, y, z in itertools.product(*(range(n) for n in ra.shape)):
        p, q = int(ra[x, y, z]), int(rb[x, y, z])
        if (p == 0 and q == 0) or ((p == 0 or q == 0) and not background):
            continue
        acc[(p, q)] = acc.get((p, q), 0) + 1
    return np.array([[*k, acc[k]] for k in sorted(acc)], np.int64).reshape(-1, 3)


def dense_iou(a, b):
    """(N, M) float32: ``mask_iou`` from the table -- fp32(inter) / fp32(union), one IEEE division per touching pair"""
    t = ref_overlaps(a, b, True)
    n, m = K.rows_of(a)[1].size, K.rows_of(b)[1].size
    size_a, size_b = np.zeros(n + 1, np.int64), np.zeros(m + 1, np.int64)
    np.add.at(size_a, t[:, 0], t[:, 2])
    np.add.at(size_b, t[:, 1], t[:, 2])
    t = t[(t[:, 0] > 0) & (t[:, 1] > 0)]
    iou = np.zeros((n, m), np.float32)
    union = size_a[t[:, 0]] + size_b[t[:, 1]] - t[:, 2]
    iou[t[:, 0] - 1, t[:, 1] - 1] = t[:, 2].astype(np.float32) / union.astype(np.float32)
    return iou


def rolled(v, shift=ROLL):
    return np.roll(v, shift, (0, 1, 2))


def noise_pair(shape, seed, ids=(0, 1, 2, 3)):
    """two independently seeded noise volumes, the second rolled by (1, 2, 3)"""
    return K.sparse_noise(shape, seed, ids), rolled(K.sparse_noise(shape, seed + 100, ids))


def many_ids_pair():
    """31 350 voxels -- no multiple of the chunk, several chunks -- and tens of thousands of distinct pairs"""
    return K.many_ids(K.CROSSING, 400, 10), rolled(K.many_ids(K.CROSSING, 300, 11))


def voxel_ids_pair(shape=(5, 6, 70)):
    """every voxel is a pair of its own: any chunk has more pairs than its LDS table holds"""
    v = K.voxel_ids(shape)
    return v, np.roll(v, 1, 2)


def balls(shape=(48, 64, 80), seed=0, k=12, radius=13):
    """k balls around random centres, a voxel taking the nearest centre's id: a dozen instances of thousands of voxels"""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.integers(0, n, k) for n in shape], 1)
    grid = np.stack(np.indices(shape), -1)[..., None, :]
    d2 = ((grid - centres) ** 2).sum(-1)
    return np.where(d2.min(-1) <= radius * radius, d2.argmin(-1) + 1, 0).astype(np.int64)


def balls_pair():
    return balls(seed=0), rolled(balls(seed=1), (3, 2, 1))


def tie_pair():
    """one ground-truth block, half under prediction 1 and half under prediction 2 of equal size: two equal IoU values"""
    g = np.zeros((6, 8, 20), np.int64)
    p = np.zeros_like(g)
    g[1:5, 2:6, 4:16] = 1
    p[1:5, 2:6, 2:10] = 1             # 6 of its 8 z-layers inside the block
    p[1:5, 2:6, 10:18] = 2
    return g, p


def shared_and_unmatched_pair():
    """ground truth 1 and 2 side by side under one prediction 5 (shared); prediction 7 clips ground truth 3, which
    prediction 8 covers better; prediction 9 lies on background (unmatched, best IoU 0); ground truth 4 has no partner"""
    g = np.zeros((10, 12, 40), np.int64)
    p = np.zeros_like(g)
    g[1:5, 1:6, 2:10], g[1:5, 6:11, 2:10] = 1, 2
    p[1:5, 1:11, 2:10] = 5
    g[6:9, 1:6, 2:12] = 3
    p[6:9, 1:6, 2:4], p[6:9, 1:6, 4:12] = 7, 8
    p[6:9, 8:11, 20:30] = 9
    g[1:4, 1:4, 30:36] = 4
    return g, p


PAIRS = {
    "many_ids": many_ids_pair,
    "one_voxel": lambda: (np.full((1, 1, 1), 6, np.int64), np.full((1, 1, 1), 4, np.int64)),
    "line_z": lambda: noise_pair((1, 1, 200), 5),
    "line_x": lambda: noise_pair((9, 1, 1), 7),
    "below_one_chunk": lambda: noise_pair((3, 5, 40), 9),
    "voxel_ids": voxel_ids_pair,
    "solid_block": lambda: (np.full((8, 16, 64), 5, np.int64),) * 2,
    "zero_a": lambda: (np.zeros((5, 9, 66), np.int64), K.sparse_noise((5, 9, 66), 12)),
    "zero_b": lambda: (K.sparse_noise((5, 9, 66), 13), np.zeros((5, 9, 66), np.int64)),
    "zero_both": lambda: (np.zeros((5, 9, 66), np.int64),) * 2,
    "ids_3_7_300_1000": lambda: noise_pair((12, 13, 9), 3, (0, 3, 7, 300, 1000)),
    "id_int32_max": lambda: noise_pair((12, 13, 9), 4, (0, 1, 2 ** 31 - 1)),
    "balls": balls_pair,
    "tie": tie_pair,
    "shared_and_unmatched": shared_and_unmatched_pair,
}


# ---- host restatements ----

def ref_relate(table, n, m, min_fraction=0.0):
    """``plan_relate`` in plain loops: (children, parents) as lists of per-row tuples
    ``(voxels, parent_row, inside_voxels, inside_fraction, parents_touched, outside_voxels)`` and
    ``(voxels, children, children_voxels, occupied_voxels, occupancy)``"""
    rows = [tuple(int(v) for v in r) for r in np.asarray(table).reshape(-1, 3).tolist()]
    children = []
    for c in range(1, n + 1):
        mine = [(rb, v) for ra, rb, v in rows if ra == c]
        voxels = sum(v for _, v in mine)
        inside = sorted(((-v, rb) for rb, v in mine if rb > 0))
        parent, shared = (inside[0][1], -inside[0][0]) if inside else (0, 0)
        if parent and shared / voxels < min_fraction:
            parent, shared = 0, 0
        children.append((voxels, parent, shared, shared / voxels if parent else 0.0, len(inside),
                         sum(v for rb, v in mine if rb == 0)))
    parents = []
    for p in range(1, m + 1):
        voxels = sum(v for _, rb, v in rows if rb == p)
        kids = [c for c in children if c[1] == p]
        occupied = sum(v for ra, rb, v in rows if rb == p and ra > 0)
        parents.append((voxels, len(kids), sum(c[0] for c in kids), occupied, occupied / voxels if voxels else 0.0))
    return children, parents
