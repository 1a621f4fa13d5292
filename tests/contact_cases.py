"""Not a test: a numpy restatement of ``sk_instance_contacts`` written from the definition with
shifted slices, the volumes the contact tests run it on, and host restatements of what is derived from the table."""
import itertools

import numpy as np

from tests.clean_cases import CROSSING, blob, checkerboard, corner_contact, edge_contact, sparse_noise  # noqa: F401

TILE = (4, 16, 64)                    # the contact kernel's tile (x, y, z); CROSSING crosses it at least twice per axis
CLASS_OF_AXES = {(0,): 0, (1,): 1, (2,): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5, (0, 1, 2): 6}
CLASSES_AT = {6: 3, 18: 6, 26: 7}

# one direction of every +-d pair: the first nonzero component is positive
FORWARD = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
assert len(FORWARD) == 13


def rows_of(volume):
    """(rows, ids): every positive value replaced by its rank 1..N among the sorted positive values, the rest 0"""
    v = np.asarray(volume).astype(np.int64)
    ids = np.unique(v[v > 0])
    rows = np.where(v > 0, np.searchsorted(ids, v) + 1, 0)
    return rows, ids


def _shifted(r, d):
    """(p, q): views of r such that q is p displaced by d, over every position where both lie inside"""
    p = tuple(slice(max(-k, 0), n - max(k, 0)) for k, n in zip(d, r.shape))
    q = tuple(slice(max(k, 0), n - max(-k, 0)) for k, n in zip(d, r.shape))
    return r[p], r[q]


def ref_contacts(volume, connectivity=6, background=False):
    """(P, 9) int64, sorted by (lo, hi): ``lo, hi, c0 .. c6`` in ROWS (ranks of the positive ids, 0 = background)"""
    r, _ = rows_of(volume)
    n = int(r.max(initial=0)) + 1
    acc = {}
    for d in FORWARD:
        cls = CLASS_OF_AXES[tuple(k for k in range(3) if d[k])]
        if cls >= CLASSES_AT[connectivity]:
            continue
        a, b = _shifted(r, d)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        on = (a != b) & ((lo > 0) | ((hi > 0) & bool(background)))
        keys, counts = np.unique(lo[on] * n + hi[on], return_counts=True)
        for k, c in zip(keys.tolist(), counts.tolist()):
            acc.setdefault(k, [0] * 7)[cls] += c
    return np.array([[k // n, k % n, *acc[k]] for k in sorted(acc)], np.int64).reshape(-1, 9)


def loop_contacts(volume, connectivity=6, background=False):
    """the same table from a plain loop over every voxel and its 26 neighbours, every unordered pair once"""
    r, _ = rows_of(volume)
    X, Y, Z = r.shape
    acc = {}
    for x, y, z in itertools.product(range(X), range(Y), range(Z)):
        for d in itertools.product((-1, 0, 1), repeat=3):
            q = (x + d[0], y + d[1], z + d[2])
            if d == (0, 0, 0) or not all(0 <= c < n for c, n in zip(q, r.shape)) or (x, y, z) > q:
                continue
            cls = CLASS_OF_AXES[tuple(k for k in range(3) if d[k])]
            if cls >= CLASSES_AT[connectivity]:
                continue
            a, b = int(r[x, y, z]), int(r[q])
            if a == b or max(a, b) == 0 or (min(a, b) == 0 and not background):
                continue
            acc.setdefault((min(a, b), max(a, b)), [0] * 7)[cls] += 1
    return np.array([[*k, *acc[k]] for k in sorted(acc)], np.int64).reshape(-1, 9)


def with_ids(table, ids):
    """the table with its rows 1..N replaced by ids (0 stays 0)"""
    lut = np.concatenate(([0], np.asarray(ids, np.int64)))
    return np.concatenate((lut[table[:, :2]], table[:, 2:]), 1)


def exposed_faces(volume):
    """(N, 3) int64: per row the faces exposed to another row, background or the outside of the volume, with the normal
    along x / y / z -- counted per id with a padded boolean mask, independently of the contact table"""
    r, ids = rows_of(volume)
    out = np.zeros((ids.size, 3), np.int64)
    for k in range(ids.size):
        m = np.pad(r == k + 1, 1)
        for ax in range(3):
            out[k, ax] = int((m & ~np.roll(m, 1, ax)).sum() + (m & ~np.roll(m, -1, ax)).sum())
    return out


def border_voxels(volume):
    """(N, 3) int64: per row its voxels in the two border planes of each axis (a voxel in both counts twice)"""
    r, ids = rows_of(volume)
    out = np.zeros((ids.size, 3), np.int64)
    for ax in range(3):
        for plane in (np.take(r, 0, ax), np.take(r, r.shape[ax] - 1, ax)):
            out[:, ax] += np.bincount(plane.reshape(-1), minlength=ids.size + 1)[1:]
    return out


def face_contacts_per_row(table, n):
    """(N, 3) int64: the face contacts of every row summed over all partners, background included"""
    out = np.zeros((n + 1, 3), np.int64)
    np.add.at(out, table[:, 0], table[:, 2:5])
    np.add.at(out, table[:, 1], table[:, 2:5])
    return out[1:]


# ---- case volumes ----

def voxel_ids(shape):
    """every voxel carries its own id: every neighbouring voxel pair is a distinct key"""
    return (np.arange(int(np.prod(shape)), dtype=np.int64) + 1).reshape(shape)


def many_ids(shape, k, seed):
    """a random id in 1..k per voxel, one voxel in eight zero"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, k + 1, shape)
    v[rng.random(shape) < 0.125] = 0
    return v.astype(np.int64)


def split_blob(shape=(24, 22, 20)):
    """one ball cut in two by a flat wall, ids 2 and 5, and a distant small ball of id 9"""
    x, y, z = np.indices(shape)
    ball = (x - 9) ** 2 + (y - 10) ** 2 + (z - 9) ** 2 <= 49
    m = np.where(ball, np.where(y < 10, 2, 5), 0)
    m[(x - 20) ** 2 + (y - 17) ** 2 + (z - 16) ** 2 <= 4] = 9
    return m.astype(np.int32)


def ref_merge(volume, groups):
    """every id of a group replaced by the group's smallest"""
    out = np.asarray(volume).astype(np.int64).copy()
    for g in groups:
        out[np.isin(out, list(g))] = min(g)
    return out


def ref_renumber(volume):
    """1..K by first appearance in C order"""
    flat = np.asarray(volume).reshape(-1)
    seen, first = np.unique(flat, return_index=True)
    seen, first = seen[seen > 0], first[seen > 0]
    lut = np.zeros(int(flat.max(initial=0)) + 1, np.int64)
    lut[seen[np.argsort(first)]] = np.arange(1, seen.size + 1)
    return lut[flat].reshape(np.asarray(volume).shape)
