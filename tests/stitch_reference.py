"""Naive restatements of skoots/utils/flood_and_stitch.py for the tests of ``skoots_amd.utils.flood_and_stitch``
(numpy / scipy only; nothing here touches the code under test).

``voxel_stitch``     the reference's loops over voxels, from its description: label every slice, two greedy passes
``plane_tables``     scipy / numpy tables of a mask: global-id labels, offsets, sorted overlap rows
``naive_table_walk`` the two passes on tables with one label per component and a full sweep for every rename
``first_seen``       ids 1..K in order of first appearance in C order, 0 kept
"""
from __future__ import annotations

import numpy as np
import scipy.ndimage


def _slice(dim, i):
    idx = [slice(None)] * 3
    idx[dim] = i
    return tuple(idx)


def voxel_stitch(mask: np.ndarray, dim: int) -> np.ndarray:
    """The stitched int32 labels BEFORE the final renumbering."""
    vol = (mask > 0).astype(np.int32)
    n = vol.shape[dim]
    for i in range(n):
        vol[_slice(dim, i)] = scipy.ndimage.label(vol[_slice(dim, i)])[0]   # 4-connected, numbering restarts at 1
    if n == 1:
        return vol
    for _ in range(2):
        newind = int(vol.max()) if vol.size else 0    # the first new id equals the largest id present
        for i in range(1, n):
            a, b = vol[_slice(dim, i - 1)], vol[_slice(dim, i)]
            for u in np.unique(a):                    # the list is taken before the loop
                if u == 0:
                    continue
                labels, counts = np.unique(b[a == u], return_counts=True)
                keep = (labels != 0) & (labels != u)  # a slice-b label equal to u counts as the same object already
                labels, counts = labels[keep], counts[keep]
                if labels.size == 0:
                    continue
                to_replace = labels[np.argmax(counts)]   # ties: the smallest label
                before = vol[_slice(dim, slice(0, i))]
                before[before == u] = newind              # every voxel before slice i that carries u
                b[b == to_replace] = newind
                newind += 1
        vol = np.flip(vol, axis=dim)
    return np.ascontiguousarray(vol)


def first_seen(labels: np.ndarray) -> np.ndarray:
    flat = labels.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    first, ids = first[ids != 0], ids[ids != 0]
    lut = {int(v): k + 1 for k, v in enumerate(ids[np.argsort(first)])}
    lut[0] = 0
    return np.array([lut[int(v)] for v in flat], dtype=np.int32).reshape(labels.shape)


def plane_labels(mask: np.ndarray, dim: int):
    """(global-id int32 labels, offsets): slice p owns offsets[p] + 1 .. offsets[p + 1], in scipy's order."""
    n = mask.shape[dim]
    labels = np.zeros(mask.shape, dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.int32)
    for p in range(n):
        lab, k = scipy.ndimage.label(mask[_slice(dim, p)] > 0)
        labels[_slice(dim, p)] = np.where(lab > 0, lab + offsets[p], 0)
        offsets[p + 1] = offsets[p] + k
    return labels, offsets


def overlap_rows(labels: np.ndarray, dim: int) -> np.ndarray:
    """(R, 3) int32 rows (id_a, id_b, n) of adjacent slices, sorted by (id_a, id_b)."""
    n = labels.shape[dim]
    a = labels[_slice(dim, slice(0, n - 1))].reshape(-1).astype(np.int64)
    b = labels[_slice(dim, slice(1, n))].reshape(-1).astype(np.int64)
    both = (a > 0) & (b > 0)
    keys, counts = np.unique(a[both] * (1 << 32) + b[both], return_counts=True)
    return np.stack([keys >> 32, keys & 0xFFFFFFFF, counts], axis=1).astype(np.int32).reshape(-1, 3)


def plane_tables(mask: np.ndarray, dim: int):
    labels, offsets = plane_labels(mask, dim)
    return labels, offsets, overlap_rows(labels, dim)


def naive_table_walk(offsets, rows, without=None):
    """lut[id] = label of component id after both passes; every rename sweeps every component.  ``without`` switches one
    of the reference's quirks off ("tie": the largest label wins a tie, "newind": new ids start past the maximum,
    "same": a slice-b label equal to u competes like any other), to show that a fixture case depends on it."""
    offsets = [int(v) for v in offsets]
    P, T = len(offsets) - 1, offsets[-1]
    plane = [0] * (T + 1)
    lab = [0] * (T + 1)
    for p in range(P):
        for c in range(offsets[p] + 1, offsets[p + 1] + 1):
            plane[c], lab[c] = p, c - offsets[p]
    overlap = {}
    for a, b, n in np.asarray(rows).reshape(-1, 3).tolist():
        overlap[(a, b)] = overlap[(b, a)] = n
    comps = [list(range(offsets[p] + 1, offsets[p + 1] + 1)) for p in range(P)]
    if P > 1:
        for order in (list(range(P)), list(range(P - 1, -1, -1))):
            newind = max(lab[1:], default=0) + (without == "newind")
            for i in range(1, P):
                A, B = comps[order[i - 1]], comps[order[i]]
                before = [c for p in order[:i] for c in comps[p]]
                for u in sorted({lab[c] for c in A}):
                    count = {}
                    for c in A:
                        if lab[c] != u:
                            continue
                        for d in B:
                            if (c, d) in overlap and (lab[d] != u or without == "same"):
                                count[lab[d]] = count.get(lab[d], 0) + overlap[(c, d)]
                    if not count:
                        continue
                    best = max(count.values())
                    to_replace = (max if without == "tie" else min)(k for k, v in count.items() if v == best)
                    for c in before:
                        if lab[c] == u:
                            lab[c] = newind
                    for d in B:
                        if lab[d] == to_replace:
                            lab[d] = newind
                    newind += 1
    return np.array(lab, dtype=np.int32)
