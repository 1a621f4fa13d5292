"""CPU references (scipy / numpy only) and seeded inputs for the tests of the Z-sharded labelling stage.

Nothing here touches the code under test: the slab formula and the halo are restated, the labelling is
``scipy.ndimage.label`` with its default face connectivity, the union is a plain union-find.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Set, Tuple

import numpy as np
import scipy.ndimage

HALO = 48           # planes kept either side of a slab (parallel.HALO; tests assert the two agree)
PAIR_CAP = 16384    # seam pairs per rank in the metadata gather (flood_fill.PAIR_CAP)
NNZ_CAP = 1 << 16   # foreground voxels per slab in the label gather at these sizes (flood_fill.label_slab)


# ----------------------------------------------------------------------------- plan
def slab_bounds(Z: int, world: int) -> List[Tuple[int, int]]:
    return [(Z * r // world, Z * (r + 1) // world) for r in range(world)]


def window_of(slab: Tuple[int, int], Z: int, world: int, halo: int = HALO) -> Tuple[int, int]:
    return (0, Z) if world == 1 else (max(0, slab[0] - halo), min(Z, slab[1] + halo))


def mask_driven(Z: int, world: int) -> List[bool]:
    """Per rank: does the slab's crop inside its window satisfy z0 % 16 == d % 16 == window % 16 == 0?"""
    out = []
    for lo, hi in slab_bounds(Z, world):
        wlo, whi = window_of((lo, hi), Z, world)
        out.append((lo - wlo) % 16 == 0 and (hi - lo) % 16 == 0 and (whi - wlo) % 16 == 0)
    return out


# ----------------------------------------------------------------------------- references
def slab_labels(mask: np.ndarray, world: int) -> List[np.ndarray]:
    """scipy's labelling of every slab on its own (local ids 1..k_r)."""
    return [scipy.ndimage.label(mask[:, :, lo:hi])[0].astype(np.int32) for lo, hi in slab_bounds(mask.shape[2], world)]


def slab_partition(mask: np.ndarray, world: int) -> Tuple[np.ndarray, List[int]]:
    """(whole-volume scipy labels, number of components of every slab labelled on its own)."""
    whole = scipy.ndimage.label(mask)[0].astype(np.int32)
    return whole, [int(l.max()) if l.size else 0 for l in slab_labels(mask, world)]


def _planes(labels: np.ndarray, axis: int, v: int) -> Tuple[np.ndarray, np.ndarray]:
    return np.take(labels, v, axis=axis), np.take(labels, v - 1, axis=axis)


def seam_pair_set(labels: np.ndarray, axis: int, v: int) -> Set[Tuple[int, int]]:
    """{(label at plane v, label at plane v - 1)} over the face-adjacent voxels that are both non-zero."""
    a, b = _planes(labels, axis, v)
    both = (a != 0) & (b != 0)
    return set(zip(a[both].tolist(), b[both].tolist()))


def seam_adjacent(labels: np.ndarray, axis: int, v: int) -> int:
    """Number of positions of plane v whose neighbour in plane v - 1 is non-zero too."""
    a, b = _planes(labels, axis, v)
    return int(((a != 0) & (b != 0)).sum())


def seam_runs(labels: np.ndarray, axis: int, v: int) -> int:
    """Number of adjacent positions that start a run along the plane's fastest axis (the last one): a position whose
    predecessor along that axis carries the same pair of labels is not counted."""
    a, b = _planes(labels, axis, v)
    both = (a != 0) & (b != 0)
    same = np.zeros_like(both)
    same[:, 1:] = (a[:, 1:] == a[:, :-1]) & (b[:, 1:] == b[:, :-1])
    return int((both & ~same).sum())


def min_of_component(n_ids: int, pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
    """Plain union-find over ids 0..n_ids-1: out[i] = smallest id of i's component."""
    parent = list(range(n_ids))

    def find(i: int) -> int:
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n_ids)], dtype=np.int64)


def merge_slabs(mask: np.ndarray, world: int) -> Tuple[np.ndarray, List[int], List[int], List[int]]:
    """The sharded procedure on the CPU: label every slab, shift its ids by the exclusive prefix sum of the counts,
    unite through the seam pairs of every slab boundary.  Returns (merged labels, components per slab, seam runs per
    boundary, foreground voxels per slab)."""
    slabs = slab_bounds(mask.shape[2], world)
    local = slab_labels(mask, world)
    counts = [int(l.max()) if l.size else 0 for l in local]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    glob = np.concatenate([np.where(l > 0, l.astype(np.int64) + offs[r], 0) for r, l in enumerate(local)], axis=2)
    pairs: List[Tuple[int, int]] = []
    runs = []
    for r in range(world - 1):
        v = slabs[r + 1][0]
        pairs += sorted(seam_pair_set(glob, 2, v))
        # the ranks compare LOCAL ids: the upper slab's first plane against the lower slab's last
        two = np.stack([local[r][:, :, -1], local[r + 1][:, :, 0]], axis=2)
        runs.append(seam_runs(two, 2, 1))
    lut = min_of_component(int(offs[-1]) + 1, pairs)
    return lut[glob].astype(np.int32), counts, runs, [int((l > 0).sum()) for l in local]


def partition_equal(got: np.ndarray, ref: np.ndarray) -> bool:
    """Zeros exactly where ``ref`` is zero, and a bijection between the ids of ``got`` and those of ``ref``."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or not np.array_equal(got == 0, ref == 0) or (got < 0).any():
        return False
    g, r = got.ravel().astype(np.int64), ref.ravel().astype(np.int64)
    pairs = np.unique(g * (int(r.max()) + 1) + r)
    return len(np.unique(g)) == len(pairs) == len(np.unique(r))


# ----------------------------------------------------------------------------- inputs
def serpentine(shape: Sequence[int], rng: np.random.Generator, breaks: int = 8) -> np.ndarray:
    """Bars along z at even x and even y; neighbouring bars of a row (one x) joined at alternating ends (z = 0, then
    z = Z - 1, ...), so a row is ONE snake; ``breaks`` bars are cut at a random interior voxel.  Every middle slab sees
    each bar as a component of its own: the global components are connected only through the first and the last slab."""
    X, Y, Z = shape
    m = np.zeros(shape, dtype=np.uint8)
    m[0::2, 0::2, :] = 1
    for j, y in enumerate(range(1, Y - 1, 2)):
        m[0::2, y, 0 if j % 2 == 0 else Z - 1] = 1
    xs, ys = np.arange(0, X, 2), np.arange(0, Y, 2)
    bars = rng.choice(len(xs) * len(ys), size=breaks, replace=False)
    for bar in bars:
        m[xs[bar // len(ys)], ys[bar % len(ys)], int(rng.integers(1, Z - 1))] = 0
    return m


def random_field(shape: Sequence[int], fill: float, rng: np.random.Generator) -> np.ndarray:
    return (rng.random(shape) < fill).astype(np.uint8)


def hollow_field(shape: Sequence[int], fill: float, z_low: int, z_high: int, rng: np.random.Generator) -> np.ndarray:
    """Random field in z < z_low and z >= z_high, nothing in between: the middle ranks have no component at all."""
    m = random_field(shape, fill, rng)
    m[:, :, z_low:z_high] = 0
    return m


# every input of the sharded GPU tests: name -> (builder, world sizes)
def _serp_big():
    return serpentine((32, 32, 256), np.random.default_rng(101), breaks=8)


def _serp_small():
    return serpentine((20, 18, 90), np.random.default_rng(102), breaks=3)


CASES: Dict[str, Tuple] = {
    "serpentine": (_serp_big, (2, 4, 8)),
    "serpentine_generic": (_serp_small, (3,)),
    "random30": (lambda: random_field((48, 48, 256), 0.30, np.random.default_rng(103)), (4,)),
    "random33": (lambda: random_field((48, 48, 256), 0.33, np.random.default_rng(104)), (8,)),
    "dense50": (lambda: random_field((48, 48, 128), 0.50, np.random.default_rng(105)), (2,)),
    "hollow": (lambda: hollow_field((32, 32, 256), 0.30, 70, 250, np.random.default_rng(106)), (8,)),
}
FG_OVERFLOW = ("dense50",)               # more than NNZ_CAP foreground voxels in a slab: the sync-free path must flag it
GENERIC_PATH = ("serpentine_generic",)   # slabs that are not 16-aligned: one thread per voxel
CASE_IDS = [(name, world) for name, (_, worlds) in CASES.items() for world in worlds]

_built: Dict[str, np.ndarray] = {}
_refs: Dict[Tuple[str, int], Tuple[np.ndarray, List[int]]] = {}


def case_mask(name: str) -> np.ndarray:
    """The input of a case, built once; read-only."""
    if name not in _built:
        m = CASES[name][0]()
        m.setflags(write=False)
        _built[name] = m
    return _built[name]


def case_reference(name: str, world: int) -> Tuple[np.ndarray, List[int]]:
    """:func:`slab_partition` of a case, computed once; read-only."""
    if (name, world) not in _refs:
        whole, counts = slab_partition(case_mask(name), world)
        whole.setflags(write=False)
        _refs[(name, world)] = (whole, counts)
    return _refs[(name, world)]
