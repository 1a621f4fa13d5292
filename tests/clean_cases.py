"""Not a test: a scipy / numpy restatement of ``lib.morphology.label_components`` and ``utils.clean.clean`` (DESIGN.md
section 26), and the volumes the tests run them on.  Written from the definition, not from the implementation: per id
``scipy.ndimage.label(mask == id, generate_binary_structure(3, k))`` with the pieces sorted by first voxel; holes from
``label(out == 0)`` with the 6-structure, a face test, and the ids in a one-step dilation of the pocket."""
import numpy as np
from scipy import ndimage as ndi

TILE = (4, 8, 64)                     # the labelling kernel's tile (x, y, z)
CROSSING = (11, 19, 150)              # crosses tile faces, edges and corners at least twice on every axis, with a remainder
COLUMNS = ("value", "voxels", "first_voxel", "border_bits", "min_neighbour_id", "max_neighbour_id")
REPORT_FIELDS = ("instances_in", "pieces", "ids_in_pieces", "pieces_removed", "ids_added", "ids_removed_small",
                 "ids_removed_border", "holes_filled", "holes_ambiguous", "voxels_cleared", "voxels_filled", "instances_out")


def structure(connectivity):
    return ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


def _pieces_of(binary, connectivity):
    """[(first voxel, flat indices)] of the pieces of a boolean volume, in scipy's order (= by first voxel)."""
    lab, n = ndi.label(binary, structure(connectivity))
    flat = lab.reshape(-1)
    order = np.argsort(flat, kind="stable")
    cuts = np.searchsorted(flat[order], np.arange(1, n + 2))
    return [(int(order[cuts[k]]), order[cuts[k]:cuts[k + 1]]) for k in range(n)]


def _border_bits(idx, shape):
    x, y, z = np.unravel_index(idx, shape)
    bits = 0
    for b, (c, n) in enumerate(((x, shape[0]), (y, shape[1]), (z, shape[2]))):
        bits |= (1 << (2 * b)) * bool((c == 0).any()) | (2 << (2 * b)) * bool((c == n - 1).any())
    return bits


def _neighbour_ids(idx, mask):
    """the positive values among the 6-neighbours of the voxels ``idx``: a one-step dilation of the pocket with the
    6-structure, done in the pocket's box grown by one voxel (thousands of pockets, each a few voxels)"""
    c = np.stack(np.unravel_index(idx, mask.shape))
    lo = np.maximum(c.min(1) - 1, 0)
    hi = np.minimum(c.max(1) + 2, mask.shape)
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    pocket = np.zeros(tuple(hi - lo), bool)
    pocket[tuple(c - lo[:, None])] = True
    v = mask[box][ndi.binary_dilation(pocket, structure(6)) & ~pocket]
    return np.unique(v[v > 0])


def ref_label_components(mask, connectivity=6, background=False):
    """(piece map int32, table int64 (P, 6)) as ``label_components`` defines them."""
    mask = np.asarray(mask).astype(np.int64)
    pieces = []
    if background:
        pieces = [(f, idx, 0) for f, idx in _pieces_of(mask == 0, 6)]
    else:
        for u in np.unique(mask[mask > 0]):
            pieces += [(f, idx, int(u)) for f, idx in _pieces_of(mask == u, connectivity)]
    pieces.sort(key=lambda p: p[0])
    out = np.zeros(mask.shape, np.int32)
    table = np.zeros((len(pieces), 6), np.int64)
    for k, (first, idx, value) in enumerate(pieces):
        out.reshape(-1)[idx] = k + 1
        near = _neighbour_ids(idx, mask) if background else np.zeros(0, np.int64)
        table[k] = (value, idx.size, first, _border_bits(idx, mask.shape),
                    near.min() if near.size else 0, near.max() if near.size else 0)
    return out, table


def ref_clean(mask, components="keep", connectivity=6, min_voxels=0, clear_border=False, fill_holes=False,
              renumber=False):
    """(cleaned int64 array, report dict) by the five steps of ``clean``, one id at a time."""
    mask = np.asarray(mask).astype(np.int64)
    out = mask.copy()
    rep = dict.fromkeys(REPORT_FIELDS, 0)
    ids = np.unique(mask[mask > 0])
    rep["instances_in"] = int(ids.size)
    spare = []                                               # (first voxel, indices) of the pieces an id does not keep
    for u in ids:
        pieces = _pieces_of(mask == u, connectivity)
        rep["pieces"] += len(pieces)
        rep["ids_in_pieces"] += len(pieces) > 1
        best = max(range(len(pieces)), key=lambda k: (pieces[k][1].size, -pieces[k][0]))
        spare += [p for k, p in enumerate(pieces) if k != best]
    spare.sort(key=lambda p: p[0])
    if components == "largest":
        for _, idx in spare:
            out.reshape(-1)[idx] = 0
        rep["pieces_removed"] = len(spare)
    elif components == "split":
        top = int(ids.max()) if ids.size else 0
        for k, (_, idx) in enumerate(spare):
            out.reshape(-1)[idx] = top + 1 + k
        rep["ids_added"] = len(spare)
    for u in np.unique(out[out > 0]):
        if (out == u).sum() < min_voxels:
            out[out == u] = 0
            rep["ids_removed_small"] += 1
    axes = (clear_border,) * 3 if isinstance(clear_border, bool) else tuple(clear_border)
    for u in np.unique(out[out > 0]):
        m = out == u
        faces = ((m[0].any() or m[-1].any()), (m[:, 0].any() or m[:, -1].any()), (m[:, :, 0].any() or m[:, :, -1].any()))
        if any(f and a for f, a in zip(faces, axes)):
            out[m] = 0
            rep["ids_removed_border"] += 1
    rep["voxels_cleared"] = int(((mask > 0) & (out == 0)).sum())
    if fill_holes:
        before = out.copy()
        for _, idx in _pieces_of(before == 0, 6):
            if _border_bits(idx, mask.shape):
                continue
            near = _neighbour_ids(idx, before)
            if near.size == 1:
                out.reshape(-1)[idx] = near[0]
                rep["holes_filled"] += 1
                rep["voxels_filled"] += int(idx.size)
            else:
                rep["holes_ambiguous"] += 1
    rep["instances_out"] = int(np.unique(out[out > 0]).size)
    if renumber:
        flat = out.reshape(-1)
        seen, first = np.unique(flat, return_index=True)
        seen, first = seen[seen > 0], first[seen > 0]
        lut = {int(u): k + 1 for k, u in enumerate(seen[np.argsort(first)])}
        out = np.array([lut.get(int(v), 0) for v in flat], np.int64).reshape(out.shape)
    return out, {k: int(v) for k, v in rep.items()}


# ---- case volumes ----

def serpentine(shape=CROSSING, value=3):
    """a one-voxel-wide path through many tiles: in every other x plane every other y row runs the length of z and is
    joined to the next row by one voxel at alternating ends; the planes are joined by one voxel at alternating corners.
    One piece at every connectivity, and its root, voxel 0, is far from most of its voxels."""
    X, Y, Z = shape
    m = np.zeros(shape, np.int32)
    rows = list(range(0, Y, 2))
    for xi, x in enumerate(range(0, X, 2)):
        for yi, y in enumerate(rows):
            m[x, y, :] = value
            if yi + 1 < len(rows):
                m[x, y + 1, (Z - 1) if yi % 2 == 0 else 0] = value
        if x + 2 < X:
            m[x + 1, rows[-1] if xi % 2 == 0 else 0, (Z - 1) if xi % 2 == 0 else 0] = value
    return m


def u_shape(shape=CROSSING):
    """a U, extruded along y: two arms along x, tiles apart in z, joined only at the last x; the first raster voxel is in
    the arm at low z.  A lone voxel between the arms comes later in raster order than the U's first voxel and earlier than
    the second arm's, so it must get number 2 and the whole U number 1."""
    X, Y, Z = shape
    m = np.zeros(shape, np.int32)
    lo, hi = 2, Z - 3
    m[:, 1:Y - 1, lo] = 7
    m[:, 1:Y - 1, hi] = 7
    m[X - 1, 1:Y - 1, lo:hi + 1] = 7
    m[0, 1, (lo + hi) // 2] = 7
    return m


def checkerboard(shape, value=1):
    x, y, z = np.indices(shape)
    return (((x + y + z) % 2 == 0) * value).astype(np.int32)


def edge_contact(shape=CROSSING):
    """a 3-D checkerboard of two ids: equal values never share a face and always share edges (two coordinates differ by
    one: the parity is the same); across a corner the other id sits.  Every voxel is a piece at 6; each id is one piece
    at 18 and at 26 -- inside the tiles and across their edges."""
    x, y, z = np.indices(shape)
    return np.where((x + y + z) % 2 == 0, 1, 2).astype(np.int32)


def corner_contact(shape=CROSSING):
    """id 1 on the voxels whose coordinates are all even or all odd, id 2 on the rest: two voxels of id 1 touch across
    a corner or not at all, so id 1 is all single voxels at 6 and at 18 and one piece at 26 -- also where the corner is
    a corner of four or eight tiles."""
    x, y, z = np.indices(shape)
    one = ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)) | ((x % 2 == 1) & (y % 2 == 1) & (z % 2 == 1))
    return np.where(one, 1, 2).astype(np.int32)


def sparse_noise(shape, seed, ids=(0, 1, 2, 3)):
    rng = np.random.default_rng(seed)
    return np.asarray(ids, np.int64)[rng.integers(0, len(ids), shape)]


def blob(shape=(20, 22, 18), seed=0, threshold=0.5, value=1):
    """smoothed noise above a threshold: bodies with pockets and specks"""
    rng = np.random.default_rng(seed)
    f = ndi.gaussian_filter(rng.random(shape), 1.0)
    f = (f - f.min()) / (f.max() - f.min())
    return ((f > threshold) * value).astype(np.int32)


def nested_shells():
    """13^3: a shell of id 5, a gap, a shell of id 9 with a one-voxel cavity"""
    m = np.zeros((13, 13, 13), np.int32)
    m[1:12, 1:12, 1:12] = 5
    m[3:10, 3:10, 3:10] = 0
    m[5:8, 5:8, 5:8] = 9
    m[6, 6, 6] = 0
    return m


def cavity_with_speck():
    """a 12^3 block of id 2 with a 7^3 cavity that holds a 124-voxel body of id 3 (5^3 less one corner)"""
    m = np.zeros((14, 14, 14), np.int32)
    m[1:13, 1:13, 1:13] = 2
    m[3:10, 3:10, 3:10] = 0
    m[4:9, 4:9, 4:9] = 3
    m[4, 4, 4] = 0
    return m


def diagonal_pocket():
    """a block with a one-voxel pocket whose only way out is a diagonal step to a notch that opens to the outside"""
    m = np.zeros((7, 7, 7), np.int32)
    m[1:6, 1:6, 1:6] = 4
    m[2, 2, 2] = 0            # the pocket
    m[1, 1, 2] = 0            # the notch: edge-adjacent to the pocket, 6-connected to the outside
    return m


def border_pocket():
    m = np.zeros((6, 7, 8), np.int32)
    m[:, 1:6, 1:7] = 6
    m[0, 3, 3] = 0            # open to the x = 0 face
    m[3, 3, 3] = 0            # enclosed
    return m


def border_bodies():
    m = np.zeros((8, 9, 10), np.int32)
    m[3:5, 3:5, 0:3] = 1      # touches only z low
    m[0:2, 6:8, 4:6] = 2      # touches x low
    m[3:5, 6:9, 4:6] = 3      # touches y high
    m[5:7, 1:3, 5:7] = 4      # touches nothing
    return m


TIE = np.array([4, 4, 4, 0, 0, 4, 4, 4, 0], np.int32).reshape(1, 1, 9)
