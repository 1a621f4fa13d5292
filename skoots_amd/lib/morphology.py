"""``skoots.lib.morphology`` dilations on the MI355X
(reference: skoots/lib/morphology.py:155-175 ``binary_dilation``, :178-199 ``binary_dilation_2d``), and the Lee
thinning that skoots/train/generate_skeletons.py takes from scikit-image (``skeletonize``, ``thin_objects``) with the
skeletons read as graphs (``skeleton_graph``) and traced into node and branch tables
(``skeleton_branches``); ``label_edt`` is the exact Euclidean distance
transform of every instance of a label volume, which the reference does not have, and
``label_components`` the connected pieces of every instance at once, which it does not have
either, nor ``nearest_label``, the nearest instance of every voxel and its distance, nor
``local_thickness``, the radius of the largest ball inside the instance that holds the voxel, nor
``geodesic_assign``, the nearest seed of every voxel along paths inside its instance, nor
``pool``, one level of a multiscale pyramid by mode, mean or max, nor ``resample`` (section 37).

``filter_volume`` is the exact rank filter (median, min, max, any rank) and the exact integer tap
filter (box mean, Gaussian) in front of the network, and under the reference's names ``median_filter``, ``dilate`` and
``binary_erosion`` (skoots/lib/morphology.py:131-152, 202-232) run on float32 tensors with zero padding.  The
reference's ``mean_filter`` and ``gauss_filter`` on float tensors are not built: a float sum has no defined order, so
nothing exact could be promised; use ``filter_volume(..., "mean" | "gauss")`` on the integer image.

``equalize`` transforms the grey values themselves, driven by histograms: percentile stretch,
histogram equalisation (global, and contrast-limited in tiles) and histogram matching, made of ``tile_histograms``, the
pure table builders ``stretch_lut`` / ``equalize_lut`` / ``match_lut`` and ``apply_tile_luts``.  Not in the reference."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _ffi


def _max_filter(image: Tensor, radius) -> Tensor:
    if image.ndim != 5:
        raise ValueError("image must be (B, C, X, Y, Z)")
    _ffi.require_gpu(image, "image")
    x = image.float() if image.dtype != torch.float32 else image
    out = torch.empty_like(x)
    b, c, w, h, d = x.shape
    for i in range(b * c):
        src = x.view(b * c, w, h, d)[i]
        dst = out.view(b * c, w, h, d)[i]
        _ffi.check(_ffi.lib.sk_max_filter3d(_ffi.ptr(src), _ffi.ptr(dst), w, h, d, *radius,
                                            _ffi.stream_ptr(x.device)))
    return out


def binary_dilation(image: Tensor) -> Tensor:
    """3x3x3 max filter with zero padding on a (B, C, X, Y, Z) tensor."""
    return _max_filter(image, (1, 1, 1))


def binary_dilation_2d(image: Tensor) -> Tensor:
    """3x3x1 max filter with zero padding on a (B, C, X, Y, Z) tensor."""
    return _max_filter(image, (1, 1, 0))


THIN_ERRORS = {1: "a re-check round bound was hit", 2: "the pass bound was hit"}


def _thin(labels: Tensor, ids, boxes, thin: bool = True):
    """The ``sk_skeletonize`` launch of ``thin_objects``, ``skeleton_graph`` and ``skeleton_branches``: ``None`` without
    a box, else ``(boxes, boxes_p, n, work, nbytes, counts)`` and ``stats``, both still on the device, the skeletons in
    ``work``.  ``thin=False`` is the ``sk_skeleton_pack`` launch instead: ``labels`` holds skeletons already."""
    if labels.ndim != 3:
        raise ValueError("labels must be (X, Y, Z)")
    _ffi.require_gpu(labels, "labels")
    if labels.dtype != torch.int32:
        raise ValueError("labels must be int32")
    dev = labels.device
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 6))
    n = boxes.shape[0]
    if n == 0:
        return None
    ids_d = torch.as_tensor(np.asarray(ids, dtype=np.int32).reshape(-1), device=dev)
    if ids_d.numel() != n:
        raise ValueError("one id per box")
    boxes_p = boxes.ctypes.data_as(_ffi.ip)
    nbytes = _ffi.lib.sk_skeletonize_workspace_bytes(boxes_p, n)
    if nbytes == 0:
        raise ValueError("every box must be non-empty: " + _ffi.last_error())
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty((n, 2), dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    X, Y, Z = labels.shape
    launch = _ffi.lib.sk_skeletonize if thin else _ffi.lib.sk_skeleton_pack
    _ffi.check(launch(_ffi.ptr(labels), X, Y, Z, _ffi.ptr(ids_d), boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes),
                      _ffi.ptr(counts), _ffi.ptr(stats), _ffi.ptr(err), _ffi.stream_ptr(dev)))
    code = int(err.item())
    if code:
        msg = "; ".join(v for k, v in THIN_ERRORS.items() if code & k)
        raise _ffi.SkootsHipError(f"sk_skeletonize: {msg} (error word {code})")
    return (boxes, boxes_p, n, work, nbytes, counts), stats    # boxes: boxes_p points into it


def _emit(thinned, want_offsets: bool = False):
    """(sum(counts), 3) int32: the skeleton voxels that ``_thin`` left in its workspace, as crop coordinates; with
    ``want_offsets`` also the (n + 1) int32 exclusive prefix sum of the counts that placed them"""
    _, boxes_p, n, work, nbytes, counts = thinned
    dev = work.device
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    points = torch.empty((total, 3), dtype=torch.int32, device=dev)
    _ffi.check(_ffi.lib.sk_skeletonize_emit(boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(offsets), total,
                                            _ffi.ptr(points), _ffi.stream_ptr(dev)))
    return (points, offsets) if want_offsets else points


def thin_objects(labels: Tensor, ids, boxes) -> Tuple[Tensor, np.ndarray, np.ndarray]:
    """Lee thinning of every object in its own crop, in one launch (one workgroup per object).

    labels (X, Y, Z) int32 on the GPU; ids: n object ids; boxes (n, 6) ints (x0, y0, z0, x1, y1, z1): object i is
    thinned in the binary crop ``labels[x0:x1, y0:y1, z0:z1] == ids[i]`` (voxels of other ids are background).
    Returns (points, counts, stats): points (sum(counts), 3) int32 on the GPU, the skeleton voxels of object 0, 1, ...
    in raster order of their crop as crop coordinates; counts (n,) int64; stats (n, 2) = passes and the most
    re-check rounds of one sub-iteration (the kernel's counters)."""
    done = _thin(labels, ids, boxes)
    if done is None:
        return (torch.zeros((0, 3), dtype=torch.int32, device=labels.device), np.zeros(0, np.int64),
                np.zeros((0, 2), np.int64))
    thinned, stats = done
    points = _emit(thinned)
    return points, thinned[5].cpu().numpy().astype(np.int64), stats.cpu().numpy().astype(np.int64)


N_GRAPH = 12    # int64 values per object of sk_skeleton_graph (checked against the library below)


def skeleton_graph(labels: Tensor, ids, boxes, want_points: bool = False):
    """The skeletons of ``thin_objects(labels, ids, boxes)`` read as graphs, on the workspace the thinning leaves them
    in: ``sk_skeletonize``, then ``sk_skeleton_graph``, then ``sk_skeletonize_emit`` when ``want_points``.

    Returns (graph, counts, points): graph (n, 12) int64 on the GPU -- skeleton voxels, voxels of degree 0 / 1 / 2 /
    >= 3, and the links (pairs of 26-neighbouring skeleton voxels, each once) by direction class (1,0,0) (0,1,0)
    (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); include/skoots_hip.h and DESIGN.md section 22 -- counts (n,) int64 as
    ``thin_objects`` gives them, and points as ``thin_objects`` gives them or ``None``."""
    assert _ffi.lib.sk_skeleton_graph_row_values() == N_GRAPH
    done = _thin(labels, ids, boxes)
    if done is None:
        dev = labels.device
        return (torch.zeros((0, N_GRAPH), dtype=torch.int64, device=dev), np.zeros(0, np.int64),
                torch.zeros((0, 3), dtype=torch.int32, device=dev) if want_points else None)
    thinned, _ = done
    _, boxes_p, n, work, nbytes, counts = thinned
    graph = torch.empty((n, N_GRAPH), dtype=torch.int64, device=work.device)
    _ffi.check(_ffi.lib.sk_skeleton_graph(boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(graph),
                                          _ffi.stream_ptr(work.device)))
    points = _emit(thinned) if want_points else None
    return graph, counts.cpu().numpy().astype(np.int64), points


N_NODE, N_BRANCH = 8, 18   # int32 values per row of sk_skeleton_branches_emit's tables (checked against the library below)


def _offsets(counts: Tensor) -> Tensor:
    out = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=out[1:])
    return out


def skeleton_branches(labels: Tensor, ids, boxes, thin: bool = True):
    """Every skeleton of ``thin_objects(labels, ids, boxes)`` traced into nodes and branches, on
    the workspace the thinning leaves them in: ``sk_skeletonize``, ``sk_skeleton_graph``, ``sk_skeletonize_emit``, then
    ``sk_skeleton_branches_count`` and ``sk_skeleton_branches_emit``.  ``thin=False`` takes ``labels`` as skeletons
    already (``sk_skeleton_pack``): object i is ``labels[box i] == ids[i]`` as it is, any binary object.

    Returns ``(graph, counts, points, nodes, branches, owner)``: graph, counts and points as ``skeleton_graph`` gives
    them with ``want_points``; nodes (Nn, 8) int32 -- object index, type (0 isolated voxel, 1 endpoint, 2 junction, 3
    ring anchor), voxels, internal links, first voxel (x, y, z) in the coordinates of ``labels``, branch ends attached;
    branches (Nb, 18) int32 -- object index, node rows of ends a and b, chain voxels, links by the seven direction
    classes of ``skeleton_graph``, end voxels a and b, direction code at a; owner (sum(counts)) int32, aligned with
    points -- a chain voxel's branch row, or -1 - the node row of a node voxel.  All on the GPU but counts; rows come
    object by object, nodes by first voxel and branches by (end voxel a, direction code); the same bytes on every run."""
    assert (_ffi.lib.sk_skeleton_graph_row_values(), _ffi.lib.sk_skeleton_nodes_row_values(),
            _ffi.lib.sk_skeleton_branches_row_values()) == (N_GRAPH, N_NODE, N_BRANCH)
    done = _thin(labels, ids, boxes, thin)
    dev = labels.device
    if done is None:
        empty = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        return (torch.zeros((0, N_GRAPH), dtype=torch.int64, device=dev), np.zeros(0, np.int64), empty(0, 3),
                empty(0, N_NODE), empty(0, N_BRANCH), empty(0))
    thinned, _ = done
    _, boxes_p, n, work, nbytes, counts = thinned
    graph = torch.empty((n, N_GRAPH), dtype=torch.int64, device=dev)
    stream = _ffi.stream_ptr(dev)
    _ffi.check(_ffi.lib.sk_skeleton_graph(boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(graph), stream))
    points, offsets = _emit(thinned, want_offsets=True)
    total = int(points.shape[0])
    counts_host = np.ascontiguousarray(counts.cpu().numpy().astype(np.int32))
    sbytes = int(_ffi.lib.sk_skeleton_branches_scratch_bytes(boxes_p, counts_host.ctypes.data_as(_ffi.ip), n))
    if sbytes == 0:
        raise _ffi.SkootsHipError("sk_skeleton_branches_scratch_bytes refused the counts of the thinning")
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    per_object = torch.empty((n, 2), dtype=torch.int32, device=dev)
    common = (boxes_p, n, _ffi.ptr(work), C.c_size_t(nbytes), _ffi.ptr(offsets), total, _ffi.ptr(scratch),
              C.c_size_t(sbytes))
    _ffi.check(_ffi.lib.sk_skeleton_branches_count(*common, _ffi.ptr(per_object), stream))
    if bool((per_object < 0).any()):
        raise _ffi.SkootsHipError("sk_skeleton_branches_count: the workspace does not hold the skeletons its counts name")
    node_off, branch_off = _offsets(per_object[:, 0]), _offsets(per_object[:, 1])
    n_nodes, n_branches = int(node_off[-1].item()), int(branch_off[-1].item())
    if max(n_nodes, n_branches) >= 2 ** 31:
        raise ValueError(f"{n_nodes} nodes and {n_branches} branches: rows are int32; trace fewer objects at a time")
    nodes = torch.empty((n_nodes, N_NODE), dtype=torch.int32, device=dev)
    branches = torch.empty((n_branches, N_BRANCH), dtype=torch.int32, device=dev)
    owner = torch.empty(total, dtype=torch.int32, device=dev)
    node_off, branch_off = node_off.to(torch.int32), branch_off.to(torch.int32)
    _ffi.check(_ffi.lib.sk_skeleton_branches_emit(*common, _ffi.ptr(node_off), _ffi.ptr(branch_off), n_nodes, n_branches,
                                                  _ffi.ptr(nodes), _ffi.ptr(branches), _ffi.ptr(owner), stream))
    return graph, counts_host.astype(np.int64), points, nodes, branches, owner


def squared_spacing(spacing) -> Tuple[float, float, float]:
    """(wx, wy, wz) = (sx sx, sy sy, sz sz) in float64, the weights of the distance kernels: the spacing must be three
    positive finite numbers whose squares are positive and finite too."""
    s = tuple(float(v) for v in (spacing.detach().cpu().tolist() if isinstance(spacing, Tensor) else spacing))
    if len(s) != 3 or not all(0 < v < float("inf") for v in s) or not all(0 < v * v < float("inf") for v in s):
        raise ValueError(f"spacing must be three positive finite numbers (x, y, z), got {spacing}")
    return s[0] * s[0], s[1] * s[1], s[2] * s[2]


def check_transform_shape(shape, what: str) -> None:
    """The guard of the distance transforms (``what`` names one): d^2 must stay exact in float64."""
    X, Y, Z = (int(v) for v in shape)
    if max(X, Y, Z) > 2 ** 26 or X * Y * Z >= 2 ** 62:
        raise ValueError(f"a volume of shape {(X, Y, Z)} is too large for {what}: every extent must stay at or below "
                         "2^26 and X*Y*Z below 2^62")


def label_edt(labels: Tensor, spacing=(1.0, 1.0, 1.0), closed: bool = False, rows=None) -> Tuple[Tensor, Tensor]:
    """Exact squared Euclidean distance transform of every instance of an (X, Y, Z) or (1, X, Y, Z) integer device
    tensor at the voxel spacing ``spacing`` (sx, sy, sz): ``(dist2, row_max)``, both float64 on the device.

    ``dist2`` (X, Y, Z): for a voxel of a positive id, the squared distance between voxel centres to the nearest voxel
    that is not of that id -- background or another instance alike -- and 0 on the other voxels; ``row_max`` (N): the
    largest ``dist2`` of every positive id in ascending order, the rows of ``validate.lib.instance_sums``.  The value
    is ``fl(wx dx^2 + fl(wy dy^2 + wz dz^2))`` with ``wx = sx * sx`` formed in float64 here, minimised exactly
    (include/skoots_hip.h: sk_label_edt), the same on every run; at integer-valued spacings ``dist2.sqrt()`` equals
    ``scipy.ndimage.distance_transform_edt(labels == id, sampling=spacing)`` bit for bit on the voxels of every id.

    ``closed=False`` is scipy's meaning: only voxels of the volume count, and an id that is the only value of the whole
    volume gets ``inf``.  ``closed=True`` measures the volume padded with one layer of background.  ``rows`` is
    ``validate.lib.id_rows(labels)`` when the caller already has it."""
    from ..validate.lib import _Rows
    m = _Rows(labels, rows)
    w = squared_spacing(spacing)
    check_transform_shape(m.shape, "the distance transform")
    dist2 = torch.zeros(m.shape, dtype=torch.float64, device=m.dev)
    if m.empty or dist2.numel() == 0:
        return dist2, torch.zeros(0, dtype=torch.float64, device=m.dev)
    scratch = torch.empty_like(dist2)
    row_max = torch.zeros(m.N, dtype=torch.int64, device=m.dev)
    m.call(_ffi.lib.sk_label_edt, *w, int(bool(closed)), _ffi.ptr(dist2), _ffi.ptr(scratch), _ffi.ptr(row_max))
    return dist2, row_max.view(torch.float64)


def nearest_label(labels: Tensor, spacing=(1.0, 1.0, 1.0), max_distance=None, where=None, rows=None) -> Tuple[Tensor, Tensor]:
    """The nearest instance of every voxel of an (X, Y, Z) or (1, X, Y, Z) integer device tensor at the voxel spacing
    ``spacing`` (sx, sy, sz): ``(nearest_id (X, Y, Z) int64, dist2 (X, Y, Z) float64)``, both on the device (DESIGN.md
    section 27; the reference has no counterpart).

    ``dist2`` is the squared distance between voxel centres to the nearest voxel of a positive id, 0 on such a voxel
    itself, and ``nearest_id`` that voxel's id.  The value is ``fl(wx dx^2 + fl(wy dy^2 + wz dz^2))`` with
    ``wx = sx * sx`` formed in float64 here, minimised exactly (include/skoots_hip.h: sk_nearest_label); among voxels at
    the same value the one the three passes z, y, x reach with the smallest coordinate wins, so the result is the same on
    every run.  At integer-valued spacings ``dist2.sqrt()`` equals ``scipy.ndimage.distance_transform_edt(labels == 0,
    sampling=spacing)`` bit for bit; scipy's nearest voxel lies at the same distance but need not be the same voxel.

    ``max_distance`` (``None`` = no limit, or a non-negative finite float d) bounds the search at ``dist2 <= fl(d d)``:
    beyond it, and in a volume without a positive id, ``dist2`` is ``inf`` and ``nearest_id`` 0.  Without a limit a voxel
    costs as many reads as the volume is long, with one about ``2 d / spacing`` per axis.  ``where`` (bool or integer
    tensor of the volume's shape on the same device, non-zero = wanted) restricts which voxels are answered: the others
    get ``inf`` and 0 unless they hold an id themselves.  It never restricts which voxels count as nearest: distances
    are Euclidean, through anything, not geodesic.  ``rows`` is ``validate.lib.id_rows(labels)`` when the caller
    already has it; sparse or huge ids go through its relabelled volume, and ``nearest_id`` still names the ids."""
    from ..validate.lib import _Rows
    m = _Rows(labels, rows)
    w = squared_spacing(spacing)
    limit2 = max_distance_squared(max_distance)
    check_transform_shape(m.shape, "the nearest-instance transform")
    dev, ids, (X, Y, Z) = m.dev, m.ids, m.shape
    if where is not None:
        if not isinstance(where, Tensor) or where.device != dev or where.is_floating_point() or where.is_complex():
            raise ValueError("where must be a bool or integer tensor on the device of labels")
        where = where[0] if where.ndim == 4 and where.shape[0] == 1 else where
        if tuple(where.shape) != (X, Y, Z):
            raise ValueError(f"where must have the volume's shape {(X, Y, Z)}, got {tuple(where.shape)}")
        where = (where != 0).to(torch.uint8).contiguous()
    dist2 = torch.full((X, Y, Z), float("inf"), dtype=torch.float64, device=dev)
    if m.empty or dist2.numel() == 0:
        return torch.zeros((X, Y, Z), dtype=torch.int64, device=dev), dist2
    nearest = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    scratch_d2, scratch_row = torch.empty_like(dist2), torch.empty_like(nearest)
    m.call(_ffi.lib.sk_nearest_label, *w, limit2, _ffi.ptr(where), _ffi.ptr(dist2), _ffi.ptr(nearest),
           _ffi.ptr(scratch_d2), _ffi.ptr(scratch_row))
    return torch.cat((ids.new_zeros(1), ids))[nearest.long()], dist2


# Box voxels (d2 tests, before the comparison decides) one ``sk_local_thickness_paint`` launch may be asked for.  The
# work of a call has no bound of its own -- every voxel of a solid 300^3 block is a centre and the block is about 10^12
# tests -- so ``local_thickness`` splits the centre list into launches of at most this many.  The value is meant to
# keep a launch well under a second on a device that others share.  It was chosen on an estimate of 3e11 tests per
# second (a test is a multiply, an add, a compare and an 8-byte load that mostly hits the cache: a tenth of the vector
# rate) and has since been held against one measurement (tools/bench_local_thickness.py on one MI355X,
# profiles/local_thickness_bench.json): 3.3e11 box voxels per second on a mask of 1 000 blobs and 2.2e11 on one of
# 8 192 small balls, both in one launch (5.9 and 26 ms).  The list is split by the upper estimate of the boxes, about
# twice their exact sum, so a full launch is 25 to 40 ms of such work.  The value stays; the result does not depend on it.
PAINT_BUDGET = 1 << 34


def paint_centres(dist2: Tensor, w) -> Tuple[Tensor, Tensor]:
    """``(centres, boxes)`` of ``local_thickness``: the flat indices (int64, raster order) of the voxels whose ball
    holds more than its own centre -- ``dist2`` finite and above ``min(w)`` -- and an upper estimate of each one's
    clipped bounding box in voxels (int64), which is used for splitting the list only."""
    X, Y, Z = (int(v) for v in dist2.shape)
    flat = dist2.reshape(-1)
    centres = torch.nonzero(torch.isfinite(flat) & (flat > min(w)))[:, 0]
    D = flat[centres]
    boxes = torch.ones_like(centres)
    for wk, E in zip(w, (X, Y, Z)):
        h = torch.sqrt(D / wk).floor().clamp_(max=float(E)).to(torch.int64) + 1     # never below the exact half-extent
        boxes *= (2 * h + 1).clamp_(max=E)
    return centres, boxes


def local_thickness(labels: Tensor, spacing=(1.0, 1.0, 1.0), closed: bool = False, rows=None, dist2=None,
                    budget: int = PAINT_BUDGET) -> Tuple[Tensor, Tensor, Tensor]:
    """Local thickness of every instance of an (X, Y, Z) or (1, X, Y, Z) integer device tensor at the voxel spacing
    ``spacing``: ``(thick2 (X, Y, Z), dist2 (X, Y, Z), row_max (N))``, all float64 on the device (DESIGN.md section 28;
    the reference has no counterpart).

    ``thick2`` is, for a voxel of a positive id, the squared radius of the largest open ball around a voxel centre that
    holds voxels of that id only and holds the voxel: ``max D2(c)`` over the voxels c with ``d2(p, c) < D2(c)``, where
    ``D2`` is ``label_edt``'s ``dist2`` and ``d2 = fl(wx dx^2 + fl(wy dy^2 + wz dz^2))`` (include/skoots_hip.h:
    sk_local_thickness_paint); 0 on the other voxels.  It is a radius between voxel centres, not a diameter, with no
    half-voxel correction, exact and the same on every run.  ``thick2 >= dist2`` everywhere and, per id, its maximum is
    ``row_max``.  In open mode an id that is alone in the volume has ``inf``, as in ``label_edt``.

    ``closed`` and ``rows`` are those of ``label_edt``.  ``dist2`` is ``label_edt``'s pair ``(dist2, row_max)`` when the
    caller already has it, in the same mode and at the same spacing; it is not modified.  Every voxel whose ball holds
    more than itself is a centre, and a centre costs its bounding box: a compact object of radius R voxels costs about
    R^6 tests, so the centre list is painted in consecutive launches of at most ``budget`` box voxels each (a centre
    whose own box is larger goes alone).  The result does not depend on ``budget``."""
    from ..validate.lib import _Rows
    budget = int(budget)
    if budget < 1:
        raise ValueError(f"budget must be a positive number of box voxels, got {budget}")
    if dist2 is None:
        m = _Rows(labels, rows)
        dist2, row_max = label_edt(m.x, spacing, closed, m.pair)
    else:
        dist2, row_max = dist2
        if not isinstance(dist2, Tensor) or not dist2.is_cuda or dist2.dtype != torch.float64 or dist2.ndim != 3:
            raise ValueError("dist2 must be label_edt's pair (dist2 (X, Y, Z) float64 on the device, row_max)")
        dist2 = dist2.contiguous()
    w = squared_spacing(spacing)
    X, Y, Z = (int(v) for v in dist2.shape)
    thick2 = dist2.clone()
    if thick2.numel() == 0:
        return thick2, dist2, row_max
    centres, boxes = paint_centres(dist2, w)
    n = int(centres.numel())
    if n == 0:
        return thick2, dist2, row_max
    dev = dist2.device
    ends = torch.cumsum(boxes, 0)                            # boxes <= X Y Z < 2^62 each; int64 holds any real list
    first, done = 0, 0                                       # done: the box voxels of the launches so far
    while first < n:
        last = int(torch.searchsorted(ends, done + budget, right=True).item())
        last = max(last, first + 1)                          # a centre whose own box exceeds the budget goes alone
        _ffi.check(_ffi.lib.sk_local_thickness_paint(_ffi.ptr(dist2), X, Y, Z, w[0], w[1], w[2],
                                                     _ffi.ptr(centres[first:last]), last - first,
                                                     _ffi.ptr(thick2), _ffi.stream_ptr(dev)))
        done, first = int(ends[last - 1].item()), last
    return thick2, dist2, row_max


def max_distance_squared(max_distance) -> float:
    """``limit2`` of ``sk_nearest_label``: ``inf`` for ``None``, else ``fl(d d)`` of a non-negative finite number."""
    if max_distance is None:
        return float("inf")
    if isinstance(max_distance, (bool, np.bool_)) or not isinstance(max_distance, (int, float, np.integer, np.floating)):
        raise ValueError(f"max_distance must be None or a non-negative finite number, got {max_distance!r}")
    d = float(max_distance)
    if not 0 <= d < float("inf"):
        raise ValueError(f"max_distance must be None or a non-negative finite number, got {max_distance!r}")
    return d * d


N_PIECE_COLS = 6            # int64 values per piece of sk_component_table (checked against the library below)
PIECE_COLUMNS = ("value", "voxels", "first_voxel", "border_bits", "min_neighbour_id", "max_neighbour_id")
CONNECTIVITIES = (6, 18, 26)
MAX_PIECE_VOXELS = 2 ** 31  # sk_label_components: parents are int32 voxel indices


def check_piece_shape(shape) -> None:
    """The library's guard, applied before anything touches the device."""
    X, Y, Z = (int(v) for v in shape)
    if X * Y * Z >= MAX_PIECE_VOXELS:
        raise ValueError(f"a volume of shape {(X, Y, Z)} is too large to label: X*Y*Z must stay below 2^31, the parents "
                         "of the labelling are int32 voxel indices")


def _label_pieces(a: Tensor, connectivity: int, which: int) -> Tuple[Tensor, Tensor]:
    """``sk_label_components`` + ``sk_component_table`` on the contiguous int32 device volume ``a``: (piece map, rows)."""
    assert _ffi.lib.sk_component_table_row_values() == N_PIECE_COLS
    X, Y, Z = (int(v) for v in a.shape)
    dev = a.device
    piece = torch.zeros((X, Y, Z), dtype=torch.int32, device=dev)
    if piece.numel() == 0:
        return piece, torch.zeros((0, N_PIECE_COLS), dtype=torch.int64, device=dev)
    parent = torch.empty_like(piece)
    nbytes = int(_ffi.lib.sk_label_components_workspace_bytes(X, Y, Z))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _ffi.check(_ffi.lib.sk_label_components(_ffi.ptr(a), X, Y, Z, connectivity, which, _ffi.ptr(parent), _ffi.ptr(piece),
                                            _ffi.ptr(count), _ffi.ptr(work), C.c_size_t(nbytes), _ffi.stream_ptr(dev)))
    P = int(count.item())
    table = torch.empty((P, N_PIECE_COLS), dtype=torch.int64, device=dev)
    _ffi.check(_ffi.lib.sk_component_table(_ffi.ptr(a), _ffi.ptr(piece), X, Y, Z, P, _ffi.ptr(table),
                                           _ffi.stream_ptr(dev)))
    return piece, table


def label_components(labels: Tensor, connectivity: int = 6, background: bool = False, rows=None) -> Tuple[Tensor, Tensor]:
    """The connected pieces of every instance of an (X, Y, Z) or (1, X, Y, Z) integer device tensor at once:
    ``(piece_map, table)``, both on the device (the reference has no counterpart).

    Two voxels belong to one piece when a chain of neighbours of the same id joins them, at ``connectivity`` 6, 18 or 26.
    ``piece_map`` (X, Y, Z) int32 numbers the pieces of all ids together, 1..P by their first voxel in C order over the
    whole volume, and is 0 on the background: for a mask of one id it is ``scipy.ndimage.label(mask,
    generate_binary_structure(3, k))[0]``.  ``table`` (P, 6) int64 has one row per piece, ``PIECE_COLUMNS``: the id, its
    voxels, its first voxel ``(x Y + y) Z + z``, six bits for the faces of the volume it touches (x low, x high, y low,
    y high, z low, z high) and two zeros.

    ``background=True`` labels the zero voxels instead, always 6-connected whatever ``connectivity`` says (as
    ``scipy.ndimage.binary_fill_holes`` sees the background); the last two columns are then the smallest and the largest
    positive id among the 6-neighbours of the piece's voxels, both 0 without one: a piece that touches no face and has
    ``min == max`` is a hole of that id.

    The numbers are exact and the same on every run.  Negative values raise ``ValueError``; ``X*Y*Z`` must stay below
    2^31.  ``rows`` is ``validate.lib.id_rows(labels)`` when the caller already has it; sparse or huge ids go through its
    relabelled volume, and the ``value`` column still names the ids themselves."""
    from ..validate.lib import _Rows
    if connectivity not in CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    m = _Rows(labels, rows, check_piece_shape, "labels", nonnegative=True)
    # no positive id: one call on the zeros themselves
    a = torch.zeros(m.shape, dtype=torch.int32, device=m.dev) if m.empty else m.a
    piece, table = _label_pieces(a, int(connectivity), 0 if background else 1)
    if m.N and int(m.ids[-1].item()) != m.max_id and table.shape[0]:
        # _id_rows relabelled the mask: `a` holds the rows 1..N, and the columns that name ids hold rows
        back = torch.cat((m.ids.new_zeros(1), m.ids))
        for col in (0, 4, 5):
            table[:, col] = back[table[:, col]]
    return piece, table


GEODESIC_TILE = (4, 8, 64)  # the workgroup's tile of sk_geodesic_rounds
GEODESIC_BATCH = 8          # rounds launched between two looks at the device's counters
_INT32_MAX = 2 ** 31 - 1


def geodesic_costs(costs) -> Tuple[int, int, int]:
    """(cx, cy, cz) of ``geodesic_assign``: three integers in 1..255."""
    try:
        c = tuple(costs.detach().cpu().tolist() if isinstance(costs, Tensor) else costs)
    except TypeError:
        c = ()
    if len(c) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 1 <= v <= 255
                              for v in c):
        raise ValueError(f"costs must be three integers in 1..255 (x, y, z), got {costs!r}")
    return tuple(int(v) for v in c)


def geodesic_max_cost(max_cost) -> int:
    """``max_cost`` of ``sk_geodesic_rounds``: -1 for ``None``, else a non-negative integer (above int32: no limit)."""
    if max_cost is None:
        return -1
    if isinstance(max_cost, (bool, np.bool_)) or not isinstance(max_cost, (int, np.integer)) or max_cost < 0:
        raise ValueError(f"max_cost must be None or a non-negative integer, got {max_cost!r}")
    return min(int(max_cost), _INT32_MAX)


def check_geodesic_shape(shape, costs=(1, 1, 1)) -> None:
    """The library's guard, applied before anything touches the device: voxel indices and path costs stay in int32."""
    X, Y, Z = (int(v) for v in shape)
    if X * Y * Z >= 2 ** 31 or max(costs) * X * Y * Z >= 2 ** 31:
        raise ValueError(f"a volume of shape {(X, Y, Z)} at costs {tuple(costs)} is too large for the geodesic assignment: "
                         "max(costs)*X*Y*Z must stay below 2^31, the cost of a path is an int32")


def geodesic_tiles(shape) -> int:
    """The tiles of ``GEODESIC_TILE`` that cover a volume: the workgroups of one round."""
    return int(np.prod([-(-int(n) // t) for n, t in zip(shape, GEODESIC_TILE)]))


def geodesic_round_bound(shape) -> int:
    """Rounds that always suffice: ``X Y Z + 1``.  Every round before the last settles for good at least the unsettled
    voxel with the smallest true key (its predecessor on a shortest path has a smaller key and is settled), so the
    voxels bound the rounds that change something, and one more finds nothing to change.  The rounds a volume really
    takes are the tiles its longest shortest path crosses, re-entries counted."""
    return int(np.prod([int(n) for n in shape])) + 1


def geodesic_assign(labels: Tensor, seeds: Tensor, costs=(1, 1, 1), max_cost=None, rows=None,
                    stats=None) -> Tuple[Tensor, Tensor]:
    """Hands every voxel of an instance to the seed that is nearest along paths inside the instance:
    ``(owner, cost)``, both (X, Y, Z) int32 on the device (the reference has no counterpart).

    ``labels`` and ``seeds`` are integer device tensors of one shape, (X, Y, Z) or (1, X, Y, Z); ``costs = (cx, cy, cz)``
    are integers in 1..255.  A path is a chain of 6-neighbours that all hold the same positive ``labels`` value; its cost
    is the sum of its steps, ``cx`` for a step along x, and so on.  For every voxel v with ``labels[v] > 0``, ``cost[v]``
    is the smallest path cost to v from any voxel that holds a seed (``seeds > 0``), and ``owner[v]`` the smallest
    ``seeds`` value among the seeds that attain it.  A seed voxel has cost 0.  A voxel that no seed of its own value
    reaches has ``owner = 0`` and ``cost = -1``, and so has the background.  With ``max_cost`` (a non-negative integer) a
    voxel further away counts as unreached.  Each voxel has a neighbour of the same owner one step nearer, so the voxels
    an owner gets inside an instance are one 6-connected piece whenever its seed voxels there are.

    The numbers are exact and the same on every run, whatever the order of execution: include/skoots_hip.h has the
    fixed-point form.  Negative values in either volume, ``seeds`` beyond int32 and ``max(costs)*X*Y*Z >= 2^31`` raise
    ``ValueError`` before a kernel runs.  An empty volume, one without a positive label and one without a seed give
    ``owner = 0`` and ``cost = -1`` everywhere.  ``rows`` is ``validate.lib.id_rows(labels)`` when the caller already has
    it; only which voxels hold the same value matters, so sparse or huge ids go through its relabelled volume.

    The host launches rounds in batches of ``GEODESIC_BATCH`` and reads the batch's counters once; it stops after a round
    that changed nothing and raises ``SkootsHipError`` -- never a partial result -- should ``geodesic_round_bound``
    rounds not suffice.  ``stats`` (a dict, optional) receives ``rounds`` (the rounds that changed a key), ``launched``,
    ``bound`` and ``tiles``."""
    from ..validate.lib import _Rows, _as_volume
    costs = geodesic_costs(costs)
    limit = geodesic_max_cost(max_cost)
    m = _Rows(labels, rows, lambda shape: check_geodesic_shape(shape, costs), "labels", nonnegative=True)
    s = _as_volume(seeds, "seeds")
    if tuple(s.shape) != m.shape or s.device != m.dev:
        raise ValueError(f"seeds must have the shape {m.shape} of labels and live on its device, got {tuple(s.shape)} on "
                         f"{s.device}")
    lo, hi = (int(s.min().item()), int(s.max().item())) if s.numel() else (0, 0)
    if lo < 0 or hi > _INT32_MAX:
        raise ValueError(f"seeds must lie in 0..2^31 - 1 (owners are int32), got values from {lo} to {hi}")
    X, Y, Z = m.shape
    dev = m.dev
    owner = torch.zeros((X, Y, Z), dtype=torch.int32, device=dev)
    cost = torch.full((X, Y, Z), -1, dtype=torch.int32, device=dev)
    info = dict(rounds=0, launched=0, bound=geodesic_round_bound(m.shape), tiles=geodesic_tiles(m.shape))
    if stats is not None:
        stats.update(info)
    if m.empty or owner.numel() == 0 or hi == 0:
        return owner, cost
    s = s.to(torch.int32).contiguous()
    n = owner.numel()
    tiles = int(_ffi.lib.sk_geodesic_tiles(X, Y, Z))
    if tiles != info["tiles"]:
        raise _ffi.SkootsHipError(f"sk_geodesic_tiles: {tiles} tiles, expected {info['tiles']}: " + _ffi.last_error())
    batch = min(GEODESIC_BATCH, int(_ffi.lib.sk_geodesic_max_rounds()))
    keys = torch.empty((2, n), dtype=torch.int64, device=dev)
    flags = torch.empty(2 * tiles, dtype=torch.int32, device=dev)
    words = torch.empty(1 + batch, dtype=torch.int32, device=dev)           # the error word, then a counter per round
    stream = _ffi.stream_ptr(dev)
    _ffi.check(_ffi.lib.sk_geodesic_init(_ffi.ptr(m.a), _ffi.ptr(s), X, Y, Z, _ffi.ptr(keys[0]), _ffi.ptr(flags),
                                         _ffi.ptr(words), stream))
    launched, rounds, done = 0, 0, False
    while not done and launched < info["bound"]:
        k = min(batch, info["bound"] - launched)
        _ffi.check(_ffi.lib.sk_geodesic_rounds(_ffi.ptr(m.a), X, Y, Z, *costs, limit, _ffi.ptr(keys[0]), _ffi.ptr(keys[1]),
                                               _ffi.ptr(flags), launched, k, _ffi.ptr(words[1:]), stream))
        host = words.cpu().tolist()                                          # the one read-back of the batch
        if host[0]:
            raise ValueError("labels or seeds hold a negative value: ids are positive and 0 is the background")
        launched += k
        for c in host[1:1 + k]:
            if c == 0:
                done = True
                break
            rounds += 1
    info.update(rounds=rounds, launched=launched)
    if stats is not None:
        stats.update(info)
    if not done:
        raise _ffi.SkootsHipError(f"geodesic_assign: {launched} rounds and keys still fall; the bound is "
                                  f"{info['bound']}.  No result is returned")
    # round r wrote keys[1] when r is even; after a round without a change both copies hold the answer
    final = keys[1 if (launched - 1) % 2 == 0 else 0]
    _ffi.check(_ffi.lib.sk_geodesic_finish(_ffi.ptr(final), n, _ffi.ptr(owner), _ffi.ptr(cost), stream))
    return owner, cost


def skeletonize(image: Tensor) -> Tensor:
    """Lee thinning of one 3-D binary volume on the GPU: ``skimage.morphology.skeletonize(image, method="lee") != 0``
    (scikit-image 0.18.3), as a bool tensor of the same shape.  Non-zero voxels are foreground."""
    if image.ndim != 3:
        raise ValueError("image must be a 3-D volume")
    _ffi.require_gpu(image, "image")
    labels = (image != 0).to(torch.int32).contiguous()
    X, Y, Z = labels.shape
    out = torch.zeros((X, Y, Z), dtype=torch.bool, device=image.device)
    if labels.numel() == 0:
        return out
    points, _, _ = thin_objects(labels, [1], [(0, 0, 0, X, Y, Z)])
    if points.shape[0]:
        p = points.long()
        out[p[:, 0], p[:, 1], p[:, 2]] = True
    return out


# ---- one level of a multiscale pyramid ----

POOL_HOW = {"mode": 0, "mean": 1, "max": 2}     # SK_POOL_MODE / _MEAN / _MAX of include/skoots_hip.h
_SK_U16 = 5                                     # SK_U16: the dtype code sk_pool_volume and sk_resample_volume take
_POOL_SIGNED = (torch.int8, torch.int16, torch.int32, torch.int64)


def pool_factors(factors) -> Tuple[int, int, int]:
    """(fx, fy, fz) of ``pool``: three integers, each 1 or 2, not all 1."""
    try:
        f = tuple(factors)
    except TypeError:
        raise ValueError(f"factors must be three integers (fx, fy, fz), each 1 or 2, got {factors!r}") from None
    if len(f) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in (1, 2) for v in f):
        raise ValueError(f"factors must be three integers (fx, fy, fz), each 1 or 2, got {factors!r}")
    f = tuple(int(v) for v in f)
    if f == (1, 1, 1):
        raise ValueError("factors (1, 1, 1) pool nothing: at least one factor must be 2")
    return f


def check_pool_volume(volume, how: str, name: str = "volume") -> Tuple[int, int, int]:
    """What ``pool`` takes, checked on the tensor's description alone, before any device is touched; the (X, Y, Z) of it.
    ``how="mode"``: int32, int16 or uint8.  ``how="mean"``: uint8 or uint16, or a signed integer dtype under the
    convention of ``validate.lib.instance_intensity`` (values in 0 .. 65535, checked when it is pooled).  ``how="max"``:
    uint8 or uint16.  Float volumes are refused by name."""
    if how not in POOL_HOW:
        raise ValueError(f"how = {how!r}, must be 'mode', 'mean' or 'max'")
    if not isinstance(volume, Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(volume).__name__}")
    dt = volume.dtype
    if dt.is_floating_point or dt.is_complex or dt == torch.bool:
        raise TypeError(f"{name} is {dt}: float, complex and bool volumes are not pooled, the reductions are exact integer "
                        "work (labels int32 / int16 / uint8, images uint8 / uint16)")
    u16 = getattr(torch, "uint16", torch.uint8)
    allowed = {"mode": (torch.int32, torch.int16, torch.uint8), "mean": (torch.uint8, u16) + _POOL_SIGNED,
               "max": (torch.uint8, u16)}[how]
    if dt not in allowed:
        raise TypeError(f"{name} is {dt}: how={how!r} takes " +
                        {"mode": "int32, int16 or uint8", "mean": "uint8 or uint16 (or a signed integer dtype with values "
                         "in 0 .. 65535)", "max": "uint8 or uint16"}[how])
    s = tuple(int(v) for v in volume.shape)
    s = s[1:] if len(s) == 4 and s[0] == 1 else s
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{name} has the shape {tuple(volume.shape)}: it must be (X, Y, Z) or (1, X, Y, Z) with every "
                         "extent at least 1")
    return s


def pool_source(volume: Tensor, how: str, name: str = "volume") -> Tensor:
    """The (X, Y, Z) contiguous tensor ``pool`` reads: ``volume`` without its leading 1 and, for ``how="mean"`` on a
    signed dtype, checked to lie in 0 .. 65535 and converted (int8 to uint8, the others to uint16)."""
    check_pool_volume(volume, how, name)
    v = volume[0] if volume.ndim == 4 else volume
    if how == "mean" and v.dtype in _POOL_SIGNED:
        low, top = int(v.min().item()), int(v.max().item())
        if low < 0 or top > 65535:
            raise ValueError(f"{name} is {v.dtype} with values in {low} .. {top}: only 0 .. 65535 can be averaged")
        v = v.to(torch.uint8 if v.dtype == torch.int8 else torch.uint16)
    return v.contiguous()


def _pool_host(a: np.ndarray, f, how: str, sparse: bool) -> np.ndarray:
    """The definitions of ``pool`` as numpy statements on whole arrays: the slots of every block side by side, a
    validity flag for the slots the far edge clips."""
    shape_o = tuple(-(-n // k) for n, k in zip(a.shape, f))
    padded = np.zeros(tuple(n * k for n, k in zip(shape_o, f)), dtype=a.dtype)
    padded[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    there = np.zeros(padded.shape, dtype=bool)
    there[:a.shape[0], :a.shape[1], :a.shape[2]] = True
    vals, valid = [], []
    for dx in range(f[0]):
        for dy in range(f[1]):
            for dz in range(f[2]):
                vals.append(padded[dx::f[0], dy::f[1], dz::f[2]])
                valid.append(there[dx::f[0], dy::f[1], dz::f[2]])
    wide = [v.astype(np.int64) for v in vals]
    n = sum(v.astype(np.int64) for v in valid)
    if how == "mean":
        total = sum(np.where(ok, v, 0) for v, ok in zip(wide, valid))
        return ((total + n // 2) // n).astype(a.dtype)
    if how == "max":
        low = np.iinfo(a.dtype).min
        return np.max(np.stack([np.where(ok, v, low) for v, ok in zip(wide, valid)]), axis=0).astype(a.dtype)
    best_count = np.full(shape_o, -1, dtype=np.int64)
    best = np.zeros(shape_o, dtype=np.int64)
    for v, ok in zip(wide, valid):
        count = sum(((w == v) & okw).astype(np.int64) for w, okw in zip(wide, valid))
        if sparse:
            count = np.where(v == 0, 0, count)    # a zero never outvotes; an all-zero block still gives 0
        count = np.where(ok, count, -1)
        better = (count > best_count) | ((count == best_count) & (v < best))
        best = np.where(better, v, best)
        best_count = np.where(better, count, best_count)
    return best.astype(a.dtype)


def pool(volume: Tensor, factors, how: str = "mode", sparse: bool = False) -> Tensor:
    """One level of a multiscale pyramid: an (X, Y, Z) or (1, X, Y, Z) integer tensor pooled by ``factors`` (fx, fy,
    fz), each 1 or 2 and not all 1, on the device it lives on (the reference has no counterpart).
    The result has the extents ``ceil(n / f)``, the input's rank, dtype and device.  The block of an output voxel is
    clipped at the far edge of an odd extent to the voxels that exist.

    ``how="mode"`` (int32, int16, uint8: label volumes): the value that occurs most often in the block, ties to the
    smallest value in the dtype's order; with ``sparse`` zeros are not counted unless the whole block is zero, so thin
    instances survive.  ``how="mean"`` (uint8, uint16; a signed integer image with values in 0 .. 65535 is converted as
    ``instance_intensity`` converts it): ``(sum + n // 2) // n`` with ``n`` the clipped block's voxel count.
    ``how="max"`` (uint8, uint16): the largest value.  ``sparse`` belongs to ``"mode"`` alone.

    On a device tensor this is one launch of ``sk_pool_volume`` on the current stream; on a CPU tensor the same
    definitions run as numpy statements and give the same bits.  Wrong dtypes (``TypeError``), factors, ``how`` and
    shapes (``ValueError``) are refused by name before any device is touched."""
    if how not in POOL_HOW:
        raise ValueError(f"how = {how!r}, must be 'mode', 'mean' or 'max'")
    f = pool_factors(factors)
    if sparse and how != "mode":
        raise ValueError(f"sparse leaves zeros out of the vote of how='mode' and has no meaning for how={how!r}")
    check_pool_volume(volume, how)
    v = pool_source(volume, how)
    X, Y, Z = (int(n) for n in v.shape)
    if max(X, Y, Z) > 2 ** 31 - 1 or -(-X // f[0]) * -(-Y // f[1]) > 2 ** 31 - 1:
        raise ValueError(f"volume of shape {(X, Y, Z)} is too large to pool: every extent and ceil(X / fx) * ceil(Y / fy) "
                         "must stay below 2^31")
    if not v.is_cuda:
        if v.dtype == getattr(torch, "uint16", None):
            out = torch.from_numpy(_pool_host(v.view(torch.int16).numpy().view(np.uint16), f, how, bool(sparse))
                                   .view(np.int16)).view(torch.uint16)
        else:
            out = torch.from_numpy(_pool_host(v.numpy(), f, how, bool(sparse)))
    else:
        out = torch.empty(tuple(-(-n // k) for n, k in zip((X, Y, Z), f)), dtype=v.dtype, device=v.device)
        code = _SK_U16 if v.dtype == getattr(torch, "uint16", None) else _ffi.dtype_code(v)
        _ffi.check(_ffi.lib.sk_pool_volume(_ffi.ptr(v), code, X, Y, Z, *f, POOL_HOW[how], int(bool(sparse)), _ffi.ptr(out),
                                           _ffi.stream_ptr(v.device)))
    return out.unsqueeze(0) if volume.ndim == 4 else out


# ---- exact change of grid by any ratio per axis ----

RESAMPLE_OP = {"nearest": 0, "linear": 1, "area": 2}    # SK_RESAMPLE_NEAREST / _LINEAR / _AREA of include/skoots_hip.h
RESAMPLE_HOW = ("auto", "nearest", "linear", "area")
RESAMPLE_PATHS = ("gather", "acc32", "acc64")           # SK_RESAMPLE_PATH_*: what sk_resample_path answers
_RESAMPLE_MAX_EXTENT = 2 ** 30


def resample_shape(shape, factors) -> Tuple[int, int, int]:
    """The extents ``resample`` gives an (X, Y, Z) ``shape`` at ``factors`` (fx, fy, fz), output voxels per input voxel:
    ``max(1, floor(n * f + 0.5))`` per axis."""
    try:
        s, f = tuple(int(n) for n in shape), tuple(float(v) for v in factors)
    except (TypeError, ValueError):
        raise ValueError(f"shape and factors must be three numbers each, got {shape!r} and {factors!r}") from None
    if len(s) != 3 or len(f) != 3 or min(s) < 1:
        raise ValueError(f"shape and factors must be three numbers each, every extent at least 1, got {shape!r} and "
                         f"{factors!r}")
    if not all(np.isfinite(v) and v > 0 for v in f):
        raise ValueError(f"factors must be positive and finite, got {factors!r}")
    return tuple(max(1, int(np.floor(n * v + 0.5))) for n, v in zip(s, f))


def resample_operators(src_shape, dst_shape, how: str) -> Tuple[str, str, str]:
    """The operator of every axis: ``how`` itself, or under ``"auto"`` linear where ``m >= n`` and area where ``m < n``."""
    if how not in RESAMPLE_HOW:
        raise ValueError(f"how = {how!r}, must be 'auto', 'nearest', 'linear' or 'area'")
    if how != "auto":
        return (how,) * 3
    return tuple("linear" if m >= n else "area" for n, m in zip(src_shape, dst_shape))


def check_resample(volume, shape, how: str = "auto", name: str = "volume") -> Tuple[Tuple[int, int, int], Tuple[str, str, str]]:
    """What ``resample`` takes, checked on the tensor's description alone, before any device is touched: the source
    (X, Y, Z) and the operator of every axis.  ``how="nearest"``: int32, int16, uint8 or uint16.  ``"linear"``,
    ``"area"`` and ``"auto"``: uint8 or uint16.  Float volumes are refused by name.  Also refused: an axis ratio outside
    ``n / 8 <= m <= 8 n``, an unreduced weight total ``Wx Wy Wz`` (linear ``2 m``, area ``n``, nearest 1) that reaches
    2^63 when multiplied by the dtype's largest value, extents beyond 2^30 and more than 2^31 - 1 output rows."""
    if how not in RESAMPLE_HOW:
        raise ValueError(f"how = {how!r}, must be 'auto', 'nearest', 'linear' or 'area'")
    if not isinstance(volume, Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(volume).__name__}")
    dt = volume.dtype
    if dt.is_floating_point or dt.is_complex or dt == torch.bool:
        raise TypeError(f"{name} is {dt}: float, complex and bool volumes are not resampled, the operators are exact "
                        "integer work (labels int32 / int16 / uint8, images uint8 / uint16)")
    images = (torch.uint8, torch.uint16)
    allowed = images + (torch.int32, torch.int16) if how == "nearest" else images
    if dt not in allowed:
        raise TypeError(f"{name} is {dt}: how={how!r} takes " +
                        ("int32, int16, uint8 or uint16" if how == "nearest" else "uint8 or uint16 (labels take 'nearest')"))
    s = tuple(int(v) for v in volume.shape)
    s = s[1:] if len(s) == 4 and s[0] == 1 else s
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{name} has the shape {tuple(volume.shape)}: it must be (X, Y, Z) or (1, X, Y, Z) with every "
                         "extent at least 1")
    try:
        m = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be three integers (X, Y, Z), got {shape!r}") from None
    if len(m) != 3 or min(m) < 1 or any(float(a) != float(b) for a, b in zip(m, shape)):
        raise ValueError(f"shape must be three integers (X, Y, Z), each at least 1, got {shape!r}")
    if max(s + m) > _RESAMPLE_MAX_EXTENT or m[0] * m[1] > 2 ** 31 - 1:
        raise ValueError(f"{s} -> {m} is too large to resample: every extent must stay within 2^30 and the output rows "
                         "X * Y below 2^31")
    for axis, n, k in zip("XYZ", s, m):
        if 8 * k < n or k > 8 * n:
            raise ValueError(f"the ratio of {axis}, {n} -> {k}, is outside n / 8 <= m <= 8 n: halve with pool() first, or "
                             "resample in two steps")
    ops = resample_operators(s, m, how)
    total = 1
    for n, k, op in zip(s, m, ops):
        total *= {"nearest": 1, "linear": 2 * k, "area": n}[op]
    vmax = {torch.uint8: 255, torch.uint16: 65535, torch.int16: 32767, torch.int32: 2 ** 31 - 1}[dt]
    if total * vmax >= 2 ** 63:
        raise ValueError(f"{s} -> {m} with {ops}: the weight total {total} times the largest {dt} value reaches 2^63 and "
                         "cannot be summed exactly; resample in two steps")
    return s, ops


def resample_taps(n: int, m: int, op: str):
    """The tap table of one axis as numpy arrays: ``start`` (m,), ``count`` (m,), ``weights`` (m, T) int64 with zeros
    behind ``count``, and the total ``W`` -- weights divided by their common factor, as the kernel's prologue does."""
    i = np.arange(m, dtype=np.int64)
    if op == "nearest":
        return ((2 * i + 1) * n) // (2 * m), np.ones(m, np.int64), np.ones((m, 1), np.int64), 1
    if op == "linear":
        den, num = 2 * m, (2 * i + 1) * n - m
        k0 = num // den                                      # floor: num is negative at i = 0 when m > n
        r = num - k0 * den
        one = (k0 < 0) | (k0 + 1 > n - 1) | (r == 0)
        g = int(np.gcd(np.gcd(2 * m, 2 * n), abs(n - m)))
        w = np.stack([np.where(one, den, den - r), np.where(one, 0, r)], axis=1) // g
        return np.clip(k0, 0, n - 1), np.where(one, 1, 2), w, den // g
    lo, hi = i * n, (i + 1) * n
    kb, ke = lo // m, -(-hi // m) - 1
    T = -(-n // m) + 1
    k = kb[:, None] + np.arange(T, dtype=np.int64)[None, :]
    w = np.minimum((k + 1) * m, hi[:, None]) - np.maximum(k * m, lo[:, None])
    g = int(np.gcd(n, m))
    return kb, ke - kb + 1, np.where(k <= ke[:, None], w, 0) // g, n // g


def _resample_host(a: np.ndarray, shape, ops) -> np.ndarray:
    """The definition of ``resample`` as numpy statements: one axis after the other in exact int64 sums (the product of
    the three tap lists factorises), then the one rounded division."""
    if all(op == "nearest" for op in ops):
        for axis, (n, m) in enumerate(zip(a.shape, shape)):
            a = np.take(a, resample_taps(n, m, "nearest")[0], axis=axis)
        return np.ascontiguousarray(a)
    s, W = a.astype(np.int64), 1
    for axis, (n, m, op) in enumerate(zip(a.shape, shape, ops)):
        start, count, w, total = resample_taps(n, m, op)
        acc = 0
        for t in range(w.shape[1]):
            wt = w[:, t].reshape([-1 if d == axis else 1 for d in range(3)])
            acc = acc + wt * np.take(s, np.minimum(start + t, n - 1), axis=axis)     # weight 0 behind count
        s, W = acc, W * total
    q = s // W
    return (q + (2 * (s - q * W) >= W)).astype(a.dtype)


def resample(volume: Tensor, shape=None, factors=None, how: str = "auto") -> Tensor:
    """An exactly defined change of grid by any ratio per axis: an (X, Y, Z) or (1, X, Y, Z) integer tensor brought to
    ``shape`` (three extents) or to ``resample_shape(its shape, factors)`` -- exactly one of the two is given -- on the
    device it lives on (the reference has no counterpart).  Source and result cover the same
    physical extent (pixel centres, no ``align_corners``).  The result has the input's rank, dtype and device.

    Per axis of ``n`` source and ``m`` output voxels one operator, a list of integer taps ``(k, w)`` per output index
    ``i`` with the total ``W``: ``"nearest"`` the voxel ``((2i+1) n) // (2m)`` that holds the output voxel's centre (the
    upper one for a centre on a boundary); ``"linear"`` the two voxels around the centre, ``num = (2i+1) n - m``,
    ``k0 = num // (2m)``, ``r = num - 2m k0``, taps ``(clamp(k0), 2m - r)`` and ``(clamp(k0 + 1), r)``, ``W = 2m``;
    ``"area"`` every voxel the output cell covers, weighted by the covered length in units of ``1 / m``, ``W = n``.
    ``"auto"`` (the default) is linear where ``m >= n`` and area where ``m < n``.  The output voxel is the exact quotient
    ``S / W`` of the weighted sum over the product of the three tap lists and ``W = Wx Wy Wz``, rounded to nearest,
    halves up -- ``pool(..., "mean")``'s rule, which area at even extents and factors of two reproduces.

    ``"nearest"`` takes int32, int16, uint8 and uint16 (labels keep their ids; an instance smaller than an output voxel
    can vanish), the others uint8 and uint16.  On a device tensor this is ``sk_resample_volume`` on the current stream;
    on a CPU tensor the same definition runs as numpy statements and gives the same bits.  ``check_resample`` lists what
    is refused by name (``TypeError`` for dtypes, ``ValueError`` otherwise) before any device is touched."""
    if (shape is None) == (factors is None):
        raise ValueError("resample takes exactly one of shape and factors")
    if how not in RESAMPLE_HOW:
        raise ValueError(f"how = {how!r}, must be 'auto', 'nearest', 'linear' or 'area'")
    if shape is None:
        if not isinstance(volume, Tensor):
            raise TypeError(f"volume must be a tensor, got {type(volume).__name__}")
        s = tuple(int(v) for v in volume.shape)
        shape = resample_shape(s[1:] if len(s) == 4 and s[0] == 1 else s, factors) if len(s) in (3, 4) else (0, 0, 0)
    (X, Y, Z), ops = check_resample(volume, shape, how)
    m = tuple(int(v) for v in shape)
    v = (volume[0] if volume.ndim == 4 else volume).contiguous()
    if not v.is_cuda:
        if v.dtype == torch.uint16:
            out = torch.from_numpy(_resample_host(v.view(torch.int16).numpy().view(np.uint16), m, ops)
                                   .view(np.int16)).view(torch.uint16)
        else:
            out = torch.from_numpy(_resample_host(v.numpy(), m, ops))
    else:
        code = _SK_U16 if v.dtype == torch.uint16 else _ffi.dtype_code(v)
        geometry = (code, X, Y, Z, *m, *(RESAMPLE_OP[op] for op in ops))
        nbytes = int(_ffi.lib.sk_resample_workspace_bytes(*geometry))
        if nbytes == 0:
            raise ValueError(_ffi.last_error())
        out = torch.empty(m, dtype=v.dtype, device=v.device)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
        _ffi.check(_ffi.lib.sk_resample_volume(_ffi.ptr(v), _ffi.ptr(out), *geometry, _ffi.ptr(workspace), nbytes,
                                               _ffi.stream_ptr(v.device)))
    return out.unsqueeze(0) if volume.ndim == 4 else out


def resample_path(dtype, src_shape, dst_shape, ops) -> str:
    """Which kernel ``resample`` runs for this geometry, answered on the host: ``"gather"`` (nearest on every axis),
    ``"acc32"`` (weighted sums in 32 bits) or ``"acc64"``."""
    code = {torch.uint8: 4, torch.uint16: _SK_U16, torch.int16: 2, torch.int32: 3}[dtype]
    rc = int(_ffi.lib.sk_resample_path(code, *(int(n) for n in src_shape), *(int(n) for n in dst_shape),
                                       *(RESAMPLE_OP[op] for op in ops)))
    _ffi.check(rc if rc < 0 else 0)
    return RESAMPLE_PATHS[rc]


# ---- exact rank and tap filters ----

FILTER_HOW = ("median", "min", "max", "rank", "mean", "gauss", "taps")
FILTER_BORDER = {"zero": 0, "edge": 1, "mirror": 2}     # SK_FILTER_BORDER_* of include/skoots_hip.h
FILTER_KERNELS = ("extreme", "radix", "acc32", "acc64", "network")   # SK_FILTER_PATH_*: sk_filter_path's low three bits
FILTER_METHOD = {"auto": 0, "radix": 1, "network": 2}    # SK_FILTER_METHOD_*: the selection of a rank filter
FILTER_TILE = (4, 8, 128)                                # the rank kernels' tile: rows in x, rows in y, bytes along z
FILTER_MAX_RANK_RADIUS, FILTER_MAX_TAP_RADIUS, FILTER_MAX_TAP_SUM = 2, 8, 4096
_FILTER_MAX_EXTENT = 2 ** 30
_FILTER_CODE = {torch.uint8: 4, torch.uint16: _SK_U16, torch.float32: 1}


def border_index(i: int, n: int, border: str) -> int:
    """The source index of any integer ``i`` on an axis of extent ``n``: ``"zero"`` -1 outside ``0 <= i < n`` (the sample
    is 0), ``"edge"`` ``clamp(i, 0, n - 1)``, ``"mirror"`` ``j = i mod 2n``, ``j`` if ``j < n`` else ``2n - 1 - j``
    (numpy's ``symmetric``: the edge sample repeats, reflection repeats as often as needed)."""
    if border not in FILTER_BORDER:
        raise ValueError(f"border = {border!r}, must be 'zero', 'edge' or 'mirror'")
    i, n = int(i), int(n)
    if n < 1:
        raise ValueError(f"an axis has at least one sample, got n = {n}")
    if 0 <= i < n:
        return i
    if border == "zero":
        return -1
    if border == "edge":
        return min(max(i, 0), n - 1)
    j = i % (2 * n)
    return j if j < n else 2 * n - 1 - j


def gaussian_taps(sigma: float, radius=None, total: int = 256):
    """Integer taps of a Gaussian of ``sigma`` voxels that sum to ``total``: the only place of the filters a float
    enters.  ``sigma == 0`` gives ``[total]``.  Otherwise ``r = radius`` if given, else ``min(8, ceil(3 sigma))``;
    ``g_i = exp(-i^2 / (2 sigma^2))`` in float64 for ``i = -r .. r``, normalised to sum 1; ``w_i = floor(total g_i + 0.5)``
    for ``i != 0`` and the centre tap is ``total`` minus the others; zero taps at both ends are trimmed symmetrically."""
    sigma = float(sigma)
    if isinstance(total, bool) or not isinstance(total, (int, np.integer)) or not 1 <= total <= FILTER_MAX_TAP_SUM:
        raise ValueError(f"total must be an integer in 1 .. {FILTER_MAX_TAP_SUM}, got {total!r}")
    if not 0 <= sigma < float("inf"):
        raise ValueError(f"sigma must be a non-negative finite number, got {sigma!r}")
    total = int(total)
    if sigma == 0:
        return [total]
    if radius is None:
        r = min(FILTER_MAX_TAP_RADIUS, int(np.ceil(3 * sigma)))
    else:
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= FILTER_MAX_TAP_RADIUS:
            raise ValueError(f"radius must be an integer in 0 .. {FILTER_MAX_TAP_RADIUS}, got {radius!r}")
        r = int(radius)
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    g = g / g.sum()
    w = [int(v) for v in np.floor(total * g + 0.5)]
    w[r] = total - (sum(w) - w[r])
    while len(w) > 1 and w[0] == 0 and w[-1] == 0:
        w = w[1:-1]
    if min(w) < 0:
        raise ValueError(f"sigma = {sigma} at radius {r} leaves a negative centre tap of total {total}")
    return w


def _three(values, what: str, kind=int):
    try:
        v = tuple(values.detach().cpu().tolist() if isinstance(values, Tensor) else values)
    except TypeError:
        v = ()
    if len(v) != 3:
        raise ValueError(f"{what} must be three numbers (x, y, z), got {values!r}")
    if kind is int and not all(isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)) for k in v):
        raise ValueError(f"{what} must be three integers (x, y, z), got {values!r}")
    return tuple(kind(k) for k in v)


def filter_plan(how: str, radius=None, rank=None, sigma=None, taps=None):
    """What ``how`` and its arguments ask for, checked by name: ``("rank", (rx, ry, rz), rank)`` or ``("taps", (tx, ty,
    tz))`` with three lists of integers."""
    if how not in FILTER_HOW:
        raise ValueError(f"how = {how!r}, must be one of {FILTER_HOW}")
    takes = {"median": ("radius",), "min": ("radius",), "max": ("radius",), "rank": ("radius", "rank"), "mean": ("radius",),
             "gauss": ("sigma",), "taps": ("taps",)}[how]
    given = {"radius": radius, "rank": rank, "sigma": sigma, "taps": taps}
    for key, value in given.items():
        if (value is not None) != (key in takes):
            raise ValueError(f"how={how!r} takes {' and '.join(takes)}" + (f", not {key}" if value is not None else
                                                                         f": {key} is missing"))
    if how in ("median", "min", "max", "rank"):
        r = _three(radius, "radius")
        if not all(0 <= k <= FILTER_MAX_RANK_RADIUS for k in r):
            raise ValueError(f"radius = {r}: a rank filter takes radii in 0 .. {FILTER_MAX_RANK_RADIUS} per axis")
        n = (2 * r[0] + 1) * (2 * r[1] + 1) * (2 * r[2] + 1)
        if how == "rank":
            rank = {"min": 0, "median": n // 2, "max": n - 1}.get(rank, rank) if isinstance(rank, str) else rank
            if isinstance(rank, (bool, np.bool_)) or not isinstance(rank, (int, np.integer)) or not 0 <= rank < n:
                raise ValueError(f"rank = {rank!r}: the window of radius {r} has the ranks 0 .. {n - 1}, or 'min', 'median', "
                                 "'max'")
            return "rank", r, int(rank)
        return "rank", r, {"min": 0, "median": n // 2, "max": n - 1}[how]
    if how == "mean":
        r = _three(radius, "radius")
        if not all(0 <= k <= FILTER_MAX_TAP_RADIUS for k in r):
            raise ValueError(f"radius = {r}: a mean takes radii in 0 .. {FILTER_MAX_TAP_RADIUS} per axis")
        return "taps", tuple([1] * (2 * k + 1) for k in r)
    if how == "gauss":
        return "taps", tuple(gaussian_taps(s) for s in _three(sigma, "sigma", float))
    try:
        lists = tuple([k for k in (t.tolist() if isinstance(t, (Tensor, np.ndarray)) else t)] for t in taps)
    except TypeError:
        lists = ()
    if len(lists) != 3:
        raise ValueError(f"taps must be three lists of integers (x, y, z), got {taps!r}")
    for axis, t in zip("xyz", lists):
        if not all(isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)) and k >= 0 for k in t):
            raise ValueError(f"the taps of {axis} must be non-negative integers, got {t!r}")
        if len(t) % 2 == 0 or not 1 <= len(t) <= 2 * FILTER_MAX_TAP_RADIUS + 1:
            raise ValueError(f"{len(t)} taps on {axis}: the count must be odd and in 1 .. {2 * FILTER_MAX_TAP_RADIUS + 1}")
        if not 1 <= sum(t) <= FILTER_MAX_TAP_SUM:
            raise ValueError(f"the tap sum of {axis} is {sum(t)}, it must be in 1 .. {FILTER_MAX_TAP_SUM}")
    return "taps", tuple([int(k) for k in t] for t in lists)


def check_filter(volume, how: str, radius=None, rank=None, sigma=None, taps=None, border: str = "mirror",
                 name: str = "volume"):
    """What ``filter_volume`` takes, checked on the tensor's description alone, before any device is touched: the
    (X, Y, Z) of it and ``filter_plan``'s answer.  Refused by name: a ``how`` or ``border`` that is not one, arguments
    that do not belong to ``how`` or are missing, rank radii beyond 2, mean radii beyond 8, a rank outside the window,
    tap lists that are not three odd-length lists of non-negative integers with sums in 1 .. 4096 (``ValueError``); a
    volume that is not a tensor, float volumes under a tap filter, and every dtype but uint8, uint16 and -- rank filters
    only -- float32 (``TypeError``); shapes that are not (X, Y, Z) or (1, X, Y, Z), extents beyond 2^30."""
    if border not in FILTER_BORDER:
        raise ValueError(f"border = {border!r}, must be 'zero', 'edge' or 'mirror'")
    plan = filter_plan(how, radius, rank, sigma, taps)
    if not isinstance(volume, Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(volume).__name__}")
    dt = volume.dtype
    if plan[0] == "taps" and (dt.is_floating_point or dt.is_complex or dt == torch.bool):
        raise TypeError(f"{name} is {dt}: float, complex and bool volumes take no tap filter, a float sum has no defined "
                        "order; filter the integer image (uint8 / uint16)")
    allowed = (torch.uint8, torch.uint16) + ((torch.float32,) if plan[0] == "rank" else ())
    if dt not in allowed:
        raise TypeError(f"{name} is {dt}: how={how!r} takes " + ("uint8, uint16 or float32" if plan[0] == "rank" else
                                                                "uint8 or uint16"))
    s = tuple(int(v) for v in volume.shape)
    s = s[1:] if len(s) == 4 and s[0] == 1 else s
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{name} has the shape {tuple(volume.shape)}: it must be (X, Y, Z) or (1, X, Y, Z) with every "
                         "extent at least 1")
    if max(s) > _FILTER_MAX_EXTENT:
        raise ValueError(f"{name} of shape {s} is too large to filter: every extent must stay within 2^30")
    return s, plan


def _bordered(a: np.ndarray, axis: int, r: int, border: str) -> np.ndarray:
    """``a`` with ``r`` bordered samples on both sides of ``axis``, by ``border_index``"""
    n = a.shape[axis]
    idx = np.array([border_index(i, n, border) for i in range(-r, n + r)], dtype=np.int64)
    out = np.take(a, np.maximum(idx, 0), axis=axis)
    if (idx < 0).any():
        out = np.where((idx >= 0).reshape([-1 if d == axis else 1 for d in range(a.ndim)]), out, np.zeros((), a.dtype))
    return out


def _filter_host(a: np.ndarray, plan, border: str) -> np.ndarray:
    """The definitions of ``filter_volume`` as numpy statements: the bordered volume, then the sorted window or the
    three exact int64 sums and the one rounded division."""
    if plan[0] == "rank":
        _, r, rank = plan
        p = a
        for axis in range(3):
            p = _bordered(p, axis, r[axis], border)
        X, Y, Z = a.shape
        window = np.stack([p[dx:dx + X, dy:dy + Y, dz:dz + Z] for dx in range(2 * r[0] + 1) for dy in range(2 * r[1] + 1)
                           for dz in range(2 * r[2] + 1)])
        return np.ascontiguousarray(np.partition(window, rank, axis=0)[rank])
    s, W = a.astype(np.int64), 1
    for axis, t in enumerate(plan[1]):
        n = a.shape[axis]
        p = _bordered(s, axis, len(t) // 2, border)
        s = sum(int(w) * np.take(p, np.arange(k, k + n), axis=axis) for k, w in enumerate(t))
        W *= sum(t)
    return ((s + W // 2) // W).astype(a.dtype)


def _int_array(values):
    return (C.c_int32 * len(values))(*values)


def filter_rank_device(v: Tensor, radius, rank: int, border: str = "mirror", method: str = "auto") -> Tensor:
    """One launch of ``sk_filter_rank`` on a contiguous (X, Y, Z) device tensor that ``check_filter`` has passed.
    ``method`` forces a selection (``FILTER_METHOD``); every method gives the same bits, and the forced ones exist for
    tests and for tools/bench_filter.py."""
    X, Y, Z = (int(n) for n in v.shape)
    out = torch.empty_like(v)
    _ffi.check(_ffi.lib.sk_filter_rank(_ffi.ptr(v), _ffi.ptr(out), _FILTER_CODE[v.dtype], X, Y, Z, *radius, int(rank),
                                       FILTER_BORDER[border], FILTER_METHOD[method], _ffi.stream_ptr(v.device)))
    return out


def filter_volume(volume: Tensor, how: str, radius=None, rank=None, sigma=None, taps=None, border: str = "mirror") -> Tensor:
    """An exactly defined neighbourhood filter of an (X, Y, Z) or (1, X, Y, Z) tensor on the device it lives on
    (DESIGN.md section 38).  The result has the input's rank, dtype, shape and device.

    ``border`` gives the sample at any source index ``i`` of an axis of extent ``n``, windows wider than the volume
    included: ``"zero"`` 0 outside the volume (the reference's padding), ``"edge"`` ``clamp(i, 0, n - 1)``, ``"mirror"``
    (the default) ``j = i mod 2n``, ``j`` if ``j < n`` else ``2n - 1 - j``.

    Rank filters -- ``how="median" | "min" | "max"`` with ``radius=(rx, ry, rz)``, each 0 .. 2, and ``how="rank"`` with
    ``rank`` as well, an integer in ``0 .. n - 1`` or one of those three names: the ``rank``-th smallest, counted from 0,
    of the ``n = (2rx+1)(2ry+1)(2rz+1)`` bordered samples of the window; the median is rank ``n // 2``.  uint8, uint16 and
    float32.  float32 is ordered by value: ``-0.0`` and ``0.0`` are equal and either may be returned, infinities are
    ordinary values.  A volume with a NaN in it is outside the definition: what comes back is unspecified.

    Tap filters -- ``how="mean"`` with ``radius`` up to 8 per axis (the taps ``[1] * (2r + 1)``), ``how="gauss"`` with
    ``sigma=(sx, sy, sz)`` in voxels (``gaussian_taps`` of each), ``how="taps"`` with ``taps=(tx, ty, tz)``, three odd-length
    lists of 1 .. 17 non-negative integers with sums in 1 .. 4096: ``(S + W // 2) // W`` with ``S`` the sum of
    ``wx wy wz v`` over the product of the three lists applied to the bordered samples and ``W = Wx Wy Wz`` -- the exact
    weighted mean rounded to nearest, halves up, rounded once; the rule of ``pool(..., "mean")`` and ``resample``.  uint8
    and uint16.

    On a device tensor this is one launch of ``sk_filter_rank`` or ``sk_filter_taps`` on the current stream; on a CPU
    tensor the same definitions run as numpy statements and give the same bits.  ``check_filter`` lists what is refused
    by name (``TypeError`` for dtypes, ``ValueError`` otherwise) before any device is touched."""
    (X, Y, Z), plan = check_filter(volume, how, radius, rank, sigma, taps, border)
    v = (volume[0] if volume.ndim == 4 else volume).contiguous()
    if not v.is_cuda:
        if v.dtype == torch.uint16:
            out = torch.from_numpy(_filter_host(v.view(torch.int16).numpy().view(np.uint16), plan, border)
                                   .view(np.int16)).view(torch.uint16)
        else:
            out = torch.from_numpy(_filter_host(v.numpy(), plan, border))
    elif plan[0] == "rank":
        out = filter_rank_device(v, plan[1], plan[2], border)
    else:
        out = torch.empty_like(v)
        arrays = [_int_array(t) for t in plan[1]]
        lists = [arg for a in arrays for arg in (a, len(a))]
        _ffi.check(_ffi.lib.sk_filter_taps(_ffi.ptr(v), _ffi.ptr(out), _FILTER_CODE[v.dtype], X, Y, Z, *lists,
                                           FILTER_BORDER[border], _ffi.stream_ptr(v.device)))
    return out.unsqueeze(0) if volume.ndim == 4 else out


def filter_path(dtype, shape, how: str, radius=None, rank=None, sigma=None, taps=None, aligned: bool = True):
    """Which kernel ``filter_volume`` runs for this geometry, answered on the host: ``(kernel, rows)`` with ``kernel``
    one of ``FILTER_KERNELS`` -- ``"extreme"`` (min and max: one pass over the window), ``"network"`` (the median of
    radius (1, 1, 0) and (1, 1, 1)), ``"radix"`` (every other rank), ``"acc32"`` / ``"acc64"`` (taps, by the width of the
    sums) -- and ``rows`` ``"vector"`` (16-byte loads and stores:
    rows are dword multiples and the bases ``aligned``) or ``"scalar"``."""
    assert tuple(int(_ffi.lib.sk_filter_tile(k)) for k in range(3)) == FILTER_TILE
    plan = filter_plan(how, radius, rank, sigma, taps)
    X, Y, Z = (int(n) for n in shape)
    if plan[0] == "rank":
        rc = int(_ffi.lib.sk_filter_path(_FILTER_CODE[dtype], X, Y, Z, *plan[1], plan[2], None, 0, None, 0, None, 0,
                                         int(bool(aligned))))
    else:
        arrays = [_int_array(t) for t in plan[1]]
        rc = int(_ffi.lib.sk_filter_path(_FILTER_CODE[dtype], X, Y, Z, 0, 0, 0, 0, *[arg for a in arrays for arg in (a, len(a))],
                                         int(bool(aligned))))
    _ffi.check(rc if rc < 0 else 0)
    return FILTER_KERNELS[rc & 7], "vector" if rc & 8 else "scalar"


def _reference_rank(image: Tensor, rank: int, name: str) -> Tensor:
    """(B C, X, Y, Z): the rank-th smallest of the 27 zero-padded samples around every voxel of every channel"""
    if not isinstance(image, Tensor) or image.ndim != 5:
        raise ValueError(f"{name} must be a (B, C, X, Y, Z) tensor")
    _ffi.require_gpu(image, name)
    if image.dtype != torch.float32:
        raise TypeError(f"{name} is {image.dtype}: the reference's filters take float32; integer images go through "
                        "filter_volume")
    b, c, w, h, d = image.shape
    x = image.view(b * c, w, h, d)
    if x.numel() == 0:
        return torch.empty_like(x)
    return torch.stack([filter_rank_device(x[i], (1, 1, 1), rank, "zero") for i in range(b * c)])


def median_filter(input: Tensor) -> Tensor:
    """The reference's ``median_filter`` (skoots/lib/morphology.py:202-210, which cannot run as written): the lower
    median -- ``torch.median``'s, rank 13 of 27 -- of the 3x3x3 window with zero padding on a (B, C, X, Y, Z) float32
    device tensor.  NaNs are outside the definition."""
    return _reference_rank(input, 13, "input").view(input.shape)


def dilate(input: Tensor) -> Tensor:
    """The reference's ``dilate`` (skoots/lib/morphology.py:224-232, which cannot run as written): the maximum of the
    3x3x3 window with zero padding on a (B, C, X, Y, Z) float32 device tensor."""
    return _reference_rank(input, 26, "input").view(input.shape)


def binary_erosion(image: Tensor) -> Tensor:
    """The reference's ``binary_erosion`` (skoots/lib/morphology.py:131-152): the minimum of the 3x3x3 window with zero
    padding on a (B, C, X, Y, Z) float32 device tensor, with the reference's result shape (1, B C, X, Y, Z)."""
    return _reference_rank(image, 0, "image").unsqueeze(0)


# ---- tile histograms and look-up-table transforms ----

EQUALIZE_HOW = ("stretch", "equalize", "match")
EQUALIZE_BINS = {torch.uint8: (256,), torch.uint16: (256, 1024, 4096)}
EQUALIZE_DEFAULT_BINS = {torch.uint8: 256, torch.uint16: 1024}
EQUALIZE_MAX_SHIFT = 8
EQUALIZE_HIST_PATHS = ("one", "planes", "ztiles", "global")            # SK_EQUALIZE_HIST_*
EQUALIZE_Z_MODES = ("one", "tile", "interp")                           # SK_EQUALIZE_APPLY_Z_*
_EQUALIZE_MAX_EXTENT = 2 ** 30
_EQUALIZE_MAX_TOTAL = 2 ** 31
_EQUALIZE_DEFAULTS = {"low": 0.5, "high": 99.5, "clip": 3.0, "target": None}
_EQUALIZE_TAKES = {"stretch": ("low", "high"), "equalize": ("clip",), "match": ("target",)}


def _dtype_top(dtype) -> int:
    return 255 if dtype == torch.uint8 else 65535


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def histogram_shift(vmax: int, bins: int) -> int:
    """The smallest ``s`` with ``vmax >> s < bins``"""
    if not _is_int(vmax) or vmax < 0 or not _is_int(bins) or bins < 1:
        raise ValueError(f"histogram_shift takes a maximum >= 0 and bins >= 1, got {vmax!r} and {bins!r}")
    s = 0
    while (int(vmax) >> s) >= bins:
        s += 1
    return s


def equalize_tile(tile) -> Tuple[int, int, int]:
    """``tile`` as ``(tx, ty, tz)``: ``None`` is ``(0, 0, 0)``, ``"slices"`` is ``(0, 0, 1)``, ``0`` the whole axis"""
    if tile is None:
        return 0, 0, 0
    if isinstance(tile, str):
        if tile != "slices":
            raise ValueError(f"tile = {tile!r}: the only name is 'slices'")
        return 0, 0, 1
    try:
        t = tuple(tile.tolist() if isinstance(tile, (Tensor, np.ndarray)) else tile)
    except TypeError:
        t = ()
    if len(t) != 3 or not all(_is_int(k) for k in t):
        raise ValueError(f"tile must be None, 'slices' or three integers (tx, ty, tz), got {tile!r}")
    if not all(0 <= k <= _EQUALIZE_MAX_EXTENT for k in t):
        raise ValueError(f"tile = {t}: every side must be >= 1 (or 0: the whole axis) and within 2^30")
    return tuple(int(k) for k in t)


def tile_grid(shape, tile) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """``(sides, counts)`` of ``tile`` on a volume of ``shape``: a side of 0, or larger than the extent, is the extent;
    there are ``ceil(n / t)`` tiles per axis and the last may be clipped"""
    t = equalize_tile(tile)
    sides = tuple(int(n) if k == 0 or k > n else k for k, n in zip(t, shape))
    return sides, tuple(-(-int(n) // k) for k, n in zip(sides, shape))


def equalize_plan(how: str, tile=None, bins=None, low=0.5, high=99.5, clip=3.0, target=None, top=None,
                  interpolate=True) -> dict:
    """The arguments of ``equalize`` that can be judged without the volume, checked by name; returns them as keywords"""
    if how not in EQUALIZE_HOW:
        raise ValueError(f"how = {how!r}, must be one of {EQUALIZE_HOW}")
    given = {"low": low, "high": high, "clip": clip, "target": target}
    for key, value in given.items():
        default = _EQUALIZE_DEFAULTS[key]
        if key not in _EQUALIZE_TAKES[how] and not (value is default or (default is not None and value == default)):
            raise ValueError(f"how={how!r} takes {' and '.join(_EQUALIZE_TAKES[how])}, not {key}")
    t = equalize_tile(tile)
    if bins is not None and bins not in EQUALIZE_BINS[torch.uint16]:
        raise ValueError(f"bins = {bins!r}, must be 256, 1024 or 4096 (uint8: 256)")
    if how == "stretch":
        try:
            low, high = float(low), float(high)
        except (TypeError, ValueError):
            raise ValueError(f"low and high must be numbers, got {low!r} and {high!r}") from None
        if not (0 <= low <= 100 and 0 <= high <= 100):
            raise ValueError(f"low = {low} and high = {high} must lie in 0 .. 100")
        if not low < high:
            raise ValueError(f"low = {low} must be below high = {high}")
    if how == "equalize" and clip is not None:
        if isinstance(clip, (bool, str)) or not isinstance(clip, (int, float, np.integer, np.floating)) or \
                not 0 < float(clip) < float("inf"):
            raise ValueError(f"clip = {clip!r}: a multiple of the mean bin height > 0, or None for no clipping")
        clip = float(clip)
    if top is not None and (not _is_int(top) or not 1 <= top <= 65535):
        raise ValueError(f"top = {top!r}: the output maximum must be an integer in 1 .. the dtype's maximum")
    if not isinstance(interpolate, (bool, np.bool_)):
        raise ValueError(f"interpolate = {interpolate!r}, must be True or False")
    return dict(how=how, tile=t, bins=bins, low=low, high=high, clip=clip, target=target, top=top,
                interpolate=bool(interpolate))


def _equalize_volume(volume, name: str):
    """dtype and (X, Y, Z) of a volume the histogram kernels take, from its description"""
    if not isinstance(volume, Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(volume).__name__}")
    dt = volume.dtype
    if dt not in EQUALIZE_BINS:
        raise TypeError(f"{name} is {dt}: grey-value transforms take uint8 or uint16; float, signed, bool and complex volumes "
                        "are refused")
    s = tuple(int(v) for v in volume.shape)
    s = s[1:] if len(s) == 4 and s[0] == 1 else s
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{name} has the shape {tuple(volume.shape)}: it must be (X, Y, Z) or (1, X, Y, Z) with every "
                         "extent at least 1")
    if max(s) > _EQUALIZE_MAX_EXTENT:
        raise ValueError(f"{name} of shape {s} is too large: every extent must stay within 2^30")
    return dt, s


def _equalize_bins(dt, bins, name: str) -> int:
    if bins is None:
        return EQUALIZE_DEFAULT_BINS[dt]
    if bins not in EQUALIZE_BINS[dt]:
        raise ValueError(f"bins = {bins!r}: {name} is {dt} and takes {' or '.join(str(b) for b in EQUALIZE_BINS[dt])}")
    return int(bins)


def check_equalize(volume, how: str, *, tile=None, bins=None, low=0.5, high=99.5, clip=3.0, target=None, top=None,
                   interpolate=True, name: str = "volume"):
    """What ``equalize`` takes, checked on the tensors' descriptions alone, before any device is touched.  Returns
    ``((X, Y, Z), plan)`` with ``plan`` the checked keywords, ``bins`` and ``top`` filled in.  Refused by name: a ``how``
    that is not one, arguments that belong to another ``how``, a tile that is not ``None``, ``"slices"`` or three sides
    >= 0, a tile of 2^31 voxels or more, ``bins`` the dtype does not take, ``low`` / ``high`` outside 0 .. 100 or not in
    order, a ``clip`` that is not positive, a ``top`` beyond the dtype's maximum, a target that is neither a volume of
    the same dtype with fewer than 2^31 voxels nor a 1-D int64 histogram of ``bins`` entries (``ValueError``); a volume
    that is not a tensor or not uint8 / uint16 (``TypeError``); shapes that are not (X, Y, Z) or (1, X, Y, Z), extents
    beyond 2^30."""
    plan = equalize_plan(how, tile, bins, low, high, clip, target, top, interpolate)
    dt, s = _equalize_volume(volume, name)
    plan["bins"] = _equalize_bins(dt, bins, name)
    if plan["top"] is None:
        plan["top"] = _dtype_top(dt)
    elif plan["top"] > _dtype_top(dt):
        raise ValueError(f"top = {plan['top']} is beyond the maximum of {dt}")
    sides, _ = tile_grid(s, plan["tile"])
    if sides[0] * sides[1] * sides[2] >= _EQUALIZE_MAX_TOTAL:
        raise ValueError(f"a tile of {sides} has 2^31 voxels or more: the tables are built from totals below 2^31")
    if target is not None:
        if isinstance(target, np.ndarray):
            target = torch.from_numpy(target)
        if not isinstance(target, Tensor):
            raise TypeError(f"target must be a volume, a 1-D int64 histogram or None, got {type(target).__name__}")
        if target.ndim == 1:
            if target.dtype != torch.int64 or target.numel() != plan["bins"]:
                raise ValueError(f"a target histogram must be int64 with bins = {plan['bins']} entries, got {target.dtype} "
                                 f"with {target.numel()}")
        else:
            tdt, ts = _equalize_volume(target, "target")
            if tdt != dt:
                raise TypeError(f"target is {tdt} and {name} is {dt}: a target volume has the volume's dtype")
            if ts[0] * ts[1] * ts[2] >= _EQUALIZE_MAX_TOTAL:
                raise ValueError(f"target of shape {ts} has 2^31 voxels or more")
        plan["target"] = target
    return s, plan


def _as_numpy(t: Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def _from_numpy(a: np.ndarray) -> Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def volume_max(v: Tensor) -> int:
    """The largest sample of a uint8 / uint16 tensor, where it lives"""
    if v.dtype == torch.uint16:
        s = v.view(torch.int16)
        return (int(torch.bitwise_xor(s, -32768).max()) ^ -32768) & 0xFFFF    # unsigned order through the sign bit
    return int(v.max())


def _hist_shift(dt, bins: int, shift, vmax) -> int:
    if dt == torch.uint8:
        if shift not in (None, 0):
            raise ValueError(f"shift = {shift!r}: uint8 takes shift 0")
        return 0
    if shift is None:
        return histogram_shift(vmax(), bins)
    if not _is_int(shift) or not 0 <= shift <= EQUALIZE_MAX_SHIFT:
        raise ValueError(f"shift = {shift!r}, must be an integer in 0 .. {EQUALIZE_MAX_SHIFT}")
    return int(shift)


def _axis_tiles(n: int, t: int) -> np.ndarray:
    return np.arange(n, dtype=np.int64) // t


def _axis_pairs(n: int, t: int, count: int, interpolate: bool):
    """per index of an axis: the two tiles and their weights"""
    i = np.arange(n, dtype=np.int64)
    if not interpolate:
        k = i // t
        return k, k, np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    p = 2 * i + 1 - t
    k0 = p // (2 * t)
    w1 = p - 2 * t * k0
    return np.clip(k0, 0, count - 1), np.clip(k0 + 1, 0, count - 1), 2 * t - w1, w1


def _histograms_host(a: np.ndarray, sides, counts, bins: int, shift: int) -> np.ndarray:
    b = np.minimum(a.astype(np.int64) >> shift, bins - 1)
    kx, ky, kz = (_axis_tiles(n, t) for n, t in zip(a.shape, sides))
    tile = (kx[:, None, None] * counts[1] + ky[None, :, None]) * counts[2] + kz[None, None, :]
    flat = np.bincount((tile * bins + b).ravel(), minlength=counts[0] * counts[1] * counts[2] * bins)
    return flat.astype(np.int64).reshape(*counts, bins)


def _apply_host(a: np.ndarray, luts: np.ndarray, sides, counts, bins: int, shift: int, interpolate: bool) -> np.ndarray:
    b = np.minimum(a.astype(np.int64) >> shift, bins - 1)
    luts = luts.astype(np.int64)
    ax = [_axis_pairs(n, t, c, interpolate) for n, t, c in zip(a.shape, sides, counts)]
    if not interpolate:
        return luts[ax[0][0][:, None, None], ax[1][0][None, :, None], ax[2][0][None, None, :], b].astype(a.dtype)
    W = 8 * sides[0] * sides[1] * sides[2]
    if W * 65535 >= 2 ** 63:
        raise ValueError(f"tile sides {sides} are too large for the host path")
    S = np.zeros(a.shape, dtype=np.int64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = ax[0][2 + cx][:, None, None] * ax[1][2 + cy][None, :, None] * ax[2][2 + cz][None, None, :]
                S += w * luts[ax[0][cx][:, None, None], ax[1][cy][None, :, None], ax[2][cz][None, None, :], b]
    return ((S + W // 2) // W).astype(a.dtype)


def tile_histograms(volume: Tensor, tile=None, bins=None, shift=None) -> Tensor:
    """int64 ``(nx, ny, nz, bins)`` on the volume's device: entry ``[kx, ky, kz, b]`` counts the voxels of that tile with
    ``min(v >> shift, bins - 1) == b``.  ``shift=None`` is ``histogram_shift`` of the volume's maximum.  Exact, and the
    same on every run; one launch of ``sk_tile_histograms`` on a device tensor, numpy statements on a CPU tensor."""
    dt, s = _equalize_volume(volume, "volume")
    bins = _equalize_bins(dt, bins, "volume")
    sides, counts = tile_grid(s, tile)
    v = (volume[0] if volume.ndim == 4 else volume).contiguous()
    shift = _hist_shift(dt, bins, shift, lambda: volume_max(v))
    if not v.is_cuda:
        return torch.from_numpy(_histograms_host(_as_numpy(v), sides, counts, bins, shift))
    out = torch.empty(counts + (bins,), dtype=torch.int64, device=v.device)
    _ffi.check(_ffi.lib.sk_tile_histograms(_ffi.ptr(v), _FILTER_CODE[dt], *s, *sides, bins, shift, _ffi.ptr(out),
                                           _ffi.stream_ptr(v.device)))
    return out


def apply_tile_luts(volume: Tensor, luts: Tensor, tile=None, shift: int = 0, interpolate: bool = True, out=None) -> Tensor:
    """Every voxel through the tables of the tiles around it: ``luts`` is int32 ``(nx, ny, nz, bins)`` with values in
    ``0 .. dtype max``.  ``interpolate=False``: ``luts[tile of the voxel][bin(v)]``.  ``interpolate=True``: the weighted
    mean of the 8 surrounding tiles' entries, weights linear between the tile centres, ``(S + W // 2) // W`` with
    ``W = 8 tx ty tz``, rounded once (include/skoots_hip.h has the formulas).  One launch of ``sk_apply_tile_luts`` on a
    device tensor; a CPU tensor gives the same bits through numpy.  ``out``, device tensors only: a contiguous (X, Y, Z)
    tensor of the volume's dtype and device to write into, another buffer than the volume."""
    dt, s = _equalize_volume(volume, "volume")
    sides, counts = tile_grid(s, tile)
    if isinstance(luts, np.ndarray):
        luts = torch.from_numpy(luts)
    if not isinstance(luts, Tensor) or luts.dtype != torch.int32 or luts.ndim != 4 or tuple(luts.shape[:3]) != counts \
            or luts.shape[3] not in EQUALIZE_BINS[dt]:
        raise ValueError(f"luts must be an int32 tensor {counts + ('bins',)} with bins one of {EQUALIZE_BINS[dt]}, got "
                         f"{getattr(luts, 'dtype', type(luts).__name__)} {tuple(getattr(luts, 'shape', ()))}")
    bins = int(luts.shape[3])
    shift = _hist_shift(dt, bins, int(shift) if _is_int(shift) else shift, None)
    if not isinstance(interpolate, (bool, np.bool_)):
        raise ValueError(f"interpolate = {interpolate!r}, must be True or False")
    v = (volume[0] if volume.ndim == 4 else volume).contiguous()
    luts = luts.to(v.device).contiguous()
    if int(luts.min()) < 0 or int(luts.max()) > _dtype_top(dt):
        raise ValueError(f"luts holds values outside 0 .. {_dtype_top(dt)}, the range of {dt}")
    if not v.is_cuda:
        if out is not None:
            raise ValueError("out is for device tensors")
        out = _from_numpy(_apply_host(_as_numpy(v), luts.numpy(), sides, counts, bins, shift, bool(interpolate)))
    else:
        if out is None:
            out = torch.empty_like(v)
        elif not isinstance(out, Tensor) or out.dtype != dt or out.device != v.device or tuple(out.shape) != s or \
                not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dt} tensor of shape {s} on {v.device}")
        _ffi.check(_ffi.lib.sk_apply_tile_luts(_ffi.ptr(v), _ffi.ptr(out), _FILTER_CODE[dt], *s, *sides, _ffi.ptr(luts), bins,
                                               shift, int(bool(interpolate)), _ffi.stream_ptr(v.device)))
    return out.unsqueeze(0) if volume.ndim == 4 else out


def _hist_array(h, what: str = "h"):
    h = np.asarray(h.detach().cpu().numpy() if isinstance(h, Tensor) else h)
    if h.ndim < 1 or h.dtype.kind not in "iu":
        raise ValueError(f"{what} must be an integer array (..., bins)")
    h = h.astype(np.int64)
    n = h.sum(axis=-1)
    if h.min() < 0 or n.min() < 1 or n.max() >= _EQUALIZE_MAX_TOTAL:
        raise ValueError(f"{what}: every histogram needs counts >= 0 and a total in 1 .. 2^31 - 1")
    return h, n


def _lut_top(top, bins: int) -> int:
    if top is None:
        return 255 if bins == 256 else 65535
    if not _is_int(top) or not 1 <= top <= 65535:
        raise ValueError(f"top = {top!r}: the output maximum must be an integer in 1 .. 65535")
    return int(top)


def _first_reaching(H: np.ndarray, k: np.ndarray) -> np.ndarray:
    """per leading index the first bin whose inclusive cumulative sum reaches k"""
    return (H >= k[..., None]).argmax(axis=-1)


def stretch_bounds(h, low: float = 0.5, high: float = 99.5):
    """``(lo, hi)``: the nearest-rank percentile bins of ``(..., bins)`` histograms -- for ``q`` percent the first bin
    whose cumulative sum reaches ``clamp(ceil(q / 100 * n), 1, n)``, numpy's ``method="inverted_cdf"`` on the bins"""
    h, n = _hist_array(h)
    equalize_plan("stretch", low=low, high=high)
    H = np.cumsum(h, axis=-1)
    ks = [np.clip(np.ceil(float(q) / 100 * n.astype(np.float64)).astype(np.int64), 1, n) for q in (low, high)]
    return _first_reaching(H, ks[0]), _first_reaching(H, ks[1])


def stretch_lut(h, low: float = 0.5, high: float = 99.5, top=None, shift: int = 0) -> np.ndarray:
    """Percentile stretch: ``lut[b] = clamp(((b - lo) * top + (hi - lo) // 2) // (hi - lo), 0, top)`` with ``lo``, ``hi``
    of ``stretch_bounds``; where ``hi == lo`` the identity ``b << shift`` clamped to ``top``.  ``h`` is ``(..., bins)``
    int64, the result int32 of the same shape; ``top=None`` is 255 for 256 bins and 65535 otherwise."""
    lo, hi = stretch_bounds(h, low, high)
    bins = np.shape(h)[-1]
    top = _lut_top(top, bins)
    b = np.arange(bins, dtype=np.int64)
    d = (hi - lo)[..., None]
    lut = np.clip(((b - lo[..., None]) * top + d // 2) // np.maximum(d, 1), 0, top)
    return np.where(d > 0, lut, np.minimum(b << shift, top)).astype(np.int32)


def equalize_lut(h, clip=None, top=None) -> np.ndarray:
    """Histogram equalisation: ``lut[b] = (H'[b] * top + n // 2) // n`` with ``H'`` the cumulative sum of the clipped
    histogram.  ``clip`` (a multiple of the mean bin height, > 0): ``c = max(1, ceil(clip * n / bins))``, the excess
    ``E = sum(max(h - c, 0))`` is cut off and handed back, ``E // bins`` to every bin and one more to the ``E % bins``
    lowest-numbered bins, once.  ``clip=None`` is plain equalisation."""
    h, n = _hist_array(h)
    bins = h.shape[-1]
    top = _lut_top(top, bins)
    if clip is not None:
        clip = equalize_plan("equalize", clip=clip)["clip"]
        c = np.maximum(1, np.ceil(clip * n.astype(np.float64) / bins).astype(np.int64))[..., None]
        E = np.maximum(h - c, 0).sum(axis=-1)
        q, r = np.divmod(E, bins)
        h = np.minimum(h, c) + q[..., None] + (np.arange(bins, dtype=np.int64) < r[..., None])
    H = np.cumsum(h, axis=-1)
    return ((H * top + (n // 2)[..., None]) // n[..., None]).astype(np.int32)


def match_lut(h, g, shift: int = 0, top=None) -> np.ndarray:
    """Histogram matching to the target histogram ``g`` (``(bins,)`` or of ``h``'s shape): ``t[b]`` is the smallest ``t``
    with ``G[t] * n >= H[b] * m`` (``G``, ``m`` the target's cumulative sum and total) and ``lut[b] = min(t[b] << shift,
    top)``."""
    h, n = _hist_array(h)
    g, m = _hist_array(g, "g")
    bins = h.shape[-1]
    if g.shape[-1] != bins:
        raise ValueError(f"the target has {g.shape[-1]} bins and h has {bins}")
    top = _lut_top(top, bins)
    H, G = np.cumsum(h, axis=-1), np.cumsum(g, axis=-1)
    need = (H * np.broadcast_to(m, n.shape)[..., None] + n[..., None] - 1) // n[..., None]   # G[t] n >= H m <=> G[t] >= ceil(H m / n)
    if g.ndim == 1:
        t = np.searchsorted(G, need, side="left")
    else:                                         # one sorted array of all targets: target k lives in k M .. k M + m_k
        G = np.broadcast_to(G, h.shape).reshape(-1, bins)
        M = int(m.max()) + 1
        off = np.arange(G.shape[0], dtype=np.int64)[:, None] * M
        t = np.searchsorted((G + off).ravel(), (need.reshape(-1, bins) + off).ravel(), side="left").reshape(-1, bins)
        t = (t - np.arange(G.shape[0], dtype=np.int64)[:, None] * bins).reshape(h.shape)
    return np.minimum(t.astype(np.int64) << shift, top).astype(np.int32)


def equalize(volume: Tensor, how: str, *, tile=None, bins=None, low=0.5, high=99.5, clip=3.0, target=None, top=None,
             interpolate=True, report=None) -> Tensor:
    """A histogram-driven transform of the grey values of a uint8 / uint16 (X, Y, Z) or (1, X, Y, Z) tensor on the device
    it lives on: ``tile_histograms``, then a table per tile, then ``apply_tile_luts``.

    ``how="stretch"``: the ``low`` and ``high`` percentiles (nearest rank, on the bins) go to 0 and ``top``
    (``stretch_lut``).  ``how="equalize"``: histogram equalisation with the histogram clipped at ``clip`` times the mean bin
    height (``equalize_lut``); ``clip=None`` with ``tile=None`` is global equalisation, with tiles it is CLAHE in 3-D, with
    ``(tx, ty, 0)`` CLAHE per column of planes.  ``how="match"``: histogram matching (``match_lut``) to ``target`` -- a
    volume of the same dtype (its global histogram at the same bins and shift), a 1-D int64 histogram of ``bins`` entries,
    or ``None``, the volume's own global histogram, which with ``tile="slices"`` removes slice flicker.

    ``tile``: ``(tx, ty, tz)``, 0 = the whole axis; ``None`` = one tile; ``"slices"`` = one per z-plane.  ``bins``: 256 for
    uint8; 256, 1024 (default) or 4096 for uint16, with ``bin(v) = min(v >> shift, bins - 1)`` and the shift
    ``histogram_shift`` of the volume's maximum (for a target volume: of the larger of the two).  ``top``: the output
    maximum, the dtype's by default.  ``interpolate``: tables are interpolated between tile centres so that no tile edge
    shows.  ``report``, a dict, receives ``shift``, ``bins``, ``grid``, ``paths`` and for ``"stretch"`` ``lo`` / ``hi``.
    Everything is integer arithmetic: a CPU tensor gives the same bits through numpy.  ``check_equalize`` lists what is
    refused."""
    s, plan = check_equalize(volume, how, tile=tile, bins=bins, low=low, high=high, clip=clip, target=target, top=top,
                             interpolate=interpolate)
    v = (volume[0] if volume.ndim == 4 else volume).contiguous()
    dt, nbins, out_top, t = v.dtype, plan["bins"], plan["top"], plan["tile"]
    goal = plan["target"]
    goal_volume = None
    if goal is not None and goal.ndim != 1:
        goal_volume = (goal[0] if goal.ndim == 4 else goal).contiguous()
    shift = 0
    if dt == torch.uint16:
        vmax = volume_max(v)
        if goal_volume is not None:
            vmax = max(vmax, volume_max(goal_volume))
        shift = histogram_shift(vmax, nbins)
    h = tile_histograms(v, t, nbins, shift).cpu().numpy()
    if how == "stretch":
        luts = stretch_lut(h, plan["low"], plan["high"], out_top, shift)
    elif how == "equalize":
        luts = equalize_lut(h, plan["clip"], out_top)
    else:
        if goal_volume is not None:
            g = tile_histograms(goal_volume, None, nbins, shift)[0, 0, 0].cpu().numpy()
        elif goal is not None:
            g = goal.cpu().numpy()
        else:
            g = h.reshape(-1, nbins).sum(axis=0)
        luts = match_lut(h, g, shift, out_top)
    if report is not None:
        sides, counts = tile_grid(s, t)
        report.update(shift=shift, bins=nbins, grid=counts, sides=sides,
                      paths=equalize_path(dt, s, t, nbins, shift, plan["interpolate"]) if v.is_cuda else ("numpy", "numpy"))
        if how == "stretch":
            lo, hi = stretch_bounds(h, plan["low"], plan["high"])
            report.update(lo=lo, hi=hi)
    out = apply_tile_luts(v, torch.from_numpy(luts), t, shift, plan["interpolate"])
    return out.unsqueeze(0) if volume.ndim == 4 else out


def equalize_path(dtype, shape, tile=None, bins=None, shift: int = 0, interpolate: bool = True) -> Tuple[str, str]:
    """Which kernels ``tile_histograms`` and ``apply_tile_luts`` run for this geometry, answered on the host:
    ``(histograms, apply)``.  ``histograms`` is one of ``EQUALIZE_HIST_PATHS`` -- ``"one"`` (a workgroup counts one tile in
    LDS), ``"planes"`` (``tz == 1``: a table per z-plane), ``"ztiles"`` (several z-tiles per workgroup), ``"global"`` (tile
    columns of fewer than 16 rows).  ``apply`` is ``"<lds|gather>/<xy|-><z-mode>/<lookup|acc32|acc64>"``: tables staged in
    LDS or gathered from global memory; whether x or y interpolates and how z picks its table (``one``, ``tile``,
    ``interp``); a plain look-up or weighted sums of that width."""
    bins = _equalize_bins(dtype, bins, "the volume")
    X, Y, Z = (int(n) for n in shape)
    t = equalize_tile(tile)
    rc = [int(_ffi.lib.sk_equalize_path(which, _FILTER_CODE[dtype], X, Y, Z, *t, bins, int(shift), int(bool(interpolate))))
          for which in (0, 1)]
    for r in rc:
        _ffi.check(r if r < 0 else 0)
    a = rc[1]
    return EQUALIZE_HIST_PATHS[rc[0]], "/".join(("gather" if a & 32 else "lds", ("xy+" if a & 4 else "-+") + EQUALIZE_Z_MODES[a & 3],
                                                 "acc64" if a & 16 else "acc32" if a & 8 else "lookup"))
