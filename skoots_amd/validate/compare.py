"""Per-instance measurements of an instance mask, and ``python -m skoots_amd.validate.compare MASK``.

The reference sketches this step in ``skoots/validate/compare.py``: ``stats_per_instance`` forms one full-volume mask
per id and hands it to ``get_volume`` (which raises ``TypeError``) and to a marching-cubes ``get_surface_area``, and
``compare()`` raises ``NotImplementedError``; the last paragraph below is this project's ``compare()``.  Here one kernel
pass (``sk_instance_stats``) gives 13 integer sums and a box per instance, and ``derive`` turns them into
volume, centroid, face area and the axes of the ellipsoid with the same second moments.  Every kernel output is an
integer, so the measurement is exact and the same on every run.

``face_area`` is the area of the exposed voxel faces, which is exact for what it defines and overestimates a curved
surface.  The reference's marching-cubes ``surface_area`` is available with ``surface="open"`` (its
meaning) or ``"closed"``: a second kernel pass (``sk_instance_mesh_cells``) counts every instance's
cells per triangle class, integers again, and ``class_areas`` turns the counts into an area on the host.

``skeleton=True`` / ``--skeleton`` adds the centre line: every instance is Lee-thinned in its box and the skeleton is
read as a graph (``sk_skeleton_graph``) -- voxels, endpoints, junction voxels and the links per direction
class, integers once more -- and ``skeleton_columns`` turns the links into a length at the voxel spacing.
``branches=True`` / ``--branches`` traces the skeletons instead of counting them (``sk_skeleton_branches_count`` /
``_emit``): a node table and a branch table, from which ``branch_columns`` derives components, junction
nodes, branches, rings, cycles and branch lengths per instance, and the command writes ``<mask>_branches.csv`` and
``<mask>_nodes.csv``.

``thickness="open"`` / ``"closed"`` / ``--thickness`` adds the width: the exact Euclidean distance transform of every
instance (``sk_label_edt``) and ``inscribed_radius``, the square root of its maximum; together with the
skeleton, the mean, minimum and maximum radius along the centre line.

``local_thickness="open"`` / ``"closed"`` / ``--local-thickness`` adds the width everywhere: for every voxel the radius
of the largest ball inside its instance that holds it (``sk_local_thickness_paint`` on the distance transform, DESIGN.md
§28), and per instance its mean, spread and thinnest place; ``--save-thickness`` writes the map.

``mesh="open"`` / ``"closed"`` / ``--mesh`` adds the size of the marching-cubes mesh itself -- vertices, triangles and,
closed, the Euler characteristic (``sk_instance_mesh_count``) -- and ``--save-meshes`` writes the
meshes of ``lib.instance_meshes`` into one PLY file.

``contacts=6`` / ``18`` / ``26`` / ``--contacts`` adds who touches whom: the table of touching pairs with their shared
faces, edges and corners from one kernel pass (``sk_instance_contacts``), per instance its neighbours and
the share of its surface that lies against them, and ``<mask>_contacts.csv``, one row per pair.

``image=I`` / ``--image I`` adds the other half of the question, the image under every instance: one kernel pass over
mask and image (``sk_instance_intensity``) gives count, sums, extrema and a 256-bin histogram per instance,
integers all, and ``intensity_columns`` turns them into ``intensity_mean``, ``intensity_std``, ``intensity_min``,
``intensity_max``, ``intensity_median``, ``intensity_p05``, ``intensity_p95`` and the intensity-weighted centroid
``wcx, wcy, wcz``.  The image is 8- or 16-bit; a 16-bit image whose largest sample is 256 or more is binned by
``v >> shift`` and its three quantiles are then the LOWER EDGE of their bin, ``bin << shift``.
``intensity_ring=D`` / ``--intensity-ring D`` adds the background within the distance D that is nearer to this instance
than to any other (``lib.intensity_ring``): ``ring_voxels``, ``ring_mean``, ``ring_std`` and ``contrast`` =
``(intensity_mean - ring_mean) / (intensity_mean + ring_mean)``.  ``--save-histograms`` writes
``<mask>_histograms.csv``, the 256 counts of every instance.

``compare(ground_truth, predictions)`` / ``--ground-truth GT`` matches every ground-truth instance to a predicted one
by IoU and measures the pair: overlap, volume and centroid differences, and the distances between the two voxel
surfaces -- Hausdorff, its 95th percentile, average symmetric surface distance, surface Dice -- from an exact
nearest-neighbour search over all pairs at once (``sk_surface_distances``).  ``sparse=True`` /
``--sparse-matching`` matches on the sparse table of overlapping pairs (``sk_instance_overlaps``) instead
of the dense N x M matrix and returns the same.

``parents=P`` / ``--parents P`` adds, for a second mask of other and larger objects, the object of P every instance
lies in and the share of it inside: ``parent,inside_fraction``, as ``utils.relate`` decides them.

``near=B | "self"`` with ``near_distance=D`` / ``--near B|self --near-distance D`` adds which instances of B -- or of the
mask itself -- lie within D of every instance: ``near_partners,nearest_id,nearest_gap,near_voxels,near_fraction``, as
``utils.proximity`` derives them.
"""
from __future__ import annotations

import argparse
import logging
import math
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .lib import (_Rows, check_shape, id_rows, instance_contacts, instance_intensity, instance_local_thickness,
                  instance_mesh_cells, instance_mesh_counts, instance_meshes, instance_skeleton_branches,
                  instance_skeleton_graph, instance_sums,
                  instance_thickness, nearest_rank)
from .lib import intensity_ring as _intensity_ring
from .mc_table import CLASS_TRIANGLES, TRIANGLE_TYPES

CSV_COLUMNS = ("id,voxels,volume,x0,y0,z0,x1,y1,z1,touches_border,cx,cy,cz,face_area,axis_major,axis_mid,"
               "axis_minor")
SURFACE_COLUMNS = "surface_area,surface_to_volume"       # appended with --surface-area
SURFACE_MODES = (None, "open", "closed")
SKELETON_COLUMNS = "skeleton_voxels,skeleton_length,skeleton_endpoints,skeleton_junctions,skeleton_branches"  # --skeleton
THICKNESS_COLUMNS = "inscribed_radius"                   # appended with --thickness
SKELETON_RADIUS_COLUMNS = "skeleton_radius_mean,skeleton_radius_min,skeleton_radius_max"  # --thickness with --skeleton
THICKNESS_MODES = (None, "open", "closed")
MESH_COLUMNS = "mesh_vertices,mesh_triangles"            # appended with --mesh
MESH_CLOSED_COLUMNS = "euler_characteristic"             # ... and behind them with --mesh closed
MESH_MODES = (None, "open", "closed")
PIECES_COLUMNS = "pieces,largest_piece_voxels"           # appended with --pieces
CORES_COLUMNS = "cores"                                  # appended with --cores
PIECES_MODES = (None, 6, 18, 26)
LOCAL_THICKNESS_COLUMNS = "local_radius_mean,local_radius_std,local_radius_min"  # appended with --local-thickness
CONTACT_COLUMNS = "neighbours,contact_area,contact_fraction,largest_contact_id,largest_contact_area"  # --contacts
CONTACT_MODES = (None, 6, 18, 26)
CONTACT_CSV_COLUMNS = ("id_a,id_b,faces_x,faces_y,faces_z,edges_xy,edges_xz,edges_yz,corners,contact_area,fraction_a,"
                       "fraction_b")
INTENSITY_COLUMNS = ("intensity_mean,intensity_std,intensity_min,intensity_max,intensity_median,intensity_p05,"
                     "intensity_p95,wcx,wcy,wcz")                                          # appended with --image
RING_COLUMNS = "ring_voxels,ring_mean,ring_std,contrast"                                  # --intensity-ring
BRANCH_COLUMNS = ("graph_components,graph_endpoints,graph_junctions,graph_branches,graph_rings,graph_corner_loops,"
                  "graph_cycles,graph_length,branch_length_mean,longest_branch")             # appended with --branches
PARENT_COLUMNS = "parent,inside_fraction"                                                   # appended with --parents
NEAR_COLUMNS = "near_partners,nearest_id,nearest_gap,near_voxels,near_fraction"             # appended with --near
BRANCH_CSV_COLUMNS = "id,branch,kind,node_a,node_b,voxels,length,chord,tortuosity,ax,ay,az,bx,by,bz"
BRANCH_RADIUS_COLUMNS = "radius_mean,radius_min,radius_max"                               # --branches with --thickness
NODE_CSV_COLUMNS = "id,node,type,voxels,internal_links,x,y,z,branch_ends"
NODE_TYPES = ("isolated", "endpoint", "junction", "ring-anchor")
BRANCH_KINDS = ("endpoint-endpoint", "endpoint-junction", "junction-junction", "self-loop", "corner-loop", "ring")
# (|dx|, |dy|, |dz|) of the link classes, columns 5 .. 11 of sk_skeleton_graph
LINK_CLASSES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))

# An eigenvalue of the covariance matrix below this share of the largest one is the round-off of an exactly flat
# object (a line, a one-voxel-thick sheet) and is set to 0 together with negative round-off: 2 sqrt(5 lambda) would
# otherwise turn 1e-16 of noise into 1e-8 of axis.
FLAT_EIGENVALUE = 1e-12

_LOG_LEVELS = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]


def _spacing(spacing) -> Tuple[float, float, float]:
    if isinstance(spacing, Tensor):
        spacing = spacing.detach().cpu().tolist()
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(v > 0 for v in s):
        raise ValueError(f"spacing must be three positive numbers (x, y, z), got {spacing}")
    return s


def derive(sums: Tensor, boxes: Tensor, shape, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The derived columns of ``stats_per_instance`` from the kernel's (N, 13) int64 sums and (N, 6) int32 boxes of a
    mask of ``shape`` (X, Y, Z), in float64, on the tensors' own device (host tensors included; ``stats_per_instance``
    calls it on host copies).

    ``axis_lengths`` are ``2 sqrt(5 lambda_k)``, descending, of the eigenvalues of the covariance matrix of the voxel
    centres in physical units: the full axes of the solid ellipsoid with the same second moments.  The eigenvalues
    of the N 3 x 3 matrices are computed by LAPACK on the host (a few KiB either way)."""
    sx, sy, sz = _spacing(spacing)
    X, Y, Z = (int(v) for v in shape)
    sums = sums.to(torch.int64)
    boxes = boxes.to(torch.int32)
    dev = sums.device
    s = torch.tensor([sx, sy, sz], dtype=torch.float64, device=dev)
    f = sums.to(torch.float64)
    n = f[:, 0]
    mean = f[:, 1:4] / n[:, None]                                   # index units
    diag = f[:, 4:7] / n[:, None] - mean * mean
    off = f[:, 7:10] / n[:, None] - torch.stack((mean[:, 0] * mean[:, 1], mean[:, 0] * mean[:, 2],
                                                 mean[:, 1] * mean[:, 2]), dim=1)
    cov = torch.empty((sums.shape[0], 3, 3), dtype=torch.float64, device=dev)
    for i in range(3):
        cov[:, i, i] = diag[:, i]
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        cov[:, i, j] = cov[:, j, i] = off[:, k]
    cov = cov * (s[:, None] * s[None, :])
    cov[sums[:, 0] == 1] = 0.0                                      # a single voxel has no extent
    lam = torch.linalg.eigvalsh(cov.cpu()).flip(-1).to(dev) if cov.shape[0] else cov.new_empty((0, 3))
    lam = torch.where(lam > FLAT_EIGENVALUE * lam[:, :1], lam, torch.zeros_like(lam))
    faces = sums[:, 10:13]
    lim = torch.tensor([X - 1, Y - 1, Z - 1], dtype=torch.int32, device=dev)
    return {
        "voxels": sums[:, 0],
        "volume": n * (sx * sy * sz),
        "bbox": boxes,
        "touches_border": ((boxes[:, :3] == 0) | (boxes[:, 3:] == lim)).any(dim=1),
        "centroid": mean * s,
        "face_area": f[:, 10] * (sy * sz) + f[:, 11] * (sx * sz) + f[:, 12] * (sx * sy),
        "faces": faces,
        "axis_lengths": 2.0 * torch.sqrt(5.0 * lam),
    }


def class_areas(spacing=(1.0, 1.0, 1.0)) -> Tensor:
    """(30) float64 host tensor: the mesh area of one cell of each class of ``mc_table.CLASS_TRIANGLES`` at the voxel
    spacing (sx, sy, sz).  A triangle of type (a, b, c) has the cross product (a sy sz, b sx sz, c sx sy) / 4 and half
    its length as area; a class sums its triangles in the table's order, so the value is the same wherever it is
    computed."""
    sx, sy, sz = _spacing(spacing)
    tri = [math.sqrt((a * sy * sz) ** 2 + (b * sx * sz) ** 2 + (c * sx * sy) ** 2) / 8.0 for a, b, c in TRIANGLE_TYPES]
    out = []
    for row in CLASS_TRIANGLES:
        area = 0.0
        for n, t in zip(row, tri):
            area += n * t
        out.append(area)
    return torch.tensor(out, dtype=torch.float64)


def mesh_area(cells: Tensor, spacing=(1.0, 1.0, 1.0)) -> Tensor:
    """(N) float64 host tensor: ``cells.double() @ class_areas(spacing)`` of (N, 30) cell counts, summed on the host
    class by class in the table's order, so that a row's area does not depend on how many rows are computed with it or
    on a BLAS: the dict, the CSV file and ``get_surface_area`` agree to the last bit."""
    c = cells.cpu().to(torch.float64)
    area = torch.zeros(c.shape[0], dtype=torch.float64)
    for k, a in enumerate(class_areas(spacing).tolist()):
        area += c[:, k] * a
    return area


def surface_columns(cells: Tensor, volume: Tensor, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """``surface_area`` and ``surface_to_volume`` (float64, host) from the (N, 30) cell counts and the (N) volumes"""
    area = mesh_area(cells, spacing)
    return {"surface_area": area, "surface_to_volume": area / volume.cpu().to(torch.float64)}


def skeleton_columns(graph: Tensor, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The skeleton columns (host tensors) from the (N, 12) int64 rows of ``sk_skeleton_graph``:

    ``skeleton_voxels``, ``skeleton_endpoints`` (degree 1) and ``skeleton_junctions`` (degree >= 3), int64: the
    kernel's columns 0, 2 and 4.  ``skeleton_links``, int64: the sum of columns 5 .. 11, every pair of 26-neighbouring
    skeleton voxels once.  ``skeleton_branches`` = ``skeleton_links`` - column 3, int64: contracting every chain voxel
    (degree 2) takes one link with it, so this many edges remain between the other voxels; it is half the degree sum
    of the non-chain voxels.  A rod has 1, a T has 3, and a closed ring made of chain voxels only has 0: it has no
    voxel for a branch to end at.  ``skeleton_length``, float64: sum over the classes of links times
    ``sqrt((a sx)^2 + (b sy)^2 + (c sz)^2)``, summed class by class in the table's order as ``mesh_area`` does, so
    that the dict and the CSV file agree to the last bit; 0.0 for an empty skeleton.

    Known bias: every link counts.  Where three skeleton voxels are pairwise 26-neighbours -- a corner that Lee
    thinning leaves as a small triangle -- all three sides enter the length and the link count, and the corner voxels
    reach degree 3, so a path through such a corner is measured a little long and the corner counts as junction
    voxels."""
    sx, sy, sz = _spacing(spacing)
    g = graph.cpu().to(torch.int64)
    links = g[:, 5:12].sum(dim=1)
    length = torch.zeros(g.shape[0], dtype=torch.float64)
    for k, (a, b, c) in enumerate(LINK_CLASSES):
        length += g[:, 5 + k].to(torch.float64) * math.sqrt((a * sx) ** 2 + (b * sy) ** 2 + (c * sz) ** 2)
    return {"skeleton_voxels": g[:, 0].clone(), "skeleton_length": length, "skeleton_endpoints": g[:, 2].clone(),
            "skeleton_junctions": g[:, 4].clone(), "skeleton_links": links, "skeleton_branches": links - g[:, 3]}


def _link_steps(spacing):
    sx, sy, sz = _spacing(spacing)
    return [math.sqrt((a * sx) ** 2 + (b * sy) ** 2 + (c * sz) ** 2) for a, b, c in LINK_CLASSES]


def branch_lengths(branches: Tensor, spacing=(1.0, 1.0, 1.0)) -> Tensor:
    """(Nb) float64, host: the length of every row of the (Nb, 18) branch table at the voxel spacing -- its links per
    direction class (columns 4 .. 10) times the class's step, summed class by class in the table's order"""
    br = branches.cpu().to(torch.int64).reshape(-1, 18)
    length = torch.zeros(br.shape[0], dtype=torch.float64)
    for k, step in enumerate(_link_steps(spacing)):
        length += br[:, 4 + k].to(torch.float64) * step
    return length


def branch_kinds(nodes: Tensor, branches: Tensor) -> np.ndarray:
    """(Nb) int64: the place in ``BRANCH_KINDS`` of every row of the branch table.  A ring is the branch of a ring anchor;
    a corner loop is a self-loop with exactly one chain voxel whose two end voxels are 26-neighbours -- a triangle of
    pairwise adjacent voxels, which cannot enclose anything; any other branch with both ends in one node is a
    self-loop; the rest go by the types of their two nodes."""
    nd = nodes.cpu().numpy().astype(np.int64).reshape(-1, 8)
    br = branches.cpu().numpy().astype(np.int64).reshape(-1, 18)
    ta, tb = nd[br[:, 1], 1], nd[br[:, 2], 1]
    same = br[:, 1] == br[:, 2]
    gap = np.abs(br[:, 11:14] - br[:, 14:17]).max(1) if br.shape[0] else np.zeros(0, np.int64)
    kind = (ta == 2).astype(np.int64) + (tb == 2)            # 0, 1 or 2 junction ends
    kind[same] = 3
    kind[same & (br[:, 3] == 1) & (gap == 1)] = 4
    kind[ta == 3] = 5
    return kind


def branch_columns(nodes: Tensor, branches: Tensor, N: int, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The traced-graph columns (host tensors, N rows) from the node and branch tables of
    ``lib.instance_skeleton_branches`` -- column 0 of both the instance's index 0 .. N - 1 -- and the spacing; a pure
    function of its arguments:

    ``graph_components``: the connected pieces of the skeleton, from a union-find over the nodes along the branches (a
    node's own voxels are connected, a branch joins its two nodes).  ``graph_endpoints``, ``graph_junctions``,
    ``graph_rings``: the nodes of type 1, 2 and 3 -- junctions as NODES, however many voxels each has.
    ``graph_branches``: the rows of the branch table.  ``graph_corner_loops``: ``branch_kinds`` says what they are.
    ``graph_cycles`` = branches - nodes + components - corner loops: the independent loops of the traced graph, a
    corner's triangle not counted.  All int64.

    ``graph_length``, float64: the links of the instance's branches per direction class, summed as integers, times the
    class's step, class by class in the table's order as ``skeleton_columns`` does; the internal links of junctions
    are not in it.  ``branch_length_mean`` = ``graph_length / graph_branches`` and ``longest_branch``, the largest
    ``branch_lengths`` value.  An empty skeleton gives zeros in every column, never NaN."""
    N = int(N)
    nd = nodes.cpu().numpy().astype(np.int64).reshape(-1, 8)
    br = branches.cpu().numpy().astype(np.int64).reshape(-1, 18)
    steps = _link_steps(spacing)
    if nd.shape[0] and (nd[:, 0].min() < 0 or nd[:, 0].max() >= N):
        raise ValueError(f"the node table names instance {int(nd[:, 0].max())} and there are {N}")
    # union-find by minimum label: a branch pulls both of its nodes to the smaller label, then every label jumps
    label = np.arange(nd.shape[0])
    while br.shape[0]:
        low = np.minimum(label[br[:, 1]], label[br[:, 2]])
        new = label.copy()
        np.minimum.at(new, br[:, 1], low)
        np.minimum.at(new, br[:, 2], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    count = lambda rows: torch.from_numpy(np.bincount(rows, minlength=N).astype(np.int64))  # noqa: E731
    kinds = branch_kinds(nodes, branches)
    out = {"graph_components": count(nd[label == np.arange(nd.shape[0]), 0]),
           "graph_endpoints": count(nd[nd[:, 1] == 1, 0]), "graph_junctions": count(nd[nd[:, 1] == 2, 0]),
           "graph_branches": count(br[:, 0]), "graph_rings": count(nd[nd[:, 1] == 3, 0]),
           "graph_corner_loops": count(br[kinds == 4, 0])}
    out["graph_cycles"] = out["graph_branches"] - count(nd[:, 0]) + out["graph_components"] - out["graph_corner_loops"]
    length = torch.zeros(N, dtype=torch.float64)
    for k, step in enumerate(steps):
        links = np.zeros(N, np.int64)
        np.add.at(links, br[:, 0], br[:, 4 + k])
        length += torch.from_numpy(links).to(torch.float64) * step
    out["graph_length"] = length
    n_br = out["graph_branches"].to(torch.float64)
    out["branch_length_mean"] = torch.where(n_br > 0, length / n_br.clamp(min=1.0), torch.zeros_like(length))
    longest = np.zeros(N, np.float64)
    np.maximum.at(longest, br[:, 0], branch_lengths(branches, spacing).numpy())
    out["longest_branch"] = torch.from_numpy(longest)
    return out


def branch_radii(branches: Tensor, points: Tensor, owner: Tensor, dist2: Tensor) -> np.ndarray:
    """(Nb, 3) float64: mean, minimum and maximum of ``sqrt(dist2)`` over every branch's end voxel a, its chain voxels in
    the order of ``points`` and its end voxel b (once, where both ends are one voxel).  The values are gathered on the
    device through ``owner`` and the end voxels of the table; the mean is a plain left-to-right sum over the count,
    kept inside [minimum, maximum], as ``lib.instance_thickness`` forms it."""
    br = branches.long().reshape(-1, 18)
    at = lambda v: np.sqrt(dist2[v[:, 0], v[:, 1], v[:, 2]].cpu().numpy().astype(np.float64))  # noqa: E731
    ra, rb = at(br[:, 11:14]), at(br[:, 14:17])
    one_voxel = (br[:, 11:14] == br[:, 14:17]).all(1).cpu().numpy()
    chain = torch.nonzero(owner >= 0)[:, 0]
    row = owner[chain].cpu().numpy().astype(np.int64)
    radius = at(points.long()[chain])
    order = np.argsort(row, kind="stable")
    row, radius = row[order], radius[order]
    first = np.searchsorted(row, np.arange(br.shape[0] + 1))
    out = np.zeros((br.shape[0], 3), np.float64)
    for r in range(br.shape[0]):
        v = [ra[r]] + radius[first[r]:first[r + 1]].tolist() + ([] if one_voxel[r] else [rb[r]])
        total = 0.0
        for t in v:
            total += t
        out[r] = (min(max(total / len(v), min(v)), max(v)), min(v), max(v))
    return out


def format_branches_csv(mask_path: str, ids, nodes: Tensor, branches: Tensor, spacing=(1.0, 1.0, 1.0), keep=None,
                        radius=None) -> str:
    """The text of ``_branches.csv``: two header lines (file, spacing), the column names ``BRANCH_CSV_COLUMNS`` and one
    row per branch in table order: the instance's id, the branch's row in the table, its kind (``BRANCH_KINDS``), the
    rows of its two nodes in ``_nodes.csv``, its chain voxels, its length (``branch_lengths``), the chord -- the
    distance between its end voxels at the spacing -- the tortuosity ``length / chord`` (empty where the chord is 0:
    rings and loops that return to their voxel) and both end voxels.  ``keep`` (N bools) leaves out the branches of
    the instances it does not name; ``radius`` (Nb, 3; ``branch_radii``) appends ``BRANCH_RADIUS_COLUMNS``."""
    spacing = _spacing(spacing)
    ids = ids.cpu().tolist() if isinstance(ids, Tensor) else list(ids)
    br = branches.cpu().numpy().astype(np.int64).reshape(-1, 18)
    kinds = branch_kinds(nodes, branches).tolist()
    length = branch_lengths(branches, spacing).tolist()
    lines = [f"Mask File: {mask_path}\n", "Spacing: {} {} {}\n".format(*(repr(v) for v in spacing)),
             BRANCH_CSV_COLUMNS + ("," + BRANCH_RADIUS_COLUMNS if radius is not None else "") + "\n"]
    for r, row in enumerate(br.tolist()):
        if keep is not None and not keep[row[0]]:
            continue
        chord = math.sqrt(sum(((a - b) * s) ** 2 for a, b, s in zip(row[11:14], row[14:17], spacing)))
        cells = [int(ids[row[0]]), r, BRANCH_KINDS[kinds[r]], row[1], row[2], row[3], repr(length[r]), repr(chord),
                 repr(length[r] / chord) if chord > 0 else "", *row[11:17]]
        if radius is not None:
            cells += [repr(float(v)) for v in radius[r]]
        lines.append(",".join(str(c) for c in cells) + "\n")
    return "".join(lines)


def format_nodes_csv(mask_path: str, ids, nodes: Tensor, keep=None) -> str:
    """The text of ``_nodes.csv``: a header line (file), the column names ``NODE_CSV_COLUMNS`` and one row per node in
    table order: the instance's id, the node's row in the table (what ``_branches.csv`` names), its type
    (``NODE_TYPES``), voxels, internal links, first voxel and the branch ends attached.  ``keep`` as in
    ``format_branches_csv``."""
    ids = ids.cpu().tolist() if isinstance(ids, Tensor) else list(ids)
    lines = [f"Mask File: {mask_path}\n", NODE_CSV_COLUMNS + "\n"]
    for r, row in enumerate(nodes.cpu().numpy().astype(np.int64).reshape(-1, 8).tolist()):
        if keep is not None and not keep[row[0]]:
            continue
        lines.append(",".join(str(c) for c in [int(ids[row[0]]), r, NODE_TYPES[row[1]], *row[2:]]) + "\n")
    return "".join(lines)


def thickness_columns(max_d2: Tensor, skel_stats: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """The width columns (float64 host tensors) from the (N) largest squared distances of ``instance_thickness`` and,
    when given, its (N, 3) skeleton statistics:

    ``inscribed_radius`` = ``sqrt(max_d2)``: the largest distance from a voxel centre of the instance to the nearest
    voxel centre outside it.  Distances run between voxel centres (scipy's convention) and no half-voxel correction is
    applied: a sheet one voxel thick has a radius of one spacing, a tube k voxels across about (k + 1) / 2 spacings.
    It is a radius; doubling it is the reader's choice.  Deliberate: an instance that is alone in the volume in open
    mode has no outside voxel and reports ``inf``.

    ``skeleton_radius_mean``, ``skeleton_radius_min``, ``skeleton_radius_max``: ``sqrt(D2)`` over the instance's
    skeleton voxels; 0.0 for an empty skeleton."""
    # numpy's square root is the correctly rounded one at every length of the array (the host library's vectorised
    # one is not: sqrt(2.0) comes out one unit low), so a row's radius does not depend on the rows computed with it
    out = {"inscribed_radius": torch.from_numpy(np.sqrt(max_d2.cpu().to(torch.float64).numpy()))}
    if skel_stats is not None:
        st = skel_stats.cpu().to(torch.float64).reshape(-1, 3)
        for k, name in enumerate(SKELETON_RADIUS_COLUMNS.split(",")):
            out[name] = st[:, k].clone()
    return out


def local_thickness_columns(table, N: int) -> Dict[str, Tensor]:
    """The local-thickness columns (float64 host tensors, N rows) from the (K, 3) table of
    ``lib.instance_local_thickness`` -- ``(row 1..N, T2 bit pattern, voxels)``, sorted by row and then value:

    ``local_radius_mean``: the mean of ``sqrt(T2)`` over the instance's voxels, a plain left-to-right sum of
    ``voxels * sqrt(value)`` in ascending order of the values over the voxel count, kept inside [minimum, maximum]
    (rounding can put the mean of equal values a unit outside them); ``local_radius_std``: the population standard
    deviation around that mean, accumulated in the same order, 0.0 for a single value; ``local_radius_min``: the
    thinnest place.  The maximum is ``inscribed_radius`` (per instance ``max T2 = max D2``).  The radii follow
    ``thickness_columns``' conventions: between voxel centres, a radius and not a diameter, no half-voxel correction.
    An instance alone in the volume in open mode has ``inf`` everywhere and reports ``inf, 0.0, inf``; a row without
    voxels reports 0.0 in all three (no real radius is 0)."""
    t = np.asarray(table.cpu() if isinstance(table, Tensor) else table, dtype=np.int64).reshape(-1, 3)
    # numpy's square root is the correctly rounded one at every length of the array (thickness_columns)
    radius = np.sqrt(np.ascontiguousarray(t[:, 1]).view(np.float64))
    first = np.searchsorted(t[:, 0], np.arange(1, int(N) + 2))
    out = np.zeros((int(N), 3), np.float64)
    for r in range(int(N)):
        v, c = radius[first[r]:first[r + 1]].tolist(), t[first[r]:first[r + 1], 2].tolist()
        if not v:
            continue
        if v[0] == float("inf"):                             # ascending: every value of the row is inf
            out[r] = (float("inf"), 0.0, float("inf"))
            continue
        n, total = 0, 0.0
        for value, count in zip(v, c):                       # one order, whatever numpy does
            n += count
            total += count * value
        mean = min(max(total / n, v[0]), v[-1])
        spread = 0.0
        for value, count in zip(v, c):
            spread += count * ((value - mean) * (value - mean))
        out[r] = (mean, float(np.sqrt(np.float64(spread / n))) if len(v) > 1 else 0.0, v[0])
    return {name: torch.from_numpy(out[:, k].copy()) for k, name in enumerate(LOCAL_THICKNESS_COLUMNS.split(","))}


def mesh_columns(counts: Tensor, closed: bool) -> Dict[str, Tensor]:
    """The mesh columns (int64 host tensors) from the (N, 2) counts of ``instance_mesh_counts``: ``mesh_vertices`` and
    ``mesh_triangles``, and for a closed mesh ``euler_characteristic`` = V - E + F = V - F / 2.  A closed mesh is
    edge-manifold -- every edge has two triangles, E = 3 F / 2 -- so the value is an integer: 2 per surface component
    less twice its handles (a ball 2, a ball with a cavity 4, a torus 0).  Two parts of an instance that meet in a voxel
    edge or corner only are separate surfaces.  An open mesh has boundary edges and no such identity: no column."""
    c = counts.cpu().to(torch.int64).reshape(-1, 2)
    out = {"mesh_vertices": c[:, 0].clone(), "mesh_triangles": c[:, 1].clone()}
    if closed:
        if bool((c[:, 1] % 2 != 0).any()):
            raise RuntimeError("a closed mesh with an odd number of triangles: the counts are not those of closed mode")
        out["euler_characteristic"] = c[:, 0] - c[:, 1] // 2
    return out


def pieces_columns(table: Tensor, ids) -> Dict[str, Tensor]:
    """The piece columns (int64 host tensors, one row per id of ``ids``, ascending) from the (P, 6) table of
    ``lib.morphology.label_components``: ``pieces``, the connected pieces the id is in, and ``largest_piece_voxels``,
    the voxels of the largest of them.  An id with ``pieces > 1`` is not one body, and what the other columns say of
    its skeleton, radius or surface distances describes no physical object."""
    t = table.cpu().numpy().astype(np.int64).reshape(-1, 6)
    ids = np.asarray(ids.cpu() if isinstance(ids, Tensor) else ids, dtype=np.int64).reshape(-1)
    row = np.searchsorted(ids, t[:, 0])
    if t.shape[0] and (row.max(initial=0) >= ids.size or not np.array_equal(ids[row], t[:, 0])):
        raise ValueError("the table names an id that is not among ids")
    count = np.zeros(ids.size, np.int64)
    largest = np.zeros(ids.size, np.int64)
    np.add.at(count, row, 1)
    np.maximum.at(largest, row, t[:, 1])
    return {"pieces": torch.from_numpy(count), "largest_piece_voxels": torch.from_numpy(largest)}


def cores_columns(table: Tensor, ids) -> Dict[str, Tensor]:
    """The column that ``stats_per_instance(cores=R)`` adds, from the (P, 6) table of ``utils.split.core_pieces``:
    ``cores``, the 6-connected pieces that remain of the id at depth R.  An id with two or more is what
    ``utils.split.split`` cuts at that radius; one with none is thinner than R everywhere."""
    t = table.cpu().numpy() if isinstance(table, Tensor) else np.asarray(table)
    ids = np.asarray(ids.cpu() if isinstance(ids, Tensor) else ids, dtype=np.int64).reshape(-1)
    count = np.zeros(ids.size, np.int64)
    if t.size:
        np.add.at(count, np.searchsorted(ids, t[:, 0].astype(np.int64)), 1)
    return {"cores": torch.from_numpy(count)}


def _cores_radius(cores):
    if cores is None:
        return None
    if isinstance(cores, (bool, np.bool_)) or not isinstance(cores, (int, float, np.integer, np.floating)) \
            or not 0 <= float(cores) < float("inf"):
        raise ValueError(f"cores must be None or a non-negative finite radius, got {cores!r}")
    return float(cores)


def _contact_table(table) -> np.ndarray:
    t = table.cpu().numpy() if isinstance(table, Tensor) else np.asarray(table)
    return t.astype(np.int64).reshape(-1, 9) if t.size else np.zeros((0, 9), np.int64)


def contact_area(table, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """(P) float64: the face-contact area of every row of a (P, 9) contact table (``lo, hi, c0 .. c6``) at the voxel
    spacing, ``c0 sy sz + c1 sx sz + c2 sx sy`` -- ``derive``'s expression for ``face_area``, so an instance wholly
    enclosed by another has a fraction of exactly 1.  Edge and corner contacts have no area.  The one place the area is
    computed: the dict, both CSV files and ``utils.merge`` call it, so they agree to the last bit."""
    sx, sy, sz = _spacing(spacing)
    t = _contact_table(table).astype(np.float64)
    return t[:, 2] * (sy * sz) + t[:, 3] * (sx * sz) + t[:, 4] * (sx * sy)


def _contact_pairs(table, ids, face_area, spacing):
    """(t, ia, ib, area, fa): the rows of the table between two instances (a row with id 0, the background, is left
    out), the positions of their two ids in ``ids``, their contact areas and the (N) face areas as float64."""
    ids = np.asarray(ids.cpu() if isinstance(ids, Tensor) else ids, dtype=np.int64).reshape(-1)
    fa = np.asarray(face_area.cpu() if isinstance(face_area, Tensor) else face_area, dtype=np.float64).reshape(-1)
    if fa.size != ids.size:
        raise ValueError(f"face_area has {fa.size} values for {ids.size} ids")
    t = _contact_table(table)
    t = t[t[:, 0] != 0]
    ia, ib = np.searchsorted(ids, t[:, 0]), np.searchsorted(ids, t[:, 1])
    if t.shape[0] and (max(ia.max(), ib.max()) >= ids.size or not np.array_equal(ids[ia], t[:, 0])
                       or not np.array_equal(ids[ib], t[:, 1])):
        raise ValueError("the table names an id that is not among ids")
    return t, ia, ib, contact_area(t, spacing), fa


def contact_columns(table, ids, face_area, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The contact columns (host tensors, one row per id of ``ids``, ascending) from the (P, 9) contact table with ids in
    its first two columns (``stats_per_instance``'s ``contact_table``) and the (N) ``face_area`` of ``derive``:

    ``neighbours`` int64: the distinct instances the id touches at the table's connectivity.  ``contact_area`` float64:
    its face-contact area (``contact_area``) summed over the partners in ascending order of their ids.
    ``contact_fraction`` = ``contact_area / face_area``: the share of the instance's exposed faces that lie against
    another instance (the rest faces background or the volume's border).  ``largest_contact_id`` int64 and
    ``largest_contact_area`` float64: the partner with the largest face-contact area, the smaller id on a tie; 0 and 0.0
    when no partner shares a face.  Rows of the table against the background (id 0) are ignored."""
    t, ia, ib, area, fa = _contact_pairs(table, ids, face_area, spacing)
    n = fa.size
    me = np.concatenate((ia, ib))
    partner = np.concatenate((t[:, 1], t[:, 0]))
    ar = np.concatenate((area, area))
    neighbours = np.zeros(n, np.int64)
    np.add.at(neighbours, me, 1)
    total = np.zeros(n, np.float64)
    order = np.lexsort((partner, me))
    np.add.at(total, me[order], ar[order])                   # unbuffered: one order, ascending partner id
    best_id, best_area = np.zeros(n, np.int64), np.zeros(n, np.float64)
    order = np.lexsort((partner, -ar, me))                   # per id: largest area first, then the smaller partner
    first = order[np.concatenate(([True], me[order][1:] != me[order][:-1]))] if order.size else order
    first = first[ar[first] > 0]
    best_id[me[first]], best_area[me[first]] = partner[first], ar[first]
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = total / fa
    return {"neighbours": torch.from_numpy(neighbours), "contact_area": torch.from_numpy(total),
            "contact_fraction": torch.from_numpy(fraction), "largest_contact_id": torch.from_numpy(best_id),
            "largest_contact_area": torch.from_numpy(best_area)}


def format_contacts_csv(mask_path: str, table, ids, face_area, spacing=(1.0, 1.0, 1.0), connectivity: int = 6) -> str:
    """The text of ``_contacts.csv``: two header lines (file; spacing and connectivity), the column names, and one row
    per touching pair of instances sorted by ``(id_a, id_b)``: the seven counts of the (P, 9) contact table (ids in its
    first two columns), the pair's ``contact_area`` and that area over the ``face_area`` of either side.  Floats are
    printed with ``repr``.  A pure function of its arguments."""
    spacing = _spacing(spacing)
    t, ia, ib, area, fa = _contact_pairs(table, ids, face_area, spacing)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr_a, fr_b = area / fa[ia], area / fa[ib]
    lines = [f"Mask File: {mask_path}\n",
             "Spacing: {} {} {} Connectivity: {}\n".format(*(repr(v) for v in spacing), int(connectivity)),
             CONTACT_CSV_COLUMNS + "\n"]
    for k in np.lexsort((t[:, 1], t[:, 0])).tolist():
        lines.append(",".join([*(str(v) for v in t[k].tolist()), repr(float(area[k])), repr(float(fr_a[k])),
                               repr(float(fr_b[k]))]) + "\n")
    return "".join(lines)


def _int_table(t, width: int) -> np.ndarray:
    t = t.cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)
    return t.astype(np.int64).reshape(-1, width)


def _mean_std(m: np.ndarray):
    """(mean, std) float64 of the rows ``n, S v, S v^2, ...``: ``S v / n`` and ``sqrt((n S v^2 - (S v)^2) / n^2)``, the
    numerator in exact integers; ``nan`` where n is 0"""
    mean, std = np.full(m.shape[0], np.nan), np.full(m.shape[0], np.nan)
    for i, (n, sv, svv) in enumerate(m[:, :3].tolist()):
        if n > 0:
            mean[i] = sv / n
            std[i] = float(np.sqrt(np.float64((n * svv - sv * sv) / (n * n))))
    return mean, std


def intensity_columns(moments, extrema, hist, shift: int, spacing=(1.0, 1.0, 1.0)) -> Dict[str, Tensor]:
    """The intensity columns (host tensors, float64 unless noted) from the tables of ``lib.instance_intensity``:
    (N, 6) ``n, S v, S v^2, S v x, S v y, S v z``, (N, 2) ``min, max`` and the (N, 256) histogram with bins ``v >> shift``:

    ``intensity_mean`` = ``S v / n``.  ``intensity_std`` = ``sqrt((n S v^2 - (S v)^2) / n^2)``, the population standard
    deviation, its numerator formed in exact integer arithmetic.  ``intensity_min``, ``intensity_max``, int64.
    ``intensity_median``, ``intensity_p05``, ``intensity_p95``, int64: the nearest-rank quantile from the histogram, the
    lowest bin whose cumulative count reaches ``lib.nearest_rank(n, p) + 1``, reported as ``bin << shift``.  At
    ``shift = 0`` (every 8-bit image) that is ``np.sort(values)[nearest_rank(n, p)]``, one of the samples; at
    ``shift > 0`` it is the LOWER EDGE of the bin that holds that sample.  ``weighted_centroid`` (N, 3) =
    ``(S v x, S v y, S v z) / S v * spacing``, ``nan`` where ``S v`` is 0 (an instance on an all-zero image).  A row
    without voxels has ``nan`` floats and 0 quantiles."""
    s = np.array(_spacing(spacing), np.float64)
    m, e, h = _int_table(moments, 6), _int_table(extrema, 2), _int_table(hist, 256)
    shift = int(shift)
    if not (m.shape[0] == e.shape[0] == h.shape[0]) or not 0 <= shift <= 8:
        raise ValueError(f"tables of {m.shape[0]}, {e.shape[0]} and {h.shape[0]} rows, shift {shift}: the rows must agree "
                         "and the shift lie in 0 .. 8")
    mean, std = _mean_std(m)
    cum = np.cumsum(h, axis=1)
    quant = np.zeros((m.shape[0], 3), np.int64)
    for i, n in enumerate(m[:, 0].tolist()):
        if n > 0:
            for k, p in enumerate((50, 5, 95)):
                quant[i, k] = int(np.searchsorted(cum[i], nearest_rank(n, p) + 1)) << shift
    sv = m[:, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        centroid = np.where(m[:, 1:2] > 0, m[:, 3:6].astype(np.float64) / sv[:, None], np.nan) * s
    return {"intensity_mean": torch.from_numpy(mean), "intensity_std": torch.from_numpy(std),
            "intensity_min": torch.from_numpy(e[:, 0].copy()), "intensity_max": torch.from_numpy(e[:, 1].copy()),
            "intensity_median": torch.from_numpy(quant[:, 0].copy()), "intensity_p05": torch.from_numpy(quant[:, 1].copy()),
            "intensity_p95": torch.from_numpy(quant[:, 2].copy()), "weighted_centroid": torch.from_numpy(centroid)}


def ring_columns(ring_moments, moments) -> Dict[str, Tensor]:
    """The ring columns (host tensors) from the (N, 6) moments of ``lib.intensity_ring`` and those of the instances
    themselves: ``ring_voxels`` int64; ``ring_mean`` and ``ring_std`` float64 as ``intensity_mean`` and
    ``intensity_std``, ``nan`` where the ring is empty; ``contrast`` = ``(intensity_mean - ring_mean) / (intensity_mean +
    ring_mean)``, in [-1, 1], ``nan`` where the ring is empty or the denominator is 0."""
    r, m = _int_table(ring_moments, 6), _int_table(moments, 6)
    if r.shape[0] != m.shape[0]:
        raise ValueError(f"{r.shape[0]} ring rows for {m.shape[0]} instances")
    ring_mean, ring_std = _mean_std(r)
    mean = _mean_std(m)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        contrast = np.where(mean + ring_mean != 0, (mean - ring_mean) / (mean + ring_mean), np.nan)
    return {"ring_voxels": torch.from_numpy(r[:, 0].copy()), "ring_mean": torch.from_numpy(ring_mean),
            "ring_std": torch.from_numpy(ring_std), "contrast": torch.from_numpy(contrast)}


def format_histograms_csv(mask_path: str, ids, hist, shift: int) -> str:
    """The text of ``_histograms.csv``: two header lines (the file; ``Bin width: 2^shift``), ``id,b0,...,b255`` and one
    row per instance: the voxels whose sample v has ``v >> shift`` equal to the bin.  A pure function of its arguments."""
    ids = ids.cpu().tolist() if isinstance(ids, Tensor) else list(ids)
    h = _int_table(hist, 256)
    if h.shape[0] != len(ids):
        raise ValueError(f"{h.shape[0]} histograms for {len(ids)} ids")
    lines = [f"Mask File: {mask_path}\n", f"Bin width: 2^{int(shift)}\n",
             "id," + ",".join(f"b{k}" for k in range(256)) + "\n"]
    for u, row in zip(ids, h.tolist()):
        lines.append(",".join(str(v) for v in (int(u), *row)) + "\n")
    return "".join(lines)


def points_volume(points: Tensor, graph: Tensor, shape) -> Tensor:
    """(X, Y, Z) int32, the row volume of ``lib.instance_skeleton_graph(..., want_volume=True)`` from the points of
    ``lib.instance_skeleton_branches``: 0 outside the skeletons, the instance's row 1 .. N on its skeleton voxels"""
    volume = torch.zeros(tuple(int(v) for v in shape), dtype=torch.int32, device=points.device)
    row = torch.repeat_interleave(torch.arange(1, graph.shape[0] + 1, device=points.device), graph[:, 0])
    p = points.long()
    volume[p[:, 0], p[:, 1], p[:, 2]] = row.to(torch.int32)
    return volume


def stats_per_instance(x: Tensor, anisotropy=(1.0, 1.0, 1.0), surface: Optional[str] = None,
                       skeleton: bool = False, thickness: Optional[str] = None,
                       mesh: Optional[str] = None, pieces: Optional[int] = None,
                       local_thickness: Optional[str] = None, contacts: Optional[int] = None,
                       image: Optional[Tensor] = None, intensity_ring=None, branches: bool = False,
                       skeleton_volume: Optional[Tensor] = None, cores=None, parents: Optional[Tensor] = None,
                       parent_min_fraction: float = 0.0, near=None, near_distance=None) -> Dict[str, Tensor]:
    """Measures every instance of ``x``, a device tensor (X, Y, Z) or (1, X, Y, Z) of any integer dtype, in one kernel
    pass; ``anisotropy`` is the voxel spacing along x, y and z of that tensor.

    Returns device tensors with one row per positive id, ascending like ``torch.unique``: ``id`` int64, ``voxels``
    int64, ``volume`` float64, ``bbox`` (N, 6) int32 ``[x0, y0, z0, x1, y1, z1]`` inclusive, ``touches_border`` bool,
    ``centroid`` (N, 3) float64 in physical units, ``face_area`` float64, ``faces`` (N, 3) int64 exposed faces with
    their normal along x / y / z, ``axis_lengths`` (N, 3) float64 descending, and ``sums`` (N, 13) int64, the raw
    accumulators.  (The reference's sketch of the same name returns ``id``, ``volume`` and a marching-cubes
    ``surface_area`` and cannot run: skoots/validate/compare.py:8-28.)

    ``surface="open"`` or ``"closed"`` adds, from one more kernel pass, ``mesh_cells`` (N, 30) int64, ``surface_area``
    float64 -- the area of the marching-cubes mesh of ``x == id``, which is what the reference's ``get_surface_area``
    returns -- and ``surface_to_volume`` = ``surface_area / volume``.  "open" is the reference's meaning: where an
    instance touches a face of the volume its surface stays open.  "closed" measures the mask padded with one layer of
    background.  Deliberate difference: an instance that fills the whole volume in open mode, or any instance of a
    volume with an extent below 2, has area 0 here; scikit-image raises there ("No surface found", "must be at least
    2x2x2"), which would fail the whole mask for one instance.

    ``skeleton=True`` adds ``skeleton_graph`` (N, 12) int64, the rows of ``sk_skeleton_graph`` for every instance
    thinned in its box (``lib.instance_skeleton_graph``), and the columns of ``skeleton_columns``: ``skeleton_voxels``,
    ``skeleton_length``, ``skeleton_endpoints``, ``skeleton_junctions``, ``skeleton_links``, ``skeleton_branches``
    (DESIGN.md §22).

    ``thickness="open"`` or ``"closed"`` adds ``dist2`` (X, Y, Z) float64, the exact squared Euclidean distance of every
    instance voxel to the nearest voxel outside its instance (``lib.instance_thickness``; "open" counts the voxels of
    the volume only, "closed" pads it with background), ``max_dist2`` (N) float64 and ``inscribed_radius`` =
    ``sqrt(max_dist2)``; together with ``skeleton=True`` also ``skeleton_radius_mean`` / ``_min`` / ``_max``, the radius
    sampled on the skeleton voxels (``thickness_columns``).

    ``mesh="open"`` or ``"closed"`` adds ``mesh_vertices`` and ``mesh_triangles`` (int64), the size of the mesh that
    ``lib.instance_meshes`` would return, from its count pass, and in closed mode ``euler_characteristic`` (int64;
    ``mesh_columns``).

    ``pieces=6``, ``18`` or ``26`` adds ``pieces`` and ``largest_piece_voxels`` (int64): the connected pieces of every
    id at that connectivity and the size of the largest, from ``lib.morphology.label_components`` (``pieces_columns``,
    DESIGN.md §26).

    ``local_thickness="open"`` or ``"closed"`` adds ``thick2`` (X, Y, Z) float64, for every instance voxel the squared
    radius of the largest ball inside its instance that holds it (``lib.instance_local_thickness``; the modes are those
    of ``thickness``, and when both name the same mode the distance transform runs once), ``max_dist2`` if ``thickness``
    did not add it, and ``local_radius_mean``, ``local_radius_std``, ``local_radius_min`` (``local_thickness_columns``,
    DESIGN.md §28).

    ``contacts=6``, ``18`` or ``26`` adds ``contact_table`` (P, 9) int64 -- one row ``id_a, id_b, c0 .. c6`` per pair of
    instances that touch at that connectivity, ``id_a < id_b``, sorted, from ``lib.instance_contacts`` -- and the
    columns of ``contact_columns``: ``neighbours``, ``contact_area``, ``contact_fraction``, ``largest_contact_id``,
    ``largest_contact_area``.

    ``image`` (a uint8 or uint16 tensor of the mask's shape on its device; ``lib.instance_intensity`` says what else is
    taken) adds ``intensity_moments`` (N, 6) int64, ``intensity_extrema`` (N, 2) int32, ``intensity_hist`` (N, 256) int64,
    ``intensity_shift`` (a Python int) and the columns of ``intensity_columns``: ``intensity_mean``, ``intensity_std``,
    ``intensity_min``, ``intensity_max``, ``intensity_median``, ``intensity_p05``, ``intensity_p95``,
    ``weighted_centroid``.  ``intensity_ring=D`` with it adds ``ring_moments`` (N, 6) int64, the image
    over the background within D (in the units of ``anisotropy``) that is nearest to this instance
    (``lib.intensity_ring``), and the columns of ``ring_columns``: ``ring_voxels``, ``ring_mean``, ``ring_std``,
    ``contrast``.  ``intensity_ring`` without ``image`` raises ``ValueError``.

    ``branches=True`` implies ``skeleton=True`` and adds the traced skeletons of ``lib.instance_skeleton_branches``
    (DESIGN.md §32): ``skeleton_nodes`` (Nn, 8) and ``skeleton_branch_table`` (Nb, 18) int32, ``skeleton_points`` (P, 3)
    and ``skeleton_owner`` (P) int32, and the columns of ``branch_columns``: ``graph_components``, ``graph_endpoints``,
    ``graph_junctions``, ``graph_branches``, ``graph_rings``, ``graph_corner_loops``, ``graph_cycles``,
    ``graph_length``, ``branch_length_mean``, ``longest_branch``.  ``skeleton_volume`` (an integer device volume with an
    instance's id on its skeleton voxels, what ``--save-skeletons`` writes) is traced instead of thinning anything.

    ``cores=R`` (a radius in the units of ``anisotropy``) adds ``cores`` (int64): the 6-connected pieces that remain of
    every id at depth R, steps 1 to 3 of ``utils.split.split`` (``utils.split.core_pieces``, ``cores_columns``, DESIGN.md
    §33).  An id with two or more is what ``split`` would cut at that radius.  The depth is that of ``thickness`` when
    that names "closed", else open.

    ``parents=P`` (an integer device volume of the mask's shape: a mask of other, larger objects) adds ``parent`` int64,
    the id of P that holds most of the instance's voxels, 0 for none, and ``inside_fraction`` float64, the share of the
    instance inside it: ``parent_id`` and ``inside_fraction`` of ``utils.relate.relate(x, P, parent_min_fraction)``
    (DESIGN.md §34).

    ``near=B`` (an integer device volume of the mask's shape) or ``near="self"`` with ``near_distance=D`` (in the units
    of ``anisotropy``) adds the columns of ``utils.proximity.proximity``'s per-instance table:
    ``near_partners`` int64, the instances of B -- or the other instances of the mask -- within D; ``nearest_id`` int64
    (0: none) and ``nearest_gap`` float64 (``inf``: none), the closest of them and the gap to it; ``near_voxels`` int64,
    the instance's voxels within D of any of them, and ``near_fraction`` float64, their share.  One without the other
    raises ``ValueError``."""
    if (near is None) != (near_distance is None):
        raise ValueError("near names what to measure the distance to and near_distance the distance: they come together")
    if isinstance(near, str) and near != "self":
        raise ValueError(f'near must be a mask or "self", got {near!r}')
    cores = _cores_radius(cores)
    if skeleton_volume is not None and not branches:
        raise ValueError("skeleton_volume is what branches=True traces: it needs branches")
    if intensity_ring is not None and image is None:
        raise ValueError("intensity_ring measures the image around every instance: it needs image")
    if contacts not in CONTACT_MODES or isinstance(contacts, bool):
        raise ValueError(f"contacts must be one of {CONTACT_MODES}, got {contacts!r}")
    if local_thickness not in THICKNESS_MODES:
        raise ValueError(f"local_thickness must be one of {THICKNESS_MODES}, got {local_thickness!r}")
    if pieces not in PIECES_MODES or isinstance(pieces, bool):
        raise ValueError(f"pieces must be one of {PIECES_MODES}, got {pieces!r}")
    if mesh not in MESH_MODES:
        raise ValueError(f"mesh must be one of {MESH_MODES}, got {mesh!r}")
    if surface not in SURFACE_MODES:
        raise ValueError(f"surface must be one of {SURFACE_MODES}, got {surface!r}")
    if thickness not in THICKNESS_MODES:
        raise ValueError(f"thickness must be one of {THICKNESS_MODES}, got {thickness!r}")
    spacing = _spacing(anisotropy)
    rows = id_rows(x)                                       # once, for both kernels
    ids, sums, boxes = instance_sums(x, rows)
    shape = tuple(x.shape[-3:])
    out = {"id": ids}
    # N rows of a few numbers: derived on the host, where the eigenvalues are computed anyway, and uploaded -- the
    # same machine code as format_csv runs, so the file and this dict agree to the last bit
    out.update({k: v.to(sums.device) for k, v in derive(sums.cpu(), boxes.cpu(), shape, spacing).items()})
    out["sums"] = sums
    if surface is not None:
        _, cells = instance_mesh_cells(x, closed=surface == "closed", rows=rows)
        out["mesh_cells"] = cells
        out.update({k: v.to(sums.device) for k, v in surface_columns(cells, out["volume"], spacing).items()})
    volume = None
    if branches:
        _, graph, nodes, table, points, owner = instance_skeleton_branches(x, rows, boxes, skeleton=skeleton_volume)
        out.update(skeleton_graph=graph, skeleton_nodes=nodes, skeleton_branch_table=table, skeleton_points=points,
                   skeleton_owner=owner)
        out.update({k: v.to(sums.device) for k, v in skeleton_columns(graph, spacing).items()})
        out.update({k: v.to(sums.device) for k, v in branch_columns(nodes, table, int(ids.numel()), spacing).items()})
        volume = [points_volume(points, graph, shape)] if thickness is not None else None
    elif skeleton:
        _, graph, *volume = instance_skeleton_graph(x, rows, boxes, want_volume=thickness is not None)
        out["skeleton_graph"] = graph
        out.update({k: v.to(sums.device) for k, v in skeleton_columns(graph, spacing).items()})
    if thickness is not None:
        _, max_d2, dist2, *skel = instance_thickness(x, spacing, thickness == "closed", rows,
                                                     volume[0] if volume else None)
        out["max_dist2"], out["dist2"] = max_d2, dist2
        out.update({k: v.to(sums.device) for k, v in thickness_columns(max_d2, *skel).items()})
    if mesh is not None:
        _, counts = instance_mesh_counts(x, mesh == "closed", rows)
        out.update({k: v.to(sums.device) for k, v in mesh_columns(counts, mesh == "closed").items()})
    if pieces is not None:
        from ..lib.morphology import label_components
        out.update({k: v.to(sums.device) for k, v in pieces_columns(label_components(x, pieces, rows=rows)[1], ids).items()})
    if local_thickness is not None:
        have = (out["dist2"], out["max_dist2"]) if thickness == local_thickness else None
        _, table, thick2, max_d2 = instance_local_thickness(x, spacing, local_thickness == "closed", rows, have)
        out["thick2"] = thick2
        out.setdefault("max_dist2", max_d2)
        out.update({k: v.to(sums.device) for k, v in local_thickness_columns(table, int(ids.numel())).items()})
    if contacts is not None:
        table = instance_contacts(x, contacts, False, rows)[1]
        table = torch.cat((ids[table[:, :2] - 1], table[:, 2:]), 1)      # rows 1..N -> ids; no background rows here
        out["contact_table"] = table
        out.update({k: v.to(sums.device) for k, v in contact_columns(table, ids, out["face_area"], spacing).items()})
    if image is not None:
        _, moments, extrema, hist, shift = instance_intensity(x, image, rows)
        out.update(intensity_moments=moments, intensity_extrema=extrema, intensity_hist=hist, intensity_shift=shift)
        out.update({k: v.to(sums.device) for k, v in intensity_columns(moments, extrema, hist, shift, spacing).items()})
        if intensity_ring is not None:
            ring = _intensity_ring(x, image, intensity_ring, spacing, rows)[0]
            out["ring_moments"] = ring
            out.update({k: v.to(sums.device) for k, v in ring_columns(ring, moments).items()})
    if cores is not None:
        from ..utils.split import core_pieces
        core_table = core_pieces(rows[0], cores, spacing, thickness == "closed", rows)[1]
        out.update({k: v.to(sums.device) for k, v in cores_columns(core_table, ids).items()})
    if parents is not None:
        from ..utils.relate import relate
        child_table = relate(rows[0], parents, parent_min_fraction, spacing, rows_children=rows)[0]
        out.update(parent=child_table["parent_id"], inside_fraction=child_table["inside_fraction"])
    if near is not None:
        from ..utils.proximity import proximity
        table = proximity(rows[0], None if isinstance(near, str) else near, near_distance, spacing, rows_a=rows,
                          voxels_a=sums[:, 0])[1]
        out.update(near_partners=table["partners"], nearest_id=table["nearest_id"], nearest_gap=table["nearest_gap"],
                   near_voxels=table["near_voxels"], near_fraction=table["near_fraction"])
    return out


def compare(ground_truth: Tensor, predictions: Tensor, anisotropy=(1.0, 1.0, 1.0), iou_threshold: float = 0.1,
            tolerance: Optional[float] = None, sparse: bool = False) -> Dict[str, Tensor]:
    """For each ground-truth instance, which predicted instance it is and how far apart their boundaries are
    (the reference's function of this name raises ``NotImplementedError``).  Both masks are device
    tensors of one shape, (X, Y, Z) or (1, X, Y, Z), of any integer dtype; ``anisotropy`` is the voxel spacing along x,
    y and z.

    Matching (``lib.match_instances``): a ground-truth instance takes the prediction with the largest ``mask_iou`` if
    that is > ``iou_threshold``, the lowest id on a tie.  Several ground-truth instances may take one prediction.

    Returns device tensors with one row per ground-truth id, ascending: ``gt_id``, ``pred_id`` (0: unmatched), int64;
    ``intersection_voxels``, ``gt_voxels``, ``pred_voxels`` int64 (0 where unmatched) and ``iou``, ``dice`` float64
    recomputed from them; ``volume_difference`` float64, (pred - gt voxels) times the voxel volume, and
    ``centroid_distance`` float64, both ``nan`` where unmatched; ``gt_surface_voxels``, ``pred_surface_voxels`` int64,
    the instances' surface voxels (``lib.instance_surfaces``); ``hausdorff``, ``hausdorff95``, ``assd``, ``nsd``
    float64 (``lib.pair_summaries``; ``nan`` where unmatched), the surface distances between voxel centres at the
    spacing, ``nsd`` at ``tolerance`` (default: the largest spacing component); ``pred_shared`` int64, how many
    ground-truth rows chose this row's ``pred_id`` (0 where unmatched; 2 or more is an under-segmentation).  The
    predictions nobody chose follow as ``unmatched_pred_id``, ``unmatched_pred_best_iou`` (float64, the largest value
    of their ``mask_iou`` column), ``unmatched_pred_voxels`` and ``unmatched_pred_surface_voxels``.

    Every integer is exact and every float is a function of exact integers or of the exact squared distances in a
    fixed order: two runs give the same bits.

    Memory: beside the two masks as int32 the call holds two int32 row volumes, and while it counts the intersections
    one more int32 volume and three bool ones -- about 15 bytes per voxel on top of the masks (``mask_iou`` adds its own
    int32 copies while it runs), and ``mask_iou``'s (N + 1) x (M + 1) table, the (N, M) matrix and the (N, M) int64
    temporaries of the matching.

    ``sparse=True`` takes the IoU values, the match, ``intersection_voxels`` and ``unmatched_pred_best_iou`` from one
    ``lib.instance_overlaps`` pass over the two masks instead: nothing of size N x M and none of the
    volume-sized temporaries above exist, and the returned dict is the same, bit for bit."""
    from .lib import (instance_overlaps, instance_surfaces, mask_iou, match_instances, match_instances_sparse,
                      overlap_ious, pair_summaries, surface_distances)
    spacing = _spacing(anisotropy)
    tau = max(spacing) if tolerance is None else float(tolerance)
    if not (tau >= 0.0 and math.isfinite(tau)):
        raise ValueError(f"tolerance must be a finite number >= 0, got {tolerance}")
    g, grows = id_rows(ground_truth)
    p, prows = id_rows(predictions)
    if tuple(g.shape) != tuple(p.shape) or g.device != p.device:
        raise ValueError(f"ground_truth {tuple(g.shape)} on {g.device} and predictions {tuple(p.shape)} on {p.device} "
                         "must have one shape and one device")
    shape, dev = tuple(int(v) for v in g.shape), g.device
    ids_g, sums_g, boxes_g = instance_sums(g, (g, grows))
    ids_p, sums_p, boxes_p = instance_sums(p, (p, prows))
    N, M = int(ids_g.numel()), int(ids_p.numel())
    cen_g = derive(sums_g.cpu(), boxes_g.cpu(), shape, spacing)["centroid"].numpy()
    cen_p = derive(sums_p.cpu(), boxes_p.cpu(), shape, spacing)["centroid"].numpy()
    if sparse:
        pairs, values = overlap_ious(instance_overlaps(g, p, True, (g, grows), (p, prows))[2], N, M)
        match = match_instances_sparse(pairs, values, N, M, iou_threshold)
    else:
        if N and M:
            # every voxel's row, 1..N / 1..M and 0 for the rest; int32 indices and results: no 8-byte-per-voxel temporary
            rg, rp = _Rows(g, (g, grows)).row_volume(), _Rows(p, (p, prows)).row_volume()
            iou = mask_iou(rg, rp)                                      # rows ascend with the ids: the same matrix
        else:
            iou = torch.zeros((N, M), dtype=torch.float32, device=dev)
        match = match_instances(iou, iou_threshold)
    matched = match >= 0
    col = match.clamp(min=0)
    rows_m = torch.nonzero(matched)[:, 0]
    cols_m = match[rows_m]
    K = int(rows_m.numel())
    zeros = torch.zeros(N, dtype=torch.int64, device=dev)
    inter = zeros.clone()
    if K and sparse:                                         # the table is sorted by (ra, rb): one search per matched row
        keys = pairs[:, 0] * (M + 1) + pairs[:, 1]
        want = (rows_m + 1) * (M + 1) + cols_m + 1
        at = torch.searchsorted(keys, want).clamp(max=max(int(keys.numel()) - 1, 0))
        if keys.numel():                                     # a match at IoU 0 (a negative threshold) shares nothing
            inter[rows_m] = torch.where(keys[at] == want, pairs[at, 2], inter.new_zeros(1))
    elif K:
        chose = torch.cat((match.new_zeros(1), match + 1)).to(torch.int32)     # row of gt -> the row of pred it chose, or 0
        want = chose[rg]
        inter = torch.bincount(rg[(want > 0) & (rp == want)].long(), minlength=N + 1)[1:]
        del want
    gv = sums_g[:, 0]
    pv = torch.where(matched, sums_p[col, 0], zeros) if M else zeros.clone()
    sg, sp = instance_surfaces(g, (g, grows)), instance_surfaces(p, (p, prows))
    ns_g, ns_p = sg[1].diff(), sp[1].diff()
    nan = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    out = {"gt_id": ids_g, "pred_id": torch.where(matched, ids_p[col], zeros) if M else zeros.clone(),
           "iou": inter.double() / (gv + pv - inter).double(), "dice": (2 * inter).double() / (gv + pv).double(),
           "intersection_voxels": inter, "gt_voxels": gv, "pred_voxels": pv,
           "volume_difference": nan.clone(), "centroid_distance": nan.clone(),
           "gt_surface_voxels": ns_g, "pred_surface_voxels": torch.where(matched, ns_p[col], zeros) if M else zeros.clone(),
           "hausdorff": nan.clone(), "hausdorff95": nan.clone(), "assd": nan.clone(), "nsd": nan.clone()}
    chosen = torch.bincount(cols_m, minlength=M)
    out["pred_shared"] = torch.where(matched, chosen[col], zeros) if M else zeros.clone()
    if K:
        sx, sy, sz = spacing
        out["volume_difference"][rows_m] = (pv - gv)[rows_m].double() * (sx * sy * sz)
        r, c = rows_m.cpu().numpy(), cols_m.cpu().numpy()
        d = cen_p[c] - cen_g[r]
        out["centroid_distance"][rows_m] = torch.from_numpy(np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] +
                                                                                       d[:, 2] * d[:, 2]))).to(dev)
        off_g, d2_g = surface_distances(sg, sp, torch.stack((rows_m, cols_m), 1), shape, spacing)
        off_p, d2_p = surface_distances(sp, sg, torch.stack((cols_m, rows_m), 1), shape, spacing)
        s = pair_summaries(torch.cat((off_g, off_g[-1] + off_p[1:])), torch.cat((d2_g, d2_p)), K, tau * tau)
        for k in ("hausdorff", "hausdorff95", "assd", "nsd"):
            out[k][rows_m] = s[k].to(dev)
    un = torch.nonzero(chosen == 0)[:, 0]
    out["unmatched_pred_id"] = ids_p[un]
    if sparse:                                               # a column's largest value; 0 where it shares nothing
        best = torch.zeros(M, dtype=torch.float32, device=dev).scatter_reduce_(0, pairs[:, 1] - 1, values, "amax")
        out["unmatched_pred_best_iou"] = best[un].double()
    else:
        out["unmatched_pred_best_iou"] = (iou.max(dim=0)[0][un] if N else iou.new_zeros(int(un.numel()))).double()
    out["unmatched_pred_voxels"] = sums_p[un, 0]
    out["unmatched_pred_surface_voxels"] = ns_p[un]
    return out


COMPARE_COLUMNS = ("gt_id,pred_id,iou,dice,intersection_voxels,gt_voxels,pred_voxels,volume_difference,"
                   "centroid_distance,gt_surface_voxels,pred_surface_voxels,hausdorff,hausdorff95,assd,nsd,pred_shared")


def format_compare_csv(mask_path: str, ground_truth_path: str, result: Dict[str, Tensor], spacing=(1.0, 1.0, 1.0),
                       iou_threshold: float = 0.1, tolerance: Optional[float] = None) -> str:
    """The text of ``_compare.csv`` from the dict of ``compare``: two header lines (the files; spacing, threshold and
    tolerance), the column names, one row per ground-truth instance and then one per prediction nobody chose, with
    ``gt_id`` 0, its best IoU under ``iou`` and ``nan`` in the columns that need a pair.  Floats are printed with
    ``repr``; ``nan`` prints as ``nan``.  A pure function of its arguments."""
    spacing = _spacing(spacing)
    tau = max(spacing) if tolerance is None else float(tolerance)
    names = COMPARE_COLUMNS.split(",")
    d = {k: v.cpu().tolist() for k, v in result.items()}
    lines = [f"Mask File: {mask_path} Ground Truth File: {ground_truth_path}\n",
             "Spacing: {} {} {} IoU Threshold: {} Tolerance: {}\n".format(*(repr(float(v)) for v in
                                                                           (*spacing, iou_threshold, tau))),
             COMPARE_COLUMNS + "\n"]
    for i in range(len(d["gt_id"])):
        lines.append(",".join(repr(d[k][i]) for k in names) + "\n")
    nan = float("nan")
    for i, u in enumerate(d["unmatched_pred_id"]):
        row = {"gt_id": 0, "pred_id": u, "iou": d["unmatched_pred_best_iou"][i], "dice": nan, "intersection_voxels": 0,
               "gt_voxels": 0, "pred_voxels": d["unmatched_pred_voxels"][i], "volume_difference": nan,
               "centroid_distance": nan, "gt_surface_voxels": 0,
               "pred_surface_voxels": d["unmatched_pred_surface_voxels"][i], "hausdorff": nan, "hausdorff95": nan,
               "assd": nan, "nsd": nan, "pred_shared": 0}
        lines.append(",".join(repr(row[k]) for k in names) + "\n")
    return "".join(lines)


def format_csv(mask_path: str, ids, sums: Tensor, boxes: Tensor, shape, spacing=(1.0, 1.0, 1.0),
               min_voxels: int = 1, mesh_cells: Optional[Tensor] = None,
               skeleton_graph: Optional[Tensor] = None, max_dist2: Optional[Tensor] = None,
               skeleton_radius: Optional[Tensor] = None, mesh_counts: Optional[Tensor] = None,
               mesh_closed: bool = False, piece_table: Optional[Tensor] = None, thickness_table=None,
               contact_table=None, intensity=None, ring=None, branch_tables=None, core_table=None,
               parent_table=None, near_table=None) -> str:
    """The text of ``_instance_stats.csv``: two header lines (file, spacing), the column names, and one row per
    instance with at least ``min_voxels`` voxels; floats are printed with ``repr``.  With ``mesh_cells`` (the (N, 30)
    counts of ``instance_mesh_cells``) the columns ``surface_area,surface_to_volume`` follow; without, the text is what
    it was before they existed.  With ``skeleton_graph`` (the (N, 12) rows of ``instance_skeleton_graph``) the columns
    ``skeleton_voxels,skeleton_length,skeleton_endpoints,skeleton_junctions,skeleton_branches`` follow those; without,
    again, nothing changes.  With ``max_dist2`` (the (N) maxima of ``instance_thickness``) ``inscribed_radius`` follows,
    and with ``skeleton_radius`` (its (N, 3) skeleton statistics) ``skeleton_radius_mean,skeleton_radius_min,
    skeleton_radius_max``, in that order behind everything else; an instance alone in the volume in open mode prints
    ``inf``.  With ``mesh_counts`` (the (N, 2) counts of ``instance_mesh_counts``) ``mesh_vertices,mesh_triangles``
    follow behind all of those, and ``euler_characteristic`` behind them when ``mesh_closed`` says the counts are those
    of closed mode.  With ``piece_table`` (the (P, 6) table of ``label_components``) ``pieces,largest_piece_voxels``
    follow behind everything else; without it the text is byte for byte what it was before they existed.  With
    ``thickness_table`` (the (K, 3) table of ``instance_local_thickness``) ``local_radius_mean,local_radius_std,
    local_radius_min`` follow behind all of that, under the same rule.  With ``contact_table`` (the (P, 9) table of
    ``stats_per_instance(contacts=...)``, ids in its first two columns) ``neighbours,contact_area,contact_fraction,
    largest_contact_id,largest_contact_area`` follow behind those, under the same rule again.  With ``intensity`` (the
    ``(moments, extrema, hist, shift)`` of ``instance_intensity``) ``intensity_mean,intensity_std,intensity_min,
    intensity_max,intensity_median,intensity_p05,intensity_p95,wcx,wcy,wcz`` follow, and with ``ring`` (the (N, 6) moments
    of ``intensity_ring``; it needs ``intensity``) ``ring_voxels,ring_mean,ring_std,contrast`` last, under the same rule
    once more: floats with ``repr`` (``nan`` prints as ``nan``), integers as integers.  With ``branch_tables`` (the
    ``(nodes, branches)`` of ``instance_skeleton_branches``) the columns of ``branch_columns`` come last of all:
    ``graph_components,graph_endpoints,graph_junctions,graph_branches,graph_rings,graph_corner_loops,graph_cycles,
    graph_length,branch_length_mean,longest_branch``.  With ``core_table`` (the (P, 6) table of
    ``utils.split.core_pieces``) ``cores`` comes behind even those; without it the text is byte for byte what it was.
    With ``parent_table`` (the ``(parent_id, inside_fraction)`` of ``utils.relate.relate``, N values each)
    ``parent,inside_fraction`` are the last columns, under the same rule.  With ``near_table`` (the per-instance table of
    ``utils.proximity.proximity``) ``near_partners,nearest_id,nearest_gap,near_voxels,near_fraction`` follow them."""
    if ring is not None and intensity is None:
        raise ValueError("ring comes with intensity: the contrast needs both")
    spacing = _spacing(spacing)
    d = derive(sums.cpu(), boxes.cpu(), shape, spacing)
    if mesh_cells is not None:
        d.update(surface_columns(mesh_cells, d["volume"], spacing))
    if skeleton_graph is not None:
        d.update(skeleton_columns(skeleton_graph, spacing))
    if skeleton_radius is not None and max_dist2 is None:
        raise ValueError("skeleton_radius comes with max_dist2: both are results of instance_thickness")
    if max_dist2 is not None:
        d.update(thickness_columns(max_dist2, skeleton_radius))
    mesh_names = []
    if mesh_counts is not None:
        d.update(mesh_columns(mesh_counts, bool(mesh_closed)))
        mesh_names = (MESH_COLUMNS + ("," + MESH_CLOSED_COLUMNS if mesh_closed else "")).split(",")
    if piece_table is not None:
        d.update(pieces_columns(piece_table, ids))
    ids = ids.cpu().tolist() if isinstance(ids, Tensor) else list(ids)
    if thickness_table is not None:
        d.update(local_thickness_columns(thickness_table, len(ids)))
    if contact_table is not None:
        d.update(contact_columns(contact_table, ids, d["face_area"], spacing))
    if intensity is not None:
        d.update(intensity_columns(*intensity, spacing))
    if ring is not None:
        d.update(ring_columns(ring, intensity[0]))
    if branch_tables is not None:
        d.update(branch_columns(*branch_tables, len(ids), spacing))
    if core_table is not None:
        d.update(cores_columns(core_table, ids))
    if parent_table is not None:
        d.update(parent=torch.as_tensor(parent_table[0]).to(torch.int64).reshape(-1),
                 inside_fraction=torch.as_tensor(parent_table[1]).to(torch.float64).reshape(-1))
        if d["parent"].numel() != len(ids) or d["inside_fraction"].numel() != len(ids):
            raise ValueError(f"parent_table has {d['parent'].numel()} and {d['inside_fraction'].numel()} values for "
                             f"{len(ids)} ids")
    if near_table is not None:
        near_keys = ("partners", "nearest_id", "nearest_gap", "near_voxels", "near_fraction")
        d.update({n: torch.as_tensor(near_table[k]).reshape(-1) for n, k in zip(NEAR_COLUMNS.split(","), near_keys)})
        if any(d[n].numel() != len(ids) for n in NEAR_COLUMNS.split(",")):
            raise ValueError(f"near_table does not have one row for each of the {len(ids)} ids")
    d = {k: v.cpu().tolist() for k, v in d.items()}
    lines = [f"Mask File: {mask_path}\n", "Spacing: {} {} {}\n".format(*(repr(v) for v in spacing)),
             CSV_COLUMNS + ("," + SURFACE_COLUMNS if mesh_cells is not None else "") +
             ("," + SKELETON_COLUMNS if skeleton_graph is not None else "") +
             ("," + THICKNESS_COLUMNS if max_dist2 is not None else "") +
             ("," + SKELETON_RADIUS_COLUMNS if skeleton_radius is not None else "") +
             "".join("," + k for k in mesh_names) + ("," + PIECES_COLUMNS if piece_table is not None else "") +
             ("," + LOCAL_THICKNESS_COLUMNS if thickness_table is not None else "") +
             ("," + CONTACT_COLUMNS if contact_table is not None else "") +
             ("," + INTENSITY_COLUMNS if intensity is not None else "") +
             ("," + RING_COLUMNS if ring is not None else "") +
             ("," + BRANCH_COLUMNS if branch_tables is not None else "") +
             ("," + CORES_COLUMNS if core_table is not None else "") +
             ("," + PARENT_COLUMNS if parent_table is not None else "") +
             ("," + NEAR_COLUMNS if near_table is not None else "") + "\n"]
    for i, u in enumerate(ids):
        if d["voxels"][i] < min_voxels:
            continue
        cells = [int(u), d["voxels"][i], repr(d["volume"][i]), *d["bbox"][i], int(d["touches_border"][i]),
                 *(repr(v) for v in d["centroid"][i]), repr(d["face_area"][i]),
                 *(repr(v) for v in d["axis_lengths"][i])]
        if mesh_cells is not None:
            cells += [repr(d["surface_area"][i]), repr(d["surface_to_volume"][i])]
        if skeleton_graph is not None:
            cells += [d["skeleton_voxels"][i], repr(d["skeleton_length"][i]), d["skeleton_endpoints"][i],
                      d["skeleton_junctions"][i], d["skeleton_branches"][i]]
        if max_dist2 is not None:
            cells += [repr(d["inscribed_radius"][i])]
        if skeleton_radius is not None:
            cells += [repr(d[k][i]) for k in SKELETON_RADIUS_COLUMNS.split(",")]
        cells += [d[k][i] for k in mesh_names]
        if piece_table is not None:
            cells += [d[k][i] for k in PIECES_COLUMNS.split(",")]
        if thickness_table is not None:
            cells += [repr(d[k][i]) for k in LOCAL_THICKNESS_COLUMNS.split(",")]
        if contact_table is not None:
            cells += [d["neighbours"][i], repr(d["contact_area"][i]), repr(d["contact_fraction"][i]),
                      d["largest_contact_id"][i], repr(d["largest_contact_area"][i])]
        if intensity is not None:
            cells += [repr(d["intensity_mean"][i]), repr(d["intensity_std"][i]),
                      *(d[k][i] for k in INTENSITY_COLUMNS.split(",")[2:7]), *(repr(v) for v in d["weighted_centroid"][i])]
        if ring is not None:
            cells += [d["ring_voxels"][i], repr(d["ring_mean"][i]), repr(d["ring_std"][i]), repr(d["contrast"][i])]
        if branch_tables is not None:
            names = BRANCH_COLUMNS.split(",")
            cells += [d[k][i] for k in names[:7]] + [repr(d[k][i]) for k in names[7:]]
        if core_table is not None:
            cells += [d["cores"][i]]
        if parent_table is not None:
            cells += [d["parent"][i], repr(d["inside_fraction"][i])]
        if near_table is not None:
            cells += [d["near_partners"][i], d["nearest_id"][i], repr(d["nearest_gap"][i]), d["near_voxels"][i],
                      repr(d["near_fraction"][i])]
        lines.append(",".join(str(c) for c in cells) + "\n")
    return "".join(lines)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m skoots_amd.validate.compare",
                                     description="SKOOTS: volume, box, centroid, face area and axes of every instance, "
                                                 "and the mesh surface area, the skeleton and the width on request")
    parser.add_argument("mask", type=str, help="Path to an instance mask (.tif or .npy, stored [Z, X, Y])")
    parser.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"),
                        help="Voxel spacing along x, y and z")
    parser.add_argument("--min-voxels", type=int, default=1, help="Leave out instances with fewer voxels")
    parser.add_argument("--surface-area", type=str, default=None, choices=("open", "closed"),
                        help="Append surface_area,surface_to_volume: the marching-cubes mesh area of every instance, "
                             "left open where the volume's faces cut it (the reference's meaning) or closed there")
    parser.add_argument("--skeleton", action="store_true",
                        help="Append " + SKELETON_COLUMNS + ": every instance thinned to its centre line (Lee), the "
                             "length of its links at the spacing, its endpoints, junction voxels and branches")
    parser.add_argument("--save-skeletons", action="store_true",
                        help="Also write <mask>_skeletons.tif, every skeleton voxel carrying its instance id, stored "
                             "[Z, X, Y] like the mask (implies --skeleton)")
    parser.add_argument("--branches", action="store_true",
                        help="Append " + BRANCH_COLUMNS + ": every skeleton traced into nodes and branches; also write "
                             "<mask>_branches.csv, one row per branch (" + BRANCH_CSV_COLUMNS + "; with --thickness also " +
                             BRANCH_RADIUS_COLUMNS + " along the branch) and <mask>_nodes.csv, one row per node (" +
                             NODE_CSV_COLUMNS + ") (implies --skeleton)")
    parser.add_argument("--skeleton-from", type=str, default=None, metavar="PATH",
                        help="With --branches: trace the skeletons of PATH, a stack that --save-skeletons wrote for this "
                             "mask, instead of thinning the instances again")
    parser.add_argument("--thickness", type=str, default=None, choices=("open", "closed"),
                        help="Append " + THICKNESS_COLUMNS + ": the largest distance from a voxel of the instance to the "
                             "nearest voxel outside it, from an exact Euclidean distance transform at the spacing, "
                             "counting the voxels of the volume only (open: an instance alone in the volume has inf) or "
                             "the volume padded with background (closed); with --skeleton also " +
                             SKELETON_RADIUS_COLUMNS + ", the radius along the centre line")
    parser.add_argument("--save-distance", action="store_true",
                        help="Also write <mask>_distance.tif, float32, every instance voxel its distance to the nearest "
                             "voxel outside its instance and background 0, stored [Z, X, Y] like the mask (implies "
                             "--thickness open when no mode is given)")
    parser.add_argument("--local-thickness", type=str, default=None, choices=("open", "closed"),
                        help="Append " + LOCAL_THICKNESS_COLUMNS + ": for every voxel the radius of the largest ball "
                             "inside its instance that holds it (the local thickness, as a radius between voxel "
                             "centres), and per instance its mean, standard deviation and smallest value, the thinnest "
                             "place; open and closed as for --thickness.  Every voxel paints its ball: a compact object "
                             "many tens of voxels across takes long")
    parser.add_argument("--save-thickness", action="store_true",
                        help="Also write <mask>_thickness.tif, float32, every instance voxel its local radius and "
                             "background 0, stored [Z, X, Y] like the mask (implies --local-thickness open when no mode "
                             "is given)")
    parser.add_argument("--mesh", type=str, default=None, choices=("open", "closed"),
                        help="Append " + MESH_COLUMNS + ": the size of every instance's marching-cubes mesh, left open "
                             "where the volume's faces cut it or closed there; closed also appends " +
                             MESH_CLOSED_COLUMNS + " = vertices - triangles / 2")
    parser.add_argument("--save-meshes", action="store_true",
                        help="Also write <mask>_meshes.ply: the meshes of the instances the CSV file lists (--min-voxels "
                             "applies), one binary PLY, coordinates in physical units x, y, z, the instance id as a "
                             "property of vertices and faces, normals pointing out (implies --mesh closed when no mode is "
                             "given)")
    parser.add_argument("--mesh-ids", type=int, nargs="+", default=None, metavar="ID",
                        help="With --save-meshes: write only these instances")
    parser.add_argument("--pieces", type=int, default=None, choices=(6, 18, 26),
                        help="Append " + PIECES_COLUMNS + ": the connected pieces of every id at this connectivity and "
                             "the voxels of the largest (an id in several pieces is not one body)")
    parser.add_argument("--cores", type=float, default=None, metavar="R",
                        help="Append " + CORES_COLUMNS + ": the 6-connected pieces that remain of every id at depth R (in "
                             "the units of --spacing; closed depth with --thickness closed): an id with two or more is "
                             "what python -m skoots_amd.utils.split --radius R cuts")
    parser.add_argument("--contacts", type=int, default=None, choices=(6, 18, 26),
                        help="Append " + CONTACT_COLUMNS + ": the instances every id touches at this connectivity and the "
                             "area of the voxel faces it shares with them; also write <mask>_contacts.csv, one row per "
                             "touching pair: " + CONTACT_CSV_COLUMNS)
    parser.add_argument("--image", type=str, default=None, metavar="I",
                        help="Append " + INTENSITY_COLUMNS + ": the image under every instance, from I (.tif or .npy, 8- "
                             "or 16-bit, stored [Z, X, Y] like the mask): mean, population standard deviation, extrema, "
                             "nearest-rank quantiles from a 256-bin histogram (the lower edge of the bin when a 16-bit "
                             "image needs bins wider than 1) and the intensity-weighted centroid")
    parser.add_argument("--intensity-ring", type=float, default=None, metavar="D",
                        help="With --image: append " + RING_COLUMNS + ": the image over the background within D (in the "
                             "units of --spacing) that is nearer to this instance than to any other, and the contrast "
                             "(intensity_mean - ring_mean) / (intensity_mean + ring_mean)")
    parser.add_argument("--save-histograms", action="store_true",
                        help="With --image: also write <mask>_histograms.csv, the 256 histogram counts of every instance")
    parser.add_argument("--ground-truth", type=str, default=None, metavar="GT",
                        help="Also write <mask>_compare.csv: the mask is a prediction and GT (.tif or .npy of the same "
                             "shape) the ground truth; one row per ground-truth instance with the predicted instance it "
                             "matches (largest IoU above --iou-threshold), their overlap and the distances between their "
                             "surfaces: " + COMPARE_COLUMNS + "; then one row per predicted instance nobody chose")
    parser.add_argument("--iou-threshold", type=float, default=None, metavar="T",
                        help="With --ground-truth: a match needs an IoU above T (default 0.1)")
    parser.add_argument("--tolerance", type=float, default=None, metavar="TAU",
                        help="With --ground-truth: nsd counts the surface voxels within TAU of the other surface "
                             "(default: the largest spacing component)")
    parser.add_argument("--sparse-matching", action="store_true",
                        help="With --ground-truth: match on the sparse table of overlapping pairs instead of the dense "
                             "N x M IoU matrix: the same file, byte for byte, in memory that does not grow with N x M")
    parser.add_argument("--parents", type=str, default=None, metavar="P",
                        help="Append " + PARENT_COLUMNS + ": P (.tif or .npy of the same shape) is a mask of other, larger "
                             "objects, such as the cells around mitochondria; the id of P that holds most of the "
                             "instance's voxels (0: none) and the share of the instance inside it, as python -m "
                             "skoots_amd.utils.relate decides")
    parser.add_argument("--parent-min-fraction", type=float, default=None, metavar="F",
                        help="With --parents: an instance with less than this share of its voxels inside its parent gets "
                             "parent 0 (default 0)")
    parser.add_argument("--near", type=str, default=None, metavar="B|self",
                        help="Append " + NEAR_COLUMNS + ": B (.tif or .npy of the same shape) is a second mask, 'self' "
                             "the mask itself; the instances of it within --near-distance of every instance, the "
                             "closest of them and the gap to it, and the instance's voxels that lie that close, as "
                             "python -m skoots_amd.utils.proximity derives them")
    parser.add_argument("--near-distance", type=float, default=None, metavar="D",
                        help="With --near: the distance, in the units of --spacing")
    parser.add_argument("--out", type=str, default=None, help="Output file (default: <mask>_instance_stats.csv)")
    parser.add_argument("--log", type=int, default=3, choices=range(5),
                        help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    args = parser.parse_args(argv)
    args.skeleton = args.skeleton or args.save_skeletons or args.branches
    if args.skeleton_from is not None and not args.branches:
        parser.error("--skeleton-from names the skeletons that --branches traces")
    if args.save_distance and args.thickness is None:
        args.thickness = "open"
    if args.save_thickness and args.local_thickness is None:
        args.local_thickness = "open"
    if args.save_meshes and args.mesh is None:
        args.mesh = "closed"
    if args.mesh_ids is not None and not args.save_meshes:
        parser.error("--mesh-ids selects the instances of --save-meshes")
    if args.ground_truth is None and (args.iou_threshold is not None or args.tolerance is not None):
        parser.error("--iou-threshold and --tolerance belong to --ground-truth")
    if args.ground_truth is None and args.sparse_matching:
        parser.error("--sparse-matching belongs to --ground-truth")
    if args.parents is None and args.parent_min_fraction is not None:
        parser.error("--parent-min-fraction belongs to --parents")
    if args.parent_min_fraction is None:
        args.parent_min_fraction = 0.0
    if not 0.0 <= args.parent_min_fraction <= 1.0:
        parser.error("--parent-min-fraction takes a share in [0, 1]")
    if (args.near is None) != (args.near_distance is None):
        parser.error("--near and --near-distance come together")
    if args.near_distance is not None and not (0.0 <= args.near_distance < float("inf")):
        parser.error("--near-distance takes a non-negative finite distance")
    if args.iou_threshold is None:
        args.iou_threshold = 0.1
    if args.image is None and (args.intensity_ring is not None or args.save_histograms):
        parser.error("--intensity-ring and --save-histograms belong to --image")
    if args.cores is not None and not (0.0 <= args.cores < float("inf")):
        parser.error("--cores takes a non-negative finite radius")
    if args.intensity_ring is not None and not (0.0 < args.intensity_ring < float("inf")):
        parser.error("--intensity-ring takes a positive finite distance")
    return args


def load_image(path: str, mask_path: str, mask_shape) -> Tensor:
    """(X, Y, Z) uint8 or uint16 host tensor from a .tif or .npy stored [Z, X, Y] like the mask, its dtype kept; any
    other dtype, or a shape that is not the mask's (X, Y, Z), is an error that names both files."""
    from ..lib.tiff import read_image
    image = read_image(path)
    want = tuple(int(v) for v in mask_shape[-3:])
    if image.dtype not in (np.uint8, np.uint16) or image.ndim != 3 or (image.shape[1], image.shape[2],
                                                                         image.shape[0]) != want:
        raise ValueError(f"{path} holds {image.dtype} samples of shape {tuple(image.shape)} [Z, X, Y(, C)] and {mask_path} "
                         f"has (X, Y, Z) = {want}: --image takes one 8- or 16-bit sample per voxel of the mask")
    return torch.from_numpy(np.ascontiguousarray(image.transpose(1, 2, 0)))


def main(argv: Optional[Sequence[str]] = None) -> str:
    """Runs the command; returns the path of the CSV file.  The whole mask is measured: there is no border crop."""
    args = parse_args(argv)
    logging.basicConfig(level=_LOG_LEVELS[args.log],
                        format="[%(asctime)s] skoots-instance-stats [%(levelname)s]: %(message)s")
    if not os.path.exists(args.mask):
        raise RuntimeError(f"{args.mask} does not exist")
    spacing = _spacing(args.spacing)
    from .__main__ import load_mask
    mask = load_mask(args.mask)
    logging.debug(f"Mask Shape: {tuple(mask.shape)}")
    check_shape(mask.shape[-3:])
    dev_mask = mask.to("cuda")                              # the HIP library: no CPU fallback
    rows = id_rows(dev_mask)                                # once, for both kernels
    ids, sums, boxes = instance_sums(dev_mask, rows)
    cells = instance_mesh_cells(dev_mask, args.surface_area == "closed", rows)[1] if args.surface_area else None
    graph = branch_tables = None
    if args.branches:
        from .__main__ import load_mask as load_stack
        saved = None
        if args.skeleton_from is not None:
            if not os.path.exists(args.skeleton_from):
                raise RuntimeError(f"{args.skeleton_from} does not exist")
            saved = load_stack(args.skeleton_from)
            if tuple(saved.shape) != tuple(mask.shape):
                raise ValueError(f"{args.skeleton_from} has the shape {tuple(saved.shape)} and {args.mask} "
                                 f"{tuple(mask.shape)}: the skeletons of a mask have its shape")
            saved = saved.to("cuda")
        if args.save_skeletons and ids.numel() and int(ids.max().item()) > 2 ** 31 - 1:
            raise ValueError(f"--save-skeletons writes int32 labels and {args.mask} has the id {int(ids.max().item())}, "
                             "which does not fit; renumber the mask, or use --skeleton alone")
        graph, nodes, branch_table, points, owner = instance_skeleton_branches(dev_mask, rows, boxes, skeleton=saved)[1:]
        branch_tables = (nodes, branch_table)
        volume = [points_volume(points, graph, mask.shape[-3:])]
    elif args.skeleton:
        if args.save_skeletons and ids.numel() and int(ids.max().item()) > 2 ** 31 - 1:
            raise ValueError(f"--save-skeletons writes int32 labels and {args.mask} has the id {int(ids.max().item())}, "
                             "which does not fit; renumber the mask, or use --skeleton alone")
        graph, *volume = instance_skeleton_graph(dev_mask, rows, boxes,
                                                 want_volume=args.save_skeletons or bool(args.thickness))[1:]
    max_d2 = dist2 = skel_radius = None
    if args.thickness:
        max_d2, dist2, *skel = instance_thickness(dev_mask, spacing, args.thickness == "closed", rows,
                                                  volume[0] if args.skeleton else None)[1:]
        skel_radius = skel[0] if skel else None
    mesh_counts = instance_mesh_counts(dev_mask, args.mesh == "closed", rows)[1] if args.mesh else None
    piece_table = None
    if args.pieces:
        from ..lib.morphology import label_components
        piece_table = label_components(dev_mask, args.pieces, rows=rows)[1]
    thickness_table = thick2 = None
    if args.local_thickness:
        have = (dist2, max_d2) if args.thickness == args.local_thickness else None
        thickness_table, thick2 = instance_local_thickness(dev_mask, spacing, args.local_thickness == "closed", rows,
                                                           have)[1:3]
    contact_table = None
    if args.contacts:
        contact_table = instance_contacts(dev_mask, args.contacts, False, rows)[1]
        contact_table = torch.cat((ids[contact_table[:, :2] - 1], contact_table[:, 2:]), 1)      # rows 1..N -> ids
    intensity = ring = None
    if args.image:
        if not os.path.exists(args.image):
            raise RuntimeError(f"{args.image} does not exist")
        dev_image = load_image(args.image, args.mask, mask.shape).to("cuda")
        intensity = instance_intensity(dev_mask, dev_image, rows)[1:]
        if args.intensity_ring is not None:
            ring = _intensity_ring(dev_mask, dev_image, args.intensity_ring, spacing, rows)[0]
    core_table = None
    if args.cores is not None:
        from ..utils.split import core_pieces
        core_table = core_pieces(rows[0], args.cores, spacing, args.thickness == "closed", rows)[1]
    parent_table = None
    if args.parents is not None:
        if not os.path.exists(args.parents):
            raise RuntimeError(f"{args.parents} does not exist")
        from ..utils.relate import relate
        parent_mask = load_mask(args.parents)
        if tuple(parent_mask.shape) != tuple(mask.shape):
            raise ValueError(f"{args.parents} has the shape {tuple(parent_mask.shape)} and {args.mask} "
                             f"{tuple(mask.shape)}: the parents of a mask have its shape")
        child_table = relate(rows[0], parent_mask.to("cuda"), args.parent_min_fraction, spacing, rows_children=rows)[0]
        parent_table = (child_table["parent_id"], child_table["inside_fraction"])
    near_table = None
    if args.near is not None:
        from ..utils.proximity import proximity
        near_mask = None
        if args.near != "self":
            if not os.path.exists(args.near):
                raise RuntimeError(f"{args.near} does not exist")
            near_mask = load_mask(args.near)
            if tuple(near_mask.shape) != tuple(mask.shape):
                raise ValueError(f"{args.near} has the shape {tuple(near_mask.shape)} and {args.mask} "
                                 f"{tuple(mask.shape)}: the mask of --near has the mask's shape")
            near_mask = near_mask.to("cuda")
        near_table = proximity(rows[0], near_mask, args.near_distance, spacing, rows_a=rows, voxels_a=sums[:, 0])[1]
    text = format_csv(args.mask, ids, sums, boxes, tuple(mask.shape[-3:]), spacing, args.min_voxels, cells, graph,
                      max_d2, skel_radius, mesh_counts, args.mesh == "closed", piece_table, thickness_table,
                      contact_table, intensity, ring, branch_tables, core_table, parent_table, near_table)
    out_path = args.out or f"{os.path.splitext(args.mask)[0]}_instance_stats.csv"
    with open(out_path, "w") as file:
        file.write(text)
    print(f"File Written: {out_path}")
    if args.branches:
        keep = (sums[:, 0] >= args.min_voxels).cpu().tolist()
        radius = branch_radii(branch_table, points, owner, dist2) if args.thickness else None
        for suffix, body in (("branches", format_branches_csv(args.mask, ids, nodes, branch_table, spacing, keep, radius)),
                             ("nodes", format_nodes_csv(args.mask, ids, nodes, keep))):
            path = f"{os.path.splitext(args.mask)[0]}_{suffix}.csv"
            with open(path, "w") as file:
                file.write(body)
            print(f"File Written: {path}")
    if args.contacts:
        face_area = derive(sums.cpu(), boxes.cpu(), tuple(mask.shape[-3:]), spacing)["face_area"]
        contacts_path = f"{os.path.splitext(args.mask)[0]}_contacts.csv"
        with open(contacts_path, "w") as file:
            file.write(format_contacts_csv(args.mask, contact_table, ids, face_area, spacing, args.contacts))
        print(f"File Written: {contacts_path}")
    if args.save_histograms:
        hist_path = f"{os.path.splitext(args.mask)[0]}_histograms.csv"
        with open(hist_path, "w") as file:
            file.write(format_histograms_csv(args.mask, ids, intensity[2], intensity[3]))
        print(f"File Written: {hist_path}")
    if args.save_skeletons:
        from ..lib import tiff
        # rows 1 .. N -> ids, 0 stays 0; (X, Y, Z) -> the mask's [Z, X, Y]
        table = torch.cat((ids.new_zeros(1), ids)).to(torch.int32)
        skel_path = f"{os.path.splitext(args.mask)[0]}_skeletons.tif"
        tiff.write_label_stack(skel_path, table[volume[0].long()].permute(2, 0, 1).contiguous())
        print(f"File Written: {skel_path}")
    if args.save_distance:
        from ..lib import tiff
        dist_path = f"{os.path.splitext(args.mask)[0]}_distance.tif"
        # (X, Y, Z) -> the mask's [Z, X, Y]; inf (an instance alone in the volume, open mode) stays inf in float32
        tiff.write_float_stack(dist_path, torch.sqrt(dist2).to(torch.float32).permute(2, 0, 1).contiguous())
        print(f"File Written: {dist_path}")
    if args.save_thickness:
        from ..lib import tiff
        thick_path = f"{os.path.splitext(args.mask)[0]}_thickness.tif"
        # (X, Y, Z) -> the mask's [Z, X, Y]; inf (an instance alone in the volume, open mode) stays inf in float32
        tiff.write_float_stack(thick_path, torch.sqrt(thick2).to(torch.float32).permute(2, 0, 1).contiguous())
        print(f"File Written: {thick_path}")
    if args.save_meshes:
        from ..lib.ply import write_ply
        keep = ids[sums[:, 0] >= args.min_voxels]
        if args.mesh_ids is not None:
            missing = sorted(set(args.mesh_ids) - set(keep.tolist()))
            if missing:
                raise ValueError(f"--mesh-ids {missing}: not among the instances of {args.mask} with at least "
                                 f"{args.min_voxels} voxels")
            keep = torch.tensor(sorted(set(args.mesh_ids)), dtype=torch.int64)
        m = instance_meshes(dev_mask, args.mesh == "closed", rows, ids=keep)
        mesh_path = f"{os.path.splitext(args.mask)[0]}_meshes.ply"
        name = os.path.basename(args.mask).encode("ascii", "replace").decode("ascii")     # a PLY header is ASCII
        write_ply(mesh_path, m["ids"], m["vertices"], m["faces"], m["vertex_offsets"], m["face_offsets"], spacing,
                  comment=f"skoots_amd marching-cubes meshes ({args.mesh}) of {name}")
        print(f"File Written: {mesh_path}")
    if args.ground_truth is not None:
        if not os.path.exists(args.ground_truth):
            raise RuntimeError(f"{args.ground_truth} does not exist")
        truth = load_mask(args.ground_truth)
        if tuple(truth.shape) != tuple(mask.shape):
            raise ValueError(f"{args.ground_truth} has the shape {tuple(truth.shape)} and {args.mask} "
                             f"{tuple(mask.shape)}: a comparison needs one shape")
        result = compare(truth.to("cuda"), dev_mask, spacing, args.iou_threshold, args.tolerance,
                         sparse=args.sparse_matching)
        compare_path = f"{os.path.splitext(args.mask)[0]}_compare.csv"
        with open(compare_path, "w") as file:
            file.write(format_compare_csv(args.mask, args.ground_truth, result, spacing, args.iou_threshold,
                                          args.tolerance))
        print(f"File Written: {compare_path}")
    return out_path


if __name__ == "__main__":
    main()
