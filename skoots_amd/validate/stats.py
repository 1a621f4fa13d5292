"""Measurements of ONE binary mask (reference: skoots/validate/stats.py), on top of the one-pass kernel of
``validate/compare.py``.  For every instance of a mask at once use ``compare.stats_per_instance``.

``get_volume`` has the evident intent of the reference's function of that name, which cannot run
(``torch.sum`` of a Python int raises ``TypeError``, stats.py:24).

``get_surface_area`` is the reference's marching-cubes mesh area (``skimage.measure.marching_cubes`` and
``mesh_surface_area``, stats.py:30-48) without a mesh: one kernel pass counts the mask's cells per triangle class
(DESIGN.md §21).  ``get_face_area`` is the area of the exposed voxel faces, exact for what it defines and an
overestimate of a curved surface.

``get_mesh`` is that mesh itself, vertices and faces, for one binary mask.

``get_skeleton_length`` is the length of the mask's Lee skeleton read as a graph, on the path of
``compare.stats_per_instance(skeleton=True)``.

``get_inscribed_radius`` is the largest value of the mask's exact Euclidean distance transform, on the
path of ``compare.stats_per_instance(thickness=...)``.

``get_local_thickness`` is the mask's local-thickness map, the radius of the largest ball inside the mask that holds the
voxel, on the path of ``compare.stats_per_instance(local_thickness=...)``.

``get_branches`` is the mask's skeleton traced into nodes and branches, on the path of
``compare.stats_per_instance(branches=True)``.

``get_intensity`` is the mean of an image under every instance of a mask, on the path of
``compare.stats_per_instance(image=...)``.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch
from torch import Tensor

from .compare import _spacing, branch_columns, branch_lengths, mesh_area, skeleton_columns, thickness_columns
from .lib import (instance_intensity, instance_local_thickness, instance_mesh_cells, instance_meshes, instance_skeleton_branches,
                  instance_skeleton_graph, instance_sums,
                  instance_thickness)


def _one_row(x: Tensor) -> Tensor:
    """The 13 sums of the non-zero voxels of x as ONE object (zeros when there is none)."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, sums, _ = instance_sums((x != 0).to(torch.int32))
    return sums[0] if sums.shape[0] else torch.zeros(13, dtype=torch.int64, device=x.device)


def get_volume(x: Tensor, spacing: Optional[Union[List[float], Tensor]] = None) -> Tensor:
    """The number of non-zero voxels of the (X, Y, Z) mask ``x`` (int64), times the product of ``spacing`` (float64)
    when one is given -- stats.py:12-27."""
    n = _one_row(x)[0]
    if spacing is None:
        return n
    sx, sy, sz = _spacing(spacing)
    return n.to(torch.float64) * (sx * sy * sz)


def get_face_area(x: Tensor, spacing: Union[List[float], Tensor]) -> Tensor:
    """The area of the exposed faces of the non-zero voxels of the (X, Y, Z) mask ``x`` (float64): a face is exposed
    when the voxel across it is zero or lies outside the volume; one along x has the area ``sy sz``, and so on."""
    sx, sy, sz = _spacing(spacing)
    f = _one_row(x)[10:13].to(torch.float64)
    return f[0] * (sy * sz) + f[1] * (sx * sz) + f[2] * (sx * sy)


def get_surface_area(x: Tensor, anisotropy_ratio: Union[List[float], Tensor], closed: bool = False) -> Tensor:
    """The area of the marching-cubes mesh of ``x > 0`` at the voxel spacing ``anisotropy_ratio`` (float64, on x's
    device) -- stats.py:30-48, which meshes ``x.gt(0).mul(255)`` at level 127.5.  ``closed=False`` is the reference's
    meaning: the mesh stays open where the mask touches a face of the volume; ``closed=True`` pads the mask with one
    layer of background first.

    Deliberate difference: a mask without surface inside the volume (empty, or full in open mode) or with an extent
    below 2 gives 0 where scikit-image raises ("No surface found", "must be at least 2x2x2")."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, cells = instance_mesh_cells((x > 0).to(torch.int32), closed=closed)
    area = mesh_area(cells, anisotropy_ratio)            # checks the spacing, also for a mask without foreground
    return (area[0] if area.numel() else torch.zeros((), dtype=torch.float64)).to(x.device)


def get_mesh(x: Tensor, anisotropy_ratio: Union[List[float], Tensor], closed: bool = False):
    """(verts (V, 3) float64 in physical units, faces (F, 3) int64), on x's device: the marching-cubes mesh of ``x > 0``
    at the voxel spacing ``anisotropy_ratio`` -- the mesh whose area ``get_surface_area`` returns, which the reference
    builds with ``skimage.measure.marching_cubes`` and throws away (stats.py:30-48).  Vertices are welded and in the
    canonical order of ``lib.instance_meshes``; faces keep scikit-image's vertex order.  ``closed`` is
    ``get_surface_area``'s.  A mask without surface gives (0, 3) arrays where scikit-image raises."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    s = torch.tensor(_spacing(anisotropy_ratio), dtype=torch.float64, device=x.device)
    m = instance_meshes((x > 0).to(torch.int32), closed=closed)
    return m["vertices"].to(torch.float64) * s / 2.0, m["faces"].to(torch.int64)


def get_skeleton_length(x: Tensor, spacing: Union[List[float], Tensor]) -> Tensor:
    """The length of the skeleton of ``x > 0`` (one binary object; scikit-image 0.18.3's Lee thinning of the whole
    volume) at the voxel spacing ``spacing`` (float64, on x's device): every pair of 26-neighbouring skeleton voxels
    contributes the distance of their centres -- ``compare.skeleton_columns`` states the bias this has at corners.  A
    mask without foreground, or one that thins to a single voxel, gives 0."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, graph = instance_skeleton_graph((x > 0).to(torch.int32))
    length = skeleton_columns(graph, spacing)["skeleton_length"]      # checks the spacing, also for an empty mask
    return (length[0] if length.numel() else torch.zeros((), dtype=torch.float64)).to(x.device)


def get_branches(x: Tensor, spacing: Union[List[float], Tensor]):
    """The skeleton of ``x > 0`` (one binary object, thinned as in ``get_skeleton_length``) traced into nodes and
    branches: a dict with ``nodes`` (Nn, 8) and ``branches`` (Nb, 18) int32 on x's device (``lib.instance_skeleton_branches``
    names the columns), ``lengths`` (Nb) float64, the length of every branch at the voxel spacing ``spacing``, and the
    columns of ``compare.branch_columns`` as Python numbers: ``graph_components``, ``graph_endpoints``,
    ``graph_junctions``, ``graph_branches``, ``graph_rings``, ``graph_corner_loops``, ``graph_cycles``,
    ``graph_length``, ``branch_length_mean``, ``longest_branch``.  A mask without foreground gives empty tables and
    zeros."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, _, nodes, branches, _, _ = instance_skeleton_branches((x > 0).to(torch.int32))
    out = {k: v[0].item() for k, v in branch_columns(nodes, branches, 1, spacing).items()}
    out.update(nodes=nodes, branches=branches, lengths=branch_lengths(branches, spacing).to(x.device))
    return out


def get_inscribed_radius(x: Tensor, spacing: Union[List[float], Tensor], closed: bool = False) -> Tensor:
    """The radius of the largest sphere around a voxel centre of ``x > 0`` (one binary object) that holds no centre of a
    voxel outside it, at the voxel spacing ``spacing`` (float64, on x's device): the maximum of
    ``scipy.ndimage.distance_transform_edt(x > 0, sampling=spacing)``, computed exactly.  Distances run between voxel
    centres, without a half-voxel correction (``compare.thickness_columns``).  ``closed=False`` counts the voxels of the
    volume only, so a mask that fills it gives ``inf``; ``closed=True`` pads the volume with background.  A mask without
    foreground gives 0."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, max_d2, _ = instance_thickness((x > 0).to(torch.int32), _spacing(spacing), closed)
    radius = thickness_columns(max_d2)["inscribed_radius"]
    return (radius[0] if radius.numel() else torch.zeros((), dtype=torch.float64)).to(x.device)


def get_local_thickness(x: Tensor, spacing: Union[List[float], Tensor], closed: bool = False) -> Tensor:
    """The local-thickness map of ``x > 0`` (one binary object) at the voxel spacing ``spacing``: (X, Y, Z) float64 on
    x's device, for every voxel of the mask the radius of the largest open ball around a voxel centre that holds voxels
    of the mask only and holds the voxel, and 0 elsewhere (Hildebrand and Ruegsegger's local thickness as a radius;
    ``lib.morphology.local_thickness`` gives the exact squared values).  Distances run between voxel centres, without a
    half-voxel correction; ``closed`` is ``get_inscribed_radius``'s, and a mask that fills the volume in open mode is
    ``inf`` everywhere.  The largest value of the map is ``get_inscribed_radius``."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    return torch.sqrt(instance_local_thickness((x > 0).to(torch.int32), _spacing(spacing), closed)[2])


def get_intensity(x: Tensor, image: Tensor) -> Tensor:
    """The mean of ``image`` under every instance of the (X, Y, Z) mask ``x``: (N) float64 on x's device, one value per
    positive id in ascending order -- one value for a binary mask -- ``S v / n`` of exact integer sums
    (``compare.intensity_columns``).  ``image`` is uint8 or uint16 of the mask's shape on its device
    (``lib.instance_intensity``); the histogram is not computed.  A mask without foreground gives an empty tensor."""
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on the MI355X: the measurement is a HIP kernel and has no CPU fallback")
    _, moments, _, _, _ = instance_intensity(x, image, want_hist=False)
    n = moments[:, 0].cpu().tolist()
    sv = moments[:, 1].cpu().tolist()
    return torch.tensor([b / a for a, b in zip(n, sv)], dtype=torch.float64).to(x.device)
