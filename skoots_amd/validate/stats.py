"""Measurements of ONE binary mask (reference: skoots/validate/stats.py), on top of the one-pass kernel of
``validate/compare.py``.  For every instance of a mask at once use ``compare.stats_per_instance``.

``get_volume`` has the evident intent of the reference's function of that name, which cannot run
(``torch.sum`` of a Python int raises ``TypeError``, stats.py:24).

There is deliberately no ``get_surface_area``.  The reference's is a marching-cubes mesh area
(``skimage.measure.marching_cubes``, stats.py:30-48); scikit-image is not available where this project is tested, so
such an area could not be checked against it, and a function of the same name with another meaning would mislead.
``get_face_area`` is what is offered instead: the area of the exposed voxel faces, exact for what it defines and an
overestimate of a curved surface.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch
from torch import Tensor

from .compare import _spacing
from .lib import instance_sums


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
