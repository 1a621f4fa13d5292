#!/usr/bin/env python3
"""Generate tests/golden/mesh.npz: scikit-image's own marching-cubes meshes of single instances.

Run where scikit-image (written with 0.18.3) is available; the tests read only the committed .npz.  The interpreter
needs numpy and scikit-image, and no torch and nothing of this project:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mesh_golden.py

Per input, id and mode it calls ``skimage.measure.marching_cubes((mask == id) * 255)`` -- what the reference's
``get_surface_area`` meshes (skoots/validate/stats.py:30-48) -- on the mask as it is (open) and padded with one layer of
zeros (closed).  Every vertex is an edge midpoint, so twice its coordinates are integers; they are stored relative to
the unpadded volume.  Stored per mesh: ``<name>_<id>_<mode>_tri`` (F, 3, 3) int16, the triangles as doubled
coordinates, each rotated so that its smallest vertex (x, then y, then z) comes first, which keeps the orientation, and
the rows sorted; ``<name>_<id>_<mode>_v`` the number of vertices scikit-image returned (it welds them).

Inputs: the mask of instance_stats.npz (ids 3 and 7 share a face, 300 is ragged, 1000 is one voxel in the corner), a
6 x 7 x 8 volume of 50 % noise as one label, the two touching ellipsoids of surface_area.npz, and a ball, a hollow ball
and a torus in 15 x 15 x 9 (Euler characteristic 2, 4 and 0 when closed).  The masks that no other fixture holds are
stored as ``<name>_mask``.
"""
import os

import numpy as np
from skimage.measure import marching_cubes

HERE = os.path.dirname(os.path.abspath(__file__))


def solids(shape=(15, 15, 9)):
    g = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1).astype(np.float64)
    d = g - (7.0, 7.0, 4.0)
    r = np.sqrt((d ** 2).sum(-1))
    ring = np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - 4.5) ** 2 + d[..., 2] ** 2)
    return {"ball": (r < 3.6).astype(np.int32) * 2, "hollow_ball": ((r < 3.6) & (r >= 1.5)).astype(np.int32) * 2,
            "torus": (ring < 1.6).astype(np.int32) * 2}


def canonical(verts, faces, shift):
    d = verts.astype(np.float64) * 2
    assert np.array_equal(d, np.round(d)), "a vertex is not on the half grid"
    t = (d.astype(np.int64) - shift)[faces.astype(np.int64)]            # (F, 3, 3)
    rank = (t[..., 0] * 2 ** 20 + t[..., 1]) * 2 ** 20 + t[..., 2]
    k = np.argmin(rank, axis=1)
    t = t[np.arange(len(t))[:, None], (k[:, None] + np.arange(3)) % 3]
    t = t[np.lexsort(t.reshape(len(t), 9).T[::-1])]
    assert np.abs(t).max() < 2 ** 15
    return t.astype(np.int16)


def main():
    masks = {
        "instance_stats": np.load(os.path.join(HERE, "instance_stats.npz"))["mask"][0],
        "noise": (np.random.default_rng(2424).random((6, 7, 8)) < 0.5).astype(np.int32) * 4,
        "ellipsoids": np.load(os.path.join(HERE, "surface_area.npz"))["ellipsoids_mask"],
    }
    masks.update(solids())
    out = {"names": np.array(list(masks))}
    for name, lab in masks.items():
        if name not in ("instance_stats", "ellipsoids"):
            out[name + "_mask"] = lab.astype(np.int32)
        ids = np.unique(lab)
        ids = ids[ids > 0]
        out[name + "_ids"] = ids.astype(np.int64)
        for u in ids:
            one = (lab == u).astype(np.float64) * 255
            for mode, vol, shift in (("open", one, 0), ("closed", np.pad(one, 1), 2)):
                verts, faces, _, _ = marching_cubes(vol)
                assert len(np.unique(verts, axis=0)) == len(verts), "scikit-image did not weld the vertices"
                tri = canonical(verts, faces, shift)
                out[f"{name}_{u}_{mode}_tri"], out[f"{name}_{u}_{mode}_v"] = tri, np.int64(len(verts))
                print(name, lab.shape, int(u), mode, "V", len(verts), "F", len(faces), "chi", len(verts) - len(faces) / 2)
    path = os.path.join(HERE, "mesh.npz")
    np.savez_compressed(path, **out)
    print(f"mesh.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
