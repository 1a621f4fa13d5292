"""``write_ply``: the meshes of ``validate.lib.instance_meshes`` as ONE binary PLY file.  Pure host code:
numpy arrays or tensors on any device go in, a file comes out.

Layout (``binary_little_endian 1.0``): per vertex ``float x, y, z`` and ``int instance``; per face
``list uchar int vertex_indices`` (always three) and ``int instance``.  Vertex indices are global to the file; the
``instance`` property is the instance id, on the vertices and on the faces, so a viewer can colour or split by it."""
from __future__ import annotations

from typing import Optional

import numpy as np

_INT32_MAX = 2 ** 31 - 1


def _host(a, dtype) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dtype, copy=False)


def write_ply(path: str, ids, vertices, faces, vertex_offsets, face_offsets, spacing=(1.0, 1.0, 1.0), flip: bool = True,
              comment: Optional[str] = None) -> str:
    """Writes the N meshes to ``path`` and returns it.  ``ids`` (N), ``vertices`` (V, 3) in DOUBLED index coordinates,
    ``faces`` (F, 3) local to their instance, ``vertex_offsets`` and ``face_offsets`` (N + 1) are the tensors of
    ``instance_meshes``.  A coordinate is ``doubled * spacing / 2``, computed in float64 and rounded to float32 once.

    The library's faces keep scikit-image's vertex order, whose right-hand normal points into the object;
    ``flip=True`` writes every face reversed, so that normals point out of it and the signed volume is positive.
    ``comment`` becomes a ``comment`` line of the header (one line, ASCII).

    Raises ``ValueError`` when V reaches 2^31 (the indices are int32), when an id does not fit int32, or when the
    arrays do not fit each other."""
    ids = _host(ids, np.int64).reshape(-1)
    v = _host(vertices, np.int64).reshape(-1, 3)
    f = _host(faces, np.int64).reshape(-1, 3)
    vo = _host(vertex_offsets, np.int64).reshape(-1)
    fo = _host(face_offsets, np.int64).reshape(-1)
    s = np.array([float(t) for t in spacing], np.float64)
    if s.shape != (3,) or not np.all(s > 0) or not np.all(np.isfinite(s)):
        raise ValueError(f"spacing must be three positive numbers (x, y, z), got {spacing}")
    N, V, F = len(ids), len(v), len(f)
    if V >= 2 ** 31:
        raise ValueError(f"{V} vertices do not fit the int32 indices of a PLY face list; write fewer instances per file")
    if N and (ids.max() > _INT32_MAX or ids.min() < -_INT32_MAX - 1):
        bad = ids[(ids > _INT32_MAX) | (ids < -_INT32_MAX - 1)][0]
        raise ValueError(f"the id {int(bad)} does not fit the int32 instance property; renumber the mask")
    if len(vo) != N + 1 or len(fo) != N + 1 or vo[0] != 0 or fo[0] != 0 or vo[-1] != V or fo[-1] != F or \
            np.any(np.diff(vo) < 0) or np.any(np.diff(fo) < 0):
        raise ValueError(f"offsets do not fit: {N} ids, {V} vertices, {F} faces, vertex_offsets {vo.tolist()[:4]}.., "
                         f"face_offsets {fo.tolist()[:4]}..")
    nv, nf = np.diff(vo), np.diff(fo)
    if F and (f.min() < 0 or np.any(f >= np.repeat(nv, nf)[:, None])):
        raise ValueError("a face names a vertex outside its instance")
    if comment is not None and ("\n" in comment or "\r" in comment or not comment.isascii()):
        raise ValueError("comment must be one line of ASCII")

    vert = np.zeros(V, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("instance", "<i4")]))
    xyz = v.astype(np.float64) * s / 2.0
    for k, name in enumerate("xyz"):
        vert[name] = xyz[:, k].astype(np.float32)
    vert["instance"] = np.repeat(ids, nv)
    face = np.zeros(F, np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("instance", "<i4")]))
    face["n"] = 3
    glob = f + np.repeat(vo[:-1], nf)[:, None]
    face["v"] = glob[:, ::-1] if flip else glob
    face["instance"] = np.repeat(ids, nf)
    header = ["ply", "format binary_little_endian 1.0"]
    if comment is not None:
        header.append(f"comment {comment}")
    header += [f"element vertex {V}", "property float x", "property float y", "property float z",
               "property int instance", f"element face {F}", "property list uchar int vertex_indices",
               "property int instance", "end_header"]
    with open(path, "wb") as file:
        file.write(("\n".join(header) + "\n").encode("ascii"))
        file.write(vert.tobytes())
        file.write(face.tobytes())
    return path
