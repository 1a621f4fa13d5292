#!/usr/bin/env python3
"""Generate tests/golden/skeleton_graph.npz with scikit-image 0.18.3: for every case of tests/skeleton_graph_cases.py,
``skimage.morphology.skeletonize_3d(lab == id)`` of every positive id on the whole volume, as one label volume.

Name an interpreter that imports scikit-image 0.18.3, as tests/golden/make_skeleton_golden.py does (this script
itself needs numpy only):

    SKIMAGE_PYTHON=<python with skimage 0.18.3> python tests/golden/make_skeleton_graph_golden.py

  skeleton_graph.npz
    names   the case names, in the order of cases()
    shapes  (n, 3) int32
    rows    the skeleton volumes, concatenated flat int32: 0 outside the skeletons, and on a skeleton voxel the ROW of
            its instance, 1 .. N in ascending order of the case's positive ids (an id itself may not fit int32)

The file holds data only.  The ring's and the T's voxel counts are asserted after generating; the other anchors are
printed, and tests/test_skeleton_graph_cpu.py asserts them."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.skeleton_graph_cases import RING_ID, T_ID, cases, positive_ids  # noqa: E402

_THIN = r"""
import sys
import numpy as np
import skimage
from skimage.morphology import skeletonize_3d
assert skimage.__version__ == "0.18.3", skimage.__version__
d = np.load(sys.argv[1])
out = {}
for i in range(int(d["n"])):
    lab = d["c%d" % i]
    u = np.unique(lab)
    rows = np.zeros(lab.shape, np.int32)
    for r, obj in enumerate(u[u > 0]):
        rows[skeletonize_3d(lab == obj) != 0] = r + 1
    out["o%d" % i] = rows
np.savez(sys.argv[2], **out)
"""


def main():
    py = os.environ.get("SKIMAGE_PYTHON")
    if not py:
        raise SystemExit("set SKIMAGE_PYTHON to an interpreter that imports scikit-image 0.18.3")
    vols = cases()
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, script = (os.path.join(tmp, n) for n in ("in.npz", "out.npz", "thin.py"))
        np.savez(src, n=len(vols), **{"c%d" % i: v for i, v in enumerate(vols.values())})
        with open(script, "w") as f:
            f.write(_THIN)
        subprocess.check_call([py, script, src, dst], env={"PATH": os.environ.get("PATH", "")})
        d = np.load(dst)
        rows = [d["o%d" % i] for i in range(len(vols))]
    for lab, r in zip(vols.values(), rows):
        ids = positive_ids(lab)
        assert r.shape == lab.shape and not ((r > 0) & (lab != np.concatenate(([0], ids))[r])).any()
    # anchors
    name = "blobs (24, 40, 70)"
    lab, r = vols[name], rows[list(vols).index(name)]
    ids = positive_ids(lab).tolist()
    n = np.bincount(r.ravel(), minlength=len(ids) + 1)[1:]
    print(name, "ids", len(ids), "ring", n[ids.index(RING_ID)], "T", n[ids.index(T_ID)],
          "thin away", [i for i, c in zip(ids, n) if c == 0], "single voxel", [i for i, c in zip(ids, n) if c == 1])
    assert n[ids.index(RING_ID)] == 60 and n[ids.index(T_ID)] == 32
    path = os.path.join(HERE, "skeleton_graph.npz")
    np.savez_compressed(path, names=np.array(list(vols)), shapes=np.array([v.shape for v in vols.values()], np.int32),
                        rows=np.concatenate([r.reshape(-1) for r in rows]).astype(np.int32))
    print("wrote", path, os.path.getsize(path), "bytes;", len(vols), "cases")


if __name__ == "__main__":
    main()
