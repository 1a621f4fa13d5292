"""The cases of tests/golden/convert.npz (make_convert_golden.py: what the reference's ``convert`` handed to
``skimage.io.imsave``), shared by test_convert.py and test_hip_convert.py."""
import os
from typing import NamedTuple

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convert.npz")


class Case(NamedTuple):
    name: str
    kind: str            # "zarr" / "trch"
    array: np.ndarray    # the input
    out: np.ndarray      # the array the reference saved
    out_name: str        # base name of the file it saved to
    compression: str     # "zlib" or ""


_CACHE = {}


def load_cases():
    if not _CACHE:
        with np.load(GOLDEN) as z:
            for name in z["cases"].tolist():
                arr = z[name + "_in"]
                if arr.dtype.kind == "U":       # the input of an earlier case
                    arr = z[str(arr) + "_in"]
                _CACHE[name] = Case(name, str(z[name + "_kind"]), arr, z[name + "_out"], str(z[name + "_name"]),
                                    str(z[name + "_compression"]))
    return _CACHE


CASE_NAMES = ("vectors_store", "skeleton_store", "cast_store", "labels_store", "vectors_trch", "half3_trch",
              "labels_trch", "every_fp16_store", "every_fp16_trch")


def write_case(case: Case, directory: str) -> str:
    """The case's input as a real file: a zarr store or a ``torch.save`` file."""
    from skoots_amd.lib import zarr_store
    path = os.path.join(directory, case.name + "." + case.kind)
    if case.kind == "zarr":
        zarr_store.save(path, case.array)
    else:
        torch.save(torch.from_numpy(case.array.copy()), path)
    return path


def expected_pages(case: Case) -> np.ndarray:
    """What the file must read back as: the captured array, (Z, X, Y, 1) as the (Z, X, Y) grey pages it is written as."""
    return case.out[..., 0] if case.out.ndim == 4 and case.out.shape[3] == 1 else case.out
