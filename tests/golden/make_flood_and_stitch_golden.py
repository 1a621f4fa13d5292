"""Writes tests/golden/flood_and_stitch.npz from the reference's own ``watershed_and_stitch``.

Run with the reference checkout on PYTHONPATH (``skoots.utils.flood_and_stitch`` importable).  Two of the module's
imports are replaced before it loads: ``skimage.io`` (only the command uses it) and ``fastremap``, whose ``renumber``
returns its argument -- so what is stored is the stitched int32 volume BEFORE the final renumbering, the part of the
function that is pinned.  Per case: ``mask_<name>`` (uint8) and ``labels_<name>_d<dim>`` for
dim 0, 1, 2; ``names`` lists the cases.  The tests read only the .npz.

    PYTHONPATH=/path/to/reference python tests/golden/make_flood_and_stitch_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np
import scipy.ndimage

SHAPES = [(6, 17, 19), (12, 33, 31), (24, 48, 40), (3, 9, 70), (40, 20, 20)]
FIELDS = [((0.8, 2, 2), 0.02), ((0.5, 1, 1), 0.1), ((1.5, 3, 3), 0.0)]   # (gaussian sigma, threshold)


def load_reference():
    fastremap = types.ModuleType("fastremap")
    fastremap.renumber = lambda a, in_place=False: a
    fastremap.refit = lambda a: a
    skimage = types.ModuleType("skimage")
    skimage.io = types.ModuleType("skimage.io")
    sys.modules.setdefault("fastremap", fastremap)
    sys.modules.setdefault("skimage", skimage)
    sys.modules.setdefault("skimage.io", skimage.io)
    return importlib.import_module("skoots.utils.flood_and_stitch")


def random_cases():
    out = {}
    for si, shape in enumerate(SHAPES):
        for fi, (sigma, thr) in enumerate(FIELDS):
            rng = np.random.default_rng(1000 + 10 * si + fi)
            field = scipy.ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
            out[f"field{si}{fi}"] = (field > thr).astype(np.uint8)
    return out


def picture(*slices):
    """Slices as lists of strings, '#' = foreground."""
    return np.array([[[c == "#" for c in row] for row in sl] for sl in slices], dtype=np.uint8)


def hand_cases():
    out = {}
    # slice 0's component (label 1) meets labels 1, 2 and 3 of slice 1 with one voxel each: 1 is left out as "the same
    # number", the smaller of 2 and 3 must win (the largest winning gives another partition)
    out["tie"] = picture(["####", "##.."],
                         ["#.#.", ".#.."])
    # slice 2 holds labels 1..3, so the first new id is 3: the pair stitched first takes the number of slice 2's
    # third component, which touches nothing
    out["newind_taken"] = picture(["......", ".##...", ".##...", "......", "......"],
                                  ["#.....", "......", ".##...", "......", "......"],
                                  ["#.#...", "......", "......", "......", "....##"])
    # the only overlap of slice 0's component carries the same number in slice 1, so nothing is renamed; competing like
    # any other label it would be stitched under the first new id, 2, and take slice 1's unrelated component 2 along
    out["same_number"] = picture(["....", ".##.", ".##.", "...."],
                                 ["....", ".##.", "....", "...#"])
    # one object that splits in two and rejoins
    out["split_rejoin"] = picture([".......", ".#####.", ".#####.", "......."],
                                  [".......", ".##.##.", ".##.##.", "......."],
                                  [".......", ".##.##.", ".#...#.", "......."],
                                  [".......", ".#####.", ".#####.", "......."])
    out["single_slice"] = picture(["##..#..", "....#..", "#..###.", "#......", "..##..#"])
    out["empty"] = np.zeros((3, 4, 5), dtype=np.uint8)
    return out


def main():
    ref = load_reference()
    cases = {**random_cases(), **hand_cases()}
    arrays = {"names": np.array(sorted(cases))}
    for name, mask in cases.items():
        arrays[f"mask_{name}"] = mask
        for dim in range(3):
            arrays[f"labels_{name}_d{dim}"] = np.ascontiguousarray(ref.watershed_and_stitch(mask.copy(), dim)).astype(np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flood_and_stitch.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 256 * 1024, size
    print(path, size, "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
