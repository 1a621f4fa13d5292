"""``python -m skoots_amd.utils.remove_margin image mask``: crop the [50, 50, 5] margin ``eval()`` works with off an
image / mask pair, for correcting training data (skoots/utils/remove_margin.py).  A crop of two files: host work."""
from __future__ import annotations

import os
from typing import Tuple


def remove_margin(im_path: str, mask_path: str) -> Tuple[str, str]:
    """Writes ``<file>_removed_margins<ext>`` for both [Z, X, Y] stacks, cropped to ``[5:-5, 50:-50, 50:-50]``; returns
    the two paths.  The reference's assertions (:36-47) are ``ValueError``s here."""
    from ..lib import tiff
    for p in (im_path, mask_path):
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} does not exist")
    im = tiff.read_image(im_path)
    print(f"Image loaded with shape: {im.shape} and dtype: {im.dtype}.", flush=True)
    ma = tiff.read_image(mask_path)
    print(f"Mask loaded with shape: {ma.shape} and dtype: {ma.dtype}.", flush=True)
    if im.shape != ma.shape:
        raise ValueError(f"image shape {im.shape} != mask shape {ma.shape}")
    if im.ndim != 3:
        raise ValueError(f"image and mask must be 3-D [Z, X, Y], got {im.ndim}-D")
    for axis, (name, least) in enumerate((("Z", 10), ("X", 100), ("Y", 100))):
        if not im.shape[axis] > least:
            raise ValueError(f"[Z, X, Y]: {im.shape} | {name} must be above {least}")
    im, ma = im[5:-5, 50:-50, 50:-50], ma[5:-5, 50:-50, 50:-50]
    print(f"Image shape: {im.shape}, Mask shape: {ma.shape}", flush=True)
    out = []
    for p, arr in ((im_path, im), (mask_path, ma)):
        file, ext = os.path.splitext(p)
        out.append(file + "_removed_margins" + ext)
        tiff.write_stack(out[-1], arr)
        print(f"Saved to path: {out[-1]}", flush=True)
    return out[0], out[1]


if __name__ == "__main__":
    import argparse

    parser = argparse.ArgumentParser(description="SKOOTS Utils Remove Margin")
    parser.add_argument("image_filepath", type=str, help="Path to image")
    parser.add_argument("mask_filepath", type=str, help="path to mask")
    args = parser.parse_args()
    remove_margin(args.image_filepath, args.mask_filepath)
