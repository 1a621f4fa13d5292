"""Multi-page TIFF input shared by ``eval()`` and the training dataset (the reference reads both with skimage.io)."""
from __future__ import annotations

import numpy as np


def read_image(path: str) -> np.ndarray:
    """[Z, X, Y(, C)] array from a multi-page TIFF (Pillow) or a .npy file (eval.py:61)."""
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    pages = []
    with Image.open(path) as im:
        for i in range(getattr(im, "n_frames", 1)):
            im.seek(i)
            pages.append(np.array(im))
    return np.stack(pages, axis=0)
