"""``python -m skoots_amd.utils.renumber image [-o]``: renumber the instance ids of a label TIFF to 1..K
(skoots/utils/renumber.py).  The reference remaps the ids to their sorted rank and then calls ``fastremap.renumber``
(order of first appearance); both steps run on the device the stack was read to."""
from __future__ import annotations

import os

import torch


def compact_by_rank(labels: torch.Tensor):
    """The reference's first remap (:29-47): 0 stays 0, every other id becomes its rank among the sorted ids, 1..K.
    ``torch.unique`` on the tensor's device, so that the table ``sk_renumber`` needs has K entries, not ``max id``.
    Returns (int32 tensor of the same shape, K)."""
    uniq, inverse = torch.unique(labels, sorted=True, return_inverse=True)
    if int(uniq[0]) < 0:
        raise ValueError(f"negative instance id {int(uniq[0])}")
    has_zero = int(uniq[0]) == 0
    rank = inverse if has_zero else inverse + 1   # without a 0 in the volume the smallest id still becomes 1
    return rank.to(torch.int32).reshape(labels.shape), int(uniq.numel()) - (1 if has_zero else 0)


def renumber_first_seen(compact: torch.Tensor, k: int) -> torch.Tensor:
    """``fastremap.renumber`` (:54; oracle/pipeline.py: renumber): ids 1..K of the contiguous int32 ``compact`` in order of
    first appearance in C order.  On a GPU ``sk_renumber`` (in place), on ``"cpu"`` the same in torch."""
    compact = compact.contiguous()
    n = compact.numel()
    if n == 0 or k == 0:
        return compact
    if compact.is_cuda:
        from .. import _ffi
        ws_bytes = _ffi.lib.sk_renumber_workspace_bytes(n, k)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=compact.device)
        count = torch.zeros(1, dtype=torch.int32, device=compact.device)
        _ffi.check(_ffi.lib.sk_renumber(_ffi.ptr(compact), n, k, _ffi.ptr(ws), ws_bytes, _ffi.ptr(count),
                                        _ffi.stream_ptr(compact.device)))
        assert int(count.item()) == k
        return compact
    flat = compact.reshape(-1).long()
    first = torch.full((k + 1,), n, dtype=torch.int64)
    first.scatter_reduce_(0, flat, torch.arange(n), "amin")
    lut = torch.zeros(k + 1, dtype=torch.int32)
    lut[torch.argsort(first[1:]) + 1] = torch.arange(1, k + 1, dtype=torch.int32)
    return lut[flat].reshape(compact.shape)


def narrow(labels: torch.Tensor, k: int) -> torch.Tensor:
    """uint8 pages for K <= 255, uint16 for K <= 65535, else int32 (the reference writes uint32; ``write_stack`` has
    int32 pages)."""
    if k <= 255:
        return labels.to(torch.uint8)
    if k <= 65535:
        return labels.to(torch.int16).view(torch.uint16)   # the low two bytes: int16 storage holds the uint16 patterns
    return labels


def load_renumber_save(path: str, overwrite: bool = False, device=None) -> str:
    """Reads the label TIFF ``path`` ([Z, X, Y]), renumbers it and writes ``<file>_remapped<ext>``, or ``path`` itself
    with ``overwrite``.  ``device``: the current GPU if there is one, else ``"cpu"``.  Returns the path written."""
    from ..lib import tiff
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} does not exist")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    im = tiff.read_stack(path, device)
    print(f"Image loaded with shape: {tuple(im.shape)} and dtype: {im.dtype}", flush=True)
    if im.dtype in (torch.uint16, torch.uint32):
        im = im.to(torch.int64)    # torch.unique has no kernels for the wider unsigned types
    try:
        compact, k = compact_by_rank(im)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    print(f"Found {k} numbers to remap", flush=True)
    out = narrow(renumber_first_seen(compact, k), k)
    if not overwrite:
        file, ext = os.path.splitext(path)
        path = file + "_remapped" + ext
    tiff.write_stack(path, out)
    print(f"Saved to path: {path} with dtype: {out.dtype}", flush=True)
    return path


if __name__ == "__main__":
    import argparse

    parser = argparse.ArgumentParser(description="SKOOTS Utils Renumber")
    parser.add_argument("image_filepath", type=str, help="Path to image")
    parser.add_argument("-o", "--overwrite", action="store_true", help="write the result over the image")
    args = parser.parse_args()
    load_renumber_save(args.image_filepath, args.overwrite)
