#!/usr/bin/env python3
"""Generate tests/golden/convert.npz from the REFERENCE's own ``convert`` (skoots/utils/convert_trch_to_tif.py).

Run where the reference checkout is available (the tests read only the committed .npz), like make_validate_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_convert_golden.py

``zarr`` and ``skimage.io`` are stand-ins: ``zarr.load`` hands over the array registered for the store's name, and
``skimage.io.imsave`` captures (file name, array, compression) instead of writing.  ``.trch`` files are real
``torch.save`` files that the reference reads itself.

  G14 convert.npz  per case: <case>_in (the array; a case with the input of an earlier one holds that case's name),
                   <case>_kind ("zarr" / "trch"), <case>_out (what imsave was given), <case>_name (base name of the
                   output), <case>_compression ("zlib" or "")
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_STORES = {}
_SAVED = []


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _imsave(fname, arr, **kwargs):
    _SAVED.append((os.path.basename(fname), np.array(arr), kwargs.get("compression") or ""))


_stub("zarr", load=lambda path: _STORES[os.path.basename(path)])
_sk = _stub("skimage")
_sk.io = _stub("skimage.io", imsave=_imsave)

from skoots.utils.convert_trch_to_tif import convert as ref_convert  # noqa: E402


def every_fp16_up_to_one():
    """Every fp16 value with |x| <= 1 (30 722 bit patterns, -0.0 included) laid into one (3, 11, 31, 31) array."""
    bits = np.concatenate([np.arange(0x0000, 0x3C01), np.arange(0x8000, 0xBC01)]).astype(np.uint16)
    assert bits.size == 30722
    flat = np.zeros(3 * 11 * 31 * 31, dtype=np.uint16)
    # spread over the array by a stride coprime to its size, so that neighbours along every axis differ
    n = flat.size
    flat[(np.arange(bits.size, dtype=np.int64) * 7919) % n] = bits
    return flat.view(np.float16).reshape(3, 11, 31, 31)


def cases():
    gen = torch.Generator().manual_seed(1414)
    vec = (torch.rand((3, 5, 7, 9), generator=gen) * 2 - 1).to(torch.float16)
    vec[0, 1, 2, 3] = 0.0
    vec[2, 4, 6, 8] = -0.0
    vec[1, 0, 0, 0] = 1.0
    vec[1, 0, 0, 1] = -1.0
    skel = (torch.rand((1, 5, 7, 9), generator=gen) < 0.3).to(torch.uint8)
    big = torch.rand((3, 5, 7, 9), generator=gen) * 255.99
    big[0, 0, 0, 0], big[0, 0, 0, 1] = 2.0, 255.5
    lab = torch.randint(0, 70000, (5, 7, 9), generator=gen, dtype=torch.int32)
    half3 = (torch.rand((5, 7, 9), generator=gen) * 2 - 1).to(torch.float16)
    half3[2, 3, 4] = 0.0
    allh = every_fp16_up_to_one()
    return [("vectors_store", "zarr", vec.numpy()), ("skeleton_store", "zarr", skel.numpy()),
            ("cast_store", "zarr", big.numpy()), ("labels_store", "zarr", lab.numpy()),
            ("vectors_trch", "trch", vec.numpy()), ("half3_trch", "trch", half3.numpy()),
            ("labels_trch", "trch", lab.numpy()), ("every_fp16_store", "zarr", allh),
            ("every_fp16_trch", "trch", allh)]


def main():
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, kind, arr in cases():
            path = os.path.join(tmp, name + "." + kind)
            if kind == "zarr":
                os.makedirs(path)
                _STORES[os.path.basename(path)] = arr.copy()
            else:
                torch.save(torch.from_numpy(arr.copy()), path)
            del _SAVED[:]
            ref_convert(path)
            assert len(_SAVED) == 1, (name, len(_SAVED))
            fname, saved, compression = _SAVED[0]
            same = [n for n in names if out[n + "_in"].dtype == arr.dtype and np.array_equal(out[n + "_in"].view(np.uint8),
                                                                                              arr.view(np.uint8))]
            out[name + "_in"], out[name + "_kind"] = (np.array(same[0]) if same else arr), np.array(kind)
            out[name + "_out"], out[name + "_name"], out[name + "_compression"] = saved, np.array(fname), np.array(compression)
            names.append(name)
            print(f"{name}: {arr.shape} {arr.dtype} -> {fname} {saved.shape} {saved.dtype} compression={compression!r}")
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "convert.npz")
    np.savez_compressed(path, **out)
    print(f"convert.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
