"""The ``huffman`` keyword on its way from the command line to ``deflate_streams``, without a GPU: on CPU tensors both
modes go through ``zlib.compress(row, 1)``, so the files must be byte for byte those written without the keyword, and
any other value is refused before a file is touched."""
import os
import zlib

import numpy as np
import pytest
import torch

from skoots_amd.lib import deflate, tiff, zarr_store


def test_deflate_streams_modes_on_cpu_rows():
    rng = np.random.default_rng(1)
    rows = torch.from_numpy((rng.integers(0, 4, (3, 5000)) * (rng.random((3, 5000)) < 0.3)).astype(np.uint8))
    want = [zlib.compress(r.numpy().tobytes(), 1) for r in rows]
    assert deflate.deflate_streams(rows) == want
    assert deflate.deflate_streams(rows, huffman="fixed") == want
    assert deflate.deflate_streams(rows, huffman="dynamic") == want
    for bad in ("Dynamic", "best", "", None, 0, 1):
        with pytest.raises(ValueError, match="huffman"):
            deflate.deflate_streams(rows, huffman=bad)
    with pytest.raises(ValueError, match="huffman"):
        deflate.deflate_streams(torch.zeros((0, 4), dtype=torch.uint8), huffman="none")


def _tree(path):
    if os.path.isfile(path):
        return open(path, "rb").read()
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


def test_writers_take_the_keyword(tmp_path):
    rng = np.random.default_rng(2)
    vec = (rng.standard_normal((2, 70, 40, 33)) * (rng.random((2, 70, 40, 33)) < 0.2)).astype(np.float16)
    lab = torch.from_numpy(rng.integers(0, 9, (3, 20, 30)).astype(np.int32))
    flt = rng.standard_normal((2, 9, 11)).astype(np.float32)
    made = {}
    for mode in (None, "fixed", "dynamic"):
        kw = {} if mode is None else {"huffman": mode}
        d = tmp_path / str(mode)
        d.mkdir()
        zarr_store.save_device(str(d / "v.zarr"), vec, (1, 32, 32, 16), **kw)
        tiff.write_stack(str(d / "s.tif"), lab.to(torch.uint8), **kw)
        tiff.write_label_stack(str(d / "l.tif"), lab, **kw)
        tiff.write_float_stack(str(d / "f.tif"), flt, **kw)
        made[mode] = {n: _tree(str(d / n)) for n in ("v.zarr", "s.tif", "l.tif", "f.tif")}
    assert made[None] == made["fixed"] == made["dynamic"]
    for fn in (lambda p: zarr_store.save_device(p, vec, huffman="huff"),
               lambda p: tiff.write_stack(p, lab.to(torch.uint8), huffman="huff"),
               lambda p: tiff.write_label_stack(p, lab, huffman="huff"),
               lambda p: tiff.write_float_stack(p, flt, huffman="huff")):
        path = str(tmp_path / "refused")
        with pytest.raises(ValueError, match="huffman"):
            fn(path)
        assert not os.path.exists(path)


def test_command_line_and_eval_default():
    from skoots_amd.__main__ import parse_args
    from skoots_amd.lib import eval as E
    assert E.OUTPUT_HUFFMAN == "fixed"
    assert parse_args(["--image", "x.tif"]).output_huffman is None
    assert parse_args(["--image", "x.tif", "--output-huffman", "dynamic"]).output_huffman == "dynamic"
    assert parse_args(["--convert", "dir", "--output-huffman", "fixed"]).output_huffman == "fixed"
    with pytest.raises(SystemExit):
        parse_args(["--image", "x.tif", "--output-huffman", "best"])
    with pytest.raises(ValueError, match="huffman"):   # refused before the checkpoint is opened
        E.eval("no_such_image.tif", "no_such_checkpoint.trch", output_huffman="best")


def test_convert_takes_the_keyword(tmp_path):
    from skoots_amd.utils.convert_trch_to_tif import convert
    with pytest.raises(ValueError, match="huffman"):
        convert(str(tmp_path), "cpu", huffman="best")
    assert convert(str(tmp_path), "cpu", huffman="dynamic") == []
