"""Minimal zarr v2 directory store, enough for the two intermediates ``eval()`` leaves next to the image --
``<base>_skoots_skeleton.zarr`` and ``<base>_skoots_vectors.zarr`` (skoots/lib/eval.py:101-111,160-176).

The ``zarr`` / ``numcodecs`` packages are not in this image.  What is written here follows the published v2 layout
(``.zarray`` JSON + one C-order file per chunk, edge chunks padded to the full chunk shape), so the real package opens
it.  Chunks are compressed with the numcodecs ``zlib`` codec (``{"id": "zlib", "level": 1}`` -- the stdlib's zlib) or
stored raw (``compressor=None``); chunks that hold only the fill value are not written, as zarr does.  ``load`` reads
raw, zlib and gzip stores and the stores the reference itself writes: zarr's default ``blosc`` compressor with the lz4
codec and byte shuffle (``lib/blosc.py``; the frame carries everything, the ``.zarray`` fields ``cname``, ``shuffle`` and
``blocksize`` are not looked at).  Before any chunk of a ``blosc`` store is decoded the first 16 bytes of every chunk
file are checked: a file that is no Blosc-1 frame of a chunk, another inner codec (blosclz, zlib, zstd, snappy) or
bitshuffle refuses the whole store with a ``RuntimeError`` that names the file and the codec.  Every other codec and
every filter is refused by name.  Blosc is only read, never written: the zlib stores open everywhere.

``save_device`` writes the same zlib store from a torch tensor without taking the array to the host first: chunks are
gathered and deflated on the tensor's device (``lib/deflate.py``), only compressed bytes cross to the host.
``load_device`` is the way back: chunk files go to the device as they are and are inflated (zlib) or expanded and
unshuffled (blosc) there."""
from __future__ import annotations

import gzip
import itertools
import json
import os
import shutil
import time
import zlib
from typing import Optional, Sequence

import numpy as np


def _dtype_str(dt: np.dtype) -> str:
    dt = np.dtype(dt)
    return dt.str if dt.itemsize > 1 else "|" + dt.str[1:]


def save(path: str, arr: np.ndarray, chunks: Optional[Sequence[int]] = None, compressor: Optional[str] = "zlib",
         level: int = 1) -> None:
    arr = np.ascontiguousarray(arr)
    if chunks is None:
        chunks = [min(s, c) for s, c in zip(arr.shape, (1, 256, 256, 64)[-arr.ndim:])]
    chunks = [max(1, int(c)) for c in chunks]
    if os.path.isdir(path):
        shutil.rmtree(path)
    os.makedirs(path)
    if compressor not in (None, "zlib"):
        raise ValueError("compressor must be None or 'zlib'")
    meta = {"zarr_format": 2, "shape": list(arr.shape), "chunks": chunks, "dtype": _dtype_str(arr.dtype),
            "compressor": {"id": "zlib", "level": int(level)} if compressor else None, "fill_value": 0, "order": "C",
            "filters": None}
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f, indent=2)
    grid = [range((s + c - 1) // c) for s, c in zip(arr.shape, chunks)]
    for idx in itertools.product(*grid):
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, arr.shape))
        block = np.zeros(chunks, dtype=arr.dtype)
        part = arr[sl]
        if not part.any():
            continue  # only the fill value: zarr leaves such chunks out (write_empty_chunks=False)
        block[tuple(slice(0, n) for n in part.shape)] = part
        raw = block.tobytes()
        with open(os.path.join(path, ".".join(str(i) for i in idx)), "wb") as f:
            f.write(zlib.compress(raw, int(level)) if compressor else raw)


SAVE_DEVICE_BUDGET = 256 << 20  # bytes of staging + encoder buffers per batch of chunks (see save_device)


def save_device(path: str, tensor, chunks: Optional[Sequence[int]] = None, budget_bytes: int = SAVE_DEVICE_BUDGET,
                timings=None, huffman: str = "fixed") -> None:
    """The store ``save(path, array, compressor="zlib")`` writes -- same default chunks, same ``.zarray`` text, edge
    chunks zero-padded, fill-value chunks left out -- from a torch tensor on either device (a numpy array is taken as a
    CPU tensor).  Chunks are copied into a ``(n, chunk_bytes)`` staging buffer with torch indexing on the tensor's device
    and deflated there in batches: one batch takes about three times its chunks' bytes (staging, the encoder's worst-case
    output, its workspace), and a batch is sized to keep that under ``budget_bytes`` (256 MiB by default; at least one
    chunk), so the memory this takes does not grow with the array.  On a CPU tensor the files are byte for byte
    those of ``save``; on a device tensor the chunk files hold other bytes that inflate to the same chunks.
    ``huffman`` (``"fixed" | "dynamic"``) goes to ``deflate.deflate_streams``: it changes the chunk files' bytes on a
    device tensor, never the ``.zarray`` text or what the chunks inflate to."""
    import torch

    from . import deflate
    # refused before the store is touched; the keyword goes down only when it is not the default
    coded = {"huffman": huffman} if deflate.huffman_mode(huffman) else {}
    t = torch.from_numpy(np.ascontiguousarray(tensor)) if isinstance(tensor, np.ndarray) else tensor
    np_dtype = torch.empty(0, dtype=t.dtype).numpy().dtype
    if chunks is None:
        chunks = [min(s, c) for s, c in zip(t.shape, (1, 256, 256, 64)[-t.ndim:])]
    chunks = [max(1, int(c)) for c in chunks]
    if os.path.isdir(path):
        shutil.rmtree(path)
    os.makedirs(path)
    meta = {"zarr_format": 2, "shape": list(t.shape), "chunks": chunks, "dtype": _dtype_str(np_dtype),
            "compressor": {"id": "zlib", "level": 1}, "fill_value": 0, "order": "C", "filters": None}
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f, indent=2)
    item = np_dtype.itemsize
    chunk_bytes = int(np.prod(chunks)) * item
    grid = [range((s + c - 1) // c) for s, c in zip(t.shape, chunks)]
    todo = [idx for idx in itertools.product(*grid)]
    per_chunk = chunk_bytes + deflate.device_bytes_per_stream(chunk_bytes)
    batch = max(1, int(budget_bytes) // per_chunk)
    by_value = np_dtype.kind not in "iub"   # -0.0 is the fill value too: such dtypes are tested by value, as save does
    for lo in range(0, len(todo), batch):
        part = todo[lo:lo + batch]
        staging = torch.zeros([len(part)] + chunks, dtype=t.dtype, device=t.device)
        for b, idx in enumerate(part):
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, t.shape))
            src = t[sl]
            staging[b][tuple(slice(0, n) for n in src.shape)] = src
        rows = staging.view(len(part), -1)
        if by_value:
            keep = rows.ne(0).any(dim=1).cpu().tolist()
            part = [idx for idx, k in zip(part, keep) if k]
            if not part:
                continue
            if not all(keep):
                rows = rows[torch.tensor(keep, device=rows.device)]
        streams = deflate.deflate_streams(rows.contiguous().view(torch.uint8).view(len(part), chunk_bytes),
                                          elem_bytes=item if item in (1, 2, 4) else 1, skip_zero=not by_value,
                                          timings=timings, **coded)
        t0 = time.perf_counter()
        for idx, stream in zip(part, streams):
            if stream is None:
                continue  # only the fill value
            with open(os.path.join(path, ".".join(str(i) for i in idx)), "wb") as f:
                f.write(stream)
        if timings is not None:
            timings["file_s"] = timings.get("file_s", 0.0) + time.perf_counter() - t0


def _codec(path: str, meta: dict) -> Optional[str]:
    """The codec id of a store both readers can read; everything else is refused by name, with one text."""
    comp = meta.get("compressor")
    codec = comp.get("id") if comp else None
    if meta.get("zarr_format") != 2 or meta.get("filters") or codec not in (None, "zlib", "gzip", "blosc"):
        raise RuntimeError(f"{path}: zarr v2 stores with compressor {codec!r} / filters {meta.get('filters')!r} cannot be "
                           "read here (raw, zlib, gzip and blosc with the lz4 codec only)")
    if meta.get("order", "C") != "C":
        raise RuntimeError(f"{path}: only C-order stores are supported")
    return codec


def _check_blosc_frames(files: Sequence[str], chunk_bytes: int) -> None:
    """Looks at the first 16 bytes of every chunk file of a ``blosc`` store before any chunk is decoded: a file that is
    not a Blosc-1 frame of this store's chunks with the lz4 codec and at most a byte shuffle refuses the whole store."""
    from . import blosc
    for fn in files:
        with open(fn, "rb") as f:
            head = f.read(16)
        why = blosc.refusal(head, os.path.getsize(fn), chunk_bytes)
        if why is not None:
            raise RuntimeError(f"{fn}: not a chunk a 'blosc' store of this reader holds: {why}")


def load(path: str) -> np.ndarray:
    with open(os.path.join(path, ".zarray")) as f:
        meta = json.load(f)
    codec = _codec(path, meta)
    shape, chunks, dt = meta["shape"], meta["chunks"], np.dtype(meta["dtype"])
    out = np.full(shape, meta.get("fill_value") or 0, dtype=dt)
    grid = [range((s + c - 1) // c) for s, c in zip(shape, chunks)]
    names = [os.path.join(path, ".".join(str(i) for i in idx)) for idx in itertools.product(*grid)]
    if codec == "blosc":
        from . import blosc
        chunk_bytes = int(np.prod(chunks)) * dt.itemsize
        _check_blosc_frames([fn for fn in names if os.path.exists(fn)], chunk_bytes)
    for idx, fn in zip(itertools.product(*grid), names):
        if not os.path.exists(fn):
            continue  # missing chunk = fill value
        with open(fn, "rb") as f:
            raw = f.read()
        if codec == "zlib":
            raw = zlib.decompress(raw)
        elif codec == "gzip":
            raw = gzip.decompress(raw)
        elif codec == "blosc":
            try:
                raw = blosc.decode_host([raw], chunk_bytes)[0].tobytes()
            except blosc.BloscError as e:
                raise ValueError(f"{fn}: the Blosc frame does not decode: {e.reason}") from None
        block = np.frombuffer(raw, dtype=dt).reshape(chunks)
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
        out[sl] = block[tuple(slice(0, s.stop - s.start) for s in sl)]
    return out


LOAD_DEVICE_BUDGET = 256 << 20  # bytes of compressed + inflated chunks per batch (see load_device)


def load_device(path: str, device, budget_bytes: int = LOAD_DEVICE_BUDGET, timings=None):
    """The tensor ``torch.from_numpy(load(path)).to(device)`` gives, same metadata checks and error texts, without the
    array ever existing on the host: raw and ``zlib`` chunk files are uploaded as they are and (``zlib``) inflated on
    the device (``lib/deflate.py: inflate_streams``), in batches, then cropped (edge chunks) and copied to their place, one
    copy per chunk.  ``budget_bytes`` (256 MiB by default; a batch holds at least one chunk) bounds what a batch adds on
    the device besides the result: the uploaded chunk files + their inflated chunks.  The host holds the same chunk files
    twice for a moment (the list and its join for the one upload), which the budget does not count.
    Missing chunks are the fill value.  ``gzip`` chunks are decompressed on the host and uploaded.  ``blosc`` chunk
    files (lz4 codec) are uploaded as they are too and decoded by ``lib/blosc.py: decode_device`` (one wave per LZ4
    stream, then the byte unshuffle, which takes one more copy of the batch's chunks that the budget does not count).
    On ``"cpu"`` the same code runs with the stdlib's zlib and the host build of the Blosc decoder.  A chunk that does
    not decode to the chunk's size raises ``ValueError`` naming its file."""
    import torch

    from . import deflate
    with open(os.path.join(path, ".zarray")) as f:
        meta = json.load(f)
    codec = _codec(path, meta)
    shape, chunks, dt = meta["shape"], meta["chunks"], np.dtype(meta["dtype"])
    if dt.byteorder == ">" or dt.kind not in "iufb":
        return torch.from_numpy(load(path)).to(device)   # nothing torch can view bytes as: the host reader decides
    tdt = torch.from_numpy(np.empty(0, dtype=dt)).dtype
    dev = torch.device(device)
    out = torch.full(shape, meta.get("fill_value") or 0, dtype=tdt, device=dev)
    chunk_bytes = int(np.prod(chunks)) * dt.itemsize
    grid = [range((s + c - 1) // c) for s, c in zip(shape, chunks)]
    todo = []
    for idx in itertools.product(*grid):
        fn = os.path.join(path, ".".join(str(i) for i in idx))
        if os.path.exists(fn):
            todo.append((idx, fn, os.path.getsize(fn)))
    if codec == "blosc":
        from . import blosc
        _check_blosc_frames([fn for _, fn, _ in todo], chunk_bytes)

    def flush(part, files):
        t0 = time.perf_counter()
        if codec == "zlib":
            try:
                rows = deflate.inflate_streams(files, chunk_bytes, dev, timings=timings)
            except deflate.InflateError as e:
                raise ValueError(f"{part[e.index][1]}: {e}") from None
        elif codec == "blosc":
            try:
                rows = blosc.decode_device(files, chunk_bytes, dev, timings=timings)
            except blosc.BloscError as e:
                raise ValueError(f"{part[e.index][1]}: the Blosc frame does not decode: {e.reason}") from None
        else:
            for (idx, fn, _), raw in zip(part, files):
                if len(raw) != chunk_bytes:
                    raise ValueError(f"{fn}: {len(raw)} bytes, a chunk of {chunks} {dt} has {chunk_bytes}")
            rows = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(dev).view(len(part), chunk_bytes)
        blocks = rows.view(tdt).view([len(part)] + list(chunks))
        for b, (idx, _, _) in enumerate(part):
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
            out[sl] = blocks[b][tuple(slice(0, s.stop - s.start) for s in sl)]
        if timings is not None:
            timings["inflate_scatter_s"] = timings.get("inflate_scatter_s", 0.0) + time.perf_counter() - t0

    part, files, held = [], [], 0
    for item in todo:
        if part and held + item[2] + chunk_bytes > int(budget_bytes):
            flush(part, files)
            part, files, held = [], [], 0
        t0 = time.perf_counter()
        with open(item[1], "rb") as f:
            raw = f.read()
        if codec == "gzip":
            raw = gzip.decompress(raw)
        if timings is not None:
            timings["file_s"] = timings.get("file_s", 0.0) + time.perf_counter() - t0
        part.append(item)
        files.append(raw)
        held += len(raw) + chunk_bytes
    if part:
        flush(part, files)
    return out
