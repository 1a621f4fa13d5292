#!/usr/bin/env python3
"""Generate tests/golden/forward_trace.json: every library call ``HipUNet.forward_tiles`` issues, per configuration.

The forward runs WITHOUT a GPU: the model is built on the CPU, ``_ffi.lib`` is replaced by a recorder that lets the
host-only functions through (``*_num_blocks``, ``*_workspace_bytes``, ``*pack_weight*_host``) and records every other
call -- scalars as they are, pointers resolved at call time to the name of the tensor they point at -- and returns 0.
No kernel runs; the buffers hold whatever ``torch.empty`` left in them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_forward_trace_golden.py

tests/test_forward_plan.py repeats the recording (``record_all``) and compares it with the committed file, so the
fixture is regenerated only when the launch sequence is MEANT to change.  Names of pointers: activation and scratch
buffers by their ``_bufs`` tag, layer tensors ``<layer>.bias|gamma|beta|w[<packed key>]``, ``image``, ``zeros``,
``heads.w|b`` (on the CPU the fp32 mode's ``head_w5`` is a view of the same storage and reads ``heads.w``),
``stream``, or null; a pointer that has no name is an error.  Precision "fp32" works on fresh allocations: its
tensors other than the layers' are recorded as "*".  The file holds every distinct call once (``calls``), every
distinct trace once as indices into them (``traces``) and the table configuration -> trace.

``sk_conv3d_upfold_num_blocks`` accepts every thin tile (extents that are multiples of 4 have even halves, the only
thing it asks of x and y); what it refuses is a DEEP one: z = 32 at level 0 only, z = 64 at both decoder levels
(``REFUSED_TILES``, run on a deeper image), which puts the unfolded decoder path into the table.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from skoots_amd import _ffi, unet  # noqa: E402

NETWORKS = (((32, 64, 128, 64, 32), (2, 2, 2, 2, 2)), ((32, 32, 64, 32, 32), (1, 2, 3, 2, 1)),
            ((32, 64, 64, 64, 32), (3, 1, 1, 1, 3)))
SWITCHES = ("defer_activation", "fold_upsample", "box_store", "stem_single_pass")
IMAGE_SHAPE, TILE, ODD_TILE = (64, 64, 24), (60, 64, 20), (58, 63, 18)
DEEP_IMAGE_SHAPE, REFUSED_TILES = (64, 64, 72), ((16, 16, 32), (16, 16, 64))   # the folded conv covers level 1 only / neither
ORIGINS = ((0, 0, 0), (4, 0, 4))
MEAN, STD = 0.5, 0.25
STREAM = 0x5757
HOST_ONLY = ("_num_blocks", "_workspace_bytes", "_host")


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return 0.0


def _address(v):
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    if isinstance(v, C.c_void_p):
        return v.value or 0
    return C.cast(v, C.c_void_p).value or 0


class Recorder:
    """Stands in for ``_ffi.lib`` while one model runs on the CPU."""

    def __init__(self, lib, model, image, exact_names):
        self._lib, self._model, self._image, self._exact = lib, model, image, exact_names
        self.calls = []

    def _names(self):
        m = self._model
        names = {STREAM: "stream", self._image.data_ptr(): "image", m.zeros.data_ptr(): "zeros",
                 m.head_w5.data_ptr(): "heads.w5", m.head_w.data_ptr(): "heads.w", m.head_b.data_ptr(): "heads.b"}
        for (tag, _), t in m._bufs.items():
            assert names.setdefault(t.data_ptr(), tag) == tag, (tag, names[t.data_ptr()])
        for layer in _layers(m):
            for attr in ("bias", "gamma", "beta", "weight_f32"):
                names.setdefault(getattr(layer, attr).data_ptr(), f"{layer.name}.{attr}")
            for key, w in layer._packed.items():
                w = w[0] if isinstance(w, tuple) else w
                names.setdefault(w.data_ptr(), f"{layer.name}.w[{key!r}]")
        return names

    def _name(self, v, names):
        a = _address(v)
        if a == 0:
            return None
        if a not in names and self._exact:
            raise KeyError(f"a pointer argument {a:#x} has no name")
        return names.get(a, "*")

    def __getattr__(self, fname):
        fn = getattr(self._lib, fname)
        if fname.endswith(HOST_ONLY):
            return fn
        argtypes = _ffi._SIGS[fname][1]

        def record(*args):
            assert len(args) == len(argtypes), fname
            names, rec = self._names(), [fname]
            for i, (v, ty) in enumerate(zip(args, argtypes)):
                if ty is C.POINTER(_ffi.ConvSrc):
                    rec.append([[self._name(s.data, names), self._name(s.affine, names), s.c, s.upsample]
                                for s in v[:args[i + 1]]])
                elif ty is _ffi.ip:
                    rec.append(None if v is None else [int(x) for x in v])
                elif ty is _ffi.vp:
                    rec.append(self._name(v, names))
                else:
                    rec.append(v)
            self.calls.append(rec)
            return 0
        return record


def _layers(model):
    """Every conv layer object of the model, wherever it keeps them."""
    found = []

    def visit(v):
        if hasattr(v, "gamma") and hasattr(v, "_packed"):
            found.append(v)
        elif isinstance(v, (list, tuple)):
            for x in v:
                visit(x)
        elif isinstance(v, dict):
            for x in v.values():
                visit(x)
    for v in vars(model).values():
        visit(v)
    return found


def record(model, image, tile, keep_features, out_box):
    """One ``forward_tiles`` call under the recorder -> the trace as a JSON-ready dict."""
    saved = _ffi.lib, _ffi.stream_ptr, _ffi.require_gpu, torch.cuda.Event, torch.cuda.current_stream
    rec = Recorder(_ffi.lib, model, image, exact_names=model.precision != "fp32")
    _ffi.lib, _ffi.stream_ptr, _ffi.require_gpu = rec, (lambda device=None: C.c_void_p(STREAM)), (lambda t, name: None)
    torch.cuda.Event, torch.cuda.current_stream = _Event, (lambda device=None: None)
    model.profile = unet.ConvProfile()
    try:
        out = model.forward_tiles(image, ORIGINS, tile, MEAN, STD, keep_features=keep_features, out_box=out_box)
        trace = {"calls": rec.calls, "out_shape": list(out.shape), "features": list(model.last_features),
                 "executed_flops": model.profile.executed_flops,
                 "events": [[flops, name] for _, _, flops, name in model.profile.events]}
        if model.precision != "fp32":
            assert out.data_ptr() == model._bufs[("out5", torch.float16)].data_ptr()
    finally:
        _ffi.lib, _ffi.stream_ptr, _ffi.require_gpu, torch.cuda.Event, torch.cuda.current_stream = saved
        model.profile = None
    return trace


def fold_covers(tile):
    """Per decoder level 0, 1: does the folded kernel cover this tile (for both widths it is built for)?"""
    up = _ffi.lib.sk_conv3d_upfold_num_blocks
    return [all(up(tile[0] >> l, tile[1] >> l, tile[2] >> l, c) > 0 for c in (32, 64)) for l in (0, 1)]


def configurations():
    """(key, network index, precision, switch values, tile, keep_features, with out_box) of every recorded call."""
    cfgs = []
    on = (True, True, True, False)   # the switches' defaults
    for n, prec in itertools.product(range(len(NETWORKS)), ("fp16", "split", "mix8")):
        for sw in itertools.product((True, False), repeat=len(SWITCHES)):
            for keep, box in itertools.product((False, True), repeat=2):
                cfgs.append((n, prec, sw, TILE, keep, box))
        for box in (False, True):
            cfgs.append((n, prec, on, ODD_TILE, False, box))
    for n in range(len(NETWORKS)):
        cfgs.append((n, "fp32", on, TILE, False, True))
    cfgs.append((0, "fp32", on, ODD_TILE, False, False))
    assert [fold_covers(t) for t in REFUSED_TILES] == [[False, True], [False, False]] and fold_covers(TILE) == [True, True]
    for tile, n, prec in itertools.product(REFUSED_TILES, range(len(NETWORKS)), ("fp16", "split", "mix8")):
        cfgs.append((n, prec, on, tile, False, True))
    for n, prec, sw, tile, keep, box in cfgs:
        key = "net%d %s %s tile=%s keep=%d box=%d" % (n, prec, "".join("01"[v] for v in sw), "x".join(map(str, tile)), keep, box)
        yield key, n, prec, sw, tile, keep, box


def state_dict_digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


def record_all():
    """The fixture's content: distinct traces (stored once each), the table configuration -> trace, weight digests."""
    image, deep = torch.zeros(IMAGE_SHAPE, dtype=torch.float16), torch.zeros(DEEP_IMAGE_SHAPE, dtype=torch.float16)
    sds = [unet.random_state_dict(d, p) for d, p in NETWORKS]
    models = [unet.HipUNet(sd, "cpu", d, p) for sd, (d, p) in zip(sds, NETWORKS)]
    calls, traces, index, table = {}, [], {}, {}
    for key, n, prec, sw, tile, keep, box in configurations():
        m = models[n]
        m.precision = prec
        for name, v in zip(SWITCHES, sw):
            setattr(m, name, v)
        t = record(m, deep if tile in REFUSED_TILES else image, tile, keep, ((2, 3, 1), tuple(v - 4 for v in tile)) if box else None)
        t["calls"] = [calls.setdefault(json.dumps(c), len(calls)) for c in t["calls"]]
        s = json.dumps(t)
        if s not in index:
            index[s] = len(traces)
            traces.append(t)
        table[key] = index[s]
    return {"state_dict_sha256": [state_dict_digest(sd) for sd in sds], "configurations": table, "traces": traces,
            "calls": [json.loads(c) for c in calls]}


def dump(doc, path):
    """Readable and compact: one configuration, one trace and one call per line."""
    def lines(items):
        return ",\n".join("  " + json.dumps(v, separators=(",", ":")) for v in items)
    with open(path, "w") as f:
        f.write('{"state_dict_sha256": %s,\n "configurations": {\n' % json.dumps(doc["state_dict_sha256"]))
        f.write(",\n".join("  %s: %d" % (json.dumps(k), v) for k, v in doc["configurations"].items()))
        f.write('},\n "traces": [\n%s],\n "calls": [\n%s]}\n' % (lines(doc["traces"]), lines(doc["calls"])))


if __name__ == "__main__":
    doc = record_all()
    path = os.path.join(HERE, "forward_trace.json")
    dump(doc, path)
    assert json.load(open(path)) == json.loads(json.dumps(doc))
    print(f"forward_trace.json: {os.path.getsize(path) / 1024:.0f} KiB, {len(doc['configurations'])} configurations, "
          f"{len(doc['traces'])} distinct traces of {len(doc['calls'])} distinct calls")
