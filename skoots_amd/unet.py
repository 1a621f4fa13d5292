"""HIP runner of the build's U-Net (graph: oracle/unet_spec.py ``UNetSpec``).

Stands where the reference calls ``cfg_to_bism_model(cfg)`` + ``torch.compile`` and
runs the model on each tile under fp16 autocast (skoots/lib/utils.py:17-107,
skoots/lib/eval.py:117-124,142-143).  PyTorch only owns the device memory and the
stream; every layer is a kernel of libskoots_hip.so:

  stem (VALU, Cin=1)  ->  [conv3 MFMA -> GroupNorm finalize -> fused GN+SiLU] x N
  2x2x2 stride-2 / 1x1x1 convs through the gather GEMM, heads (tanh / sigmoid).

Tiles are read in place from the HBM-resident fp16 volume (no crop copies); a batch of
B tiles runs per launch so that every launch has >> 256 workgroups.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _ffi

from .plan import PRECISIONS, Form, Kernel, conv_flops, network_blocks, plan_forward

GN_GROUPS = 8
GN_EPS = 1e-5
SWITCHES = ("precision", "defer_activation", "fold_upsample", "box_store", "stem_single_pass")

# the library function of a kernel family ("norm": the separate GroupNorm + SiLU pass; "stem apply": the stem's second
# pass) by the layout it works on
_KERNELS = {
    (Kernel.CONV, Form.F16): "sk_conv3d", (Kernel.CONV, Form.SPLIT): "sk_conv3d_split",
    (Kernel.DOWN, Form.F16): "sk_conv3d", (Kernel.DOWN, Form.SPLIT): "sk_conv3d_split",
    (Kernel.CONV_BOX, Form.F16): "sk_conv3d_box", (Kernel.CONV_BOX, Form.SPLIT): "sk_conv3d_box_split",
    (Kernel.UPFOLD, Form.F16): "sk_conv3d_upfold", (Kernel.UPFOLD, Form.SPLIT): "sk_conv3d_upfold_split",
    (Kernel.MIX8, Form.SPLIT): "sk_conv3d_mix8", (Kernel.UPFOLD_MIX8, Form.SPLIT): "sk_conv3d_upfold_mix8",
    (Kernel.DOWN_ACT, Form.F16): "sk_conv3d_down_act", (Kernel.DOWN_ACT, Form.SPLIT): "sk_conv3d_down_act_split",
    (Kernel.DOWN_ACT, Form.MIX8): "sk_conv3d_down_act_mix8",
    ("stem apply", Form.F16): "sk_conv3d_stem_apply", ("stem apply", Form.SPLIT): "sk_conv3d_stem_apply_split",
    ("stem apply", Form.MIX8): "sk_conv3d_stem_apply_mix8",
    ("norm", Form.F16): "sk_groupnorm_silu", ("norm", Form.SPLIT): "sk_groupnorm_silu_split",
    ("norm", Form.MIX8): "sk_groupnorm_silu_mix8", ("norm", Form.F32): "sk_groupnorm_silu_f32",
    (Kernel.HEADS, Form.F16): "sk_heads", (Kernel.HEADS, Form.SPLIT): "sk_heads_split",
}


def _kernel(family, form):
    return getattr(_ffi.lib, _KERNELS[family, form])


class _ConvLayer:
    """One Conv3d -> GroupNorm -> SiLU block with weights packed for the kernels."""

    def __init__(self, prefix: str, sd: Dict[str, Tensor], device, ksize: int):
        w = sd[prefix + ".conv.weight"].detach().float().cpu().contiguous()
        self.weight_f32 = w.to(device)  # torch layout, used by the fp32 precision mode
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        assert tuple(w.shape[2:]) == (ksize,) * 3, (prefix, tuple(w.shape))
        self.ksize = ksize
        self.name = prefix
        self.bias = sd[prefix + ".conv.bias"].detach().float().to(device).contiguous()
        self.gamma = sd[prefix + ".norm.weight"].detach().float().to(device).contiguous()
        self.beta = sd[prefix + ".norm.bias"].detach().float().to(device).contiguous()
        self._w_cpu, self._device, self._packed = w, device, {}
        if self.cin == 1:  # stem: (27, cout) fp32, tap-major (the kernel splits it into hi + lo itself)
            assert ksize == 3
            self._packed[False] = self._packed[True] = w.reshape(self.cout, 27).t().contiguous().to(device)

    def _cached(self, key, pack, *args):
        """The weight image ``pack`` makes of this layer's weight on the device; packed on first use."""
        if key not in self._packed:
            self._packed[key] = pack(self._w_cpu, *args)
        return self._packed[key]

    def packed(self, split: bool = False) -> Tensor:
        return self._cached(split, pack_conv_weight, self._device, split)

    def packed_mix8(self) -> Tuple[Tensor, int]:
        return self._cached("mix8", pack_conv_weight_mix8, self._device)

    def packed_upfold(self, c_skip: int, split: bool = False) -> Tensor:
        return self._cached(("upfold", c_skip, split), pack_conv_weight_upfold, c_skip, self._device, split)

    def packed_upfold_mix8(self, c_skip: int) -> Tuple[Tensor, int]:
        return self._cached(("upfold_mix8", c_skip), pack_conv_weight_upfold_mix8, c_skip, self._device)


class ConvProfile:
    """HIP-event timing of every 3x3x3 MFMA conv launch (the dominant kernel), recorded on
    the stream the kernels are launched on; bench.py turns it into the roofline figure."""

    def __init__(self):
        self.events = []  # (start, end, flops, layer name): flops = the ALGORITHMIC count 2*Cin*Cout*27 per output voxel
        self.executed_flops = 0.0  # what the launches put on the matrix pipe (plan.conv_flops)

    def named(self):
        if self.events:
            self.events[-1][1].synchronize()
        return list(self.events)

    def totals(self):
        if not self.events:
            return 0.0, 0.0, 0
        self.events[-1][1].synchronize()
        ms = sum(e[0].elapsed_time(e[1]) for e in self.events)
        return ms, sum(e[2] for e in self.events), len(self.events)


class _Run(NamedTuple):
    """What one ``forward_tiles`` call hands to its launchers."""
    image: Tensor
    origins: Sequence[Sequence[int]]
    shapes: Tuple[Tuple[int, int, int], ...]   # the tile's extents per resolution level
    mean: float
    std: float
    out_box: Optional[Tuple]
    live: Dict[str, Tensor]                    # buffer tag -> the tensor in it

    @property
    def B(self) -> int:
        return len(self.origins)


def _switch(name):
    return property(lambda self: self._switches[name], lambda self, value: self._switches.__setitem__(name, value))


class HipUNet:
    """``model.forward_tiles(image, origins, tile, mean, std) -> (B, 5, w, h, d)`` fp16."""

    # The precision and the tools/ A/B switches.  They live in one dict that the stream contexts of ``clone_context``
    # share with their model, so a context can not run another plan than its model.
    #   defer_activation: single-consumer tensors stay RAW and are activated on load
    #   fold_upsample:    decoder convs: nearest-upsample folded into the weights (sk_conv3d_upfold)
    #   box_store:        with an out_box the last conv stores only the box the heads read (sk_conv3d_box)
    #   stem_single_pass: stem conv once (raw + statistics), enc0.1 activates it in LDS (fp16 mode)
    precision, defer_activation, fold_upsample, box_store, stem_single_pass = (_switch(n) for n in SWITCHES)

    def __init__(self, state_dict: Dict[str, Tensor], device="cuda:0",
                 dims: Sequence[int] = (32, 64, 128, 64, 32),
                 depths: Sequence[int] = (2, 2, 2, 2, 2), precision: str = "fp16"):
        """``precision``: "fp16" (fast path: fp16 MFMA operands, fp32 accumulation -- what the reference's fp16
        autocast does, eval.py:142; max-abs ~5e-3 against an fp32 forward), "split" (activations and weights as
        fp16 hi + lo pairs, three fp16 MFMAs per product: max-abs <= 1e-3 against fp32, BASELINE.json's tolerance,
        at ~1/3 of the fast path's speed), "mix8" ("split" whose 32 -> 32 3x3x3 convs -- enc0.1.., dec0.1.. -- take their two
        correction products w_lo x and w x_lo as one block-scaled fp8 matrix product, sk_conv3d_mix8: the corrections are
        2^-11 of the result, so e4m3's 2^-4 keeps them to ~2^-15; every other layer as "split") or "fp32" (every layer on
        the exact-fp32 matrix instruction; the parity reference of the others, ~1/11 of the fast path's speed)."""
        self.dims, self.depths = tuple(dims), tuple(depths)
        plan_forward(self.dims, self.depths, precision)   # raises for a precision or widths the kernels are not built for
        self._switches = dict(zip(SWITCHES, (precision, True, True, True, False)))
        self.device = dev = torch.device(device)
        sd = state_dict
        blocks = network_blocks(self.dims, self.depths)
        self.layers = {b.name: _ConvLayer(b.name, sd, dev, b.ksize) for b in blocks}
        for b in blocks:
            assert (self.layers[b.name].cin, self.layers[b.name].cout) == (b.cin, b.cout), (b.name, b.cin, b.cout)
        if self.layers["enc0.0"].cin != 1:
            raise ValueError("the stem kernel is built for IN_CHANNELS == 1")
        self.head_w5 = sd["heads.weight"].detach().float().to(dev).contiguous()  # (5, C, 1, 1, 1)
        self.head_w = sd["heads.weight"].detach().float().reshape(5, self.dims[4]).to(dev).contiguous()
        self.head_b = sd["heads.bias"].detach().float().to(dev).contiguous()
        self.zeros = torch.zeros(4096, dtype=torch.uint8, device=dev)
        self._bufs: Dict[Tuple, Tensor] = {}
        self.last_features: Dict[str, Tensor] = {}
        self.profile: Optional[ConvProfile] = None

    def clone_context(self) -> "HipUNet":
        """Same weights and switches, separate activation buffers: lets two tile batches be in flight on two
        HIP streams (the HBM-bound GN/heads kernels of one overlap the MFMA-bound convs of the other)."""
        import copy
        other = copy.copy(self)
        other._bufs = {}
        other.last_features = {}
        other.profile = None
        other.__dict__.pop("_stream_ctxs", None)   # the primary's list of contexts (parallel.ShardedVolume.run) is not the clone's
        return other

    # -- reference-compatible construction ---------------------------------------------
    @classmethod
    def from_module(cls, module: torch.nn.Module, device="cuda:0", precision: str = "fp16") -> "HipUNet":
        return cls(module.state_dict(), device, getattr(module, "dims", (32, 64, 128, 64, 32)),
                   getattr(module, "depths", (2, 2, 2, 2, 2)), precision)

    # -- buffers -----------------------------------------------------------------------
    def _buf(self, tag: str, shape: Tuple[int, ...], dtype=torch.float16) -> Tensor:
        """Activation / scratch buffer ``tag``: ONE allocation per tag that only ever grows; a smaller request (the last
        tile batch of a volume -- 49 of 64 tiles at 1024x1024x256 --, another layer's partial sums) is a view of it.
        Rounds 1-3 re-allocated a tag whenever its shape changed: every step freed and re-requested tens of GB through
        torch's caching allocator, whose blocks had meanwhile been split for other tags -- the first steps after a
        precision switch then called hipMalloc inside the step (2 calls, ~480 ms on some boxes: what made the
        split-precision figure of the driver's line read 170 where the steady state is 215 Mvox/s)."""
        n = 1
        for v in shape:
            n *= int(v)
        key = (tag, dtype)
        t = self._bufs.get(key)
        if t is None or t.numel() < n:
            self._bufs.pop(key, None)
            t = None   # release the old block before asking for the larger one
            t = torch.empty(n, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t[:n].view(shape)

    # -- launchers: one per kernel family, each runs one step of the plan ---------------
    def _affine(self, name: str, B: int, c: int) -> Tensor:
        """Where the GroupNorm affine of block ``name`` lies: its readers apply it to the block's RAW output."""
        return self._buf("affine_" + name, (B, 2, c), torch.float32)

    def _output(self, step, run: _Run) -> Tensor:
        return self._buf(step.tag, (run.B, *run.shapes[step.level], step.cout * step.lanes))

    def _norm_act(self, step, x: Tensor, partial: Tensor, nblk: int) -> None:
        """GroupNorm statistics -> per-channel affine, then the step's fused affine + SiLU pass in place, if it has
        one: without it the tensor stays RAW and its (single) consumer applies the affine on load."""
        layer, B = self.layers[step.name], x.shape[0]
        vox = x.shape[1] * x.shape[2] * x.shape[3]
        aff = self._affine(step.name, B, step.cout)
        st = _ffi.stream_ptr(self.device)
        _ffi.check(_ffi.lib.sk_groupnorm_finalize(_ffi.ptr(partial), B, nblk, GN_GROUPS, step.cout, vox,
                                                  _ffi.ptr(layer.gamma), _ffi.ptr(layer.beta), GN_EPS,
                                                  _ffi.ptr(aff), st))
        if step.norm_pass is not None:
            _ffi.check(_kernel("norm", step.norm_pass)(_ffi.ptr(x), _ffi.ptr(aff), B, vox, step.cout, st))

    def _partial(self, step, B: int, nblk: int) -> Tensor:
        """The GroupNorm partial sums of the step's launch: one row per workgroup."""
        return self._buf("partial", (B * nblk * (step.cout // 4) * 2,), torch.float32)

    def _run_conv(self, step, run: _Run) -> Tensor:
        """CONV, DOWN, CONV_BOX, MIX8: the kernels that take an array of sources; UPFOLD, UPFOLD_MIX8: skip and
        upsampled source as two arguments, and a workgroup count (hence a number of partial-sum rows) of their own."""
        layer, B, (ox, oy, oz) = self.layers[step.name], run.B, run.shapes[step.level]
        out = self._output(step, run)
        arr = (_ffi.ConvSrc * len(step.srcs))()
        for a, s in zip(arr, step.srcs):
            a.data, a.c, a.upsample = run.live[s.tag].data_ptr(), s.c, s.up
            a.affine = self._affine(s.name, B, s.c).data_ptr() if s.form is Form.RAW else None
        folded = step.kernel in (Kernel.UPFOLD, Kernel.UPFOLD_MIX8)
        nblk = (_ffi.lib.sk_conv3d_upfold_num_blocks(ox, oy, oz, step.cout) if folded else
                _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, step.cout, step.ksize))
        if nblk <= 0:
            raise ValueError(f"{step.name}: unsupported output shape {(ox, oy, oz)}")
        partial = self._partial(step, B, nblk)
        timed = self.profile is not None and step.ksize == 3
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        split = step.store is Form.SPLIT
        if step.kernel in (Kernel.MIX8, Kernel.UPFOLD_MIX8):   # weight image + its fp8 scale exponent; C -> C 3x3x3 only
            wimg, wexp = layer.packed_mix8() if not folded else layer.packed_upfold_mix8(step.srcs[0].c)
            weight, ksize = (_ffi.ptr(wimg), wexp), ()
        else:
            weight = (_ffi.ptr(layer.packed_upfold(step.srcs[0].c, split) if folded else layer.packed(split)),)
            ksize = (step.ksize,)
        dst = (_ffi.ptr(layer.bias), _ffi.ptr(out), B, ox, oy, oz, step.cout)
        if folded:
            args = (arr[0].data, arr[0].c, arr[1].data, arr[1].c, *weight, *dst, _ffi.ptr(partial))
        else:
            box = (_box6(*run.out_box) if step.box else None,) if step.kernel in (Kernel.MIX8, Kernel.CONV_BOX) else ()
            args = (arr, len(arr), *weight, *dst, *ksize, _ffi.ptr(partial), _ffi.ptr(self.zeros), *box)
        _ffi.check(_kernel(step.kernel, step.store)(*args, _ffi.stream_ptr(self.device)))
        if timed:
            e1.record(torch.cuda.current_stream(self.device))
            algorithmic, executed, passes = conv_flops(step)
            self.profile.events.append((e0, e1, algorithmic * B * ox * oy * oz, step.name))
            self.profile.executed_flops += executed * B * ox * oy * oz * passes
        self._norm_act(step, out, partial, nblk)
        return out

    def _run_down_act(self, step, run: _Run) -> Tensor:
        """Stride-2 down conv of the RAW output of the previous block: the kernel activates it while staging it
        (GroupNorm affine + SiLU in LDS) and writes the activated values back -- the tensor is activated afterwards,
        in the form the decoder's skip conv reads -- which saves the separate in-place GroupNorm pass over the skip tensor."""
        layer, B, (ox, oy, oz), src = self.layers[step.name], run.B, run.shapes[step.level], step.srcs[0]
        out = self._output(step, run)
        nblk = _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, step.cout, 2)
        partial = self._partial(step, B, nblk)
        _ffi.check(_kernel(Kernel.DOWN_ACT, step.writeback)(
            _ffi.ptr(run.live[src.tag]), _ffi.ptr(self._affine(src.name, B, src.c)),
            _ffi.ptr(layer.packed(step.store is Form.SPLIT)), _ffi.ptr(layer.bias), _ffi.ptr(out), B, ox, oy, oz,
            src.c, step.cout, _ffi.ptr(partial), _ffi.ptr(self.zeros), _ffi.stream_ptr(self.device)))
        self._norm_act(step, out, partial, nblk)
        return out

    def _run_stem(self, step, run: _Run) -> Tensor:
        """First block (Cin = 1).  STEM: normalise + conv statistics, GroupNorm finalize, then the conv again with the
        affine + SiLU fused into its epilogue: the raw tensor is never written.  STEM_RAW: one pass that writes the
        raw result and its statistics; the consumer activates."""
        layer, B, (xt, yt, zt) = self.layers[step.name], run.B, run.shapes[0]
        X, Y, Z = run.image.shape
        out = self._output(step, run)
        nblk = _ffi.lib.sk_conv3d_stem_num_blocks(xt, yt, zt)
        partial = self._partial(step, B, nblk)
        org = (C.c_int32 * (3 * B))(*[int(v) for o in run.origins for v in o])
        ws_bytes = _ffi.lib.sk_conv3d_stem_workspace_bytes(B, xt, yt, zt)
        ws = self._buf("stem_ws", (ws_bytes,), torch.uint8)
        st = _ffi.stream_ptr(self.device)
        head = (_ffi.ptr(run.image), X, Y, Z, org, B, xt, yt, zt, run.mean, run.std,
                _ffi.ptr(layer.packed()), _ffi.ptr(layer.bias), step.cout)
        if step.kernel is Kernel.STEM_RAW:
            _ffi.check(_ffi.lib.sk_conv3d_stem_raw(*head, _ffi.ptr(out), _ffi.ptr(partial), _ffi.ptr(ws), ws_bytes, st))
            self._norm_act(step, out, partial, nblk)
            return out
        _ffi.check(_ffi.lib.sk_conv3d_stem(*head, _ffi.ptr(partial), _ffi.ptr(ws), ws_bytes, st))
        self._norm_act(step, out, partial, nblk)
        _ffi.check(_kernel("stem apply", step.out)(B, xt, yt, zt, _ffi.ptr(layer.packed()), _ffi.ptr(layer.bias),
                                                   _ffi.ptr(self._affine(step.name, B, step.cout)), _ffi.ptr(out),
                                                   step.cout, _ffi.ptr(ws), st))
        return out

    def _run_heads(self, step, run: _Run) -> Tensor:
        B, (xt, yt, zt), src = run.B, run.shapes[0], step.srcs[0]
        out5 = self._buf("out5", (B, 5, xt, yt, zt))
        i3 = C.c_int32 * 3
        blo, bhi = (i3(*[int(v) for v in b]) for b in run.out_box) if run.out_box is not None else (None, None)
        aff = self._affine(src.name, B, src.c) if src.form is Form.RAW else None
        _ffi.check(_kernel(Kernel.HEADS, step.store)(
            _ffi.ptr(run.live[src.tag]), _ffi.ptr(aff), _ffi.ptr(self.head_w), _ffi.ptr(self.head_b),
            _ffi.ptr(out5), B, xt, yt, zt, src.c, blo, bhi, _ffi.stream_ptr(self.device)))
        return out5

    def _run_f32(self, step, run: _Run) -> Tensor:
        """Precision "fp32": sk_conv3d_f32 on fresh fp32 tensors, then GroupNorm + SiLU -- or, for the heads, tanh / sigmoid."""
        heads = step.kernel is Kernel.HEADS_F32
        layer, B, (ox, oy, oz), cout = self.layers.get(step.name), run.B, run.shapes[step.level], step.cout
        if step.srcs[0].name == "image":
            xt, yt, zt = run.shapes[0]

            def crop(x, y, z):  # normalise (eval.py:139, fp16 arithmetic), then zero-pad an overhanging tile
                c = run.image[x:x + xt, y:y + yt, z:z + zt].sub(run.mean).div(run.std).float()
                return torch.nn.functional.pad(c, (0, zt - c.shape[2], 0, yt - c.shape[1], 0, xt - c.shape[0]))

            run.live["image"] = torch.stack([crop(x, y, z) for (x, y, z) in run.origins]).unsqueeze(-1).contiguous()
        out = torch.empty((B, ox, oy, oz, cout), dtype=torch.float32, device=self.device)
        nblk = _ffi.lib.sk_conv3d_f32_num_blocks(ox, oy, oz)
        partial = None if heads else torch.empty((B, nblk, cout // 4, 2), dtype=torch.float32, device=self.device)
        arr = (_ffi.ConvSrc * len(step.srcs))()
        for a, s in zip(arr, step.srcs):
            a.data, a.affine, a.c, a.upsample = run.live[s.tag].data_ptr(), None, s.c, s.up
        st = _ffi.stream_ptr(self.device)
        _ffi.check(_ffi.lib.sk_conv3d_f32(arr, len(arr), _ffi.ptr(self.head_w5 if heads else layer.weight_f32),
                                          _ffi.ptr(self.head_b if heads else layer.bias), _ffi.ptr(out), B,
                                          ox, oy, oz, cout, step.ksize, _ffi.ptr(partial), st))
        if heads:
            y = out.permute(0, 4, 1, 2, 3)
            return torch.cat([torch.tanh(y[:, 0:3]), torch.sigmoid(y[:, 3:5])], dim=1).contiguous()
        aff = torch.empty((B, 2, cout), dtype=torch.float32, device=self.device)
        vox = ox * oy * oz
        _ffi.check(_ffi.lib.sk_groupnorm_finalize(_ffi.ptr(partial), B, nblk, GN_GROUPS, cout, vox,
                                                  _ffi.ptr(layer.gamma), _ffi.ptr(layer.beta), GN_EPS,
                                                  _ffi.ptr(aff), st))
        _ffi.check(_kernel("norm", Form.F32)(_ffi.ptr(out), _ffi.ptr(aff), B, vox, cout, st))
        return out

    _LAUNCH = {Kernel.STEM: _run_stem, Kernel.STEM_RAW: _run_stem, Kernel.CONV: _run_conv, Kernel.DOWN: _run_conv,
               Kernel.CONV_BOX: _run_conv, Kernel.MIX8: _run_conv, Kernel.UPFOLD: _run_conv, Kernel.UPFOLD_MIX8: _run_conv,
               Kernel.DOWN_ACT: _run_down_act, Kernel.HEADS: _run_heads, Kernel.F32: _run_f32, Kernel.HEADS_F32: _run_f32}

    # -- forward -----------------------------------------------------------------------
    def forward_tiles(self, image: Tensor, origins: Sequence[Sequence[int]], tile: Sequence[int],
                      mean: float, std: float, keep_features: bool = False, out_box=None) -> Tensor:
        """image (X, Y, Z) fp16 on the GPU; B tile origins; tile extents (w, h, d).
        ``out_box`` = (lo, hi) tile-local: only that box of the 5-channel output is evaluated (every
        conv still covers the whole tile -- its GroupNorm statistics need it -- but the heads do not).
        The result is a view of this context's output buffer: valid until the next ``forward_tiles`` call on it."""
        _ffi.require_gpu(image, "image")
        if image.dtype != torch.float16 or image.ndim != 3:
            raise ValueError("image must be an (X, Y, Z) fp16 tensor")
        ext = tuple(int(v) for v in tile)
        # The network runs on extents padded up to a multiple of 4 (two stride-2 levels) with zeros in
        # normalised space -- exactly what oracle/unet_spec.py defines for such a crop -- and the output
        # is cropped back: a volume thinner than the 300x300x20 tile gives tiles of its own extent
        # (cropper.py:58-144), which need not be a multiple of 4.
        xt, yt, zt = ((v + 3) // 4 * 4 for v in ext)
        if (xt, yt, zt) != ext:
            if keep_features:
                raise ValueError("keep_features needs tile extents that are multiples of 4")
            full = self.forward_tiles(image, origins, (xt, yt, zt), mean, std, out_box=out_box)
            return full[:, :, :ext[0], :ext[1], :ext[2]]
        shapes = tuple((xt >> l, yt >> l, zt >> l) for l in range(3))
        covers = tuple(_ffi.lib.sk_conv3d_upfold_num_blocks(*shapes[l], self.dims[4 - l]) > 0 for l in (0, 1))
        plan = plan_forward(self.dims, self.depths, *(self._switches[n] for n in SWITCHES),
                            bool(keep_features), out_box is not None, covers)   # cached on its arguments
        run = _Run(image, origins, shapes, float(mean), float(std), out_box, {"image": image})
        feats = {}
        for step in plan:
            out = run.live[step.tag] = self._LAUNCH[step.kernel](self, step, run)
            if step.keep:
                feats[step.name] = out.clone()
        if plan[0].kernel is not Kernel.F32:   # the fp32 mode keeps no features and leaves the last ones alone
            self.last_features = feats
        return run.live["out5"]

    def flops_per_tile_voxel(self) -> float:
        """Algorithmic conv FLOPs per full-resolution tile voxel (2*Cin*Cout*k^3 / downsampling)."""
        blocks = network_blocks(self.dims, self.depths)
        return sum(2.0 * b.cin * b.cout * b.ksize ** 3 / 8 ** b.level for b in blocks) + 2.0 * self.dims[4] * 5


# what this build's network implements of the reference's MODEL config (skoots/config.py:20-34)
SUPPORTED_ARCHITECTURE = "skoots_amd_unet"   # oracle/unet_spec.py; NOT bism's "bism_unext" / "bism_unet" (absent package)


def cfg_to_model(cfg, device="cuda:0", state_dict: Optional[Dict[str, Tensor]] = None,
                 precision: str = "fp16") -> HipUNet:
    """Counterpart of ``cfg_to_bism_model`` (skoots/lib/utils.py:17-107): reads the same
    ``cfg.MODEL`` keys from an attribute/dict config.  The network body is the build's own U-Net
    (oracle/unet_spec.py: Conv3d k=3 -> GroupNorm(8) -> SiLU blocks): a config that asks for anything else --
    the reference's default ``bism_unext`` with LayerNorm / GELU / 7^3 depthwise kernels, whose code lives in
    the absent ``bism`` package -- raises instead of silently running a different network.  Checkpoints written
    by the reference's trainer (pickled yacs ``CfgNode`` + bism ``UNeXT_3D`` keys) are therefore NOT loadable;
    checkpoints written by ``skoots_amd.train`` are."""
    model = cfg["MODEL"] if isinstance(cfg, dict) else cfg.MODEL
    get = (lambda k, d: model.get(k, d)) if isinstance(model, dict) else (lambda k, d: getattr(model, k, d))
    dims, depths = get("DIMS", [32, 64, 128, 64, 32]), get("DEPTHS", [2, 2, 2, 2, 2])
    if get("IN_CHANNELS", 1) != 1:
        raise RuntimeError("IN_CHANNELS must be 1")
    for key, ok in (("ARCHITECTURE", (SUPPORTED_ARCHITECTURE,)), ("NORMALIZATION", ("groupnorm",)),
                    ("ACTIVATION", ("silu",)), ("KERNEL_SIZE", (3,))):
        v = get(key, ok[0])
        if v not in ok:
            raise RuntimeError(f"MODEL.{key}={v!r} is not implemented by skoots_amd (supported: {ok}); "
                               "bism architectures need the bism package, which this build does not reimplement")
    if state_dict is None:
        raise RuntimeError("a model_state_dict is required (random init lives in oracle/unet_spec.py)")
    return HipUNet(state_dict, device, dims, depths, precision)


def random_state_dict(dims=(32, 64, 128, 64, 32), depths=(2, 2, 2, 2, 2), seed: int = 101196) -> Dict[str, Tensor]:
    """Deterministic random-init parameters under the module's key names (seed: train/engine.py:53);
    what a from-scratch training run starts from and what smoke() / the benches run on."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, Tensor] = {}

    def conv(name, cin, cout, k):
        fan = cin * k ** 3
        sd[name + ".conv.weight"] = (torch.rand((cout, cin, k, k, k), generator=g) * 2 - 1) / fan ** 0.5
        sd[name + ".conv.bias"] = (torch.rand(cout, generator=g) * 2 - 1) / fan ** 0.5
        sd[name + ".norm.weight"] = torch.rand(cout, generator=g) + 0.5
        sd[name + ".norm.bias"] = torch.rand(cout, generator=g) * 0.6 - 0.3

    for b in network_blocks(dims, depths):
        conv(b.name, b.cin, b.cout, b.ksize)
    d4 = dims[4]
    sd["heads.weight"] = (torch.rand((5, d4, 1, 1, 1), generator=g) * 2 - 1) / d4 ** 0.5
    sd["heads.bias"] = (torch.rand(5, generator=g) * 2 - 1) / d4 ** 0.5
    return sd


def smoke_model(device="cuda:0") -> Optional[HipUNet]:
    """Deterministic random-init network for __graft_entry__.smoke() (built without the oracle)."""
    dims, depths = (32, 64, 128, 64, 32), (2, 2, 2, 2, 2)
    return HipUNet(random_state_dict(dims, depths), device, dims, depths)


# ----------------------------------------------------------------------------------------
# Operator-level entry points (used by the parity tests and by bench.py's conv-only leg)
# ----------------------------------------------------------------------------------------
def _pack(fn, weight: Tensor, sizes: Sequence[int], device, scaled: bool = False):
    """The library's two-call packing protocol: ask ``fn`` for the image's size, then have it packed into a host buffer
    of that size -> the image on ``device``; ``scaled``: ``fn`` also reports an fp8 scale exponent -> (image, exponent)."""
    w = weight.detach().float().cpu().contiguous().numpy()
    fpt = w.ctypes.data_as(C.POINTER(C.c_float))
    nbytes = fn(fpt, *sizes, None, *((None,) if scaled else ()))
    if nbytes < 0:
        _ffi.check(int(nbytes))
    buf = np.empty(nbytes, dtype=np.uint8)
    exp = C.c_int32(0)
    fn(fpt, *sizes, buf.ctypes.data_as(C.c_void_p), *((C.byref(exp),) if scaled else ()))
    t = torch.from_numpy(buf).to(device)
    return (t, int(exp.value)) if scaled else t


def _box6(lo, hi):
    """A store box as the kernels take it: (x0, y0, z0, x1, y1, z1)."""
    return (C.c_int32 * 6)(*[int(v) for v in lo], *[int(v) for v in hi])


def pack_conv_weight(weight: Tensor, device, split: bool = False) -> Tensor:
    """(cout, cin, k, k, k) fp32 -> MFMA A-fragment order (fp16 bytes) on the device; ``split``: the hi + lo
    fragment sets of ``sk_conv3d_split``."""
    fn = _ffi.lib.sk_conv3d_pack_weight_split_host if split else _ffi.lib.sk_conv3d_pack_weight_host
    return _pack(fn, weight, weight.shape[:3], device)


def pack_conv_weight_mix8(weight: Tensor, device) -> Tuple[Tensor, int]:
    """(C, C, 3, 3, 3) fp32, C = 32 | 64 | 128 -> (weight image of ``sk_conv3d_mix8`` on the device, its fp8 scale exponent)."""
    return _pack(_ffi.lib.sk_conv3d_pack_weight_mix8_host, weight, weight.shape[:2], device, scaled=True)


def mix8_line(hi: Tensor, x8: Tensor, lo8: Tensor) -> Tensor:
    """The mix8 voxel line from its three parts: hi (..., C) fp16, x8 and lo8 (..., C) float8_e4m3fn (the CODES are
    stored: x8 stands for 16 x, lo8 for 2^15 (x - hi)) -> (..., 2C) fp16-typed tensor
    [hi (C) | per 32-channel chunk: x8 (32 bytes) | lo8 (32 bytes)]."""
    C = hi.shape[-1]
    lead = hi.shape[:-1]
    xb = x8.contiguous().view(torch.uint8).reshape(lead + (C // 32, 1, 32))
    lb = lo8.contiguous().view(torch.uint8).reshape(lead + (C // 32, 1, 32))
    tail = torch.cat([xb, lb], dim=-2).reshape(lead + (2 * C,))
    b = torch.cat([hi.contiguous().view(torch.uint8), tail], dim=-1)
    return b.contiguous().view(torch.float16)


def mix8_of(x: Tensor) -> Tensor:
    """fp32 (..., C) -> its mix8 line (host restatement of sk_groupnorm_silu_mix8's store)."""
    hi = x.half()
    x8 = (x * 16.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    lo8 = ((x - hi.float()) * 32768.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return mix8_line(hi, x8, lo8)


def conv3d_mix8(src: Tensor, packed_weight: Tensor, scale_exp: int, bias: Tensor, out_shape: Sequence[int], zeros: Tensor,
                store_box=None, out: Optional[Tensor] = None):
    """Raw 3x3x3 C -> C conv of precision "mix8" (C = 32 | 64 | 128): src (B, x, y, z, 2C) mix8 lines -> ((B, x, y, z, 2C) split
    pair, gn_partial)."""
    _ffi.require_gpu(src, "src")
    B, dev = src.shape[0], src.device
    ch = src.shape[-1] // 2
    ox, oy, oz = (int(v) for v in out_shape)
    if out is None:
        out = torch.empty((B, ox, oy, oz, 2 * ch), dtype=torch.float16, device=dev)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, ch, 3)
    partial = torch.zeros((B, nblk, ch // 4, 2), dtype=torch.float32, device=dev)
    arr = (_ffi.ConvSrc * 1)()
    arr[0].data, arr[0].c, arr[0].upsample, arr[0].affine = src.data_ptr(), ch, 0, None
    box = _box6(store_box[:3], store_box[3:]) if store_box is not None else None
    _ffi.check(_ffi.lib.sk_conv3d_mix8(arr, 1, _ffi.ptr(packed_weight), int(scale_exp), _ffi.ptr(bias), _ffi.ptr(out), B, ox, oy, oz,
                                       ch, _ffi.ptr(partial), _ffi.ptr(zeros), box, _ffi.stream_ptr(dev)))
    return out, partial


def split_pair(x: Tensor) -> Tensor:
    """fp32 (..., C) -> the split layout (..., 2C) fp16 = [hi | lo], hi = fp16(x), lo = fp16(x - hi)."""
    hi = x.half()
    return torch.cat([hi, (x - hi.float()).half()], dim=-1).contiguous()


def join_pair(x: Tensor) -> Tensor:
    """Split layout (..., 2C) fp16 -> fp32 (..., C) = hi + lo."""
    c = x.shape[-1] // 2
    return x[..., :c].float() + x[..., c:].float()


def conv3d(srcs: List[Tuple[Tensor, int]], packed_weight: Tensor, bias: Tensor, cout: int, ksize: int,
           out_shape: Sequence[int], zeros: Tensor, want_stats: bool = True, split: bool = False):
    """Raw conv (no normalisation): srcs [(B,x,y,z,c) fp16 tensor, upsample flag] ->
    ((B, ox, oy, oz, cout) fp16, gn_partial (B, nblk, cout/4, 2) fp32 or None).  ``split``: sources and
    output are split pairs (..., 2c) (see :func:`split_pair`), weight packed with ``split=True``."""
    B = srcs[0][0].shape[0]
    dev = srcs[0][0].device
    ox, oy, oz = (int(v) for v in out_shape)
    lanes = 2 if split else 1
    out = torch.empty((B, ox, oy, oz, cout * lanes), dtype=torch.float16, device=dev)
    nblk = _ffi.lib.sk_conv3d_num_blocks(B, ox, oy, oz, cout, ksize)
    if nblk <= 0:
        raise ValueError(f"unsupported conv output shape {tuple(out_shape)}")
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=dev) if want_stats else None
    arr = (_ffi.ConvSrc * len(srcs))()
    for i, (t, up) in enumerate(srcs):
        _ffi.require_gpu(t, "src")
        arr[i].data = t.data_ptr()
        arr[i].affine = None
        arr[i].c = t.shape[-1] // lanes
        arr[i].upsample = up
    fn = _ffi.lib.sk_conv3d_split if split else _ffi.lib.sk_conv3d
    _ffi.check(fn(arr, len(srcs), _ffi.ptr(packed_weight), _ffi.ptr(bias), _ffi.ptr(out), B,
                  ox, oy, oz, cout, ksize, _ffi.ptr(partial), _ffi.ptr(zeros), _ffi.stream_ptr(dev)))
    return out, partial


def pack_conv_weight_upfold(weight: Tensor, c_skip: int, device, split: bool = False) -> Tensor:
    """Torch-layout (cout, c_skip + c_up, 3, 3, 3) fp32 weight -> the fragments of ``sk_conv3d_upfold`` (``split``:
    ``sk_conv3d_upfold_split``) on ``device``: the nearest-upsample of the last ``c_up`` input channels folded in."""
    fn = _ffi.lib.sk_conv3d_pack_weight_upfold_split_host if split else _ffi.lib.sk_conv3d_pack_weight_upfold_host
    return _pack(fn, weight, (weight.shape[0], c_skip, weight.shape[1] - c_skip), device)


def pack_conv_weight_upfold_mix8(weight: Tensor, c_skip: int, device) -> Tuple[Tensor, int]:
    """Torch-layout (cout, c_skip + c_up, 3, 3, 3) fp32 weight -> (weight image of ``sk_conv3d_upfold_mix8``, fp8 scale exponent)."""
    return _pack(_ffi.lib.sk_conv3d_pack_weight_upfold_mix8_host, weight, (weight.shape[0], c_skip, weight.shape[1] - c_skip),
                 device, scaled=True)


def conv3d_upfold_mix8(skip: Tensor, up: Tensor, packed_weight: Tensor, scale_exp: int, bias: Tensor, cout: int):
    """``conv3d_upfold`` for precision "mix8": skip / up hold mix8 lines (:func:`mix8_of`), the result is a split pair."""
    _ffi.require_gpu(skip, "skip")
    _ffi.require_gpu(up, "up")
    B, ox, oy, oz = (int(v) for v in skip.shape[:4])
    if tuple(up.shape[:4]) != (B, ox // 2, oy // 2, oz // 2):
        raise ValueError(f"up {tuple(up.shape)} is not half of skip {tuple(skip.shape)}")
    nblk = _ffi.lib.sk_conv3d_upfold_num_blocks(ox, oy, oz, cout)
    if nblk <= 0:
        raise ValueError(f"sk_conv3d_upfold does not cover the output shape {(ox, oy, oz)} / cout {cout}")
    out = torch.empty((B, ox, oy, oz, cout * 2), dtype=torch.float16, device=skip.device)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=skip.device)
    _ffi.check(_ffi.lib.sk_conv3d_upfold_mix8(_ffi.ptr(skip), skip.shape[-1] // 2, _ffi.ptr(up), up.shape[-1] // 2, _ffi.ptr(packed_weight),
                                              int(scale_exp), _ffi.ptr(bias), _ffi.ptr(out), B, ox, oy, oz, cout, _ffi.ptr(partial),
                                              _ffi.stream_ptr(skip.device)))
    return out, partial


def conv3d_upfold(skip: Tensor, up: Tensor, packed_weight: Tensor, bias: Tensor, cout: int, want_stats: bool = True,
                  split: bool = False):
    """Raw decoder conv over cat([skip, nearest-upsample(up)]) with the upsample folded into the weights:
    skip (B, x, y, z, c) fp16, up (B, x/2, y/2, z/2, c') fp16 -> ((B, x, y, z, cout) fp16, gn_partial or None).
    ``split``: the tensors are split pairs (..., 2c) (:func:`split_pair`), the weight packed with ``split=True``."""
    _ffi.require_gpu(skip, "skip")
    _ffi.require_gpu(up, "up")
    B, ox, oy, oz = (int(v) for v in skip.shape[:4])
    if tuple(up.shape[:4]) != (B, ox // 2, oy // 2, oz // 2):
        raise ValueError(f"up {tuple(up.shape)} is not half of skip {tuple(skip.shape)}")
    nblk = _ffi.lib.sk_conv3d_upfold_num_blocks(ox, oy, oz, cout)
    if nblk <= 0:
        raise ValueError(f"sk_conv3d_upfold does not cover the output shape {(ox, oy, oz)} / cout {cout}")
    lanes = 2 if split else 1
    out = torch.empty((B, ox, oy, oz, cout * lanes), dtype=torch.float16, device=skip.device)
    partial = torch.zeros((B, nblk, cout // 4, 2), dtype=torch.float32, device=skip.device) if want_stats else None
    fn = _ffi.lib.sk_conv3d_upfold_split if split else _ffi.lib.sk_conv3d_upfold
    _ffi.check(fn(_ffi.ptr(skip), skip.shape[-1] // lanes, _ffi.ptr(up), up.shape[-1] // lanes, _ffi.ptr(packed_weight),
                  _ffi.ptr(bias), _ffi.ptr(out), B, ox, oy, oz, cout, _ffi.ptr(partial), _ffi.stream_ptr(skip.device)))
    return out, partial


def groupnorm_silu_(x: Tensor, partial: Tensor, gamma: Tensor, beta: Tensor, groups: int = GN_GROUPS,
                    eps: float = GN_EPS) -> Tensor:
    """In place GroupNorm (statistics from the conv partials) + SiLU on (B, x, y, z, C) fp16."""
    B, C_ = x.shape[0], x.shape[-1]
    vox = x[0].numel() // C_
    aff = torch.empty((B, 2, C_), dtype=torch.float32, device=x.device)
    st = _ffi.stream_ptr(x.device)
    _ffi.check(_ffi.lib.sk_groupnorm_finalize(_ffi.ptr(partial), B, partial.shape[1], groups, C_, vox,
                                              _ffi.ptr(gamma), _ffi.ptr(beta), eps, _ffi.ptr(aff), st))
    _ffi.check(_ffi.lib.sk_groupnorm_silu(_ffi.ptr(x), _ffi.ptr(aff), B, vox, C_, st))
    return x
