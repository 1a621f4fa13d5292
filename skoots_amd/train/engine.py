"""One training step of the U-Net on the HIP kernels (BASELINE.json configs[4]).

Reference: the inner step of skoots/train/engine.py:456-499 --

    out = model(images)                                   # (B, 5, X, Y, Z)
    embedding = vector_to_embedding(vector_scale, out[:, 0:3])
    emb_prob  = baked_embed_to_prob(embedding, baked, sigma(e))
    loss = w_e * tversky_e(emb_prob, masks > 0) + w_p * tversky_p(out[:, [-1]], masks > 0)
         + w_s * tversky_s(out[:, [-2]], skele_masks > 0)
    loss.backward(); optimizer.step()                     # AdamW, config.py:96-101

Here the same step runs as explicit kernels of libskoots_hip.so (no autograd): the forward
keeps each block's raw conv output, GroupNorm affine and statistics; the loss and its gradient
come from one fused kernel pair; the backward walks the recorded layer list in reverse (GN+SiLU
backward, weight gradient, data gradient); AdamW updates one flat parameter buffer.  Master
parameters, GroupNorm statistics, loss and optimizer are fp32 in every precision; the convolutions
and the tensors between them are fp32 ("fp32", the parity mode) or 16-bit on the MFMA kernels
("mixed" = fp16, "bf16": the reference runs bf16 with channels_last_3d, engine.py:68,107-109).
Which way each data gradient of the backward travels is decided in routes.py, before the first
kernel.  The network graph is oracle/unet_spec.py's; data loading, augmentation, schedulers
and logging of the reference's loop are out of scope.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _ffi
from ..unet import GN_EPS, GN_GROUPS
from .routes import FAST_KINDS, GraphBlock, Kind, Route, route_gradients


class _Layer:
    """Views of one conv (+ GroupNorm) layer's parameters and gradients in the flat buffers."""

    def __init__(self, name: str, ksize: int, norm: bool):
        self.name, self.ksize, self.norm = name, ksize, norm
        self.weight = self.bias = self.gamma = self.beta = None
        self.g_weight = self.g_bias = self.g_gamma = self.g_beta = None
        self.cin = self.cout = 0


TRAIN_PRECISIONS = ("fp32", "mixed", "bf16")


class _Lib:
    """``libskoots_hip.so`` with the 16-bit entry points resolved to one build: "" = fp16, "_bf16" = the bf16 twins
    (include/skoots_hip_bf16.h).  Dtype-independent functions resolve to their plain names.

    ``profile`` (a :class:`skoots_amd.profile.KernelProfile`): HIP-event spans around every MFMA conv launch of the
    step -- forward and data-gradient convs (``sk_conv3d``) and weight gradients (``sk_train_conv_wgrad_f16``) -- with
    their algorithmic FLOPs, for bench.py's training roofline."""

    def __init__(self, suffix: str, device=None):
        self._suffix = suffix
        self._device = device
        self.profile = None

    def __getattr__(self, name: str):
        fn = getattr(_ffi.lib, name + self._suffix if (self._suffix and name in _ffi.BF16_TWINS) else name)
        if name in ("sk_conv3d", "sk_train_conv_wgrad_f16"):
            raw, kind = fn, ("conv_fwd_dgrad" if name == "sk_conv3d" else "conv_wgrad")

            def fn(srcs, n_src, *rest):
                if self.profile is None:
                    return raw(srcs, n_src, *rest)
                # sk_conv3d: (w, bias, out, B, ox, oy, oz, cout, k, ...); wgrad: (dy, scale, B, ox, oy, oz, cout, k, ...)
                B, ox, oy, oz, cout, k = rest[3:9] if name == "sk_conv3d" else rest[2:8]
                cin = sum(int(srcs[i].c) for i in range(n_src))
                with self.profile.span(kind, self._device, 2.0 * cin * cout * k ** 3 * B * ox * oy * oz):
                    return raw(srcs, n_src, *rest)
        setattr(self, name, fn)
        return fn


class _Grad16(NamedTuple):
    """A gradient held as a 16-bit tensor: ``data`` * ``scale[1]`` is the gradient (a fast block's dy; a data gradient
    on a 16-bit route).  ``complete`` is False for a Route.PENDING contribution, which the stride-2 reader's interleave
    pass still has to sum."""
    data: Tensor
    scale: Tensor
    complete: bool


@dataclass
class _Block:
    """One entry of the tape: what the forward keeps of a block for its backward."""
    kind: Kind
    layer: _Layer
    srcs: List[Tuple[Tensor, int]]   # (tensor as the caller passed it, upsampled)
    y: Tensor                        # raw conv output (16-bit for FAST / STEM; the logits for the heads)
    affine: Optional[Tensor]         # GroupNorm scale / shift per (b, c) and mean / rstd per (b, group); None without norm
    stats: Optional[Tensor]
    out: Tensor                      # what the consumers read

    def graph(self) -> GraphBlock:
        return GraphBlock(self.layer.name, self.kind, self.layer.ksize, self.layer.cout, self.out.data_ptr(),
                          tuple((t.data_ptr(), up, t.shape[-1]) for t, up in self.srcs))


class TrainUNet:
    """The U-Net of oracle/unet_spec.py with fp32 master parameters on the GPU.

    ``forward(images)`` -> logits (B, X, Y, Z, 5) (pre-tanh / pre-sigmoid head outputs) and records
    what the backward needs; ``backward(dlogits)`` fills ``flat_grad``."""

    def __init__(self, state_dict: Dict[str, Tensor], device="cuda:0",
                 dims: Sequence[int] = (32, 64, 128, 64, 32), depths: Sequence[int] = (2, 2, 2, 2, 2),
                 precision: str = "fp32", f16_grad_handoff: bool = True):
        """``f16_grad_handoff=False``: single-reader data gradients travel as fp32 copies instead of scaled 16-bit tensors
        (the hand-off is lossy by one 16-bit rounding per tensor: parameter gradients move by ~1e-4 of the largest one).

        ``precision``: "fp32" (every kernel fp32; the parity mode), "bf16" (below, on bf16 tensors and bf16 matrix
        instructions: BASELINE configs[4]'s dtype) or "mixed" (fp32 master weights, GroupNorm,
        loss and optimizer; the convolutions of the forward pass, the data gradients and the weight gradients
        on the fp16 MFMA kernels with fp32 accumulation, output gradients scaled per tensor by a power of
        two -- the counterpart of the reference's bf16 step, engine.py:68,107-109)."""
        if precision not in TRAIN_PRECISIONS:
            raise ValueError(f"precision must be one of {TRAIN_PRECISIONS}")
        self.precision = precision
        # "bf16": the mixed step on the bf16 build of the same kernels (library entry points *_bf16): bf16 storage of
        # activations / output gradients and v_mfma_*_bf16 -- the dtype the reference trains in (engine.py:68,107-109)
        self.fast16 = precision in ("mixed", "bf16")
        self.t16 = torch.bfloat16 if precision == "bf16" else torch.float16
        self._L = _Lib("_bf16" if precision == "bf16" else "", torch.device(device))
        self.device = torch.device(device)
        self.dims, self.depths = tuple(dims), tuple(depths)
        self.f16_grad_handoff = bool(f16_grad_handoff)   # single-reader fp16 data gradients handed on without an fp32 copy
        # tests only: a list here makes backward() record, per fast block, copies of exactly the 16-bit tensors its kernels
        # read and wrote (sources, raw output, incoming gradient, dy, data gradients, scales) next to the parameter
        # gradients they produced, so that every kernel of the step can be replayed in torch ON THE SAME OPERANDS
        # (tests/test_hip_train.py: test_bf16_step_kernels_replayed_in_situ)
        self.audit: Optional[list] = None

        def stack(name, n):
            return [_Layer(f"{name}.{i}", 3, True) for i in range(n)]

        self.enc0 = stack("enc0", depths[0])
        self.down0 = _Layer("down0", 2, True)
        self.enc1 = stack("enc1", depths[1])
        self.down1 = _Layer("down1", 2, True)
        self.mid = stack("mid", depths[2])
        self.red1 = _Layer("red1", 1, True)
        self.dec1 = stack("dec1", depths[3])
        self.red0 = _Layer("red0", 1, True)
        self.dec0 = stack("dec0", depths[4])
        self.heads = _Layer("heads", 1, False)
        self.layers: List[_Layer] = (self.enc0 + [self.down0] + self.enc1 + [self.down1] + self.mid + [self.red1] +
                                     self.dec1 + [self.red0] + self.dec0 + [self.heads])
        # flat parameter / gradient buffers, state_dict key order of the module
        self.param_names: List[str] = []
        shapes = []
        for l in self.layers:
            keys = ([f"{l.name}.conv.weight", f"{l.name}.conv.bias", f"{l.name}.norm.weight", f"{l.name}.norm.bias"]
                    if l.norm else [f"{l.name}.weight", f"{l.name}.bias"])
            for k in keys:
                if k not in state_dict:
                    raise KeyError(f"state_dict lacks {k}")
                self.param_names.append(k)
                shapes.append(tuple(state_dict[k].shape))
        total = sum(math.prod(s) for s in shapes)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._views: Dict[str, Tuple[Tensor, Tensor]] = {}
        off = 0
        for k, s in zip(self.param_names, shapes):
            n = math.prod(s)
            p = self.flat_param[off:off + n].view(s)
            p.copy_(state_dict[k].detach().float())
            self._views[k] = (p, self.flat_grad[off:off + n].view(s))
            off += n
        for l in self.layers:
            if l.norm:
                (l.weight, l.g_weight), (l.bias, l.g_bias) = self._views[f"{l.name}.conv.weight"], self._views[f"{l.name}.conv.bias"]
                (l.gamma, l.g_gamma), (l.beta, l.g_beta) = self._views[f"{l.name}.norm.weight"], self._views[f"{l.name}.norm.bias"]
            else:
                (l.weight, l.g_weight), (l.bias, l.g_bias) = self._views[f"{l.name}.weight"], self._views[f"{l.name}.bias"]
            l.cout, l.cin = int(l.weight.shape[0]), int(l.weight.shape[1])
            if tuple(l.weight.shape[2:]) != (l.ksize,) * 3:
                raise ValueError(f"{l.name}: weight shape {tuple(l.weight.shape)} does not fit ksize {l.ksize}")
        self._tape: List[_Block] = []
        self._ws: Optional[Tensor] = None
        self._half: Dict[int, Tensor] = {}   # data_ptr of an fp32 activation -> its fp16 twin (mixed mode)
        self._keep: List[Tensor] = []        # buffers of the forward that must outlive their launch (see the stem)
        self._zero_page = torch.zeros(4096, dtype=torch.uint8, device=self.device)
        self._zero_bias = torch.zeros(128, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Tensor]:
        """Parameters under the module's key names (what a checkpoint's ``model_state_dict`` holds)."""
        return {k: self._views[k][0].detach().clone() for k in self.param_names}

    def grads(self) -> Dict[str, Tensor]:
        return {k: self._views[k][1] for k in self.param_names}

    def _workspace(self, floats: int) -> Tensor:
        if self._ws is None or self._ws.numel() < floats:
            self._ws = torch.empty(int(floats), dtype=torch.float32, device=self.device)
        return self._ws

    def _run(self, name: str, *args) -> None:
        """One entry point of the library on the stream of the running pass: tensors go as their data pointers (None as
        a null pointer), the stream goes last, a non-zero status raises."""
        _ffi.check(getattr(self._L, name)(*[a.data_ptr() if isinstance(a, Tensor) else a for a in args], self._st))

    @staticmethod
    def _srcs(srcs) -> "C.Array":
        arr = (_ffi.ConvSrc * len(srcs))()
        for i, (t, up) in enumerate(srcs):
            arr[i].data = t.data_ptr()
            arr[i].affine = None
            arr[i].c = t.shape[-1]
            arr[i].upsample = up
        return arr

    # ------------------------------------------------------------------------------
    # -- mixed precision helpers ------------------------------------------------------------
    def _fast(self, layer: _Layer, srcs) -> bool:
        """The fp16 MFMA kernels take this layer: GroupNorm block, widths 32/64/128, channel counts % 32."""
        return (self.fast16 and layer.norm and layer.cout in (32, 64, 128) and
                all(t.shape[-1] % 32 == 0 for t, _ in srcs))

    def _pack(self, layer: _Layer, transposed: int = 0, c_lo: int = 0, c_n: Optional[int] = None) -> Tensor:
        c_n = layer.cin if c_n is None else c_n
        cout_eff, cin_eff = (c_n, layer.cout) if transposed else (layer.cout, layer.cin)
        buf = torch.empty(layer.ksize ** 3 * (cin_eff // 16) * (cout_eff // 32) * 1024, dtype=torch.uint8, device=self.device)
        self._run("sk_train_pack_weight", layer.weight, layer.cout, layer.cin, layer.ksize, int(transposed), c_lo, c_n, buf)
        return buf

    def _to_half(self, t: Tensor, scale: Optional[Tensor] = None) -> Tensor:
        h = torch.empty(t.shape, dtype=self.t16, device=self.device)
        self._run("sk_train_cast_f32_f16", t, h, t.numel(), scale)
        return h

    def _fast_conv(self, srcs16: List[Tuple[Tensor, int]], packed: Tensor, bias: Tensor, out_shape, cout: int, ksize: int,
                   partial: Optional[Tensor]) -> Tensor:
        B = srcs16[0][0].shape[0]
        ox, oy, oz = out_shape
        y16 = torch.empty((B, ox, oy, oz, cout), dtype=self.t16, device=self.device)
        self._run("sk_conv3d", self._srcs(srcs16), len(srcs16), packed, bias, y16, B, ox, oy, oz, cout, ksize, partial,
                  self._zero_page)
        return y16

    def _h(self, t: Tensor) -> Tensor:
        """fp16 form of an activation: itself, or the registered twin of an fp32 tensor."""
        return t if t.dtype == self.t16 else self._half[t.data_ptr()]

    # -- forward blocks -------------------------------------------------------------------------
    def _norm_tail(self, kind: Kind, layer: _Layer, srcs, y: Tensor, partial: Tensor, nblk: int,
                   want32: bool = False) -> Tensor:
        """The second half of every GroupNorm block: statistics from the conv's partial sums, SiLU(GroupNorm(y)) in
        y's precision, and the tape entry.  ``want32``: a 16-bit block also writes an fp32 activation and hands that
        on (its consumer is an fp32 kernel, i.e. the heads); the 16-bit one stays registered as its twin."""
        B, ox, oy, oz, cout = y.shape
        vox = ox * oy * oz
        affine = torch.empty((B, 2, cout), dtype=torch.float32, device=self.device)
        stats = torch.empty((B, GN_GROUPS, 2), dtype=torch.float32, device=self.device)
        self._run("sk_groupnorm_finalize_stats", partial, B, nblk, GN_GROUPS, cout, vox, layer.gamma, layer.beta, GN_EPS,
                  affine, stats)
        out = torch.empty_like(y)
        if kind is Kind.FP32:
            self._run("sk_train_gn_silu", y, affine, out, B, vox, cout)
        else:
            z16 = out
            z32 = torch.empty(y.shape, dtype=torch.float32, device=self.device) if want32 else None
            self._run("sk_train_gn_silu_f16", y, affine, z16, z32, B, vox, cout)
            if want32:
                self._half[z32.data_ptr()] = z16
                out = z32
        self._tape.append(_Block(kind, layer, srcs, y, affine, stats, out))
        return out

    def _block_mixed(self, layer: _Layer, srcs: List[Tuple[Tensor, int]], out_shape: Tuple[int, int, int],
                     want32: bool = False) -> Tensor:
        """Fast block: keeps the RAW fp16 conv output for the backward and hands the fp16 activation on."""
        B = srcs[0][0].shape[0]
        ox, oy, oz = out_shape
        srcs16 = [(self._h(t), up) for t, up in srcs]
        nblk = self._L.sk_conv3d_num_blocks(B, ox, oy, oz, layer.cout, layer.ksize)
        partial = torch.empty((B, nblk, layer.cout // 4, 2), dtype=torch.float32, device=self.device)
        y16 = self._fast_conv(srcs16, self._pack(layer), layer.bias, out_shape, layer.cout, layer.ksize, partial)
        return self._norm_tail(Kind.FAST, layer, srcs, y16, partial, nblk, want32)

    def _stem_fast(self, layer: _Layer, srcs, out_shape) -> bool:
        """The stem (Cin = 1, 27 taps, Cout 32) as a fast block: fp16 image operand, exact weights (hi + lo split)."""
        B = srcs[0][0].shape[0]
        return (self.fast16 and layer.norm and layer.cin == 1 and layer.cout == 32 and layer.ksize == 3 and
                len(srcs) == 1 and B <= 32 and out_shape[2] % 2 == 0)

    def _block_stem_mixed(self, layer: _Layer, srcs, out_shape) -> Tensor:
        image = srcs[0][0]                       # (B, X, Y, Z, 1) fp32
        B = image.shape[0]
        X, Y, Z = out_shape
        nblk = self._L.sk_conv3d_stem_num_blocks(X, Y, Z)
        partial = torch.empty((B, nblk, 8, 2), dtype=torch.float32, device=self.device)
        wsb = int(self._L.sk_conv3d_stem_workspace_bytes(B, X, Y, Z))
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
        w_t = layer.weight.reshape(32, 27).t().contiguous()   # (27, 32) tap-major, the stem kernel's layout
        y16 = torch.empty((B, X, Y, Z, 32), dtype=self.t16, device=self.device)
        self._run("sk_train_stem_fwd_f16", image, B, X, Y, Z, w_t, layer.bias, y16, partial, ws, wsb)
        self._keep += [ws, w_t]   # alive until the stream has consumed them
        return self._norm_tail(Kind.STEM, layer, srcs, y16, partial, nblk)

    def _heads_fast(self, layer: _Layer) -> bool:
        return self.fast16 and not layer.norm and layer.ksize == 1 and layer.cout == 5 and layer.cin == 32

    def _block_heads_mixed(self, layer: _Layer, srcs, out_shape) -> Tensor:
        """1x1x1 heads straight on the fp16 activation (an HBM stream: no fp32 copy of the last feature map)."""
        z16 = srcs[0][0]
        B = z16.shape[0]
        ox, oy, oz = out_shape
        logits = torch.empty((B, ox, oy, oz, 5), dtype=torch.float32, device=self.device)
        self._run("sk_train_heads_fwd_f16", z16, layer.weight, layer.bias, logits, B * ox * oy * oz)
        self._tape.append(_Block(Kind.HEADS16, layer, srcs, logits, None, None, logits))
        return logits

    def _block(self, layer: _Layer, srcs: List[Tuple[Tensor, int]], out_shape: Tuple[int, int, int],
               want32: bool = False) -> Tensor:
        if self._stem_fast(layer, srcs, out_shape):
            return self._block_stem_mixed(layer, srcs, out_shape)
        if self._heads_fast(layer) and srcs[0][0].dtype == self.t16:
            return self._block_heads_mixed(layer, srcs, out_shape)
        if self._fast(layer, srcs):
            return self._block_mixed(layer, srcs, out_shape, want32)
        z = self._block_fp32(layer, srcs, out_shape)
        if self.fast16 and layer.norm:
            self._half[z.data_ptr()] = self._to_half(z)   # the stem's output feeds a fast layer
        return z

    def _block_fp32(self, layer: _Layer, srcs: List[Tuple[Tensor, int]], out_shape: Tuple[int, int, int]) -> Tensor:
        B = srcs[0][0].shape[0]
        ox, oy, oz = out_shape
        y = torch.empty((B, ox, oy, oz, layer.cout), dtype=torch.float32, device=self.device)
        if not layer.norm:
            self._run("sk_conv3d_f32", self._srcs(srcs), len(srcs), layer.weight, layer.bias, y, B, ox, oy, oz, layer.cout,
                      layer.ksize, None)
            self._tape.append(_Block(Kind.FP32, layer, srcs, y, None, None, y))
            return y
        nblk = self._L.sk_conv3d_f32_num_blocks(ox, oy, oz)
        partial = torch.empty((B, nblk, layer.cout // 4, 2), dtype=torch.float32, device=self.device)
        self._run("sk_conv3d_f32", self._srcs(srcs), len(srcs), layer.weight, layer.bias, y, B, ox, oy, oz, layer.cout,
                  layer.ksize, partial)
        return self._norm_tail(Kind.FP32, layer, srcs, y, partial, nblk)

    def forward(self, images: Tensor) -> Tensor:
        """images: (B, 1, X, Y, Z) or (B, X, Y, Z), already normalised (the reference's loader does
        it); extents multiples of 4.  Returns the head logits (B, X, Y, Z, 5)."""
        if images.ndim == 5:
            if images.shape[1] != 1:
                raise ValueError("images must have one channel")
            images = images[:, 0]
        x = images.to(self.device, torch.float32).contiguous().unsqueeze(-1)
        _ffi.require_gpu(x, "images")
        _, X, Y, Z, _ = x.shape
        if X % 4 or Y % 4 or Z % 4:
            raise ValueError("crop extents must be multiples of 4 (two stride-2 levels)")
        L0, L1, L2 = (X, Y, Z), (X // 2, Y // 2, Z // 2), (X // 4, Y // 4, Z // 4)
        self._tape = []
        self._half = {}
        self._image = x
        self._st = _ffi.stream_ptr(self.device)
        a = x
        for l in self.enc0:
            a = self._block(l, [(a, 0)], L0)
        s0 = a
        a = self._block(self.down0, [(s0, 0)], L1)
        for l in self.enc1:
            a = self._block(l, [(a, 0)], L1)
        s1 = a
        a = self._block(self.down1, [(s1, 0)], L2)
        for l in self.mid:
            a = self._block(l, [(a, 0)], L2)
        r1 = self._block(self.red1, [(a, 0)], L2)
        for i, l in enumerate(self.dec1):
            a = self._block(l, [(s1, 0), (r1, 1)] if i == 0 else [(a, 0)], L1)
        r0 = self._block(self.red0, [(a, 0)], L1)
        for i, l in enumerate(self.dec0):
            a = self._block(l, [(s0, 0), (r0, 1)] if i == 0 else [(a, 0)], L0,
                            want32=(i == len(self.dec0) - 1 and not self._heads_fast(self.heads)))
        return self._block(self.heads, [(a, 0)], L0)

    def release(self) -> None:
        """Drop what the last forward kept for a backward (a forward that is not followed by one: validation)."""
        self._tape = []
        self._half = {}
        self._keep = []

    # -- backward -------------------------------------------------------------------------------
    def backward(self, dlogits: Tensor) -> None:
        """Walk the recorded blocks in reverse; gradients of every parameter land in ``flat_grad``.  ``grads`` maps a
        tensor's data pointer to its gradient so far: an fp32 tensor or a :class:`_Grad16`."""
        if not self._tape:
            raise RuntimeError("backward() needs a preceding forward()")
        self._st = _ffi.stream_ptr(self.device)
        routes = route_gradients([b.graph() for b in self._tape], self._image.data_ptr(), self.f16_grad_handoff)
        deliver = {Route.FP32: self._dx_fp32, Route.DIRECT: self._dx_direct, Route.PENDING: self._dx_pending,
                   Route.INTERLEAVED: self._dx_interleaved, Route.POOLED: self._dx_pooled, Route.HEADS: self._dx_heads}
        grads: Dict[int, object] = {self._tape[-1].out.data_ptr(): dlogits}
        for blk, blk_routes in zip(reversed(self._tape), reversed(routes)):
            dz = grads.pop(blk.out.data_ptr())
            dy = self._param_grads(blk, dz)
            rec = self._audit_record(blk, dz, dy)
            lo = 0   # channel offset of the source in the conv's concatenated input
            for (t, up), route in zip(blk.srcs, blk_routes):
                if route is not Route.NONE:
                    deliver[route](blk, dy, t, up, lo, grads, rec)
                lo += t.shape[-1]
        self.release()

    def _param_grads(self, blk: _Block, dz):
        """The parameter side of a block's backward: GroupNorm + SiLU backward of the incoming gradient ``dz`` (an fp32
        tensor or a complete :class:`_Grad16`), then the conv's weight and bias gradient.  Returns the gradient of the
        raw conv output for the routes: a :class:`_Grad16` from a fast block, else fp32."""
        layer, srcs, y = blk.layer, blk.srcs, blk.y
        B, ox, oy, oz, cout = y.shape
        vox = ox * oy * oz
        if blk.kind in FAST_KINDS:
            # GroupNorm + SiLU backward straight to the scaled fp16 output gradient (no fp32 dy, no max / cast passes)
            ws = self._workspace(max(self._L.sk_train_gn_bwd_f16_workspace_floats(B, vox, cout),
                                     self._L.sk_train_conv_wgrad_workspace_floats(B, ox, oy, oz, cout, layer.cin, layer.ksize)))
            scale = torch.empty(3, dtype=torch.float32, device=self.device)
            dy16 = torch.empty(y.shape, dtype=self.t16, device=self.device)
            if isinstance(dz, _Grad16):
                assert dz.complete, f"{layer.name}: route_gradients hands a pending gradient to an interleave only"
                self._run("sk_train_gn_silu_bwd_f16h", dz.data, dz.scale, y, blk.affine, blk.stats, layer.gamma, B, vox, cout,
                          GN_GROUPS, dy16, scale, layer.g_gamma, layer.g_beta, ws)
            else:
                self._run("sk_train_gn_silu_bwd_f16", dz, y, blk.affine, blk.stats, layer.gamma, B, vox, cout, GN_GROUPS,
                          dy16, scale, layer.g_gamma, layer.g_beta, ws)
            if blk.kind is Kind.STEM:   # taps as the GEMM's N, fp32 image x scaled fp16 dy
                self._run("sk_train_stem_wgrad_f16", srcs[0][0], dy16, scale, B, ox, oy, oz, layer.g_weight, layer.g_bias, ws)
            else:
                srcs16 = [(self._h(t), up) for t, up in srcs]
                self._run("sk_train_conv_wgrad_f16", self._srcs(srcs16), len(srcs16), dy16, scale, B, ox, oy, oz, cout,
                          layer.ksize, layer.g_weight, layer.g_bias, ws, self._zero_page)
            return _Grad16(dy16, scale, True)
        if layer.norm:   # in place: dz becomes dy
            ws = self._workspace(self._L.sk_train_gn_bwd_workspace_floats(B, vox, cout))
            self._run("sk_train_gn_silu_bwd", dz, y, blk.affine, blk.stats, layer.gamma, B, vox, cout, GN_GROUPS, dz,
                      layer.g_gamma, layer.g_beta, ws)
        if blk.kind is Kind.HEADS16:
            ws = self._workspace(self._L.sk_train_heads_wgrad_workspace_floats(B * vox))
            self._run("sk_train_heads_wgrad_f16", srcs[0][0], dz, layer.g_weight, layer.g_bias, B * vox, ws)
        else:
            ws = self._workspace(self._L.sk_train_conv_wgrad_workspace_floats(B, ox, oy, oz, cout, layer.cin, layer.ksize))
            self._run("sk_train_conv_wgrad", self._srcs(srcs), len(srcs), dz, B, ox, oy, oz, cout, layer.ksize,
                      layer.g_weight, layer.g_bias, ws)
        return dz

    def _audit_record(self, blk: _Block, dz, dy) -> Optional[dict]:
        """With ``audit`` on, copies of what a fast block's kernels read and wrote; the routes add their ``dx16``."""
        if self.audit is None or blk.kind not in FAST_KINDS:
            return None
        layer = blk.layer
        rec = {"name": layer.name, "ksize": layer.ksize,
               "srcs": [((self._h(t) if blk.kind is not Kind.STEM else t).clone(), up) for t, up in blk.srcs],
               "y16": blk.y.clone(), "affine": blk.affine.clone(), "stats": blk.stats.clone(),
               "dz": (dz.data.clone(), dz.scale.clone()) if isinstance(dz, _Grad16) else (dz.clone(), None),
               "dy16": dy.data.clone(), "scale": dy.scale.clone(), "g_weight": layer.g_weight.clone(),
               "g_bias": layer.g_bias.clone(), "g_gamma": layer.g_gamma.clone(), "g_beta": layer.g_beta.clone(),
               "weight": layer.weight.clone(), "bias": layer.bias.clone(), "gamma": layer.gamma.clone(),
               "beta": layer.beta.clone(), "dx16": {}}
        self.audit.append(rec)
        return rec

    # -- one method per Route: (block, its dy, source tensor, upsampled, channel offset, grads, audit record) --------
    def _acc32(self, grads, t: Tensor) -> Tuple[Tensor, int]:
        """The fp32 gradient of ``t`` and whether an earlier reader already wrote it (the kernel then accumulates)."""
        have = t.data_ptr() in grads
        if not have:
            grads[t.data_ptr()] = torch.empty(t.shape, dtype=torch.float32, device=self.device)
        return grads[t.data_ptr()], int(have)

    def _dgrad16(self, blk: _Block, dy: _Grad16, t: Tensor, lo: int, rec) -> Tensor:
        """Data gradient on the fast conv kernel: the layer's weight packed transposed + tap-flipped."""
        c = t.shape[-1]
        dx16 = self._fast_conv([(dy.data, 0)], self._pack(blk.layer, True, lo, c), self._zero_bias, blk.y.shape[1:4], c,
                               blk.layer.ksize, None)
        if rec is not None:
            rec["dx16"][lo] = dx16.clone()
        return dx16

    def _parity_products(self, blk: _Block, dy: _Grad16, c: int) -> Tensor:
        """Stride-2 data gradient: eight pointwise products W_p^T dY on the fast kernel, one per parity of the fine
        voxel; the interleave kernels place them in the fine grid."""
        B, ox, oy, oz, _ = blk.y.shape
        packed = self._pack(blk.layer, 2, 0, c)
        per = packed.numel() // 8
        t16 = torch.empty((8, B, ox, oy, oz, c), dtype=self.t16, device=self.device)
        for par in range(8):
            self._run("sk_conv3d", self._srcs([(dy.data, 0)]), 1, packed[par * per:(par + 1) * per], self._zero_bias,
                      t16[par], B, ox, oy, oz, c, 1, None, self._zero_page)
        return t16

    def _dx_fp32(self, blk, dy, t, up, lo, grads, rec) -> None:
        layer = blk.layer
        B, ox, oy, oz, cout = blk.y.shape
        c = t.shape[-1]
        if blk.kind in FAST_KINDS and layer.ksize == 2:
            dst, have = self._acc32(grads, t)
            self._run("sk_train_interleave2", self._parity_products(blk, dy, c), dst, B, ox, oy, oz, c, dy.scale, have)
        elif blk.kind in FAST_KINDS:
            dx16 = self._dgrad16(blk, dy, t, lo, rec)
            dst, have = self._acc32(grads, t)
            if up:
                self._run("sk_train_sumpool2_f16", dx16, dy.scale, dst, B, ox // 2, oy // 2, oz // 2, c)
            else:
                self._run("sk_train_cast_f16_f32", dx16, dst, t.numel(), dy.scale, have)
        elif up and layer.ksize != 2:
            fine = torch.empty((B, ox, oy, oz, c), dtype=torch.float32, device=self.device)
            self._run("sk_train_conv_dgrad", dy, layer.weight, fine, B, ox, oy, oz, cout, layer.cin, lo, c, layer.ksize, 0)
            self._run("sk_train_sumpool2", fine, self._acc32(grads, t)[0], B, ox // 2, oy // 2, oz // 2, c)
        else:
            dst, have = self._acc32(grads, t)
            c_lo, c_n = (0, layer.cin) if layer.ksize == 2 else (lo, c)   # a stride-2 conv has one source
            self._run("sk_train_conv_dgrad", dy, layer.weight, dst, B, ox, oy, oz, cout, layer.cin, c_lo, c_n, layer.ksize,
                      have)

    def _dx_direct(self, blk, dy, t, up, lo, grads, rec) -> None:
        grads[t.data_ptr()] = _Grad16(self._dgrad16(blk, dy, t, lo, rec), dy.scale, True)

    def _dx_pending(self, blk, dy, t, up, lo, grads, rec) -> None:
        grads[t.data_ptr()] = _Grad16(self._dgrad16(blk, dy, t, lo, rec), dy.scale, False)

    def _dx_interleaved(self, blk, dy, t, up, lo, grads, rec) -> None:
        B, ox, oy, oz, _ = blk.y.shape
        pend = grads.get(t.data_ptr())   # the decoder's Route.PENDING contribution, if the tensor has a second reader
        pend_data, pend_scale = (pend.data, pend.scale) if pend is not None else (None, None)
        t16 = self._parity_products(blk, dy, t.shape[-1])
        dx16 = torch.empty(t.shape, dtype=self.t16, device=self.device)
        oscale = torch.empty(3, dtype=torch.float32, device=self.device)
        self._run("sk_train_interleave2_h", t16, pend_data, pend_scale, dx16, oscale, B, ox, oy, oz, t.shape[-1],
                  dy.scale)
        grads[t.data_ptr()] = _Grad16(dx16, oscale, True)

    def _dx_pooled(self, blk, dy, t, up, lo, grads, rec) -> None:
        B, ox, oy, oz, _ = blk.y.shape
        dx16 = self._dgrad16(blk, dy, t, lo, rec)
        c16 = torch.empty(t.shape, dtype=self.t16, device=self.device)
        oscale = torch.empty(3, dtype=torch.float32, device=self.device)
        self._run("sk_train_sumpool2_hh", dx16, dy.scale, c16, oscale, B, ox // 2, oy // 2, oz // 2, t.shape[-1])
        grads[t.data_ptr()] = _Grad16(c16, oscale, True)

    def _dx_heads(self, blk, dy, t, up, lo, grads, rec) -> None:
        dl_scale = torch.zeros(3, dtype=torch.float32, device=self.device)
        self._run("sk_train_absmax_scale", dy, dy.numel(), dl_scale)
        dx16 = torch.empty(t.shape, dtype=self.t16, device=self.device)
        oscale = torch.empty(3, dtype=torch.float32, device=self.device)
        self._run("sk_train_heads_dgrad_f16", dy, dl_scale, blk.layer.weight, dx16, oscale, t.numel() // t.shape[-1],
                  t.shape[-1])
        grads[t.data_ptr()] = _Grad16(dx16, oscale, True)


def _loss_term(spec):
    """A term's loss: a ``tversky`` / ``soft_dice_cldice`` object, or an (alpha, beta, eps) tuple meaning tversky.
    Returns ("tversky", [alpha, beta, eps]) or ("soft_cldice", the object)."""
    from .loss import soft_dice_cldice, tversky
    if isinstance(spec, soft_dice_cldice):
        return "soft_cldice", spec
    if isinstance(spec, tversky):
        return "tversky", [spec.alpha, spec.beta, spec.eps]
    a, b, e = spec
    return "tversky", [float(a), float(b), float(e)]


def fused_loss(logits: Tensor, masks: Tensor, skele_masks: Tensor, baked: Tensor, sigma: Sequence[float],
               vector_scale: Sequence[float] = (60, 60, 12),
               loss_params=((0.25, 0.75, 1e-8), (0.5, 0.5, 1e-8), (0.5, 1.5, 1e-8)),
               weights: Sequence[float] = (1.0, 1.0, 1.0), need_grad: bool = True):
    """The three loss terms of the step (engine.py:465-493) and d(total)/d(logits).  logits (B, X, Y, Z, 5) = head
    outputs before tanh / sigmoid; masks, skele_masks (B, 1, X, Y, Z) (> 0 = foreground); baked (B, 3, X, Y, Z);
    ``loss_params`` = the embedding, probability and skeleton term's loss: an (alpha, beta, eps) tuple or a
    ``tversky`` object (Tversky; the three Tversky terms and their gradient take two passes over the logits) or a
    ``soft_dice_cldice`` object (its probability field -- the embedding probability, sigmoid(logits[..., 4]) or
    sigmoid(logits[..., 3]) -- through the soft-clDice kernels, the gradient chained into the logits).
    Returns (losses[4] = embed, prob, skeleton, total; dlogits)."""
    _ffi.require_gpu(logits, "logits")
    B, X, Y, Z, five = logits.shape
    if five != 5 or logits.dtype != torch.float32:
        raise ValueError("logits must be fp32 (B, X, Y, Z, 5)")
    terms = [_loss_term(t) for t in loss_params]
    n = X * Y * Z
    dev = logits.device
    m = masks.reshape(B, n).to(dev, torch.float32).contiguous()
    sk = skele_masks.reshape(B, n).to(dev, torch.float32).contiguous()
    bk = baked.reshape(B, 3, n).to(dev, torch.float32).contiguous()
    params: List[float] = []
    for (kind, p), wt in zip(terms, weights):
        # a soft-clDice term weighs 0 in the Tversky kernels: its value and gradient are added below
        params += (p + [float(wt)]) if kind == "tversky" else [0.5, 0.5, 1.0, 0.0]
    losses = torch.empty(16, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    ws = torch.empty(int(_ffi.lib.sk_train_loss_workspace_floats(B, n)), dtype=torch.float32, device=dev)
    scale_h = _ffi.float_array([float(v) for v in vector_scale])
    sigma_h = _ffi.float_array([float(s) for s in sigma])
    st = _ffi.stream_ptr(dev)
    _ffi.check(_ffi.lib.sk_train_loss(_ffi.ptr(logits), _ffi.ptr(m), _ffi.ptr(sk), _ffi.ptr(bk), B, X, Y, Z,
                                      scale_h, sigma_h, _ffi.float_array(params),
                                      _ffi.ptr(losses), _ffi.ptr(dl), _ffi.ptr(ws), st))
    for term, ((kind, fn), wt) in enumerate(zip(terms, weights)):
        if kind != "soft_cldice":
            continue
        prob = torch.empty((B, n), dtype=torch.float32, device=dev)
        gt = torch.empty_like(prob)
        _ffi.check(_ffi.lib.sk_train_cldice_term_field(_ffi.ptr(logits), _ffi.ptr(sk if term == 2 else m), _ffi.ptr(bk),
                                                       B, X, Y, Z, scale_h, sigma_h, term, _ffi.ptr(prob), _ffi.ptr(gt),
                                                       st))
        term_loss = torch.empty(1, dtype=torch.float32, device=dev)
        dprob = torch.empty_like(prob) if need_grad else None
        cws = torch.empty(int(_ffi.lib.sk_train_soft_dice_cldice_workspace_floats(B, X, Y, Z, min(max(fn.iter, 0), 16))),
                          dtype=torch.float32, device=dev)
        _ffi.check(_ffi.lib.sk_train_soft_dice_cldice(_ffi.ptr(prob), _ffi.ptr(gt), B, X, Y, Z, fn.iter, fn.alpha,
                                                      fn.smooth, _ffi.ptr(term_loss), _ffi.ptr(dprob), _ffi.ptr(cws), st))
        _ffi.check(_ffi.lib.sk_train_cldice_chain(_ffi.ptr(logits), _ffi.ptr(bk), B, X, Y, Z, scale_h, sigma_h, term,
                                                  float(wt), _ffi.ptr(dprob), _ffi.ptr(term_loss), _ffi.ptr(losses),
                                                  _ffi.ptr(dl), st))
    return losses[:4], dl


class TrainStep:
    """Optimizer + loss configuration around a :class:`TrainUNet` (engine.py:272-341 of the reference).

    Defaults are the reference's (skoots/config.py:49-64,87,96-101,144): AdamW lr 5e-4, weight decay
    1e-6, betas (0.9, 0.999), eps 1e-8; Tversky (alpha, beta, eps) = embed (0.25, 0.75, 1e-8), probability
    (0.5, 0.5, 1e-8), skeleton (0.5, 1.5, 1e-8); relative weights 1; vector scaling (60, 60, 12).  Each of
    ``loss_embed`` / ``loss_prob`` / ``loss_skele`` is an (alpha, beta, eps) tuple (Tversky) or a loss object,
    ``tversky(...)`` or ``soft_dice_cldice(...)`` (e.g. ``loss.loss_from_cfg(cfg.TRAIN.LOSS_SKELETON, ...)``).

    ``lr`` is a plain attribute read by every optimizer step: the training loop sets it at the start of each epoch
    (skoots_amd/train/trainer.py)."""

    def __init__(self, model: TrainUNet, lr: float = 5e-4, weight_decay: float = 1e-6, betas=(0.9, 0.999),
                 eps: float = 1e-8, vector_scale=(60, 60, 12),
                 loss_embed=(0.25, 0.75, 1e-8), loss_prob=(0.5, 0.5, 1e-8), loss_skele=(0.5, 1.5, 1e-8),
                 weights=(1.0, 1.0, 1.0), process_group=False):
        """``process_group``: False = single process; None = the default torch.distributed group; or a group."""
        self.model = model
        self.process_group = process_group
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.vector_scale = [float(v) for v in vector_scale]
        self.loss_params = [_loss_term(t)[1] for t in (loss_embed, loss_prob, loss_skele)]
        self.weights = [float(w) for w in weights]
        self.exp_avg = torch.zeros_like(model.flat_param)
        self.exp_avg_sq = torch.zeros_like(model.flat_param)
        self.step_count = 0

    def fused_loss(self, logits: Tensor, masks: Tensor, skele_masks: Tensor, baked: Tensor, sigma: Sequence[float],
                   weights: Optional[Sequence[float]] = None, need_grad: bool = True):
        return fused_loss(logits, masks, skele_masks, baked, sigma, self.vector_scale, self.loss_params,
                          self.weights if weights is None else weights, need_grad)

    def sync_gradients(self) -> None:
        """Data-parallel training (engine.py:113-115 wraps the model in DistributedDataParallel): average the
        flat gradient buffer over the ranks -- one all-reduce of ~6.6 MB per step (RCCL on the GPU)."""
        sync_gradients(self.model.flat_grad, self.process_group)

    def optimizer_step(self) -> None:
        self.step_count += 1
        p = self.model.flat_param
        _ffi.check(_ffi.lib.sk_train_adamw(_ffi.ptr(p), _ffi.ptr(self.model.flat_grad), _ffi.ptr(self.exp_avg),
                                           _ffi.ptr(self.exp_avg_sq), p.numel(), self.lr, self.betas[0], self.betas[1],
                                           self.eps, self.weight_decay, self.step_count, _ffi.stream_ptr(p.device)))

    def __call__(self, images: Tensor, masks: Tensor, skele_masks: Tensor, baked: Tensor,
                 sigma: Sequence[float] = (20.0, 20.0, 20.0), weights: Optional[Sequence[float]] = None) -> Tensor:
        """One step (engine.py:456-499).  Returns a device tensor (embed, prob, skeleton, total)."""
        logits = self.model.forward(images)
        losses, dl = self.fused_loss(logits, masks, skele_masks, baked, sigma, weights)
        self.model.backward(dl)
        if self.process_group is not False:
            self.sync_gradients()
        self.optimizer_step()
        return losses

    @torch.no_grad()
    def evaluate(self, images: Tensor, masks: Tensor, skele_masks: Tensor, baked: Tensor,
                 sigma: Sequence[float] = (20.0, 20.0, 20.0), weights: Optional[Sequence[float]] = None) -> Tensor:
        """The validation pass of one batch (engine.py:559-595): forward and losses only -- no gradient, no optimizer
        step -- then what the forward kept for a backward is released.  Returns (embed, prob, skeleton, total) on the
        device.  As in the reference (engine.py:571), the SKELETON term is computed with the PROBABILITY term's loss
        function."""
        logits = self.model.forward(images)
        params = [self.loss_params[0], self.loss_params[1], self.loss_params[1]]
        losses, _ = fused_loss(logits, masks, skele_masks, baked, sigma, self.vector_scale, params,
                               self.weights if weights is None else weights, need_grad=False)
        self.model.release()
        return losses

    # -- checkpoint (the payload the reference documents: cfg, model_state_dict, optimizer_state_dict) ------
    def checkpoint(self, cfg: Optional[dict] = None) -> dict:
        return {"cfg": cfg if cfg is not None else {"MODEL": {"DIMS": list(self.model.dims), "DEPTHS": list(self.model.depths),
                                                              "IN_CHANNELS": 1},
                                                    "SKOOTS": {"VECTOR_SCALING": [int(v) for v in self.vector_scale]}},
                "model_state_dict": {k: v.cpu() for k, v in self.model.state_dict().items()},
                "optimizer_state_dict": {"step": self.step_count, "exp_avg": self.exp_avg.cpu(),
                                         "exp_avg_sq": self.exp_avg_sq.cpu(), "lr": self.lr,
                                         "weight_decay": self.weight_decay, "betas": list(self.betas), "eps": self.eps,
                                         "param_names": list(self.model.param_names)}}

    def save(self, path: str, cfg: Optional[dict] = None) -> None:
        """Plain-tensor checkpoint that ``skoots_amd.lib.eval.eval`` loads with ``weights_only=True``."""
        torch.save(self.checkpoint(cfg), path)

    def load_optimizer_state(self, state: dict) -> None:
        if list(state["param_names"]) != list(self.model.param_names):
            raise ValueError("optimizer state belongs to a different parameter layout")
        self.step_count = int(state["step"])
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])


def sync_gradients(flat_grad: Tensor, group=None) -> None:
    """Average a flat gradient buffer over the ranks of ``group`` (sum all-reduce, then 1/world)."""
    import torch.distributed as dist
    if not dist.is_initialized():
        raise RuntimeError("sync_gradients needs an initialised torch.distributed process group")
    world = dist.get_world_size(group)
    if world == 1:
        return
    dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=group)
    flat_grad.mul_(1.0 / world)


def train_step(step: TrainStep, images: Tensor, masks: Tensor, skele_masks: Tensor, baked: Tensor,
               sigma: Sequence[float] = (20.0, 20.0, 20.0)) -> Tensor:
    """Functional spelling of ``TrainStep.__call__``."""
    return step(images, masks, skele_masks, baked, sigma)
