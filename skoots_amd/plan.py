"""What the inference forward runs, decided before its first kernel ("The forward's plan").

Pure Python: :func:`network_blocks` describes the U-Net, :func:`plan_forward` turns that description, the precision,
the A/B switches and the shape of the request into one :class:`Step` per block plus the heads -- no tensor, no
library call -- so the choice of kernels can be read here and is tested without a GPU (tests/test_forward_plan.py).
``unet.HipUNet`` only executes the plan: one launcher per :class:`Kernel`.

Fused GroupNorm + SiLU.  A conv writes its RAW output and hands (tensor, affine) on; the consumer applies
silu(a*x + b) while it stages the tensor -- the stride-2 down convs and the single-chunk 3x3x3 convs in LDS, the 1x1x1
convs and the heads on load -- so no separate normalisation pass touches HBM for that tensor.  The two skip tensors are
activated (and written back) by their stride-2 down conv, since the decoder reads them as well.  Where it was measured
to cost more than the pass it saves, the pass stays (tools/kernel_ab.sh, 8 tiles of 300x300x20: in-LDS activation
inside the 64/128-channel convs +413 us for 325 us of passes; inside a conv that reads an UPSAMPLED raw tensor +252 us
for a 45 us pass over the low-resolution tensor; inside the single-chunk 32->32 conv +188 us for a 345 us pass: kept).
``keep_features`` and the split modes take the unfused path, except that the stride-2 convs, the 1x1x1 convs and the
heads activate their raw input in every fast mode.
"""
from __future__ import annotations

from enum import Enum
from functools import lru_cache
from typing import List, NamedTuple, Optional, Tuple

PRECISIONS = ("fp16", "split", "mix8", "fp32")


class Block(NamedTuple):
    """One Conv3d -> GroupNorm -> SiLU block.  ``level``: 0 = the tile's resolution, 1 = half, 2 = a quarter;
    ``srcs``: (producer's name or "image", upsampled, channels) per source, concatenated in this order."""
    name: str
    ksize: int
    cout: int
    level: int
    srcs: Tuple[Tuple[str, int, int], ...]

    @property
    def cin(self) -> int:
        return sum(c for _, _, c in self.srcs)


def network_blocks(dims, depths) -> Tuple[Block, ...]:
    """The network (graph: oracle/unet_spec.py ``UNetSpec``) in execution order, which is also the order of its
    parameters in a state dict."""
    d0, d1, d2, d3, d4 = dims
    blocks: List[Block] = []

    def add(name, ksize, cout, level, skip=None):
        prev = (blocks[-1].name, int(skip is not None), blocks[-1].cout) if blocks else ("image", 0, 1)
        blocks.append(Block(name, ksize, cout, level, (skip, prev) if skip else (prev,)))

    def stack(stage, n, cout, level, skip=None):   # the first conv of a decoder stage reads cat([skip, upsample(x)])
        for i in range(n):
            add(f"{stage}.{i}", 3, cout, level, skip if i == 0 else None)
        return (blocks[-1].name, 0, cout)

    s0 = stack("enc0", depths[0], d0, 0)
    add("down0", 2, d1, 1)
    s1 = stack("enc1", depths[1], d1, 1)
    add("down1", 2, d2, 2)
    stack("mid", depths[2], d2, 2)
    add("red1", 1, d3, 2)
    stack("dec1", depths[3], d3, 1, s1)
    add("red0", 1, d4, 1)
    stack("dec0", depths[4], d4, 0, s0)
    return tuple(blocks)


class Form(Enum):
    """How a tensor lies in its buffer."""
    RAW = "raw"       # conv output before GroupNorm, in the precision's layout; its reader applies the producer's affine + SiLU
    F16 = "fp16"      # activated, one fp16 per channel
    SPLIT = "split"   # activated, [hi | lo] fp16 pairs: twice the channels
    MIX8 = "mix8"     # activated, [hi | x8 | lo8] lines: what sk_conv3d_mix8 / sk_conv3d_upfold_mix8 read
    F32 = "fp32"      # activated fp32: precision "fp32", fresh allocations instead of the tagged buffers


class Kernel(Enum):
    """The kernel family a step runs; ``unet.HipUNet`` has one launcher for each."""
    STEM = "stem"                  # Cin = 1, two passes: statistics, then the conv again with GroupNorm + SiLU in its epilogue
    STEM_RAW = "stem raw"          # one pass: the raw result and its statistics
    CONV = "conv"                  # sk_conv3d / _split: any kernel size, any sources
    CONV_BOX = "conv box"          # the same, storing only the box its reader looks at
    UPFOLD = "upfold"              # decoder conv, the nearest-upsample folded into the weights
    MIX8 = "mix8"                  # C -> C 3x3x3 on mix8 lines (with or without the store box)
    UPFOLD_MIX8 = "upfold mix8"    # the folded decoder conv on mix8 lines
    DOWN_ACT = "down act"          # stride-2 conv that activates its RAW input in LDS and writes it back activated
    DOWN = "down"                  # stride-2 conv of an activated input: the plain conv kernel
    HEADS = "heads"
    F32 = "fp32"                   # sk_conv3d_f32 + GroupNorm + SiLU
    HEADS_F32 = "heads fp32"


class Src(NamedTuple):
    name: str    # the producing block, or "image"
    tag: str     # the buffer it is read from
    form: Form   # RAW: read with the affine of ``name``
    up: int
    c: int


class Step(NamedTuple):
    name: str
    kernel: Kernel
    ksize: int
    cout: int
    level: int
    srcs: Tuple[Src, ...]
    tag: str                    # the buffer it writes
    out: Form                   # how it leaves its output there
    store: Form                 # F16 | SPLIT | F32: the layout of the precision (of RAW tensors, too)
    writeback: Optional[Form]   # DOWN_ACT: the form its input is in afterwards
    box: bool                   # only ``out_box`` of the output is stored
    keep: bool                  # ``keep_features``: a copy of the output goes to ``last_features``

    @property
    def norm_pass(self) -> Optional[Form]:
        """The variant of the separate GroupNorm + SiLU pass over the output, None where there is none."""
        return None if self.out is Form.RAW or self.kernel in (Kernel.STEM, Kernel.HEADS, Kernel.HEADS_F32) else self.out

    @property
    def lanes(self) -> int:
        return 2 if self.store is Form.SPLIT else 1


@lru_cache(maxsize=None)
def plan_forward(dims: Tuple[int, ...], depths: Tuple[int, ...], precision: str = "fp16", defer_activation: bool = True,
                 fold_upsample: bool = True, box_store: bool = True, stem_single_pass: bool = False,
                 keep_features: bool = False, has_box: bool = False, fold_ok: Tuple[bool, bool] = (True, True)) -> Tuple[Step, ...]:
    """The steps of ``HipUNet.forward_tiles``.  ``has_box``: an ``out_box`` is given; ``fold_ok[level]``: the folded
    decoder kernel covers the tile at that level (``sk_conv3d_upfold_num_blocks`` > 0)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}")
    d0, d1, d2, d3, d4 = dims
    if not (d0 == d4 == 32 and d1 == d3 and d1 in (32, 64, 128) and d2 in (32, 64, 128)):
        raise ValueError(f"unsupported dims {dims}: kernels are built for widths 32/64/128")
    fast = precision != "fp32"
    store = {"fp16": Form.F16, "fp32": Form.F32}.get(precision, Form.SPLIT)
    keep = keep_features and fast
    defer, fold = defer_activation and fast, fold_upsample and fast
    fuse_down = defer and not keep             # the stride-2 and 1x1x1 convs activate a raw input in every fast mode
    fuse = fuse_down and store is Form.F16     # the 3x3x3 convs only where it was measured to pay
    mix8 = precision == "mix8" and not keep    # keep_features wants plain pairs: the split path then

    blocks = network_blocks(dims, depths)
    heads = Block("heads", 1, 5, 0, ((blocks[-1].name, 0, blocks[-1].cout),))
    readers = {b.name: [r for r in blocks + (heads,) if any(n == b.name for n, _, _ in r.srcs)] for b in blocks}
    raw_out = set()   # blocks that leave their output RAW

    def lds_act(b, r):   # does the 3x3x3 conv r activate b's raw output in LDS at a profit?  Measured at level 0 only
        return fuse and r.ksize == 3 and r.cin == 32 and b.level == 0

    def folds(r):
        return fold and len(r.srcs) == 2 and fold_ok[r.level]

    def reads_mix8(r):
        """Does r read mix8 lines?  A C -> C 3x3x3 conv does; a decoder conv if it folds and its skip tensor comes
        activated from the fused stride-2 conv, which then writes mix8 lines back."""
        if not (mix8 and r.ksize == 3):
            return False
        if len(r.srcs) == 2:
            return folds(r) and r.srcs[0][0] in raw_out
        return r.cin == r.cout and r.cout in (32, 64, 128)

    stored = {"image": ("image", Form.F16)}   # name -> (tag, form) of every tensor produced so far
    steps = []
    for b in blocks:
        srcs = tuple(Src(n, *stored[n], up, c) for n, up, c in b.srcs)
        rs = readers[b.name]
        down = next((r for r in rs if r.ksize == 2), None)   # b is a skip tensor: read by ``down`` and by the decoder
        if rs[0] is heads:
            raw = defer                        # also with keep_features
        elif b.cin == 1:
            raw = stem_single_pass and len(rs) == 1 and lds_act(b, rs[0])
        elif down is not None:                 # the two shapes sk_conv3d_down_act is built for
            raw = fuse_down and (down.cin, down.cout) == (32 << b.level, 64 << b.level)
        elif rs[0].ksize == 1:
            raw = fuse_down
        else:
            raw = lds_act(b, rs[0])
        if raw:
            raw_out.add(b.name)
        out = Form.RAW if raw else Form.MIX8 if down is None and reads_mix8(rs[0]) else store
        # the last conv's raw output is read by the heads alone, and with an out_box only inside it
        box = rs[0] is heads and raw and has_box and box_store and not keep
        writeback = None
        if not fast:
            kernel = Kernel.F32
        elif b.cin == 1:
            kernel = Kernel.STEM_RAW if raw else Kernel.STEM
        elif b.ksize == 2 and srcs[0].form is Form.RAW:
            kernel = Kernel.DOWN_ACT
            decoder = next(r for r in readers[srcs[0].name] if r is not b)
            writeback = Form.MIX8 if reads_mix8(decoder) else store
            stored[srcs[0].name] = (srcs[0].tag, writeback)
        elif b.ksize == 2:
            kernel = Kernel.DOWN
        elif srcs[0].form is Form.MIX8:
            kernel = Kernel.UPFOLD_MIX8 if len(srcs) == 2 else Kernel.MIX8
        elif folds(b):                         # its own workgroup count; the store box is not folded in
            kernel = Kernel.UPFOLD
        else:
            kernel = Kernel.CONV_BOX if box else Kernel.CONV
        # ping-pong "a" / "b" per level; a skip tensor and the output of a 1x1x1 conv outlive that, in tags of their own
        tag = (f"skip{b.level}" if down is not None else f"L{b.level}r" if b.ksize == 1 else
               f"L{b.level}b" if any(s.tag == f"L{b.level}a" for s in srcs) else f"L{b.level}a")
        steps.append(Step(b.name, kernel, b.ksize, b.cout, b.level, srcs, tag, out, store, writeback,
                          box and kernel in (Kernel.MIX8, Kernel.CONV_BOX), keep))
        stored[b.name] = (tag, out)
    last = blocks[-1]
    steps.append(Step("heads", Kernel.HEADS if fast else Kernel.HEADS_F32, 1, 5, 0,
                      (Src(last.name, *stored[last.name], 0, last.cout),), "out5", Form.F16 if fast else Form.F32,
                      store, None, False, False))
    return tuple(steps)


def conv_flops(step: Step) -> Tuple[float, float, float]:
    """Per output voxel of a 3x3x3 step: (algorithmic FLOPs 2*Cin*Cout*27, FLOPs the launch puts on the matrix pipe per
    pass, passes).  The folded kernels run 8 of the 27 taps for the upsampled channels.  Split mode: three fp16 MFMA
    products (w_lo x_hi, w_hi x_hi, w_hi x_lo) per algorithmic product; mix8: the fp16 product + one fp8 instruction
    stream that takes the time of 10/9 (K = 128: ten tap rows for nine) or 1 (K = 64, folded taps) fp16 passes --
    counted in fp16-pass equivalents against the fp16 peak."""
    c = [s.c for s in step.srcs]
    algorithmic = 2.0 * sum(c) * step.cout * step.ksize ** 3
    k128 = 1.0 + 10.0 / 9.0
    if step.kernel is Kernel.UPFOLD_MIX8:
        return algorithmic, 2.0 * step.cout * (c[0] * 27 * k128 + c[1] * 8 * 2.0), 1.0
    if step.kernel is Kernel.MIX8:
        return algorithmic, algorithmic, k128 if step.cout == 32 else 2.0
    passes = 3.0 if step.store is Form.SPLIT else 1.0
    if step.kernel is Kernel.UPFOLD:
        return algorithmic, 2.0 * step.cout * (c[0] * 27 + c[1] * 8), passes
    return algorithmic, algorithmic, passes
