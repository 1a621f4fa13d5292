"""Which way every data gradient of the training step's backward travels.

Pure Python: :func:`route_gradients` reads a description of the recorded graph -- no tensor, no library call -- so the
backward's routing can be read here and tested without a GPU.  ``engine.TrainUNet`` records the graph in its forward
and has one method per :class:`Route`; a new hand-off is a new route here plus a new method there."""
from __future__ import annotations

from collections import Counter
from enum import Enum
from typing import Dict, List, NamedTuple, Sequence, Tuple


class Kind(Enum):
    """What the forward ran for a block; it fixes the kernels of that block's backward."""
    FP32 = "fp32"         # sk_conv3d_f32 (+ GroupNorm): every block of precision="fp32", the fallbacks of a 16-bit step
    FAST = "fast"         # 16-bit MFMA conv + GroupNorm; the raw 16-bit conv output is kept
    STEM = "stem"         # the Cin = 1 stem as a fast block (fp32 image operand)
    HEADS16 = "heads16"   # the 1x1x1 heads straight on the 16-bit activation


FAST_KINDS = (Kind.FAST, Kind.STEM)


class Route(Enum):
    """How one source's data gradient travels from a reader to the block that produced the source."""
    NONE = "none"                 # the input image: no gradient
    FP32 = "fp32"                 # an fp32 tensor, created by the first reader to report and accumulated by the others
    DIRECT = "direct"             # the fast conv's scaled 16-bit dx with the reader's own dy scale: the only reader
    PENDING = "pending"           # the same, of a skip tensor whose other reader is a fast stride-2 conv walked later
    INTERLEAVED = "interleaved"   # 16-bit sum inside the stride-2 interleave, with the PENDING partner if there is one
    POOLED = "pooled"             # 16-bit 2x2x2 sum under an upsampled source
    HEADS = "heads"               # 16-bit from the heads on the 16-bit activation


class GraphBlock(NamedTuple):
    """What :func:`route_gradients` knows of a block.  Keys identify tensors (data pointers in a step, any hashable
    in a test); ``srcs`` holds (key, upsampled, channels) per source."""
    name: str
    kind: Kind
    ksize: int
    cout: int
    out: object
    srcs: Tuple[Tuple[object, int, int], ...]


def route_gradients(graph: Sequence[GraphBlock], image, handoff: bool) -> List[List[Route]]:
    """The route of every source's data gradient: ``routes[i][j]`` for source j of ``graph[i]`` (forward order; the
    last block's output receives d loss / d logits).  A function of the recorded graph and ``f16_grad_handoff`` alone
    -- no tensor data, no library call -- so every decision of the backward is made here, before its first kernel.

    A tensor produced by a fast block and read by ONE conv receives its gradient as a scaled 16-bit tensor (DIRECT,
    POOLED, HEADS, or INTERLEAVED under a stride-2 conv) that the producer's GroupNorm backward reads as it is.  A skip
    tensor has two readers: the decoder conv reports first (PENDING) and the stride-2 conv sums both contributions in
    its interleave pass (INTERLEAVED).  Everything else is FP32.  ``TrainUNet.backward`` has one method per route."""
    n_readers = Counter(key for b in graph for key, _, _ in b.srcs)
    fast_out = {b.out for b in graph if b.kind in FAST_KINDS}
    k2_read = {key for b in graph if b.ksize == 2 and b.kind in FAST_KINDS for key, _, _ in b.srcs}
    last: Dict[object, Route] = {graph[-1].out: Route.FP32}   # per tensor, the route of the latest delivery
    routes: List[List[Route]] = [[] for _ in graph]
    for b, out in zip(reversed(graph), reversed(routes)):
        if last.pop(b.out) is Route.PENDING:
            raise RuntimeError("a pending fp16 gradient was never summed")
        fast = b.kind in FAST_KINDS
        for key, up, c in b.srcs:
            if key == image:
                out.append(Route.NONE)
                continue
            if fast and c not in (32, 64, 128):
                raise RuntimeError(f"{b.name}: mixed precision needs source widths of 32, 64 or 128 channels")
            seen, n = last.get(key), n_readers[key]
            h_ok = handoff and key in fast_out   # the producer's GroupNorm backward can read a scaled 16-bit dz
            route = Route.FP32
            if b.ksize == 2:
                # the last reader to report (the decoder's contribution, if any, is PENDING): the sum leaves as 16 bits.
                # What made the partner PENDING -- hand-off on, a fast producer, two readers -- is what is asked here, so
                # a PENDING contribution always meets INTERLEAVED and never an fp32 interleave
                if fast and h_ok and seen is not Route.FP32 and n == (2 if seen is Route.PENDING else 1):
                    route = Route.INTERLEAVED
            elif up:
                if seen is not None:
                    raise RuntimeError("an upsampled tensor has one consumer in this graph")
                if fast and h_ok and n == 1:
                    route = Route.POOLED
            elif fast:
                if h_ok and seen is None and n == 1:
                    route = Route.DIRECT
                elif h_ok and seen is None and n == 2 and key in k2_read:
                    route = Route.PENDING
            elif (h_ok and b.kind is Kind.HEADS16 and b.ksize == 1 and b.cout == 5 and len(b.srcs) == 1 and seen is None and
                  n == 1 and c % 8 == 0 and 256 % (c // 8) == 0):
                route = Route.HEADS
            last[key] = route
            out.append(route)
    return routes
