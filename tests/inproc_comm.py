"""``ThreadComm``: a stand-in for ``skoots_amd.parallel.Comm`` whose R ranks are R threads of ONE process on one device.

Every collective is deposit -> barrier -> read -> barrier on a shared mailbox.  All rank threads issue their device work on the
device's default stream (each calls ``torch.cuda.set_device`` first), so stream order makes a tensor deposited before
the barrier valid to read after it; what a rank receives is a copy, as with a real transport.  Every barrier wait has a
timeout and an exception in any rank aborts the barrier, so a failing rank ends the run instead of leaving the others
waiting.  No process is spawned and no process group is needed: world sizes up to 8 cost a few milliseconds, which is what
lets the sharded stage be tested at the production alignment (tests/test_hip_sharded_kernels.py).
"""
from __future__ import annotations

import threading
import time
from typing import Callable, List, Optional, Tuple

import torch
from torch import Tensor


class _Shared:
    def __init__(self, world: int, timeout: float):
        self.world, self.timeout = world, timeout
        self.barrier = threading.Barrier(world)
        self.gathered: List[Optional[Tensor]] = [None] * world
        self.tags: List[Optional[Tuple[str, str]]] = [None] * world
        self.p2p = {}    # (src, dst) -> FIFO of tensors


class ThreadComm:
    """``rank``, ``world``, ``exchange``, ``all_gather``, ``all_reduce_min`` with the semantics of ``parallel.Comm``."""

    def __init__(self, shared: _Shared, rank: int):
        self._s, self.rank, self.world = shared, rank, shared.world
        self.calls = {}   # what -> number of calls (the accounting the tests read)

    def _wait(self) -> None:
        self._s.barrier.wait(self._s.timeout)

    def _enter(self, kind: str, what: str) -> None:
        self.calls[what] = self.calls.get(what, 0) + 1
        self._s.tags[self.rank] = (kind, what)

    def _check_tags(self) -> None:
        tags = list(self._s.tags)
        if any(t != tags[0] for t in tags):
            raise RuntimeError(f"ranks are in different collectives: {tags}")

    def all_gather(self, t: Tensor, what: str = "all_gather") -> List[Tensor]:
        if self.world == 1:
            return [t]
        self._enter("all_gather", what)
        self._s.gathered[self.rank] = t.contiguous()
        self._wait()
        self._check_tags()
        parts = list(self._s.gathered)
        for r, p in enumerate(parts):   # a real all-gather needs the same shape and type on every rank
            if p.shape != t.shape or p.dtype != t.dtype:
                raise RuntimeError(f"all_gather({what}): rank {r} brought {tuple(p.shape)} {p.dtype}, "
                                   f"rank {self.rank} {tuple(t.shape)} {t.dtype}")
        out = [p.clone() for p in parts]
        self._wait()
        return out

    def all_reduce_min(self, t: Tensor, what: str = "all_reduce") -> Tensor:
        if self.world == 1:
            return t
        parts = self.all_gather(t, what=what)
        return torch.stack(parts).amin(dim=0)

    def exchange(self, sends: List[Tuple[int, Tensor]], recv_like: List[Tuple[int, Tensor]],
                 what: str = "p2p") -> List[Tensor]:
        """Point-to-point batch: sends [(peer, tensor)], recv_like [(peer, empty tensor)]; messages between one pair
        of ranks arrive in the order they were sent."""
        if self.world == 1:
            return []
        self._enter("exchange", what)
        for peer, t in sends:
            if not (0 <= peer < self.world) or peer == self.rank:
                raise RuntimeError(f"exchange({what}): rank {self.rank} sends to rank {peer}")
            self._s.p2p.setdefault((self.rank, peer), []).append(t.contiguous())
        self._wait()
        self._check_tags()
        out = []
        for peer, like in recv_like:
            box = self._s.p2p.get((peer, self.rank))
            if not box:
                raise RuntimeError(f"exchange({what}): rank {self.rank} expects a message from rank {peer}, none was sent")
            t = box.pop(0)
            if t.shape != like.shape or t.dtype != like.dtype:
                raise RuntimeError(f"exchange({what}): rank {peer} sent {tuple(t.shape)} {t.dtype}, rank {self.rank} "
                                   f"expects {tuple(like.shape)} {like.dtype}")
            out.append(t.clone())
        self._wait()
        for peer, _ in sends:   # every message must have been taken
            if self._s.p2p.get((self.rank, peer)):
                raise RuntimeError(f"exchange({what}): rank {peer} did not receive what rank {self.rank} sent")
        return out


def run_ranks(world: int, fn: Callable[[ThreadComm], object], timeout: float = 60.0, device=None) -> list:
    """Run ``fn(comm)`` on ``world`` rank threads and return their results in rank order.  The first exception of a rank
    is re-raised here (the others then fail on the aborted barrier, which is not reported); a rank that has not finished
    after ``timeout`` seconds raises ``TimeoutError``.  ``device``: the CUDA device every thread selects before it starts."""
    shared = _Shared(world, timeout)
    results: list = [None] * world
    errors: list = [None] * world

    def body(r: int) -> None:
        try:
            if device is not None:
                torch.cuda.set_device(device)
            results[r] = fn(ThreadComm(shared, r))
        except BaseException as e:   # noqa: BLE001 -- handed to the driver
            errors[r] = e
            shared.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,), name=f"rank{r}", daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        shared.barrier.abort()
    real = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)]
    if real:
        raise real[0]
    if stuck:
        raise TimeoutError(f"{stuck} still running after {timeout} s")
    broken = [e for e in errors if e is not None]
    if broken:
        raise broken[0]
    return results
