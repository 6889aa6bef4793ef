"""The workspace allocator the tests install: every scratch block an op requests through ``_lib.workspace`` comes pre-filled and
stands between two guard pages.

    with poisoned("ones") as run:
        out = op(...)                     # every `ws` argument of the C ABI is now 0xFF where the op has not written
    run.sizes                             # the requests seen, in order

Modes
  zero     0x00 everywhere: what a fresh allocation reads as, the baseline the other modes are compared with
  ones     0xFF everywhere: NaN in a float, -1 in an int, 2^32-1 in a counter
  recycle  the k-th request holds the bytes the k-th request of the PREVIOUS poisoned() run held when that run ended, tiled or
           truncated to the new size (0xFF where that run had no k-th request); the guards are 0xFF.  A caching allocator hands a
           larger call's block to a smaller call exactly like this.

Each request allocates GUARD + n + GUARD bytes and hands out the middle.  GUARD is a multiple of the 16 and 256 byte alignments the
layouts assume and of the caching allocator's 512, so the slice is aligned as the block itself.  On exit the device is synchronised
and both guards of every block must still hold their fill; blocks an autograd node keeps for its backward are checked then too, as
long as the backward ran inside the ``with``.  A write farther than GUARD bytes outside a workspace is not seen.
"""
from __future__ import annotations

import contextlib

import torch

from geosplatting_amd import _lib

GUARD = 4096
MODES = ("zero", "ones", "recycle")

_previous: list = []          # the middle slices (clones) of the last finished run, in request order


class GuardError(AssertionError):
    pass


class Run:
    def __init__(self, mode: str, previous: list):
        if mode not in MODES:
            raise ValueError(f"poisoned(): mode {mode!r} is not one of {MODES}")
        self.mode, self._previous = mode, previous
        self.parents: list = []        # the GUARD + n + GUARD blocks, kept alive in request order
        self.sizes: list = []

    def alloc(self, n, dtype=torch.uint8, device=None):
        assert dtype == torch.uint8, "workspaces are byte blocks"
        n, k = int(n), len(self.parents)
        parent = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=device)
        parent.fill_(0x00 if self.mode == "zero" else 0xFF)
        if self.mode == "recycle" and k < len(self._previous) and self._previous[k].numel() > 0 and n > 0:
            old = self._previous[k].to(parent.device)
            parent[GUARD:GUARD + n] = old.repeat((n + old.numel() - 1) // old.numel())[:n]
        self.parents.append(parent)
        self.sizes.append(n)
        return parent[GUARD:GUARD + n]

    def fill(self) -> int:
        return 0x00 if self.mode == "zero" else 0xFF

    def broken(self) -> list:
        """[(request index, size, "front" | "back", first bad offset relative to the slice)] of every guard that changed."""
        bad = []
        for k, (parent, n) in enumerate(zip(self.parents, self.sizes)):
            for side, g, origin in (("front", parent[:GUARD], -GUARD), ("back", parent[GUARD + n:], n)):
                wrong = (g != self.fill()).nonzero()
                if wrong.numel():
                    bad.append((k, n, side, origin + int(wrong[0])))
        return bad

    def snapshot(self) -> list:
        return [p[GUARD:GUARD + n].clone() for p, n in zip(self.parents, self.sizes)]


@contextlib.contextmanager
def poisoned(mode: str):
    global _previous
    run = Run(mode, _previous)
    saved, _lib._alloc_workspace = _lib._alloc_workspace, run.alloc
    try:
        yield run
    finally:
        _lib._alloc_workspace = saved
    if torch.cuda.is_available() and any(p.is_cuda for p in run.parents):
        torch.cuda.synchronize()
    _previous = run.snapshot()
    bad = run.broken()
    if bad:
        raise GuardError("workspace guard overwritten (mode %s): " % mode + "; ".join(
            f"request #{k} of {n} bytes, {side} guard, first at offset {off}" for k, n, side, off in bad))
