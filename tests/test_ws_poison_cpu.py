"""tests/ws_poison.py on the CPU: what a request gets, what recycle carries over, and which writes the guards report."""
import pytest
import torch

from geosplatting_amd import _lib
from tests.ws_poison import GUARD, GuardError, poisoned

CPU = torch.device("cpu")


def test_default_allocator_is_torch_empty():
    assert _lib._alloc_workspace is torch.empty
    for n, want in ((0, 1), (1, 1), (777, 777)):
        w = _lib.workspace(n, CPU)
        assert w.dtype == torch.uint8 and w.dim() == 1 and w.numel() == want and w.device == CPU


@pytest.mark.parametrize("mode,fill", [("zero", 0x00), ("ones", 0xFF)])
def test_sizes_alignment_fill(mode, fill):
    assert GUARD % 512 == 0
    with poisoned(mode) as run:
        got = [_lib.workspace(n, CPU) for n in (0, 1, 255, 256, 5000)]
        assert _lib._alloc_workspace == run.alloc
    assert _lib._alloc_workspace is torch.empty                               # restored
    assert run.sizes == [1, 1, 255, 256, 5000]
    for w, parent, n in zip(got, run.parents, run.sizes):
        assert w.dtype == torch.uint8 and w.dim() == 1 and w.numel() == n and w.is_contiguous()
        assert parent.numel() == GUARD + n + GUARD
        assert w.data_ptr() == parent.data_ptr() + GUARD                      # the middle, so aligned as the block torch.empty gave
        assert (w.data_ptr() - parent.data_ptr()) % 256 == 0
        assert bool((parent == fill).all())


def test_allocator_restored_when_the_body_raises():
    with pytest.raises(KeyError):
        with poisoned("ones"):
            raise KeyError("body")
    assert _lib._alloc_workspace is torch.empty


def test_recycle_carries_the_previous_run_over():
    with poisoned("ones"):
        a = _lib.workspace(1000, CPU)
        b = _lib.workspace(10, CPU)
        a.copy_(torch.arange(1000) % 251)                                     # what the "larger call" left behind
        b.copy_(torch.arange(10) + 1)
    with poisoned("recycle") as run:
        small = _lib.workspace(300, CPU)                                      # truncated
        big = _lib.workspace(25, CPU)                                         # tiled
        fresh = _lib.workspace(40, CPU)                                       # the previous run had no third request
        assert torch.equal(small, (torch.arange(300) % 251).to(torch.uint8))
        assert torch.equal(big, (torch.arange(25) % 10 + 1).to(torch.uint8))
        assert bool((fresh == 0xFF).all())
        for parent, n in zip(run.parents, run.sizes):
            assert bool((parent[:GUARD] == 0xFF).all()) and bool((parent[GUARD + n:] == 0xFF).all())
        small.zero_()
    with poisoned("recycle"):                                                 # ... and the recycle run is the next one's "previous"
        assert bool((_lib.workspace(300, CPU) == 0).all())


@pytest.mark.parametrize("mode", ["zero", "ones", "recycle"])
def test_guards(mode):
    fill = 0x00 if mode == "zero" else 0xFF
    with poisoned(mode) as run:                                               # writes inside, the last byte included: silent
        w = _lib.workspace(100, CPU)
        w[0] = fill ^ 0x5A
        w[99] = fill ^ 0x5A
    assert run.broken() == []
    with pytest.raises(GuardError, match=r"request #1 of 100 bytes, front guard, first at offset -1\b"):
        with poisoned(mode) as run:
            _lib.workspace(64, CPU)
            w = _lib.workspace(100, CPU)
            run.parents[1][GUARD - 1] = fill ^ 0x5A                           # one byte in front of the slice
    with pytest.raises(GuardError, match=r"request #0 of 100 bytes, back guard, first at offset 100\b"):
        with poisoned(mode) as run:
            w = _lib.workspace(100, CPU)
            run.parents[0][GUARD + 100] = fill ^ 0x5A                         # one byte behind it
            _lib.workspace(64, CPU)
    assert _lib._alloc_workspace is torch.empty
