"""The large class of the tile-first binning's segment sort (gs_isect_bin_front with tile_counts): segments longer than 2 048 items go
to one 512-thread workgroup each, which sorts up to 8 192 items in LDS and a longer segment in 8 192-item chunks in LDS with the wide
stages of the network in place in the item buffer.

Reference as in test_gpu_bin_tilefirst.py: expand every Gaussian's rectangle into (tile, key, slot) triples, order them with
np.lexsort((slot, key, tile)); the offsets are the exclusive cumulative sum of the tile counts clamped to I.  Everything is compared
bit for bit, the words behind the output must keep their sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -0x5A5A5A5B


def _expand(rects, tw):
    """(tile, slot) of every intersection, any order"""
    x0, y0, x1, y1 = (rects[:, 0] & 0xffff).astype(np.int64), (rects[:, 0] >> 16).astype(np.int64), \
        (rects[:, 1] & 0xffff).astype(np.int64), (rects[:, 1] >> 16).astype(np.int64)
    w, h = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    cnt = w * h
    slot = np.repeat(np.arange(len(rects), dtype=np.int64), cnt)
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ww = np.repeat(w, cnt)
    tile = (np.repeat(y0, cnt) + k // np.maximum(ww, 1)) * tw + np.repeat(x0, cnt) + k % np.maximum(ww, 1)
    return tile, slot


def _reference(keys, rects, tw, th, key_bits):
    tile, slot = _expand(rects, tw)
    key = (keys.astype(np.int64) & ((1 << key_bits) - 1))[slot]
    order = np.lexsort((slot, key, tile))
    counts = np.bincount(tile, minlength=tw * th).astype(np.int64)
    I = int(counts.sum())
    offsets = np.minimum(np.cumsum(counts) - counts, I).astype(np.int32)
    return slot[order].astype(np.int32), offsets, counts.astype(np.uint32), I


def _pack(x0, y0, x1, y1):
    return np.stack([x0 | (y0 << 16), x1 | (y1 << 16)], axis=1).astype(np.uint32)


def _run(cuda, keys, rects, tw, th, key_bits, cap=None, v_extra=0):
    """-> (flat incl. guard, offsets, status, reference).  cap None: exact mode; else capacity mode with V_cap = V + v_extra garbage rows."""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    V = len(keys)
    ref_flat, ref_off, tcounts, I = _reference(keys, rects, tw, th, key_bits)
    rng = np.random.default_rng(99)
    k_host = np.concatenate([keys.astype(np.uint32), rng.integers(0, 2 ** 32, v_extra, dtype=np.uint32)])
    r_host = np.concatenate([rects.astype(np.uint32), rng.integers(0, 2 ** 32, (v_extra, 2), dtype=np.uint32)])
    k_dev = torch.from_numpy(k_host.view(np.int32)).to(cuda).contiguous()
    r_dev = torch.from_numpy(r_host.view(np.int32).reshape(-1, 2)).to(cuda).contiguous()
    t_dev = torch.from_numpy(tcounts.view(np.int32)).to(cuda).contiguous()
    if cap is None:
        v_arg, i_arg, counts, status = V, I, None, None
    else:
        v_arg, i_arg = V + v_extra, cap
        counts = torch.tensor([V, I, 0, 0], dtype=torch.int64, device=cuda)
        status = torch.zeros(4, dtype=torch.int64, device=cuda)
    flat = torch.full((max(i_arg, 1) + GUARD,), SENTINEL, dtype=torch.int32, device=cuda)
    offsets = torch.full((tw * th,), -7, dtype=torch.int32, device=cuda)
    nbytes = lib.gs_isect_bin_front_ws_bytes(v_arg, L.i64(i_arg), tw, th)
    ws = torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=cuda)
    rc = lib.gs_isect_bin_front(v_arg, L.ptr(k_dev), L.ptr(r_dev), L.ptr(t_dev), L.ptr(counts), L.i64(i_arg), key_bits, tw, th,
                                L.ptr(flat), L.ptr(offsets), L.ptr(ws), C.c_size_t(nbytes), L.ptr(status), L.stream())
    L.check(rc, "gs_isect_bin_front")
    torch.cuda.synchronize()
    return flat.cpu().numpy(), offsets.cpu().numpy(), (status.cpu().tolist() if status is not None else None), (ref_flat, ref_off, I)


def _check(cuda, keys, rects, tw, th, key_bits, **kw):
    flat, off, status, (ref_flat, ref_off, I) = _run(cuda, keys, rects, tw, th, key_bits, **kw)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(flat[:I], ref_flat)
    assert (flat[I:] == SENTINEL).all() and len(flat) >= I + GUARD
    if status is not None:
        assert status == [0, 0, 0, 0]
    return flat[:I]


def _keys(rng, n, key_bits, distinct):
    """keys from `distinct` values; 32-bit keys carry bit 31 on a third of the items (the integer compare must be unsigned)"""
    keys = rng.integers(0, distinct, n).astype(np.uint32) << np.uint32(9)
    if key_bits == 32:
        keys = keys | (np.uint32(0x80000000) * (np.arange(n) % 3 == 0).astype(np.uint32))
    return keys


def test_paths_reported():
    from geosplatting_amd import _lib as L
    caps = (C.c_int * 8)()
    assert L.lib().gs_isect_bin_front_classes(caps, 8) == 2 and [caps[0], caps[1]] == [2048, 8192]


@pytest.mark.parametrize("distinct", [16, 1])
@pytest.mark.parametrize("key_bits", [24, 32])
@pytest.mark.parametrize("n", [8191, 8192, 8193, 12288, 12289, 16384, 16385, 24577, 32769])
def test_one_long_tile(cuda, n, key_bits, distinct):
    """the middle tile of a 3 x 1 grid holds n items: whole chunks, one item more (a last chunk with a single live item), one less,
    a half-filled last chunk; 24 577 and 32 769: two and three wide stages above the chunk"""
    rng = np.random.default_rng(n * 7 + key_bits + distinct)
    o = np.ones(n, np.int64)
    _check(cuda, _keys(rng, n, key_bits, distinct), _pack(o, 0 * o, o + 1, o), 3, 1, key_bits)


@pytest.mark.parametrize("key_bits", [24, 32])
def test_neighbouring_segments(cuda, key_bits):
    """4 x 2 grid, two long tiles side by side (5 000 and 9 000 items), one of 3 000, an empty one and short ones, slots shuffled over
    the tiles, capacity mode with garbage rows behind V: nothing behind a segment's end is loaded or stored -- the next segment's ids
    are right, the words behind I keep their sentinel"""
    lengths = [5000, 9000, 3000, 0, 17, 1, 2048, 300]
    rng = np.random.default_rng(21 + key_bits)
    tile = rng.permutation(np.repeat(np.arange(8), lengths)).astype(np.int64)
    V = len(tile)
    keys = _keys(rng, V, key_bits, 16)
    keys[::5] = rng.integers(0, 1 << 24, len(keys[::5]), dtype=np.uint32)
    x0, y0 = tile % 4, tile // 4
    I = V
    _check(cuda, keys, _pack(x0, y0, x0 + 1, y0 + 1), 4, 2, key_bits, cap=((I + 4095) // 4096) * 4096 + 4096, v_extra=777)


@pytest.mark.parametrize("long_tile", [0, 5])
def test_overflow_with_a_long_tile(cuda, long_tile):
    """cap = I - 100 with one tile of 10 000 items (first: a short tile is cut; last: the long one is): status reports {ENOSPC, I, V},
    nothing behind cap is written, every offset <= cap, every id a valid row; contents unspecified"""
    lengths = [700] * 6
    lengths[long_tile] = 10000
    rng = np.random.default_rng(31 + long_tile)
    tile = rng.permutation(np.repeat(np.arange(6), lengths)).astype(np.int64)
    V = I = len(tile)
    keys = rng.integers(0, 1 << 32, V, dtype=np.uint32)
    x0, y0 = tile % 3, tile // 3
    cap = I - 100
    flat, off, status, _ = _run(cuda, keys, _pack(x0, y0, x0 + 1, y0 + 1), 3, 2, 32, cap=cap, v_extra=0)
    assert status[0] != 0 and status[1] == I and status[2] == V and status[3] == 0       # {ENOSPC, required I, V seen, -}
    assert (flat[cap:] == SENTINEL).all() and len(flat) == cap + GUARD
    assert (off >= 0).all() and (off <= cap).all() and (np.diff(off) >= 0).all()
    assert (flat[:cap] >= 0).all() and (flat[:cap] < V).all()       # still valid rows for whoever gathers by them
