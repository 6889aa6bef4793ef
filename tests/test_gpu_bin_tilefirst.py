"""The tile-first binning of the engine (gs_isect_bin_front with tile_counts: scatter into per-tile segments, segment sort on chip)
against NumPy on synthetic keys, rectangles and tile counts, passed to the C entry as front.bin_stage passes them.

Reference: expand every Gaussian's rectangle into (tile, key, slot) triples, order them with np.lexsort((slot, key, tile)); the offsets
are the exclusive cumulative sum of the tile counts clamped to I.  Everything is compared bit for bit -- the order inside a segment
after the scatter is arbitrary, the sort on (key, slot) must make the result unique."""
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


def _run(cuda, keys, rects, tw, th, key_bits, cap=None, v_extra=0, counts_override=None):
    """-> (flat incl. guard, offsets, status, rc).  cap None: exact mode; else capacity mode with V_cap = V + v_extra garbage rows."""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    V = len(keys)
    ref_flat, ref_off, tcounts, I = _reference(keys, rects, tw, th, key_bits)
    if counts_override is not None:
        tcounts = counts_override
    rng = np.random.default_rng(99)
    k_host = np.concatenate([keys.astype(np.uint32), rng.integers(0, 2 ** 32, v_extra, dtype=np.uint32)])
    r_host = np.concatenate([rects.astype(np.uint32), rng.integers(0, 2 ** 32, (v_extra, 2), dtype=np.uint32)])
    dev = lambda a, dt: torch.from_numpy(a.view(dt) if a.dtype != dt else a).to(cuda).contiguous()
    k_dev = dev(k_host.view(np.int32), np.int32) if len(k_host) else torch.zeros(1, dtype=torch.int32, device=cuda)
    r_dev = dev(r_host.view(np.int32).reshape(-1, 2), np.int32) if len(r_host) else torch.zeros(1, 2, dtype=torch.int32, device=cuda)
    t_dev = dev(tcounts.view(np.int32), np.int32)
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
    assert (flat[-GUARD:] == SENTINEL).all()
    if status is not None:
        assert status == [0, 0, 0, 0]
    return flat[:I]


def _classes():
    from geosplatting_amd import _lib as L
    caps = (C.c_int * 8)()
    n = L.lib().gs_isect_bin_front_classes(caps, 8)
    assert 1 <= n <= 8
    out = [int(caps[i]) for i in range(n)]
    assert out == sorted(out) and out[0] >= 1
    return out


def test_trivial(cuda):
    """V = 1 in one tile of a 3 x 2 grid; V = 0; I = 0"""
    one = np.array([1], np.int64)
    _check(cuda, np.array([123456], np.uint32), _pack(one, one, one + 1, one + 1), 3, 2, 32)
    _, off, _, _ = _run(cuda, np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32), 3, 2, 32)
    assert (off == 0).all()
    z = np.zeros(5, np.int64)
    _, off, _, _ = _run(cuda, np.arange(5, dtype=np.uint32), _pack(z, z, z, z), 3, 2, 32)      # five Gaussians, no tile
    assert (off == 0).all()


def _random_case(key_bits, V=5000, tw=7, th=5, seed=0):
    rng = np.random.default_rng(seed)
    w, h = rng.integers(1, 4, V), rng.integers(1, 4, V)
    x0, y0 = rng.integers(0, tw, V), rng.integers(0, th, V)
    x1, y1 = np.minimum(x0 + w, tw), np.minimum(y0 + h, th)
    hit0 = (x0 == 0) & (y0 == 0)                                  # first tile empty: move those one tile to the right
    x0 = np.where(hit0, 1, x0); x1 = np.maximum(x1, x0 + 1)
    x1[-1], y1[-1], x0[-1], y0[-1] = tw, th, tw - 1, th - 1      # last tile non-empty
    if key_bits == 24:
        keys = rng.integers(0, 1 << 24, V, dtype=np.uint32)
    else:
        keys = rng.integers(0, 1 << 32, V, dtype=np.uint32) | np.uint32(0x80000000 * (np.arange(V) % 3 == 0))
    keys[: V // 10] = keys[0]                                     # a run of ties
    return keys, _pack(x0, y0, x1, y1), tw, th


@pytest.mark.parametrize("key_bits", [24, 32])
@pytest.mark.parametrize("mode", ["exact", "capacity"])
def test_random(cuda, key_bits, mode):
    keys, rects, tw, th = _random_case(key_bits)
    _, off, counts, I = _reference(keys, rects, tw, th, key_bits)
    assert counts[0] == 0 and counts[-1] > 0
    if mode == "exact":
        _check(cuda, keys, rects, tw, th, key_bits)
    else:
        _check(cuda, keys, rects, tw, th, key_bits, cap=((I + 4095) // 4096) * 4096 + 4096, v_extra=777)


@pytest.mark.parametrize("distinct", [1, 3])
def test_ties(cuda, distinct):
    """3 000 Gaussians on all four tiles of a 2 x 2 grid, keys all equal / three values: the slots break the ties, and three calls agree"""
    V = 3000
    rng = np.random.default_rng(5)
    keys = (rng.integers(0, distinct, V).astype(np.uint32) * np.uint32(1000)) + np.uint32(77)
    z = np.zeros(V, np.int64)
    rects = _pack(z, z, z + 2, z + 2)
    a = _check(cuda, keys, rects, 2, 2, 32)
    b = _check(cuda, keys, rects, 2, 2, 32)
    c = _check(cuda, keys, rects, 2, 2, 32)
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_class_boundaries(cuda):
    """for every class capacity C of the segment sort: one tile with C - 1, C and C + 1 items, keys from 16 values"""
    rng = np.random.default_rng(11)
    for cap in _classes():
        for n in (cap - 1, cap, cap + 1):
            if n < 1:
                continue
            keys = rng.integers(0, 16, n).astype(np.uint32) << np.uint32(9)
            o = np.ones(n, np.int64)
            _check(cuda, keys, _pack(o, 0 * o, o + 1, o), 3, 1, 32)      # the middle tile of a 3 x 1 grid


def test_general_path(cuda):
    """1 x 1 grid, V = 20 000: one segment longer than the largest class"""
    V = 20000
    assert V > max(_classes())
    rng = np.random.default_rng(13)
    keys = rng.integers(0, 1 << 24, V, dtype=np.uint32)
    keys[5000:9000] = keys[5000]
    z = np.zeros(V, np.int64)
    _check(cuda, keys, _pack(z, z, z + 1, z + 1), 1, 1, 24)


def test_overflow(cuda):
    """cap = I - 100: status reports {ENOSPC, I, V}, nothing behind cap is written, every offset <= cap; contents unspecified"""
    keys, rects, tw, th = _random_case(32, seed=3)
    _, _, _, I = _reference(keys, rects, tw, th, 32)
    cap = I - 100
    flat, off, status, _ = _run(cuda, keys, rects, tw, th, 32, cap=cap, v_extra=0)
    assert status[0] != 0 and status[1] == I and status[2] == len(keys) and status[3] == 0       # {ENOSPC, required I, V seen, -}
    assert (flat[cap:] == SENTINEL).all() and len(flat) == cap + GUARD
    assert (off >= 0).all() and (off <= cap).all() and (np.diff(off) >= 0).all()
    assert (flat[:cap] >= 0).all() and (flat[:cap] < len(keys)).all()       # still valid rows for whoever gathers by them
