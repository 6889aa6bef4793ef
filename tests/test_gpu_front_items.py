"""GPU parity of the front kernel with several Gaussians per thread (csrc/gs_front.hip: a chunk of the chained scan is
GS_FRONT_BLOCK x GS_FRONT_ITEMS Gaussians) and of the stream build (build_stream_packed_kernel, csrc/gs_raster.hip) at counts
around the sizes a several-records-per-lane form of it would block by (one was measured and not kept: DESIGN.md section 6):
  gs_front_fwd  == gs_shade_fwd + gs_project_fwd_vis (+ tile rectangles), bit for bit, at Gaussian counts around the chunk size, on
                   a scene whose culled rows are interleaved with the visible ones (packed slot != Gaussian index), in every mode,
                   as a geometry-only launch followed by a records launch, with 24-bit keys and with clipped tile rectangles;
  record stream == a gather of the per-visible records by flatten_ids, through the workspace layout of gs_raster_ws_bytes
                   ([rec0 | rec1 | rec2 | ...], every segment 256-byte aligned), entries behind the device count untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.util import proj_budget_scene, proj_camera

pytestmark = pytest.mark.gpu

W, H = 120, 88                       # 8 x 6 tiles, neither a multiple of 16
MODES = ("pbr", "specular", "diffuse")


def _chunk():
    """C = GS_FRONT_BLOCK * GS_FRONT_ITEMS, read from the source the library was built from"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geosplatting_amd", "csrc", "gs_front.hip")).read()
    block = int(re.search(r"^#define GS_FRONT_BLOCK (\d+)", src, re.M).group(1))
    items = int(re.search(r"^#define GS_FRONT_ITEMS (\d+)", src, re.M).group(1))
    assert block % 64 == 0 and items >= 1
    return block * items


C_ = _chunk()
SIZES = (37, C_, C_ + 1, 3 * C_ + 517, 5 * C_ - 1)
_cache = {}


def _scene(cuda):
    """5C - 1 Gaussians of the projection-budget regimes (tests/util.py) in one random order, a quarter of them built to be culled
    (behind the camera, before the near plane, off screen), with random shading attributes; a prefix of it is a scene of its own."""
    if "scene" not in _cache:
        n_total = 5 * C_ - 1
        n_culled = n_total // 4
        n_per = (n_total - n_culled + 9) // 10
        view = proj_camera(0.4, 0.0, 0.0, (0.5, -0.2, -1.0), W, H, 90.0, 100.0, 54.0, 50.0)
        sc = proj_budget_scene("front_items", [view], n_per=n_per, n_culled=n_culled)
        g = torch.Generator().manual_seed(21)
        n = len(sc["regime"])
        assert n >= n_total
        d = lambda a: torch.as_tensor(a).to(cuda).contiguous()
        vm = torch.as_tensor(view["viewmat"])
        x = dict(means=d(sc["means"]), quats=d(sc["quats"]), scales=d(sc["scales"]), opac=d(sc["opacities"]),
                 normals=d(torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)), kd=d(torch.rand(n, 3, generator=g)),
                 ks=d(torch.rand(n, 2, generator=g)), vm=d(vm), K=d(view["K"]), cam_pos=d(-(vm[:3, :3].T @ vm[:3, 3])), W=W, H=H)
        _cache["scene"] = x
    return _cache["scene"]


def _env(cuda):
    import geosplatting_amd as gs
    if "env" not in _cache:
        g = torch.Generator().manual_seed(3)
        levels = [(torch.rand(6, r, r, 3, generator=g) + 0.05).to(cuda) for r in (64, 32, 16)]
        base = (torch.rand(6, 16, 16, 3, generator=g) + 0.05).to(cuda)
        _cache["env"] = gs.TextureSplitSum(base, levels)
    return _cache["env"]


def _rows(x, rows):
    """the scene of the Gaussians `rows` (ascending indices into the whole scene)"""
    y = dict(x)
    idx = torch.as_tensor(rows, device=x["means"].device)
    for k in ("means", "quats", "scales", "opac", "normals", "kd", "ks"):
        y[k] = x[k][idx].contiguous()
    return y


def _prefix(x, n):
    return _rows(x, np.arange(n))


def _restrict(ref, rows):
    """the reference of the scene _rows(x, rows): the visible Gaussians among `rows`, their ids renumbered"""
    sel = np.isin(ref["gaussian_ids"], rows)
    out = {k: v[sel] for k, v in ref.items() if k != "colors"}
    out["gaussian_ids"] = np.searchsorted(rows, ref["gaussian_ids"][sel]).astype(np.int32)
    out["colors"] = ref["colors"][rows]
    return out


def _reference(cuda, mode):
    """the op-by-op path on the WHOLE scene, once per mode: shading and projection are per Gaussian, so the reference of a subset
    of its rows is a part of it (_restrict)"""
    key = ("ref", mode)
    if key not in _cache:
        import geosplatting_amd as gs
        x, env = _scene(cuda), _env(cuda)
        col = gs.shade(x["means"], x["normals"], x["kd"], x["ks"], x["cam_pos"], env, min_roughness=0.1, max_metallic=1.0, mode=mode)
        _, _, meta = gs.rasterization(x["means"], x["quats"], x["scales"], x["opac"], col, x["vm"][None], x["K"][None], W, H)
        m = {k: meta[k].cpu().numpy() for k in ("gaussian_ids", "means2d", "conics", "opacities", "compensations", "depths", "radii",
                                                 "tiles_per_gauss")}
        m["colors"] = col.detach().cpu().numpy()
        _cache[key] = m
    return _cache[key]


def _square_rects(m2, radii):
    """tile_range_exact (gs_project_dev.h) in float32: (x0, y0, x1, y1) of gsplat's tile square"""
    ts = np.float32(16.0)
    tw, th = (W + 15) // 16, (H + 15) // 16
    tr = radii.astype(np.float32) / ts
    tx, ty = m2[:, 0] / ts, m2[:, 1] / ts
    lo = lambda f, hi: np.where(f < 0, 0, np.where(f > hi, hi, f)).astype(np.int64)
    return (lo(np.floor(tx - tr), tw), lo(np.floor(ty - tr), th), lo(np.ceil(tx + tr), tw), lo(np.ceil(ty + tr), th))


def _unpack_rects(rects):
    rc = rects.cpu().numpy().view(np.uint32).astype(np.int64)
    return rc[:, 0] & 0xffff, rc[:, 0] >> 16, rc[:, 1] & 0xffff, rc[:, 1] >> 16


def _tile_histogram(x0, y0, x1, y1):
    tw, th = (W + 15) // 16, (H + 15) // 16
    h = np.zeros((th, tw), np.int64)
    for a, b, c, d in zip(x0, y0, x1, y1):
        h[b:d, a:c] += 1
    return h.reshape(-1)


def _front(x, cuda, mode="pbr", **kw):
    import geosplatting_amd as gs
    from geosplatting_amd import front as F
    from geosplatting_amd.shading import _MODE, _make_env
    records = kw.get("records", True)
    e = _make_env(gs.get_fg_lut(cuda), _env(cuda)) if records else None
    fr = F.front_stage(x["means"], x["quats"], x["scales"], x["opac"], x["normals"], x["kd"], x["ks"], x["vm"], x["K"], x["cam_pos"], e,
                       x["W"], x["H"], 0.1, 1.0, _MODE[mode], want_packed_index=True, **kw)
    torch.cuda.synchronize()
    return fr


def _check_against_reference(fr, ref, n, with_records=True, with_binning=True):
    """`ref`: the reference of exactly the n Gaussians the front was given (_restrict)"""
    sel = slice(None)
    gid = ref["gaussian_ids"].astype(np.int32)
    V = len(gid)
    counts = fr.counts.cpu().numpy()
    assert int(counts[0]) == V
    assert 0 < V < n or n < 64                                                   # culled rows inside: slots differ from indices
    pidx = fr.packed_index[:n].cpu().numpy()
    want_pidx = np.full(n, -1, np.int32); want_pidx[gid] = np.arange(V, dtype=np.int32)
    assert np.array_equal(pidx, want_pidx)
    bits = ref["depths"][sel].view(np.uint32)
    if V:
        assert 0xffffffff - int(counts[2]) == int(bits.min()) and int(counts[3]) == int(bits.max())
    if with_records:
        vis = fr.vis[:V].cpu().numpy()
        m2, con = ref["means2d"][sel], ref["conics"][sel]
        assert np.array_equal(np.ascontiguousarray(vis[:, 13]).view(np.int32), gid)
        assert np.array_equal(vis[:, 0:2], m2)
        assert np.array_equal(vis[:, 2], 0.5 * con[:, 0]) and np.array_equal(vis[:, 3], con[:, 1]) and np.array_equal(vis[:, 4], 0.5 * con[:, 2])
        assert np.array_equal(vis[:, 5], ref["opacities"][sel])
        assert np.array_equal(vis[:, 8:11], ref["colors"][gid])
        assert np.array_equal(vis[:, 12], ref["compensations"][sel])
        assert np.array_equal(vis[:, 14], ref["depths"][sel])
        assert np.array_equal(np.ascontiguousarray(vis[:, 15]).view(np.int32), ref["radii"][sel])
    if with_binning:
        assert np.array_equal(fr.keys[:V].cpu().numpy().view(np.uint32), bits)       # 32-bit keys = the depth bits
        x0, y0, x1, y1 = _unpack_rects(fr.rects[:V])
        wx0, wy0, wx1, wy1 = _square_rects(ref["means2d"][sel], ref["radii"][sel])
        assert np.array_equal(x0, wx0) and np.array_equal(y0, wy0) and np.array_equal(x1, wx1) and np.array_equal(y1, wy1)
        area = (x1 - x0) * (y1 - y0)
        assert np.array_equal(area.astype(np.int32), ref["tiles_per_gauss"][sel])
        assert int(counts[1]) == int(area.sum())
        assert np.array_equal(fr.tile_counts.cpu().numpy().astype(np.int64), _tile_histogram(x0, y0, x1, y1))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_front_items_equal_shade_plus_project(cuda, mode, n):
    ref = _restrict(_reference(cuda, mode), np.arange(n))
    fr = _front(_prefix(_scene(cuda), n), cuda, mode=mode)
    _check_against_reference(fr, ref, n)


@pytest.mark.parametrize("n", (C_ + 1, 3 * C_ + 517))
def test_front_items_geometry_launch_then_records_launch(cuda, n):
    """the engine's first views: a geometry-only launch (vis == NULL: keys, rectangles, tile counts, slots), the records later"""
    ref = _restrict(_reference(cuda, "pbr"), np.arange(n))
    x = _prefix(_scene(cuda), n)
    geo = _front(x, cuda, records=False)
    assert geo.vis is None
    _check_against_reference(geo, ref, n, with_records=False)
    rec = _front(x, cuda, binning=False)
    assert rec.keys is None and rec.tile_counts is None
    _check_against_reference(rec, ref, n, with_binning=False)


def test_front_items_24_bit_keys_report_a_depth_outside_the_range(cuda):
    """24-bit keys (depth bits - base, clamped): the rows of the scene whose depth lies in [2, 8) -- two octaves, 2^24 depth bits --
    and the culled ones fit the range; with ONE Gaussian of the near-plane regime among them the status word is set and its key
    clamps to 0.  Everything else stays what the 32-bit launch writes."""
    n = 3 * C_ + 517
    full = _reference(cuda, "pbr")
    n_all = full["colors"].shape[0]
    depth = np.full(n_all, np.nan, np.float32); depth[full["gaussian_ids"]] = full["depths"]
    near = np.nonzero(depth < 2.0)[0]
    far = np.nonzero(~(depth < 2.0))[0][:n]                                      # visible in [2, 8) or culled
    assert len(far) == n and len(near) > 10 and np.nanmax(depth) < 8.0
    base = int(np.float32(2.0).view(np.uint32))
    status = torch.zeros(4, dtype=torch.int64, device=cuda)
    for rows, outside in ((far, 0), (np.sort(np.append(far[:-1], near[len(near) // 2])), 1)):
        ref = _restrict(full, rows)
        bits = ref["depths"].view(np.uint32).astype(np.int64)
        assert int((bits < base).sum()) == outside and int(bits.max()) - base < (1 << 24)
        status.zero_()
        fr = _front(_rows(_scene(cuda), rows), cuda, key_base=base, key_bits=24, status=status)
        assert status.cpu().tolist() == [0, 0, 0, outside]
        V = len(bits)
        assert np.array_equal(fr.keys[:V].cpu().numpy().view(np.uint32).astype(np.int64), np.where(bits < base, 0, bits - base))
        _check_against_reference(fr, ref, n, with_binning=False)
        x0, y0, x1, y1 = _unpack_rects(fr.rects[:V])
        assert int(fr.counts[1]) == int(((x1 - x0) * (y1 - y0)).sum())
        assert np.array_equal(fr.tile_counts.cpu().numpy().astype(np.int64), _tile_histogram(x0, y0, x1, y1))


def test_front_items_tight_tiles(cuda):
    """rectangles clipped to the alpha extents: same records, keys and slots as the square launch, every rectangle inside its square,
    fewer intersections, and tile_counts / counts[1] the histogram / the sum of the rectangles written"""
    n = 5 * C_ - 1
    ref = _restrict(_reference(cuda, "pbr"), np.arange(n))
    x = _prefix(_scene(cuda), n)
    sq = _front(x, cuda)
    tt = _front(x, cuda, tight_tiles=True)
    V = int(sq.counts[0])
    assert int(tt.counts[0]) == V and torch.equal(sq.vis[:V], tt.vis[:V]) and torch.equal(sq.keys[:V], tt.keys[:V])
    assert torch.equal(sq.packed_index, tt.packed_index) and torch.equal(sq.counts[2:], tt.counts[2:])
    _check_against_reference(tt, ref, n, with_binning=False)
    sx0, sy0, sx1, sy1 = _unpack_rects(sq.rects[:V])
    x0, y0, x1, y1 = _unpack_rects(tt.rects[:V])
    ne = (x1 > x0) & (y1 > y0)
    assert (x0[ne] >= sx0[ne]).all() and (y0[ne] >= sy0[ne]).all() and (x1 <= sx1).all() and (y1 <= sy1).all()
    area = (x1 - x0) * (y1 - y0)
    assert 0 < int(area.sum()) == int(tt.counts[1]) < int(sq.counts[1])
    assert np.array_equal(tt.tile_counts.cpu().numpy().astype(np.int64), _tile_histogram(x0, y0, x1, y1))


# ---------------------------------------------------------------------------------------------------------------- stream build
def _align256(b):
    return (b + 255) & ~255


@pytest.mark.parametrize("I", (1, 200, 3 * 1024 - 1, 2 * 1024, 2 * 1024 + 1, 5 * 1024 + 255))
@pytest.mark.parametrize("capacity", (False, True))
def test_stream_build_equals_gather_of_records(cuda, I, capacity):
    from geosplatting_amd import _lib as L
    lib = L.lib()
    V, Wt, Ht = 3000, 64, 64
    g = torch.Generator().manual_seed(100 + I)
    vis = (torch.rand(V, 16, generator=g) * 8 - 4).to(cuda)
    cap = I + 1500 if capacity else I                                            # capacity mode: the grid covers blocks behind the count
    flat = torch.randint(0, V, (cap,), generator=g, dtype=torch.int32).to(cuda)
    offsets = torch.div(torch.arange(16, dtype=torch.int64) * I, 16, rounding_mode="floor").to(torch.int32).to(cuda)
    counts = torch.tensor([V, I, 0, 0], dtype=torch.int64, device=cuda)
    nbytes = lib.gs_raster_ws_bytes(L.i64(cap), V, Wt, Ht, 16)
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=cuda)
    if capacity:
        L.check(lib.gs_raster_prepare_vis_cap(Wt, Ht, 16, 3, V, L.ptr(vis), L.i64(cap), L.ptr(counts), L.ptr(offsets), L.ptr(flat), L.ptr(ws),
                                              C.c_size_t(nbytes), L.stream()), "gs_raster_prepare_vis_cap")
    else:
        L.check(lib.gs_raster_prepare_vis(Wt, Ht, 16, 3, V, L.ptr(vis), L.i64(I), L.ptr(offsets), L.ptr(flat), L.ptr(ws), C.c_size_t(nbytes),
                                          L.stream()), "gs_raster_prepare_vis")
    torch.cuda.synchronize()
    seg = _align256(cap * 16)
    ids = flat[:I].long()
    want = [vis[ids, 0:4], vis[ids, 4:8], torch.cat([vis[ids, 8:11], flat[:I].view(torch.float32)[:, None]], 1)]
    for k in range(3):
        got = ws[k * seg:(k + 1) * seg]
        assert torch.equal(got[:I * 16].view(torch.int32), want[k].contiguous().view(-1).view(torch.int32)), k
        assert bool((got[I * 16:] == 0x5a).all()), k                             # entries behind the count, and the padding: untouched
