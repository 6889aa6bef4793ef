"""Drop-in for the rasterizer boundary of the reference: ``gsplat.rasterization`` exactly as it is called at
rfstudio/model/gsplat.py:334-355 (and :240-261; rfstudio/model/geosplat.py:276-295 with D=14).

Same argument names / meaning / return triple ``(render[1,H,W,D], alpha[1,H,W,1], meta)``; differentiable
w.r.t. means / quats / scales / opacities / colors and, when it requires grad, viewmats (Ks has no gradient).  Every stage runs in libgeosplat_hip.so (hand-written HIP
for gfx950) through the C-ABI in include/geosplat_hip.h -- there is no PyTorch or CPU fallback.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L

_META_KEYS = ("gaussian_ids_i32", "radii", "means2d", "depths", "conics", "compensations", "opacities", "colors",
              "tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets", "last_ids", "raster_ws")


class _Projected:
    """Outputs of the projection stage (A1 + A1' + A2 count) of one view, with the (V, I) counts on their way to a
    pinned host buffer.  Nothing here blocks: `counts()` waits for the copy only when the sizes are needed, so a
    caller can launch the projection of view i+1 before it finishes view i (engine.RenderStep does)."""
    __slots__ = ("args", "bufs", "host_counts", "event", "D", "vis")


_pinned_pool = []

GS_PROJ_CLASSIC = 1           # include/geosplat_hip.h


# "depth_major" (gs_isect_bin) or "emit_sort" (gs_isect_emit + gs_isect_sort: the upstream call shape, kept for callers that hold
# emitted keys; tests compare the two bit for bit)
BINNING = "depth_major"

def _project_stage(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Optional[Tensor],
                   viewmat: Tensor, K: Tensor, W: int, H: int, tile_size: int, eps2d: float, near: float,
                   far: float, radius_clip: float, sh_degree: Optional[int] = None, classic: bool = False) -> _Projected:
    """sh_degree set: `colors` holds SH coefficients [N, K, 3] and 3 colour channels are evaluated.  classic: no compensation
    factor on the packed opacities (gsplat rasterize_mode='classic')."""
    lib = L.lib()
    dev = means.device
    N, D = means.shape[0], (3 if sh_degree is not None else 0 if colors is None else colors.shape[1])
    i32, f32 = torch.int32, torch.float32
    gids = torch.empty(N, dtype=i32, device=dev); radii = torch.empty(N, dtype=i32, device=dev)
    means2d = torch.empty(N, 2, dtype=f32, device=dev); depths = torch.empty(N, dtype=f32, device=dev)
    conics = torch.empty(N, 3, dtype=f32, device=dev); comps = torch.empty(N, dtype=f32, device=dev)
    opac_p = torch.empty(N, dtype=f32, device=dev)
    colors_p = torch.empty(N, D, dtype=f32, device=dev) if D > 0 else None
    tpg = torch.empty(N, dtype=i32, device=dev); cum = torch.empty(N, dtype=torch.int64, device=dev)
    ws_bytes = lib.gs_project_ws_bytes(N)
    ws = L.workspace(ws_bytes, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    # the compositor's 64-byte per-visible records come straight out of the projection (colours ride along for D <= 3)
    vis = torch.empty(N, 16, dtype=f32, device=dev) if (0 < D <= 3 and N > 0) else None
    st = L.stream()
    if sh_degree is None and not classic:
        L.check(lib.gs_project_fwd_vis(N, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(colors), D,
                                       L.ptr(viewmat), L.ptr(K), W, H, tile_size, eps2d, near, far, radius_clip, L.ptr(gids),
                                       L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(conics), L.ptr(comps), L.ptr(opac_p),
                                       L.ptr(colors_p), L.ptr(tpg), L.ptr(cum), None, L.ptr(vis), L.ptr(ws), ws_bytes,
                                       L.ptr(counts), st), "gs_project_fwd_vis")
    else:
        sh = sh_degree is not None
        L.check(lib.gs_project_fwd_vis_ex(N, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), None if sh else L.ptr(colors),
                                          D, L.ptr(colors) if sh else None, colors.shape[1] if sh else 0, -1 if not sh else sh_degree,
                                          GS_PROJ_CLASSIC if classic else 0, L.ptr(viewmat), L.ptr(K), W, H, tile_size, eps2d, near,
                                          far, radius_clip, L.ptr(gids), L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(conics),
                                          L.ptr(comps), L.ptr(opac_p), L.ptr(colors_p), L.ptr(tpg), L.ptr(cum), None, L.ptr(vis),
                                          L.ptr(ws), ws_bytes, L.ptr(counts), st),
                "gs_project_fwd_vis_ex")
    pr = _Projected()
    pr.host_counts = _pinned_pool.pop() if _pinned_pool else torch.empty(2, dtype=torch.int64).pin_memory()
    pr.host_counts.copy_(counts, non_blocking=True)          # 16 bytes, asynchronous
    pr.event = torch.cuda.Event()
    pr.event.record()
    pr.bufs = (gids, radii, means2d, depths, conics, comps, opac_p, colors_p, tpg, cum, counts)
    pr.vis = vis
    pr.args = (W, H, tile_size)
    pr.D = D
    return pr


def _bin_stage(pr: _Projected, depth_channel: bool = False):
    """A2 emit, A3 sort, A4 offsets for a projected view; waits for its (V, I) -- the one host sync of the forward
    (as upstream).  Returns the state dict without the compositor outputs."""
    lib = L.lib()
    W, H, tile_size = pr.args
    gids, radii, means2d, depths, conics, comps, opac_p, colors_p, tpg, cum, _ = pr.bufs
    dev = means2d.device
    D = pr.D
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    i32 = torch.int32
    st = L.stream()
    pr.event.synchronize()
    V, I = (int(x) for x in pr.host_counts.tolist())
    _pinned_pool.append(pr.host_counts)
    if V < 0 or I < 0 or I >= 2 ** 31:
        raise L.GeoSplatHipError(f"bad intersection count V={V} I={I}")
    gids, radii, means2d, depths = gids[:V], radii[:V], means2d[:V], depths[:V]
    conics, comps, opac_p, tpg, cum = conics[:V], comps[:V], opac_p[:V], tpg[:V], cum[:V]
    colors_p = colors_p[:V] if colors_p is not None else None
    if depth_channel:
        colors_p = depths.unsqueeze(-1).clone() if colors_p is None else torch.cat((colors_p, depths.unsqueeze(-1)), dim=1)
        D = D + 1
    colors_p = colors_p.contiguous()

    ids_s = torch.empty(I, dtype=torch.int64, device=dev); flat_s = torch.empty(I, dtype=i32, device=dev)
    if BINNING == "emit_sort":                                                   # the upstream call shape: emit, then sort the pairs
        ids = torch.empty(I, dtype=torch.int64, device=dev); flat = torch.empty(I, dtype=i32, device=dev)
        L.check(lib.gs_isect_emit(V, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(cum), tile_size, tw, th,
                                  L.ptr(ids), L.ptr(flat), st), "gs_isect_emit")
        sort_bytes = lib.gs_sort_ws_bytes(I, tw, th)
        sort_ws = L.workspace(max(sort_bytes, 1), dev)
        L.check(lib.gs_isect_sort(I, L.ptr(ids), L.ptr(flat), L.ptr(ids_s), L.ptr(flat_s), tw, th, L.ptr(sort_ws),
                                  sort_bytes, st), "gs_isect_sort")
    else:                                                                        # depth-major binning (csrc/gs_sort.hip)
        bin_bytes = lib.gs_isect_bin_ws_bytes(V, I, tw, th)
        bin_ws = L.workspace(max(bin_bytes, 1), dev)
        L.check(lib.gs_isect_bin(V, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(tpg), I, tile_size, tw, th,
                                 L.ptr(ids_s), L.ptr(flat_s), L.ptr(bin_ws), bin_bytes, st), "gs_isect_bin")
    offsets = torch.empty(th * tw, dtype=i32, device=dev)
    L.check(lib.gs_isect_offsets(I, L.ptr(ids_s), tw * th, L.ptr(offsets), st), "gs_isect_offsets")
    state = dict(gaussian_ids_i32=gids, radii=radii, means2d=means2d, depths=depths, conics=conics,
                 compensations=comps, opacities=opac_p, colors=colors_p, tiles_per_gauss=tpg, isect_ids=ids_s,
                 flatten_ids=flat_s, isect_offsets=offsets)
    if pr.vis is not None and not depth_channel:             # (a depth channel changes the composited colours after the projection)
        state["vis_records"] = pr.vis
    return state, V, I, D, (W, H, tile_size)


def _prepare_stage(state, V: int, I: int, D: int, whs):
    """A5 preparation (per-visible records, sorted record stream, tile order) on the current stream."""
    lib = L.lib()
    W, H, tile_size = whs
    rws_bytes = lib.gs_raster_ws_bytes(I, V, W, H, tile_size)
    rws = L.workspace(rws_bytes, state["means2d"].device)   # written here, read by fwd AND bwd
    vis = state.get("vis_records")
    if vis is not None:
        L.check(lib.gs_raster_prepare_vis(W, H, tile_size, D, V, L.ptr(vis), I, L.ptr(state["isect_offsets"]),
                                          L.ptr(state["flatten_ids"]), L.ptr(rws), rws_bytes, L.stream()),
                "gs_raster_prepare_vis")
    else:
        L.check(lib.gs_raster_prepare(W, H, tile_size, D, V, L.ptr(state["means2d"]), L.ptr(state["conics"]),
                                      L.ptr(state["opacities"]), L.ptr(state["colors"]), I,
                                      L.ptr(state["isect_offsets"]), L.ptr(state["flatten_ids"]), L.ptr(rws),
                                      rws_bytes, L.stream()), "gs_raster_prepare")
    return dict({k: v for k, v in state.items() if k != "vis_records"}, raster_ws=rws)


def _composite_stage(state, V: int, I: int, D: int, whs, background: Optional[Tensor]):
    """A5 proper (the compositor) on the current stream; prepares the workspace first if the caller has not."""
    lib = L.lib()
    W, H, tile_size = whs
    dev = state["means2d"].device
    i32, f32 = torch.int32, torch.float32
    if "raster_ws" not in state:
        state = _prepare_stage(state, V, I, D, whs)
    rws = state["raster_ws"]
    render = torch.empty(H, W, D, dtype=f32, device=dev); alphas = torch.empty(H, W, dtype=f32, device=dev)
    last_ids = torch.empty(H, W, dtype=i32, device=dev)
    L.check(lib.gs_raster_composite(W, H, tile_size, D, V, L.ptr(state["colors"]), L.ptr(background), I,
                                    L.ptr(state["isect_offsets"]), L.ptr(render), L.ptr(alphas), L.ptr(last_ids),
                                    L.ptr(rws), rws.numel(), L.stream()), "gs_raster_composite")
    state = dict(state, last_ids=last_ids)
    return render, alphas, state, V, I


# ---- capacity protocol (include/geosplat_hip.h): the same three stages without the (V, I) read-back --------------------------
def _bin_stage_cap(pr: _Projected, I_cap: int, status: Tensor, want_ids: bool = True):
    """A2-A4 with the counts left on the device: buffers, workspaces and grids are sized by (N, I_cap), the kernels read
    (V, I) from pr's device counts; an overflow is reported in `status` (int64[3], sticky), never written out of bounds."""
    lib = L.lib()
    W, H, tile_size = pr.args
    gids, radii, means2d, depths, conics, comps, opac_p, colors_p, tpg, cum, counts = pr.bufs
    dev = means2d.device
    N = means2d.shape[0]
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    st = L.stream()
    flat_s = torch.empty(I_cap, dtype=torch.int32, device=dev)
    bin_bytes = lib.gs_isect_bin_ws_bytes(N, I_cap, tw, th)
    bin_ws = L.workspace(max(bin_bytes, 1), dev)
    offsets = torch.empty(th * tw, dtype=torch.int32, device=dev)
    if want_ids:
        ids_s = torch.empty(I_cap, dtype=torch.int64, device=dev)
        L.check(lib.gs_isect_bin_cap(N, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(counts), I_cap, tile_size, tw, th,
                                     L.ptr(ids_s), L.ptr(flat_s), L.ptr(bin_ws), bin_bytes, L.ptr(status), st),
                "gs_isect_bin_cap")
        L.check(lib.gs_isect_offsets_cap(I_cap, L.ptr(counts), L.ptr(ids_s), tw * th, L.ptr(offsets), st), "gs_isect_offsets_cap")
    else:                      # the caller only composites: int32 tile ids instead of the 64-bit keys (the `isect_ids` entry holds them)
        ids_s = torch.empty(I_cap, dtype=torch.int32, device=dev)
        L.check(lib.gs_isect_bin_tiles_cap(N, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(counts), I_cap, tile_size, tw, th,
                                           L.ptr(ids_s), L.ptr(flat_s), L.ptr(bin_ws), bin_bytes, L.ptr(status), st),
                "gs_isect_bin_tiles_cap")
        L.check(lib.gs_isect_offsets_tiles_cap(I_cap, L.ptr(counts), L.ptr(ids_s), tw * th, L.ptr(offsets), st),
                "gs_isect_offsets_tiles_cap")
    state = dict(gaussian_ids_i32=gids, radii=radii, means2d=means2d, depths=depths, conics=conics, compensations=comps,
                 opacities=opac_p, colors=colors_p, tiles_per_gauss=tpg, isect_ids=ids_s, flatten_ids=flat_s,
                 isect_offsets=offsets, counts=counts, vis_records=pr.vis)
    return state, N, I_cap, pr.D, (W, H, tile_size)


def _prepare_stage_cap(state, V_cap: int, I_cap: int, D: int, whs):
    lib = L.lib()
    W, H, tile_size = whs
    rws_bytes = lib.gs_raster_ws_bytes(I_cap, V_cap, W, H, tile_size)
    rws = L.workspace(rws_bytes, state["means2d"].device)
    L.check(lib.gs_raster_prepare_vis_cap(W, H, tile_size, D, V_cap, L.ptr(state["vis_records"]), I_cap, L.ptr(state["counts"]),
                                          L.ptr(state["isect_offsets"]), L.ptr(state["flatten_ids"]), L.ptr(rws), rws_bytes,
                                          L.stream()), "gs_raster_prepare_vis_cap")
    return dict({k: v for k, v in state.items() if k != "vis_records"}, raster_ws=rws)


def _composite_stage_cap(state, V_cap: int, I_cap: int, D: int, whs, background: Optional[Tensor]):
    lib = L.lib()
    W, H, tile_size = whs
    dev = state["means2d"].device
    rws = state["raster_ws"]
    render = torch.empty(H, W, D, dtype=torch.float32, device=dev); alphas = torch.empty(H, W, dtype=torch.float32, device=dev)
    last_ids = torch.empty(H, W, dtype=torch.int32, device=dev)
    L.check(lib.gs_raster_composite_cap(W, H, tile_size, D, V_cap, L.ptr(state["colors"]), L.ptr(background), I_cap,
                                        L.ptr(state["counts"]), L.ptr(state["isect_offsets"]), L.ptr(render), L.ptr(alphas),
                                        L.ptr(last_ids), L.ptr(rws), rws.numel(), L.stream()), "gs_raster_composite_cap")
    return render, alphas, dict(state, last_ids=last_ids)


def _raster_stage(pr: _Projected, background: Optional[Tensor], depth_channel: bool = False):
    state, V, I, D, whs = _bin_stage(pr, depth_channel)
    return _composite_stage(state, V, I, D, whs, background)


def _forward_stages(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Optional[Tensor],
                    viewmat: Tensor, K: Tensor, W: int, H: int, tile_size: int, eps2d: float, near: float,
                    far: float, radius_clip: float, background: Optional[Tensor], depth_channel: bool = False,
                    sh_degree: Optional[int] = None, classic: bool = False):
    """A1..A5 through the C-ABI.  depth_channel appends the camera-space depth of every visible Gaussian as one
    more composited channel (gsplat render modes 'D' / 'ED' / 'RGB+D' / 'RGB+ED'; colors may be None for 'D'/'ED')."""
    pr = _project_stage(means, quats, scales, opacities, colors, viewmat, K, W, H, tile_size, eps2d, near, far, radius_clip,
                        sh_degree, classic)
    return _raster_stage(pr, background, depth_channel)


def _project_backward(saved, cfg, st, v_packed: Tensor, want_viewmat: bool = False):
    """A7 for one view from the compositor's packed gradients v_packed [V, stride]: gradients of (means, quats, scales,
    opacities, colors); `colors` are the SH coefficients [N, K, 3] when sh_degree is set.  want_viewmat: through
    gs_project_bwd_view, which writes the same five and the gradient of the view matrix [4, 4], returned as a sixth (else None)."""
    lib = L.lib()
    W, H, eps2d, V, depth_channel, sh_degree, classic = cfg
    means, quats, scales, opacities, colors, viewmat, K = saved
    dev = means.device
    N = means.shape[0]
    f32 = torch.float32
    sh = sh_degree is not None
    Dc = 3 if sh else 0 if colors is None else colors.shape[1]     # composited colour channels
    stride = v_packed.shape[1]
    s = L.stream()
    g_means = torch.empty(N, 3, dtype=f32, device=dev); g_quats = torch.empty(N, 4, dtype=f32, device=dev)
    g_scales = torch.empty(N, 3, dtype=f32, device=dev); g_opac = torch.empty(N, dtype=f32, device=dev)
    g_colors = torch.empty_like(colors) if colors is not None else None
    v_depths = v_packed[:, 6 + Dc].contiguous() if depth_channel else None   # grad of the appended depth channel
    if want_viewmat:
        g_view = torch.empty(4, 4, dtype=f32, device=dev)
        ws_bytes = lib.gs_project_bwd_view_ws_bytes(N)
        ws = L.workspace(ws_bytes, dev)
        L.check(lib.gs_project_bwd_view(N, V, Dc, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(viewmat),
                                        L.ptr(K), W, H, eps2d, L.ptr(st["gaussian_ids_i32"]), L.ptr(st["conics"]),
                                        L.ptr(st["compensations"]), L.ptr(v_packed), stride, L.ptr(v_depths),
                                        L.ptr(colors) if sh else None, colors.shape[1] if sh else 0, sh_degree if sh else -1,
                                        GS_PROJ_CLASSIC if classic else 0, L.ptr(g_means), L.ptr(g_quats), L.ptr(g_scales),
                                        L.ptr(g_opac), None if sh else L.ptr(g_colors), L.ptr(g_colors) if sh else None, 0,
                                        L.ptr(g_view), L.ptr(ws), ws_bytes, s), "gs_project_bwd_view")
        return g_means, g_quats, g_scales, g_opac, g_colors, g_view
    if not sh and not classic:
        L.check(lib.gs_project_bwd(N, V, Dc, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(viewmat),
                                   L.ptr(K), W, H, eps2d, L.ptr(st["gaussian_ids_i32"]), L.ptr(st["conics"]),
                                   L.ptr(st["compensations"]), L.ptr(v_packed), stride, L.ptr(v_depths), L.ptr(g_means),
                                   L.ptr(g_quats), L.ptr(g_scales), L.ptr(g_opac), L.ptr(g_colors), 0, s), "gs_project_bwd")
    else:
        L.check(lib.gs_project_bwd_ex(N, V, Dc, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(viewmat),
                                      L.ptr(K), W, H, eps2d, L.ptr(st["gaussian_ids_i32"]), L.ptr(st["conics"]),
                                      L.ptr(st["compensations"]), L.ptr(v_packed), stride, L.ptr(v_depths),
                                      L.ptr(colors) if sh else None, colors.shape[1] if sh else 0, sh_degree if sh else -1,
                                      GS_PROJ_CLASSIC if classic else 0, L.ptr(g_means), L.ptr(g_quats), L.ptr(g_scales),
                                      L.ptr(g_opac), None if sh else L.ptr(g_colors), L.ptr(g_colors) if sh else None, 0, s),
                "gs_project_bwd_ex")
    return g_means, g_quats, g_scales, g_opac, g_colors, None


def _raster_backward(W: int, H: int, tile_size: int, D: int, V: int, I: int, st, background, alphas, v_render, v_alphas):
    """A6: the compositor's backward into the packed per-Gaussian records {v_means2d, v_conics, v_opacity, v_colors}."""
    lib = L.lib()
    dev = alphas.device
    f32 = torch.float32
    v_render = torch.zeros(H, W, D, dtype=f32, device=dev) if v_render is None else v_render.contiguous()
    v_alphas = torch.zeros(H, W, dtype=f32, device=dev) if v_alphas is None else v_alphas.contiguous()
    stride = lib.gs_raster_grad_stride(D)
    v_packed = torch.empty(V, stride, dtype=f32, device=dev)
    rws = st["raster_ws"]
    L.check(lib.gs_raster_bwd(W, H, tile_size, D, V, L.ptr(st["colors"]), L.ptr(background), I, L.ptr(st["isect_offsets"]),
                              L.ptr(alphas), L.ptr(st["last_ids"]), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_packed), L.ptr(rws),
                              rws.numel(), L.stream()), "gs_raster_bwd")
    return v_packed


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, background, W, H, tile_size, eps2d, near, far,
                radius_clip, depth_channel, sh_degree=None, classic=False):
        means, quats, scales = means.contiguous(), quats.contiguous(), scales.contiguous()
        opacities = opacities.contiguous()
        colors = colors.contiguous() if colors is not None else None
        viewmat, K = viewmat.contiguous(), K.contiguous()
        render, alphas, st, V, I = _forward_stages(means, quats, scales, opacities, colors, viewmat, K, W, H, tile_size,
                                                   eps2d, near, far, radius_clip, background, depth_channel, sh_degree, classic)
        ctx.cfg = (W, H, tile_size, eps2d, V, I, depth_channel, sh_degree, classic)
        ctx.save_for_backward(means, quats, scales, opacities, colors, viewmat, K, background, alphas,
                              *[st[k] for k in _META_KEYS])
        outs = (render, alphas) + tuple(st[k] for k in _META_KEYS)
        ctx.mark_non_differentiable(*outs[2:])
        return outs

    @staticmethod
    def backward(ctx, v_render, v_alphas, *_unused):
        W, H, tile_size, eps2d, V, I, depth_channel, sh_degree, classic = ctx.cfg
        (means, quats, scales, opacities, colors, viewmat, K, background, alphas, *meta) = ctx.saved_tensors
        st = dict(zip(_META_KEYS, meta))
        D = render_channels(colors, sh_degree, depth_channel)
        v_packed = _raster_backward(W, H, tile_size, D, V, I, st, background, alphas, v_render, v_alphas)
        grads = _project_backward((means, quats, scales, opacities, colors, viewmat, K),
                                  (W, H, eps2d, V, depth_channel, sh_degree, classic), st, v_packed, ctx.needs_input_grad[5])
        return grads + (None,) * 12


def render_channels(colors: Optional[Tensor], sh_degree: Optional[int], depth_channel: bool) -> int:
    """Composited channels D: the colour channels (3 with SH colours) plus the appended depth."""
    Dc = 3 if sh_degree is not None else 0 if colors is None else colors.shape[1]
    return Dc + (1 if depth_channel else 0)


class _Link:
    """What the two autograd nodes of the means2d_grad=True path hand each other: the binning state (forward) and the
    compositor's packed gradients (backward)."""
    __slots__ = ("state", "v_packed", "stride")


class _ProjectBin(torch.autograd.Function):
    """A1..A4 as their own autograd node, so that the projected `means2d` is a graph tensor (gsplat's info["means2d"], whose
    .grad GSplatter reads for densification).  Backward: A7 from the compositor's v_packed, with its v_means2d columns
    replaced by the incoming means2d gradient -- the same bytes when the compositor is the only consumer."""
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, link, W, H, tile_size, eps2d, near, far, radius_clip,
                depth_channel, sh_degree, classic):
        means, quats, scales = means.contiguous(), quats.contiguous(), scales.contiguous()
        opacities = opacities.contiguous()
        colors = colors.contiguous() if colors is not None else None
        viewmat, K = viewmat.contiguous(), K.contiguous()
        pr = _project_stage(means, quats, scales, opacities, colors, viewmat, K, W, H, tile_size, eps2d, near, far, radius_clip,
                            sh_degree, classic)
        state, V, I, D, whs = _bin_stage(pr, depth_channel)
        link.state, link.v_packed = (state, V, I, D, whs), None
        link.stride = L.lib().gs_raster_grad_stride(D)
        ctx.cfg = (W, H, eps2d, V, depth_channel, sh_degree, classic)
        ctx.link = link
        ctx.save_for_backward(means, quats, scales, opacities, colors, viewmat, K, state["gaussian_ids_i32"], state["conics"],
                              state["compensations"])
        return state["means2d"]

    @staticmethod
    def backward(ctx, v_means2d):
        (means, quats, scales, opacities, colors, viewmat, K, gids, conics, comps) = ctx.saved_tensors
        link = ctx.link
        V = ctx.cfg[3]
        v_packed, link.v_packed = link.v_packed, None
        if v_packed is None:                                  # the image was not part of the loss: only means2d has a gradient
            v_packed = torch.zeros(V, link.stride, dtype=torch.float32, device=means.device)
        if v_means2d is not None and v_means2d.data_ptr() != v_packed.data_ptr():
            v_packed[:, :2] = v_means2d                       # the caller's own means2d terms, summed by autograd
        st = dict(gaussian_ids_i32=gids, conics=conics, compensations=comps)
        grads = _project_backward((means, quats, scales, opacities, colors, viewmat, K), ctx.cfg, st, v_packed, ctx.needs_input_grad[5])
        return grads + (None,) * 13


class _Composite(torch.autograd.Function):
    """A5 of the means2d_grad=True path; its backward (A6) returns the compositor's dL/dmeans2d and leaves the rest of the
    packed gradients to _ProjectBin through the link."""
    @staticmethod
    def forward(ctx, means2d, link, background):
        state, V, I, D, whs = link.state
        render, alphas, st, V, I = _composite_stage(state, V, I, D, whs, background)
        link.state = None
        ctx.cfg = (whs, D, V, I)
        ctx.link = link
        ctx.save_for_backward(background, alphas, st["colors"], st["isect_offsets"], st["last_ids"], st["raster_ws"])
        ctx.mark_non_differentiable(st["last_ids"])
        link.state = st
        return render, alphas, st["last_ids"]

    @staticmethod
    def backward(ctx, v_render, v_alphas, *_unused):
        (W, H, tile_size), D, V, I = ctx.cfg
        background, alphas, colors, offsets, last_ids, rws = ctx.saved_tensors
        st = dict(colors=colors, isect_offsets=offsets, last_ids=last_ids, raster_ws=rws)
        v_packed = _raster_backward(W, H, tile_size, D, V, I, st, background, alphas, v_render, v_alphas)
        ctx.link.v_packed = v_packed
        return v_packed[:, :2], None, None


_ARGS = ("means", "quats", "scales", "opacities", "colors", "viewmats", "Ks", "width", "height", "near_plane", "far_plane",
         "radius_clip", "eps2d", "sh_degree", "packed", "tile_size", "backgrounds", "render_mode", "sparse_grad", "absgrad",
         "rasterize_mode", "means2d_grad")


def rasterization(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmats: Tensor,
                  Ks: Tensor, width: int, height: int, near_plane: float = 0.01, far_plane: float = 1e10,
                  radius_clip: float = 0.0, eps2d: float = 0.3, sh_degree: Optional[int] = None, packed: bool = True,
                  tile_size: int = 16, backgrounds: Optional[Tensor] = None, render_mode: str = "RGB",
                  sparse_grad: bool = False, absgrad: bool = False, rasterize_mode: str = "antialiased",
                  means2d_grad: bool = False) -> Tuple[Tensor, Tensor, Dict]:
    """``gsplat.rasterization`` (1.4, packed, one camera) as GeoSplatting calls it: 'antialiased' only -- any other
    rasterize_mode raises NotImplementedError, as it always has (GSplatter's 'classic' is rasterization_3dgs).  Also takes
    ``sh_degree`` 0..3 with ``colors`` [N, K, 3], K >= (sh_degree+1)^2, and ``means2d_grad`` (see rasterization_3dgs).
    Unsupported options raise (same error behaviour as upstream: Python exceptions)."""
    a = locals()
    return _rasterization(*(a[k] for k in _ARGS), allow_classic=False)


def rasterization_3dgs(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmats: Tensor,
                       Ks: Tensor, width: int, height: int, near_plane: float = 0.01, far_plane: float = 1e10,
                       radius_clip: float = 0.0, eps2d: float = 0.3, sh_degree: Optional[int] = None, packed: bool = True,
                       tile_size: int = 16, backgrounds: Optional[Tensor] = None, render_mode: str = "RGB",
                       sparse_grad: bool = False, absgrad: bool = False, rasterize_mode: str = "classic",
                       means2d_grad: bool = True) -> Tuple[Tensor, Tensor, Dict]:
    """``gsplat.rasterization`` (1.4, packed, one camera) as the reference's vanilla-3DGS model calls it (GSplatter,
    rfstudio/model/gsplat.py:23-36, :240-261, :334-355): rasterize_mode 'classic' (upstream's default) or 'antialiased',
    ``sh_degree`` 0..3 with ``colors`` [N, K, 3], K >= (sh_degree+1)^2 (``meta["colors"]`` = the evaluated [V, 3] colours).

    means2d_grad (not an upstream argument; True here): ``meta["means2d"]`` is a graph tensor that requires grad whenever the
    inputs do; after ``retain_grad()`` and ``backward()`` its ``.grad`` is the compositor's dL/dmeans2d [V, 2] in packed order
    (what GSplatter's densification reads).  The projection and the compositing then run as two autograd nodes; the parameter
    gradients are the same bits as with means2d_grad=False unless the loss uses means2d itself."""
    a = locals()
    return _rasterization(*(a[k] for k in _ARGS), allow_classic=True)


def _rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height, near_plane, far_plane, radius_clip, eps2d,
                   sh_degree, packed, tile_size, backgrounds, render_mode, sparse_grad, absgrad, rasterize_mode, means2d_grad,
                   allow_classic: bool):
    L.require_cuda(means, quats, scales, opacities, colors, viewmats, Ks)
    if viewmats.shape[:-2] != (1,) or Ks.shape[:-2] != (1,):
        raise ValueError("exactly one camera per call (rfstudio/model/gsplat.py:293 asserts cameras.shape == (1,))")
    if render_mode not in ("RGB", "D", "ED", "RGB+D", "RGB+ED"):
        raise ValueError(f"unknown render_mode {render_mode!r}")
    if not allow_classic and rasterize_mode != "antialiased":
        raise NotImplementedError("rasterize_mode 'antialiased' only (rfstudio/model/geosplat.py:796); "
                                  "GSplatter's 'classic' is geosplatting_amd.rasterization_3dgs")
    if rasterize_mode not in ("antialiased", "classic"):
        raise ValueError(f"rasterize_mode must be 'antialiased' or 'classic', not {rasterize_mode!r}")
    if sparse_grad or absgrad:
        raise NotImplementedError("sparse_grad / absgrad are False on the reference path")
    N = means.shape[0]
    assert means.shape == (N, 3) and quats.shape == (N, 4) and scales.shape == (N, 3) and opacities.shape == (N,)
    depth_channel = render_mode != "RGB"
    if render_mode in ("D", "ED"):
        colors, sh_degree = None, None                   # upstream ignores colours in the depth-only modes
    elif sh_degree is not None:
        if not isinstance(sh_degree, int) or sh_degree < 0:
            raise ValueError(f"sh_degree must be None or a degree >= 0, not {sh_degree!r}")
        if sh_degree >= 4:
            raise NotImplementedError("sh_degree 0..3 (degree 4 is not implemented)")
        if colors.dim() != 3 or colors.shape[0] != N or colors.shape[2] != 3 or colors.shape[1] < (sh_degree + 1) ** 2:
            raise ValueError(f"sh_degree={sh_degree} needs colors [N, K, 3] with K >= {(sh_degree + 1) ** 2}, "
                             f"got {tuple(colors.shape)}")
    else:
        assert colors.dim() == 2 and colors.shape[0] == N
    Dc = 0 if colors is None else 3 if sh_degree is not None else colors.shape[1]
    bg = None
    if backgrounds is not None:
        bg = backgrounds.reshape(-1).contiguous().float()
        if depth_channel:                                # upstream pads the background of the depth channel with 0
            bg = torch.cat((bg, bg.new_zeros(1))) if colors is not None else bg.new_zeros(1)
        assert bg.shape[0] == Dc + (1 if depth_channel else 0)
    classic = rasterize_mode == "classic"
    args = (means.float(), quats.float(), scales.float(), opacities.float(), None if colors is None else colors.float(),
            viewmats.reshape(4, 4).float(), Ks.reshape(3, 3).float())
    cfg = (int(width), int(height), int(tile_size), float(eps2d), float(near_plane), float(far_plane), float(radius_clip),
           depth_channel)
    if means2d_grad:
        link = _Link()
        means2d = _ProjectBin.apply(*args, link, *cfg, sh_degree, classic)
        render, alphas, _ = _Composite.apply(means2d, link, bg)
        st = dict(link.state, means2d=means2d)
        link.state = None
    else:
        outs = _Rasterize.apply(*args, bg, *cfg, sh_degree, classic)
        render, alphas = outs[0], outs[1]
        st = dict(zip(_META_KEYS, outs[2:]))
    if render_mode in ("ED", "RGB+ED"):                  # expected depth = accumulated depth / alpha (rfstudio/model/gsplat.py:151-172)
        render = torch.cat((render[..., :-1], render[..., -1:] / alphas.unsqueeze(-1).clamp(min=1e-10)), dim=-1)
    tw, th = (width + tile_size - 1) // tile_size, (height + tile_size - 1) // tile_size
    V = st["radii"].shape[0]
    meta = {
        "camera_ids": torch.zeros(V, dtype=torch.int64, device=means.device),
        "gaussian_ids": st["gaussian_ids_i32"].long(),
        "radii": st["radii"], "means2d": st["means2d"], "depths": st["depths"], "conics": st["conics"],
        "opacities": st["opacities"], "tile_width": tw, "tile_height": th, "tiles_per_gauss": st["tiles_per_gauss"],
        "isect_ids": st["isect_ids"], "flatten_ids": st["flatten_ids"],
        "isect_offsets": st["isect_offsets"].view(1, th, tw), "width": width, "height": height,
        "tile_size": tile_size, "n_cameras": 1,
        # extras (not in upstream's dict)
        "compensations": st["compensations"], "last_ids": st["last_ids"].view(1, height, width),
    }
    if sh_degree is not None:                            # the evaluated colours [V, 3] the compositor received
        meta["colors"] = st["colors"][:, :3]
    return render.unsqueeze(0), alphas.view(1, height, width, 1), meta
