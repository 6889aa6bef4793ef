"""2D Gaussian splatting (surfels): the reference's third rasterize mode.

  rasterization_2dgs(...)  == gsplat.rasterization_2dgs as GSplatter calls it with rasterize_mode='2dgs'
                              (rfstudio/model/gsplat.py:129-150, :217-238, :312-332): same arguments, same seven returns
  SurfelModel              == GSplatter(rasterize_mode='2dgs'): render_rgb on 'RGB+ED' with the distortion map while training,
                              render_depth on 'ED', update_info fed from meta["gradient_2dgs"], the normal-consistency and distortion
                              scalars of :265-279
  SurfelTrainer            == GSplatTrainer with the two regularisers of rfstudio/trainer/gsplat_trainer.py:135-139, :161-164

The surfel projection and the ray-splat compositor, forward and backward, are csrc/gs_surfel.hip; binning, sort, tile offsets, SH
colours, densification statistics and the refinement are the kernels the 3DGS modes run.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib as L
from .cameras import Camera
from .gsplat3d import GSplatModel, GSplatTrainer, UpdateInfo
from .loss import photo_loss
from .shading import _gsplatter_colors

_RENDER_MODES = ("RGB", "D", "ED", "RGB+D", "RGB+ED")


class _Link:
    """What the two autograd nodes hand each other: the projected and binned view (forward), the compositor's packed gradients (backward)."""
    __slots__ = ("state", "v_packed")


def _off(t: Tensor, col: int) -> C.c_void_p:
    """device pointer of column `col` of a contiguous fp32 matrix (the rows keep the matrix's stride)"""
    return C.c_void_p(t.data_ptr() + 4 * col)


def _project_bin(means, quats, scales, opacities, colors, viewmat, K, W, H, tile_size, near, far, radius_clip, sh_degree, depth_channel):
    """surfel projection, the (V, I) read-back, binning and tile offsets of one view"""
    lib, dev, N = L.lib(), means.device, means.shape[0]
    i32, f32 = torch.int32, torch.float32
    sh = sh_degree is not None
    Dc = 3 if sh else 0 if colors is None else colors.shape[1]
    Cn = Dc + (1 if depth_channel else 0)
    gids = torch.empty(N, dtype=i32, device=dev); radii = torch.empty(N, dtype=i32, device=dev)
    means2d = torch.empty(N, 2, dtype=f32, device=dev); depths = torch.empty(N, dtype=f32, device=dev)
    rt = torch.empty(N, 9, dtype=f32, device=dev); normals = torch.empty(N, 3, dtype=f32, device=dev)
    opac_p = torch.empty(N, dtype=f32, device=dev); colors_p = torch.empty(N, Cn, dtype=f32, device=dev)
    tpg = torch.empty(N, dtype=i32, device=dev)
    ws_bytes = lib.gs_surfel_project_ws_bytes(N)
    ws = L.workspace(ws_bytes, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    st = L.stream()
    L.check(lib.gs_surfel_project_fwd(N, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), None if sh else L.ptr(colors), Dc,
                                      L.ptr(colors) if sh else None, colors.shape[1] if sh else 0, sh_degree if sh else -1,
                                      1 if depth_channel else 0, L.ptr(viewmat), L.ptr(K), W, H, tile_size, near, far, radius_clip,
                                      L.ptr(gids), L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(rt), L.ptr(normals),
                                      L.ptr(opac_p), L.ptr(colors_p), L.ptr(tpg), L.ptr(ws), ws_bytes, L.ptr(counts),
                                      st), "gs_surfel_project_fwd")
    V, I = (int(x) for x in counts.tolist())                 # the one host sync of the forward, where upstream has its own
    if V < 0 or V > N or I < 0 or I >= 2 ** 31:
        raise L.GeoSplatHipError(f"bad intersection count V={V} I={I}")
    gids, radii, means2d, depths, rt, normals = gids[:V], radii[:V], means2d[:V], depths[:V], rt[:V], normals[:V]
    opac_p, colors_p, tpg = opac_p[:V], colors_p[:V], tpg[:V]
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    ids_s = torch.empty(I, dtype=torch.int64, device=dev); flat_s = torch.empty(I, dtype=i32, device=dev)
    bin_bytes = lib.gs_isect_bin_ws_bytes(V, I, tw, th)
    bin_ws = L.workspace(max(bin_bytes, 1), dev)
    L.check(lib.gs_isect_bin(V, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(tpg), I, tile_size, tw, th, L.ptr(ids_s),
                             L.ptr(flat_s), L.ptr(bin_ws), bin_bytes, st), "gs_isect_bin")
    offsets = torch.empty(th * tw, dtype=i32, device=dev)
    L.check(lib.gs_isect_offsets(I, L.ptr(ids_s), tw * th, L.ptr(offsets), st), "gs_isect_offsets")
    return dict(gaussian_ids_i32=gids, radii=radii, means2d=means2d, depths=depths, ray_transforms=rt, normals=normals,
                opacities=opac_p, colors=colors_p, tiles_per_gauss=tpg, isect_ids=ids_s, flatten_ids=flat_s, isect_offsets=offsets,
                V=V, I=I, C=Cn, Dc=Dc)


class _SurfelProjectBin(torch.autograd.Function):
    """Projection + binning.  Returns means2d as the graph tensor that ties the compositor's node to this one; backward: the projection
    backward from the compositor's packed gradients, with the incoming means2d gradient in their means2d columns."""
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, link, W, H, tile_size, near, far, radius_clip, sh_degree,
                depth_channel):
        means, quats, scales, opacities = means.contiguous(), quats.contiguous(), scales.contiguous(), opacities.contiguous()
        colors = colors.contiguous() if colors is not None else None
        viewmat, K = viewmat.contiguous(), K.contiguous()
        state = _project_bin(means, quats, scales, opacities, colors, viewmat, K, W, H, tile_size, near, far, radius_clip, sh_degree,
                             depth_channel)
        link.state, link.v_packed = state, None
        ctx.link = link
        ctx.cfg = (state["V"], state["Dc"], state["C"], sh_degree, depth_channel)
        ctx.save_for_backward(means, quats, scales, colors, viewmat, K, state["gaussian_ids_i32"])
        return state["means2d"]

    @staticmethod
    def backward(ctx, v_means2d):
        means, quats, scales, colors, viewmat, K, gids = ctx.saved_tensors
        V, Dc, Cn, sh_degree, depth_channel = ctx.cfg
        lib, dev, N = L.lib(), means.device, means.shape[0]
        stride = lib.gs_surfel_grad_stride()
        v_packed, ctx.link.v_packed = ctx.link.v_packed, None
        if v_packed is None:                                  # the images were not part of the loss
            v_packed = torch.zeros(V, stride, dtype=torch.float32, device=dev)
        if v_means2d is not None and V > 0 and v_means2d.data_ptr() != v_packed.data_ptr() + 4 * 9:
            v_packed[:, 9:11] = v_means2d
        sh = sh_degree is not None
        f32 = torch.float32
        g_means = torch.empty(N, 3, dtype=f32, device=dev); g_quats = torch.empty(N, 4, dtype=f32, device=dev)
        g_scales = torch.empty(N, 3, dtype=f32, device=dev); g_opac = torch.empty(N, dtype=f32, device=dev)
        g_colors = torch.empty_like(colors) if colors is not None else None
        L.check(lib.gs_surfel_project_bwd(N, V, Dc, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(colors) if sh else None,
                                          colors.shape[1] if sh else 0, sh_degree if sh else -1, L.ptr(viewmat), L.ptr(K), L.ptr(gids),
                                          _off(v_packed, 0), _off(v_packed, 9), _off(v_packed, 15 + Cn - 1) if depth_channel else None,
                                          _off(v_packed, 12), _off(v_packed, 11), _off(v_packed, 15), stride, L.ptr(g_means),
                                          L.ptr(g_quats), L.ptr(g_scales), L.ptr(g_opac), None if sh else L.ptr(g_colors),
                                          L.ptr(g_colors) if sh else None, L.stream()), "gs_surfel_project_bwd")
        return (g_means, g_quats, g_scales, g_opac, g_colors) + (None,) * 11


def _raster_fwd(st, background, W, H, tile_size, depth_channel, distloss):
    """the compositor's forward on a projected and binned view `st` (of _project_bin): (render [H,W,C], alphas, normals, distort or None,
    median, last_ids, final_T, final_D or None).  The last three are the per-pixel state _raster_bwd walks back from."""
    lib, dev, f32 = L.lib(), st["means2d"].device, torch.float32
    Cn, V, I = st["C"], st["V"], st["I"]
    render = torch.empty(H, W, Cn, dtype=f32, device=dev); alphas = torch.empty(H, W, dtype=f32, device=dev)
    normals = torch.empty(H, W, 3, dtype=f32, device=dev); median = torch.empty(H, W, dtype=f32, device=dev)
    distort = torch.empty(H, W, dtype=f32, device=dev) if distloss else None
    last_ids = torch.empty(H, W, dtype=torch.int32, device=dev); final_T = torch.empty(H, W, dtype=f32, device=dev)
    final_D = torch.empty(H, W, dtype=f32, device=dev) if distloss else None
    L.check(lib.gs_surfel_raster_fwd(W, H, tile_size, Cn, 1 if depth_channel else 0, 1 if distloss else 0, V,
                                     L.ptr(st["ray_transforms"]), L.ptr(st["means2d"]), L.ptr(st["opacities"]), L.ptr(st["colors"]),
                                     L.ptr(st["normals"]), L.ptr(background), I, L.ptr(st["isect_offsets"]),
                                     L.ptr(st["flatten_ids"]), L.ptr(render), L.ptr(alphas), L.ptr(normals), L.ptr(distort),
                                     L.ptr(median), L.ptr(last_ids), L.ptr(final_T), L.ptr(final_D), L.stream()),
            "gs_surfel_raster_fwd")
    return render, alphas, normals, distort, median, last_ids, final_T, final_D


def _raster_bwd(st, background, W, H, tile_size, depth_channel, distloss, last_ids, final_T, final_D, v_render, v_alphas, v_normals,
                v_distort):
    """the compositor's backward: (v_packed [V, gs_surfel_grad_stride()], v_densify [V,2]) from the cotangents of the four images
    (contiguous fp32; v_distort None without distloss) and the state _raster_fwd stored.  `st` needs the per-Gaussian tensors, the
    tile offsets and the list of _project_bin."""
    lib, dev, f32 = L.lib(), st["means2d"].device, torch.float32
    Cn, V, I = st["C"], st["V"], st["I"]
    v_packed = torch.empty(V, lib.gs_surfel_grad_stride(), dtype=f32, device=dev)
    v_densify = torch.empty(V, 2, dtype=f32, device=dev)
    L.check(lib.gs_surfel_raster_bwd(W, H, tile_size, Cn, 1 if depth_channel else 0, 1 if distloss else 0, V, L.ptr(st["ray_transforms"]),
                                     L.ptr(st["means2d"]), L.ptr(st["opacities"]), L.ptr(st["colors"]), L.ptr(st["normals"]),
                                     L.ptr(st["depths"]), L.ptr(background), I, L.ptr(st["isect_offsets"]), L.ptr(st["flatten_ids"]),
                                     L.ptr(last_ids), L.ptr(final_T), L.ptr(final_D), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_normals),
                                     L.ptr(v_distort), L.ptr(v_packed), L.ptr(v_densify), L.stream()),
            "gs_surfel_raster_bwd")
    return v_packed, v_densify


_RASTER_STATE = ("ray_transforms", "means2d", "opacities", "colors", "normals", "depths", "isect_offsets", "flatten_ids")


class _SurfelComposite(torch.autograd.Function):
    """The ray-splat compositor.  `gradient_2dgs` is the zeros [V,2] leaf of meta: it does not enter the forward; the backward hands it
    v_densify, means2d the compositor's dL/dmeans2d, and leaves the rest of the packed gradients to _SurfelProjectBin."""
    @staticmethod
    def forward(ctx, means2d, gradient_2dgs, link, background, W, H, tile_size, depth_channel, distloss):
        st = link.state
        render, alphas, normals, distort, median, last_ids, final_T, final_D = _raster_fwd(st, background, W, H, tile_size, depth_channel,
                                                                                           distloss)
        ctx.cfg = (W, H, tile_size, st["C"], st["V"], st["I"], depth_channel, distloss)
        ctx.link = link
        ctx.save_for_backward(background, *(st[k] for k in _RASTER_STATE), last_ids, final_T, final_D)
        ctx.mark_non_differentiable(median, last_ids)
        if distort is None:
            distort = torch.empty(0, dtype=torch.float32, device=means2d.device)
            ctx.mark_non_differentiable(distort)
        return render, alphas, normals, distort, median, last_ids

    @staticmethod
    def backward(ctx, v_render, v_alphas, v_normals, v_distort, *_unused):
        W, H, tile_size, Cn, V, I, depth_channel, distloss = ctx.cfg
        bg, *state, last_ids, final_T, final_D = ctx.saved_tensors
        st = dict(zip(_RASTER_STATE, state), C=Cn, V=V, I=I)
        dev, f32 = st["means2d"].device, torch.float32

        def dense(v, *shape):
            return torch.zeros(*shape, dtype=f32, device=dev) if v is None else v.contiguous().float()
        v_render, v_alphas, v_normals = dense(v_render, H, W, Cn), dense(v_alphas, H, W), dense(v_normals, H, W, 3)
        v_distort = dense(v_distort, H, W) if distloss else None
        v_packed, v_densify = _raster_bwd(st, bg, W, H, tile_size, depth_channel, distloss, last_ids, final_T, final_D, v_render, v_alphas,
                                          v_normals, v_distort)
        ctx.link.v_packed = v_packed
        return v_packed[:, 9:11], v_densify, None, None, None, None, None, None, None


def depth_to_normal(depth: Tensor, viewmat: Tensor, K: Tensor) -> Tensor:
    """gsplat's depth_to_normal: depth [H,W,1] (z-depth), viewmat [4,4] world->camera, K [3,3] -> world-space normals [H,W,3] from the
    finite differences of the back-projected points, zero on the one-pixel border.  Plain torch, differentiable through the depth."""
    H, W = depth.shape[:2]
    dev, dt = depth.device, depth.dtype
    xs = torch.arange(W, device=dev, dtype=dt) + 0.5
    ys = torch.arange(H, device=dev, dtype=dt) + 0.5
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    dirs = torch.stack(((gx - K[0, 2]) / K[0, 0], (gy - K[1, 2]) / K[1, 1], torch.ones_like(gx)), dim=-1)
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    origin = -(t @ Rcw)                                       # camera centre in the world frame
    points = origin + depth * (dirs @ Rcw)                    # row vectors: camera -> world is multiplication by Rcw from the right
    dx = points[2:, 1:-1] - points[:-2, 1:-1]
    dy = points[1:-1, 2:] - points[1:-1, :-2]
    n = F.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    return F.pad(n.permute(2, 0, 1), (1, 1, 1, 1), value=0.0).permute(1, 2, 0)


def rasterization_2dgs(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmats: Tensor, Ks: Tensor,
                       width: int, height: int, near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
                       sh_degree: Optional[int] = None, packed: bool = True, tile_size: int = 16, backgrounds: Optional[Tensor] = None,
                       render_mode: str = "RGB", sparse_grad: bool = False, absgrad: bool = False, distloss: bool = False
                       ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor], Optional[Tensor], Tensor, Dict]:
    """``gsplat.rasterization_2dgs`` (1.4, packed, one camera).  Returns
    ``(render_colors [1,H,W,D], render_alphas [1,H,W,1], render_normals [1,H,W,3], normals_from_depth, render_distort, render_median
    [1,H,W,1], meta)``.

    render_normals are world-space (the composited camera-space normals times Rcw).  normals_from_depth [1,H,W,3] exists in the 'ED' /
    'RGB+ED' modes (None otherwise): depth_to_normal of the expected depth.  render_distort [1,H,W,1] exists with distloss=True (None
    otherwise), which needs a mode with a depth channel.  render_median is forward-only: it carries no gradient.
    meta has the keys of rasterization_3dgs (no conics / compensations) plus ``ray_transforms`` [V,3,3], ``normals`` [V,3] (camera space)
    and ``gradient_2dgs``: a zeros [V,2] leaf inside the graph whose ``.grad`` after ``retain_grad()`` and ``backward()`` is the
    compositor's gradient of the two centre terms of the ray transform in pixel units (what GSplatter's densification reads in this
    mode).  ``meta["means2d"]`` is a graph tensor as in rasterization_3dgs.  sparse_grad / absgrad raise NotImplementedError."""
    L.require_cuda(means, quats, scales, opacities, colors, viewmats, Ks)
    if viewmats.shape[:-2] != (1,) or Ks.shape[:-2] != (1,):
        raise ValueError("exactly one camera per call (rfstudio/model/gsplat.py:293 asserts cameras.shape == (1,))")
    if render_mode not in _RENDER_MODES:
        raise ValueError(f"unknown render_mode {render_mode!r}")
    if sparse_grad or absgrad:
        raise NotImplementedError("sparse_grad / absgrad are False on the reference path")
    depth_channel = render_mode != "RGB"
    if distloss and not depth_channel:
        raise ValueError("distloss=True needs a render_mode with a depth channel ('D', 'ED', 'RGB+D' or 'RGB+ED')")
    if tile_size not in (8, 16):
        raise ValueError("tile_size 8 or 16")
    N = means.shape[0]
    assert means.shape == (N, 3) and quats.shape == (N, 4) and scales.shape == (N, 3) and opacities.shape == (N,)
    if render_mode in ("D", "ED"):
        colors, sh_degree = None, None                    # upstream ignores colours in the depth-only modes
    elif sh_degree is not None:
        if not isinstance(sh_degree, int) or sh_degree < 0:
            raise ValueError(f"sh_degree must be None or a degree >= 0, not {sh_degree!r}")
        if sh_degree >= 4:
            raise NotImplementedError("sh_degree 0..3 (degree 4 is not implemented)")
        if colors.dim() != 3 or colors.shape[0] != N or colors.shape[2] != 3 or colors.shape[1] < (sh_degree + 1) ** 2:
            raise ValueError(f"sh_degree={sh_degree} needs colors [N, K, 3] with K >= {(sh_degree + 1) ** 2}, got {tuple(colors.shape)}")
    elif colors.dim() != 2 or colors.shape != (N, 3):
        raise ValueError(f"colors must be [N, 3] without sh_degree, got {tuple(colors.shape)}")
    W, H = int(width), int(height)
    bg = None
    if backgrounds is not None and colors is not None:
        bg = backgrounds.reshape(-1).contiguous().float()
        assert bg.shape[0] == 3
    viewmat, K = viewmats.reshape(4, 4).float(), Ks.reshape(3, 3).float()
    link = _Link()
    means2d = _SurfelProjectBin.apply(means.float(), quats.float(), scales.float(), opacities.float(),
                                      None if colors is None else colors.float(), viewmat, K, link, W, H, int(tile_size),
                                      float(near_plane), float(far_plane), float(radius_clip), sh_degree, depth_channel)
    st = link.state
    V = st["V"]
    gradient_2dgs = torch.zeros(V, 2, dtype=torch.float32, device=means.device, requires_grad=means2d.requires_grad)
    render, alphas, normals, distort, median, last_ids = _SurfelComposite.apply(means2d, gradient_2dgs, link, bg, W, H, int(tile_size),
                                                                                depth_channel, bool(distloss))
    link.state = None
    alphas = alphas.view(H, W, 1)
    normals_from_depth = None
    if render_mode in ("ED", "RGB+ED"):
        render = torch.cat((render[..., :-1], render[..., -1:] / alphas.clamp(min=1e-10)), dim=-1)
        normals_from_depth = depth_to_normal(render[..., -1:], viewmat, K).unsqueeze(0)
    render_normals = normals @ viewmat[:3, :3]
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    meta = {
        "camera_ids": torch.zeros(V, dtype=torch.int64, device=means.device),
        "gaussian_ids": st["gaussian_ids_i32"].long(),
        "radii": st["radii"], "means2d": means2d, "depths": st["depths"], "opacities": st["opacities"],
        "ray_transforms": st["ray_transforms"].view(V, 3, 3), "normals": st["normals"], "gradient_2dgs": gradient_2dgs,
        "tile_width": tw, "tile_height": th, "tiles_per_gauss": st["tiles_per_gauss"], "isect_ids": st["isect_ids"],
        "flatten_ids": st["flatten_ids"], "isect_offsets": st["isect_offsets"].view(1, th, tw), "width": width, "height": height,
        "tile_size": tile_size, "n_cameras": 1,
        "last_ids": last_ids.view(1, H, W),
    }
    if sh_degree is not None:
        meta["colors"] = st["colors"][:, :3]
    return (render.unsqueeze(0), alphas.unsqueeze(0), render_normals.unsqueeze(0), normals_from_depth,
            distort.view(1, H, W, 1) if distloss else None, median.view(1, H, W, 1), meta)


# ------------------------------------------------------------------------------------------------ the model and the trainer
@dataclass
class SurfelUpdateInfo(UpdateInfo):
    normal_loss: Optional[Tensor] = None
    distort_loss: Optional[Tensor] = None


@dataclass
class SurfelModel(GSplatModel):
    """GSplatter with rasterize_mode='2dgs' (rfstudio/model/gsplat.py:112-282) on rasterization_2dgs."""
    rasterize_mode: str = "2dgs"

    def _rasterize(self, camera: Camera, render_mode: str):
        if self.rasterize_mode != "2dgs":
            raise ValueError(f"SurfelModel renders rasterize_mode='2dgs', not {self.rasterize_mode!r}")
        g = self.gaussians
        L.require_cuda(g.means)
        dev = g.means.device
        if render_mode == "ED":
            colors, sh_degree = g.colors.detach(), None
        else:
            colors, sh_degree = _gsplatter_colors(g.colors, g.shs, self._active_sh_degree())
        track = self.training and self.prepare_densification and g.requires_grad and torch.is_grad_enabled()
        render, alpha, normal, pseudo_normal, distort, _median, info = rasterization_2dgs(
            means=g.means, quats=g.quats, scales=g.scales.exp(), opacities=torch.sigmoid(g.opacities).squeeze(-1), colors=colors,
            viewmats=camera.view_matrix.to(dev).view(1, 4, 4), Ks=camera.intrinsic_matrix.to(dev).view(1, 3, 3), width=camera.width,
            height=camera.height, tile_size=self.block_width, packed=True, near_plane=0.01, far_plane=1e10, render_mode=render_mode,
            sh_degree=sh_degree, sparse_grad=False, absgrad=False, distloss=self.training and render_mode != "ED")
        if track and info["gradient_2dgs"].requires_grad:
            normal_loss = distort_loss = None
            if render_mode != "ED":
                normal_loss = (1 - (normal * (pseudo_normal * alpha)).sum(-1)).mean()[None]
                distort_loss = distort.mean()[None] if distort is not None else None
            info["gradient_2dgs"].retain_grad()
            self.update_info = SurfelUpdateInfo(xys=info["gradient_2dgs"], indices=info["gaussian_ids"], last_width=int(camera.width),
                                                last_height=int(camera.height), normal_loss=normal_loss, distort_loss=distort_loss)
        return render, alpha

    def render_layers(self, camera: Camera) -> Tuple[Tensor, Tensor]:
        render, alpha = self._rasterize(camera, "RGB+ED")
        return render[..., :3].squeeze(0), alpha.squeeze(0)


@dataclass
class SurfelTrainer(GSplatTrainer):
    """GSplatTrainer with the 2DGS regularisers (rfstudio/trainer/gsplat_trainer.py:135-139, :161-164); densification, culling and the
    Adam mutation are inherited."""
    normal_weight: float = 5e-2
    distort_weight: float = 1e-2
    normal_start: int = 7000
    distort_start: int = 3000

    def before_update(self, model: GSplatModel, *, curr_step: int) -> None:
        super().before_update(model, curr_step=curr_step)
        self._curr_step = curr_step

    def step(self, model: GSplatModel, camera: Camera, gt: Tensor):
        if not model.prepare_densification:
            raise ValueError("SurfelTrainer reads the regularisers from update_info: the model needs prepare_densification=True")
        loss, metrics = super().step(model, camera, gt)
        info, step = model.update_info, getattr(self, "_curr_step", 0)
        if step > self.normal_start and info.normal_loss is not None:
            loss = loss + self.normal_weight * info.normal_loss.squeeze(0)
            metrics["normal"] = info.normal_loss.detach()
        if step > self.distort_start and info.distort_loss is not None:
            loss = loss + self.distort_weight * info.distort_loss.squeeze(0)
            metrics["distort"] = info.distort_loss.detach()
        return loss, metrics
