"""Shading an extracted mesh with its materials under a split-sum environment: 2-D texture lookups and the per-pixel PBR shader.
What the reference gets from `TriangleMesh.render(cameras, shader=PBRShader(envmap=...))` (rfstudio/graphics/shaders.py:44-105)
and, with constant materials, from `PrettyShader(occlusion_type='none')` (shaders.py:199-233).  The kernels are
csrc/gs_meshshade.hip; the semantics are this project's and are stated in full in include/geosplat_hip.h.

  texture2d(tex [Ht,Wt,C], uv [...,2], boundary_mode='wrap' | 'clamp') -> [...,C]
      dr.texture(tex[None], uv, filter_mode='linear'): C in 1..4, fp32, no mip chain.
      wrap   u' = u - floor(u), x = u' Wt - 0.5, ix0 = floor(x) (may be -1), fx = x - ix0, taps at ix0 mod Wt and (ix0 + 1) mod Wt;
             y likewise with Ht.
      clamp  x = clamp(u Wt - 0.5, 0, Wt - 1), taps ix0 and min(ix0 + 1, Wt - 1): the FG-LUT lookup for C channels; gradient 0 in a
             clamped coordinate.
      value  top + fy (bot - top) with top = t00 + fx (t10 - t00).  Gradients to `tex` and to `uv` (the derivative of the selected
             cell's bilinear patch).  A non-finite uv row gives zeros and no gradient.  Tap indices are reduced into range in
             integer arithmetic: no input addresses memory outside the texture.
  Texture2D(data [Ht,Wt,3])
      .from_constants((r, g, b), device=) a 1x1 texture;  .sample(uv) the wrap lookup at (u (1 - 1/Wt) + 0.5/Wt,
      v (1 - 1/Ht) + 0.5/Ht)  (rfstudio/graphics/_mesh/_texture.py:168-175).
  shade_pixels(position, normal, uv, rast, kd, ks, camera_pos, envmap, *, occlusion='texture' | 'none' | 'ao' | 'screen',
               visibility=None, min_visibility=0.0, bend_back_normal=False, fg_lut=None) -> colour [H,W,3]
      PBRShader.shade on a G-buffer: position [H,W,3] world space, normal [H,W,3] unit vectors in world space, uv [H,W,2],
      kd / ks Texture2D (ks = occlusion, roughness, metallic -- no min_roughness / max_metallic remap).  Per pixel with
      rast[..., 3] > 0:
        kd, ks = kd.sample(uv), ks.sample(uv);  rough = ks[1], metal = ks[2]
        spec = (1 - metal) 0.04 + kd metal;  diff = kd (1 - metal)
        wo = safe_normalize(camera_pos - position);  d = n.wo
        bend_back_normal: n <- (d > 0 ? n : -n), d <- n.wo, ndv = d;  otherwise ndv = max(d, 1e-4)
        fg = LUT(ndv, rough) with clamp;  refl = 2 d n - wo
        l_diff = cube(base, n);  l_spec = cube_mip(levels, refl, mip_from_roughness(rough))  (TextureSplitSum.sample, no transform)
        visibility = max(1 - ks[0], min_visibility) for 'texture', 1 for 'none'
        colour = (l_diff diff + l_spec (spec fg[0] + fg[1])) visibility
      occlusion 'ao' and 'screen' (PBRShader(occlusion_type='ao' | 'ssao'), shaders.py:92-104) take the map `visibility` [H,W] --
      occlusion.face_ambient_occlusion through the face ids, or any map of the caller's -- and v = max(visibility, min_visibility):
        'ao'      colour = l_diff diff v + l_spec (spec fg[0] + fg[1])            (the diffuse term alone)
        'screen'  colour = (l_diff diff + l_spec (spec fg[0] + fg[1])) v
      `visibility` is required for these two and refused for the others; it receives no gradient.  A map of ones gives the bits of
      'none', forward and backward.  The reference spells the second mode 'ssao'; that name keeps raising ValueError here.
      Pixels with rast[..., 3] == 0 get colour 0 and no gradient anywhere -- a documented difference: the reference shades them from
      face 0 and hides them behind alpha 0.  A pixel with a non-finite position, normal or uv is treated the same way.
      TextureSG environments are not provided.
      Gradients go to position, normal, uv, kd.data, ks.data, envmap.base and every envmap.levels[l]; every selection (texel, LUT
      cell, cube face, mip level, the ndv and visibility clamps, the bend) takes the derivative of the selected piece, 0 where a
      clamp is active.  The forward and the per-pixel gradients are bit-identical between runs; the texel gradients are sums of
      fp32 atomics.
Every op raises GeoSplatHipError on CPU tensors; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L
from .shading import _make_env, get_fg_lut
from .splitsum import TextureSplitSum

_BOUNDARY = {"wrap": 0, "clamp": 1}
_OCCLUSION = {"texture": 0, "none": 1, "ao": 2, "screen": 3}
_WITH_MAP = ("ao", "screen")


class _Texture2DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex: Tensor, uv: Tensor, boundary: int):
        t = tex.detach().contiguous()
        q = uv.detach().reshape(-1, 2).contiguous()
        Ht, Wt, Cc = t.shape
        P = q.shape[0]
        out = torch.empty(P, Cc, dtype=torch.float32, device=t.device)
        L.check(L.lib().gs_tex2d_fwd(P, Ht, Wt, Cc, boundary, L.ptr(t), L.ptr(q), L.ptr(out), L.stream()), "gs_tex2d_fwd")
        ctx.save_for_backward(t, q)
        ctx.boundary, ctx.uv_shape = boundary, uv.shape
        return out.reshape(*uv.shape[:-1], Cc)

    @staticmethod
    def backward(ctx, d_out: Tensor):
        t, q = ctx.saved_tensors
        Ht, Wt, Cc = t.shape
        P = q.shape[0]
        g = d_out.reshape(P, Cc).contiguous().float()
        d_uv = torch.empty_like(q)
        d_tex = torch.zeros_like(t)
        L.check(L.lib().gs_tex2d_bwd(P, Ht, Wt, Cc, ctx.boundary, L.ptr(t), L.ptr(q), L.ptr(g), L.ptr(d_uv), L.ptr(d_tex),
                                     L.stream()), "gs_tex2d_bwd")
        return d_tex, d_uv.reshape(ctx.uv_shape), None


def texture2d(tex: Tensor, uv: Tensor, boundary_mode: str = "wrap") -> Tensor:
    """tex [Ht,Wt,C] (C in 1..4), uv [...,2] -> [...,C]: bilinear lookup with 'wrap' or 'clamp' (module docstring); differentiable in
    `tex` and `uv`."""
    if boundary_mode not in _BOUNDARY:
        raise ValueError("boundary_mode must be 'wrap' or 'clamp'")
    L.require_cuda(tex, uv)
    if tex.ndim != 3 or not (1 <= tex.shape[2] <= 4) or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise L.GeoSplatHipError("tex must be [Ht,Wt,C] with C in 1..4")
    if uv.ndim < 1 or uv.shape[-1] != 2:
        raise L.GeoSplatHipError("uv must be [...,2]")
    return _Texture2DFn.apply(tex.float(), uv.float(), _BOUNDARY[boundary_mode])


class Texture2D:
    """A 3-channel 2-D texture `data` [Ht,Wt,3] (the reference's Texture2D, rfstudio/graphics/_mesh/_texture.py)."""

    def __init__(self, data: Tensor):
        if data.ndim != 3 or data.shape[2] != 3 or data.shape[0] < 1 or data.shape[1] < 1:
            raise L.GeoSplatHipError("Texture2D data must be [Ht,Wt,3]")
        self.data = data

    @classmethod
    def from_constants(cls, rgb: Sequence[float], *, device=None) -> "Texture2D":
        r, g, b = rgb
        return cls(torch.tensor([float(r), float(g), float(b)], dtype=torch.float32, device=device).view(1, 1, 3))

    @property
    def height(self) -> int:
        return int(self.data.shape[0])

    @property
    def width(self) -> int:
        return int(self.data.shape[1])

    def sample(self, uv: Tensor) -> Tensor:
        """uv [...,2] -> [...,3]: the wrap lookup at (u (1 - 1/Wt) + 0.5/Wt, v (1 - 1/Ht) + 0.5/Ht)."""
        Ht, Wt = self.height, self.width
        scale = torch.tensor([1.0 - 1.0 / Wt, 1.0 - 1.0 / Ht], dtype=torch.float32, device=uv.device)
        offset = torch.tensor([0.5 / Wt, 0.5 / Ht], dtype=torch.float32, device=uv.device)
        return texture2d(self.data, uv.float() * scale + offset, "wrap")


def _as_texture(t, name: str) -> Texture2D:
    if isinstance(t, Texture2D):
        return t
    if isinstance(t, Tensor):
        return Texture2D(t)
    raise L.GeoSplatHipError(f"{name} must be a Texture2D or a tensor [Ht,Wt,3]")


def check_occlusion(occlusion: str) -> None:
    if occlusion not in _OCCLUSION:
        raise ValueError("occlusion must be 'texture', 'none', 'ao' or 'screen' (the reference's 'ssao' is spelled 'screen' here)")


class _ShadePixels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, position, normal, uv, rast, kd, ks, cam_pos, lut, base, cfg, vis, *levels):
        position, normal, uv, rast = (t.detach().contiguous() for t in (position, normal, uv, rast))
        kd, ks, cam_pos, base = kd.detach().contiguous(), ks.detach().contiguous(), cam_pos.detach().contiguous(), base.detach().contiguous()
        levels = [l.detach().contiguous() for l in levels]
        occlusion, min_visibility, bend, env_min_r, env_max_r = cfg
        H, W = rast.shape[:2]
        color = torch.empty(H, W, 3, dtype=torch.float32, device=rast.device)
        e = _make_env(lut, TextureSplitSum(base, levels, env_min_r, env_max_r))
        if vis is None:
            L.check(L.lib().gs_meshshade_fwd(H, W, L.ptr(rast), L.ptr(position), L.ptr(normal), L.ptr(uv), kd.shape[0], kd.shape[1], L.ptr(kd),
                                             ks.shape[0], ks.shape[1], L.ptr(ks), L.ptr(cam_pos), C.byref(e), occlusion, min_visibility,
                                             int(bend), L.ptr(color), L.stream()), "gs_meshshade_fwd")
        else:
            vis = vis.detach().contiguous()
            L.check(L.lib().gs_meshshade_vis_fwd(H, W, L.ptr(rast), L.ptr(position), L.ptr(normal), L.ptr(uv), kd.shape[0], kd.shape[1],
                                                 L.ptr(kd), ks.shape[0], ks.shape[1], L.ptr(ks), L.ptr(cam_pos), C.byref(e), occlusion,
                                                 min_visibility, int(bend), L.ptr(vis), L.ptr(color), L.stream()), "gs_meshshade_vis_fwd")
        ctx.save_for_backward(position, normal, uv, rast, kd, ks, cam_pos, lut, base, *levels)
        ctx.cfg, ctx.vis = cfg, vis
        return color

    @staticmethod
    def backward(ctx, d_color):
        position, normal, uv, rast, kd, ks, cam_pos, lut, base, *levels = ctx.saved_tensors
        occlusion, min_visibility, bend, env_min_r, env_max_r = ctx.cfg
        H, W = rast.shape[:2]
        g = d_color.contiguous().float()
        d_position = torch.empty_like(position); d_normal = torch.empty_like(normal); d_uv = torch.empty_like(uv)
        d_kd = torch.zeros_like(kd); d_ks = torch.zeros_like(ks)
        d_base = torch.zeros_like(base); d_levels = [torch.zeros_like(l) for l in levels]
        e = _make_env(lut, TextureSplitSum(base, list(levels), env_min_r, env_max_r))
        eg = L.GsEnvGrad()
        eg.base = d_base.data_ptr()
        for i, t in enumerate(d_levels):
            eg.levels[i] = t.data_ptr()
        if ctx.vis is None:
            L.check(L.lib().gs_meshshade_bwd(H, W, L.ptr(rast), L.ptr(position), L.ptr(normal), L.ptr(uv), kd.shape[0], kd.shape[1], L.ptr(kd),
                                             ks.shape[0], ks.shape[1], L.ptr(ks), L.ptr(cam_pos), C.byref(e), occlusion, min_visibility,
                                             int(bend), L.ptr(g), L.ptr(d_position), L.ptr(d_normal), L.ptr(d_uv), L.ptr(d_kd), L.ptr(d_ks),
                                             C.byref(eg), L.stream()), "gs_meshshade_bwd")
        else:
            L.check(L.lib().gs_meshshade_vis_bwd(H, W, L.ptr(rast), L.ptr(position), L.ptr(normal), L.ptr(uv), kd.shape[0], kd.shape[1],
                                                 L.ptr(kd), ks.shape[0], ks.shape[1], L.ptr(ks), L.ptr(cam_pos), C.byref(e), occlusion,
                                                 min_visibility, int(bend), L.ptr(ctx.vis), L.ptr(g), L.ptr(d_position), L.ptr(d_normal),
                                                 L.ptr(d_uv), L.ptr(d_kd), L.ptr(d_ks), C.byref(eg), L.stream()), "gs_meshshade_vis_bwd")
        return (d_position, d_normal, d_uv, None, d_kd, d_ks, None, None, d_base, None, None, *d_levels)


def shade_pixels(position: Tensor, normal: Tensor, uv: Tensor, rast: Tensor, kd, ks, camera_pos: Tensor, envmap: TextureSplitSum, *,
                 occlusion: str = "texture", min_visibility: float = 0.0, bend_back_normal: bool = False,
                 fg_lut: Optional[Tensor] = None, visibility: Optional[Tensor] = None) -> Tensor:
    """PBRShader.shade on a G-buffer -> colour [H,W,3] (module docstring).  `kd`, `ks`: Texture2D (or [Ht,Wt,3] tensors);
    differentiable in position, normal, uv, kd.data, ks.data, envmap.base and envmap.levels.  `visibility` [H,W]: the map of
    occlusion 'ao' / 'screen' (required there, refused otherwise; no gradient)."""
    check_occlusion(occlusion)
    if (occlusion in _WITH_MAP) != (visibility is not None):
        raise ValueError(f"occlusion={occlusion!r} needs a visibility map [H,W]" if visibility is None else
                         f"visibility is taken by occlusion 'ao' and 'screen' only, not by {occlusion!r}")
    if visibility is not None and (not isinstance(visibility, Tensor) or tuple(visibility.shape) != tuple(rast.shape[:2])):
        raise ValueError(f"visibility must be a tensor [H,W] with rast's H and W, got "
                         f"{tuple(visibility.shape) if isinstance(visibility, Tensor) else type(visibility).__name__}")
    if not isinstance(envmap, TextureSplitSum):
        raise L.GeoSplatHipError("envmap must be a TextureSplitSum")
    kd, ks = _as_texture(kd, "kd"), _as_texture(ks, "ks")
    L.require_cuda(position, normal, uv, rast, kd.data, ks.data, camera_pos, envmap.base, *envmap.levels, visibility)
    if rast.ndim != 3 or rast.shape[2] != 4 or rast.shape[0] < 1 or rast.shape[1] < 1:
        raise L.GeoSplatHipError("rast must be [H,W,4]")
    H, W = rast.shape[:2]
    if position.shape != (H, W, 3) or normal.shape != (H, W, 3) or uv.shape != (H, W, 2):
        raise L.GeoSplatHipError("position and normal must be [H,W,3] and uv [H,W,2], with rast's H and W")
    if camera_pos.numel() != 3:
        raise L.GeoSplatHipError("camera_pos must hold 3 values")
    if len(envmap.levels) < 2:
        raise L.GeoSplatHipError("envmap needs at least two specular levels")
    lut = get_fg_lut(rast.device) if fg_lut is None else fg_lut.contiguous()
    cfg = (_OCCLUSION[occlusion], float(min_visibility), bool(bend_back_normal), float(envmap.min_roughness), float(envmap.max_roughness))
    return _ShadePixels.apply(position.float(), normal.float(), uv.float(), rast.float(), kd.data.float(), ks.data.float(),
                              camera_pos.reshape(3).float(), lut, envmap.base, cfg,
                              None if visibility is None else visibility.detach().float(), *envmap.levels)
