"""Monte-Carlo environment shading on a MeshBVH (csrc/gs_envshade.hip): what the reference's stage 2 gets from ``optix_env_shade``
and ``TextureLatLng.compute_pdf_`` (rfstudio/graphics/_mesh/_optix/ops.py, rfstudio/graphics/_mesh/_texture.py:287-305).  Per point
``2 n_samples_x^2`` directions -- half from the light's CDF tables, half from the BSDF -- combined with the balance heuristic, each
weighted by a shadow ray through the mesh.  include/geosplat_hip.h states the semantics; gradients reach the point attributes and
the light, never the sample directions, the pdfs or the visibility (the reference's choice, envsampling/kernel.cu:97-99)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .raytrace import MeshBVH

__all__ = ["LatLngEnvMap", "make_perms", "env_shade", "BSDF_NAMES", "require_baked"]

BSDF_NAMES = ("pbr", "diffuse", "white")            # the order is the kernel's encoding


# The frame changes of TextureCubeMap / TextureLatLng (rfstudio/graphics/_mesh/_texture.py:307-357): the reference's matrices, composed
# as ``new @ old``.  `EnvCubeMap` (envmap.py) shares them.
def frame_z_up_to_y_up() -> Tensor:
    return torch.tensor([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])


def frame_y_up_to_z_up() -> Tensor:
    return torch.tensor([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def frame_rotation(axis: str, rad: float) -> Tensor:
    """Rotation by ``rad`` about 'x', 'y' or 'z' in float32, as get_rotation_from_axis_angle builds it (Rodrigues):
    cos I + (1 - cos) a a^T + sin [a]x."""
    x, y, z = (1.0 if k == "xyz".index(axis) else 0.0 for k in range(3))
    a = torch.tensor([x, y, z])
    cos, sin = torch.tensor(float(rad)).cos(), torch.tensor(float(rad)).sin()
    skew = torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return cos * torch.eye(3) + (1 - cos) * (a[:, None] @ a[None, :]) + sin * skew


def compose_transform(new: Tensor, old: Optional[Tensor]) -> Tensor:
    """``new @ old`` (the reference's order: the latest frame change is applied last), on old's device"""
    if old is None:
        return new
    return new.to(old.device) @ old


class _FrameMethods:
    """the frame methods of TextureCubeMap / TextureLatLng, in place on ``self.transform``"""
    transform: Optional[Tensor]

    def _compose(self, new: Tensor):
        self.transform = compose_transform(new.to(self.data.device), self.transform)
        return self

    def z_up_to_y_up_(self):
        return self._compose(frame_z_up_to_y_up())

    def y_up_to_z_up_(self):
        return self._compose(frame_y_up_to_z_up())

    def rotateX_(self, rad: float):
        return self._compose(frame_rotation("x", rad))

    def rotateY_(self, rad: float):
        return self._compose(frame_rotation("y", rad))

    def rotateZ_(self, rad: float):
        return self._compose(frame_rotation("z", rad))


class LatLngEnvMap(_FrameMethods):
    """A lat-long radiance map ``data`` [H,W,3] with the sampling tables of ``TextureLatLng``: after ``compute_pdf_()``,
    ``pdf`` is [H,W,3] = stack(pdf, rows, cols) and the shader takes ``pdf[..., 0]``, ``pdf[:, 0, 1]`` and ``pdf[..., 2]``.
    ``transform`` [3,3] (default None) is the frame the texels are stored in, changed by the frame methods; the shaders take a map
    without one: bake it with ``as_cubemap(...).as_latlng(..., apply_transform=True)``."""

    def __init__(self, data: Tensor, transform: Optional[Tensor] = None):
        if data.ndim != 3 or data.shape[-1] != 3 or data.shape[0] < 2 or data.shape[1] < 2:
            raise ValueError(f"data must be [H,W,3] with H, W >= 2, got {tuple(data.shape)}")
        if transform is not None and tuple(transform.shape) != (3, 3):
            raise ValueError(f"transform must be [3,3], got {tuple(transform.shape)}")
        self.data = data
        self.pdf: Optional[Tensor] = None
        self.transform = transform

    def clone(self) -> "LatLngEnvMap":
        out = LatLngEnvMap(self.data.clone(), None if self.transform is None else self.transform.clone())
        out.pdf = None if self.pdf is None else self.pdf.clone()
        return out

    def as_cubemap(self, resolution: int):
        """TextureLatLng.as_cubemap -> `EnvCubeMap` [6,R,R,3]; the transform is carried over.  Differentiable in ``data``."""
        from .envmap import EnvCubeMap, latlng_to_cube
        return EnvCubeMap(latlng_to_cube(self.data, resolution), transform=self.transform)

    def visualize(self) -> Tensor:
        """The light as a lat-long picture in the world frame: ``data`` itself without a transform, otherwise resampled through a
        cube map of max(W, H)^2 faces with the transform applied, as the reference does."""
        if self.transform is None:
            return self.data
        return self.as_cubemap(max(self.width, self.height)).visualize(width=self.width, height=self.height)

    @property
    def height(self) -> int:
        return self.data.shape[0]

    @property
    def width(self) -> int:
        return self.data.shape[1]

    @torch.no_grad()
    def compute_pdf_(self) -> "LatLngEnvMap":
        """The reference's tables, operation for operation: max over the channels clamped at 1e-3, times the sine of the latitude of
        the row centre, normalised; the cumulative sum along each row, and the cumulative sum over the rows of the row totals
        (repeated along the row, as the reference keeps it); both normalised by their last entry where that is positive."""
        data = self.data.detach()
        H, W = self.height, self.width
        Y, _ = torch.meshgrid((torch.arange(0, H, device=data.device) + 0.5) / H, (torch.arange(0, W, device=data.device) + 0.5) / W,
                              indexing="ij")
        pdf = data.max(-1).values.clamp_min(1e-3) * (Y * torch.pi).sin()
        pdf = pdf / pdf.sum()
        cols = torch.cumsum(pdf, dim=1)
        rows = torch.cumsum(cols[:, -1:].repeat(1, W), dim=0)
        cols = cols / torch.where(cols[:, -1:] > 0, cols[:, -1:], torch.ones_like(cols))
        rows = rows / torch.where(rows[-1:, :] > 0, rows[-1:, :], torch.ones_like(rows))
        self.pdf = torch.stack((pdf, rows, cols), dim=-1)
        return self

    def tables(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(pdf [H,W], rows [H], cols [H,W]) as ``env_shade`` takes them"""
        if self.pdf is None:
            self.compute_pdf_()
        return self.pdf[..., 0], self.pdf[:, 0, 1], self.pdf[..., 2]


def require_baked(envmap, who: str) -> None:
    """The shaders look a lat-long map up in its own frame (the reference asserts ``envmap.transform is None``)"""
    if getattr(envmap, "transform", None) is not None:
        raise ValueError(f"{who} needs a lat-long map without a transform: bake it with "
                         "as_cubemap(...).as_latlng(..., apply_transform=True)")


def make_perms(n_samples_x: int, device, tables: int = 32768, generator: Optional[torch.Generator] = None) -> Tensor:
    """``tables`` random permutations of 0 .. n^2 - 1 as int32 [tables, n^2]: they decorrelate the strata of the light and of the BSDF
    samples (the reference's ``argsort(rand(32768, n^2))``)."""
    if n_samples_x < 1 or tables < 1:
        raise ValueError(f"n_samples_x and tables must be at least 1, got {n_samples_x} and {tables}")
    return torch.argsort(torch.rand(tables, n_samples_x * n_samples_x, device=device, generator=generator), dim=-1).int()


_perm_cache: Dict[Tuple[int, str], Tensor] = {}


def _cached_perms(n: int, device: torch.device) -> Tensor:
    key = (n, str(device))
    if key not in _perm_cache:
        _perm_cache[key] = make_perms(n, device)
    return _perm_cache[key]


def _draw_seed() -> int:
    return int(np.random.randint(2 ** 31))


def _head(bvh: MeshBVH, mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms, n, seed, bsdf, shadow_scale, lanes):
    H, W = light.shape[0], light.shape[1]
    v, f = bvh.vertices, bvh.faces
    return (mask.shape[0], _lib.ptr(mask), _lib.ptr(ro), _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(view), _lib.ptr(kd), _lib.ptr(ks), H, W,
            _lib.ptr(light), _lib.ptr(pdf), _lib.ptr(rows), _lib.ptr(cols), perms.shape[0], n, _lib.ptr(perms), int(seed), bsdf,
            float(shadow_scale), v.shape[0], f.shape[0], _lib.ptr(v), _lib.ptr(f), _lib.ptr(bvh.nodes), int(lanes))


class _EnvShade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bvh, mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms, bsdf, n, rnd_seed, shadow_scale, log, lanes, merge):
        seed = _draw_seed() if rnd_seed is None else rnd_seed
        P, dev = mask.shape[0], mask.device
        diff = torch.empty(P, 3, dtype=torch.float32, device=dev)
        spec = torch.empty(P, 3, dtype=torch.float32, device=dev)
        resi = torch.empty(P, 2, dtype=torch.float32, device=dev)
        logs = (None, None, None)
        if log:
            S = 2 * n * n
            logs = (torch.zeros(P, S, 3, dtype=torch.float32, device=dev), torch.zeros(P, S, dtype=torch.float32, device=dev),
                    torch.zeros(P, S, dtype=torch.float32, device=dev))
        head = _head(bvh, mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms, n, seed, bsdf, shadow_scale, lanes)
        _lib.check(_lib.lib().gs_envshade_fwd(*head, _lib.ptr(diff), _lib.ptr(spec), _lib.ptr(resi), *[_lib.ptr(t) for t in logs],
                                              _lib.stream()), "gs_envshade_fwd")
        ctx.save_for_backward(mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms)
        ctx.bvh, ctx.bsdf, ctx.n, ctx.rnd_seed, ctx.shadow_scale, ctx.lanes, ctx.merge = bvh, bsdf, n, rnd_seed, shadow_scale, lanes, merge
        if log:
            ctx.mark_non_differentiable(resi, *logs)
            return (diff, spec, resi, *logs)
        ctx.mark_non_differentiable(resi)
        return diff, spec, resi

    @staticmethod
    def backward(ctx, d_diff, d_spec, *_unused):
        mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms = ctx.saved_tensors
        seed = _draw_seed() if ctx.rnd_seed is None else ctx.rnd_seed        # a fresh draw, as in the reference (see env_shade)
        d_diff = torch.zeros_like(pos) if d_diff is None else d_diff.contiguous().float()
        d_spec = torch.zeros_like(pos) if d_spec is None else d_spec.contiguous().float()
        d_pos, d_nrm, d_kd, d_ks = (torch.empty_like(pos) for _ in range(4))
        d_light = torch.zeros_like(light)
        head = _head(ctx.bvh, mask, ro, pos, nrm, view, kd, ks, light, pdf, rows, cols, perms, ctx.n, seed, ctx.bsdf, ctx.shadow_scale,
                     ctx.lanes)
        _lib.check(_lib.lib().gs_envshade_bwd(*head, int(ctx.merge), _lib.ptr(d_diff), _lib.ptr(d_spec), _lib.ptr(d_pos), _lib.ptr(d_nrm),
                                              _lib.ptr(d_kd), _lib.ptr(d_ks), _lib.ptr(d_light), _lib.stream()), "gs_envshade_bwd")
        return (None, None, None, d_pos, d_nrm, None, d_kd, d_ks, d_light) + (None,) * 11


def _rows3(name: str, t: Tensor, P: Optional[int], last: int = 3) -> Tensor:
    if t.dtype != torch.float32 or t.shape[-1:] != (last,) or not (t.ndim == 2 or (t.ndim == 4 and t.shape[:2] == (1, 1))):
        raise ValueError(f"{name} must be float32 [N,{last}] or [1,1,N,{last}], got {t.dtype} {tuple(t.shape)}")
    t = t.reshape(-1, last)
    if P is not None and t.shape[0] != P:
        raise ValueError(f"{name} has {t.shape[0]} rows, expected {P}")
    return t.contiguous()


def env_shade(bvh: MeshBVH, mask: Tensor, ro: Tensor, gb_pos: Tensor, gb_normal: Tensor, gb_view_pos: Tensor, gb_kd: Tensor,
              gb_ks: Tensor, light, pdf: Optional[Tensor] = None, rows: Optional[Tensor] = None, cols: Optional[Tensor] = None,
              BSDF: str = "pbr", n_samples_x: int = 8,
              rnd_seed: Optional[int] = None, shadow_scale: float = 1.0, *, perms: Optional[Tensor] = None,
              return_samples: bool = False, lanes_per_point: int = 0, merge_rounds: int = -1):
    """``optix_env_shade`` on a `MeshBVH` -> (diff, spec, resi): the diffuse and specular irradiance sums [..,3] and the shadowed
    share of both [..,2], zero where ``mask <= 0``, in the shape family of the inputs ([1,1,N,.] as the reference passes them, or flat
    [N,.]).  ``light`` [H,W,3] with its tables ``pdf`` [H,W], ``rows`` [H], ``cols`` [H,W] (`LatLngEnvMap.tables`), or a `LatLngEnvMap`
    alone (its data and tables; ValueError while it carries a transform); ``gb_ks`` is
    (occlusion factor, roughness, metallic); ``BSDF`` is 'pbr', 'diffuse' or 'white'.

    Differentiable in gb_pos, gb_normal, gb_kd, gb_ks and light; ``resi`` carries no gradient.  The forward is deterministic for a
    given seed.  ``rnd_seed=None`` draws ``np.random.randint(2**31)`` once in forward AND ONCE AGAIN in backward -- the reference's
    behaviour: the gradient is then an independent estimate over fresh samples, not the derivative of the forward's own sum.  An explicit
    seed is reused in backward.  ``perms`` [T, n^2] int32 defaults to one cached `make_perms` table set per (n_samples_x, device).

    ``return_samples=True`` appends the per-sample log (dirs [N, 2 n^2, 3], pdf_sum and vis [N, 2 n^2]; even slots are the light
    samples, odd slots the BSDF samples, in iteration order).  ``lanes_per_point`` (0: default, 1, 16, 64) and ``merge_rounds`` choose
    the kernel's arrangement; they change the order of sums only (scripts/envshade_bench.py measures them)."""
    if BSDF not in BSDF_NAMES:
        raise ValueError(f"BSDF must be one of {BSDF_NAMES}, got {BSDF!r}")
    if isinstance(light, LatLngEnvMap):
        require_baked(light, "env_shade")
        if pdf is None and rows is None and cols is None:
            pdf, rows, cols = light.tables()
        light = light.data
    if pdf is None or rows is None or cols is None:
        raise ValueError("env_shade needs pdf, rows and cols with a light tensor (LatLngEnvMap.tables), or a LatLngEnvMap as light")
    _lib.require_cuda(mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms)
    if not isinstance(bvh, MeshBVH):
        raise TypeError(f"bvh must be a MeshBVH, got {type(bvh).__name__}")
    n = int(n_samples_x)
    if n < 1:
        raise ValueError(f"n_samples_x must be at least 1, got {n_samples_x}")
    if rnd_seed is not None and not 0 <= int(rnd_seed) < 2 ** 31:
        raise ValueError(f"rnd_seed must be in [0, 2^31), got {rnd_seed}")
    flat = gb_pos.ndim == 2
    pos = _rows3("gb_pos", gb_pos, None)
    P = pos.shape[0]
    ro_, nrm, kd, ks = (_rows3(k, t, P) for k, t in (("ro", ro), ("gb_normal", gb_normal), ("gb_kd", gb_kd), ("gb_ks", gb_ks)))
    if mask.dtype != torch.float32 or mask.numel() != P:
        raise ValueError(f"mask must be float32 with {P} elements, got {mask.dtype} {tuple(mask.shape)}")
    if gb_view_pos.dtype != torch.float32 or gb_view_pos.numel() != 3:
        raise ValueError(f"gb_view_pos must be one float32 position (3 elements), got {gb_view_pos.dtype} {tuple(gb_view_pos.shape)}")
    if light.dtype != torch.float32 or light.ndim != 3 or light.shape[2] != 3 or light.shape[0] < 2 or light.shape[1] < 2:
        raise ValueError(f"light must be float32 [H,W,3] with H, W >= 2, got {light.dtype} {tuple(light.shape)}")
    H, W = light.shape[0], light.shape[1]
    for name, t, shape in (("pdf", pdf, (H, W)), ("rows", rows, (H,)), ("cols", cols, (H, W))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}")
    if perms is None:
        perms = _cached_perms(n, pos.device)
    if perms.dtype != torch.int32 or perms.ndim != 2 or perms.shape[0] < 1 or perms.shape[1] != n * n:
        raise ValueError(f"perms must be int32 [T, {n * n}] with T >= 1, got {perms.dtype} {tuple(perms.shape)}")
    if lanes_per_point not in (0, 1, 16, 64):
        raise ValueError(f"lanes_per_point must be 0, 1, 16 or 64, got {lanes_per_point}")
    out = _EnvShade.apply(bvh, mask.detach().reshape(-1).contiguous(), ro_.detach(), pos, nrm, gb_view_pos.detach().reshape(3).contiguous(),
                          kd, ks, light.contiguous(), pdf.detach().contiguous(), rows.detach().contiguous(), cols.detach().contiguous(),
                          perms.contiguous(), BSDF_NAMES.index(BSDF), n, None if rnd_seed is None else int(rnd_seed),
                          float(shadow_scale), bool(return_samples), int(lanes_per_point), int(merge_rounds))
    diff, spec, resi = out[:3]
    if not flat:
        diff, spec, resi = diff.view(1, 1, P, 3), spec.view(1, 1, P, 3), resi.view(1, 1, P, 2)
    return (diff, spec, resi, *out[3:]) if return_samples else (diff, spec, resi)
