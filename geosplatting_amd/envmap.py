"""Environment lights between the stages, and relighting (csrc/gs_envmap.hip): what the reference gets from
``TextureCubeMap.as_latlng / sample / render / visualize`` and ``TextureLatLng.as_cubemap`` with their frame transforms
(rfstudio/graphics/_mesh/_texture.py:307-377, :411-503), from ``RGBAImages.blend_background`` and from its ``.hdr`` loader.

  cube_to_latlng(cube [6,R,R,3], width, height, transform=None) -> [height,width,3]
      texel (i, j) looks the cube up at T d with d = (sin t sin p, cos t, -sin t cos p), t = pi linspace(1/H, 1 - 1/H, H)[i] (the
      reference's end points, not the row centres), p = pi linspace(-1 + 1/W, 1 - 1/W, W)[j].  Row 0 is the +y pole (y-DOWN rows).
  latlng_to_cube(latlng [H,W,3], resolution) -> [6,R,R,3]
      texel (s, y, x) looks the map up at tu = atan2(v0, -v2) / 2 pi + 0.5, tv = acos(clamp(v1, -1, 1)) / pi for the unit direction v
      of the texel centre: the 2-D 'wrap' lookup of `texture2d` (centres at u W - 0.5, wrapped in both axes).
  sample_cubemap(cube, directions [...,3]) -> [...,3]      the lookup itself; the length of a direction does not matter
  render_background(cube, camera, transform=None, srgb=True) -> [H,W,3]
      pixel (i, j) looks the cube up at T Rc ((0.5 - cx + j) / fx, -(0.5 - cy + i) / fy, -1), Rc the rotation of camera.c2w; then
      rgb2srgb (srgb=False leaves radiance).  No gradient.
  blend_background(rgba [...,4], bg [...,3])               rgb alpha + bg (1 - alpha)

Cube lookups are the project's seam-aware bilinear lookup (csrc/gs_cube.h): a tap beyond a face edge is the adjacent texel of the
neighbouring face, the missing tap at a cube corner is the mean of the other three, a zero or non-finite direction gives zeros.  This
differs from nvdiffrast's 'cube' boundary mode only in those edge and corner taps.  Gradients reach the texels, never the directions,
the transform or the camera.  The forwards are gathers (bit-identical between runs); texel gradients are sums of fp32 atomics.

`EnvCubeMap` and `LatLngEnvMap` (envshade.py) carry an optional ``transform`` [3,3] that the frame methods compose as ``new @ old``
(z_up_to_y_up_, y_up_to_z_up_, rotateX_ / rotateY_ / rotateZ_); ``as_latlng(apply_transform=True)`` bakes it.  The shaders take baked
maps only (env_shade, splat_mc, splat_mc_deferred and as_splitsum raise ValueError while a transform is set).  TextureSG and a
transform inside TextureSplitSum are not provided.  Every op raises GeoSplatHipError on CPU tensors; there is no CPU path.
"""
from __future__ import annotations

import math
import re
from typing import Iterator, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .cameras import Camera
from .envshade import (LatLngEnvMap, _FrameMethods, compose_transform, frame_rotation, frame_y_up_to_z_up,  # noqa: F401
                       frame_z_up_to_y_up)

__all__ = ["EnvCubeMap", "cube_to_latlng", "latlng_to_cube", "sample_cubemap", "render_background", "blend_background",
           "frame_z_up_to_y_up", "frame_y_up_to_z_up", "frame_rotation", "compose_transform", "load_hdr", "save_hdr",
           "relight_sequence", "MAX_CUBE_RES"]

MAX_CUBE_RES = 4096                       # GS_CUBE_EDGE_TABLE_MAX_R of csrc/gs_cube.h


def _check_transform(transform: Optional[Tensor], device) -> Optional[Tensor]:
    if transform is None:
        return None
    if not isinstance(transform, Tensor) or tuple(transform.shape) != (3, 3):
        raise ValueError(f"transform must be a [3,3] tensor, got {tuple(getattr(transform, 'shape', ()))}")
    return transform.detach().to(device=device, dtype=torch.float32).contiguous()


def _check_cube(cube: Tensor) -> None:
    if cube.ndim != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or cube.shape[3] != 3 or cube.shape[1] < 1:
        raise ValueError(f"cube must be [6,R,R,3], got {tuple(cube.shape)}")
    if cube.shape[1] > MAX_CUBE_RES:
        raise ValueError(f"cube faces up to {MAX_CUBE_RES}^2 (the seam table of the cube lookup), got R = {cube.shape[1]}")


# ------------------------------------------------------------------------------------------------ autograd functions
class _CubeToLatLng(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube: Tensor, H: int, W: int, transform: Optional[Tensor]):
        c = cube.detach().contiguous()
        R = c.shape[1]
        out = torch.empty(H, W, 3, dtype=torch.float32, device=c.device)
        L.check(L.lib().gs_env_cube_to_latlng_fwd(R, H, W, L.ptr(c), L.ptr(transform), L.ptr(out), L.stream()),
                "gs_env_cube_to_latlng_fwd")
        ctx.cfg = (R, H, W)
        ctx.has_transform = transform is not None
        if ctx.has_transform:
            ctx.save_for_backward(transform)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        R, H, W = ctx.cfg
        transform = ctx.saved_tensors[0] if ctx.has_transform else None
        g = d_out.contiguous().float()
        d_cube = torch.zeros(6, R, R, 3, dtype=torch.float32, device=g.device)
        L.check(L.lib().gs_env_cube_to_latlng_bwd(R, H, W, L.ptr(transform), L.ptr(g), L.ptr(d_cube), L.stream()),
                "gs_env_cube_to_latlng_bwd")
        return d_cube, None, None, None


class _LatLngToCube(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latlng: Tensor, R: int):
        t = latlng.detach().contiguous()
        H, W = t.shape[:2]
        out = torch.empty(6, R, R, 3, dtype=torch.float32, device=t.device)
        L.check(L.lib().gs_env_latlng_to_cube_fwd(H, W, R, L.ptr(t), L.ptr(out), L.stream()), "gs_env_latlng_to_cube_fwd")
        ctx.cfg = (H, W, R)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        H, W, R = ctx.cfg
        g = d_out.contiguous().float()
        d_latlng = torch.zeros(H, W, 3, dtype=torch.float32, device=g.device)
        L.check(L.lib().gs_env_latlng_to_cube_bwd(H, W, R, L.ptr(g), L.ptr(d_latlng), L.stream()), "gs_env_latlng_to_cube_bwd")
        return d_latlng, None


class _SampleCube(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube: Tensor, dirs: Tensor):
        c = cube.detach().contiguous()
        d = dirs.detach().reshape(-1, 3).contiguous()
        n, R = d.shape[0], c.shape[1]
        out = torch.empty(n, 3, dtype=torch.float32, device=c.device)
        L.check(L.lib().gs_cube_sample_linear(n, L.ptr(c), R, L.ptr(d), 1.0, L.ptr(out), L.stream()), "gs_cube_sample_linear")
        ctx.save_for_backward(d)
        ctx.R = R
        return out.reshape(dirs.shape)

    @staticmethod
    def backward(ctx, d_out: Tensor):
        d, = ctx.saved_tensors
        n, R = d.shape[0], ctx.R
        g = d_out.reshape(n, 3).contiguous().float()
        d_cube = torch.zeros(6, R, R, 3, dtype=torch.float32, device=g.device)
        L.check(L.lib().gs_cube_sample_linear_bwd(n, R, L.ptr(d), 1.0, L.ptr(g), L.ptr(d_cube), L.stream()), "gs_cube_sample_linear_bwd")
        return d_cube, None


# ------------------------------------------------------------------------------------------------ functional forms
def cube_to_latlng(cube: Tensor, width: int, height: int, transform: Optional[Tensor] = None) -> Tensor:
    """cube [6,R,R,3] -> lat-long [height,width,3] looked up at ``transform @ d`` (module docstring); differentiable in ``cube``."""
    L.require_cuda(cube)
    _check_cube(cube)
    W, H = int(width), int(height)
    if H < 2 or W < 2:
        raise ValueError(f"width and height must be at least 2, got {width} x {height}")
    return _CubeToLatLng.apply(cube.float(), H, W, _check_transform(transform, cube.device))


def latlng_to_cube(latlng: Tensor, resolution: int) -> Tensor:
    """lat-long [H,W,3] -> cube [6,R,R,3] (module docstring); differentiable in ``latlng``."""
    L.require_cuda(latlng)
    if latlng.ndim != 3 or latlng.shape[2] != 3 or latlng.shape[0] < 2 or latlng.shape[1] < 2:
        raise ValueError(f"latlng must be [H,W,3] with H, W >= 2, got {tuple(latlng.shape)}")
    R = int(resolution)
    if R < 1 or R > MAX_CUBE_RES:
        raise ValueError(f"resolution must be in 1..{MAX_CUBE_RES}, got {resolution}")
    return _LatLngToCube.apply(latlng.float(), R)


def sample_cubemap(cube: Tensor, directions: Tensor) -> Tensor:
    """cube [6,R,R,3], directions [...,3] -> [...,3]: TextureCubeMap.sample.  Differentiable in ``cube`` only."""
    L.require_cuda(cube, directions)
    _check_cube(cube)
    if directions.ndim < 1 or directions.shape[-1] != 3:
        raise ValueError(f"directions must be [...,3], got {tuple(directions.shape)}")
    return _SampleCube.apply(cube.float(), directions.float())


@torch.no_grad()
def render_background(cube: Tensor, camera: Camera, transform: Optional[Tensor] = None, srgb: bool = True) -> Tensor:
    """The environment behind the object as ``camera`` sees it -> [H,W,3] (TextureCubeMap.render); sRGB unless ``srgb=False``."""
    L.require_cuda(cube)
    _check_cube(cube)
    c = cube.detach().float().contiguous()
    T = _check_transform(transform, c.device)
    c2w = camera.c2w.detach().to(device=c.device, dtype=torch.float32).contiguous()
    if tuple(c2w.shape) != (3, 4):
        raise ValueError(f"camera.c2w must be [3,4], got {tuple(c2w.shape)}")
    H, W = int(camera.height), int(camera.width)
    out = torch.empty(H, W, 3, dtype=torch.float32, device=c.device)
    L.check(L.lib().gs_env_background_fwd(c.shape[1], H, W, L.ptr(c), float(camera.fx), float(camera.fy), float(camera.cx),
                                          float(camera.cy), L.ptr(c2w), L.ptr(T), int(bool(srgb)), L.ptr(out), L.stream()),
            "gs_env_background_fwd")
    return out


def blend_background(rgba: Tensor, bg: Tensor) -> Tensor:
    """RGBAImages.blend_background: rgb alpha + bg (1 - alpha) for rgba [...,4] and bg [...,3]"""
    if rgba.shape[-1] != 4 or bg.shape[-1] != 3:
        raise ValueError(f"rgba must be [...,4] and bg [...,3], got {tuple(rgba.shape)} and {tuple(bg.shape)}")
    return rgba[..., 3:] * rgba[..., :3] + bg * (1 - rgba[..., 3:])


# ------------------------------------------------------------------------------------------------ the cube map object
class EnvCubeMap(_FrameMethods):
    """A cube-map light ``data`` [6,R,R,3] with an optional frame ``transform`` [3,3]: the reference's TextureCubeMap."""

    def __init__(self, data: Tensor, transform: Optional[Tensor] = None):
        _check_cube(data)
        if transform is not None and tuple(transform.shape) != (3, 3):
            raise ValueError(f"transform must be [3,3], got {tuple(transform.shape)}")
        self.data = data
        self.transform = transform

    @property
    def resolution(self) -> int:
        return int(self.data.shape[1])

    def clone(self) -> "EnvCubeMap":
        return EnvCubeMap(self.data.clone(), None if self.transform is None else self.transform.clone())

    def as_latlng(self, width: int = 1024, height: int = 512, apply_transform: bool = False) -> LatLngEnvMap:
        """TextureCubeMap.as_latlng: with ``apply_transform`` the transform is baked into the texels and the result carries none;
        without it the texels are sampled untransformed and the transform is carried over."""
        if apply_transform and self.transform is not None:
            return LatLngEnvMap(cube_to_latlng(self.data, width, height, self.transform))
        return LatLngEnvMap(cube_to_latlng(self.data, width, height), transform=self.transform)

    def sample(self, directions: Tensor) -> Tensor:
        return sample_cubemap(self.data, directions)

    def render(self, camera: Camera, srgb: bool = True) -> Tensor:
        return render_background(self.data, camera, self.transform, srgb=srgb)

    @torch.no_grad()
    def visualize(self, width: int = 800, height: int = 400) -> Tensor:
        """The light as a lat-long picture [height,width,3] in the world frame (the transform applied)"""
        return cube_to_latlng(self.data.detach(), width, height, self.transform)

    def as_splitsum(self, **kw):
        from .splitsum import as_splitsum
        if self.transform is not None:
            raise ValueError("as_splitsum needs a cube map without a transform (TextureSplitSum carries none): bake it with "
                             "as_latlng(..., apply_transform=True).as_cubemap(...)")
        return as_splitsum(self.data, **kw)


def relight_sequence(base: EnvCubeMap, width: int, height: int, num_frames: int) -> Iterator[LatLngEnvMap]:
    """The rotating-light loop of the reference's relighting task: yields the baked lat-long light with its sampling tables for
    each of ``num_frames`` frames, turning ``base`` (in place, as the reference does) by 2 pi / num_frames about y after each."""
    if num_frames < 1:
        raise ValueError(f"num_frames must be at least 1, got {num_frames}")
    for _ in range(int(num_frames)):
        with torch.no_grad():
            yield base.as_latlng(width=width, height=height, apply_transform=True).compute_pdf_()
        base.rotateY_(2 * math.pi / num_frames)


# ------------------------------------------------------------------------------------------------ Radiance .hdr (RGBE)
def _rgbe_to_float(rgbe: np.ndarray) -> np.ndarray:
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0).astype(np.float32)                  # 2^(e - 128) / 256
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def load_hdr(path) -> Tensor:
    """A Radiance RGBE picture -> [H,W,3] float32 RGB (CPU): flat scanlines and the new-style run-length scanlines, top-to-bottom
    rows (``-Y H +X W``)."""
    raw = open(path, "rb").read()
    if not (raw.startswith(b"#?RADIANCE") or raw.startswith(b"#?RGBE")):
        raise ValueError(f"{path}: not a Radiance picture")
    end = raw.find(b"\n\n")
    if end < 0:
        raise ValueError(f"{path}: header without end")
    if b"FORMAT=32-bit_rle_rgbe" not in raw[:end]:
        raise ValueError(f"{path}: FORMAT is not 32-bit_rle_rgbe")
    eol = raw.find(b"\n", end + 2)
    m = re.fullmatch(rb"-Y (\d+) \+X (\d+)", raw[end + 2:eol].strip())
    if m is None:
        raise ValueError(f"{path}: only the '-Y H +X W' orientation is read")
    H, W = int(m.group(1)), int(m.group(2))
    buf = np.frombuffer(raw, dtype=np.uint8, offset=eol + 1)
    out = np.empty((H, W, 4), dtype=np.uint8)
    pos = 0
    for y in range(H):
        head = buf[pos:pos + 4]
        if head.size < 4:
            raise ValueError(f"{path}: truncated at row {y}")
        if 8 <= W < 32768 and head[0] == 2 and head[1] == 2 and (int(head[2]) << 8 | int(head[3])) == W:
            pos += 4
            for c in range(4):                                        # four runs-encoded channel planes
                x = 0
                while x < W:
                    if pos >= buf.size:
                        raise ValueError(f"{path}: truncated at row {y}")
                    n = int(buf[pos]); pos += 1
                    if n > 128:
                        n -= 128
                        if n == 0 or x + n > W or pos >= buf.size:
                            raise ValueError(f"{path}: bad run at row {y}")
                        out[y, x:x + n, c] = buf[pos]; pos += 1
                    else:
                        if n == 0 or x + n > W or pos + n > buf.size:
                            raise ValueError(f"{path}: bad run at row {y}")
                        out[y, x:x + n, c] = buf[pos:pos + n]; pos += n
                    x += n
        else:
            if pos + 4 * W > buf.size:
                raise ValueError(f"{path}: truncated at row {y}")
            out[y] = buf[pos:pos + 4 * W].reshape(W, 4); pos += 4 * W
    return torch.from_numpy(_rgbe_to_float(out))


def save_hdr(path, data: Tensor) -> None:
    """[H,W,3] -> a Radiance RGBE picture with flat scanlines: every channel within 2^-8 of the pixel's largest channel"""
    a = data.detach().cpu().float().numpy()
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"data must be [H,W,3], got {tuple(a.shape)}")
    a = np.clip(np.nan_to_num(a, nan=0.0, posinf=3e38), 0.0, None)
    H, W = a.shape[:2]
    big = a.max(-1)
    _, expo = np.frexp(big)                                           # big = mant 2^expo, mant in [0.5, 1)
    on = (big > 0) & (expo >= -127)
    scale = np.where(on, np.ldexp(256.0, -expo), 0.0)                 # 256 / 2^expo: the largest channel lands in [128, 256)
    rgbe = np.zeros((H, W, 4), dtype=np.uint8)
    # nearest, and 255 where the largest channel would round to 256: that one is then off by v - 255 <= v / 256 for v < 256
    rgbe[..., :3] = np.clip(np.rint(a.astype(np.float64) * scale[..., None]), 0, 255).astype(np.uint8)
    rgbe[..., 3] = np.where(on, np.clip(expo + 128, 1, 255), 0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {H} +X {W}\n".encode())
        f.write(rgbe.tobytes())
