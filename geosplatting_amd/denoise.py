"""The bilateral denoiser of the Monte-Carlo estimates (csrc/gs_denoise.hip): what the reference's stages 2 and 3 get from
``bilateral_denoiser`` (rfstudio/graphics/_mesh/_optix/ops.py:107-140, c_src/denoising.cu).  A Gaussian window of radius
``2 ceil(2.5 sigma) + 1`` whose taps are also weighted by the 128th power of the normals' dot product and by the depth difference against
the centre's depth slope.  include/geosplat_hip.h states the semantics; the gradient reaches ``col`` only, as in the reference."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from . import _lib

__all__ = ["bilateral_denoiser", "filter_radius"]

MAX_RADIUS = 127
MAX_CHANNELS = 8


def filter_radius(sigma: float) -> int:
    """``2 ceil(2.5 sigma) + 1``: the window is (2 R + 1)^2 taps"""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0) or 2.5 * sigma > 64.0 or 2 * math.ceil(2.5 * sigma) + 1 > MAX_RADIUS:
        raise ValueError(f"sigma must be finite and positive with a radius 2 ceil(2.5 sigma) + 1 <= {MAX_RADIUS}, got {sigma}")
    return 2 * math.ceil(2.5 * sigma) + 1


class _Denoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, col, nrm, zdz, sigma, form):
        B, H, W, C = col.shape
        out = torch.empty_like(col)
        wsum = torch.empty(B, H, W, dtype=torch.float32, device=col.device)
        _lib.check(_lib.lib().gs_denoise_fwd(B, H, W, C, zdz.shape[-1], _lib.ptr(col), _lib.ptr(nrm), _lib.ptr(zdz), sigma, form, _lib.ptr(out),
                                             _lib.ptr(wsum), _lib.stream()), "gs_denoise_fwd")
        ctx.save_for_backward(nrm, zdz, wsum)
        ctx.sigma, ctx.form = sigma, form
        return out

    @staticmethod
    def backward(ctx, out_grad):
        nrm, zdz, wsum = ctx.saved_tensors
        out_grad = out_grad.contiguous().float()
        B, H, W, C = out_grad.shape
        col_grad = torch.empty_like(out_grad)
        _lib.check(_lib.lib().gs_denoise_bwd(B, H, W, C, zdz.shape[-1], _lib.ptr(nrm), _lib.ptr(zdz), ctx.sigma, ctx.form, _lib.ptr(wsum),
                                             _lib.ptr(out_grad), _lib.ptr(col_grad), _lib.stream()), "gs_denoise_bwd")
        return col_grad, None, None, None, None


def bilateral_denoiser(col: Tensor, nrm: Tensor, zdz: Tensor, sigma: float, *, tiled: Optional[bool] = None) -> Tensor:
    """``bilateral_denoiser(col, nrm, zdz, sigma)`` of the reference -> the filtered ``col``, in its shape.

    ``col`` [..., H, W, C] float32 with up to one batch axis ([H,W,C] or [B,H,W,C]; the reference's stage 2 passes [1,1,N,C] and filters
    along the Gaussian index) and 1 <= C <= 8; ``nrm`` [..., H, W, 3]; ``zdz`` [..., H, W, 1 or 2] = (depth, depth slope), one channel
    standing for both as in the reference's broadcast; ``sigma`` a Python float.  Differentiable in ``col`` only.

    Unlike the reference, which is 3-channel and broadcasts a 1-channel ``col`` to 3, the output has the C channels of the input, and
    ``nrm`` must have 3 channels.  ``tiled`` forces a form of the kernel (True: the window halo staged in LDS, ValueError when it does
    not fit; False: taps read from global memory; None picks); the forms agree bit for bit -- a debugging and test keyword."""
    for name, t, last in (("col", col, None), ("nrm", nrm, (3,)), ("zdz", zdz, (1, 2))):
        if not isinstance(t, Tensor) or t.dtype != torch.float32 or t.ndim not in (3, 4):
            raise ValueError(f"{name} must be a float32 tensor [H,W,C] or [B,H,W,C], got "
                             f"{(t.dtype, tuple(t.shape)) if isinstance(t, Tensor) else type(t).__name__}")
        if last is not None and t.shape[-1] not in last:
            raise ValueError(f"{name} must have {' or '.join(map(str, last))} channels, got {tuple(t.shape)}")
    if not 1 <= col.shape[-1] <= MAX_CHANNELS:
        raise ValueError(f"col must have 1..{MAX_CHANNELS} channels, got {tuple(col.shape)}")
    if nrm.shape[:-1] != col.shape[:-1] or zdz.shape[:-1] != col.shape[:-1]:
        raise ValueError(f"col, nrm and zdz must share [..., H, W], got {tuple(col.shape)}, {tuple(nrm.shape)}, {tuple(zdz.shape)}")
    if min(col.shape) < 1:
        raise ValueError(f"col must not be empty, got {tuple(col.shape)}")
    sigma = float(sigma)
    filter_radius(sigma)
    if tiled is not None and not isinstance(tiled, bool):
        raise ValueError(f"tiled must be None, True or False, got {tiled!r}")
    _lib.require_cuda(col, nrm, zdz)
    if tiled and not _lib.lib().gs_denoise_tiled_fits(col.shape[-1], sigma):
        raise ValueError(f"tiled=True: the halo of radius {filter_radius(sigma)} with {col.shape[-1]} channels does not fit the LDS")
    shape = col.shape
    to4 = (lambda t: t.unsqueeze(0)) if col.ndim == 3 else (lambda t: t)
    out = _Denoise.apply(to4(col).contiguous(), to4(nrm).detach().contiguous(), to4(zdz).detach().contiguous(), sigma,
                         -1 if tiled is None else int(tiled))
    return out.view(shape)
