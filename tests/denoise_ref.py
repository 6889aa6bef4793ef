"""float64 restatement of the bilateral denoiser of csrc/gs_denoise.hip (include/geosplat_hip.h states the semantics), with a
per-element error budget, and the scenes its tests share (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py).  Written from the
formulas, in the manner of tests/envshade_ref.py: torch float64 from float64 copies of the fp32 inputs; the backward is autograd
through the forward.

  R = 2 ceil(2.5 sigma) + 1, v = sigma^2; for a centre p and every tap q = p + (fx, fy), |fx|, |fy| <= R, inside the image:
    w_xy = exp(-(fx^2 + fy^2) / (2 v)),  w_n = clamp(nrm[q] . nrm[p], 1e-4, 1)^128,
    w_z = exp(-|z[q] - z[p]| / max(dz[p] sqrt(fx^2 + fy^2), 1e-4)),  w = w_xy w_n w_z,
    out[p] = sum_q w col[q] / max(sum_q w, 1e-4);  a one-channel zdz means dz = z.
  backward: col_grad[p] = sum_q w(q<-p) g[q] / max(W[q], 1e-4), w(q<-p) the weight q gave p (dz[q] in the denominator).

Error budget (u = 2^-24, one fp32 rounding; every constant counts the kernel's operations, none is tuned to what it returns).
  w_n: the dot product is two FMAs and a product: |d dot| <= 3 u sum_i |n_i n'_i|.  The clamp is 1-Lipschitz.  Seven squarings of c:
    each doubles the relative error it is given and adds u, so c^128 carries 128 (d dot / c) + 127 u relative, i.e.
    |d w_n| <= 128 c^127 * 3 u sum_i |n_i n'_i| + 127 u c^128 -- the dominant term: 384 u = 2.3e-5 relative at c = 1.
  w_xy = exp(-a), a = d2 / (2 v): d2 is an exact integer, 1 / (2 v) is rounded once from float64 (u), their product (u): a (2 u).  The
    exponential is v_exp_f32 (1 ulp = 2 u) of a * log2(e) (product and constant: 2 u of the argument, which is a 2 u relative in the
    result): relative (4 a + 2) u.
  w_z = exp(-a), a = |dz| * rcp(max(s * dist, 1e-4)): the difference u, dist = sqrtf(d2) correctly rounded u, the product u, max is
    1-Lipschitz, v_rcp_f32 1 ulp = 2 u, the product u: a (6 u), taken as 8 u; with the exponential as above: relative (10 a + 2) u.
  w: two products, 2 u.  Results below the normal range may be flushed: 2^-126 absolute per tap.
    |d w| <= w_xy w_z |d w_n| + w (4 a_xy + 10 a_z + 6) u + 2^-126.
  the sums: N in-image taps added in sequence, one FMA each: N u sum_q w |col[q]| on S, N u W on W (the standard bound).
  out = S / Wc, Wc = max(W, 1e-4) (1-Lipschitz): |d out| <= (sum_q |d w_q| |col_q| + N u sum_q w |col_q|) / Wc
    + |S| / Wc^2 (sum_q |d w_q| + N u W) + 2 u |S| / Wc.  Ratios of sums of non-negative terms: the budget is a weighted mean of the
    per-tap budgets.  Every clamp and the absolute value are continuous: no element is fragile, every element is checked.
  backward: the source t[q] = g[q] * (1 / Wc[q]) carries the forward's relative error of Wc[q] plus 2 u (reciprocal, product), and
    enters the same gather: |d col_grad| <= sum_q |d w_q| |t_q| + sum_q w_q |d t_q| + N u sum_q w_q |t_q|."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-4


def radius(sigma: float) -> int:
    return 2 * math.ceil(2.5 * sigma) + 1


def _shift(t: torch.Tensor, fy: int, fx: int):
    """(centre view, tap view) of [B,H,W,...] for the offset (fx, fy): the pixels whose tap lies inside the image"""
    H, W = t.shape[1], t.shape[2]
    ys, ye, xs, xe = max(0, -fy), min(H, H - fy), max(0, -fx), min(W, W - fx)
    return (slice(None), slice(ys, ye), slice(xs, xe)), (slice(None), slice(ys + fy, ye + fy), slice(xs + fx, xe + fx))


def gather(src: torch.Tensor, src_err, nrm: torch.Tensor, zdz: torch.Tensor, sigma: float, transpose: bool = False):
    """sum_q w src[q] and sum_q w over the window in float64 with the budget's sums: a dict of S [B,H,W,C], W, dW (sum |d w|), N
    [B,H,W], dS (sum |d w| |src| + w src_err) and A (sum w |src|) [B,H,W,C].  transpose: the backward's weights."""
    src, nrm, zdz = src.double(), nrm.double(), zdz.double()
    z, dz = zdz[..., 0], zdz[..., -1]
    B, H, W, C = src.shape
    R, v = radius(sigma), float(sigma) ** 2
    S, A, dS = (torch.zeros(B, H, W, C, dtype=torch.float64) for _ in range(3))
    Ws, dW, N = (torch.zeros(B, H, W, dtype=torch.float64) for _ in range(3))
    err = torch.zeros_like(src) if src_err is None else src_err.double()
    for fy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for fx in range(-min(R, W - 1), min(R, W - 1) + 1):
            p, q = _shift(src, fy, fx)
            d2 = float(fx * fx + fy * fy)
            dist = math.sqrt(d2)
            a_xy = d2 / (2.0 * v)
            w_xy = math.exp(-a_xy)
            dot = (nrm[q] * nrm[p]).sum(-1)
            dn = (nrm[q] * nrm[p]).abs().sum(-1)
            c = dot.clamp(EPS, 1.0)
            w_n = c ** 128
            a_z = (z[q] - z[p]).abs() / ((dz[q] if transpose else dz[p]) * dist).clamp_min(EPS)
            w_z = torch.exp(-a_z)
            w = w_xy * w_n * w_z
            d_wn = 128.0 * c ** 127 * 3.0 * U24 * dn + 127.0 * U24 * w_n
            d_w = (w_xy * w_z * d_wn + w * (4.0 * a_xy + 10.0 * a_z + 6.0) * U24 + TINY).detach()
            wd = w.detach()
            S[p] = S[p] + w[..., None] * src[q]
            A[p] = A[p] + wd[..., None] * src[q].detach().abs()
            dS[p] = dS[p] + d_w[..., None] * src[q].detach().abs() + wd[..., None] * err[q]
            Ws[p] = Ws[p] + w
            dW[p] = dW[p] + d_w
            N[p] = N[p] + 1.0
    return dict(S=S, W=Ws, dW=dW, N=N, dS=dS, A=A)


def forward(col: torch.Tensor, nrm: torch.Tensor, zdz: torch.Tensor, sigma: float):
    """-> (out float64 [B,H,W,C], differentiable in col; budget [B,H,W,C]; g: the sums of `gather`)"""
    g = gather(col, None, nrm, zdz, sigma)
    Wc = g["W"].clamp_min(EPS)[..., None]
    out = g["S"] / Wc
    N = g["N"][..., None]
    S = g["S"].detach().abs()
    budget = ((g["dS"] + N * U24 * g["A"]) / Wc + S / Wc ** 2 * (g["dW"][..., None] + N * U24 * g["W"][..., None]) + 2.0 * U24 * S / Wc
              + TINY).detach()
    return out, budget, g


def backward(grad: torch.Tensor, nrm: torch.Tensor, zdz: torch.Tensor, sigma: float, fwd_sums):
    """-> (col_grad float64 by the transposed gather, its budget); tests compare it with autograd through `forward` as well"""
    Wc = fwd_sums["W"].detach().clamp_min(EPS)
    rel_w = (fwd_sums["dW"] + fwd_sums["N"] * U24 * fwd_sums["W"].detach()) / Wc
    t = grad.double() / Wc[..., None]
    g = gather(t, t.abs() * (rel_w[..., None] + 2.0 * U24), nrm, zdz, sigma, transpose=True)
    return g["S"], g["dS"] + g["N"][..., None] * U24 * g["A"] + TINY


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(B: int, H: int, W: int, C: int, zdz_channels: int, seed: int = 0):
    """(col, nrm, zdz, grad) float32: smooth unit normals with one crease (a column where they turn by 50 degrees), a depth ramp with one
    step (a row where z jumps by 0.4), one block of all-zero normals, colours and cotangents of both signs with a few large values."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    tilt = 0.15 * torch.sin(0.21 * x + 0.1) + torch.where(x >= int(0.6 * W), math.radians(50.0), 0.0)
    roll = 0.12 * torch.cos(0.17 * y)
    n = torch.stack((torch.sin(tilt) * torch.cos(roll), torch.sin(roll), torch.cos(tilt) * torch.cos(roll)), -1)
    n[H // 5: H // 5 + max(1, H // 6), W // 7: W // 7 + max(1, W // 5)] = 0.0
    z = 2.0 + 0.01 * x + 0.02 * y + torch.where(y >= int(0.55 * H), 0.4, 0.0)
    if H == 1:
        z = z + torch.where(x >= int(0.3 * W), 0.4, 0.0)
    nrm = n.float()[None].repeat(B, 1, 1, 1)
    zdz = z.float()[None, ..., None].repeat(B, 1, 1, 1)
    if B > 1:
        zdz = zdz + 0.05 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    if zdz_channels == 2:
        zdz = torch.cat((zdz, 0.02 + 0.08 * torch.rand(B, H, W, 1, generator=g)), -1)
    col = torch.rand(B, H, W, C, generator=g) + 20.0 * (torch.rand(B, H, W, C, generator=g) > 0.97).float()
    grad = torch.randn(B, H, W, C, generator=g)
    return col.contiguous(), nrm.contiguous(), zdz.contiguous(), grad.contiguous()


@functools.lru_cache(maxsize=None)
def reference(B: int, H: int, W: int, C: int, zdz_channels: int, sigma: float, seed: int = 0):
    """float64 forward and backward of `scene` with their budgets, as numpy: (out, out_budget, col_grad, grad_budget)"""
    col, nrm, zdz, grad = scene(B, H, W, C, zdz_channels, seed)
    out, budget, sums = forward(col, nrm, zdz, sigma)
    col_grad, grad_budget = backward(grad, nrm, zdz, sigma, sums)
    return out.numpy(), budget.numpy(), col_grad.numpy(), grad_budget.numpy()
