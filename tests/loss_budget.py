"""Float64 reference and per-element error budget of the photometric loss (csrc/gs_loss.hip), shared by tests/test_loss_budget_cpu.py
and tests/test_gpu_loss_budget.py.  Everything here runs on the CPU.

The budget of a gradient element is 1e-4 of the float64 sum of the ABSOLUTE per-window contributions to it (the project's contract
for gradients): with x, y the blended images, G the 11 x 11 window, G^T its transposed valid convolution, and per window the kernel's
own partials (gs_loss.hip, loss_stats_kernel)
    dmu  = 2 mu_y A2 / (B1 B2)  -  2 S mu_x / B1  -  dcxy mu_y  -  2 dvx mu_x          (four terms dmu_k)
    dvx  = -S / B2  (0 where the clamped variance is inactive),      dcxy = 2 A1 / (B1 B2)
the element's scale is
    scale_rgb   = w_ssim (G^T sum_k |dmu_k|  +  2 |x| G^T |dvx|  +  |y| G^T |dcxy|)  +  w_l1
    scale_alpha = sum_c |bg_c| scale_rgb_c  +  |w_mask (alpha - mask)|
    w_ssim = lambda / (3 (H - 10) (W - 10)),  w_l1 = (1 - lambda) / (3 H W),  w_mask = 2 mask_weight / (H W),  all times grad_scale.
An element whose x and y differ in float64 by no more than 8 * 2^-24 (|rgb| + |bg| + 1) is *l1_fragile*: a float32 evaluation of
x - y may land on the other side of 0 (or on 0).  Such an element stays in the comparison; its bound grows by the jump 2 w_l1, the
alpha element's by |bg_c| 2 w_l1.
"""
import functools
import math
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import loss_ref

KAPPA = 1e-4                       # the contract: |error| <= KAPPA * scale per element
FRAGILE_CAP = 0.01                 # at most this share of the elements of a case may be l1_fragile
EPS32 = 2.0 ** -24
PAD = 5                            # (11 - 1) / 2

VALUE_KEYS = ("loss", "ssim_loss", "l1", "mask_mse", "mse_srgb", "psnr")


def _blend(rgb, alpha, gt_rgba, train_bg, gt_is_srgb):
    gt_lin = loss_ref.srgb2rgb(gt_rgba[..., :3]) if gt_is_srgb else gt_rgba[..., :3]
    mask = gt_rgba[..., 3:]
    return rgb + (1 - alpha) * train_bg, gt_lin * mask + (1 - mask) * train_bg


def _window_partials(x, y):
    """x, y [H,W,3] float64 -> per window [3,H-10,W-10]: the four terms of dmu, dvx, dcxy (d SSIM / d mu_x, E[xx], E[xy] as the
    kernel forms them) and the 2-D window [11,11]"""
    g = loss_ref.gaussian_window(11, 1.5, x.dtype)
    G = g[:, None] @ g[None, :]
    k = G[None, None]
    conv = lambda t: F.conv2d(t.permute(2, 0, 1)[:, None], k)[:, 0]
    mu_x, mu_y, exx, eyy, exy = conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    vxr, vyr, cxy = exx - mu_x * mu_x, eyy - mu_y * mu_y, exy - mu_x * mu_y
    vx, vy = vxr.clamp_min(0.0), vyr.clamp_min(0.0)
    A1, A2, B1, B2 = 2 * mu_x * mu_y + c1, 2 * cxy + c2, mu_x * mu_x + mu_y * mu_y + c1, vx + vy + c2
    inv = 1.0 / (B1 * B2)
    S = A1 * A2 * inv
    dvx = torch.where(vxr >= 0, -S / B2, torch.zeros_like(S))
    dcxy = 2 * A1 * inv
    dmu_terms = (2 * mu_y * A2 * inv, -S * 2 * mu_x / B1, -dcxy * mu_y, -dvx * 2 * mu_x)
    return dmu_terms, dvx, dcxy, G


def scale_rgb(x, y, ssim_lambda, grad_scale=1.0):
    """[H,W,3] float64: the sum of absolute per-window contributions to d loss / d x, L1 weight included"""
    H, W = x.shape[0], x.shape[1]
    dmu_terms, dvx, dcxy, G = _window_partials(x, y)
    k = G[None, None]
    gT = lambda t: F.conv_transpose2d(t[:, None], k)[:, 0].permute(1, 2, 0)        # [3,h,w] -> [H,W,3]
    w_ssim = ssim_lambda / (3.0 * (H - 2 * PAD) * (W - 2 * PAD)) * grad_scale
    w_l1 = (1.0 - ssim_lambda) / (3.0 * H * W) * grad_scale
    s = gT(sum(t.abs() for t in dmu_terms)) + 2 * x.abs() * gT(dvx.abs()) + y.abs() * gT(dcxy.abs())
    return w_ssim * s + w_l1


def scale_rgb_bruteforce(x, y, ssim_lambda, grad_scale=1.0):
    """the same by an explicit loop over the windows (tests only, small images)"""
    H, W = x.shape[0], x.shape[1]
    dmu_terms, dvx, dcxy, G = _window_partials(x, y)
    adm = sum(t.abs() for t in dmu_terms)
    out = torch.zeros_like(x)
    for c in range(3):
        for i in range(H - 2 * PAD):
            for j in range(W - 2 * PAD):
                sl = (slice(i, i + 11), slice(j, j + 11), c)
                out[sl] += G * (adm[c, i, j] + 2 * x[sl].abs() * dvx[c, i, j].abs() + y[sl].abs() * dcxy[c, i, j].abs())
    w_ssim = ssim_lambda / (3.0 * (H - 2 * PAD) * (W - 2 * PAD)) * grad_scale
    return w_ssim * out + (1.0 - ssim_lambda) / (3.0 * H * W) * grad_scale


def _evaluate(rgb, alpha, gt_rgba, train_bg, gt_is_srgb, ssim_lambda, mask_weight, grad_scale, dtype):
    r = rgb.to(dtype).clone().requires_grad_(True)
    a = alpha.to(dtype).clone().requires_grad_(True)
    out = loss_ref.view_loss(r, a, gt_rgba.to(dtype), train_bg.to(dtype), gt_is_srgb=gt_is_srgb, ssim_lambda=ssim_lambda,
                             mask_weight=mask_weight, metric_bg=torch.zeros(3, dtype=dtype))
    (out["loss"] * grad_scale).backward()
    vals = {k: float(out[k].detach().double()) for k in VALUE_KEYS}
    return vals, r.grad.double(), a.grad.double()


def loss_budget(rgb, alpha, gt_rgba, train_bg, gt_is_srgb=True, ssim_lambda=0.2, mask_weight=5.0, grad_scale=1.0) -> Dict:
    """float32 CPU tensors rgb [H,W,3], alpha [H,W,1], gt_rgba [H,W,4], train_bg [H,W,3] -> dict, everything float64:
      values (loss, ssim_loss, l1, mask_mse, mse_srgb, psnr; metric background 0), d_rgb [H,W,3], d_alpha [H,W,1]   -- float64
      values32, d_rgb32, d_alpha32                                  -- the same view_loss in torch.float32 on the CPU
      scale_rgb, scale_alpha, l1_fragile, bound_rgb, bound_alpha    -- the budget (bound = KAPPA * scale + the L1 jump where fragile)
    """
    args = (gt_is_srgb, ssim_lambda, mask_weight, grad_scale)
    values, d_rgb, d_alpha = _evaluate(rgb, alpha, gt_rgba, train_bg, *args, torch.float64)
    values32, d_rgb32, d_alpha32 = _evaluate(rgb, alpha, gt_rgba, train_bg, *args, torch.float32)
    r, a, gt, bg = rgb.double(), alpha.double().reshape(*rgb.shape[:2], 1), gt_rgba.double(), train_bg.double()
    H, W = r.shape[0], r.shape[1]
    x, y = _blend(r, a, gt, bg, gt_is_srgb)
    s_rgb = scale_rgb(x, y, ssim_lambda, grad_scale)
    w_l1 = (1.0 - ssim_lambda) / (3.0 * H * W) * grad_scale
    w_mask = 2.0 * mask_weight / (H * W) * grad_scale
    s_alpha = (bg.abs() * s_rgb).sum(-1, keepdim=True) + (w_mask * (a - gt[..., 3:])).abs()
    fragile = (x != y) & ((x - y).abs() <= 8 * EPS32 * (r.abs() + bg.abs() + 1))
    jump = fragile.double() * (2 * w_l1)
    return {"values": values, "d_rgb": d_rgb, "d_alpha": d_alpha.reshape(H, W, 1),
            "values32": values32, "d_rgb32": d_rgb32, "d_alpha32": d_alpha32.reshape(H, W, 1),
            "scale_rgb": s_rgb, "scale_alpha": s_alpha, "l1_fragile": fragile, "x": x, "y": y,
            "bound_rgb": KAPPA * s_rgb + jump, "bound_alpha": KAPPA * s_alpha + (bg.abs() * jump).sum(-1, keepdim=True)}


def fraction(got, want, bound) -> float:
    """largest |got - want| / bound over the elements (bound 0: the element must be exact); nan / inf in `got` -> inf"""
    err = (got.double().reshape(want.shape) - want).abs()
    if not torch.isfinite(err).all():
        return math.inf
    f = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(f.max())


def value_errors(got: Dict[str, float], want: Dict[str, float]) -> Dict[str, float]:
    """relative error of loss, ssim_loss, l1, mask_mse, mse_srgb (a reference of exactly 0 must be met exactly: inf otherwise);
    absolute error in dB for psnr"""
    out = {}
    for k in VALUE_KEYS:
        e = abs(got[k] - want[k])
        out[k] = e if k == "psnr" else (e / abs(want[k]) if want[k] != 0 else (0.0 if e == 0 else math.inf))
    return out


# ---------------------------------------------------------------------------------------------------------------- the inputs

TIER_A_SHAPES = ((11, 11), (11, 40), (40, 11), (16, 16), (17, 17), (21, 21), (22, 27), (26, 26), (27, 27), (37, 53))
TIER_A_WIDE = (12, 4097)           # 257 blocks of 16 x 16: the second trip of the finalize kernel's strided loop
TIER_B_SHAPES = ((40, 56), (67, 33))
TIER_B_AMPLITUDES = (2e-2, 1e-3)


def tier_a_inputs(H, W, gt_is_srgb):
    """Textured render with a soft alpha edge over a per-pixel random background, a hard mask that differs from alpha, a block with
    alpha = mask = 0 and rgb = 0 (x == y == bg exactly, on both sides), rgb above 1 and slightly below 0 in a few pixels, gt
    channels at 0, 1 and on both sides of the sRGB knee 0.04045.  float32 tensors (rgb, alpha, gt_rgba, train_bg)."""
    g = torch.Generator().manual_seed(H * 1000 + W + (7 if gt_is_srgb else 0))
    P = W if W <= 64 else 53                                      # a wide image repeats the pattern every 53 columns
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, P)[torch.arange(W) % P], indexing="ij")
    alpha = torch.sigmoid((0.6 - (xx * xx + yy * yy).sqrt()) * 10)[..., None]
    rgb = (0.5 + 0.5 * torch.sin(torch.stack([3 * xx, 4 * yy, 5 * (xx + yy)], -1))) * alpha
    rgb = rgb + 0.05 * torch.rand(H, W, 3, generator=g) * alpha
    mask = (((xx - 0.1) ** 2 + yy * yy).sqrt() < 0.55).float()[..., None]
    gt = (0.5 + 0.4 * torch.cos(torch.stack([2 * xx, 3 * yy, xx - yy], -1)) + 0.1 * torch.rand(H, W, 3, generator=g)).clamp(0, 1)
    bg = torch.rand(H, W, 3, generator=g)
    # transparent on both sides: rows 2..4 of the last five columns (inside the image's border, where few windows reach)
    blk = (slice(2, 5), slice(W - 5, W))
    alpha[blk] = 0.0; rgb[blk] = 0.0; mask[blk] = 0.0
    cy, cx = H // 2, W // 2                                       # inside the object and the mask
    rgb[cy, cx] = torch.tensor([1.3, 1.05, 0.9]); rgb[cy, cx - 1] = torch.tensor([-0.02, 0.5, -0.001])
    rgb[cy - 1, cx] = torch.tensor([2.0, -0.01, 1.0])
    gt[cy + 1, cx] = torch.tensor([0.0, 1.0, 0.04045]); gt[cy + 1, cx - 1] = torch.tensor([0.0404, 0.0405, 0.0])
    gt[cy - 1, cx - 1] = torch.tensor([1.0, 0.0, 0.04046])
    gt[0, 0] = torch.tensor([0.0, 1.0, 0.04])                     # a corner pixel, mask 0 there
    return rgb.contiguous(), alpha.contiguous(), torch.cat([gt, mask], -1).contiguous(), bg.contiguous()


def tier_b_inputs(H, W, amplitude):
    """The converged regime: opaque (alpha = mask = 1), bright and smooth, the render 0.9 + A sin, the (linear) ground truth
    0.88 + A cos, a per-pixel random background that multiplies zero.  The modulation is slow (at most 2.8 rad across the image, so
    a window sees a slope of A / 8 per pixel or less and a variance of 1e-5 and below) against mu^2 ~ 0.8 and c2 = 9e-4: E[xx] - mu^2
    cancels to within a few float32 roundings of 0.8, and near the extrema of the sines its sign, and with it the clamp's derivative,
    is decided by those roundings.  Never constant.  gt_is_srgb = False.  (Faster modulations are well conditioned: at three times
    these frequencies the float32 reference is within 0.05 of the bound for A = 2e-2.)"""
    g = torch.Generator().manual_seed(H * 1000 + W)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64), torch.linspace(-1, 1, W, dtype=torch.float64), indexing="ij")
    rgb = (0.9 + amplitude * torch.sin(torch.stack([1.2 * xx, 1.6 * yy, 2.0 * (xx + yy)], -1))).float()
    gt = (0.88 + amplitude * torch.cos(torch.stack([0.8 * xx, 1.2 * yy, 0.4 * (xx - yy)], -1))).float()
    one = torch.ones(H, W, 1)
    return rgb.contiguous(), one.clone(), torch.cat([gt, one], -1).contiguous(), torch.rand(H, W, 3, generator=g)


@functools.lru_cache(maxsize=None)
def tier_a_case(H, W, gt_is_srgb, mask_weight, grad_scale=1.0):
    """(inputs, budget) of one tier-A case, computed once per process and shared; treat as read-only"""
    inputs = tier_a_inputs(H, W, gt_is_srgb)
    return inputs, loss_budget(*inputs, gt_is_srgb=gt_is_srgb, mask_weight=mask_weight, grad_scale=grad_scale)


@functools.lru_cache(maxsize=None)
def tier_b_case(H, W, amplitude):
    inputs = tier_b_inputs(H, W, amplitude)
    return inputs, loss_budget(*inputs, gt_is_srgb=False)


def reference_fractions(bud) -> Dict[str, float]:
    """the float32 reference against the float64 one: largest fraction of the bound for d rgb and d alpha"""
    return {"rgb": fraction(bud["d_rgb32"], bud["d_rgb"], bud["bound_rgb"]),
            "alpha": fraction(bud["d_alpha32"], bud["d_alpha"], bud["bound_alpha"])}


def scale_fractions(d_rgb, d_alpha, bud) -> Dict[str, float]:
    """worst |error| / (KAPPA * scale) of a gradient pair, the l1_fragile elements (whose error may hold the L1 jump, which is no
    rounding error) and their pixels' alpha elements left out: a figure to print and to compare, not a bound"""
    fr = bud["l1_fragile"]
    keep_rgb, keep_a = (~fr).double(), (~fr.any(-1, keepdim=True)).double()
    e_rgb = (d_rgb.double().reshape(fr.shape) - bud["d_rgb"]).abs() * keep_rgb / (KAPPA * bud["scale_rgb"])
    e_a = (d_alpha.double().reshape(keep_a.shape) - bud["d_alpha"]).abs() * keep_a / (KAPPA * bud["scale_alpha"])
    return {"rgb": float(e_rgb.max()), "alpha": float(e_a.max())}


def f_ref(bud) -> float:
    """F_ref: the float32 reference's worst |error| / (KAPPA * scale) over d rgb and d alpha"""
    return max(scale_fractions(bud["d_rgb32"], bud["d_alpha32"], bud).values())
