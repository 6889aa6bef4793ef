"""gs_photo_loss (csrc/gs_loss.hip) per element against the float64 budget of tests/loss_budget.py, through photo_loss_and_grad.

The bound of a gradient element is 1e-4 of the float64 sum of the absolute per-window contributions to it (tests/loss_budget.py),
plus the L1 jump 2 w_l1 where the float64 x - y is within float32 rounding of 0 (l1_fragile; at most 0.15 % of a case's elements,
capped at 1 % by tests/test_loss_budget_cpu.py).  The values loss, ssim_loss, l1, mask_mse, mse_srgb are held to 1e-4 relative and
psnr to 1e-3 dB.

Tier A -- the contract.  Textured renders with a soft alpha edge over a per-pixel random background, a hard mask that differs from
alpha, a block that is transparent on both sides (x == y exactly: the L1 term must be an exact 0), colours above 1 and below 0, gt
channels at 0, 1 and around the sRGB knee; sRGB and linear ground truth, mask weight 5 and 0, at the shapes where the tiling can go
wrong: 11 x 11 (one window), 11 x 40 / 40 x 11 (one row / column of windows), 16 x 16, 17 x 17 (a one-pixel last tile), 21 x 21 (the
valid region ends at the first tile's edge, the other tiles hold no valid window and only supply halo), 22 x 27, 26 x 26 / 27 x 27 (tile
plus full halo, then one more), 37 x 53; and 12 x 4097: 257 blocks, the second trip of the finalize kernel's strided loop.

Tier B -- the converged regime.  alpha = mask = 1, render 0.9 + A sin, ground truth 0.88 + A cos with a slow modulation, A = 2e-2 and
1e-3, at 40 x 56 and 67 x 33.  E[xx] - mu^2 (~1e-5 and below) cancels against mu^2 ~ 0.8 to within a few float32 roundings and is
compared with c2 = 9e-4; no float32 evaluation of the formula holds 1e-4 of the scale there: oracle/loss_ref.view_loss in float32 on
the CPU is off by F_ref = 1.0 ... 1.5 times the tier-A bound (tests/test_loss_budget_cpu.py).  The kernel evaluates the same formula
with another summation order (two separable 11-tap passes against one 121-tap convolution), so its bound is measured on that
reference, in the same test, never on the kernel:
    per element  |error| <= max(1, 4 F_ref) 1e-4 scale,          value  |loss - loss64| <= max(1e-4 |loss64|, 4 |loss32 - loss64|).
The factor 4: the two summation orders' worst-case rounding constants differ by about 2, and so does the maximum of two independent
noise fields over ~7 000 elements; a wrong tap, weight, halo or chain-rule term shows as 1e2 ... 1e4 times the scale's 1e-4.

Every case prints its largest fraction.  Measured on an MI355X, the largest over each tier's cases:
  tier A   v_rgb 0.048 and v_alpha 0.032 of the bound on the shape grid (37 x 53, linear ground truth; the float32 reference 0.042), 0.058
           and 0.034 at 12 x 4097 (the float32 reference 0.11), all away from l1_fragile elements; at an l1_fragile element 0.50: the
           kernel's x - y is exactly 0 where float64's is a few 1e-9, half the L1 jump.  Values 3.9e-6 relative, psnr 7.4e-7 dB.
           grad_scale 1/8: the same fractions, gradients the exact float32 products (0 ulp), values the same bits.
  tier B   (40 x 56 A = 2e-2, 1e-3; 67 x 33 A = 2e-2, 1e-3)        F_ref      1.50   1.32   1.20   1.03
           kernel, in units of 1e-4 scale                           v_rgb      0.010  0.44   1.18   0.85
                                                                    v_alpha    0.005  0.35   0.94   0.34
           at most 0.25 of the tier's bound per element.  Loss value: kernel 1.8e-4, 5.2e-5, 7.7e-5, 4.6e-4 relative against the
           float32 reference's 1.9e-3, 1.3e-3, 6.2e-4, 8.6e-4: at most 0.13 of the tier's bound.  (1 - SSIM alone: kernel 8e-4 ... 0.14
           relative, reference 6e-3 ... 0.42.)  The kernel needed no change for this tier and no assertion is marked xfail.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_budget as lb

pytestmark = pytest.mark.gpu

TIER_A = [(H, W, srgb, mw) for (H, W) in lb.TIER_A_SHAPES + (lb.TIER_A_WIDE,) for srgb in (True, False) for mw in (5.0, 0.0)]
GUARD = 4096
FILL = 0xA5


def _run(cuda, inputs, srgb, mask_weight, grad_scale=1.0):
    from geosplatting_amd.loss import photo_loss_and_grad
    rgb, alpha, gt, bg = (t.to(cuda) for t in inputs)
    out, v_rgb, v_alpha = photo_loss_and_grad(rgb, alpha, gt, bg, grad_scale=grad_scale, metric_bg=torch.zeros(3, device=cuda),
                                              gt_is_srgb=srgb, use_mask_loss=mask_weight > 0)
    return out.cpu(), v_rgb.cpu(), v_alpha.cpu()


def _values(out):
    return {k: float(out[i].double()) for i, k in enumerate(lb.VALUE_KEYS)}


def _assert_values(got, want, what):
    ve = lb.value_errors(got, want)
    for k in ("loss", "ssim_loss", "l1", "mask_mse", "mse_srgb"):
        assert ve[k] <= 1e-4, (what, k, got[k], want[k])
    assert ve["psnr"] <= 1e-3, (what, got["psnr"], want["psnr"])
    return max(ve[k] for k in ("loss", "ssim_loss", "l1", "mask_mse", "mse_srgb"))


@pytest.mark.parametrize("H,W,srgb,mask_weight", TIER_A)
def test_tier_a_per_element(cuda, H, W, srgb, mask_weight):
    inputs, bud = lb.tier_a_case(H, W, srgb, mask_weight)
    out, v_rgb, v_alpha = _run(cuda, inputs, srgb, mask_weight)
    f_rgb = lb.fraction(v_rgb, bud["d_rgb"], bud["bound_rgb"])
    f_alpha = lb.fraction(v_alpha, bud["d_alpha"], bud["bound_alpha"])
    ve = lb.value_errors(_values(out), bud["values"])
    sf = lb.scale_fractions(v_rgb, v_alpha, bud)
    print(f"\n  A {H}x{W} srgb={srgb} mask_weight={mask_weight}: fraction of the bound v_rgb {f_rgb:.4f} v_alpha {f_alpha:.4f} "
          f"(away from l1_fragile: {sf['rgb']:.4f} {sf['alpha']:.4f}; float32 reference {lb.f_ref(bud):.4f}); value rel err {max(v for k, v in ve.items() if k != 'psnr'):.2e} psnr {ve['psnr']:.1e} dB")
    assert f_rgb <= 1.0, f_rgb
    assert f_alpha <= 1.0, f_alpha
    _assert_values(_values(out), bud["values"], (H, W, srgb, mask_weight))


@pytest.mark.parametrize("H,W,srgb", [(27, 27, True), (37, 53, False)])
def test_tier_a_grad_scale(cuda, H, W, srgb):
    """grad_scale 1/8: within the budget per element, within 2 ulp of the float32 product with the grad_scale 1 result, values the same bits"""
    inputs, bud = lb.tier_a_case(H, W, srgb, 5.0, 0.125)
    out1, r1, a1 = _run(cuda, inputs, srgb, 5.0, 1.0)
    out8, r8, a8 = _run(cuda, inputs, srgb, 5.0, 0.125)
    f_rgb = lb.fraction(r8, bud["d_rgb"], bud["bound_rgb"])
    f_alpha = lb.fraction(a8, bud["d_alpha"], bud["bound_alpha"])
    print(f"\n  A {H}x{W} grad_scale=1/8: fraction of the bound v_rgb {f_rgb:.4f} v_alpha {f_alpha:.4f}")
    assert f_rgb <= 1.0 and f_alpha <= 1.0, (f_rgb, f_alpha)
    assert torch.equal(out1, out8)
    for g1, g8 in ((r1, r8), (a1, a8)):
        prod = (g1 * 0.125).numpy()
        ulps = np.abs(g8.numpy().astype(np.float64) - prod.astype(np.float64)) / np.spacing(np.abs(prod)).astype(np.float64)
        print(f"  against the float32 product: {ulps.max():.2f} ulp")
        assert ulps.max() <= 2.0, ulps.max()


@pytest.mark.parametrize("A", lb.TIER_B_AMPLITUDES)
@pytest.mark.parametrize("H,W", lb.TIER_B_SHAPES)
def test_tier_b_per_element(cuda, H, W, A):
    inputs, bud = lb.tier_b_case(H, W, A)
    F_ref = lb.f_ref(bud)
    margin = max(1.0, 4.0 * F_ref)
    out, v_rgb, v_alpha = _run(cuda, inputs, False, 5.0)
    F_rgb = lb.fraction(v_rgb, bud["d_rgb"], lb.KAPPA * bud["scale_rgb"])
    F_alpha = lb.fraction(v_alpha, bud["d_alpha"], lb.KAPPA * bud["scale_alpha"])
    got, want, ref32 = _values(out), bud["values"], bud["values32"]
    e_loss, e_ref = abs(got["loss"] - want["loss"]), abs(ref32["loss"] - want["loss"])
    allowed = max(1e-4 * abs(want["loss"]), 4.0 * e_ref)
    mx = float((v_rgb.double() - bud["d_rgb"]).abs().max() / bud["d_rgb"].abs().max())
    print(f"\n  B {H}x{W} A={A}: F_ref {F_ref:.3f}; kernel F v_rgb {F_rgb:.3f} v_alpha {F_alpha:.3f} (fraction of the bound "
          f"{max(F_rgb, F_alpha) / margin:.3f}); gradient max-norm error {mx:.2e}; loss rel err {e_loss / abs(want['loss']):.2e} "
          f"(float32 reference {e_ref / abs(want['loss']):.2e}; fraction of the bound {e_loss / allowed:.3f}); ssim_loss rel err "
          f"{abs(got['ssim_loss'] - want['ssim_loss']) / abs(want['ssim_loss']):.2e} "
          f"(reference {abs(ref32['ssim_loss'] - want['ssim_loss']) / abs(want['ssim_loss']):.2e})")
    assert F_rgb <= margin, (F_rgb, F_ref)
    assert F_alpha <= margin, (F_alpha, F_ref)
    assert e_loss <= allowed, (got["loss"], want["loss"], ref32["loss"])
    # the terms that do not cancel keep the contract
    ve = lb.value_errors(got, want)
    assert ve["l1"] <= 1e-4 and ve["mse_srgb"] <= 1e-4 and ve["psnr"] <= 1e-3 and got["mask_mse"] == 0.0, ve


def _raw(cuda, inputs, srgb, with_grad):
    """gs_photo_loss through the C ABI on a workspace of exactly gs_photo_loss_ws_bytes inside a filled buffer -> (out, buffer, nbytes)"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    rgb, alpha, gt, bg = (t.to(cuda).contiguous() for t in inputs)
    H, W = rgb.shape[0], rgb.shape[1]
    nbytes = lib.gs_photo_loss_ws_bytes(W, H)
    assert nbytes == 4 * (9 * W * H + 4 * ((W + 15) // 16) * ((H + 15) // 16))
    buf = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    out = torch.full((8,), -7.0, device=cuda)
    mb = torch.zeros(3, device=cuda)
    v_rgb = torch.empty_like(rgb) if with_grad else None
    v_alpha = torch.empty_like(alpha) if with_grad else None
    L.check(lib.gs_photo_loss(W, H, L.ptr(rgb), L.ptr(alpha), L.ptr(gt), int(srgb), L.ptr(bg), L.ptr(mb), 0.2, 5.0, 1.0, L.ptr(out),
                              L.ptr(v_rgb), L.ptr(v_alpha), L.ptr(buf), C.c_size_t(nbytes), L.stream()), "gs_photo_loss")
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu(), nbytes, v_rgb


def test_value_only_call_same_bits_and_workspace_bounds(cuda):
    """v_rgb = v_alpha = NULL (maps == nullptr in the stats kernel): out[0:6] the bits of the call with gradients, nothing behind
    out[5] written, nothing behind the workspace written, and the nine maps of the workspace not written at all"""
    H = W = 27
    inputs, bud = lb.tier_a_case(H, W, True, 5.0)
    out_g, buf_g, nbytes, v_rgb = _raw(cuda, inputs, True, True)
    out_v, buf_v, _, _ = _raw(cuda, inputs, True, False)
    assert torch.equal(out_g[:6], out_v[:6]) and torch.isfinite(out_v[:6]).all()
    assert (out_g[6:] == -7.0).all() and (out_v[6:] == -7.0).all()
    assert (buf_g[nbytes:] == FILL).all() and (buf_v[nbytes:] == FILL).all()
    n_maps = 4 * 9 * W * H
    assert (buf_v[:n_maps] == FILL).all()
    assert not (buf_v[n_maps:nbytes] == FILL).all() and not (buf_g[:n_maps] == FILL).all()
    _assert_values(_values(out_v), bud["values"], "value-only")
    assert lb.fraction(v_rgb.cpu(), bud["d_rgb"], bud["bound_rgb"]) <= 1.0


def test_two_calls_same_bits(cuda):
    for inputs, srgb in ((lb.tier_a_case(37, 53, True, 5.0)[0], True), (lb.tier_b_case(40, 56, 1e-3)[0], False)):
        a, b = _run(cuda, inputs, srgb, 5.0), _run(cuda, inputs, srgb, 5.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
