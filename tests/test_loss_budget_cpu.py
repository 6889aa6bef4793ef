"""The photometric loss's float64 reference and its per-element budget (tests/loss_budget.py), without a GPU: what a float32 evaluation
of the formula can and cannot hold, from oracle/loss_ref.view_loss in float32 against float64 alone.

Tier A (the inputs of tests/test_gpu_loss_budget.py: textured, edges, transparent block, out-of-range colours): the float32 reference
stays within 1e-4 of the sum of absolute per-window contributions per element -- measured: at most 0.042 of it on the shape grid
(37 x 53) and 0.11 at 12 x 4097; where an element is l1_fragile the error is the L1 jump's half, 0.5 of the bound (11 x 40,
12 x 4097).  The share of l1_fragile elements is capped at 1 %; measured at most 0.15 % (two elements of 11 x 40).

Tier B (opaque, bright, slowly modulated: the converged regime): the same float32 reference is 1.0 ... 1.5 times the bound per
element, 2e-2 ... 6e-2 in max-norm on the gradient, 6e-4 ... 2e-3 relative on the loss and 6e-3 ... 0.4 relative on 1 - SSIM -- E[xx] - mu^2
cancels against c2 = 9e-4.  Asserted: finite, and at least ten times tier A's worst (otherwise the tier would test nothing new).
"""
import math

import pytest
import torch

from tests import loss_budget as lb

TIER_A = [(H, W, srgb, mw) for (H, W) in lb.TIER_A_SHAPES + (lb.TIER_A_WIDE,) for srgb in (True, False) for mw in (5.0, 0.0)]


def _tier_a_f_ref():
    """tier A's figure for the comparison with tier B: the worst of the shape grid.  (The 12 x 4097 case is there for the finalize
    loop; with two rows of windows and 49 164 pixels its own worst is 0.11, printed by its test.)"""
    return max(lb.f_ref(lb.tier_a_case(*c)[1]) for c in TIER_A if (c[0], c[1]) != lb.TIER_A_WIDE)


@pytest.mark.parametrize("H,W,srgb,mask_weight", TIER_A)
def test_float32_reference_within_budget_tier_a(H, W, srgb, mask_weight):
    (rgb, alpha, gt, bg), bud = lb.tier_a_case(H, W, srgb, mask_weight)
    share = float(bud["l1_fragile"].double().mean())
    fr = lb.reference_fractions(bud)
    ve = lb.value_errors(bud["values32"], bud["values"])
    print(f"\n  {H}x{W} srgb={srgb} mask_weight={mask_weight}: l1_fragile share {share:.5f}; float32 reference: fraction of the bound "
          f"d_rgb {fr['rgb']:.3f} d_alpha {fr['alpha']:.3f}, of 1e-4 scale alone {lb.f_ref(bud):.3f}; loss rel err {ve['loss']:.1e}")
    assert share <= lb.FRAGILE_CAP
    assert fr["rgb"] <= 1.0 and fr["alpha"] <= 1.0
    # the inputs hold what the tier promises
    x, y = bud["x"], bud["y"]
    blk = (slice(2, 5), slice(W - 5, W))
    assert (x[blk] == y[blk]).all() and (alpha[blk] == 0).all() and (gt[blk][..., 3] == 0).all()
    assert not bud["l1_fragile"][blk].any() and (bud["d_rgb"][blk].abs() <= bud["scale_rgb"][blk]).all()
    assert rgb.max() > 1 and rgb.min() < 0 and (gt[..., :3] == 0).any() and (gt[..., :3] == 1).any()
    assert ((gt[..., :3] > 0.04) & (gt[..., :3] <= 0.04045)).any() and ((gt[..., :3] > 0.04045) & (gt[..., :3] < 0.041)).any()
    assert ((alpha > 0.05) & (alpha < 0.95)).any() and (gt[..., 3:] != (alpha > 0.5).float()).any()
    assert (bud["scale_rgb"] > 0).all() and (bud["d_rgb"].abs() <= bud["scale_rgb"] * (1 + 1e-12)).all()
    assert (bud["d_alpha"].abs() <= bud["scale_alpha"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("A", lb.TIER_B_AMPLITUDES)
@pytest.mark.parametrize("H,W", lb.TIER_B_SHAPES)
def test_float32_reference_is_ill_conditioned_tier_b(H, W, A):
    (rgb, alpha, gt, bg), bud = lb.tier_b_case(H, W, A)
    F_ref, F_a = lb.f_ref(bud), _tier_a_f_ref()
    ve = lb.value_errors(bud["values32"], bud["values"])
    mx = float((bud["d_rgb32"] - bud["d_rgb"]).abs().max() / bud["d_rgb"].abs().max())
    print(f"\n  {H}x{W} A={A}: F_ref {F_ref:.3f} (tier A's worst {F_a:.3f}); gradient max-norm error {mx:.2e}; value rel err loss "
          f"{ve['loss']:.1e} ssim_loss {ve['ssim_loss']:.1e} l1 {ve['l1']:.1e}")
    assert math.isfinite(F_ref) and all(math.isfinite(v) for v in ve.values())
    assert F_ref > 10 * F_a
    assert not bud["l1_fragile"].any() and (alpha == 1).all() and (gt[..., 3] == 1).all()
    for t in (rgb, gt[..., :3]):                                   # never constant: every 11 x 11 window of every channel varies
        p = t.permute(2, 0, 1)[None]
        spread = torch.nn.functional.max_pool2d(p, 11, 1) + torch.nn.functional.max_pool2d(-p, 11, 1)
        assert (spread > 0).all()


def test_scale_matches_the_window_loop():
    """scale_rgb (conv_transpose2d) against an explicit loop over the 1 x 3 windows of an 11 x 13 image, to 1e-12"""
    rgb, alpha, gt, bg = (t.double() for t in lb.tier_a_inputs(11, 13, True))
    x, y = lb._blend(rgb, alpha, gt, bg, True)
    for lam, gs in ((0.2, 1.0), (0.7, 0.125)):
        a, b = lb.scale_rgb(x, y, lam, gs), lb.scale_rgb_bruteforce(x, y, lam, gs)
        assert float(((a - b).abs() / b).max()) <= 1e-12


def test_partials_reproduce_the_autograd_gradient():
    """the kernel's chain rule, restated in float64 with signs, is the autograd gradient: G^T dmu + 2 x G^T dvx + y G^T dcxy (times
    -w_ssim) plus the L1 term -- so the scale sums the absolute values of the terms that make up the gradient, not of something else"""
    for (H, W, srgb) in ((22, 27, True), (37, 53, False)):
        (rgb, alpha, gt, bg), bud = lb.tier_a_case(H, W, srgb, 5.0)
        x, y = bud["x"], bud["y"]
        dmu_terms, dvx, dcxy, G = lb._window_partials(x, y)
        k = G[None, None]
        gT = lambda t: torch.nn.functional.conv_transpose2d(t[:, None], k)[:, 0].permute(1, 2, 0)
        w_ssim = 0.2 / (3.0 * (H - 10) * (W - 10))
        g = -w_ssim * (gT(sum(dmu_terms)) + 2 * x * gT(dvx) + y * gT(dcxy)) + 0.8 / (3.0 * H * W) * torch.sign(x - y)
        assert float((g - bud["d_rgb"]).abs().max()) <= 1e-12 * float(bud["scale_rgb"].max())
        ga = -(bg.double() * g).sum(-1, keepdim=True) + 2 * 5.0 / (H * W) * (alpha.double() - gt[..., 3:].double())
        assert float((ga - bud["d_alpha"]).abs().max()) <= 1e-12 * float(bud["scale_alpha"].max())


def test_a_wrong_border_pixel_fails_the_budget_and_passes_max_norm():
    """The SSIM part of ONE gradient element in the five-pixel border band (which fewer windows reach) off by 1 % -- what a wrong tap or
    a wrong halo value does there.  The L1 term has the same size in every element, so the largest gradient of the image is about
    ten times it and the max-norm criterion of tests/test_gpu_loss.py (1e-4 of the largest element) accepts any such error below a
    tenth of the L1 weight; of the band's elements whose error it accepts, the test takes the one that shows best against the budget."""
    H, W = 37, 53
    (rgb, alpha, gt, bg), bud = lb.tier_a_case(H, W, True, 0.0)
    want = bud["d_rgb"]
    w_l1 = 0.8 / (3.0 * H * W)
    delta = 0.01 * (want - w_l1 * torch.sign(bud["x"] - bud["y"]))
    band = torch.ones(H, W, 1, dtype=torch.bool)
    band[5:H - 5, 5:W - 5] = False
    accepted = band & (delta.abs() < 0.9e-4 * want.abs().max())
    frac = torch.where(accepted, delta.abs() / bud["bound_rgb"], torch.zeros_like(delta))
    i = int(frac.argmax())
    e = (i // (3 * W), (i // 3) % W, i % 3)
    print(f"\n  element {e}: SSIM part {float(delta[e]) / 0.01 / w_l1:.3f} x the L1 weight; 1 % of it = {float(frac[e]):.1f} x the bound, "
          f"{float(delta[e].abs() / want.abs().max()):.1e} of the largest gradient")
    got = want.clone()
    got[e] += delta[e]
    assert 0 < float((got - want).abs().max() / want.abs().max()) < 1e-4              # passes max-norm
    assert lb.fraction(want, want, bud["bound_rgb"]) == 0.0
    assert lb.fraction(got, want, bud["bound_rgb"]) > 1.5                              # measured: 3.7
