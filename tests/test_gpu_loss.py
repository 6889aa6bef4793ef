"""Loss-side HIP kernels (csrc/gs_loss.hip) vs the reference golden and float64 autograd of oracle/loss_ref.py."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _case(H, W, seed, gt_is_srgb=True):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    alpha = torch.sigmoid((0.6 - (xx * xx + yy * yy).sqrt()) * 10)[..., None]
    rgb = (0.5 + 0.5 * torch.sin(torch.stack([3 * xx, 4 * yy, 5 * (xx + yy)], -1))) * alpha
    rgb = rgb + 0.05 * torch.rand(H, W, 3, generator=g) * alpha
    mask = (((xx - 0.1) ** 2 + yy * yy).sqrt() < 0.55).float()[..., None]
    gt = (0.5 + 0.4 * torch.cos(torch.stack([2 * xx, 3 * yy, xx - yy], -1)) + 0.1 * torch.rand(H, W, 3, generator=g)).clamp(0, 1)
    gt[:3, :3] = 0.01
    return rgb, alpha, torch.cat([gt, mask], -1), torch.rand(H, W, 3, generator=g)


def test_loss_golden():
    """value against the reference's own loss glue (tests/golden/ref_loss.npz)"""
    from geosplatting_amd.loss import photo_loss
    g = np.load(os.path.join(GOLD, "ref_loss.npz"))
    t = lambda k: torch.tensor(g[k]).cuda()
    loss, m = photo_loss(t("rgb"), t("alpha"), t("gt_rgba"), t("train_bg"), metric_bg=t("bg_color"))
    assert abs(loss.item() - float(g["loss"])) < 1e-4 * float(g["loss"])
    assert abs(0.2 * m["ssim_loss"].item() + 0.8 * m["l1"].item() - float(g["ssim_l1"])) < 1e-4 * float(g["ssim_l1"])
    assert abs(m["psnr"].item() - float(g["psnr"])) < 1e-3


@pytest.mark.parametrize("H,W,srgb,mask_loss", [(40, 56, True, True), (67, 33, False, True), (128, 128, True, False),
                                                 (11, 11, True, True)])
def test_loss_value_and_gradient_vs_float64(H, W, srgb, mask_loss):
    """1e-4 relative on the value and on the gradient in max-norm (relative to its largest element), on textured, noisy inputs with
    local variances of 1e-2 and more.  It is no property of a float32 evaluation of the formula on a smooth, bright, opaque render,
    where E[xx] - mu^2 cancels against c2: there torch's own float32 evaluation misses it by two orders of magnitude.  The per-element
    bound, the shapes at the tile edges and that regime are in tests/test_gpu_loss_budget.py."""
    from geosplatting_amd.loss import photo_loss
    rgb, alpha, gt, bg = _case(H, W, H * 1000 + W, srgb)
    rc = rgb.cuda().requires_grad_(True); ac = alpha.cuda().requires_grad_(True)
    loss, m = photo_loss(rc, ac, gt.cuda(), bg.cuda(), metric_bg=torch.tensor([0.0, 0.0, 0.0]).cuda(), gt_is_srgb=srgb,
                         use_mask_loss=mask_loss)
    (loss * 3.0).backward()
    rd = rgb.double().requires_grad_(True); ad = alpha.double().requires_grad_(True)
    ref = loss_ref.view_loss(rd, ad, gt.double(), bg.double(), gt_is_srgb=srgb, mask_weight=5.0 if mask_loss else 0.0,
                             metric_bg=torch.zeros(3, dtype=torch.float64))
    (ref["loss"] * 3.0).backward()
    assert abs(loss.item() - ref["loss"].item()) < 1e-4 * abs(ref["loss"].item())
    for k in ("ssim_loss", "l1", "mask_mse", "psnr"):
        assert abs(m[k].item() - ref[k].item()) < 1e-4 * max(abs(ref[k].item()), 1e-3), k
    for got, want in ((rc.grad, rd.grad), (ac.grad, ad.grad)):
        err = (got.cpu().double() - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-4, err


def test_loss_full_size_properties_and_errors():
    """800x800 (BASELINE size): identical images -> SSIM loss 0, L1 0, zero colour gradient; determinism; errors"""
    from geosplatting_amd import _lib
    from geosplatting_amd.loss import photo_loss, photo_loss_and_grad
    H = W = 800
    g = torch.Generator().manual_seed(9)
    gt_lin = torch.rand(H, W, 3, generator=g)
    mask = torch.ones(H, W, 1)
    bg = torch.rand(H, W, 3, generator=g).cuda()
    gt = torch.cat([gt_lin, mask], -1).cuda()
    out, v_rgb, v_alpha = photo_loss_and_grad(gt_lin.cuda(), mask.cuda(), gt, bg, gt_is_srgb=False)
    assert abs(out[1].item()) < 1e-6 and out[2].item() == 0.0 and out[3].item() == 0.0
    assert v_rgb.abs().max().item() < 1e-9
    rgb, alpha, gt2, bg2 = _case(H, W, 4)
    a = photo_loss_and_grad(rgb.cuda(), alpha.cuda(), gt2.cuda(), bg2.cuda(), grad_scale=0.125)
    b = photo_loss_and_grad(rgb.cuda(), alpha.cuda(), gt2.cuda(), bg2.cuda(), grad_scale=0.125)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                       # fixed-order reduction: bit-identical
    c = photo_loss_and_grad(rgb.cuda(), alpha.cuda(), gt2.cuda(), bg2.cuda(), grad_scale=1.0)
    assert torch.allclose(c[1] * 0.125, a[1], rtol=1e-5, atol=1e-12)           # linear in grad_scale
    with pytest.raises(_lib.GeoSplatHipError):
        photo_loss(rgb[:10, :10].cuda(), alpha[:10, :10].cuda(), gt2[:10, :10].cuda(), bg2[:10, :10].cuda())
    with pytest.raises(_lib.GeoSplatHipError):
        photo_loss(rgb, alpha, gt2, bg2)                                       # CPU tensors: no CPU path
