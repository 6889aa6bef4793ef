"""The smoothing regularisers of the stage-1 trainer (smooth_type 'grad' / 'tv', normal_grad_weight: rfstudio/model/geosplat.py:881-922)
on the fused step: the loss kernel (csrc/gs_smooth.hip) against stage1._edge_aware / _tv under torch autograd, the engine's attribute
renders against rasterization(), the shaded images untouched, and train_step_fused against train_step (one and two ranks)."""
import math
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_gpu_stage1 import HW, N_VIEWS, ROOT, _free_port, _model, _scene

pytestmark = pytest.mark.gpu


def _quantised(shape, g, flat_value=None):
    """Random values on a 1/256 grid (the Sobel sums are then exact in fp32 and fp64 alike: the same signs, the same exact zeros
    on both sides) with a constant patch -- a flat region whose Sobel response is exactly 0."""
    x = torch.randint(0, 257, shape, generator=g).double() / 256.0
    H, W = shape[0], shape[1]
    x[H // 4: H // 2, W // 4: W // 2] = 0.5 if flat_value is None else flat_value
    return x


def _reference(img, gt, kinds, weights):
    """sum_i w_i * term_i(render i) by stage1._edge_aware / _tv on the host in fp64, with its gradient by autograd"""
    from geosplatting_amd.loss import SMOOTH_EDGE, SMOOTH_TV
    from geosplatting_amd.stage1 import _edge_aware, _tv
    x = img.clone().requires_grad_(True)
    total = x.new_zeros(())
    for i, (k, w) in enumerate(zip(kinds, weights)):
        r = x[..., 3 * i: 3 * i + 3]
        if k == SMOOTH_EDGE:
            total = total + _edge_aware(r, gt) * w
        elif k == SMOOTH_TV:
            total = total + _tv(r) * w
    total.backward()
    return float(total.detach()), x.grad


@pytest.mark.parametrize("H,W", [(96, 96), (37, 53), (800, 800)])
def test_smooth_loss_kernel_matches_torch(cuda, H, W):
    from geosplatting_amd.loss import SMOOTH_EDGE as E, SMOOTH_NONE as N, SMOOTH_TV as T, smooth_loss_and_grad
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = _quantised((H, W, 9), g)
    gt = _quantised((H, W, 3), g, flat_value=0.25)
    cases = [((E, E, E), (0.0, 0.7, 0.3)), ((E, E, E), (1.5, 0.0, 0.3)), ((E, E, E), (1.5, 0.7, 0.0)),
             ((T, T, N), (2.0, 1.0, 0.0)), ((T, T, E), (2.0, 1.0, 0.4))]
    for kinds, weights in cases:
        kinds = tuple(k if w > 0 else N for k, w in zip(kinds, weights))
        want, want_g = _reference(img, gt, kinds, weights)
        args = (img.float().to(cuda), gt.float().to(cuda) if E in kinds else None, kinds, weights)
        out, v = smooth_loss_and_grad(*args)
        got, got_g = float(out), v.double().cpu()
        assert abs(got - want) <= 1e-5 * abs(want), (kinds, weights, got, want)
        err = (got_g - want_g).abs().max().item() / want_g.abs().max().item()
        assert err <= 1e-5, (kinds, weights, err)
        # inside the flat patch (two pixels in from its edge every Sobel response and difference around a pixel is 0): exact zeros
        flat = (slice(H // 4 + 2, H // 2 - 2), slice(W // 4 + 2, W // 2 - 2))
        assert got_g[flat].abs().max() == 0 and want_g[flat].abs().max() == 0, (kinds, weights)
        out2, v2 = smooth_loss_and_grad(*args)
        assert torch.equal(out, out2) and torch.equal(v, v2), "two calls differ"
        # ADDS into a given scalar
        acc = torch.full((), 1.0, device=cuda)
        smooth_loss_and_grad(*args, out=acc)
        assert abs(float(acc) - 1.0 - got) <= 1e-6 * max(1.0, got)


def _abs_scale(img, gt, kinds, weights):
    """per element of d(sum)/d(img): the float64 sum of the absolute stencil contributions -- edge-aware: the reference's backward with
    the absolute Sobel cotangents |sign(S(r))| exp(-|S(gt)|) w / (3 H W) through the absolute stencil weights (replicate padding as in
    the forward); TV: gscale (|up| + |dn|) + gscale_x (|lf| + |rt|) with the forward differences around the element"""
    from geosplatting_amd.loss import SMOOTH_EDGE, SMOOTH_TV
    from geosplatting_amd.stage1 import spatial_gradient
    H, W = img.shape[0], img.shape[1]
    S = torch.zeros_like(img)
    kx = torch.tensor([[1.0, 0.0, 1.0], [2.0, 0.0, 2.0], [1.0, 0.0, 1.0]], dtype=img.dtype) / 8.0
    k_abs = torch.stack((kx, kx.t()))[:, None]
    for i, (k, w) in enumerate(zip(kinds, weights)):
        r = img[..., 3 * i: 3 * i + 3]
        if k == SMOOTH_EDGE:
            cot = (spatial_gradient(r) != 0).double() * (-spatial_gradient(gt).abs()).exp() * (w / (3.0 * H * W))      # [3,2,H,W]
            z = torch.zeros(3, 1, H, W, dtype=img.dtype, requires_grad=True)
            y = torch.nn.functional.conv2d(torch.nn.functional.pad(z, (1, 1, 1, 1), mode="replicate"), k_abs)
            (y * cot).sum().backward()
            S[..., 3 * i: 3 * i + 3] = z.grad[:, 0].permute(1, 2, 0)
        elif k == SMOOTH_TV:
            dy, dx = (r[1:] - r[:-1]).abs(), (r[:, 1:] - r[:, :-1]).abs()
            s = torch.zeros_like(r)
            gy, gx = 2.0 * w / (3.0 * (H - 1) * W), 2.0 * w / (3.0 * H * (W - 1))
            s[:-1] += gy * dy; s[1:] += gy * dy                     # |dn| of the upper pixel, |up| of the lower one
            s[:, :-1] += gx * dx; s[:, 1:] += gx * dx
            S[..., 3 * i: 3 * i + 3] = s
    return S


@pytest.mark.parametrize("H,W", [(2, 2), (2, 17), (3, 3), (16, 16), (17, 17), (17, 33)])
def test_smooth_loss_kernel_per_element(cuda, H, W):
    """the smallest images the entry accepts and images whose replicate-padded halo clamps on both sides inside one tile: every
    gradient element within 1e-5 of the float64 sum of the absolute stencil contributions to it (not of the image's largest
    gradient), exact zeros where the reference has exact zeros"""
    from geosplatting_amd.loss import SMOOTH_EDGE as E, SMOOTH_NONE as N, SMOOTH_TV as T, smooth_loss_and_grad
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = _quantised((H, W, 9), g)
    gt = _quantised((H, W, 3), g, flat_value=0.25)
    cases = [((E, E, E), (0.0, 0.7, 0.3)), ((E, E, E), (1.5, 0.0, 0.3)), ((E, E, E), (1.5, 0.7, 0.0)),
             ((T, T, N), (2.0, 1.0, 0.0)), ((T, T, E), (2.0, 1.0, 0.4))]
    for kinds, weights in cases:
        kinds = tuple(k if w > 0 else N for k, w in zip(kinds, weights))
        want, want_g = _reference(img, gt, kinds, weights)
        S = _abs_scale(img, gt, kinds, weights)
        assert (want_g.abs() <= S * (1 + 1e-12)).all()
        out, v = smooth_loss_and_grad(img.float().to(cuda), gt.float().to(cuda) if E in kinds else None, kinds, weights)
        got_g = v.double().cpu()
        assert abs(float(out) - want) <= 1e-5 * abs(want), (kinds, weights, float(out), want)
        err = (got_g - want_g).abs()
        frac = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        print(f"\n  {H}x{W} {kinds} {weights}: largest fraction of 1e-5 S {float(frac.max()) / 1e-5:.4f}; exact zeros {int((want_g == 0).sum())}")
        assert float(frac.max()) <= 1e-5, (kinds, weights, float(frac.max()))
        assert (got_g[want_g == 0] == 0).all(), (kinds, weights)


def _step_scene(dev):
    import geosplatting_amd.synthetic as syn
    from geosplatting_amd.cameras import orbit_cameras
    from geosplatting_amd.engine import params_from_scene
    scene = syn.sphere_scene(2, seed=1, cubemap_res=64)
    res = 96
    cams = orbit_cameras(8, 4.0 * (2.0 / 3.0), 30.0, res, res, focal=0.5 * res / math.tan(0.5 * 0.6911112))[1:4]
    return params_from_scene(scene, dev, exposure=1.1), cams, res


def _smoothing(dev, res, n):
    from geosplatting_amd.engine import Smoothing
    from geosplatting_amd.loss import SMOOTH_EDGE as E
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(res, res, 3, generator=g).to(dev) for _ in range(n)]
    return Smoothing((E, E, E), (0.2, 0.1, 0.3), torch.tensor([1.0, 0.5, 0.25], device=dev), gts)


def test_engine_shaded_images_unchanged_and_attribute_renders(cuda):
    """Smoothing on: the shaded images are the same bits; the attribute renders are what rasterization() composites from
    (kd, 0, ks, n * 0.5 + 0.5) over the background tiled to nine channels"""
    from geosplatting_amd import rasterization
    from geosplatting_amd.engine import RenderStep
    params, cams, res = _step_scene(cuda)
    step = RenderStep(params)
    g = torch.Generator().manual_seed(0)
    vs = [(torch.rand(res, res, 4, generator=g) * 2 - 1).to(cuda) for _ in cams]
    up = lambda i, img: vs[i]
    sm = _smoothing(cuda, res, len(cams))
    for eager in (True, False):                               # exact mode, then capacity mode
        _, plain = step(cams, up, all_reduce=False, keep_images=True)
        plain = [t.clone() for t in plain]
        _, shaded = step(cams, up, all_reduce=False, keep_images=True, smoothing=sm)
        attrs = step.last_attribute_renders
        torch.cuda.synchronize()
        for a, b in zip(plain, shaded):
            assert torch.equal(a, b), "smoothing changed the shaded image"
        assert float(step.last_smoothing_loss) > 0
        assert step.poll_capacity(wait=True)
    p = params
    cols = torch.cat((p.kd, torch.zeros_like(p.ks[:, :1]), p.ks, p.normals * 0.5 + 0.5), -1).contiguous()
    bg9 = sm.background.repeat(3)
    for cam, got in zip(cams, attrs):
        render, _, _ = rasterization(p.means, p.quats, p.scales.exp(), torch.sigmoid(p.opacities).squeeze(-1), cols,
                                     cam.view_matrix.to(cuda)[None], cam.intrinsic_matrix.to(cuda)[None], res, res,
                                     backgrounds=bg9[None])
        want = render.reshape(res, res, 9)
        err = (got - want).abs().max().item()
        assert torch.equal(got, want), f"attribute render differs from rasterization() by {err:.3e}"


def test_capture_and_non_fused_paths_refuse_smoothing(cuda):
    from geosplatting_amd.engine import RenderStep
    params, cams, res = _step_scene(cuda)
    sm = _smoothing(cuda, res, len(cams))
    up = lambda i, img: torch.zeros_like(img)
    step = RenderStep(params)
    step(cams, up, all_reduce=False)
    step.poll_capacity(wait=True)
    with pytest.raises(NotImplementedError):
        step.capture(cams, up, smoothing=sm)
    with pytest.raises(NotImplementedError):
        step.capture_views(cams, up, all_reduce=False, smoothing=sm)
    with pytest.raises(NotImplementedError):
        RenderStep(params, fused=False)(cams, up, all_reduce=False, smoothing=sm)


CASES = {"grad+normal": ("grad", 0.3), "tv": ("tv", 0.0), "jitter+normal": ("jitter", 0.3)}


def _grads(dev, rank, world, fused, case):
    from geosplatting_amd.stage1 import train_step, train_step_fused
    fn = train_step_fused if fused else train_step
    torch.manual_seed(11)
    cams, gts, grid = _scene(dev)
    model = _model(dev, grid)
    model.kd_regualr_perturb_std = model.ks_regualr_perturb_std = 0.0
    model.smooth_type, model.normal_grad_weight = CASES[case]
    bgs = [torch.rand(HW, HW, 3, generator=torch.Generator().manual_seed(70 + i)).to(dev) for i in range(N_VIEWS)]
    m = fn(model, cams, gts, gt_is_srgb=False, rank=rank, world_size=world, train_bg=bgs)
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().clone() for k, v in model.named_parameters().items()}
    return grads, float(m["regularization"].detach()), float(model._last_smoothing.detach())


def _compare(want, got, what):
    for k, w in want.items():
        err = (got[k] - w).abs().max().item() / (w.abs().max().item() + 1e-30)
        assert err < 5e-4, (what, k, err)


@pytest.mark.parametrize("case", list(CASES))
def test_fused_step_with_smoothing_equals_autograd_step(cuda, case):
    """fails at the parent commit: train_step_fused raised NotImplementedError for every one of these configurations"""
    want, reg_w, sm_w = _grads(cuda, 0, 1, False, case)
    got, reg_g, sm_g = _grads(cuda, 0, 1, True, case)
    assert sm_w > 0 and abs(sm_g - sm_w) <= 1e-5 * sm_w, (sm_g, sm_w)
    assert abs(reg_g - reg_w) <= 1e-5 * abs(reg_w), (reg_g, reg_w)
    _compare(want, got, case)


def _worker(rank, world, port, out_dir, case):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      GEOSPLAT_DEBUG_SHARE_GPU="1")
    import torch.distributed as dist
    from geosplatting_amd.parallel import init_distributed_from_env
    r, w, dev = init_distributed_from_env("cuda")
    torch.save(_grads(dev, r, w, True, case)[0], os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_fused_step_with_smoothing_two_ranks_equal_single_process(cuda, tmp_path):
    one = _grads(cuda, 0, 1, True, "grad+normal")[0]
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), "grad+normal"), nprocs=2, join=True)
    for r in range(2):
        _compare(one, torch.load(os.path.join(tmp_path, f"rank{r}.pt")), f"rank{r}")
