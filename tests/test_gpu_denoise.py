"""The bilateral denoiser (csrc/gs_denoise.hip) and RenderableAttrs.splat_mc_deferred on the GPU: every element of forward and backward
against the float64 restatement within its derived budget (tests/denoise_ref.py), the exact properties bit for bit (the two forms, the
channel slices, the batch, the [1,1,N,C] shape, determinism), what the filter means, and the deferred pipeline against its hand
composition.  Shapes are small: windows clip at every border and span several 32 x 8 tiles."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import _lib
from tests import denoise_ref as ref
from tests import envshade_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _past_the_tiled_limit(C: int) -> float:
    """the smallest sigma = (k - 0.5) / 2.5 (radius 2 k + 1, clear of the ceiling's steps) whose halo no longer fits the LDS"""
    k = 1
    while _lib.lib().gs_denoise_tiled_fits(C, (k - 0.5) / 2.5):
        k += 1
    return (k - 0.5) / 2.5


# (shape, sigma, radius, form); None: the op picks
CASES = [((1, 37, 29, 3), 2.0, 11, None), ((2, 19, 23, 3), 1e-4, 3, None), ((1, 1, 300, 3), 2.0, 11, None), ((1, 40, 33, 3), 4.2, 23, True),
         ((1, 40, 33, 3), "past", 25, False)]


def _run(shape, zdz_channels, sigma, tiled=None, seed=0):
    col, nrm, zdz, grad = (t.to(DEV) for t in ref.scene(*shape, zdz_channels, seed))
    col.requires_grad_(True)
    out = gs.bilateral_denoiser(col, nrm, zdz, sigma, tiled=tiled)
    out.backward(grad)
    return out.detach(), col.grad


@pytest.mark.parametrize("zdz_channels", (1, 2))
@pytest.mark.parametrize("shape,sigma,R,tiled", CASES)
def test_forward_and_backward_against_float64(shape, sigma, R, tiled, zdz_channels):
    """Largest error / budget per case, as measured on an MI355X ("Bilateral denoiser")."""
    if sigma == "past":
        sigma = _past_the_tiled_limit(shape[-1])
        with pytest.raises(ValueError, match="does not fit"):
            _run(shape, zdz_channels, sigma, tiled=True)
    assert ref.radius(sigma) == R == gs.filter_radius(sigma)
    if tiled:
        assert _lib.lib().gs_denoise_tiled_fits(shape[-1], sigma) == 1
    want, budget, want_grad, grad_budget = ref.reference(*shape, zdz_channels, sigma)
    out, col_grad = _run(shape, zdz_channels, sigma, tiled)
    worst = {}
    for name, got, exact, bud in (("out", out, want, budget), ("col_grad", col_grad, want_grad, grad_budget)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), name
        err = np.abs(got - exact)
        worst[name] = float((err / bud).max())
    print(f"{shape} sigma={sigma:g} zdz={zdz_channels} tiled={tiled}: error / budget out {worst['out']:.3f} col_grad {worst['col_grad']:.3f}")
    assert worst["out"] <= 1.0 and worst["col_grad"] <= 1.0, worst                     # every element, none excluded


# ---- exact properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sigma", [((1, 37, 29, 3), 2.0), ((2, 19, 23, 8), 1e-4), ((1, 1, 300, 3), 2.0), ((1, 40, 33, 3), 4.2),
                                         ((1, 21, 70, 8), 2.0), ((1, 9, 33, 1), 0.41)])
@pytest.mark.parametrize("zdz_channels", (1, 2))
def test_tiled_equals_plain(shape, sigma, zdz_channels):
    a, b = _run(shape, zdz_channels, sigma, tiled=True), _run(shape, zdz_channels, sigma, tiled=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _run(shape, zdz_channels, sigma)                                               # whichever the op picks
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("tiled", (True, False))
def test_eight_channels_equal_their_slices(tiled):
    col, nrm, zdz, grad = (t.to(DEV) for t in ref.scene(1, 37, 29, 8, 1))
    col.requires_grad_(True)
    out = gs.bilateral_denoiser(col, nrm, zdz, 2.0, tiled=tiled)
    out.backward(grad)
    for lo, hi in ((0, 3), (3, 6), (6, 8), (5, 6)):
        c = col.detach()[..., lo:hi].contiguous().requires_grad_(True)
        o = gs.bilateral_denoiser(c, nrm, zdz, 2.0, tiled=tiled)
        o.backward(grad[..., lo:hi].contiguous())
        assert torch.equal(o, out[..., lo:hi]) and torch.equal(c.grad, col.grad[..., lo:hi])
    # the reference's padded call: a zero channel in front of the residual pair drops out
    pad = torch.cat((torch.zeros_like(col[..., :1]), col.detach()[..., 6:8]), -1)
    assert torch.equal(gs.bilateral_denoiser(pad, nrm, zdz, 2.0, tiled=tiled)[..., 1:], out[..., 6:8])


def test_batch_shapes_and_determinism():
    shape, sigma = (2, 19, 23, 3), 0.5
    col, nrm, zdz, grad = (t.to(DEV) for t in ref.scene(*shape, 2))
    out, col_grad = _run(shape, 2, sigma)
    again = _run(shape, 2, sigma)
    assert torch.equal(out, again[0]) and torch.equal(col_grad, again[1])              # two runs: the same bits
    for b in range(2):
        c = col[b].clone().requires_grad_(True)                                        # [H,W,C]: no batch axis
        o = gs.bilateral_denoiser(c, nrm[b], zdz[b], sigma)
        o.backward(grad[b])
        assert o.shape == (19, 23, 3) and torch.equal(o, out[b]) and torch.equal(c.grad, col_grad[b])
    # the gradient does not depend on col
    other = (col * 3.0 + 1.0).requires_grad_(True)
    gs.bilateral_denoiser(other, nrm, zdz, sigma).backward(grad)
    assert torch.equal(other.grad, col_grad)
    # [1,1,N,C], the reference's stage-2 shape, is the H = 1 image [1,N,C]
    col, nrm, zdz, grad = (t.to(DEV) for t in ref.scene(1, 1, 300, 3, 1))
    row = gs.bilateral_denoiser(col[0], nrm[0], zdz[0], 2.0)
    assert row.shape == (1, 300, 3) and torch.equal(row, _run((1, 1, 300, 3), 1, 2.0)[0][0])
    # non-contiguous inputs and a guide that requires grad: nothing but col gets a gradient
    n2 = nrm.clone().requires_grad_(True)
    c2 = col.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    gs.bilateral_denoiser(c2, n2, zdz, 2.0).backward(grad)
    assert n2.grad is None and torch.equal(c2.grad, _run((1, 1, 300, 3), 1, 2.0)[1])


# ---- what the filter means ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", (True, False))
def test_partition_of_unity_zero_normals_and_the_crease(tiled):
    H, W = 20, 45
    nrm = torch.zeros(1, H, W, 3, device=DEV)
    nrm[..., 2] = 1.0
    zdz = torch.full((1, H, W, 1), 2.0, device=DEV)
    col = torch.full((1, H, W, 2), 0.7, device=DEV)
    col[..., 1] = 123.25
    out = gs.bilateral_denoiser(col, nrm, zdz, 2.0, tiled=tiled)
    # a constant image stays constant: out = sum w c / sum w, W >= 1 from the centre tap (far above the 1e-4 clamp).  Each sum is N = 529
    # FMAs or adds in sequence, each rounding at most u = 2^-24 of the running sum, which never exceeds the final one: N u relative per
    # sum, plus the product's and the quotient's u each -- (2 N + 2) u, the bound the number format gives (measured: 13 ulp)
    ulps = ((out - col).abs() / (2.0 ** -23 * col)).max().item()
    print(f"constant image, tiled={tiled}: largest deviation {ulps:.2f} ulp")
    assert ((out - col).abs() <= (2 * 529 + 2) * 2.0 ** -24 * col).all()
    # a pixel without a normal gives 0, and nobody takes anything from it
    nrm[0, 5, 7] = 0.0
    hot = torch.zeros(1, H, W, 1, device=DEV)
    hot[0, 5, 7] = 1e6
    out = gs.bilateral_denoiser(hot, nrm, zdz, 2.0, tiled=tiled)
    assert (out == 0).all()
    # one hot pixel left of a hard crease (normals 60 degrees apart: w_n = 0.5^128): what leaks across is below w_n * hot / W with
    # W > 1: the receiver's own tap and its neighbours on its side of the crease
    nrm[0, 5, 7, 2] = 1.0
    right = torch.tensor([math.sin(math.radians(60.0)), 0.0, math.cos(math.radians(60.0))], device=DEV)
    nrm[:, :, 23:] = right
    hot = torch.zeros(1, H, W, 1, device=DEV)
    hot[0, 10, 22] = 1e6
    out = gs.bilateral_denoiser(hot, nrm, zdz, 2.0, tiled=tiled)
    w_n = (0.5 + 2.0 ** -20) ** 128
    assert out[0, :, 23:].max().item() <= w_n * 1e6 and out[0, 10, 21].item() > 1e3 and out[0, :, :23].sum().item() > 1e5


# ---- splat_mc_deferred -------------------------------------------------------------------------------------------------------------
_cache = {}


def _bvh():
    if "bvh" not in _cache:
        v, f = envshade_ref.scene_mesh()
        _cache["bvh"] = gs.MeshBVH(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    return _cache["bvh"]


def _splat_scene():
    """the small scene of tests/test_gpu_envshade.py, with the G-buffer positions of its mesh"""
    if "scene" not in _cache:
        v, f = envshade_ref.scene_mesh()
        vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        sp, nrm = gs.mesh_to_splats(vt, ft, gs.vertex_normals(vt, ft))
        g = torch.Generator().manual_seed(2)
        N = sp.means.shape[0]
        leaves = dict(kd=torch.rand(N, 3, generator=g), ks=torch.rand(N, 2, generator=g), occ=torch.randn(N, 6, generator=g) + 3.0)
        light = torch.from_numpy(np.ascontiguousarray(envshade_ref.env_map("16x32")[0])).to(DEV)
        c2w = gs.lookat_c2w(torch.tensor([0.3, 0.4, 3.0]), torch.zeros(3), torch.tensor([0.0, 1.0, 0.0]))
        cam = gs.Camera(c2w.contiguous().to(DEV), 60.0, 60.0, 32.0, 32.0, 64, 64)
        from geosplatting_amd.meshrender import to_camera_space
        rast = gs.rasterize_mesh(to_camera_space(vt, cam), ft, cam)
        positions = gs.interpolate(vt.float().contiguous(), rast, ft)
        mask = (rast[..., -1:] > 0).float()
        _cache["scene"] = (sp, nrm, {k: x.to(DEV) for k, x in leaves.items()}, light, cam, positions, mask)
    return _cache["scene"]


def _by_hand(sp, nrm, lv, env, cam, positions, mask, exposure, mode, denoise, residual, shadow_scale=1.0):
    """geosplat.py:267-376 op by op, the denoiser in three 3-channel calls as the reference writes it"""
    from geosplatting_amd.meshrender import _unit_or_z
    from geosplatting_amd.shading import _rasterize_activated
    lookat, cam_pos = -cam.c2w[:, 2], cam.c2w[:, 3]
    bend = (nrm * lookat).sum(-1, keepdim=True) > 0
    normals = torch.where(bend, -nrm, nrm)
    opac = torch.where(bend, torch.full_like(sp.opacities, -2.0), sp.opacities)
    render, alpha, _ = _rasterize_activated(sp.means, sp.scales, sp.quats, opac, torch.cat((normals, lv["kd"], lv["ks"], lv["occ"]), -1), cam, "RGB")
    render = render / alpha.clamp_min(1e-6)
    n = _unit_or_z(render[..., 0:3])
    kd, rough, metal, occ = render[..., 3:6], render[..., 6:7] * 0.9 + 0.1, render[..., 7:8] * 0.9, render[..., 8:14]
    ks = torch.cat((torch.zeros_like(rough), rough, metal), -1)
    pos = positions.view(1, 64, 64, 3)
    depth = ((pos - cam_pos) * lookat).sum(-1, keepdim=True)
    d, s, r = gs.env_shade(_bvh(), mask.reshape(-1), (n * 1e-3 + pos).reshape(-1, 3), pos.reshape(-1, 3), n.reshape(-1, 3), cam_pos.contiguous(),
                           kd.reshape(-1, 3), ks.reshape(-1, 3), env.data, *env.tables(), n_samples_x=2, rnd_seed=7, shadow_scale=shadow_scale)
    d, s, r = d.view(1, 64, 64, 3).clamp_min(1e-4), s.view(1, 64, 64, 3).clamp_min(1e-4), r.view(1, 64, 64, 2).clamp(0, 1)
    sigma = max(shadow_scale * 2, 0.0001)
    if denoise:
        d = gs.bilateral_denoiser(d, n, depth, sigma)
        s = gs.bilateral_denoiser(s, n, depth, sigma)
    if residual:
        if denoise:
            r = gs.bilateral_denoiser(torch.cat((torch.zeros_like(r[..., :1]), r), -1), n, depth, sigma)[..., 1:]
        rl = (occ - 3).sigmoid()
        d, s = d + r[..., 0:1] * rl[..., :3], s + r[..., 1:2] * rl[..., 3:]
    kdf = kd * (1 - metal)
    col = {"pbr": d * kdf + s, "diffuse": d * kdf, "specular": s}[mode]
    return gs.tone_map(torch.cat((col * alpha, alpha), -1), exposure, "naive").squeeze(0), alpha.squeeze(0)


@pytest.mark.parametrize("mode", ("pbr", "diffuse", "specular"))
def test_splat_mc_deferred_equals_its_pipeline(mode):
    sp, nrm, lv, light, cam, positions, mask = _splat_scene()
    env = gs.LatLngEnvMap(light).compute_pdf_()
    exposure = torch.tensor(1.3, device=DEV)
    attrs = gs.RenderableAttrs(kd=lv["kd"], ks=lv["ks"], normals=nrm, occ=lv["occ"])
    kw = dict(bvh=_bvh(), exposure=exposure, positions=positions, mask=mask, envmap=env, min_roughness=0.1, max_metallic=0.9, mode=mode,
              num_samples_per_ray=2, rnd_seed=7)
    images = {}
    with torch.no_grad():
        for denoise in (False, True):
            for residual in (False, True):
                img, reg = attrs.splat_mc_deferred(sp, [cam], denoise=denoise, residual=residual, **kw)
                want, alpha = _by_hand(sp, nrm, lv, env, cam, positions, mask, exposure, mode, denoise, residual)
                assert reg == 0 and img.shape == (64, 64, 4) and torch.equal(img, want), (denoise, residual)
                images[denoise, residual] = img
        assert not torch.equal(images[True, False], images[False, False]) and not torch.equal(images[True, True], images[False, True])
        assert not torch.equal(images[False, True], images[False, False])
        # masked-out pixels: the rasterizer's alpha and no light.  The reference clamps the two estimates to 1e-4 AFTER the shader has
        # written its zeros, so "no colour" is the colour of those floors alone: at most (1e-4 kd (1 - m) + 1e-4) alpha before the tone
        # map, and exactly what a black environment gives
        img, out = images[False, False], (mask.view(64, 64) == 0)
        assert out.any() and (~out).any() and img[..., 3].max() > 0.5 and torch.equal(img[..., 3], alpha[..., 0])
        dark, _ = _by_hand(sp, nrm, lv, gs.LatLngEnvMap(torch.zeros_like(light)).compute_pdf_(), cam, positions, mask, exposure, mode, False, False)
        assert torch.equal(img[out], dark[out]) and not torch.equal(img[~out], dark[~out])
        linear, _ = attrs.splat_mc_deferred(sp, [cam], tone_type="none", **kw)
        assert (linear[out][:, :3] <= 2e-4 * 1.3 * (1 + 1e-6) * alpha[out]).all() and linear[~out][:, :3].max() > 1e-2


def test_splat_mc_deferred_backward_reaches_every_input():
    sp, nrm, lv, light, cam, positions, mask = _splat_scene()
    leaves = {k: x.clone().requires_grad_(True) for k, x in lv.items()}
    light = light.clone().requires_grad_(True)
    normals = nrm.clone().requires_grad_(True)
    params = [getattr(sp, k).detach().clone().requires_grad_(True) for k in ("means", "scales", "quats", "opacities")]
    splats = SimpleNamespace(means=params[0], scales=params[1], quats=params[2], opacities=params[3])
    env = gs.LatLngEnvMap(light).compute_pdf_()
    attrs = gs.RenderableAttrs(kd=leaves["kd"], ks=leaves["ks"], normals=normals, occ=leaves["occ"])
    img, reg = attrs.splat_mc_deferred(splats, [cam], bvh=_bvh(), exposure=torch.tensor(1.0, device=DEV), positions=positions, mask=mask,
                                       envmap=env, min_roughness=0.1, max_metallic=0.9, num_samples_per_ray=2, denoise=True,
                                       residual=True)                                  # rnd_seed=None
    assert reg == 0
    (img[..., :3].mean() + img[..., 3].mean()).backward()
    for name, x in [("kd", leaves["kd"]), ("ks", leaves["ks"]), ("occ", leaves["occ"]), ("normals", normals), ("envmap", light)] + \
            list(zip(("means", "scales", "quats", "opacities"), params)):
        assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0, name
