"""Stage 3 on the GPU: `Stage3Model.from_export`, `surface`, `render_report`, `material_maps`, `stage3.train_step`, `Stage3Schedule` and
`evaluate_relighting`.  Sizes: icosphere(2, radius 0.6) (320 faces, 1 920 Gaussians), log2_hashmap_size 12, 48 x 48 images,
num_samples_per_ray 2, two cameras.  The export is written once by a `PriorModel` whose light and deform_params are seeded random."""
import math

import pytest
import torch

from tests import stage3_ref as R

pytestmark = pytest.mark.gpu

HW, LOG2, NS, SEED = 48, 12, 2, 7
_cache = {}


def _dev():
    return torch.device("cuda:0")


def _cams(n=2):
    import geosplatting_amd.synthetic as syn
    return syn.blender_cameras(n, HW, HW)


def _sphere():
    from geosplatting_amd.synthetic import icosphere
    v, f = icosphere(2, radius=0.6)
    return v.float().to(_dev()), f.long().to(_dev())


def _prior(smooth_type="jitter"):
    import geosplatting_amd as gs
    v, f = _sphere()
    p = gs.PriorModel(v, f, smooth_type=smooth_type, log2_hashmap_size=LOG2, seed=2)
    g = torch.Generator().manual_seed(11)
    light = torch.rand(256, 512, 3, generator=g) * 0.5 + 0.1
    light[40:70, 100:160] += 20.0
    with torch.no_grad():
        p.latlng.copy_(light.to(_dev()))
        p.deform_params.copy_(((torch.rand(v.shape, generator=g) * 2 - 1) * 0.01).to(_dev()))
        p.exposure_params.fill_(0.1)
    return p


@pytest.fixture(scope="module")
def export(tmp_path_factory):
    """(path of the stage-2 export, the dictionary in it, the positions its ks was evaluated at)"""
    import geosplatting_amd as gs
    p = _prior()
    path = tmp_path_factory.mktemp("stage3") / "s2.pth"
    p.export_model(path)
    with torch.no_grad():
        v = p.vertices + p.deform_params
        at = gs.mesh_to_splats(v, p.faces, gs.vertex_normals(v, p.faces))[0].means
    return path, torch.load(path, map_location="cpu"), at


def _load(export, **kw):
    import geosplatting_amd as gs
    m = gs.Stage3Model.from_export(export[0], device=_dev(), **kw)
    m.num_samples_per_ray = NS
    return m


def _hand_image(m, cam, *, kd, occ, exposure, envmap, rnd_seed=SEED):
    """`splat_mc_deferred` called by hand with render_report's arguments"""
    import geosplatting_amd as gs
    splats = m.get_gsplat()
    attrs = gs.RenderableAttrs(kd=kd, ks=m.ks_at(m.means), occ=occ, normals=splats.colors)
    positions, mask = m.surface(cam)
    img, _ = attrs.splat_mc_deferred(splats, [cam], bvh=m.bvh(), exposure=exposure, positions=positions, mask=mask, envmap=envmap,
                                     min_roughness=m.min_roughness, max_metallic=m.max_metallic, num_samples_per_ray=NS,
                                     shadow_scale=m.shadow_scale, residual=True, tone_type="naive", rnd_seed=rnd_seed)
    return img


def test_loading(export, tmp_path):
    """The export's ks was evaluated at the Gaussians' centres ON the faces; the file's `means` are those centres pushed under the
    surface by the z field (and `mc_positions` their float32 sum with the offsets again).  Stage 3 evaluates ks at its own `means`, as
    the reference does, so the bit-for-bit statement "same encoder, same positions" is checked where the positions ARE the same: the
    loaded encoder at the centres the export used.  The distance of the model's own ks from the exported one is printed."""
    import geosplatting_amd as gs
    path, a, at = export
    m = _load(export, seed=3)
    N = 6 * 320
    shapes = {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N, 1), "normals": (N, 3), "kd_params": (N, 3),
              "occ_params": (N, 6), "exposure_params": (1,), "latlng_hue": (256, 512, 3), "latlng_value": (256, 512, 3),
              "ks_enc.0": (16 * 2 ** LOG2, 2), "ks_enc.1": (32, 32), "ks_enc.2": (2, 32)}
    named = m.named_parameters()
    assert {k: tuple(p.shape) for k, p in named.items()} == shapes
    assert all(p.requires_grad and p.is_leaf and p.device.type == "cuda" for p in named.values())
    for t in (m.mesh_v, m.mesh_i, m.mesh_pos, m.initial_guess):
        assert not t.requires_grad and t.device.type == "cuda"
    assert tuple(m.mesh_v.shape) == (162, 3) and tuple(m.mesh_i.shape) == (320, 3) and tuple(m.mesh_pos.shape) == (N, 3)
    assert torch.equal(m.kd_params.detach().cpu(), a["kd"]) and torch.equal(m.occ_params.detach().cpu(), a["occ"])
    assert torch.equal(m.exposure_params.detach().cpu(), a["exposure"]) and m.scale == 1.0 and m.training
    with torch.no_grad():
        assert torch.equal(m.ks_at(at).cpu(), a["ks"])
        own = (m.ks_at(m.means).cpu() - a["ks"]).abs().max()
        print(f"ks at the model's means against the exported ks: largest difference {float(own):.3g}")
    worst = R.check_light_round_trip(a["latlng"], m.get_envmap().data.detach())
    print(f"light round trip on the device: largest error {worst:.3f} of the budget")
    # an export without occ
    bad = tmp_path / "tv.pth"
    _prior("tv").export_model(bad)
    with pytest.raises(ValueError, match="occ"):
        gs.Stage3Model.from_export(bad, device=_dev())
    # one hierarchy
    assert m._hierarchy is None
    with torch.no_grad():
        m.render_report(_cams(1), rnd_seed=SEED)
        first = m.bvh()
        m.render_report(_cams(1), rnd_seed=SEED)
    assert m.bvh() is first and isinstance(first, gs.MeshBVH)
    # checkpoints
    with torch.no_grad():
        m.kd_params.mul_(0.5); m.latlng_value.add_(0.1); m.ks_enc.weights[0].add_(0.25); m.means.add_(0.001)
    m.save_checkpoint(tmp_path / "ckpt", 12)
    m2 = _load(export, seed=9)
    assert not torch.equal(m2.kd_params, m.kd_params)
    assert m2.load_checkpoint(tmp_path / "ckpt") == 12
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(m.parameters(), m2.parameters()))


def test_surface(export):
    import geosplatting_amd as gs
    from geosplatting_amd.meshrender import to_camera_space
    m = _load(export)
    cam = _cams(2)[1]
    positions, mask = m.surface(cam)
    rast = gs.rasterize_mesh(to_camera_space(m.mesh_v, cam), m.mesh_i, cam)
    assert torch.equal(positions, gs.interpolate(m.mesh_v, rast, m.mesh_i)) and torch.equal(mask, (rast[..., -1:] > 0).float())
    assert tuple(positions.shape) == (HW, HW, 3) and tuple(mask.shape) == (HW, HW, 1)
    assert float(mask[HW // 2, HW // 2]) == 1.0 and float(mask[0, 0]) == 0.0 and float(mask[-1, -1]) == 0.0
    assert not positions.requires_grad and not mask.requires_grad
    centre = positions[HW // 2, HW // 2]
    assert abs(float(centre.norm()) - 0.6) < 0.03                                    # a point of the (slightly deformed) sphere


def test_render_report_without_ground_truth(export):
    m = _load(export, seed=1)
    m.ks_weight = 0.05
    cams = _cams(2)
    with torch.no_grad():
        state = m.generator.get_state()
        images, reg, n = m.render_report(cams, rnd_seed=SEED)
        assert n == 1920 and len(images) == 2 and all(tuple(i.shape) == (HW, HW, 4) for i in images)
        assert float(images[0][..., 3].max()) > 0.9 and float(images[0][..., :3].max()) > 0.0
        for cam, img in zip(cams, images):
            want = _hand_image(m, cam, kd=m.kd_params, occ=m.occ_params, exposure=m.exposure_params.exp()[0], envmap=m.get_envmap())
            assert torch.equal(img, want)
        assert not torch.equal(images[0], images[1])
        # the regulariser is the ks term alone
        m.generator.set_state(state)
        jitter = torch.randn(m.means.shape, device=_dev(), generator=m.generator) * 0.01
        ks_reg = (m.ks_at(m.means) - m.ks_at(m.means + jitter)).abs().mean() * 0.05
        assert torch.equal(reg, ks_reg) and float(reg) > 0
        # evaluation mode: nothing of the image depends on the generator
        m.training = False
        again, _, _ = m.render_report(cams, rnd_seed=SEED)
        third, _, _ = m.render_report(cams, rnd_seed=SEED)
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(images, again, third))
        m.generator.set_state(state)
        _, reg2, _ = m.render_report(cams, rnd_seed=SEED)
        assert torch.equal(reg2, reg)


def test_regulariser_with_ground_truth(export, monkeypatch):
    from geosplatting_amd import stage3
    from geosplatting_amd.shading import _rasterize_activated
    from geosplatting_amd.stage1 import _edge_aware
    m = _load(export, seed=2)
    cams = _cams(2)
    g = torch.Generator().manual_seed(4)
    gts = [torch.rand(HW, HW, 4, generator=g).to(_dev()) for _ in cams]
    m.kd_weight, m.ks_weight, m.normal_weight = 0.2, 0.05, 0.3
    calls = []
    real = stage3._render_channels
    monkeypatch.setattr(stage3, "_render_channels", lambda *a, **k: (calls.append(a[4].shape[-1]), real(*a, **k))[1])
    with torch.no_grad():
        state = m.generator.get_state()
        _, reg, _ = m.render_report(cams, gts, rnd_seed=SEED)
        assert calls == [6, 6]                                         # one pass per view for both terms
        m.generator.set_state(state)
        jitter = torch.randn(m.means.shape, device=_dev(), generator=m.generator) * 0.01
        ks_reg = (m.ks_at(m.means) - m.ks_at(m.means + jitter)).abs().mean() * 0.05
        splats = m.get_gsplat()
        colors = torch.cat((m.kd_params, splats.colors * 0.5 + 0.5), dim=-1)
        views = torch.zeros((), device=_dev())
        for cam, gt in zip(cams, gts):
            bg = torch.rand(3, device=_dev(), generator=m.generator)                   # 'random' while training, a draw per view
            render, alpha, _ = _rasterize_activated(m.means, m.scales, m.quats, m.opacities, colors, cam, "RGB")   # unbent opacities
            both = (render + (1 - alpha) * bg.repeat(2)).squeeze(0)
            gt_rgb = gt[..., :3] * gt[..., 3:] + (1 - gt[..., 3:])
            views = views + (_edge_aware(both[..., :3], gt_rgb) * 0.2 + _edge_aware(both[..., 3:], gt_rgb) * 0.3)
        want = ks_reg + views / 2
        print(f"reg {float(reg):.8g} by hand {float(want):.8g} (ks term {float(ks_reg):.8g})")
        assert torch.equal(reg, want) and float(reg) > float(ks_reg) > 0
        # both view weights 0: the pass is not made, the ks term remains
        del calls[:]
        m.kd_weight, m.normal_weight = 0.0, 0.0
        m.generator.set_state(state)
        _, reg0, _ = m.render_report(cams, gts, rnd_seed=SEED)
        assert calls == [] and torch.equal(reg0, ks_reg)


def test_relight_mode(export):
    import geosplatting_amd as gs
    from geosplatting_amd.synthetic import make_cubemap
    m = _load(export)
    m.training = False
    cam = _cams(2)[0]
    env = gs.LatLngEnvMap(R.sample_light(6).to(_dev()))
    s = torch.tensor([0.5, 1.5, 0.8])
    with torch.no_grad():
        learned = m.render_report([cam], rnd_seed=SEED)[0][0]
        m.set_relight_envmap(env, s)
        assert not m.learned_light and m.get_envmap() is m.get_envmap() and m.get_envmap().pdf is not None       # built once
        relit = m.render_report([cam], rnd_seed=SEED)[0][0]
        kd = m.kd_params
        occ = m.occ_params.mean(-1, keepdim=True) * torch.cat((torch.ones_like(kd), kd), dim=-1)               # the unscaled kd
        want = _hand_image(m, cam, kd=kd * s.to(_dev()), occ=occ, exposure=torch.ones((), device=_dev()),
                           envmap=gs.LatLngEnvMap(env.data.clone()).compute_pdf_())
        assert torch.equal(relit, want) and not torch.equal(relit, learned)
        cube = gs.EnvCubeMap(make_cubemap(32, seed=2).to(_dev()))
        m.set_relight_envmap(cube, s)
        assert tuple(m.get_envmap().data.shape) == (256, 512, 3)
        from_cube = m.render_report([cam], rnd_seed=SEED)[0][0]
        m.set_relight_envmap(cube.as_latlng(512, 256), s)
        assert torch.equal(from_cube, m.render_report([cam], rnd_seed=SEED)[0][0])
        m.clear_relight_envmap()
        assert m.learned_light and torch.equal(m.render_report([cam], rnd_seed=SEED)[0][0], learned)
    with pytest.raises(ValueError):
        m.set_relight_envmap(env, torch.ones(4))
    with pytest.raises(ValueError, match="transform"):
        m.set_relight_envmap(gs.LatLngEnvMap(env.data, transform=torch.eye(3, device=_dev())), s)


def test_material_maps(export):
    """One D = 9 pass against three D = 3 passes.  The compositor's contract would allow them to differ by 1e-4 of the float64 sum of
    absolute terms each; measured on an MI355X they are bit-equal (each channel is accumulated on its own, in the same order), so
    that is what is asserted.  The sRGB curve against its float64 formula: the power costs two ulp of p = x^(1/2.4), the rounded
    exponent 2.4 u (|ln x| <= 5.77 above the threshold), the product with 1.055 one u, the subtraction one u of the result r and the
    two constants 0.11 u: (7.81 p + r + 0.11) u absolute; 2 u r on the linear branch."""
    import geosplatting_amd as gs
    m = _load(export)
    m.training = False
    cam = _cams(2)[1]
    maps = m.material_maps(cam)
    assert set(maps) == {"kd", "kd_srgb", "ks", "direct", "alpha"}
    assert all(tuple(maps[k].shape) == (HW, HW, 3) for k in ("kd", "kd_srgb", "ks", "direct")) and tuple(maps["alpha"].shape) == (HW, HW, 1)
    assert not any(t.requires_grad for t in maps.values())
    with torch.no_grad():
        bg = m.get_background_color()
        assert torch.equal(bg, torch.tensor([0.1490, 0.1647, 0.2157], device=_dev()))
        lookat = -cam.c2w.to(_dev())[:, 2]
        bend = (m.normals * lookat).sum(-1, keepdim=True) > 0
        assert 0 < int(bend.sum()) < bend.numel()
        opac = torch.where(bend, torch.full_like(m.opacities, -2.0), m.opacities)
        ks = m.ks_at(m.means)
        ks3 = torch.cat((torch.zeros_like(ks[:, :1]), ks[:, :1] * (1 - m.min_roughness) + m.min_roughness, ks[:, 1:] * m.max_metallic), -1)
        rr = lambda colors: gs.render_rgb(m.means, m.scales, m.quats, opac, colors, cam, bg)
        for name, colors in (("kd", m.kd_params), ("ks", ks3), ("direct", (m.occ_params[:, :3] - 3).sigmoid())):
            assert torch.equal(maps[name], rr(colors)), name
        assert float(maps["ks"][..., 0].max()) <= float(bg[0]) and float(maps["alpha"].max()) > 0.9
        x = maps["kd"].double()
        p = x.clamp_min(0.0031308) ** (1 / 2.4)
        r = torch.where(x <= 0.0031308, x * 12.92, p * 1.055 - 0.055)
        budget = torch.where(x <= 0.0031308, 2 * r, 7.81 * p + r + 0.11) * R.U
        err = (maps["kd_srgb"].double() - r).abs()
        print(f"sRGB curve: largest error {float((err / budget).max()):.3f} of the budget")
        assert bool((err <= budget).all())
        # under a relight map the albedo is the scaled one
        m.set_relight_envmap(gs.LatLngEnvMap(R.sample_light(6).to(_dev())), torch.tensor([0.5, 0.5, 0.5]))
        half = m.material_maps(cam)["kd"]                                            # = 0.5 sum w kd + (1 - alpha) bg
        want = 0.5 * maps["kd"] + 0.5 * (1 - maps["alpha"]) * bg
        assert bool(((half - want).abs() <= 2e-4 * (1 + 2 * bg)).all())                # both within 1e-4 of terms that are <= 1 + 2 bg


def test_train_step_gradients(export):
    from geosplatting_amd import stage3
    m = _load(export, seed=5)
    cams = _cams(2)
    sched = stage3.Stage3Schedule()
    opts = sched.setup(m)
    sched.before_update(m, 0, opts)
    with torch.no_grad():
        gts = [img.clamp(0, 1) for img in m.render_report(cams, rnd_seed=5)[0]]
        m.latlng_value.sub_(0.5)
    g = torch.Generator().manual_seed(8)
    bgs = [torch.rand(HW, HW, 3, generator=g).to(_dev()) for _ in cams]
    out = stage3.train_step(m, cams, gts, gt_is_srgb=False, train_bg=bgs, rnd_seed=6)
    assert math.isfinite(float(out["loss"])) and float(out["loss"]) > 0 and int(out["#gaussians"]) == 1920
    assert float(out["regularization"]) > 0 and float(out["exposure"]) == pytest.approx(math.exp(0.1), rel=1e-6)
    named = m.named_parameters()
    for name, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
    nonzero = {name for name, p in named.items() if float(p.grad.abs().max()) > 0}
    assert {"latlng_hue", "latlng_value", "exposure_params", "kd_params", "occ_params", "normals", "means"} <= nonzero, nonzero
    assert any(n.startswith("ks_enc.") for n in nonzero), nonzero
    assert m.mesh_v.grad is None and not m.mesh_v.requires_grad
    before = (m.latlng_hue.grad.clone(), m.latlng_value.grad.clone(), m.kd_params.grad.clone())
    sched.scale_light_gradient(m)
    assert torch.equal(m.latlng_hue.grad, before[0] * 64) and torch.equal(m.latlng_value.grad, before[1] * 64)
    assert torch.equal(m.kd_params.grad, before[2])
    # the trainer's default, an sRGB ground truth: the same pictures through the curve give the same step.  The round trip costs
    # rounding only (the curve's slope is at most 12.92, float32 pictures: below 1e-5 per pixel), while the curve itself moves a
    # mid-grey by 0.2: 1 % of the loss tells a converted ground truth from an unconverted one
    srgb = [torch.cat((stage3.linear_to_srgb(g[..., :3]), g[..., 3:]), -1) for g in gts]
    out2 = stage3.train_step(m, cams, srgb, train_bg=bgs, rnd_seed=6)
    print(f"loss with a linear ground truth {float(out['loss']):.8g}, with the same as sRGB {float(out2['loss']):.8g}")
    assert float(out2["loss"]) == pytest.approx(float(out["loss"]), rel=1e-2)


def test_fits_the_light_it_was_rendered_under(export):
    """Targets: the model's own renders under the export's light (a bright patch of about 20 on 0.1 .. 0.6), fixed shader seed,
    evaluation mode.  The model under test is the same with its light reset to the constant 0.5; only the light_hue, light_value and
    exposure groups take 30 steps of `Stage3Schedule`, with fixed backgrounds.  Measured on an MI355X: first five 0.082682, last five
    0.070543, ratio 0.853 (the rates are 1e-3: thirty Adam steps move the log-light by 0.03 at most).  The bound is halfway between
    that and 1, their geometric mean 0.924."""
    from geosplatting_amd import stage3
    cams = _cams(2)
    target = _load(export)
    target.training = False
    with torch.no_grad():
        gts = [img.clamp(0, 1) for img in target.render_report(cams, rnd_seed=21)[0]]
    assert float(gts[0][..., 3].max()) > 0.9
    m = _load(export)
    with torch.no_grad():
        hue, value = stage3.light_to_params(torch.full_like(m.latlng_hue, 0.5))
        m.latlng_hue.copy_(hue); m.latlng_value.copy_(value)
    sched = stage3.Stage3Schedule()
    opts = {k: o for k, o in sched.setup(m).items() if k in ("light_hue", "light_value", "exposure")}
    g = torch.Generator().manual_seed(8)
    bgs = [torch.rand(HW, HW, 3, generator=g).to(_dev()) for _ in cams]
    losses = []
    for step in range(30):
        sched.before_update(m, step, opts)
        out = stage3.train_step(m, cams, gts, gt_is_srgb=False, train_bg=bgs, rnd_seed=21)
        sched.scale_light_gradient(m)
        for opt in opts.values():
            opt.step()
        sched.after_update(m, step)
        losses.append(float(out["loss"]))
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f"first five {first:.6f}, last five {last:.6f}, ratio {last / first:.4f}, exposure {float(out['exposure']):.4f}")
    assert all(math.isfinite(x) for x in losses) and last < 0.924 * first


def test_evaluate_relighting(export):
    import geosplatting_amd as gs
    from geosplatting_amd import stage3
    dev = _dev()
    cams = _cams(2)
    m = _load(export, seed=1)
    truth = _load(export, seed=2)
    truth.training = False
    envs = [gs.LatLngEnvMap(R.sample_light(6).to(dev)), gs.LatLngEnvMap((R.sample_light(9).flip(1) * 2.0).to(dev))]
    srgb_rgba = lambda img: torch.cat((stage3.linear_to_srgb(img[..., :3]).clamp(0, 1), img[..., 3:]), -1)
    with torch.no_grad():
        assert float(truth.kd_params.min()) > 0.4
        truth.kd_params.mul_(0.5).add_(torch.rand(truth.kd_params.shape, generator=torch.Generator().manual_seed(3)).to(dev) * 0.05)
        gt_views = [srgb_rgba(truth.render_report([c], rnd_seed=5)[0][0]) for c in cams]
        truth.background_color = "black"
        gt_albedos = []
        for c in cams:
            maps = truth.material_maps(c)
            gt_albedos.append(torch.cat((maps["kd_srgb"], maps["alpha"]), -1))
        relights = []
        for env in envs:
            truth.set_relight_envmap(env, torch.ones(3))
            relights.append((env, [srgb_rgba(truth.render_report([c], rnd_seed=5)[0][0]) for c in cams]))
    m.background_color, m.training = "random", True
    out = gs.evaluate_relighting(m, cams, gt_views, relights, gt_albedos=gt_albedos, rnd_seed=5)
    assert (m.background_color, m.training, m.learned_light, m.albedo_scaling) == ("random", True, True, None)
    # the same by hand
    psnr = lambda a, b: -10.0 * torch.log10((a - b).square().mean())
    white = torch.ones(3, device=dev)
    blend = lambda rgba, bg: rgba[..., 3:] * rgba[..., :3] + bg * (1 - rgba[..., 3:])

    def by_hand(gts):
        vals = []
        for c, gt in zip(cams, gts):
            img = m.render_report([c], rnd_seed=5)[0][0]
            vals.append(psnr(blend(srgb_rgba_unclamped(img), white).clamp(0, 1), blend(gt, white).clamp(0, 1)))
        return float(torch.stack(vals).mean())
    srgb_rgba_unclamped = lambda img: torch.cat((stage3.linear_to_srgb(img[..., :3]), img[..., 3:]), -1)
    with torch.no_grad():
        m.training, m.background_color = False, "black"
        linear_gt = [torch.cat((stage3.srgb_to_linear(g[..., :3]), g[..., 3:]), -1) for g in gt_albedos]
        scale = gs.albedo_scaling([m.material_maps(c)["kd"] for c in cams], linear_gt, "least-square")
        assert torch.equal(out["albedo_scaling"], scale.cpu())
        assert out["nvs_psnr"] == by_hand(gt_views)
        hand = []
        for env, gts in relights:
            m.set_relight_envmap(env, scale)
            hand.append(by_hand(gts))
        assert out["relight_psnr"] == hand and out["relight_psnr_mean"] == sum(hand) / 2
        m.set_relight_envmap(envs[0], scale)
        albedo = [psnr(m.material_maps(c)["kd_srgb"].clamp(0, 1), blend(g, torch.zeros(3, device=dev))) for c, g in zip(cams, gt_albedos)]
        assert out["albedo_psnr"] == float(torch.stack(albedo).mean())
        m.clear_relight_envmap()
    print({k: v for k, v in out.items() if k != "albedo_scaling"}, out["albedo_scaling"].tolist())
    every = [out["nvs_psnr"], out["albedo_psnr"]] + out["relight_psnr"]
    assert all(math.isfinite(x) for x in every) and out["relight_psnr"][0] != out["relight_psnr"][1]
    assert all(0.0 < x <= 1.0 for x in [out["nvs_ssim"], out["albedo_ssim"]] + out["relight_ssim"])
    assert "roughness_mse" not in out
    # the truth's albedo is 0.5 kd + 0.05 n with n in [0, 1): its map is 0.5 a + 0.05 n_map with 0 <= n_map <= alpha, and the
    # model's map a exceeds 0.4 alpha (kd > 0.4), so sum(a gt) / sum(a^2) lies between 0.5 and 0.5 + 0.05 / 0.4
    assert bool(((out["albedo_scaling"] > 0.5) & (out["albedo_scaling"] <= 0.625)).all()), out["albedo_scaling"]
    # restored after an exception too
    m.background_color, m.training = "white", True
    bad = gs.LatLngEnvMap(envs[0].data, transform=torch.eye(3, device=dev))
    with pytest.raises(ValueError, match="transform"):
        gs.evaluate_relighting(m, cams, gt_views, [(bad, relights[0][1])], rnd_seed=5)
    assert (m.background_color, m.training, m.learned_light, m.albedo_scaling) == ("white", True, True, None)
    # its own pictures as the ground truth: no error beyond rounding
    with torch.no_grad():
        m.training = False
        own = [srgb_rgba(m.render_report([c], rnd_seed=5)[0][0]) for c in cams]
    assert gs.evaluate_relighting(m, cams, own, [], rnd_seed=5)["nvs_psnr"] > 60.0
