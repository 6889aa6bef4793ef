"""Stage 2 on the GPU: the denoised per-Gaussian Monte-Carlo shader, the occlusion encoder, `Stage2Model.from_export`, `PriorModel`,
`Stage2Schedule` and `stage2.train_step`.  Sizes: FlexiCubes resolution 16, log2_hashmap_size 12, 48 x 48 images, num_samples_per_ray 2."""
import math

import pytest
import torch

from tests import meshreg_ref as R

pytestmark = pytest.mark.gpu

HW, LOG2, NS = 48, 12, 2
EXPORT_KEYS = {"geom_scale", "min_roughness", "max_metallic", "exposure", "latlng", "means", "scales", "quats", "opacities", "normals",
               "kd", "ks", "occ", "ks_enc", "occ_enc", "mc_positions", "mc_vertices", "mc_indices", "initial_guess"}
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


def _splat_scene():
    """a sphere's Gaussians with random attributes, its hierarchy, a light with a bright patch, one camera"""
    import geosplatting_amd as gs
    if "scene" not in _cache:
        v, f = _sphere()
        sp, nrm = gs.mesh_to_splats(v, f, gs.vertex_normals(v, f))
        g = torch.Generator().manual_seed(5)
        N = sp.means.shape[0]
        leaves = {k: x.to(_dev()) for k, x in dict(kd=torch.rand(N, 3, generator=g), ks=torch.rand(N, 2, generator=g),
                                                   occ=torch.randn(N, 6, generator=g) + 3.0).items()}
        light = torch.rand(16, 32, 3, generator=g) * 0.5 + 0.1
        light[3:6, 8:12] += 20.0
        _cache["scene"] = (sp, nrm, leaves, light.to(_dev()), _cams(1)[0], gs.MeshBVH(v, f))
    return _cache["scene"]


@pytest.mark.parametrize("residual", [False, True])
def test_splat_mc_denoised_equals_its_pipeline(residual):
    import geosplatting_amd as gs
    sp, nrm, lv, light, cam, bvh = _splat_scene()
    env = gs.LatLngEnvMap(light).compute_pdf_()
    exposure = torch.tensor(1.2, device=_dev())
    attrs = gs.RenderableAttrs(kd=lv["kd"], ks=lv["ks"], normals=nrm, occ=lv["occ"])
    kw = dict(bvh=bvh, exposure=exposure, positions=sp.means, envmap=env, min_roughness=0.1, max_metallic=0.9, num_samples_per_ray=NS,
              rnd_seed=11, shadow_scale=1.0, residual=residual)
    with torch.no_grad():
        img, reg = attrs.splat_mc_denoised(sp, [cam], **kw)
        assert reg == 0 and img.shape == (HW, HW, 4) and img[..., 3].max() > 0.5
        c2w = cam.c2w.to(_dev())
        lookat, cam_pos = -c2w[:, 2], c2w[:, 3]
        n = torch.where((nrm * lookat).sum(-1, keepdim=True) > 1e-3, -nrm, nrm)
        rough, metal = lv["ks"][:, :1] * 0.9 + 0.1, lv["ks"][:, 1:] * 0.9
        ks3 = torch.cat((torch.zeros_like(rough), rough, metal), -1)
        pdf, rows, cols = env.tables()
        d, s, r = gs.env_shade(bvh, torch.ones_like(n[:, :1]), sp.means + nrm * 1e-5, sp.means, n, cam_pos.contiguous(), lv["kd"], ks3,
                               light, pdf, rows, cols, BSDF="pbr", n_samples_x=NS, rnd_seed=11, shadow_scale=1.0)
        d, s, r = d.clamp_min(1e-4), s.clamp_min(1e-4), r.clamp(0, 1)
        depth = ((sp.means - cam_pos) * lookat).sum(-1, keepdim=True)
        planes = torch.cat((d, s, r) if residual else (d, s), -1)
        C = planes.shape[-1]
        assert C == (8 if residual else 6)
        filt = gs.bilateral_denoiser(planes.view(1, 1, -1, C), n.view(1, 1, -1, 3), depth.view(1, 1, -1, 1), 2.0).view(-1, C)
        d, s = filt[:, 0:3], filt[:, 3:6]
        if residual:
            rl = (lv["occ"] - 3).sigmoid()
            d, s = d + filt[:, 6:7] * rl[:, :3], s + filt[:, 7:8] * rl[:, 3:]
        col = d * (lv["kd"] * (1 - metal)) + s
        want = gs.tone_map(gs.render_rgba(sp.means, sp.scales, sp.quats, sp.opacities, col, cam), exposure, "naive")
        assert torch.equal(img, want)
        plain, _ = attrs.splat_mc(sp, [cam], **kw)
        assert not torch.equal(plain, img)                              # the filter changes the estimates
    with pytest.raises(NotImplementedError, match="bilateral denoiser"):
        attrs.splat_mc(sp, [cam], denoise=True, **kw)


def test_splat_mc_denoised_backward():
    import geosplatting_amd as gs
    sp, nrm, lv, light, cam, bvh = _splat_scene()
    leaves = {k: x.clone().requires_grad_(True) for k, x in lv.items()}
    light = light.clone().requires_grad_(True)
    attrs = gs.RenderableAttrs(kd=leaves["kd"], ks=leaves["ks"], normals=nrm, occ=leaves["occ"])
    img, _ = attrs.splat_mc_denoised(sp, [cam], bvh=bvh, exposure=torch.tensor(1.0, device=_dev()), positions=sp.means,
                                     envmap=gs.LatLngEnvMap(light).compute_pdf_(), min_roughness=0.1, max_metallic=0.9,
                                     num_samples_per_ray=NS, rnd_seed=3, residual=True)
    img[..., :3].mean().backward()
    for name, x in list(leaves.items()) + [("light", light)]:
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0, name


def test_field_with_the_occlusion_encoder():
    from geosplatting_amd.field import GaussianField
    v, f = _sphere()
    plain = GaussianField(device=_dev(), log2_hashmap_size=LOG2, seed=4)
    with_occ = GaussianField(device=_dev(), log2_hashmap_size=LOG2, seed=4, occ=True)
    assert plain.occ_enc is None and len(plain.parameters()) == 4 + 3 + 3
    # the three encoders keep the bits a seed gave them before the keyword existed: HashEncoding(seed), (seed + 1), (seed + 2)
    from geosplatting_amd.field import HashEncoding
    common = dict(max_res=4096, log2_hashmap_size=LOG2, grad_scaling=16.0, device=_dev())
    today = (HashEncoding([-1, 32, 32, 3], activation="sigmoid", seed=4, **common).parameters()
             + HashEncoding([-1, 32, 2], activation="none", seed=5, **common).parameters()
             + HashEncoding([-1, 32, 1], activation="none", seed=6, **common).parameters())
    for field in (plain, with_occ):
        assert all(torch.equal(a, b) for a, b in zip(field.parameters()[:10], today))
    assert len(today) == 10 and len(with_occ.parameters()) == 10 + 4 and with_occ.occ_enc.weights[-1].shape == (6, 32)
    kw = dict(scale=1.0, initial_guess=torch.zeros(2, device=_dev()))
    _, attrs, _ = with_occ.get_gaussians_from_face(v, f, **kw)
    assert attrs.occ.shape == (6 * f.shape[0], 6)
    _, attrs0, _ = plain.get_gaussians_from_face(v, f, **kw)
    assert attrs0.occ is None and torch.equal(attrs0.kd, attrs.kd) and torch.equal(attrs0.ks, attrs.ks)


def test_stage2_from_a_stage1_export(tmp_path):
    import geosplatting_amd as gs
    from geosplatting_amd import stage2
    from geosplatting_amd.stage1 import Stage1Model
    dev = _dev()
    grid = gs.FlexiCubes.from_resolution(16, device=dev, random_sdf=False, scale=1.05)
    m1 = Stage1Model(16, light_resolution=32, device=dev, seed=2, log2_hashmap_size=LOG2,
                     sdf_init=grid.vertices.norm(dim=-1, keepdim=True) - 0.55)
    with torch.no_grad():
        m1.cubemap.copy_(torch.rand(m1.cubemap.shape, generator=torch.Generator().manual_seed(1)).to(dev) + 0.2)
        m1.exposure_params.fill_(0.1)
    path = tmp_path / "stage1.pth"
    m1.export_model(path)
    m = gs.Stage2Model.from_export(path, device=dev, seed=3)
    assert m.residual and m.resolution == 16 and m.scale == 1.05
    assert m.latlng.shape == (256, 512, 3) and m.latlng.requires_grad
    assert torch.equal(m.latlng.detach(), gs.EnvCubeMap(m1.cubemap.detach()).as_latlng(512, 256).data)
    for a, b in ((m.sdf_params, m1.sdf_params), (m.deform_params, m1.deform_params), (m.weight_params, m1.weight_params),
                 (m.exposure_params, m1.exposure_params)):
        assert torch.equal(a.detach(), b.detach())
    assert all(torch.equal(a, b) for a, b in zip(m.field.ks_enc.parameters(), m1.field.ks_enc.parameters()))
    names = set(m.named_parameters())
    assert {"sdf_params", "deform_params", "weight_params", "latlng", "exposure_params", "field.occ_enc.0", "field.kd_enc.0"} <= names
    sched = gs.Stage2Schedule()
    opts = sched.setup(m)
    assert m.occ_weight == 1e-3 and set(opts) == {"deforms", "weights", "sdfs", "exposure", "light", "kd", "occ", "ks", "z"}
    assert opts["ks"].param_groups[0]["lr"] == pytest.approx(2e-3) and opts["exposure"].param_groups[0]["lr"] == pytest.approx(5e-3)
    sched.before_update(m, 0, opts)
    assert m.sdf_weight == pytest.approx(0.2) and m.kd_regualr_perturb_std == 0.01 and opts["sdfs"].param_groups[0]["lr"] == 0.0
    assert sched.lr_factor(850, 50) == pytest.approx(0.5) and sched.lr_factor(800, None) == pytest.approx(0.5)
    m.num_samples_per_ray = NS
    cams = _cams(2)
    with torch.no_grad():
        gts = [img.clamp(0, 1) for img in m.render_report(cams, rnd_seed=5)[0]]
        m.latlng.mul_(0.5)
    out = stage2.train_step(m, cams, gts, gt_is_srgb=False, rnd_seed=6)
    assert math.isfinite(float(out["loss"])) and int(out["#gaussians"]) == m.last_num_gaussians > 0
    for name, p in m.named_parameters().items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    nonzero = {name for name, p in m.named_parameters().items() if float(p.grad.abs().max()) > 0}
    assert {"latlng", "sdf_params", "exposure_params"} <= nonzero, nonzero
    assert any(n.startswith("field.kd_enc.") for n in nonzero) and any(n.startswith("field.occ_enc.") for n in nonzero), nonzero
    before = m.latlng.grad.clone()
    sched.scale_light_gradient(m)
    assert torch.equal(m.latlng.grad, before * 64)
    with torch.no_grad():
        m.latlng[0, 0] = 0.0
    sched.after_update(m, 0)
    assert float(m.latlng.min()) == float(torch.tensor(1e-2))              # the float32 floor
    out_path = tmp_path / "stage2.pth"
    m.export_model(out_path)
    a = torch.load(out_path, map_location="cpu")
    N = m.last_num_gaussians
    assert set(a) == EXPORT_KEYS | {"resolution"} and a["mc_indices"].dtype == torch.int32 and a["occ"].shape == (N, 6)
    assert a["mc_positions"].shape == (N, 3) and a["latlng"].shape == (256, 512, 3) and a["mc_indices"].shape[0] * 6 == N
    # checkpoints round-trip
    m.save_checkpoint(tmp_path / "ckpt", 7)
    m2 = gs.Stage2Model.from_export(path, device=dev, seed=9)
    assert m2.load_checkpoint(tmp_path / "ckpt") == 7
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(m.parameters(), m2.parameters()))


@pytest.mark.parametrize("smooth_type", ["jitter", "tv"])
def test_prior_model_regulariser_and_export(smooth_type, tmp_path):
    import geosplatting_amd as gs
    v32, f, topo = R.case("icosphere2")
    dev = _dev()
    m = gs.PriorModel(v32.to(dev), f.to(dev), smooth_type=smooth_type, log2_hashmap_size=LOG2, seed=1)
    assert not m.residual and m.latlng.shape == (256, 512, 3) and bool((m.latlng == 0.5).all())
    assert not bool(m.deform_params.any()) and not bool(m.exposure_params.any())
    names = set(m.named_parameters())
    F = f.shape[0]
    if smooth_type == "jitter":
        assert "field.occ_enc.0" in names and "kdks_params" not in names
    else:
        assert m.kdks_params.shape == (6 * F, 5) and m.zs_params.shape == (6 * F, 1)
        assert {"kdks_params", "zs_params"} <= names and not any(n.startswith("field.") for n in names)
        assert set(gs.Stage2Schedule.prior().setup(m)) == {"deforms", "exposure", "light", "kdks", "zs"}
    g = torch.Generator().manual_seed(3)
    deform = (torch.rand(v32.shape, generator=g) * 2 - 1) * 0.02
    with torch.no_grad():
        m.deform_params.copy_(deform.to(dev))
    (_, faces), reg = m.get_geometry()
    moved = v32 + deform                                              # the float32 sum the model forms
    ref = R.evaluate(moved, topo)
    off = deform.double().square().sum(-1)
    want = 1e-3 * ref["lap"] + 3e-4 * ref["nc"] + 0.1 * ref["edge"] + 0.1 * off.mean()
    budget = 1e-3 * ref["lap_budget"] + 3e-4 * ref["nc_budget"] + 0.1 * ref["edge_budget"] + 0.1 * R.KAPPA * off.mean()
    budget = budget + R.KAPPA * (1e-3 * ref["lap"] + 3e-4 * ref["nc"].abs() + 0.1 * ref["edge"] + 0.1 * off.mean())   # the four-term sum
    print(f"reg {float(reg):.8g} want {float(want):.8g} error {abs(float(reg) - float(want)):.3g} budget {float(budget):.3g}")
    assert abs(float(reg) - float(want)) <= float(budget)
    reg.backward()
    assert bool(torch.isfinite(m.deform_params.grad).all()) and float(m.deform_params.grad.abs().max()) > 0
    path = tmp_path / "prior.pth"
    m.export_model(path)
    a = torch.load(path, map_location="cpu")
    assert set(a) == EXPORT_KEYS                                     # no 'resolution'
    N = 6 * F
    for key, shape in (("means", (N, 3)), ("scales", (N, 3)), ("quats", (N, 4)), ("opacities", (N, 1)), ("normals", (N, 3)), ("kd", (N, 3)),
                       ("ks", (N, 2)), ("mc_positions", (N, 3)), ("mc_vertices", tuple(v32.shape)), ("mc_indices", (F, 3)),
                       ("latlng", (256, 512, 3)), ("exposure", (1,)), ("initial_guess", (2,))):
        assert tuple(a[key].shape) == shape, key
    assert a["mc_indices"].dtype == torch.int32
    assert (a["occ"] is None) if smooth_type != "jitter" else (tuple(a["occ"].shape) == (N, 6))
    assert set(a["occ_enc"]) == {"encoder.params", "mlp.nn_layers.0.weight", "mlp.nn_layers.1.weight", "mlp.nn_layers.2.weight"}


def test_prior_model_fits_a_brighter_light():
    """Targets rendered by a PriorModel whose light is 1.0; the model under test starts from 0.5 and takes 30 steps with the prior
    trainer's schedule, fixed shader seed and backgrounds.  The mean of the last five losses must be below the mean of the first five.
    Measured on an MI355X (two runs): first five 0.0770 and 0.0761, last five 0.0068 and 0.0075."""
    import geosplatting_amd as gs
    from geosplatting_amd import stage2
    v, f = _sphere()
    cams = _cams(2)
    make = lambda: gs.PriorModel(v, f, log2_hashmap_size=LOG2, seed=1)
    target = make()
    target.num_samples_per_ray = NS
    with torch.no_grad():
        target.latlng.fill_(1.0)
        gts = [img.clamp(0, 1) for img in target.render_report(cams, rnd_seed=21)[0]]
    assert float(gts[0][..., 3].max()) > 0.9
    m = make()
    m.num_samples_per_ray = NS
    sched = gs.Stage2Schedule.prior()
    opts = sched.setup(m)
    g = torch.Generator().manual_seed(8)
    bgs = [torch.rand(HW, HW, 3, generator=g).to(_dev()) for _ in cams]
    losses = []
    for step in range(30):
        sched.before_update(m, step, opts)
        out = stage2.train_step(m, cams, gts, gt_is_srgb=False, train_bg=bgs, rnd_seed=21)
        sched.scale_light_gradient(m)
        for opt in opts.values():
            opt.step()
        sched.after_update(m, step)
        losses.append(float(out["loss"]))
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f"first five {first:.6f}, last five {last:.6f}, light mean {float(m.latlng.mean()):.4f}")
    assert all(math.isfinite(x) for x in losses) and last < first
