"""Stage 3 without a device: the light's (hue, value) parametrisation, `albedo_scaling`, `Stage3Schedule` and the load errors, on a
twelve-Gaussian export dictionary built by hand (tests/stage3_ref.py)."""
import pytest
import torch

from tests import stage3_ref as R


def _model(**kw):
    from geosplatting_amd.stage3 import Stage3Model
    return Stage3Model(R.hand_export(), "cpu", **kw)


def test_light_parametrisation_round_trip():
    """hue * exp(value) reproduces L to L * 1e-5 / (L + 1): the exact value is L (L + 1.00001) / (L + 1), and float32 adds at most
    (7 + 2 |log(L + 1.00001)|) 2^-24 relative to it -- the operation count is in `stage3_ref.light_budget`."""
    from geosplatting_amd.stage3 import light_from_params, light_to_params
    L = R.sample_light(3)
    hue, value = light_to_params(L)
    assert hue.dtype == torch.float32 and bool(((hue > 0) & (hue < 1)).all())
    worst = R.check_light_round_trip(L, light_from_params(hue, value))
    print(f"light round trip: largest error {worst:.3f} of the budget")
    m = _model()
    assert torch.equal(m.latlng_hue.detach(), light_to_params(R.hand_export()["latlng"])[0])
    R.check_light_round_trip(R.hand_export()["latlng"], m.get_envmap().data.detach())
    assert m.get_envmap().pdf is not None


def _albedo_case(seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(9, 7, 3, generator=g) * 0.95 + 0.05
    assert float(a.min()) >= 0.05 and float(a.max()) < 1.0
    return a


@pytest.mark.parametrize("mode", ["least-square", "median"])
def test_albedo_scaling_returns_an_exact_factor(mode):
    """gt = c * albedo with c = (0.5, 2, 4): a power of two scales every product, sum and quotient exactly, so both modes return c
    bit for bit"""
    from geosplatting_amd.stage3 import albedo_scaling
    c = torch.tensor([0.5, 2.0, 4.0])
    albedos = [_albedo_case(1), _albedo_case(2)]
    gts = [torch.cat((a * c, torch.ones(9, 7, 1)), -1) for a in albedos]
    assert torch.equal(albedo_scaling(albedos, gts, mode), c)
    assert torch.equal(albedo_scaling(albedos[:1], gts[:1], mode), c)


def test_albedo_scaling_median_mask_and_clamp():
    from geosplatting_amd.stage3 import albedo_scaling
    c = torch.tensor([0.5, 2.0, 4.0])
    a = _albedo_case(3)
    gt = torch.cat((a * c, torch.ones(9, 7, 1)), -1)
    gt[:5, :, :3] = 100.0                                    # more than half of the pixels say something else ...
    gt[:5, :, 3] = 0.0                                       # ... and are outside the mask
    assert torch.equal(albedo_scaling([a], [gt], "median"), c)
    # an albedo below 1e-3 divides as 1e-3
    tiny = torch.full((2, 2, 3), 1e-4)
    gt_tiny = torch.cat((torch.full((2, 2, 3), 1e-3) * c, torch.ones(2, 2, 1)), -1)
    assert torch.equal(albedo_scaling([tiny], [gt_tiny], "median"), c)
    # least-square blends the ground truth over black: a transparent pixel counts as zero
    half = torch.cat((a * c, torch.ones(9, 7, 1)), -1)
    half[:, :, 3] = 0.5
    assert torch.equal(albedo_scaling([a], [half], "least-square"), c * 0.5)
    with pytest.raises(ValueError):
        albedo_scaling([a], [gt], "mean")
    with pytest.raises(ValueError):
        albedo_scaling([a], [], "median")


TABLE = {"light_hue": (1.0, True), "light_value": (1.0, True), "exposure": (0.5, True), "means": (0.16, True), "normals": (1.0, True),
         "scales": (5.0, False), "quats": (1.0, False), "opacities": (50.0, False), "kd": (5.0, False), "ks": (0.5, False),
         "occ": (2.5, False)}


def test_schedule_table_half_life_and_fixed_material():
    from geosplatting_amd.stage3 import Stage3Schedule
    m = _model()
    sched = Stage3Schedule()
    opts = sched.setup(m)
    assert set(opts) == set(TABLE)
    owner = {"light_hue": [m.latlng_hue], "light_value": [m.latlng_value], "exposure": [m.exposure_params], "means": [m.means],
             "normals": [m.normals], "scales": [m.scales], "quats": [m.quats], "opacities": [m.opacities], "kd": [m.kd_params],
             "ks": m.ks_enc.parameters(), "occ": [m.occ_params]}
    for name, (factor, _) in TABLE.items():
        group, = opts[name].param_groups
        assert group["lr"] == pytest.approx(1e-3 * factor, rel=1e-12), name
        assert group["eps"] == 1e-15, name
        assert len(group["params"]) == len(owner[name]) and all(p is q for p, q in zip(group["params"], owner[name])), name
    assert (m.kd_weight, m.ks_weight, m.normal_weight) == (0.0, 0.0, 0.0)
    sched.before_update(m, 0, opts)
    assert (m.kd_weight, m.ks_weight, m.normal_weight) == (0.2, 0.05, 0.0)
    at0 = {name: opts[name].param_groups[0]["lr"] for name in TABLE}
    sched.before_update(m, 500, opts)
    for name, (factor, decays) in TABLE.items():
        assert at0[name] == pytest.approx(1e-3 * factor, rel=1e-12), name
        assert opts[name].param_groups[0]["lr"] == pytest.approx(at0[name] * (0.5 if decays else 1.0), rel=1e-12), name
    fixed = Stage3Schedule(fix_material=True).setup(m)
    assert set(fixed) == set(TABLE) - {"kd", "ks", "occ"}
    # the light's gradients, and only those, are scaled by 64
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    sched.scale_light_gradient(m)
    for name, p in m.named_parameters().items():
        assert bool((p.grad == (64.0 if name in ("latlng_hue", "latlng_value") else 1.0)).all()), name


def test_schedule_after_update_clamps():
    from geosplatting_amd.envshade import LatLngEnvMap
    from geosplatting_amd.stage3 import Stage3Schedule
    m = _model()
    sched = Stage3Schedule()
    lo, hi = float(torch.tensor(0.01)), float(torch.tensor(0.99))

    def spoil():
        with torch.no_grad():
            m.latlng_hue[0, 0], m.latlng_hue[0, 1] = -1.0, 2.0
            m.kd_params[0], m.kd_params[1] = -1.0, 2.0
    spoil()
    value = m.latlng_value.detach().clone()
    sched.after_update(m, 0)
    assert float(m.latlng_hue.detach().min()) == lo and float(m.latlng_hue.detach().max()) == hi
    assert float(m.kd_params.detach().min()) >= lo and float(m.kd_params.detach().max()) <= hi and float(m.kd_params.detach()[0, 0]) == lo
    assert torch.equal(m.latlng_value.detach(), value)
    # under a relight map the hue is not the light in use and is left alone; kd is still clamped
    m.set_relight_envmap(LatLngEnvMap(R.sample_light(5)), torch.ones(3))
    assert not m.learned_light
    spoil()
    sched.after_update(m, 1)
    assert float(m.latlng_hue.detach().min()) == -1.0 and float(m.latlng_hue.detach().max()) == 2.0
    assert float(m.kd_params.detach().min()) >= lo and float(m.kd_params.detach().max()) <= hi
    m.clear_relight_envmap()
    assert m.learned_light and m.albedo_scaling is None
    sched.after_update(m, 2)
    assert float(m.latlng_hue.detach().min()) == lo and float(m.latlng_hue.detach().max()) == hi


def test_relight_map_from_a_picture_file(tmp_path):
    from geosplatting_amd.envmap import load_hdr, save_hdr
    from geosplatting_amd.envshade import LatLngEnvMap
    path = tmp_path / "light.hdr"
    save_hdr(path, R.sample_light(7))
    m = _model()
    learned = m.get_envmap().data.detach().clone()
    m.set_relight_envmap(str(path), torch.tensor([0.5, 1.0, 2.0]))
    env = m.get_envmap()
    assert env is m.get_envmap() and env.pdf is not None and not env.data.requires_grad            # fixed: its tables are built once
    assert torch.equal(env.data, load_hdr(path)) and torch.equal(m.albedo_scaling, torch.tensor([0.5, 1.0, 2.0]))
    from geosplatting_amd.stage3 import Stage3Model
    given = Stage3Model(R.hand_export(), "cpu", gt_envmap=LatLngEnvMap(R.sample_light(7)))
    assert not given.learned_light and given.albedo_scaling is None and torch.equal(given.get_envmap().data, R.sample_light(7))
    m.clear_relight_envmap()
    assert torch.equal(m.get_envmap().data.detach(), learned)
    with pytest.raises(ValueError, match="3-vector"):
        m.set_relight_envmap(str(path), torch.ones(2))
    with pytest.raises(ValueError, match="transform"):
        m.set_relight_envmap(LatLngEnvMap(R.sample_light(7), transform=torch.eye(3)), torch.ones(3))


def test_loading_parameters_and_errors():
    from geosplatting_amd.stage3 import Stage3Model
    a = R.hand_export()
    m = Stage3Model(a, "cpu")
    names = m.named_parameters()
    assert list(names) == ["means", "scales", "quats", "opacities", "normals", "kd_params", "occ_params", "exposure_params", "latlng_hue",
                           "latlng_value", "ks_enc.0", "ks_enc.1", "ks_enc.2"]
    assert all(p.requires_grad and p.is_leaf for p in names.values())
    for t in (m.mesh_v, m.mesh_i, m.mesh_pos, m.initial_guess):
        assert not t.requires_grad
    assert torch.equal(m.kd_params.detach(), a["kd"]) and torch.equal(m.occ_params.detach(), a["occ"])
    assert torch.equal(m.mesh_pos, a["mc_positions"]) and m.mesh_i.dtype == torch.int64
    assert (m.scale, m.min_roughness, m.max_metallic, m.num_samples_per_ray) == (1.0, 0.1, 0.9, 16)
    assert m.ks_enc.log2_hashmap_size == 4 and all(torch.equal(p.detach().cpu(), a["ks_enc"][k]) for p, k in
                                                   zip(m.ks_enc.parameters(), ("encoder.params", "mlp.nn_layers.0.weight", "mlp.nn_layers.1.weight")))
    # 'vertices' / 'indices' take precedence and make the means the surface positions
    b = dict(a, vertices=a["mc_vertices"] * 2, indices=a["mc_indices"])
    mb = Stage3Model(b, "cpu")
    assert torch.equal(mb.mesh_v, a["mc_vertices"] * 2) and torch.equal(mb.mesh_pos, a["means"])
    no_max = {k: v for k, v in a.items() if k != "max_metallic"}
    assert Stage3Model(no_max, "cpu").max_metallic == 1.0
    with pytest.raises(ValueError, match="occ"):
        Stage3Model(dict(a, occ=None), "cpu")
    with pytest.raises(ValueError, match="mesh"):
        Stage3Model({k: v for k, v in a.items() if k != "mc_vertices"}, "cpu")
    with pytest.raises(ValueError, match="background_color"):
        Stage3Model(a, "cpu", background_color="grey")


def test_background_colour_and_state_dict(tmp_path):
    m = _model(seed=4)
    state = m.generator.get_state()
    first = m.get_background_color()
    assert first.shape == (3,) and not torch.equal(first, m.get_background_color())       # 'random' while training: a draw each
    m.generator.set_state(state)
    assert torch.equal(first, m.get_background_color())
    m.training = False
    assert torch.equal(m.get_background_color(), torch.tensor([0.1490, 0.1647, 0.2157]))
    m.background_color = "black"
    assert torch.equal(m.get_background_color(), torch.zeros(3))
    m.background_color = "white"
    assert torch.equal(m.get_background_color(), torch.ones(3))
    with torch.no_grad():
        m.kd_params.mul_(0.5); m.latlng_value.add_(0.1); m.ks_enc.weights[0].add_(0.25)
    m.save_checkpoint(tmp_path / "ckpt", 3)
    m2 = _model(seed=9)
    assert not torch.equal(m2.kd_params, m.kd_params)
    assert m2.load_checkpoint(tmp_path / "ckpt") == 3 and m2.load_checkpoint(tmp_path / "none") is None
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(m.parameters(), m2.parameters()))
