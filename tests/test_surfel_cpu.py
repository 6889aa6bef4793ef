"""No-GPU checks of the 2D Gaussian splatting path: known answers for the float64 restatement (tests/surfel_ref.py), the exclusion caps
of the GPU tests' scenes on the restatement alone, and the public surface."""
import math

import pytest
import torch

from tests import surfel_ref as R

F, W, H = 40.0, 16, 16


def _cam():
    K = torch.tensor([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]], dtype=torch.float64)
    return torch.eye(4, dtype=torch.float64), K


def _surfels(zs, s=0.1, o=0.8, quat=(1.0, 0.0, 0.0, 0.0)):
    n = len(zs)
    means = torch.tensor([[0.0, 0.0, z] for z in zs], dtype=torch.float64)
    quats = torch.tensor([quat] * n, dtype=torch.float64)
    scales = torch.full((n, 3), s, dtype=torch.float64)
    return means, quats, scales, torch.full((n,), o, dtype=torch.float64), torch.full((n, 3), 0.5, dtype=torch.float64)


def _render(zs, **kw):
    vm, K = _cam()
    means, quats, scales, opac, cols = _surfels(zs, **kw)
    return R.rasterization_2dgs(means, quats, scales, opac, cols, vm, K, W, H, render_mode="RGB+D", distloss=True)


@pytest.mark.parametrize("s,z", [(0.1, 2.0), (0.004, 1.0)])          # the ray branch everywhere / the low-pass branch everywhere
def test_fronto_parallel_alpha_closed_form(s, z):
    out = _render([z], s=s)
    radius = int(out["radii"][0])
    assert radius == math.ceil(3 * max(s * F / z, 1e-2))
    for y in range(H):
        for x in range(W):
            d2 = (x + 0.5 - W / 2) ** 2 + (y + 0.5 - H / 2) ** 2
            a = R.fronto_parallel_alpha(d2, s, F, z, 0.8)
            want = a if a >= 1 / 255 else 0.0
            assert abs(float(out["alpha"][y, x]) - want) < 1e-12
    assert (out["ray_frac"] == 1.0) if s == 0.1 else (out["lowpass_frac"] == 1.0)


def test_one_surfel_has_no_distortion_two_have_the_pair_term():
    one = _render([2.0])
    assert float(one["distort"].abs().max()) == 0.0
    two = _render([2.0, 3.0])
    y, x = H // 2, W // 2
    d2 = 0.5
    a1, a2 = R.fronto_parallel_alpha(d2, 0.1, F, 2.0, 0.8), R.fronto_parallel_alpha(d2, 0.1, F, 3.0, 0.8)
    vis1, vis2 = a1, a2 * (1 - a1)
    assert abs(float(two["distort"][y, x]) - 2 * vis1 * vis2 * (3.0 - 2.0)) < 1e-12
    assert abs(float(two["median"][y, x]) - (3.0 if 1 - a1 > 0.5 else 2.0)) < 1e-12
    assert abs(float(two["render"][y, x, 3]) - (vis1 * 2.0 + vis2 * 3.0)) < 1e-12


def test_normal_faces_the_camera():
    towards = _render([2.0], quat=(0.0, 1.0, 0.0, 0.0))          # half a turn about x: the surfel's axis is (0, 0, -1)
    away = _render([2.0])                                        # its axis is (0, 0, 1), pointing away: flipped
    for out in (towards, away):
        assert torch.allclose(out["normals_cam"][0], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64), atol=1e-12)
    y, x = H // 2, W // 2
    assert float(away["normals"][y, x, 2]) < 0 and abs(float(away["normals"][y, x, 2]) + float(away["alpha"][y, x])) < 1e-12


def test_depth_to_normal_of_a_plane():
    vm, K = _cam()
    n = R.depth_to_normal(torch.full((H, W, 1), 2.0, dtype=torch.float64), vm, K)
    assert torch.allclose(n[1:-1, 1:-1], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand(H - 2, W - 2, 3), atol=1e-12)
    assert float(n[0].abs().max()) == 0.0 and float(n[:, -1].abs().max()) == 0.0
    import geosplatting_amd as gs
    got = gs.depth_to_normal(torch.full((H, W, 1), 2.0) + 0.01 * torch.arange(W)[None, :, None], vm.float(), K.float())
    want = R.depth_to_normal(torch.full((H, W, 1), 2.0, dtype=torch.float64) + 0.01 * torch.arange(W)[None, :, None], vm, K)
    assert torch.allclose(got.double(), want, atol=1e-5)


@pytest.mark.parametrize("name", ["inside", "outside", "clamp"])
def test_gpu_scene_exclusions_within_caps(name):
    """the seeds of tests/test_gpu_surfels.py: the restatement alone leaves out at most 1 % of the pixels and 0.5 % of the Gaussians"""
    sc = R.make_scene(name)
    with torch.no_grad():
        out = R.rasterization_2dgs(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["opacities"].double(),
                                   sc["sh"].double(), sc["viewmat"].double(), sc["K"].double(), sc["W"], sc["H"], sh_degree=sc["sh_degree"],
                                   background=sc["background"].double(), render_mode="RGB+ED", distloss=True, near=sc["near"])
    assert out["pix_bad"].double().mean().item() <= 0.01
    assert out["gauss_bad"].double().mean().item() <= 0.005
    assert out["n_clamped"] > 0 and out["n_skipped"] > 0
    if name == "inside":
        M2 = out["ray_transforms"][:, 2]
        d = M2[:, 0] ** 2 + M2[:, 1] ** 2 - M2[:, 2] ** 2
        assert 0 < out["ids"].numel() < 0.6 * sc["means"].shape[0] and (d > 0).any() and (d < 0).any()
    elif name == "outside":
        assert out["ray_frac"] >= 0.05 and out["lowpass_frac"] >= 0.05
    else:                                                        # the clamp active on several contributions of either branch
        assert out["n_clamped_ray"] >= 5 and out["n_clamped_lowpass"] >= 4


def test_public_surface():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    assert issubclass(gs.SurfelModel, gs.GSplatModel) and issubclass(gs.SurfelTrainer, gs.GSplatTrainer)
    z = torch.zeros(1, 3)
    args = (z, torch.ones(1, 4), z + 1, torch.ones(1), z, torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.rasterization_2dgs(*args)
    g = gs.GaussianSet.random(4, sh_degree=0, random_scale=1.0, generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError):
        gs.GSplatModel(gaussians=g, rasterize_mode="2dgs").render_rgb(None)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.SurfelModel(gaussians=g).render_rgb(gs.orbit_cameras(1, 3.0, 0.0, 16, 16, focal=20.0)[0])
    t = gs.SurfelTrainer()
    assert (t.normal_weight, t.distort_weight, t.normal_start, t.distort_start) == (5e-2, 1e-2, 7000, 3000)
