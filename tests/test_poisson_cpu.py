"""No-GPU checks of differentiable Poisson reconstruction: tests/poisson_ref.py (the float64 restatement the GPU tests compare
against) reproduces the reference's own fp32 results of tests/golden/ref_dpsr.npz -- the raster, phi and the autograd gradients to
points and normals, five cases (scripts/make_golden_dpsr.py) -- and satisfies the identities the kernels are tested for.

E_ref per case (largest deviation of the reference's fp32 result from the restatement; the gradients relative to their max-norm),
as measured:   r16 phi 4.2e-7, points 3.1e-7, normals 3.1e-7;  r24 1.2e-6, 1.4e-6, 1.5e-6;  r8x12x10 2.9e-7, 6.3e-7, 8.7e-7;
r9 4.9e-7, 5.1e-7, 5.0e-7;  r16_plain 3.2e-8, 2.4e-7, 2.6e-7.  The bound here is 1.25e-5 of the max-norm: an fp32 evaluation of a few
hundred terms against float64, and an eighth of the project's 1e-4, so that the GPU tests' 8 E_ref stays below 1e-4.  A wrong
frequency sign, a missing DC zero or a mishandled Nyquist plane is off by 1e-3 or more.
"""
import numpy as np
import pytest
import torch

from tests import poisson_ref as P


@pytest.mark.parametrize("tag", P.GOLDEN_CASES)
def test_restatement_matches_the_reference(tag):
    c, e = P.golden(tag), P.e_ref(tag)
    raster = P.splat(c["points"], c["normals"], c["res"])
    e_raster = float((raster - c["raster"].double()).abs().max())
    print(f"{tag}: E_ref phi {e['phi']:.2e} (max {e['max.phi']:.3f})  grad points {e['grad.points'] / e['max.grad.points']:.2e}"
          f"  grad normals {e['grad.normals'] / e['max.grad.normals']:.2e}  raster {e_raster:.2e} (max {float(raster.abs().max()):.2f})")
    assert e_raster <= 1.25e-5 * float(raster.abs().max())
    for name in ("phi", "grad.points", "grad.normals"):
        assert 0 < e[name] <= 1.25e-5 * e["max." + name], (name, e[name], e["max." + name])


def test_sign_convention_on_a_sphere():
    """outward normals: phi[0,0,0] = +0.5, negative at the centre, zero crossing at the sphere (world radius 0.6 -> 0.24)"""
    g = torch.Generator().manual_seed(5)
    d = torch.randn(4000, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    p = (0.5 + 0.24 * d).float()
    phi = P.indicator(p, d.float(), 32, 0.05)
    assert abs(float(phi[0, 0, 0]) - 0.5) < 1e-12 and float(phi[16, 16, 16]) < -0.4
    line = phi[16, 16, 16:]                                                     # along +axis 2 from the centre
    k = int((line < 0).sum())                                                   # first non-negative node
    cross = (k - 1 + float(line[k - 1] / (line[k - 1] - line[k]))) / 32.0
    assert abs(cross - 0.24) < 0.01, cross


def test_splat_and_sample_are_adjoint_and_wrap():
    g = torch.Generator().manual_seed(1)
    res = (8, 12, 10)
    p = torch.rand(200, 3, generator=g) * 3.0 - 1.0                              # wraps
    p[0] = torch.tensor([1.0, 0.0, 1.0 - 2.0 ** -24]); p[1] = torch.tensor([float("nan"), 0.5, 0.5]); p[2] = torch.tensor([0.5, 2000.0, 0.5])
    v = torch.randn(200, 3, generator=g)
    G = torch.randn(3, *res, generator=g, dtype=torch.float64)
    grid = P.splat(p, v, res)
    lhs, rhs = float((grid * G).sum()), float((v.double() * P.sample(G, p)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((grid.abs() * G.abs()).sum())
    assert torch.isfinite(grid).all()
    assert torch.equal(P.sample(G, p)[1:3], torch.zeros(2, 3, dtype=torch.float64))
    # p = 1.0 lands on node 0 with weight 1; a point and the point one period away splat alike
    one = P.splat(torch.tensor([[1.0, 1.0, 1.0]]), torch.ones(1, 1), res)
    assert float(one[0, 0, 0, 0]) == 1.0 and float(one.sum()) == 1.0
    a = P.splat(torch.tensor([[0.25, 0.5, 0.75]]), torch.ones(1, 1), res)
    b = P.splat(torch.tensor([[-0.75, 1.5, 2.75]]), torch.ones(1, 1), res)
    assert float((a - b).abs().max()) < 1e-6


@pytest.mark.parametrize("res", [(8, 8, 8), (9, 9, 9), (8, 12, 10)])
def test_spectral_coefficients(res):
    c = P.spectral_coefficients(res, 0.05)
    k = P.frequencies(res)
    assert torch.equal(c[:, 0, 0, 0], torch.zeros(3, dtype=torch.complex128))
    assert float(c.real.abs().max()) == 0.0                                     # -i omega G / denom: purely imaginary
    for a in range(2):                                                          # fftfreq: an even side's Nyquist term is -R/2
        assert float(k[..., a].min()) == -(res[a] // 2) and float(k[..., a].max()) == (res[a] - 1) // 2
    assert float(k[..., 2].min()) == 0 and float(k[..., 2].max()) == res[2] // 2
    # away from DC: c_d = i G k_d / (2 pi |k|^2) up to the 1e-6 regulariser
    kk = (k ** 2).sum(-1)
    want = torch.exp(-2 * 0.05 ** 2 * kk)[None] * k.permute(3, 0, 1, 2) / (2 * np.pi * kk.clamp_min(1.0))[None]
    live = kk > 0
    assert float((c.imag - want)[:, live].abs().max()) < 1e-7


def test_vertex_normals_and_gradient_rule():
    res = (12, 16, 20)
    ax = [torch.arange(r, dtype=torch.float64) / r for r in res]
    X = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)
    phi = ((X - 0.5) ** 2).sum(-1) - 0.3 ** 2                                   # grad = 2 (x - 0.5): central differences are exact
    verts = torch.tensor([[6.0, 8.0, 16.25], [9.5, 8.0, 10.0], [3.0, 4.75, 10.0]], dtype=torch.float64)
    n = P.vertex_normals(phi, verts)
    want = verts / torch.tensor(res, dtype=torch.float64) - 0.5
    want = want / want.norm(dim=-1, keepdim=True)
    assert float((n - want).abs().max()) < 1e-12
    assert torch.equal(P.vertex_normals(torch.zeros(res), verts), torch.zeros(3, 3, dtype=torch.float64))
    gv = torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [-1.0, 0.5, 0.0]], dtype=torch.float64)
    v01 = (verts / torch.tensor(res, dtype=torch.float64)).float()
    g_phi = P.vertex_gradient_rule(v01, n, gv, res)
    assert abs(float(g_phi.sum()) + float((gv * n).sum())) < 1e-12              # the splat conserves the sum


def test_ops_refuse_cpu_tensors():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    p, v = torch.rand(4, 3), torch.rand(4, 3)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.splat_to_grid(p, v, 8)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.sample_grid(torch.zeros(1, 8, 8, 8), p)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.poisson_indicator(p, v, 8, 0.05)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.mesh_from_indicator(torch.zeros(8, 8, 8))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.mesh_from_oriented_points(p, v, 8)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.remesh_poisson(p, torch.tensor([[0, 1, 2]]), 8)


def test_entry_points_validate_before_the_device():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    assert lib.gs_grid_splat_ws_bytes(3, 8, 12, 10) == 16 + 8 * 3 * 960
    assert lib.gs_grid_splat_ws_bytes(3, 3, 8, 8) == 0 and lib.gs_grid_splat_ws_bytes(5, 8, 8, 8) == 0
    assert lib.gs_grid_splat_ws_bytes(1, 2048, 2048, 512) == 0                  # 2^31 nodes
    assert lib.gs_grid_splat(1, 1, 2, 8, 8, None, None, None, None, 0, None) == -1 and b"resolution" in lib.gs_last_error()
    assert lib.gs_grid_sample_fwd(1, 5, 8, 8, 8, None, None, None, None) == -1 and b"C must be" in lib.gs_last_error()
    assert lib.gs_grid_sample_bwd(-1, 1, 8, 8, 8, None, None, None, None, None) == -1
    assert lib.gs_poisson_spectral_fwd(8, 8, 8, -1.0, None, None, None) == -1 and b"sigma" in lib.gs_last_error()
    assert lib.gs_poisson_spectral_bwd(8, 8, 8, 0.05, None, None, None) == -1 and b"null" in lib.gs_last_error()
    assert lib.gs_grid_pack_volume(8, 8, 8, None, None, None) == -1
    assert lib.gs_grid_vertex_normals(8, 8, 8, None, 1 << 31, None, None, None) == -1
