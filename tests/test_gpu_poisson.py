"""Differentiable Poisson reconstruction on the GPU (geosplatting_amd/poisson.py, csrc/gs_poisson.hip) against the float64
restatement tests/poisson_ref.py and the reference's own results in tests/golden/ref_dpsr.npz.

Budgets.  Splat, sample and the gradient to the points are compared per node / per point with the running-error budgets derived in
tests/poisson_ref.py's docstring from the kernels' arithmetic (u = 2^-24): they scale with sum |w v| and with the R u error of p R.
The spectral kernel: omega (one rounding), the filter (one cast), G S (one), times omega (one), the sum over d (two), the
denominator (four, all terms of one sign) and one division: under 16 u of sum_d |c_d S_d| per element.  poisson_indicator: 8 x that
case's E_ref (tests/test_poisson_cpu.py), never above 1e-4 of the max-norm.  Vertices: s = ta / (ta - tb) has opposite signs
under the difference (no cancellation), three roundings, then the sum with the node, the division by R and the test's product with
R: (3 + 3 R) u in node units.  Normals: a node gradient component is within R u max|phi| + u / 2 |g|, the interpolation adds three
roundings of at most 2 max|g|, the test recovers the position along the edge from v / R * R (within R u / 2, against a slope of at
most 2 G), the normalisation five: |dn| <= 2 sqrt(3) (R u max|phi| + 7 u G + R u G) / |g| + 5 u with G the largest node gradient
component.

Measured on an MI355X (error / budget, the largest over the cases of a test): see the docstrings of the tests.
"""
import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import poisson as GP
from geosplatting_amd.synthetic import icosphere
from tests import poisson_ref as P

pytestmark = pytest.mark.gpu
U = P.U


@pytest.fixture(scope="module", autouse=True)
def fft_plans(cuda):
    """one small solve, forward and backward, at every grid size of this module before the first test: the FFT library builds its
    plans per size (seconds each), and that stays out of the tests' times"""
    p = torch.tensor([[0.3, 0.4, 0.5], [0.6, 0.5, 0.4], [0.5, 0.7, 0.3], [0.4, 0.3, 0.6]], device=cuda, requires_grad=True)
    n = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]], device=cuda)
    for res in [P.golden(tag)["res"] for tag in P.GOLDEN_CASES] + [(32, 32, 32)]:
        gs.poisson_indicator(p, n, res, 0.05).sum().backward()
    torch.cuda.synchronize()


def _awkward_rows(res):
    """points on nodes, in the last cell of each axis, p = 0, 1 - 2^-24, 1.0, -0.25, 4096 points in one cell, duplicates, and three
    rows that take no part (a NaN, an inf, |p| >= 1024)"""
    R = torch.tensor(res, dtype=torch.float32)
    g = torch.Generator().manual_seed(11)
    rows = [torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [3.0, 0.0, 1.0]]) / R,                          # on nodes
            (R - 1.0 + torch.tensor([[0.5, 0.25, 0.75], [0.999, 0.5, 0.001]])) / R,                        # last cell: wraps
            torch.tensor([[0.0, 0.0, 0.0], [1.0 - 2.0 ** -24] * 3, [1.0, 1.0, 1.0], [-0.25, -0.25, -0.25],
                          [1.0, 0.3, 1.0 - 2.0 ** -24], [-2.0 ** -30, 0.5, 17.125]]),
            (torch.tensor([2.0, 3.0, 1.0]) + torch.rand(4096, 3, generator=g)) / R,                        # one cell
            torch.tensor([[0.3, 0.6, 0.9]] * 5)]                                                           # duplicates
    bad = torch.tensor([[float("nan"), 0.5, 0.5], [0.5, float("inf"), 0.5], [0.5, 0.5, -1024.0]])
    return torch.cat(rows + [bad]), 3


_cases = {}


def _case(N, C, res):
    """inputs, and the float64 reference with its budgets, computed once per shape"""
    key = (N, C, res)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * N + 10 * C + res[1])
        p = torch.rand(N, 3, generator=g) * 1.5 - 0.25                          # a quarter of them wrap
        n_bad = 0
        if N == 1000:
            extra, n_bad = _awkward_rows(res)
            p = torch.cat((p, extra))
        v = torch.randn(p.shape[0], C, generator=g)
        grid = torch.randn(C, *res, generator=g)
        c = dict(p=p, v=v, grid=grid, n_bad=n_bad)
        c["splat"], c["splat_bud"] = P.splat(p, v, res), P.splat_budget(p, v, res)
        c["sample"], c["sample_bud"] = P.sample(grid, p), P.sample_budget(grid, p)
        p64, v64 = p.double().requires_grad_(True), v.double().requires_grad_(True)
        (P.splat(p64, v64, res) * grid.double()).sum().backward()              # cotangent of the splat: `grid`
        c["splat_gp"], c["splat_gv"] = p64.grad, v64.grad
        p64, g64 = p.double().requires_grad_(True), grid.double().requires_grad_(True)
        (P.sample(g64, p64) * v.double()).sum().backward()                      # cotangent of the sample: `v`
        c["sample_gp"], c["sample_gg"] = p64.grad, g64.grad
        c["gp_bud"] = P.point_grad_budget(grid, p, v)                           # the same bound for both point gradients
        _cases[key] = c
    return _cases[key]


def _ratio(got, want, budget):
    """largest error / budget; an element with a zero budget must be exact"""
    err = (got.detach().double().cpu() - want).abs()
    assert torch.isfinite(got).all()
    assert bool((err[budget == 0] == 0).all())
    return float((err / budget.clamp_min(1e-300))[budget > 0].max()) if bool((budget > 0).any()) else 0.0


@pytest.mark.parametrize("res", [(8, 8, 8), (8, 12, 10)])
@pytest.mark.parametrize("N", [0, 1, 63, 1000])
@pytest.mark.parametrize("C", [1, 3])
def test_splat_and_sample_per_element(cuda, C, N, res):
    """Forward and both backward directions of both ops per node / per point within the running-error budgets.
    Measured error / budget, largest over the 16 cases: splat 0.70, sample 0.43 (the gradients to the values and to the grid are
    the other op: the same figures), point gradients 0.35."""
    c = _case(N, C, res)
    p = c["p"].to(cuda).requires_grad_(True)
    v = c["v"].to(cuda).requires_grad_(True)
    grid = c["grid"].to(cuda).requires_grad_(True)
    out = gs.splat_to_grid(p, v, res)
    assert out.shape == (C, *res)
    r = {"splat": _ratio(out, c["splat"], c["splat_bud"])}
    gp, gv = torch.autograd.grad(out, (p, v), grid.detach())
    r["splat.g_values"] = _ratio(gv, c["splat_gv"], c["sample_bud"])            # = sample(cotangent, p)
    r["splat.g_points"] = _ratio(gp, c["splat_gp"], c["gp_bud"])
    smp = gs.sample_grid(grid, p)
    assert smp.shape == (p.shape[0], C)
    r["sample"] = _ratio(smp, c["sample"], c["sample_bud"])
    gg, gp2 = torch.autograd.grad(smp, (grid, p), v.detach())
    r["sample.g_grid"] = _ratio(gg, c["sample_gg"], c["splat_bud"])             # = splat(p, cotangent)
    r["sample.g_points"] = _ratio(gp2, c["sample_gp"], c["gp_bud"])
    print(f"C {C} N {N} res {res}: error / budget " + "  ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert max(r.values()) <= 1.0, r
    if c["n_bad"]:                                                              # rows that take no part: nothing read, zero gradients
        k = c["n_bad"]
        zero = torch.zeros(k, 3, device=cuda)
        assert torch.equal(smp[-k:], zero[:, :C]) and torch.equal(gv[-k:], zero[:, :C])
        assert torch.equal(gp[-k:], zero) and torch.equal(gp2[-k:], zero)
        p_ok, v_ok = p.detach().clone(), v.detach().clone()                     # ... and nothing added, bit for bit: the same rows as
        p_ok[-k:], v_ok[-k:] = 0.5, 0.0                                         # valid points with zero values
        assert torch.equal(out, gs.splat_to_grid(p_ok, v_ok, res))


@pytest.mark.parametrize("res", [(8, 8, 8), (8, 12, 10)])
def test_adjointness(cuda, res):
    """<splat(p, v), g> = <v, sample(g, p)> within the two budgets summed against |g| and |v|.  Measured: |lhs - rhs| 5.7e-7 and 7.4e-7 against bounds of 0.078 and 0.095 (sums of absolute budgets)."""
    c = _case(1000, 3, res)
    p, v, g = c["p"].to(cuda), c["v"].to(cuda), c["grid"].to(cuda)
    lhs = float((gs.splat_to_grid(p, v, res).double() * g.double()).sum())
    rhs = float((v.double() * gs.sample_grid(g, p).double()).sum())
    bound = float((c["splat_bud"] * c["grid"].double().abs()).sum() + (c["sample_bud"] * c["v"].double().abs()).sum())
    print(f"adjointness {res}: |lhs - rhs| {abs(lhs - rhs):.3e}  bound {bound:.3e}  ratio {abs(lhs - rhs) / bound:.3f}")
    assert abs(lhs - rhs) <= bound


def test_reproducibility(cuda):
    """Two calls of the splat and two calls of each backward are bitwise equal (integer accumulation; gathers elsewhere)."""
    c = _case(1000, 3, (8, 12, 10))
    res = (8, 12, 10)
    runs = []
    for _ in range(2):
        p = c["p"].to(cuda).requires_grad_(True)
        v = c["v"].to(cuda).requires_grad_(True)
        grid = c["grid"].to(cuda).requires_grad_(True)
        out = gs.splat_to_grid(p, v, res)
        a = torch.autograd.grad(out, (p, v), grid.detach())
        b = torch.autograd.grad(gs.sample_grid(grid, p), (grid, p), v.detach())
        runs.append((out, *a, *b))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    # the order of the rows does not matter either: integer sums
    perm = torch.randperm(c["p"].shape[0], generator=torch.Generator().manual_seed(3))
    assert torch.equal(runs[0][0], gs.splat_to_grid(c["p"][perm].to(cuda), c["v"][perm].to(cuda), res))


@pytest.mark.parametrize("res", [(8, 8, 8), (9, 9, 9), (8, 12, 10)])
def test_spectral_kernel_alone(cuda, res):
    """The Fourier-space step on seeded complex input, no FFT: per element within 16 u sum_d |c_d S_d| of the restatement's
    coefficients, DC exactly 0, the Nyquist planes on their own, and the adjoint identity.  Measured error / budget: forward 0.17, adjoint 0.21;
    the identity holds to 0.002 of its bound."""
    g = torch.Generator().manual_seed(7)
    H = res[2] // 2 + 1
    sigma = 0.05
    S = torch.complex(torch.randn(3, res[0], res[1], H, generator=g), torch.randn(3, res[0], res[1], H, generator=g))
    gP = torch.complex(torch.randn(res[0], res[1], H, generator=g), torch.randn(res[0], res[1], H, generator=g))
    c = P.spectral_coefficients(res, sigma)
    want = (c * S.to(torch.complex128)).sum(0)
    bud = 16 * U * (c.abs() * S.to(torch.complex128).abs()).sum(0)
    Sd = S.to(cuda).requires_grad_(True)
    Phi = GP.poisson_spectral(Sd, res, sigma)
    assert Phi.dtype == torch.complex64 and Phi.shape == (res[0], res[1], H)
    got = Phi.detach().cpu().to(torch.complex128)
    assert got[0, 0, 0] == 0 and bud[0, 0, 0] == 0
    err = (got - want).abs()
    live = bud > 0
    ratio = float((err[live] / bud[live]).max())
    assert bool((err[~live] == 0).all())
    planes = [(res[0] // 2, slice(None), slice(None))] * (res[0] % 2 == 0) + [(slice(None), res[1] // 2, slice(None))] * (res[1] % 2 == 0) \
        + [(slice(None), slice(None), H - 1)] * (res[2] % 2 == 0)
    for pl in planes:                                                           # -R/2 on the first two axes, +R/2 on the last
        assert bool((err[pl] <= bud[pl]).all()) and float(want[pl].abs().max()) > 1e-3
    (gS,) = torch.autograd.grad(Phi, Sd, gP.to(cuda))
    want_g = c.conj() * gP.to(torch.complex128)[None]
    bud_g = 16 * U * c.abs() * gP.to(torch.complex128).abs()[None]
    err_g = (gS.cpu().to(torch.complex128) - want_g).abs()
    ratio_g = float((err_g[bud_g > 0] / bud_g[bud_g > 0]).max())
    assert bool((err_g[bud_g == 0] == 0).all())
    lhs = float((got * gP.to(torch.complex128).conj()).sum().real)              # Re <c S, g>
    rhs = float((S.to(torch.complex128) * gS.cpu().to(torch.complex128).conj()).sum().real)   # Re <S, conj(c) g>
    bound = float(32 * U * (c.abs() * S.to(torch.complex128).abs() * gP.to(torch.complex128).abs()[None]).sum())
    print(f"spectral {res}: error / budget fwd {ratio:.3f} bwd {ratio_g:.3f}  adjoint |lhs - rhs| / bound {abs(lhs - rhs) / bound:.3f}")
    assert ratio <= 1.0 and ratio_g <= 1.0 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("tag", P.GOLDEN_CASES)
def test_indicator_against_the_golden(cuda, tag):
    """poisson_indicator against the reference's own phi and autograd gradients, within 8 x that case's E_ref (hipFFT factorises
    differently from the CPU's FFT and the splat sums in another order), never above 1e-4 of the max-norm.
    Measured multiples of E_ref (phi, grad points, grad normals): r16 0.86, 0.82, 1.02; r24 1.04, 0.95, 0.96; r8x12x10 1.22, 0.97,
    0.97; r9 0.98, 1.39, 0.89; r16_plain 0.94, 0.93, 0.98 -- the device result is as far from the reference as the float64
    restatement is."""
    c, e = P.golden(tag), P.e_ref(tag)
    p = c["points"].to(cuda).requires_grad_(True)
    n = c["normals"].to(cuda).requires_grad_(True)
    phi = gs.poisson_indicator(p, n, c["res"], c["sigma"], shift=c["shift"], scale=c["scale"])
    assert phi.shape == c["res"] and phi.dtype == torch.float32
    gp, gn = torch.autograd.grad(phi, (p, n), c["cot"].to(cuda))
    mult = {}
    for name, got in (("phi", phi), ("grad.points", gp), ("grad.normals", gn)):
        err = float((got.detach().cpu().double() - c[name].double()).abs().max())
        bound = 8.0 * e[name]
        assert bound <= 1e-4 * e["max." + name]
        mult[name] = err / e[name]
    print(f"{tag}: multiples of E_ref " + "  ".join(f"{k} {x:.2f}" for k, x in mult.items()))
    assert max(mult.values()) <= 8.0, mult


_spheres = {}


def _sphere_phi(res):
    if res not in _spheres:
        g = torch.Generator().manual_seed(21)
        d = torch.randn(3000, 3, generator=g, dtype=torch.float64)
        d = d / d.norm(dim=-1, keepdim=True)
        _spheres[res] = P.indicator((0.5 + 0.27 * d).float(), d.float(), res, 0.05).float()
    return _spheres[res]


def _edge_count(faces):
    e = torch.cat((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    V = int(faces.max()) + 1
    directed = e[:, 0] * V + e[:, 1]
    lo, hi = e.min(1).values, e.max(1).values
    return torch.unique(directed, return_counts=True)[1], torch.unique(lo * V + hi, return_counts=True)[1]


def _signed_volume(v, f):
    a, b, c = (v[f[:, k]].double() for k in range(3))
    return float((a * torch.cross(b, c, dim=-1)).sum() / 6.0)


@pytest.mark.parametrize("res", [(16, 16, 16), (12, 16, 20)])
def test_mesh_from_indicator(cuda, res):
    """Marching cubes on the restatement's phi of a sphere: vertices on sign-changing grid edges at the linear crossing, all
    referenced, closed and consistently wound, facing outward, normals and the vertex-gradient rule within their budgets.
    Measured error / budget: crossing 0.32, normals 0.02, g_phi 0.38."""
    phi32 = _sphere_phi(res)
    phi = phi32.double()
    Rt = torch.tensor(res, dtype=torch.float64)
    phid = phi32.to(cuda).requires_grad_(True)
    v, f, n = gs.mesh_from_indicator(phid, lo=0.0, hi=1.0)                      # unit-cube coordinates: the affine map is exact
    assert v.shape[0] > 100 and f.dtype == torch.int64 and n.shape == v.shape and not n.requires_grad
    x = v.detach().cpu().double() * Rt                                          # node units
    near = torch.round(x)
    off = (x - near).abs()
    tol = (3 + 3 * Rt) * U
    axis = off.argmax(-1)
    rows = torch.arange(x.shape[0])
    others = off.clone()
    others[rows, axis] = 0
    assert bool((others <= tol).all()), "a vertex off every grid edge"
    lo = near.long()
    lo[rows, axis] = torch.floor(x[rows, axis]).long()
    hi = lo.clone()
    hi[rows, axis] += 1
    assert bool((lo >= 0).all()) and bool((hi < torch.tensor(res)).all())       # no wrap: the (R - 1)^3 cubes
    ta, tb = phi[lo[:, 0], lo[:, 1], lo[:, 2]], phi[hi[:, 0], hi[:, 1], hi[:, 2]]
    assert bool(((ta < 0) != (tb < 0)).all()), "a vertex on an edge without a sign change"
    cross = lo[rows, axis].double() + ta / (ta - tb)
    r_cross = float(((x[rows, axis] - cross).abs() / tol[axis]).max())
    # every sign-changing edge carries exactly one vertex
    n_edges = sum(int(((phi.narrow(a, 0, res[a] - 1) < 0) != (phi.narrow(a, 1, res[a] - 1) < 0)).sum()) for a in range(3))
    assert v.shape[0] == n_edges
    fc = f.cpu()
    assert torch.equal(torch.unique(fc), torch.arange(v.shape[0]))              # no unreferenced vertices
    directed, undirected = _edge_count(fc)
    assert bool((undirected == 2).all()) and bool((directed == 1).all())        # closed, consistently wound
    assert _signed_volume(v.detach().cpu(), fc) > 0.5 * 4.0 / 3.0 * np.pi * 0.27 ** 3   # faces point outward
    # normals
    gref = P.vertex_gradients(phi, near.where(torch.nn.functional.one_hot(axis, 3) == 0, x))
    nref = gref / gref.norm(dim=-1, keepdim=True)
    idx = torch.stack(torch.meshgrid(*[torch.arange(r) for r in res], indexing="ij"), -1).reshape(-1, 3)
    G = float(P.node_gradient(phi, idx).abs().max())
    Rmax = max(res)
    n_bud = 2 * 3 ** 0.5 * (Rmax * U * float(phi.abs().max()) + 7 * U * G + Rmax * U * G) / gref.norm(dim=-1) + 5 * U
    n_err = (n.cpu().double() - nref).norm(dim=-1)
    r_n = float((n_err / n_bud).max())
    assert bool(((n.cpu().double() * (x / Rt - 0.5)).sum(-1) > 0).all())        # outward
    # the Shape-as-Points backward: g_phi = splat(v, -(g_v . n))
    gv = torch.randn(v.shape, generator=torch.Generator().manual_seed(5))
    (g_phi,) = torch.autograd.grad(v, phid, gv.to(cuda))
    v01 = v.detach().cpu()
    cot = -(gv.double() * nref).sum(-1, keepdim=True)
    d_cot = (gv.double().abs() * n_bud[:, None]).sum(-1, keepdim=True) + 3 * U * (gv.double() * nref).abs().sum(-1, keepdim=True)
    want = P.vertex_gradient_rule(v01, nref, gv, res)
    bud = P.splat_budget(v01, cot, res)[0] + P.splat(v01, d_cot, res)[0] * (1 + 8 * Rmax * U)
    r_g = _ratio(g_phi, want, bud)
    print(f"mesh {res}: V {v.shape[0]} F {f.shape[0]}  error / budget crossing {r_cross:.3f} normals {r_n:.3f} g_phi {r_g:.3f}")
    assert r_cross <= 1.0 and r_n <= 1.0 and r_g <= 1.0
    # no sign change: empty outputs, and a zero gradient
    pos = (phi32.abs() + 0.1).to(cuda).requires_grad_(True)
    v0, f0, n0 = gs.mesh_from_indicator(pos)
    assert v0.shape == (0, 3) and f0.shape == (0, 3) and n0.shape == (0, 3) and f0.dtype == torch.int64
    (g0,) = torch.autograd.grad(v0.sum(), pos)
    assert torch.equal(g0, torch.zeros_like(pos))


def _fit(cuda, sign):
    g = torch.Generator().manual_seed(9)
    d = torch.randn(2000, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    t = torch.randn(2000, 3, generator=g)
    target = (0.6 * t / t.norm(dim=-1, keepdim=True)).to(cuda)
    normals = d.to(cuda)
    pts = (0.45 * d).to(cuda).requires_grad_(True)
    opt = torch.optim.Adam([pts], lr=0.005)
    losses, radii = [], []
    for _ in range(41):
        v, f, _n = gs.diff_poisson_surface_recon(pts, normals, smoothness=0.05, resolution=32)
        d1, d2 = gs.chamfer_distance(v, target)
        loss = d1.mean() + d2.mean()
        losses.append(float(loss.detach()))
        radii.append(float(v.detach().norm(dim=-1).mean()))
        if len(losses) == 41:
            break
        opt.zero_grad()
        loss.backward()
        pts.grad.mul_(sign)
        opt.step()
    return losses, radii


def test_end_to_end_fit(cuda):
    """2 000 points on a sphere of radius 0.45 with radial normals, R = 32, sigma = 0.05; 40 Adam steps on the positions against the
    Chamfer distance to a sphere of radius 0.6 lower the loss and move the mean vertex radius toward 0.6; the same loop with the
    gradient negated does not (so this test can fail).  Measured: loss 0.0462 -> 0.0022 (ratio 0.047), mean vertex radius 0.451 ->
    0.612; negated: loss -> 0.397 (ratio 8.6), radius -> 0.157."""
    losses, radii = _fit(cuda, 1.0)
    neg_losses, neg_radii = _fit(cuda, -1.0)
    print(f"fit: loss {losses[0]:.5f} -> {losses[-1]:.5f} (ratio {losses[-1] / losses[0]:.3f}), mean radius {radii[0]:.4f} -> {radii[-1]:.4f};"
          f"  negated gradient: loss -> {neg_losses[-1]:.5f} (ratio {neg_losses[-1] / neg_losses[0]:.3f}), radius -> {neg_radii[-1]:.4f}")
    assert losses[-1] < losses[0]
    assert abs(radii[-1] - 0.6) < abs(radii[0] - 0.6)
    assert neg_losses[-1] >= neg_losses[0]


def test_remesh_poisson_closes_a_mesh(cuda):
    """an icosphere with a few faces removed comes back closed, outward and near its radius"""
    v, f = icosphere(3, 0.8)
    keep = torch.ones(f.shape[0], dtype=torch.bool)
    keep[[3, 4, 5, 100, 101, 640]] = False
    v2, f2, n2 = gs.remesh_poisson(v.to(cuda), f[keep].to(cuda), resolution=32, smoothness=0.05)
    assert v2.shape[0] > 500 and n2.shape == v2.shape
    fc = f2.cpu()
    directed, undirected = _edge_count(fc)
    assert bool((undirected == 2).all()) and bool((directed == 1).all())
    assert torch.equal(torch.unique(fc), torch.arange(v2.shape[0]))
    assert _signed_volume(v2.cpu(), fc) > 0
    radius = v2.norm(dim=-1)
    assert 0.7 < float(radius.min()) and float(radius.max()) < 0.9
