"""GPU parity of the GSplatter configuration of ``rasterization()`` (rfstudio/model/gsplat.py:23-36): spherical-harmonics colours
(sh_degree 0..3, colors [N, K, 3]), rasterize_mode='classic' and a differentiable ``meta["means2d"]`` (means2d_grad=True).

Every check is against the C oracle's stage functions, and the SH arithmetic against the float64 restatement below (gsplat 1.4's
polynomial "fast" form; tests/test_sh_cpu.py pins it to the classic 3DGS eval_sh form).
"""
import numpy as np
import pytest
import torch

import oracle
from tests.util import activated, rel_err

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4


# ---------------------------------------------------------------------------------------------- float64 SH restatement
def sh_basis_fast(deg, d):
    """Real SH basis of 3DGS, degrees 0..3, at unit directions d [..., 3], in gsplat's polynomial form: [..., (deg+1)^2]."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = [torch.full_like(x, 0.2820947917738781)]
    if deg >= 1:
        b += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if deg >= 2:
        z2, fTmp0B, fC1, fS1 = z * z, -1.092548430592079 * z, x * x - y * y, 2.0 * x * y
        b += [0.5462742152960395 * fS1, fTmp0B * y, 0.9461746957575601 * z2 - 0.3153915652525201, fTmp0B * x,
              0.5462742152960395 * fC1]
        if deg >= 3:
            fTmp0C, fTmp1B = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
            fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
            b += [-0.5900435899266435 * fS2, fTmp1B * fS1, fTmp0C * y, z * (1.865881662950577 * z2 - 1.119528997770346),
                  fTmp0C * x, fTmp1B * fC1, -0.5900435899266435 * fC2]
    return torch.stack(b, -1)


def sh_colors64(deg, means, campos, coeffs):
    """gsplat: c = sum_k basis_k(normalize(means - campos)) coeffs[:, k]; returns c (before + 0.5 and the clamp)."""
    dirs = means - campos
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    nb = (deg + 1) ** 2
    return (sh_basis_fast(deg, dirs)[..., None] * coeffs[:, :nb, :]).sum(-2)


def _campos(vm):
    return torch.from_numpy(np.linalg.inv(vm.astype(np.float64))[:3, 3])


# ---------------------------------------------------------------------------------------------- scenes
def _scene(n=4000, seed=3, inside=True):
    """Random splats seen from a camera inside the cloud (near-plane and frustum culling: some Gaussians invisible) at a
    ragged image size, or from outside at 128^2."""
    import geosplatting_amd.synthetic as syn
    from geosplatting_amd.cameras import Camera, lookat_c2w
    sp = syn.random_splats(n, seed=seed)
    if inside:
        c2w = lookat_c2w(torch.tensor([0.2, 0.1, 0.3]), torch.tensor([0.0, 0.0, -1.0]), torch.tensor([0.0, 1.0, 0.0]))
        cam = Camera(c2w, 90.0, 95.0, 50.0, 37.0, 100, 75)
    else:
        c2w = lookat_c2w(torch.tensor([0.0, 0.4, 3.0]), torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0]))
        cam = Camera(c2w, 150.0, 150.0, 64.0, 64.0, 128, 128)
    means, quats, scales, opac = activated(sp)
    return means, quats, scales, np.clip(opac * 5, 0, 0.95).astype(np.float32), cam


def _coeffs(n, K, seed, clamp_every=5):
    """SH coefficients [n, K, 3]; channel 0 of every clamp_every-th Gaussian gets a DC term far below -0.5 / C0 (clamped)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, K, 3, generator=g) * 0.3
    c[:, 0, :] = (torch.rand(n, 3, generator=g) - 0.5) / 0.28209479177387814
    if clamp_every:
        c[::clamp_every, 0, 0] = -6.0
    return c.numpy().astype(np.float32)


def _t(cuda, a, grad=True):
    return torch.tensor(a, device=cuda, requires_grad=grad)


def _call(cuda, means, quats, scales, opac, colors, cam, **kw):
    import geosplatting_amd as gs
    vm, K = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    ts = [_t(cuda, a) for a in (means, quats, scales, opac, colors)]
    fn = gs.rasterization_3dgs if kw.get("rasterize_mode") == "classic" else gs.rasterization
    kw = dict(kw, means2d_grad=kw.get("means2d_grad", False))
    out = fn(*ts, torch.tensor(vm, device=cuda)[None], torch.tensor(K, device=cuda)[None], cam.width, cam.height, **kw)
    return ts, out


def _check_binning(meta, ref, cam, tile_size=16):
    """ids, radii, intersections, offsets, depths bit-exact against the oracle's A1..A4."""
    W, H = cam.width, cam.height
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    tpg, ids, flat = oracle.isect_tiles(ref["means2d"], ref["radii"], ref["depths"], tile_size, tw, th)
    ids, flat = oracle.sort_pairs(ids, flat)
    off = oracle.isect_offsets(ids, tw * th)
    for key, want in (("gaussian_ids", ref["gaussian_ids"]), ("radii", ref["radii"]), ("tiles_per_gauss", tpg),
                      ("isect_ids", ids), ("flatten_ids", flat)):
        got = meta[key].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), f"{key} not bit-exact"
    assert np.array_equal(meta["isect_offsets"].cpu().numpy().reshape(-1), off)
    assert np.array_equal(meta["depths"].cpu().numpy().view(np.int32), ref["depths"].view(np.int32))
    assert np.array_equal(meta["means2d"].detach().cpu().numpy(), ref["means2d"])
    return off, flat


def _oracle_raster(meta, cam, colors, off, flat, background=None):
    m = lambda k: meta[k].detach().cpu().numpy()
    return oracle.raster_fwd(cam.width, cam.height, 16, m("means2d"), m("conics"), m("opacities"), colors, off, flat, background)


def _check_image(render, alpha, meta, want):
    r_ref, a_ref, last_ref = want[0], want[1], want[2]
    a = alpha[0, ..., 0].detach().cpu().numpy()
    assert np.array_equal(meta["last_ids"][0].cpu().numpy(), last_ref)
    assert np.array_equal(a, a_ref), f"alphas differ on {(a != a_ref).sum()} pixels"
    r = render[0].detach().cpu().numpy()
    assert np.array_equal(r[..., :3], r_ref[..., :3]), f"render differs on {(r[..., :3] != r_ref[..., :3]).sum()} values"
    return r, a


def _upstream(cam, D, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(cam.height, cam.width, D, generator=g) * 2 - 1), (torch.rand(cam.height, cam.width, generator=g) * 2 - 1)


# ---------------------------------------------------------------------------------------------- SH forward
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("full_k", [False, True])
def test_sh_forward(cuda, deg, full_k):
    means, quats, scales, opac, cam = _scene()
    N, K = means.shape[0], (16 if full_k else (deg + 1) ** 2)
    coeffs = _coeffs(N, K, seed=10 + deg)
    _, (render, alpha, meta) = _call(cuda, means, quats, scales, opac, coeffs, cam, sh_degree=deg)
    vm, Km = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    ref = oracle.project_fwd(means, quats, scales, vm, Km, cam.width, cam.height)
    off, flat = _check_binning(meta, ref, cam)
    assert 0 < len(ref["gaussian_ids"]) < N
    gid = ref["gaussian_ids"]
    # colours: within 1e-6 of the float64 SH, [V, 3] in packed order
    c64 = sh_colors64(deg, torch.from_numpy(means[gid]).double(), _campos(vm), torch.from_numpy(coeffs[gid]).double())
    want = torch.clamp_min(c64 + 0.5, 0.0).numpy()
    got = meta["colors"].cpu().numpy()
    assert got.shape == (len(gid), 3)
    assert rel_err(got, want) < 1e-6, rel_err(got, want)
    assert (got[want == 0] == 0).all()
    # the compositor on those colours: bit-identical to the oracle's
    _check_image(render, alpha, meta, _oracle_raster(meta, cam, got, off, flat))
    # antialiased (the default): opacities still carry the compensation
    assert rel_err(meta["opacities"].cpu().numpy(), opac[gid] * ref["compensations"]) < 1e-6


def test_sh_forward_rgb_ed(cuda):
    """RGB+ED with SH colours: four composited channels (the colours_packed path instead of the per-visible records)."""
    means, quats, scales, opac, cam = _scene(seed=4)
    coeffs = _coeffs(means.shape[0], 16, seed=31)
    _, (render, alpha, meta) = _call(cuda, means, quats, scales, opac, coeffs, cam, sh_degree=3, render_mode="RGB+ED")
    assert render.shape == (1, cam.height, cam.width, 4)
    ref = oracle.project_fwd(means, quats, scales, cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy(), cam.width, cam.height)
    off, flat = _check_binning(meta, ref, cam)
    cols = np.concatenate([meta["colors"].cpu().numpy(), ref["depths"][:, None]], 1)
    want = _oracle_raster(meta, cam, cols, off, flat)
    r, a = _check_image(render, alpha, meta, want)
    ed = want[0][..., 3] / np.maximum(want[1], np.float32(1e-10))
    assert np.array_equal(r[..., 3], ed.astype(np.float32))
    # and the same colours as the RGB call
    _, (_, _, meta_rgb) = _call(cuda, means, quats, scales, opac, coeffs, cam, sh_degree=3)
    assert torch.equal(meta_rgb["colors"], meta["colors"])


# ---------------------------------------------------------------------------------------------- SH backward
def _expected_sh_grads(means, quats, scales, opac, coeffs, cam, meta, deg, vr, va, classic=False):
    """Oracle A6 + A7 plus the float64 SH chain: expected (v_means, v_quats, v_scales, v_opacities, v_coeffs)."""
    m = lambda k: meta[k].detach().cpu().numpy()
    vm, Km = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    gid = m("gaussian_ids")
    v_m2d, v_con, v_col, v_op = _raster_bwd(meta, cam, vr, va)
    v_op_proj = np.zeros_like(v_op) if classic else v_op
    g = oracle.project_bwd(means, quats, scales, opac, vm, Km, cam.width, cam.height, gid, m("conics"), m("compensations"),
                           v_m2d, v_con, v_op_proj, v_col)
    v_opac = g[3].copy()
    if classic:
        v_opac[gid] += v_op
    mu = torch.from_numpy(means[gid]).double().requires_grad_(True)
    co = torch.from_numpy(coeffs[gid]).double().requires_grad_(True)
    rgb = torch.clamp_min(sh_colors64(deg, mu, _campos(vm), co) + 0.5, 0.0)
    (rgb * torch.from_numpy(v_col).double()).sum().backward()
    v_means = g[0].astype(np.float64)
    if mu.grad is not None:                                        # (degree 0: the colour does not depend on the direction)
        v_means[gid] += mu.grad.numpy()
    v_coeffs = np.zeros(coeffs.shape, np.float64)
    v_coeffs[gid] = co.grad.numpy()
    return dict(v_means=v_means, v_quats=g[1], v_scales=g[2], v_opacities=v_opac, v_colors=v_coeffs), v_m2d


def _raster_bwd(meta, cam, vr, va):
    m = lambda k: meta[k].detach().cpu().numpy()
    return oracle.raster_bwd(cam.width, cam.height, 16, m("means2d"), m("conics"), m("opacities"), meta["_colors_np"],
                             m("isect_offsets").reshape(-1), m("flatten_ids"), meta["_alpha"], m("last_ids")[0], vr, va)


def _compare_grads(ts, want, scales):
    names = ("v_means", "v_quats", "v_scales", "v_opacities", "v_colors")
    for name, t in zip(names, ts):
        got, w = t.grad.cpu().numpy().astype(np.float64), want[name]
        scale = np.abs(w).max()
        if name == "v_quats":
            scale = max(scale, np.abs(want["v_scales"] * scales).max())
        e = float(np.abs(got - w).max() / (scale + 1e-30))
        assert e < GRAD_TOL, f"{name}: rel err {e:.3e}"


def _run_backward(cuda, deg, K, classic, seed, inside=True):
    means, quats, scales, opac, cam = _scene(seed=seed, inside=inside)
    N = means.shape[0]
    coeffs = _coeffs(N, K, seed=seed + 100)
    kw = dict(sh_degree=deg, rasterize_mode="classic" if classic else "antialiased")
    ts, (render, alpha, meta) = _call(cuda, means, quats, scales, opac, coeffs, cam, **kw)
    vr, va = _upstream(cam, 3, seed)
    (render[0] * vr.to(cuda)).sum().add((alpha[0, ..., 0] * va.to(cuda)).sum()).backward()
    meta = dict(meta, _alpha=alpha[0, ..., 0].detach().cpu().numpy(), _colors_np=meta["colors"].cpu().numpy())
    want, _ = _expected_sh_grads(means, quats, scales, opac, coeffs, cam, meta, deg, vr.numpy(), va.numpy(), classic)
    _compare_grads(ts, want, scales)
    return ts, meta, coeffs, means, cam


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_backward(cuda, deg):
    ts, meta, coeffs, means, cam = _run_backward(cuda, deg, 16, False, seed=40 + deg)
    g = ts[4].grad.cpu().numpy()
    gid = meta["gaussian_ids"].cpu().numpy()
    nb = (deg + 1) ** 2
    assert (g[:, nb:, :] == 0).all(), "inactive coefficients must get exactly 0"
    invisible = np.setdiff1d(np.arange(means.shape[0]), gid)
    assert len(invisible) > 0 and (g[invisible] == 0).all(), "culled Gaussians must get exactly 0"
    c64 = sh_colors64(deg, torch.from_numpy(means[gid]).double(), _campos(cam.view_matrix.numpy()),
                      torch.from_numpy(coeffs[gid]).double()).numpy()
    clamped = c64 + 0.5 < 0
    assert clamped[:, 0].sum() > 10
    assert (g[gid][clamped[:, None, :].repeat(16, 1)] == 0).all(), "clamped channels must get exactly 0"
    assert np.abs(g[gid][:, :nb][~clamped[:, None, :].repeat(nb, 1)]).max() > 0


def test_sh_backward_exact_k(cuda):
    """K = (d+1)^2 rows (27 floats per row at degree 2: the unaligned row path) from outside the cloud."""
    _run_backward(cuda, 2, 9, False, seed=51, inside=False)


# ---------------------------------------------------------------------------------------------- classic
@pytest.mark.parametrize("sh", [False, True])
def test_classic(cuda, sh):
    means, quats, scales, opac, cam = _scene(seed=61)
    N = means.shape[0]
    vm, Km = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    colors = _coeffs(N, 16, seed=62) if sh else torch.rand(N, 3, generator=torch.Generator().manual_seed(63)).numpy()
    kw = dict(rasterize_mode="classic", sh_degree=3 if sh else None)
    ts, (render, alpha, meta) = _call(cuda, means, quats, scales, opac, colors, cam, **kw)
    ref = oracle.project_fwd(means, quats, scales, vm, Km, cam.width, cam.height)
    off, flat = _check_binning(meta, ref, cam)
    gid = ref["gaussian_ids"]
    assert np.array_equal(meta["opacities"].cpu().numpy(), opac[gid]), "classic: opacities[gaussian_ids], no compensation"
    assert not np.array_equal(ref["compensations"], np.ones_like(ref["compensations"]))
    cols = meta["colors"].cpu().numpy() if sh else colors[gid]
    _check_image(render, alpha, meta, _oracle_raster(meta, cam, cols, off, flat))
    vr, va = _upstream(cam, 3, 64)
    (render[0] * vr.to(cuda)).sum().add((alpha[0, ..., 0] * va.to(cuda)).sum()).backward()
    meta = dict(meta, _alpha=alpha[0, ..., 0].detach().cpu().numpy(), _colors_np=cols)
    if sh:
        want, _ = _expected_sh_grads(means, quats, scales, opac, colors, cam, meta, 3, vr.numpy(), va.numpy(), classic=True)
    else:
        v_m2d, v_con, v_col, v_op = _raster_bwd(meta, cam, vr.numpy(), va.numpy())
        m = lambda k: meta[k].detach().cpu().numpy()
        g = oracle.project_bwd(means, quats, scales, opac, vm, Km, cam.width, cam.height, gid, m("conics"), m("compensations"),
                               v_m2d, v_con, np.zeros_like(v_op), v_col)
        v_opac = g[3].copy()
        v_opac[gid] += v_op
        want = dict(v_means=g[0], v_quats=g[1], v_scales=g[2], v_opacities=v_opac, v_colors=g[4])
    _compare_grads(ts, want, scales)


# ---------------------------------------------------------------------------------------------- means2d_grad
@pytest.fixture
def replay_v_packed(monkeypatch):
    """The compositor's backward sums with float atomics, so two runs differ in the last bits; this replays the first run's
    v_packed bytes in the second so that the projection's backward of the two paths can be compared bit for bit."""
    import sys
    import geosplatting_amd.rasterization  # noqa: F401  (the package re-exports the function under the module's name)
    R = sys.modules["geosplatting_amd.rasterization"]
    orig, rec = R._raster_backward, []

    def wrapped(*a):
        out = orig(*a)
        if rec:
            assert rec[0].shape == out.shape
            return rec[0].clone()
        rec.append(out.clone())
        return out
    monkeypatch.setattr(R, "_raster_backward", wrapped)
    return rec


def test_means2d_grad(cuda, replay_v_packed):
    means, quats, scales, opac, cam = _scene(seed=71)
    N = means.shape[0]
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(72)).numpy()
    vr, va = _upstream(cam, 3, 73)
    loss = lambda r, a: (r[0] * vr.to(cuda)).sum() + (a[0, ..., 0] * va.to(cuda)).sum()
    ts0, (r0, a0, meta0) = _call(cuda, means, quats, scales, opac, colors, cam)
    assert not meta0["means2d"].requires_grad                       # the default keeps today's meta
    loss(r0, a0).backward()
    ts1, (r1, a1, meta1) = _call(cuda, means, quats, scales, opac, colors, cam, means2d_grad=True)
    assert meta1["means2d"].requires_grad and meta1["means2d"].shape == (len(meta1["gaussian_ids"]), 2)
    assert torch.equal(r0, r1) and torch.equal(a0, a1) and torch.equal(meta0["means2d"], meta1["means2d"].detach())
    meta1["means2d"].retain_grad()
    loss(r1, a1).backward()
    for t0, t1 in zip(ts0, ts1):
        assert torch.equal(t0.grad, t1.grad), "means2d_grad=True must not change a bit of the parameter gradients"
    m = dict(meta1, _alpha=a1[0, ..., 0].detach().cpu().numpy(), _colors_np=colors[meta1["gaussian_ids"].cpu().numpy()])
    v_m2d, v_con, v_col, v_op = _raster_bwd(m, cam, vr.numpy(), va.numpy())
    assert rel_err(meta1["means2d"].grad.cpu().numpy(), v_m2d) < GRAD_TOL

    # a loss term of the caller's own on means2d reaches v_means through the projection's backward
    replay_v_packed.clear()
    ts2, (r2, a2, meta2) = _call(cuda, means, quats, scales, opac, colors, cam, means2d_grad=True)
    w = torch.randn(meta2["means2d"].shape, generator=torch.Generator().manual_seed(74)) * float(0.5 * np.abs(v_m2d).max())
    (loss(r2, a2) + (meta2["means2d"] * w.to(cuda)).sum()).backward()
    vm, Km = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    mm = lambda k: meta2[k].detach().cpu().numpy()
    g = oracle.project_bwd(means, quats, scales, opac, vm, Km, cam.width, cam.height, mm("gaussian_ids"), mm("conics"),
                           mm("compensations"), v_m2d + w.numpy(), v_con, v_op, v_col)
    e = rel_err(ts2[0].grad.cpu().numpy(), g[0])
    assert e < GRAD_TOL, e
    assert rel_err(ts2[0].grad.cpu().numpy(), ts1[0].grad.cpu().numpy()) > 10 * GRAD_TOL   # the extra term is really there


def test_means2d_grad_gsplatter_config_bit_identical(cuda, replay_v_packed):
    """sh_degree=3, classic, RGB+ED: the two-node path gives the same bits as the fused node."""
    means, quats, scales, opac, cam = _scene(seed=81)
    coeffs = _coeffs(means.shape[0], 16, seed=82)
    kw = dict(sh_degree=3, rasterize_mode="classic", render_mode="RGB+ED")
    vr, va = _upstream(cam, 4, 83)
    grads = []
    for m2g in (False, True):
        ts, (r, a, meta) = _call(cuda, means, quats, scales, opac, coeffs, cam, means2d_grad=m2g, **kw)
        assert meta["means2d"].requires_grad == m2g
        ((r[0] * vr.to(cuda)).sum() + (a[0, ..., 0] * va.to(cuda)).sum()).backward()
        grads.append([t.grad for t in ts])
    for g0, g1 in zip(*grads):
        assert torch.equal(g0, g1)


def test_means2d_grad_only_means2d_in_loss(cuda):
    """A loss on means2d alone (the image unused): the projection's backward runs without the compositor's."""
    means, quats, scales, opac, cam = _scene(seed=91)
    colors = torch.rand(means.shape[0], 3, generator=torch.Generator().manual_seed(92)).numpy()
    ts, (r, a, meta) = _call(cuda, means, quats, scales, opac, colors, cam, means2d_grad=True)
    meta["means2d"].sum().backward()
    vm, Km = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    mm = lambda k: meta[k].detach().cpu().numpy()
    V = len(mm("gaussian_ids"))
    z = np.zeros
    g = oracle.project_bwd(means, quats, scales, opac, vm, Km, cam.width, cam.height, mm("gaussian_ids"), mm("conics"),
                           mm("compensations"), np.ones((V, 2), np.float32), z((V, 3), np.float32), z(V, np.float32), z((V, 3), np.float32))
    assert rel_err(ts[0].grad.cpu().numpy(), g[0]) < GRAD_TOL
    assert (ts[4].grad == 0).all()


# ---------------------------------------------------------------------------------------------- error behaviour
def test_error_behaviour_3dgs(cuda):
    import geosplatting_amd as gs
    z = torch.zeros(1, 3, device=cuda)
    args = (z, torch.ones(1, 4, device=cuda), z + 1, torch.ones(1, device=cuda), z, torch.eye(4, device=cuda)[None],
            torch.eye(3, device=cuda)[None], 16, 16)
    with pytest.raises(NotImplementedError):
        gs.rasterization(*args, rasterize_mode="classic")             # GeoSplatting's entry point: 'antialiased' only
    gs.rasterization_3dgs(*args)                                       # GSplatter's: 'classic' is the default
    gs.rasterization_3dgs(*args, rasterize_mode="antialiased")
    for fn in (gs.rasterization, gs.rasterization_3dgs):
        with pytest.raises(ValueError):
            fn(*args, render_mode="bogus")
        with pytest.raises(ValueError):
            fn(z, torch.ones(1, 4, device=cuda), z + 1, torch.ones(1, device=cuda), z,
               torch.eye(4, device=cuda).repeat(2, 1, 1), torch.eye(3, device=cuda).repeat(2, 1, 1), 16, 16)
    with pytest.raises(ValueError):
        gs.rasterization_3dgs(*args, rasterize_mode="2dgs")
    sh = torch.zeros(1, 16, 3, device=cuda)
    a = args[:4] + (sh,) + args[5:]
    for fn in (gs.rasterization, gs.rasterization_3dgs):
        with pytest.raises(NotImplementedError):
            fn(*args[:4], torch.zeros(1, 25, 3, device=cuda), *args[5:], sh_degree=4)
        with pytest.raises(ValueError):
            fn(*args[:4], torch.zeros(1, 8, 3, device=cuda), *args[5:], sh_degree=2)   # K < 9
        with pytest.raises(ValueError):
            fn(*args, sh_degree=1)                                     # colours [N, 3] with a degree
        fn(*a, sh_degree=3)
        fn(*a, sh_degree=3, render_mode="D")                           # colours ignored in the depth-only modes


def test_rasterization_3dgs_defaults(cuda):
    """rasterization_3dgs defaults to 'classic' and a graph means2d; equal to the explicit call of the same configuration."""
    import geosplatting_amd as gs
    means, quats, scales, opac, cam = _scene(seed=95)
    coeffs = _coeffs(means.shape[0], 16, seed=96)
    ts = [_t(cuda, x) for x in (means, quats, scales, opac, coeffs)]
    cams = (torch.tensor(cam.view_matrix.numpy(), device=cuda)[None], torch.tensor(cam.intrinsic_matrix.numpy(), device=cuda)[None])
    r, a, meta = gs.rasterization_3dgs(*ts, *cams, cam.width, cam.height, sh_degree=3)
    assert meta["means2d"].requires_grad
    gid = meta["gaussian_ids"].cpu().numpy()
    assert np.array_equal(meta["opacities"].detach().cpu().numpy(), opac[gid])
    _, (r2, a2, meta2) = _call(cuda, means, quats, scales, opac, coeffs, cam, sh_degree=3, rasterize_mode="classic")
    assert torch.equal(r, r2) and torch.equal(a, a2) and torch.equal(meta["colors"], meta2["colors"])


# ---------------------------------------------------------------------------------------------- a GSplatter-shaped loop
def test_gsplatter_training_loop(cuda):
    """GSplatter + GSplatTrainer in miniature (rfstudio/model/gsplat.py:188-282, :361-374): SH degree ramp 1 -> 3, classic mode,
    random background, L1 against a target from perturbed parameters, Adam, and the densification statistics read from
    info["means2d"].grad."""
    import geosplatting_amd.synthetic as syn
    from geosplatting_amd.cameras import Camera, lookat_c2w
    from geosplatting_amd.shading import render_rgb
    n = 2000
    sp = syn.random_splats(n, seed=101)
    g = torch.Generator().manual_seed(102)
    c2w = lookat_c2w(torch.tensor([0.0, 0.4, 3.0]), torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0]))
    cam = Camera(c2w, 150.0, 150.0, 64.0, 64.0, 128, 128)
    shs0 = torch.randn(n, 15, 3, generator=g) * 0.1
    base = dict(means=sp.means, scales=sp.scales, quats=sp.quats, opacities=sp.opacities + 2.0, colors=sp.colors, shs=shs0)
    target_p = {k: (v + 0.05 * torch.randn(v.shape, generator=g)).to(cuda) for k, v in base.items()}
    params = {k: v.clone().to(cuda).requires_grad_(True) for k, v in base.items()}
    opt = torch.optim.Adam(params.values(), lr=5e-3)
    xys_grad_norm = torch.zeros(n, device=cuda)
    vis_counts = torch.ones(n, device=cuda)
    losses = []
    for step in range(50):
        deg = 1 + min(step // 17, 2)
        bg = torch.rand(3, generator=g).to(cuda)
        with torch.no_grad():
            target = render_rgb(target_p["means"], target_p["scales"], target_p["quats"], target_p["opacities"], target_p["colors"],
                                cam, bg, shs=target_p["shs"], sh_degree=deg, rasterize_mode="classic")
        rgb, info = render_rgb(params["means"], params["scales"], params["quats"], params["opacities"], params["colors"], cam, bg,
                               shs=params["shs"], sh_degree=deg, rasterize_mode="classic",
                               means2d_grad=True, return_meta=True)
        assert info["means2d"].requires_grad
        info["means2d"].retain_grad()
        loss = (rgb - target).abs().mean()
        opt.zero_grad()
        loss.backward()
        with torch.no_grad():                                          # GSplatter.update_grad_norm
            grads = info["means2d"].grad.norm(dim=-1)
            vis_counts[info["gaussian_ids"]] += 1
            xys_grad_norm[info["gaussian_ids"]] += grads
        opt.step()
        assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in params.values())
        losses.append(float(loss.detach()))
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:5]), losses
    seen = vis_counts > 1
    assert seen.sum() > n // 4
    assert (xys_grad_norm[seen] > 0).float().mean() > 0.5         # (occluded or faint Gaussians get no gradient)
    assert (xys_grad_norm[~seen] == 0).all()
