"""The Monte-Carlo environment shader on the GPU (csrc/gs_envshade.hip, geosplatting_amd/envshade.py) against its own sample log,
against the shipped ray queries and against the float64 restatement of tests/envshade_ref.py.  Every case runs with
return_samples=True; the budgets and the fragile masks are the restatement's (derived in its docstring, nothing tuned here).

  * exact: the logged visibility equals 1 - MeshBVH.occluded of the logged directions bit for bit, with the node buffer and by brute
    force; the same seed gives the same bits; [1,1,N,.] inputs give the bits of the flat form; a point whose lit samples are all
    occluded scales by shadow_scale exactly; splat_mc equals its hand-composed pipeline bit for bit.
  * against float64, on samples / points the restatement does not mark fragile (at most 1 % of the points, asserted): directions,
    pdf sums, the three outputs (at the kernel's own logged samples, and end to end), the five gradients.

Measured on an MI355X (largest error / budget over all cases, as the tests print it): directions 0.23, pdf sums 0.50; outputs at the
kernel's own log 0.07 (diff), 0.20 (spec), 0.32 (resi), end to end 0.05 / 0.04 / 0.07; gradients 0.22 (pos), 0.13 (normal), 0.29 (kd),
0.28 (ks), 0.11 (light), the same for 1, 16 and 64 lanes per point; no point is fragile in any case ("Monte-Carlo environment shader")."""
import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from tests import envshade_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FRAGILE_CAP = 0.01
U24 = 2.0 ** -24
_cache = {}


def _bvh():
    if "bvh" not in _cache:
        v, f = ref.scene_mesh()
        _cache["bvh"] = gs.MeshBVH(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    return _cache["bvh"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(P, map_name, mask=None, grad=False):
    pt, env = ref.points(P), ref.env_map(map_name)
    t = {k: _dev(pt[k]) for k in ("ro", "pos", "nrm", "kd", "ks")}
    light, pdf, rows, cols = (_dev(a) for a in env)
    if grad:
        for k in ("pos", "nrm", "kd", "ks"):
            t[k].requires_grad_(True)
        light.requires_grad_(True)
    m = torch.ones(P, device=DEV) if mask is None else _dev(mask.astype(np.float32))
    return t, (m, t["ro"], t["pos"], t["nrm"], _dev(ref.CAMERA), t["kd"], t["ks"], light, pdf, rows, cols), light


def _run(P, map_name, n, bsdf="pbr", shadow_scale=1.0, seed=ref.SEED, **kw):
    key = (P, map_name, n, bsdf, shadow_scale, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        _, args, _ = _inputs(P, map_name)
        with torch.no_grad():
            out = gs.env_shade(_bvh(), *args, BSDF=bsdf, n_samples_x=n, rnd_seed=seed, shadow_scale=shadow_scale, perms=_dev(ref.perms(n)),
                               return_samples=True, **kw)
        _cache[key] = dict(zip(("diff", "spec", "resi", "dirs", "pdf_sum", "vis"), (o.cpu().numpy() for o in out)), raw=out)
    return _cache[key]


def _check(name, got, want, budget, keep, worst):
    """|got - want| <= budget on the rows `keep`; records the largest error / budget"""
    err = np.abs(got.astype(np.float64) - want)
    sel = np.broadcast_to(keep.reshape(keep.shape + (1,) * (err.ndim - keep.ndim)), err.shape)
    ratio = np.where(sel & (err > 0), err / np.maximum(budget, 1e-300), 0.0)
    worst[name] = max(worst.get(name, 0.0), float(ratio.max(initial=0.0)))
    assert np.isfinite(got).all(), name
    assert (ratio <= 1.0).all(), (name, float(ratio.max()), np.argwhere(ratio > 1.0)[:5].tolist())


@pytest.mark.parametrize("P,map_name,n", ref.CASES)
def test_logged_visibility_is_the_shipped_any_hit(P, map_name, n):
    g = _run(P, map_name, n)
    ro, dirs = _dev(ref.points(P)["ro"]), g["raw"][3]
    for brute in (False, True):
        occ = _bvh().occluded(ro, dirs, tmin=0.0, tmax=1e16, brute_force=brute)
        assert torch.equal(g["raw"][5], 1.0 - occ.float())
    assert 0.0 < g["vis"].mean() < 1.0 or P == 1                                      # lit and shadowed samples both occur


@pytest.mark.parametrize("P,map_name,n", ref.CASES)
def test_sample_log_against_float64(P, map_name, n):
    g = _run(P, map_name, n)
    pt, env = ref.points(P), ref.env_map(map_name)
    smp, exp = ref.expected(P, map_name, n)
    worst = {}
    ok = ~smp["fragile"]
    _check("dirs", g["dirs"], smp["dirs"], smp["budget"][..., None] + 0.0 * smp["dirs"], ok, worst)
    # the pdf sum and the visibility at the kernel's own logged directions
    psum, pbud, pfrag, _ = ref.pdf_sums(pt, env, smp, g["dirs"].astype(np.float64))
    vis, rfrag = ref.visibility(pt, g["dirs"])
    _check("pdf_sum", g["pdf_sum"], psum, pbud, ok & ~pfrag, worst)
    assert np.array_equal(g["vis"][~rfrag], vis[~rfrag])
    # a light sample lands in the texel that the exact search selected -- every one of them, up to the rounding of its direction
    H, W = env[1].shape
    d = g["dirs"][:, 0::2].astype(np.float64)
    u = (np.arctan2(d[..., 0], -d[..., 2]) / (2.0 * np.pi) + 0.5) * W
    v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi * H
    x, y = smp["texel"][..., 0], smp["texel"][..., 1]
    sin_t = np.maximum(np.sqrt(np.maximum(1.0 - d[..., 1] ** 2, 0.0)), 1e-4)
    slack = (ref.DIR_LIGHT + 8.0) * U24 / sin_t                                       # an angle moves by the direction's error / sin(theta)
    outside = lambda c, lo: np.abs(c - np.clip(c, lo, lo + 1))
    du = np.minimum(np.minimum(outside(u, x), outside(u - W, x)), outside(u + W, x))  # (the map wraps in u)
    assert (du <= slack * W).all() and (outside(v, y) <= slack * H).all()
    share = float((smp["fragile"] | pfrag | rfrag).any(1).mean())
    print(f"P={P} {map_name} n={n}: fragile points {100 * share:.2f} %, worst error / budget {worst}")
    assert share <= FRAGILE_CAP


@pytest.mark.parametrize("bsdf", ref.BSDFS)
@pytest.mark.parametrize("P,map_name,n", ref.CASES[:4])
def test_outputs_against_float64(P, map_name, n, bsdf):
    g = _run(P, map_name, n, bsdf)
    pt, env = ref.points(P), ref.env_map(map_name)
    smp, _ = ref.expected(P, map_name, n)
    worst = {}
    # (a) the shading arithmetic alone: the restatement at the kernel's own logged directions and visibilities
    at = ref.shade(pt, env, smp, g["dirs"].astype(np.float64), g["vis"].astype(np.float64), bsdf, 1.0, n)
    keep = ~at["fragile"]
    for k in ("diff", "spec", "resi"):
        _check(k + " at the log", g[k], at[k], at[k + "_budget"], keep, worst)
    # (b) end to end: the restatement's own samples and its own visibility
    _, base = ref.expected(P, map_name, n, bsdf)
    slack = ref.direction_slack(pt, env, smp, base["vis"], bsdf, 1.0, n, base)
    keep2 = ~base["fragile"] & keep
    for k in ("diff", "spec", "resi"):
        _check(k + " end to end", g[k], base[k], base[k + "_budget"] + slack[k], keep2, worst)
    share = float((~keep2).mean())
    print(f"P={P} {map_name} n={n} {bsdf}: fragile points {100 * share:.2f} %, worst error / budget {worst}")
    assert share <= FRAGILE_CAP
    if bsdf != "pbr":
        assert not g["spec"].any() and not g["resi"][:, 1].any()


@pytest.mark.parametrize("lanes", (1, 16, 64))
def test_every_arrangement_within_budget(lanes):
    """The lanes of a point share its iterations in groups of 1, 16 or 64 (the default depends on n): the same samples, another order
    of the per-point sums -- each within the same budgets, forward and backward."""
    P, map_name, n = ref.CASES[0]
    g = _run(P, map_name, n, lanes_per_point=lanes)
    base = _run(P, map_name, n)
    assert np.array_equal(g["dirs"], base["dirs"]) and np.array_equal(g["pdf_sum"], base["pdf_sum"]) and np.array_equal(g["vis"], base["vis"])
    pt, env = ref.points(P), ref.env_map(map_name)
    smp, _ = ref.expected(P, map_name, n)
    rng = np.random.default_rng(6)
    d_diff, d_spec = rng.normal(size=(P, 3)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32)
    at = ref.shade(pt, env, smp, g["dirs"].astype(np.float64), g["vis"].astype(np.float64), "pbr", 1.0, n, d_diff=d_diff, d_spec=d_spec)
    worst = {}
    for k in ("diff", "spec", "resi"):
        _check(k, g[k], at[k], at[k + "_budget"], ~at["fragile"], worst)
    t, args, light = _inputs(P, map_name, grad=True)
    out = gs.env_shade(_bvh(), *args, n_samples_x=n, rnd_seed=ref.SEED, perms=_dev(ref.perms(n)), lanes_per_point=lanes, merge_rounds=lanes % 3)
    (out[0] * _dev(d_diff) + out[1] * _dev(d_spec)).sum().backward()
    for k in ("pos", "nrm", "kd", "ks"):
        _check("d_" + k, t[k].grad.cpu().numpy(), at["d_" + k], at["d_" + k + "_budget"], ~at["fragile_grad"], worst)
    clear = np.ones(env[1].size, bool)
    clear[at["texel"][at["fragile_grad"]]] = False
    _check("d_light", light.grad.cpu().numpy(), at["d_light"], at["d_light_budget"], clear.reshape(env[1].shape), worst)
    print(f"lanes_per_point={lanes}: worst error / budget {worst}")


@pytest.mark.parametrize("bsdf", ("pbr", "diffuse"))
@pytest.mark.parametrize("P,map_name,n", ref.CASES[:3])
def test_gradients_against_float64_autograd(P, map_name, n, bsdf):
    rng = np.random.default_rng(5)
    mask = np.ones(P, np.float32)
    if P > 1:
        mask[3::7] = 0.0
        mask[5] = -1.0
    d_diff, d_spec = rng.normal(size=(P, 3)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32)
    t, args, light = _inputs(P, map_name, mask=mask, grad=True)
    out = gs.env_shade(_bvh(), *args, BSDF=bsdf, n_samples_x=n, rnd_seed=ref.SEED, perms=_dev(ref.perms(n)), return_samples=True)
    assert not out[2].requires_grad
    (out[0] * _dev(d_diff) + out[1] * _dev(d_spec)).sum().backward()
    live = mask > 0
    for o in out[:3]:
        assert not o[~_dev(live)].any()                                               # masked rows: zero outputs ...
    for k in ("pos", "nrm", "kd", "ks"):
        assert not t[k].grad[~_dev(live)].any()                                       # ... and zero gradients
    pt = dict(ref.points(P), mask=mask)
    env = ref.env_map(map_name)
    smp, _ = ref.expected(P, map_name, n)
    dirs = np.where(live[:, None, None], out[3].detach().cpu().numpy().astype(np.float64), smp["dirs"])
    vis = out[5].detach().cpu().numpy().astype(np.float64)
    at = ref.shade(pt, env, smp, dirs, vis, bsdf, 1.0, n, d_diff=d_diff, d_spec=d_spec)
    keep = ~at["fragile_grad"] & live
    worst = {}
    for k in ("pos", "nrm", "kd", "ks"):
        _check("d_" + k, t[k].grad.cpu().numpy(), at["d_" + k], at["d_" + k + "_budget"], keep, worst)
    # light_grad per texel; the texels a fragile or masked point adds to are left out, the masked points add nothing
    touched = np.zeros(env[0].shape[:2], bool).reshape(-1)
    touched[at["texel"][at["fragile_grad"] & live]] = True
    _check("d_light", light.grad.cpu().numpy(), at["d_light"] * (~touched.reshape(env[0].shape[:2]))[..., None],
           at["d_light_budget"], ~touched.reshape(env[0].shape[:2]), worst)
    share = float(at["fragile_grad"][live].mean())
    print(f"P={P} {map_name} n={n} {bsdf}: fragile points {100 * share:.2f} %, worst error / budget {worst}")
    assert share <= FRAGILE_CAP
    if bsdf == "diffuse":
        assert not t["kd"].grad.any() and not t["ks"].grad.any() and not t["pos"].grad.any()


def test_determinism_and_seeds():
    P, map_name, n = ref.CASES[0]
    a = _run(P, map_name, n)
    _, args, _ = _inputs(P, map_name)
    kw = dict(n_samples_x=n, perms=_dev(ref.perms(n)), return_samples=True)
    with torch.no_grad():
        b = gs.env_shade(_bvh(), *args, rnd_seed=ref.SEED, **kw)
        c = gs.env_shade(_bvh(), *args, rnd_seed=ref.SEED + 1, **kw)
    for x, y in zip(a["raw"], b):
        assert torch.equal(x, y)                                                      # the same seed: the same bits, log included
    assert not torch.equal(a["raw"][0], c[0]) and not torch.equal(a["raw"][3], c[3])
    # an explicit seed is the backward's seed too: a backward after it leaves a second forward's log unchanged, and its light_grad
    # lands only on texels of the logged directions
    t, args, light = _inputs(P, map_name, grad=True)
    out = gs.env_shade(_bvh(), *args, rnd_seed=ref.SEED, **kw)
    (out[0].sum() + out[1].sum()).backward()
    with torch.no_grad():
        again = gs.env_shade(_bvh(), *args, rnd_seed=ref.SEED, **kw)
    assert torch.equal(out[3], again[3]) and torch.equal(out[5], again[5])
    env = ref.env_map(map_name)
    _, tx, ty, _, _ = ref.light_pdf(env, a["dirs"].astype(np.float64))
    seen = np.zeros(env[1].shape, bool)
    seen[ty, tx] = True
    assert not light.grad.cpu().numpy()[~seen].any() and light.grad.cpu().numpy()[seen].any()
    # the arrangements differ in the order of the per-point sums only: the sample log is the same
    for lanes in (1, 16, 64):
        with torch.no_grad():
            o = gs.env_shade(_bvh(), *args, rnd_seed=ref.SEED, lanes_per_point=lanes, **kw)
        assert torch.equal(o[3], a["raw"][3]) and torch.equal(o[4], a["raw"][4]) and torch.equal(o[5], a["raw"][5])
        assert torch.allclose(o[0], a["raw"][0], rtol=1e-4, atol=1e-6)


def test_shadow_scale_is_exact_on_a_fully_shadowed_point():
    """A point whose every non-zero sample is occluded: V = 1 - shadow_scale on all of them, so shadow_scale = 0.5 gives
    0.5 x the shadow_scale = 0 result bit for bit (a power of two commutes with every rounding; the terms are far from underflow)."""
    P, map_name, n = ref.CASES[0]
    full, half = _run(P, map_name, n, shadow_scale=0.0), _run(P, map_name, n, shadow_scale=0.5)
    # chosen from the log: every sample that can have a non-zero term (n . wi > 0; taken with a margin far above the rounding of the dot
    # product, so the kernel's own sign agrees) is occluded
    facing = (full["dirs"].astype(np.float64) * ref.points(P)["nrm"].astype(np.float64)[:, None]).sum(-1) > -1e-4
    dark = np.where(~(facing & (full["vis"] > 0)).any(1) & (full["diff"].min(-1) > 1e-6))[0]
    assert dark.size > 0
    assert np.array_equal(full["vis"], half["vis"])
    assert np.array_equal(half["diff"][dark], 0.5 * full["diff"][dark]) and np.array_equal(half["spec"][dark], 0.5 * full["spec"][dark])
    assert full["diff"][dark].min() > 1e-6
    assert not full["resi"][dark].any() and half["resi"][dark, 0].min() > 0           # the residual is the shadowed share


def _splat_scene():
    v, f = ref.scene_mesh()
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    sp, nrm = gs.mesh_to_splats(vt, ft, gs.vertex_normals(vt, ft))
    g = torch.Generator().manual_seed(2)
    N = sp.means.shape[0]
    leaves = dict(kd=torch.rand(N, 3, generator=g), ks=torch.rand(N, 2, generator=g), occ=torch.randn(N, 6, generator=g) + 3.0)
    light = _dev(ref.env_map("16x32")[0])
    c2w = gs.lookat_c2w(torch.tensor([0.3, 0.4, 3.0]), torch.zeros(3), torch.tensor([0.0, 1.0, 0.0]))
    cam = gs.Camera(c2w.contiguous().to(DEV), 60.0, 60.0, 32.0, 32.0, 64, 64)
    return sp, nrm, {k: x.to(DEV) for k, x in leaves.items()}, light, cam


@pytest.mark.parametrize("mode", ("pbr", "diffuse", "specular"))
def test_splat_mc_equals_its_pipeline(mode):
    sp, nrm, lv, light, cam = _splat_scene()
    env = gs.LatLngEnvMap(light).compute_pdf_()
    exposure = torch.tensor(1.3, device=DEV)
    attrs = gs.RenderableAttrs(kd=lv["kd"], ks=lv["ks"], normals=nrm, occ=lv["occ"])
    kw = dict(bvh=_bvh(), exposure=exposure, positions=sp.means, envmap=env, min_roughness=0.1, max_metallic=0.9, mode=mode,
              num_samples_per_ray=2, rnd_seed=7)
    with torch.no_grad():
        img, reg = attrs.splat_mc(sp, [cam], **kw)
        assert reg == 0 and img.shape == (64, 64, 4)
        # by hand
        lookat, cam_pos = -cam.c2w[:, 2], cam.c2w[:, 3]
        n = torch.where((nrm * lookat).sum(-1, keepdim=True) > 1e-3, -nrm, nrm)
        rough, metal = lv["ks"][:, :1] * 0.9 + 0.1, lv["ks"][:, 1:] * 0.9
        ks = torch.cat((torch.zeros_like(rough), rough, metal), -1)
        d, s, r = gs.env_shade(_bvh(), torch.ones_like(rough), sp.means + nrm * 1e-5, sp.means, n, cam_pos.contiguous(), lv["kd"], ks, light,
                               *env.tables(), n_samples_x=2, rnd_seed=7)
        d, s = d.clamp_min(1e-4), s.clamp_min(1e-4)
        kdf = lv["kd"] * (1 - metal)
        col = {"pbr": d * kdf + s, "diffuse": d * kdf, "specular": s}[mode]
        want = gs.tone_map(gs.render_rgba(sp.means, sp.scales, sp.quats, sp.opacities, col, cam), exposure, "naive")
        assert torch.equal(img, want) and img[..., 3].max() > 0.5
        with_resi, _ = attrs.splat_mc(sp, [cam], residual=True, **kw)
        assert not torch.equal(with_resi, img) and r.max() > 0


def test_splat_mc_backward_reaches_every_input():
    sp, nrm, lv, light, cam = _splat_scene()
    leaves = {k: x.clone().requires_grad_(True) for k, x in lv.items()}
    light = light.clone().requires_grad_(True)
    normals, positions = nrm.clone().requires_grad_(True), sp.means.clone().requires_grad_(True)
    params = [getattr(sp, k).detach().clone().requires_grad_(True) for k in ("means", "scales", "quats", "opacities")]
    from types import SimpleNamespace
    splats = SimpleNamespace(means=params[0], scales=params[1], quats=params[2], opacities=params[3])
    env = gs.LatLngEnvMap(light).compute_pdf_()
    attrs = gs.RenderableAttrs(kd=leaves["kd"], ks=leaves["ks"], normals=normals, occ=leaves["occ"])
    img, reg = attrs.splat_mc(splats, [cam], bvh=_bvh(), exposure=torch.tensor(1.0, device=DEV), positions=positions, envmap=env,
                              min_roughness=0.1, max_metallic=0.9, num_samples_per_ray=2, residual=True)          # rnd_seed=None
    assert reg == 0
    (img[..., :3].mean() + img[..., 3].mean()).backward()
    for name, x in [("kd", leaves["kd"]), ("ks", leaves["ks"]), ("occ", leaves["occ"]), ("normals", normals), ("positions", positions),
                    ("envmap", light)] + list(zip(("means", "scales", "quats", "opacities"), params)):
        assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0, name
    with pytest.raises(NotImplementedError, match="denoiser"):
        attrs.splat_mc(splats, [cam], bvh=_bvh(), exposure=1.0, positions=positions, envmap=env, min_roughness=0.1, max_metallic=0.9, denoise=True)


def test_shapes_and_the_cached_tables():
    P, map_name, n = ref.CASES[1]
    _, args, _ = _inputs(P, map_name)
    m, ro, pos, nrm, view, kd, ks, *rest = args
    from geosplatting_amd import envshade
    envshade._perm_cache.clear()
    with torch.no_grad():
        flat = gs.env_shade(_bvh(), m, ro, pos, nrm, view, kd, ks, *rest, n_samples_x=n, rnd_seed=3)
        assert list(envshade._perm_cache) == [(n, str(DEV))] and envshade._perm_cache[(n, str(DEV))].shape == (32768, n * n)
        table = envshade._perm_cache[(n, str(DEV))]
        r4 = lambda x: x.view(1, 1, P, -1)
        nested = gs.env_shade(_bvh(), r4(m), r4(ro), r4(pos), r4(nrm), view.view(1, 1, 1, 3), r4(kd), r4(ks), *rest, n_samples_x=n, rnd_seed=3)
    assert envshade._perm_cache[(n, str(DEV))] is table and len(envshade._perm_cache) == 1
    assert [tuple(x.shape) for x in flat] == [(P, 3), (P, 3), (P, 2)] and [tuple(x.shape) for x in nested] == [(1, 1, P, 3), (1, 1, P, 3), (1, 1, P, 2)]
    for a, b in zip(flat, nested):
        assert torch.equal(a, b.view(a.shape))
    assert int(table.min()) == 0 and int(table.max()) == n * n - 1 and torch.equal(table.sort(-1).values[0], torch.arange(n * n, device=DEV, dtype=torch.int32))
