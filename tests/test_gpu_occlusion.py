"""GPU tests of the ambient-occlusion map and of the shaders on it: csrc/gs_ao.hip (geosplatting_amd/occlusion.py), the visibility
modes of csrc/gs_meshshade.hip (shade_pixels / render_mesh with occlusion 'ao' | 'screen') and the Monte-Carlo mesh shader
(geosplatting_amd/meshmc.py).  The float64 restatement tests/ao_ref.py derives every bound from the arithmetic; its scenes' fragile
shares are asserted without a GPU in tests/test_occlusion_cpu.py.

ambient_occlusion   the logged hit flags are MeshBVH.occluded on the same float32 origins and directions built with torch ops, bit for
                    bit; BVH == brute force bit for bit (flags, weights, output); two runs give the same bits; on the non-fragile
                    points the flags equal float64, the weights lie within EPS_C and the output within budget(S, G) for G = 1, 16, 64.
shade_pixels        'ao' and 'screen' against tests/meshshade_ref.py's float64 terms scaled by v = max(visibility, min_visibility), with
                    that file's magnitudes, fragile and ill-conditioned flags and KAPPA_PIXEL; a map of ones gives the bits of 'none',
                    forward and backward ('ao' runs the backward of 'none' and adds the gradient of (v - 1) l_diff diff in a second
                    launch, in which a pixel with v = 1 takes no part); 'screen' equals 'none' x v TO THE LAST BIT: contraction is off in the forward kernel, so the
                    colour of 'none' is fl(c * 1) = c and that of 'screen' is fl(c * v), the product torch forms.
render_mesh         'ao' / 'screen' equal shade_pixels on render_mesh's own maps; the 'ao' map comes back as an output.
render_mesh_mc      equals its pipeline composed by hand bit for bit; the sphere's shadow on the plane; gradients.

The shadow factor.  'vis' = 1 - (denoised shadowed share) is SMALLER inside a shadow.  The factor measured here is
mean('vis' on plane pixels at least two radii from the sphere) / mean('vis' on plane pixels inside the analytic shadow): exactly 1 with
shadow_scale = 0 (nothing is shadowed: 'vis' is 1 everywhere), and asserted above SHADOW_FACTOR_MIN with shadow_scale = 1 (DESIGN.md
section 0 records the measurement the margin comes from).

Measured on an MI355X: ambient_occlusion at most 0.044 of budget(S, G) over every P, S and lane arrangement; shade_pixels forward 0.22,
per-pixel gradients 0.85 of the KAPPA_PIXEL = 8 allowed, texel gradients 0.11 of 1e-4 x magnitude; the shadow factor 1.59."""
import math

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from tests import ao_ref
from tests import meshshade_ref as ms
from tests import raytrace_ref as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHADOW_FACTOR_MIN = 1.25         # measured 1.59 on the MI355X (0.955 / 0.600); 1.25 is about its square root, half way to 1 in ratio

_bvhs = {}


def _bvh(name):
    if name not in _bvhs:
        if name == "sphere":
            v, f = ao_ref.uv_sphere(0.5)
        elif name == "box":
            v, f = ao_ref.closed_box(0.5)
        elif name == "sphere_on_plane":
            v, f, _ = ao_ref.sphere_on_plane()
        else:
            v, f = rr.mesh(name)
        _bvhs[name] = gs.MeshBVH(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    return _bvhs[name]


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


# ------------------------------------------------------------------------------------------------ ambient_occlusion
@pytest.mark.parametrize("S", ao_ref.S_VALUES)
@pytest.mark.parametrize("P", ao_ref.P_VALUES)
def test_ao_bits(P, S):
    """on the bumpy icosphere(3), 1280 faces: the log against MeshBVH.occluded, BVH against brute force, a second run"""
    bvh = _bvh("ico3")
    _, _, pos, nrm, tg = ao_ref.scene(P, S)
    pos, nrm, tg = _dev(pos, nrm, tg)
    o = pos + nrm * ao_ref.OFFSET
    want_hit = bvh.occluded(o, tg[None, :, :] - o[:, None, :], tmin=0.0, tmax=1.0)
    first = None
    for lanes in ao_ref.LANES:
        vis, hit, w = gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=lanes, return_samples=True)
        assert vis.shape == (P,) and hit.shape == (P, S) and w.shape == (P, S)
        assert torch.equal(hit, want_hit), f"lanes {lanes}: the logged hits are not MeshBVH.occluded"
        bvis, bhit, bw = gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=lanes, return_samples=True, brute_force=True)
        assert torch.equal(vis, bvis) and torch.equal(hit, bhit) and torch.equal(w, bw), f"lanes {lanes}: BVH differs from brute force"
        assert torch.equal(vis, gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=lanes)), "the log changes the output"
        assert torch.equal(vis, gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=lanes)), "two runs differ"
        assert bool(((vis >= 0) & (vis <= 1)).all())
        if first is None:
            first = (hit, w)
        assert torch.equal(w, first[1]), "the weights depend on the lane arrangement"
    default = gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET)
    assert torch.equal(default, gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=64 if S >= 64 else 16 if S >= 16 else 1))
    if P >= 67:
        assert float(default[5]) == 0.0                                               # the row with a NaN


@pytest.mark.parametrize("S", ao_ref.S_VALUES)
@pytest.mark.parametrize("P", ao_ref.P_VALUES)
def test_ao_against_float64(P, S):
    want = ao_ref.expected(P, S)
    bvh = _bvh(ao_ref.mesh_for(P))
    _, _, pos, nrm, tg = ao_ref.scene(P, S)
    pos, nrm, tg = _dev(pos, nrm, tg)
    ok = ~want["fragile"]
    assert want["fragile"].sum() <= ao_ref.FRAGILE_CAP * P
    for lanes in ao_ref.LANES:
        vis, hit, w = gs.ambient_occlusion(bvh, pos, nrm, tg, offset=ao_ref.OFFSET, lanes=lanes, return_samples=True)
        vis, hit, w = vis.cpu().numpy().astype(np.float64), hit.cpu().numpy(), w.cpu().numpy().astype(np.float64)
        assert np.array_equal(hit[ok], want["hit"][ok]), "a hit flag of a non-fragile point differs from float64"
        assert np.array_equal((w > 0)[ok], want["counts"][ok])
        err_w = np.abs(w - want["w"])[ok]
        assert np.all(err_w <= want["eps_w"][ok][:, None]), f"weights: {err_w.max():.3g}"
        budget = ao_ref.budget(want, S, lanes)
        err = np.abs(vis - want["vis"])
        ratio = float((err[ok] / budget[ok]).max()) if ok.any() else 0.0
        print(f"P = {P}, S = {S}, lanes = {lanes}: worst |vis - float64| / budget = {ratio:.4f} (budget up to {budget[ok].max():.3g})")
        assert ratio <= 1.0
        assert np.all(vis[~want["finite"]] == 0.0)


def test_ao_known_answers():
    v, f = ao_ref.uv_sphere(0.5)
    tri = v.astype(np.float64)[f]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cen, nrm = _dev(tri.mean(1).astype(np.float32), nrm.astype(np.float32))
    for targets in (None, _dev(ao_ref.scene(67, 130)[4])[0]):
        vis = gs.ambient_occlusion(_bvh("sphere"), cen, nrm, targets)
        assert torch.all(vis == 1.0), "a convex body occludes none of its own front-facing targets"
    floor = torch.tensor([[0.1, -0.2, -0.5], [0.0, 0.0, -0.5], [float("nan"), 0.0, -0.5]], device=DEV)
    up = torch.tensor([[0.0, 0.0, 1.0]], device=DEV).repeat(3, 1)
    vis, hit, w = gs.ambient_occlusion(_bvh("box"), floor, up, None, return_samples=True)
    assert torch.all(vis == 0.0) and bool((w[:2] > 0).any(1).all()) and bool(hit[:2][w[:2] > 0].all())
    assert gs.occlusion.default_ao_targets(DEV).shape == (128, 3)
    assert torch.allclose(gs.occlusion.default_ao_targets(DEV).norm(dim=-1), torch.full((128,), 3.0, device=DEV), atol=1e-5)


def test_face_ambient_occlusion():
    """targets within 37 degrees of the zenith at radius 3: a segment from a plane point two units away rises too steeply to meet the
    sphere of radius 0.5 (it passes its centre at a distance of 0.89 or more), one from under the sphere starts inside its shadow"""
    v, f, n_sphere = ao_ref.sphere_on_plane()
    vt, ft = _dev(v, f)
    rng = np.random.default_rng(12)
    cos_t, phi = rng.uniform(0.8, 1.0, 64), rng.uniform(0.0, 2.0 * np.pi, 64)
    sin_t = np.sqrt(1.0 - cos_t ** 2)
    targets = _dev((3.0 * np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], -1)).astype(np.float32))[0]
    ao = gs.face_ambient_occlusion(vt, ft, targets=targets)
    assert ao.shape == (f.shape[0],) and torch.equal(ao, gs.face_ambient_occlusion(vt, ft, _bvh("sphere_on_plane"), targets))
    assert gs.face_ambient_occlusion(vt, ft).shape == ao.shape                        # the default targets
    cen = torch.from_numpy(v.astype(np.float64)[f].mean(1))
    plane = torch.arange(f.shape[0]) >= n_sphere
    rho = cen[:, :2].norm(dim=-1)
    under, far = plane & (rho < 0.45), plane & (rho > 2.0)
    assert int(under.sum()) >= 2 and int(far.sum()) >= 50
    got = ao.cpu()
    print(f"plane faces under the sphere {got[under].min():.3f} .. {got[under].max():.3f}, far away {got[far].min():.3f} .. {got[far].max():.3f}")
    assert torch.all(got[under] < 1.0) and torch.all(got[far] == 1.0)
    with pytest.raises(ValueError):
        gs.face_ambient_occlusion(vt, ft, _bvh("box"))


# ------------------------------------------------------------------------------------------------ shade_pixels with a visibility map
MIN_VIS = 0.3


def _env(sc, grad=False):
    base = sc["base"].to(DEV).requires_grad_(grad)
    levels = [l.to(DEV).requires_grad_(grad) for l in sc["levels"]]
    return gs.TextureSplitSum(base, levels, ms.MIN_R, ms.MAX_R)


def _rast(sc):
    rast = torch.zeros(sc["H"], sc["W"], 4)
    rast[..., 3] = torch.where(sc["covered"].view(sc["H"], sc["W"]), 5.0, 0.0)
    return rast.to(DEV)


def _vis_map(sc):
    """seeded, in [0, 1], about 30 % below MIN_VIS"""
    return torch.rand(sc["H"], sc["W"], generator=torch.Generator().manual_seed(17 + sc["W"]))


def _run(sc, cot, mode, vis):
    """forward + backward on fresh leaves -> evaluate()-shaped result on the CPU"""
    H, W = sc["H"], sc["W"]
    maps = [sc[k].view(H, W, -1).to(DEV).requires_grad_() for k in ("position", "normal", "uv")]
    kd, ks = gs.Texture2D(sc["kd"].to(DEV).requires_grad_()), gs.Texture2D(sc["ks"].to(DEV).requires_grad_())
    env = _env(sc, grad=True)
    vmap = None if vis is None else vis.to(DEV).requires_grad_()
    color = gs.shade_pixels(*maps, _rast(sc), kd, ks, sc["cam"].to(DEV), env, occlusion=mode, min_visibility=MIN_VIS,
                            bend_back_normal=sc["bend"], visibility=vmap)
    (color * cot.view_as(color).to(DEV)).sum().backward()
    assert vmap is None or vmap.grad is None, "the visibility map received a gradient"
    flat = lambda t: t.grad.cpu().reshape(-1, t.shape[-1])
    return dict(color=color.detach().cpu().reshape(-1, 3),
                grad=dict(position=flat(maps[0]), normal=flat(maps[1]), uv=flat(maps[2]), kd=kd.data.grad.cpu(), ks=ks.data.grad.cpu(),
                          base=env.base.grad.cpu(), levels=[l.grad.cpu() for l in env.levels]))


def _reference(sc, cot, mode, vis, monkeypatch):
    """tests/meshshade_ref.evaluate with its two terms scaled by v: 'ao' the diffuse term alone, 'screen' both"""
    v = vis.reshape(-1)[ms.shaded_mask(sc)].double().clamp(min=MIN_VIS)[:, None]
    plain = ms._terms

    def scaled(position, normal, uv, kd, ks, cam, lut, base, levels, occlusion, min_visibility, bend, hook=None):
        t_diff, t_spec = plain(position, normal, uv, kd, ks, cam, lut, base, levels, "none", 0.0, bend, hook)
        vv = v.to(t_diff.dtype)
        return t_diff * vv, (t_spec * vv if mode == "screen" else t_spec)

    monkeypatch.setattr(ms, "_terms", scaled)
    try:
        return ms.evaluate(sc, cot, torch.float64)
    finally:
        monkeypatch.setattr(ms, "_terms", plain)


@pytest.mark.parametrize("mode", ["ao", "screen"])
@pytest.mark.parametrize("name", ["1x1", "37x53 textured", "64x64 none"])
def test_shade_with_visibility(name, mode, monkeypatch):
    sc = ms.scene(name)
    cot, _ = ms.reference(name, "dense")                       # zero on that file's fragile and ill-conditioned pixels
    vis = _vis_map(sc)
    if sc["H"] > 1:
        assert 0.15 < float((vis < MIN_VIS).float().mean()) < 0.45
    want = _reference(sc, cot, mode, vis, monkeypatch)
    got = _run(sc, cot, mode, vis)
    forward, pixel, texel = ms.ratios(got, want)
    print(f"{name} / {mode}: forward {forward:.4f}, per-pixel gradients {pixel:.4f} (KAPPA_PIXEL {ms.KAPPA_PIXEL}), texel gradients {texel:.4f} "
          f"of 1e-4 x magnitude")
    assert forward <= 1.0 and pixel <= ms.KAPPA_PIXEL and texel <= 1.0
    assert torch.all(got["color"][~want["shaded"]] == 0)
    # a map of ones: the bits of 'none', forward and every gradient
    none = _run(sc, cot, "none", None)
    ones = _run(sc, cot, mode, torch.ones(sc["H"], sc["W"]))
    assert torch.equal(ones["color"], none["color"])
    for k in ("position", "normal", "uv"):
        assert torch.equal(ones["grad"][k], none["grad"][k]), k
    if mode == "screen":                                         # fl(colour of 'none' * v), to the last bit (module docstring)
        v = vis.clamp(min=MIN_VIS).reshape(-1, 1)
        assert torch.equal(got["color"], none["color"] * v)
    else:
        assert not torch.equal(got["color"], none["color"])


# ------------------------------------------------------------------------------------------------ render_mesh
def _mesh_scene(H=64, W=64):
    """the sphere on the plane, y up (the lat-long light's up axis): (x, y, z) -> (x, z, -y), a rotation"""
    v, f, n_sphere = ao_ref.sphere_on_plane()
    v = np.stack([v[:, 0], v[:, 2], -v[:, 1]], -1)
    c2w = ao_ref.lookat((1.6, 1.5, 2.2), (0.0, 0.3, 0.0), up=(0.0, 1.0, 0.0))
    focal = 0.9 * W
    cam = gs.Camera(torch.from_numpy(c2w).to(DEV), focal, focal, W / 2.0, H / 2.0, W, H)
    vt, ft = _dev(v.astype(np.float32), f)
    return vt, ft, cam, n_sphere


def _split_sum_env():
    sc = ms.scene("1x1")
    return _env(sc)


def test_render_mesh_occlusion_modes():
    v, f, cam, _ = _mesh_scene()
    kd = gs.Texture2D.from_constants((0.7, 0.6, 0.5), device=DEV)
    ks = gs.Texture2D.from_constants((0.0, 0.4, 0.1), device=DEV)
    env = _split_sum_env()
    vn = gs.vertex_normals(v, f)                                  # (computed once: its sums are atomic, two calls differ in the last bit)
    kw = dict(kd=kd, ks=ks, envmap=env, min_visibility=0.2, vertex_normals=vn)
    # 'ao': the default per-face values, and a given tensor
    maps = gs.render_mesh(v, f, cam, outputs=("color", "normal", "ao"), occlusion="ao", **kw)
    rast = maps["rast"]
    assert maps["ao"].shape == (64, 64, 1)
    face = (rast[..., 3].long() - 1).clamp_min(0)
    own = gs.face_ambient_occlusion(v, f)[face]
    assert torch.equal(maps["ao"][..., 0], own)
    covered = rast[..., 3] > 0
    assert bool((own[covered] < 0.9).any()) and bool((own[covered] == 1.0).any())
    position = gs.interpolate(v, rast, f)
    uv = torch.zeros(64, 64, 2, device=DEV)
    cam_pos = cam.c2w[:, 3]
    by_hand = gs.shade_pixels(position, maps["normal"], uv, rast, kd, ks, cam_pos, env, occlusion="ao", min_visibility=0.2, visibility=own)
    assert torch.equal(maps["color"], by_hand)
    per_face = torch.rand(f.shape[0], generator=torch.Generator().manual_seed(2)).to(DEV)
    given = gs.render_mesh(v, f, cam, outputs=("color", "ao"), occlusion="ao", ao=per_face, bvh=_bvh("sphere_on_plane"), **kw)
    assert torch.equal(given["ao"][..., 0], per_face[face])
    by_hand = gs.shade_pixels(position, maps["normal"], uv, rast, kd, ks, cam_pos, env, occlusion="ao", min_visibility=0.2,
                              visibility=per_face[face])
    assert torch.equal(given["color"], by_hand)
    # 'screen': the caller's map
    vis = torch.rand(64, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    screen = gs.render_mesh(v, f, cam, outputs=("color",), occlusion="screen", visibility=vis, **kw)
    by_hand = gs.shade_pixels(position, maps["normal"], uv, rast, kd, ks, cam_pos, env, occlusion="screen", min_visibility=0.2, visibility=vis)
    assert torch.equal(screen["color"], by_hand)
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("ao",), ao=per_face[:-1])
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("color",), occlusion="screen", **kw)
    with pytest.raises(ValueError, match="visibility"):
        gs.render_mesh(v, f, cam, outputs=("depth",), visibility=vis)
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("ssao",))


# ------------------------------------------------------------------------------------------------ render_mesh_mc
LIGHT_DIR = np.array([-0.5, 1.0, -0.6]) / np.linalg.norm([-0.5, 1.0, -0.6])      # from behind the sphere: the shadow falls towards the camera


def _patch_light(H=32, W=64, dim=0.02, bright=400.0):
    """a lat-long map (y up) that is dim everywhere except 3x3 texels around LIGHT_DIR"""
    data = torch.full((H, W, 3), dim)
    u = math.atan2(LIGHT_DIR[0], -LIGHT_DIR[2]) / (2 * math.pi) + 0.5
    vv = math.acos(LIGHT_DIR[1]) / math.pi
    x, y = int(u * W), int(vv * H)
    data[y - 1:y + 2, x - 1:x + 2] = bright
    return data.to(DEV)


_mc_cache = {}


def _mc_scene():
    v, f, cam, n_sphere = _mesh_scene(48, 48)
    g = torch.Generator().manual_seed(4)
    kd = gs.Texture2D((torch.rand(4, 4, 3, generator=g) * 0.6 + 0.3).to(DEV))
    ks = gs.Texture2D(torch.tensor([0.0, 0.5, 0.1]).repeat(2, 2, 1).to(DEV) + torch.rand(2, 2, 3, generator=g).to(DEV) * 0.1)
    uvs = torch.rand(f.shape[0], 3, 2, generator=g).to(DEV)
    if "vn" not in _mc_cache:
        _mc_cache["vn"] = gs.vertex_normals(v, f)                 # (computed once: its sums are atomic, two calls differ in the last bit)
    return v, f, cam, n_sphere, kd, ks, uvs


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("render_type", ["pbr", "diffuse", "vis"])
def test_render_mesh_mc_is_its_pipeline(render_type, denoise):
    v, f, cam, _, kd, ks, uvs = _mc_scene()
    light = gs.LatLngEnvMap(_patch_light())
    bvh = gs.MeshBVH(v, f)
    vn = _mc_cache["vn"]
    got = gs.render_mesh_mc(v, f, cam, kd=kd, ks=ks, uvs=uvs, envmap=light, bvh=bvh, num_samples_per_ray=4, rnd_seed=77, denoise=denoise,
                            render_type=render_type, vertex_normals=vn)
    assert got.shape == (48, 48, 3) and bool(torch.isfinite(got).all())
    # by hand
    vc = gs.meshrender.to_camera_space(v, cam)
    rast = gs.rasterize_mesh(vc, f, cam, cull="back")
    pos = gs.interpolate(v, rast, f)
    nrm = gs.meshrender._unit_or_z(gs.interpolate(vn, rast, f))
    uv = gs.interpolate(uvs, rast, f)
    kd_map, ks_map = kd.sample(uv), ks.sample(uv)
    c2w = cam.c2w
    depth = ((pos - c2w[:, 3]) * (-c2w[:, 2])).sum(-1, keepdim=True)
    flat = lambda t: t.reshape(-1, t.shape[-1])
    diff, spec, resi = gs.env_shade(bvh, (rast[..., 3] > 0).float().reshape(-1), flat(pos + nrm * 1e-3), flat(pos), flat(nrm),
                                    c2w[:, 3].contiguous(), flat(kd_map), flat(ks_map), light, BSDF="pbr", n_samples_x=4, rnd_seed=77,
                                    shadow_scale=1.0)
    diff, spec, resi = diff.view(48, 48, 3), spec.view(48, 48, 3), resi.view(48, 48, 2)
    den = (lambda t: gs.bilateral_denoiser(t.contiguous(), nrm, depth, 2.0)) if denoise else (lambda t: t)
    if render_type == "pbr":
        want = den(diff) * kd_map * (1.0 - ks_map[..., 2:3]) + den(spec)
    elif render_type == "diffuse":
        want = den(diff) * kd_map
    else:
        want = 1.0 - den(resi.sum(-1, keepdim=True).expand(48, 48, 3))
    assert torch.equal(got, want)
    assert torch.equal(got, gs.render_mesh_mc(v, f, cam, kd=kd, ks=ks, uvs=uvs, envmap=light, num_samples_per_ray=4, rnd_seed=77,
                                              denoise=denoise, render_type=render_type, vertex_normals=vn)), "the bvh built inside gives other bits"


def _shadow_factor(shadow_scale):
    v, f, cam, n_sphere, kd, ks, uvs = _mc_scene()
    light = gs.LatLngEnvMap(_patch_light())
    vis = gs.render_mesh_mc(v, f, cam, kd=kd, ks=ks, uvs=uvs, envmap=light, num_samples_per_ray=4, rnd_seed=5, render_type="vis",
                            shadow_scale=shadow_scale, vertex_normals=_mc_cache["vn"])[..., 0]
    rast = gs.rasterize_mesh(gs.meshrender.to_camera_space(v, cam), f, cam, cull="back")
    pos = gs.interpolate(v, rast, f).cpu().numpy().astype(np.float64)
    plane = ((rast[..., 3] - 1) >= n_sphere).cpu().numpy()
    centre = np.array([0.0, 0.5 + 1e-3, 0.0])
    rel = centre - pos
    along = (rel * LIGHT_DIR).sum(-1)
    dist = np.linalg.norm(rel - along[..., None] * LIGHT_DIR, axis=-1)               # from the sphere's centre to the ray towards the light
    shadow = plane & (dist < 0.35) & (along > 0)
    far = plane & (np.linalg.norm(pos[..., [0, 2]], axis=-1) >= 1.0)
    assert shadow.sum() >= 10 and far.sum() >= 100, (shadow.sum(), far.sum())
    vis = vis.cpu().numpy().astype(np.float64)
    return float(vis[far].mean() / vis[shadow].mean()), float(vis[shadow].mean()), float(vis[far].mean())


def test_render_mesh_mc_shadow():
    flat, s0, f0 = _shadow_factor(0.0)
    assert flat == 1.0 and s0 == 1.0 and f0 == 1.0, "shadow_scale = 0 shadows nothing"
    factor, s1, f1 = _shadow_factor(1.0)
    print(f"shadow factor: 'vis' far from the sphere {f1:.4f} / inside its shadow {s1:.4f} = {factor:.3f} (1.0 with shadow_scale = 0)")
    assert factor > SHADOW_FACTOR_MIN


def test_render_mesh_mc_gradients_and_arguments():
    v, f, cam, _, kd, ks, uvs = _mc_scene()
    v = v.clone().requires_grad_()
    kd, ks = gs.Texture2D(kd.data.clone().requires_grad_()), gs.Texture2D(ks.data.clone().requires_grad_())
    light = gs.LatLngEnvMap(_patch_light(dim=0.5, bright=20.0).requires_grad_())
    out = gs.render_mesh_mc(v, f, cam, kd=kd, ks=ks, uvs=uvs, envmap=light, num_samples_per_ray=4, rnd_seed=9)
    (out * torch.rand(48, 48, 3, generator=torch.Generator().manual_seed(1)).to(DEV)).sum().backward()
    for name, t in (("kd", kd.data), ("ks", ks.data), ("light", light.data), ("vertices", v)):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
    with pytest.raises(ValueError, match="transform"):
        gs.render_mesh_mc(v, f, cam, kd=kd, ks=ks, uvs=uvs, envmap=gs.LatLngEnvMap(_patch_light()).rotateY_(0.4))
