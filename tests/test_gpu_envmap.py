"""Environment resampling on the GPU (csrc/gs_envmap.hip, geosplatting_amd/envmap.py) against the float64 restatement of
tests/envmap_ref.py: EVERY element of the forward and of the texel gradients within KAPPA x 1e-4 x magnitude (budgets, magnitudes and
the fragile rule are the restatement's, derived in its docstring; nothing is tuned here), the exact properties, what the transforms
mean, the hand-off between the stages and the errors.

Measured on an MI355X (largest error / budget over the four cases, as the tests print it): cube -> lat-long 0.554 and 0.141 (texel
gradient), lat-long -> cube 0.507 and 0.087, sample_cubemap 0.217 and 0.011, background 0.043 (sRGB) and 0.132 (radiance); no element is
left out of the conversions, none is fragile among the sample directions and the background pixels ("Environment
resampling and relighting")."""
import math

import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import envmap as E
from geosplatting_amd._lib import GeoSplatHipError
from tests import envmap_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _within(what, got, want, mag, keep=None):
    ratio = ref.worst_ratio(got.detach().cpu(), want, mag, what, keep) / ref.KAPPA
    print(f"\n  {what}: worst error / budget {ratio:.3f}", end="")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------ every element against float64
@pytest.mark.parametrize("k", range(len(ref.CASES)))
def test_cube_to_latlng_against_float64(k):
    R, H, W, name = ref.CASES[k]
    x = ref.case_inputs(k)
    cube = x["cube"].to(DEV).requires_grad_(True)
    out = gs.cube_to_latlng(cube, W, H, _dev(x["transform"]))
    assert out.shape == (H, W, 3)
    (out * x["cot_latlng"].to(DEV)).sum().backward()
    want = ref.cube_to_latlng(x["cube"], H, W, x["transform"], x["cot_latlng"])
    _within(f"{ref.CASES[k]} cube -> lat-long", out, want["value"], want["mag"])
    _within(f"{ref.CASES[k]} cube -> lat-long, texel gradient", cube.grad, want["grad"], want["mag_grad"])


@pytest.mark.parametrize("k", range(len(ref.CASES)))
def test_latlng_to_cube_against_float64(k):
    R, H, W, name = ref.CASES[k]
    x = ref.case_inputs(k)
    lat = x["latlng"].to(DEV).requires_grad_(True)
    out = gs.latlng_to_cube(lat, R)
    assert out.shape == (6, R, R, 3)
    (out * x["cot_cube"].to(DEV)).sum().backward()
    want = ref.latlng_to_cube(x["latlng"], R, x["cot_cube"])
    _within(f"{ref.CASES[k]} lat-long -> cube", out, want["value"], want["mag"])
    _within(f"{ref.CASES[k]} lat-long -> cube, texel gradient", lat.grad, want["grad"], want["mag_grad"])


def test_sample_cubemap_against_float64():
    s = ref.sample_inputs()
    keep = ~ref.fragile_dirs(s["dirs"], ref.SAMPLE_R)
    assert float((~keep).float().mean()) <= ref.FRAGILE_CAP
    cot = s["cot"] * keep[:, None]
    cube = s["cube"].to(DEV).requires_grad_(True)
    dirs = s["dirs"].to(DEV).requires_grad_(True)
    out = gs.sample_cubemap(cube, dirs)
    (out * cot.to(DEV)).sum().backward()
    assert dirs.grad is None                                              # no gradient to the directions
    want = ref.sample_cubemap(s["cube"], s["dirs"], cot)
    _within("sample_cubemap", out, want["value"], want["mag"], keep)
    _within("sample_cubemap, texel gradient", cube.grad, want["grad"], want["mag_grad"])
    n = ref.SAMPLE_N
    assert torch.equal(out[n:n + 3].cpu(), torch.zeros(3, 3))             # the zero row and the NaN rows
    centre = gs.sample_cubemap(cube.detach(), torch.tensor([[1.0, 0.0, 0.0]], device=DEV)).cpu()
    assert torch.equal(out[n + 3:n + 4].cpu(), centre)                    # an axis is the mean of the four centre texels of its face
    assert torch.allclose(centre[0], s["cube"][0, 7:9, 7:9].reshape(4, 3).mean(0), atol=1e-6)
    # the shape family: [..., 3] in, [..., 3] out, the same bits
    again = gs.sample_cubemap(cube.detach(), s["dirs"][:4000].to(DEV).reshape(40, 100, 3))
    assert again.shape == (40, 100, 3) and torch.equal(again.reshape(-1, 3), out[:4000].detach())


@pytest.mark.parametrize("srgb", [True, False])
def test_background_against_float64(srgb):
    b, g = ref.background_inputs(), ref.BG
    cam = gs.Camera(b["c2w"].to(DEV), g["fx"], g["fy"], g["cx"], g["cy"], g["W"], g["H"])
    out = gs.render_background(b["cube"].to(DEV), cam, _dev(b["transform"]), srgb=srgb)
    assert out.shape == (g["H"], g["W"], 3)
    want = ref.background(b["cube"], g["H"], g["W"], g["fx"], g["fy"], g["cx"], g["cy"], b["c2w"], b["transform"], srgb)
    assert float(want["fragile"].float().mean()) <= ref.FRAGILE_CAP
    _within(f"background srgb={srgb}", out, want["value"], want["mag"], ~want["fragile"])
    via_map = E.EnvCubeMap(b["cube"].to(DEV), _dev(b["transform"])).render(cam, srgb=srgb)
    assert torch.equal(via_map, out)
    # over an opaque pixel the picture stays, over an empty one the background shows
    rgba = torch.rand(g["H"], g["W"], 4, device=DEV)
    rgba[:5, :, 3], rgba[5:10, :, 3] = 1.0, 0.0
    blent = gs.blend_background(rgba, out)
    assert torch.equal(blent[:5], rgba[:5, :, :3]) and torch.equal(blent[5:10], out[5:10])


# ------------------------------------------------------------------------------------------------ exact properties
def test_forwards_are_bit_reproducible_and_the_class_forms_agree():
    R, H, W, name = ref.CASES[3]
    x = ref.case_inputs(3)
    cube, lat, T = x["cube"].to(DEV), x["latlng"].to(DEV), x["transform"].to(DEV)
    a, b = gs.cube_to_latlng(cube, W, H, T), gs.cube_to_latlng(cube, W, H, T)
    assert torch.equal(a, b)
    assert torch.equal(gs.latlng_to_cube(lat, R), gs.latlng_to_cube(lat, R))
    m = E.EnvCubeMap(cube, T.clone())
    baked = m.as_latlng(width=W, height=H, apply_transform=True)
    assert torch.equal(baked.data, a) and baked.transform is None         # the functional form with the same matrix, bit for bit
    carried = m.as_latlng(width=W, height=H)
    assert torch.equal(carried.data, gs.cube_to_latlng(cube, W, H)) and torch.equal(carried.transform, T)
    assert not torch.equal(carried.data, a)
    assert torch.equal(m.visualize(width=W, height=H), a)
    back = gs.LatLngEnvMap(lat, T.clone()).as_cubemap(R)
    assert torch.equal(back.data, gs.latlng_to_cube(lat, R)) and torch.equal(back.transform, T)
    plain = gs.LatLngEnvMap(lat)
    assert plain.visualize() is plain.data and plain.as_cubemap(R).transform is None
    seen = gs.LatLngEnvMap(lat, T.clone()).visualize()
    assert torch.equal(seen, gs.cube_to_latlng(gs.latlng_to_cube(lat, max(H, W)), W, H, T))
    twin = m.clone()
    twin.data.zero_()
    assert float(m.data.abs().sum()) > 0


def test_backwards_add_into_the_gradient_and_zero_stays_zero():
    from geosplatting_amd import _lib as L
    R, H, W, name = ref.CASES[2]
    x = ref.case_inputs(2)
    cube, lat, T = x["cube"].to(DEV), x["latlng"].to(DEV), x["transform"].to(DEV)
    s = ref.sample_inputs()
    dirs, scube = s["dirs"].to(DEV), s["cube"].to(DEV)
    n = dirs.shape[0]
    lib = L.lib()
    jobs = (("cube -> lat-long", (6, R, R, 3), x["cot_latlng"].to(DEV),
             lambda g, buf: lib.gs_env_cube_to_latlng_bwd(R, H, W, L.ptr(T), L.ptr(g), L.ptr(buf), L.stream())),
            ("lat-long -> cube", (H, W, 3), x["cot_cube"].to(DEV),
             lambda g, buf: lib.gs_env_latlng_to_cube_bwd(H, W, R, L.ptr(g), L.ptr(buf), L.stream())),
            ("sample", (6, ref.SAMPLE_R, ref.SAMPLE_R, 3), torch.nan_to_num(s["cot"]).to(DEV),
             lambda g, buf: lib.gs_cube_sample_linear_bwd(n, ref.SAMPLE_R, L.ptr(dirs), 1.0, L.ptr(g), L.ptr(buf), L.stream())))
    for what, shape, cot, call in jobs:
        cot = cot.contiguous()
        fresh = torch.zeros(shape, device=DEV)
        L.check(call(cot, fresh), what)
        assert float(fresh.abs().sum()) > 0
        filled = torch.full(shape, 2.0, device=DEV)
        L.check(call(cot, filled), what)
        assert torch.allclose(filled, fresh + 2.0, atol=1e-5), what       # ADDED to what the buffer held (atomics: sums in any order)
        zero = torch.zeros(shape, device=DEV)
        L.check(call(torch.zeros_like(cot), zero), what)
        assert torch.equal(zero, torch.zeros_like(zero)), what            # a zero cotangent gives a zero gradient
        seven = torch.full(shape, 7.0, device=DEV)
        L.check(call(torch.zeros_like(cot), seven), what)
        assert torch.equal(seven, torch.full_like(seven, 7.0)), what
    # through autograd: two uses of one cube sum their gradients
    c = cube.clone().requires_grad_(True)
    (gs.cube_to_latlng(c, W, H, T).sum() + gs.cube_to_latlng(c, W, H).sum()).backward()
    c1 = cube.clone().requires_grad_(True)
    gs.cube_to_latlng(c1, W, H, T).sum().backward()
    c2 = cube.clone().requires_grad_(True)
    gs.cube_to_latlng(c2, W, H).sum().backward()
    assert torch.allclose(c.grad, c1.grad + c2.grad, atol=1e-4)
    assert float(c1.grad.sum()) == pytest.approx(3.0 * H * W, rel=1e-5)   # every lookup's weights sum to 1


# ------------------------------------------------------------------------------------------------ meaning
def _bump_cube(R, d0, width=0.2):
    """a cube map with one smooth bright patch around the direction d0, at the restatement's texel directions"""
    g = torch.linspace(-1.0 + 1.0 / R, 1.0 - 1.0 / R, R, dtype=torch.float64)
    gy, gx = torch.meshgrid(g, g, indexing="ij")
    face = torch.arange(6).repeat_interleave(R * R)
    v = ref.tr._face_point(face, gx.reshape(-1).repeat(6), gy.reshape(-1).repeat(6))
    v = v / v.norm(dim=-1, keepdim=True)
    ang = torch.acos((v @ d0.double()).clamp(-1, 1))
    return torch.exp(-(ang / width) ** 2).float().reshape(6, R, R, 1).repeat(1, 1, 1, 3).contiguous()


def test_a_rotated_light_lands_where_the_transform_says():
    d0 = torch.nn.functional.normalize(torch.tensor([0.6, 0.3, -0.7]), dim=0)
    angle, H, W = 0.9, 32, 64
    m = E.EnvCubeMap(_bump_cube(32, d0).to(DEV))
    m.rotateY_(angle)
    T = m.transform.cpu().double()
    d = T.T @ d0.double()                                                 # T d = d0
    lat = m.as_latlng(width=W, height=H, apply_transform=True).data
    flat = int(lat[..., 0].argmax())
    i, j = flat // W, flat % W
    theta, phi = math.acos(float(d[1])), math.atan2(float(d[0]), -float(d[2]))
    row = (theta / math.pi - 1.0 / H) / ((1.0 - 2.0 / H) / (H - 1))
    col = (phi / math.pi - (-1.0 + 1.0 / W)) / ((2.0 - 2.0 / W) / (W - 1))
    assert abs(i - row) <= 1.0 and min(abs(j - col), W - abs(j - col)) <= 1.0, (i, j, row, col)
    # without the rotation the patch sits at d0 itself: the transform moved it
    lat0 = gs.cube_to_latlng(m.data, W, H)
    flat0 = int(lat0[..., 0].argmax())
    phi0 = math.atan2(float(d0[0]), -float(d0[2]))
    col0 = (phi0 / math.pi - (-1.0 + 1.0 / W)) / ((2.0 - 2.0 / W) / (W - 1))
    assert abs(flat0 % W - col0) <= 1.0 and abs(col0 - col) > 5.0
    # a camera that looks along d sees the patch at its principal point
    eye = torch.zeros(3)
    c2w = gs.lookat_c2w(eye, d.float(), torch.tensor([0.0, 1.0, 0.0]))
    Hc, Wc, cx, cy = 41, 57, 30.5, 17.5
    cam = gs.Camera(c2w.to(DEV), 60.0, 55.0, cx, cy, Wc, Hc)
    for srgb in (True, False):
        img = m.render(cam, srgb=srgb)
        p = int(img[..., 1].argmax())
        assert abs(p // Wc - (cy - 0.5)) <= 1.0 and abs(p % Wc - (cx - 0.5)) <= 1.0, (p // Wc, p % Wc)


def test_an_analytic_light_survives_both_resamplings():
    R, H, W = 64, 32, 64
    a, b = torch.tensor([0.8, 0.6, 0.7], dtype=torch.float64), torch.tensor([0.3, -0.2, 0.25], dtype=torch.float64)
    g = torch.linspace(-1.0 + 1.0 / R, 1.0 - 1.0 / R, R, dtype=torch.float64)
    gy, gx = torch.meshgrid(g, g, indexing="ij")
    face = torch.arange(6).repeat_interleave(R * R)
    v = ref.tr._face_point(face, gx.reshape(-1).repeat(6), gy.reshape(-1).repeat(6))
    v = v / v.norm(dim=-1, keepdim=True)
    cube = (a + v @ b[:, None]).float().reshape(6, R, R, 3)                # L(d) = a + b . d per channel
    d = ref.latlng_dirs(H, W, None, torch.float64)
    exact = (a + d @ b[:, None]).reshape(H, W, 3)
    want = ref.cube_to_latlng(cube, H, W)
    got = gs.cube_to_latlng(cube.to(DEV), W, H).cpu().double()
    ref_err = (want["value"] - exact).abs()
    assert float(ref_err.max()) < 2e-3                                    # bilinear interpolation of a smooth map on 64^2 faces
    assert bool(((got - exact).abs() <= ref_err + ref.KAPPA * 1e-4 * want["mag"]).all())


# ------------------------------------------------------------------------------------------------ hand-off between the stages
def test_stage1_cube_feeds_env_shade_and_a_transform_is_refused():
    from tests import envshade_ref as er
    v, f = er.scene_mesh()
    bvh = gs.MeshBVH(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    pt = er.points(33)
    t = {k: torch.from_numpy(pt[k]).to(DEV) for k in ("ro", "pos", "nrm", "kd", "ks")}
    cube = ref.case_inputs(2)["cube"].to(DEV).requires_grad_(True)
    light = E.EnvCubeMap(cube).as_latlng(64, 32).compute_pdf_()
    assert light.data.shape == (32, 64, 3) and light.pdf.shape == (32, 64, 3) and light.transform is None
    args = (bvh, torch.ones(33, device=DEV), t["ro"], t["pos"], t["nrm"], torch.from_numpy(er.CAMERA).to(DEV), t["kd"], t["ks"])
    diff, spec, resi = gs.env_shade(*args, light, n_samples_x=4, rnd_seed=5)
    same = gs.env_shade(*args, light.data, *light.tables(), n_samples_x=4, rnd_seed=5)
    assert torch.equal(diff, same[0]) and torch.equal(spec, same[1])
    assert bool(torch.isfinite(diff).all()) and float(diff.detach().sum()) > 0
    (diff.sum() + spec.sum()).backward()                                  # ... and the stage-1 cube map gets a gradient through it
    assert bool(torch.isfinite(cube.grad).all()) and float(cube.grad.abs().sum()) > 0
    turned = E.EnvCubeMap(cube.detach()).z_up_to_y_up_().as_latlng(64, 32).compute_pdf_()
    assert turned.transform is not None
    with pytest.raises(ValueError, match="without a transform"):
        gs.env_shade(*args, turned, n_samples_x=4, rnd_seed=5)
    attrs = gs.RenderableAttrs(t["kd"], t["ks"][:, 1:], t["nrm"], occ=torch.zeros(33, 6, device=DEV))
    for fn in (attrs.splat_mc, attrs.splat_mc_deferred):
        with pytest.raises(ValueError, match="without a transform"):
            fn(None, None, bvh=bvh, exposure=torch.tensor(1.0, device=DEV), positions=t["pos"], envmap=turned, min_roughness=0.1,
               max_metallic=0.5, **({"mask": torch.ones(33, 1, device=DEV)} if fn == attrs.splat_mc_deferred else {}))
    baked = turned.as_cubemap(32).as_latlng(64, 32, apply_transform=True).compute_pdf_()
    assert baked.transform is None
    gs.env_shade(*args, baked, n_samples_x=4, rnd_seed=5)


def test_latlng_light_feeds_the_mesh_shader_and_gets_a_gradient():
    """as_cubemap(64): the smallest cube map that `as_splitsum()` takes.  A 16^2 map has no pyramid (64 -> 32 -> 16 are the three
    levels the default min_resolution = 16 needs; a smaller one ends in "Min resolution is too large", here as in the reference)."""
    lat = ref.case_inputs(2)["latlng"].to(DEV).requires_grad_(True)
    with pytest.raises(AssertionError, match="Min resolution"):
        gs.LatLngEnvMap(lat.detach()).as_cubemap(16).as_splitsum()
    cube = gs.LatLngEnvMap(lat).as_cubemap(64)
    assert cube.data.shape == (6, 64, 64, 3)
    env = cube.as_splitsum()
    assert len(env.levels) == 3 and env.base.shape == (6, 16, 16, 3)
    Hp = Wp = 12
    yy, xx = torch.meshgrid(torch.linspace(-0.7, 0.7, Hp), torch.linspace(-0.7, 0.7, Wp), indexing="ij")
    zz = (1.0 - xx * xx - yy * yy).clamp(min=0.0).sqrt()
    position = torch.stack((xx, -yy, zz), -1).to(DEV)
    normal = torch.nn.functional.normalize(position, dim=-1)
    uv = torch.rand(Hp, Wp, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    rast = torch.ones(Hp, Wp, 4, device=DEV)
    kd = gs.Texture2D.from_constants((0.7, 0.5, 0.3), device=DEV)
    ks = gs.Texture2D.from_constants((0.0, 0.4, 0.2), device=DEV)
    color = gs.shade_pixels(position, normal, uv, rast, kd, ks, torch.tensor([0.0, 0.0, 3.0], device=DEV), env)
    assert color.shape == (Hp, Wp, 3) and bool(torch.isfinite(color).all()) and float(color.detach().mean()) > 0.01
    ((color - 0.5) ** 2).mean().backward()
    assert bool(torch.isfinite(lat.grad).all()) and float(lat.grad.abs().sum()) > 0
    with pytest.raises(ValueError, match="without a transform"):
        gs.LatLngEnvMap(lat.detach()).rotateY_(0.2).as_cubemap(64).as_splitsum()


def test_relight_sequence_turns_the_light_once_around():
    d0 = torch.nn.functional.normalize(torch.tensor([0.5, 0.2, 0.8]), dim=0)
    base = E.EnvCubeMap(_bump_cube(16, d0, 0.4).to(DEV)).z_up_to_y_up_()
    first = base.clone().as_latlng(32, 16, apply_transform=True)
    frames = list(gs.relight_sequence(base, 32, 16, 4))
    assert len(frames) == 4 and all(f.transform is None and f.pdf is not None and f.data.shape == (16, 32, 3) for f in frames)
    assert torch.equal(frames[0].data, first.data)
    spots = [int(f.data[..., 0].argmax()) for f in frames]
    assert len(set(spots)) == 4                                           # the bright patch moves with every frame ...
    dirs = ref.latlng_dirs(16, 32, None, torch.float64)
    for k, spot in enumerate(spots):                                      # ... to where that frame's transform puts it: T_k d = d0
        T = (E.frame_rotation("y", k * math.pi / 2) @ E.frame_z_up_to_y_up()).double()
        assert float(torch.acos((T @ dirs[spot]).dot(d0.double()).clamp(-1, 1))) < math.pi / 16, k     # one texel
    assert torch.allclose(base.transform.cpu(), E.frame_z_up_to_y_up(), atol=1e-6)   # ... and four quarter turns are the identity


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    cube, lat = torch.rand(6, 4, 4, 3), torch.rand(4, 8, 3)
    for call in (lambda: gs.cube_to_latlng(cube, 8, 4), lambda: gs.latlng_to_cube(lat, 4), lambda: gs.sample_cubemap(cube, torch.rand(2, 3)),
                 lambda: gs.sample_cubemap(cube.to(DEV), torch.rand(2, 3)),
                 lambda: gs.render_background(cube, gs.Camera(torch.eye(4)[:3], 8.0, 8.0, 4.0, 4.0, 8, 8))):
        with pytest.raises(GeoSplatHipError, match="GPU only"):
            call()
    cube, lat = cube.to(DEV), lat.to(DEV)
    with pytest.raises(ValueError, match="at least 2"):
        gs.cube_to_latlng(cube, 8, 1)
    with pytest.raises(ValueError, match="at least 2"):
        E.EnvCubeMap(cube).as_latlng(width=1, height=4)
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        gs.cube_to_latlng(cube, 8, 4, torch.eye(4, device=DEV))
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        gs.render_background(cube, gs.Camera(torch.eye(4)[:3].to(DEV), 8.0, 8.0, 4.0, 4.0, 8, 8), torch.zeros(9, device=DEV))
    with pytest.raises(ValueError, match="4096"):
        gs.latlng_to_cube(lat, E.MAX_CUBE_RES + 1)
    big = torch.empty(1, device=DEV).expand(6, E.MAX_CUBE_RES + 1, E.MAX_CUBE_RES + 1, 3)       # a shape without memory behind it
    with pytest.raises(ValueError, match="4096"):
        gs.cube_to_latlng(big, 8, 4)
    with pytest.raises(ValueError, match="4096"):
        gs.sample_cubemap(big, torch.rand(2, 3, device=DEV))
    with pytest.raises(ValueError):
        gs.latlng_to_cube(torch.rand(1, 8, 3, device=DEV), 4)
    with pytest.raises(ValueError):
        gs.sample_cubemap(cube, torch.rand(2, 4, device=DEV))
