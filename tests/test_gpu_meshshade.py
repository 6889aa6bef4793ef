"""GPU tests of the mesh shading kernels (csrc/gs_meshshade.hip through geosplatting_amd.meshshade and render_mesh) against the float64
restatement tests/meshshade_ref.py, whose scenes, magnitudes, fragile flags and KAPPA_PIXEL are checked without a GPU in
tests/test_meshshade_cpu.py.

Forward.   |colour - reference| <= 1e-4 magnitude per element on every pixel (the value is continuous across every selection); empty
           pixels and pixels with a non-finite input exactly 0; two runs bit-identical.
Backward.  Cotangents are zero on the fragile and on the ill-conditioned pixels (tests/meshshade_ref.py); dense and single-channel
           cotangents.  d_position, d_normal, d_uv within KAPPA_PIXEL 1e-4 magnitude per element (per vector only for d_position under
           the single-channel cotangent, where one pass contributes), every texel array (kd, ks, base, the levels) within 1e-4
           magnitude; magnitude 0 means exactly 0 (empty pixels, texels no footprint touches); the per-pixel gradients of two runs
           bit-identical; gradients accumulate on top of a non-zero .grad.  The scene '64x64 constants' is the pile-up case: every
           shaded pixel adds into the 3 + 3 floats of two 1x1 textures.
texture2d. The same bounds for C = 1, 3, 4 and both boundary modes on 1x1, 2x3, 5x7 and 64x64 textures with uv in [-1.3, 2.3] (texel
           coordinates within DELTA of an integer are fragile), and on a lattice of dyadic uv on the texel centres and borders of a 4x8
           texture, where every weight is exactly 0, 1/2 or 1 on both sides and nothing is fragile.
render_mesh(outputs=('color', ...)) equals shade_pixels on the maps render_mesh itself produces, bit for bit, and the restatement on
those maps within the forward bound; with antialias=True, color equals antialias of the plain colour bit for bit (antialias does
not depend on the channel count of the image, which has a test of its own); a call without
'color' returns what it returned before.  Sixty Adam steps on a 16x16 kd texture bring the L1 to a target render below a tenth.

Measured on an MI355X, worst ratio to 1e-4 x magnitude: forward 0.27 (render_mesh's colour 0.036); per-pixel gradients 2.83 of the
KAPPA_PIXEL = 8 allowed (the float32 CPU restatement: 2.91); texel gradients 0.113; texture2d out 0.018, d_uv 0.20 (of 8), d_tex
0.0009.  The texture fit ends at 0.016 of its starting L1.
"""
import math

import pytest
import torch

import geosplatting_amd as gs
from tests import meshraster_ref as ref
from tests import meshshade_ref as ms

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = sorted(ms.SCENES)


def _env(sc, grad=False):
    base = sc["base"].to(DEV).requires_grad_(grad)
    levels = [l.to(DEV).requires_grad_(grad) for l in sc["levels"]]
    return gs.TextureSplitSum(base, levels, ms.MIN_R, ms.MAX_R)


def _rast(sc):
    rast = torch.zeros(sc["H"], sc["W"], 4)
    rast[..., 3] = torch.where(sc["covered"].view(sc["H"], sc["W"]), 5.0, 0.0)
    return rast.to(DEV)


def _inputs(sc, grad=False):
    H, W = sc["H"], sc["W"]
    maps = [sc[k].view(H, W, -1).to(DEV).requires_grad_(grad) for k in ("position", "normal", "uv")]
    return maps, gs.Texture2D(sc["kd"].to(DEV).requires_grad_(grad)), gs.Texture2D(sc["ks"].to(DEV).requires_grad_(grad))


def _shade(sc, maps, kd, ks, env):
    return gs.shade_pixels(*maps, _rast(sc), kd, ks, sc["cam"].to(DEV), env, occlusion=sc["occlusion"],
                           min_visibility=sc["min_visibility"], bend_back_normal=sc["bend"])


# ------------------------------------------------------------------------------------------------ shade_pixels
@pytest.mark.parametrize("name", NAMES)
def test_shade_forward(name):
    sc = ms.scene(name)
    _, want = ms.reference(name, "dense")
    maps, kd, ks = _inputs(sc)
    color = _shade(sc, maps, kd, ks, _env(sc))
    again = _shade(sc, maps, kd, ks, _env(sc))
    assert color.shape == (sc["H"], sc["W"], 3) and torch.equal(color, again), "two forward runs differ"
    got = color.cpu().reshape(-1, 3)
    assert torch.all(got[~want["shaded"]] == 0), "an empty pixel or one with a non-finite input is not exactly 0"
    assert bool((got[want["shaded"]] != 0).any())
    r = ms.worst_ratio(got, want["color"], want["mag_color"], "colour")
    print(f"{name}: forward {r:.4f} of 1e-4 x magnitude")
    assert r <= 1.0


def _backward(sc, cot, preset=None):
    """one forward + backward on fresh leaves -> evaluate()-shaped gradients on the CPU; `preset`: fill every .grad with it first"""
    maps, kd, ks = _inputs(sc, grad=True)
    env = _env(sc, grad=True)
    leaves = maps + [kd.data, ks.data, env.base] + list(env.levels)
    if preset is not None:
        for t in leaves:
            t.grad = torch.full_like(t, preset)
    color = _shade(sc, maps, kd, ks, env)
    (color * cot.view_as(color).to(DEV)).sum().backward()
    flat = lambda t: t.grad.cpu().reshape(-1, t.shape[-1])
    return dict(color=color.detach().cpu().reshape(-1, 3),
                grad=dict(position=flat(maps[0]), normal=flat(maps[1]), uv=flat(maps[2]), kd=kd.data.grad.cpu(), ks=ks.data.grad.cpu(),
                          base=env.base.grad.cpu(), levels=[l.grad.cpu() for l in env.levels]))


@pytest.mark.parametrize("kind", ["dense", "single"])
@pytest.mark.parametrize("name", NAMES)
def test_shade_backward(name, kind):
    sc = ms.scene(name)
    cot, want = ms.reference(name, kind)
    got = _backward(sc, cot)
    forward, pixel, texel = ms.ratios(got, want)
    print(f"{name} / {kind}: per-pixel gradients {pixel:.4f} (KAPPA_PIXEL {ms.KAPPA_PIXEL}), texel gradients {texel:.4f} of 1e-4 x magnitude")
    assert forward <= 1.0 and pixel <= ms.KAPPA_PIXEL and texel <= 1.0
    empty = ~want["shaded"]
    for k in ("position", "normal", "uv"):
        assert torch.all(got["grad"][k][empty] == 0), f"d_{k} is not zero at an empty pixel"
    again = _backward(sc, cot)
    for k in ("position", "normal", "uv"):
        assert torch.equal(got["grad"][k], again["grad"][k]), f"two runs of d_{k} differ"


@pytest.mark.parametrize("name", ["37x53 textured", "64x64 constants"])
def test_shade_gradients_accumulate(name):
    """every .grad holds 0.5 before the backward: afterwards it holds 0.5 + the gradient, under the same bounds (plus the rounding of
    that one addition, 2^-23 of max(0.5, |gradient|), which the bound covers wherever the gradient exceeds 0.5)"""
    sc = ms.scene(name)
    cot, want = ms.reference(name, "dense")
    onto = _backward(sc, cot, preset=0.5)["grad"]
    triples = [(onto[k], want["grad"][k], ms.KAPPA_PIXEL * want["mag"][k]) for k in ("position", "normal", "uv")]
    triples += [(onto[k], want["grad"][k], want["mag"][k]) for k in ("kd", "ks", "base")]
    triples += list(zip(onto["levels"], want["grad"]["levels"], want["mag"]["levels"]))
    for got, ref_grad, mag in triples:
        assert torch.all(got[mag == 0] == 0.5), "an element of magnitude 0 must keep its preset value exactly"
        assert torch.all(((got.double() - 0.5) - ref_grad).abs()[mag > 0] <= (1e-4 * mag + 2.0 ** -23)[mag > 0])


# ------------------------------------------------------------------------------------------------ texture2d
def _lattice():
    """dyadic uv on the texel centres and borders of a 4x8 texture, one and a half periods around [0, 1)"""
    u = torch.arange(-8, 25, dtype=torch.float32) / 16.0              # multiples of 1/16: centres (odd) and borders (even) of 8 texels
    v = torch.arange(-4, 13, dtype=torch.float32) / 8.0
    return torch.stack(torch.meshgrid(u, v, indexing="ij"), -1).reshape(-1, 2)


def _tex_case(size, C, boundary, lattice):
    g = torch.Generator().manual_seed(size[0] * 100 + size[1] + C)
    tex = torch.rand(*size, C, generator=g) + 0.1
    if lattice:
        uv = _lattice()
        fragile = torch.zeros(uv.shape[0], dtype=torch.bool)
    else:
        uv = torch.rand(37 * 53, 2, generator=g) * 3.6 - 1.3
        uv[3, 0] = float("nan"); uv[4, 1] = float("inf")
        Ht, Wt = size
        q = torch.where(torch.isfinite(uv), uv, torch.zeros_like(uv)).double()
        near = lambda x: (x - x.round()).abs() < ms.DELTA
        fragile = torch.zeros(uv.shape[0], dtype=torch.bool)
        for k, n in ((0, Wt), (1, Ht)):
            if n > 1:
                fragile |= near(q[:, k] * n - 0.5) | (((q[:, k] - q[:, k].round()).abs() * n < ms.DELTA) if boundary == "wrap" else torch.zeros_like(fragile))
    cot = torch.randn(uv.shape[0], C, generator=g)
    cot[fragile] = 0.0
    return tex, uv, cot


def _tex_reference(tex, uv, cot, boundary):
    t, q, g = tex.double().requires_grad_(), uv.double().requires_grad_(), cot.double()
    out = ms.texture2d(t, q, boundary)
    C = tex.shape[-1]
    (g * out).sum().backward()
    finite = torch.isfinite(uv).all(-1)
    qz = torch.where(finite[:, None], uv.double(), torch.zeros(1, dtype=torch.float64))
    Ht, Wt = tex.shape[:2]
    if boundary == "wrap":
        taps, x, y = ms.wrap_taps(Ht, Wt, qz)
        su, sv = torch.full_like(x, Wt), torch.full_like(y, Ht)
    else:
        rx, ry = qz[:, 0] * Wt - 0.5, qz[:, 1] * Ht - 0.5
        su = torch.where((rx < 0) | (rx > Wt - 1), 0.0, float(Wt)).double()        # gradient 0 in a clamped coordinate
        sv = torch.where((ry < 0) | (ry > Ht - 1), 0.0, float(Ht)).double()
        x = (qz[:, 0] * Wt - 0.5).clamp(0, Wt - 1); y = (qz[:, 1] * Ht - 0.5).clamp(0, Ht - 1)
        ix0, iy0 = x.floor().long(), y.floor().long()
        ix1, iy1 = (ix0 + 1).clamp(max=Wt - 1), (iy0 + 1).clamp(max=Ht - 1)
        taps = [iy0 * Wt + ix0, iy0 * Wt + ix1, iy1 * Wt + ix0, iy1 * Wt + ix1]
    mag_tex = torch.zeros(Ht * Wt, C, dtype=torch.float64)
    seen = []
    for i in taps:
        ok = finite.clone()
        for j in seen:
            ok &= i != j
        mag_tex.index_add_(0, i[ok], g.abs()[ok])
        seen.append(i)
    # d_uv, per element: the patch derivative W ((1 - fy)(t10 - t00) + fy (t11 - t01)) with every term replaced by its absolute value
    # (a float32 fy carries an absolute error, which the derivative's own value does not bound where its terms cancel)
    fx, fy = (x - x.floor())[:, None], (y - y.floor())[:, None]
    flat = tex.double().reshape(-1, C)
    t00, t10, t01, t11 = (flat[i] for i in taps)
    du = su[:, None] * ((1 - fy) * (t10 - t00).abs() + fy * (t11 - t01).abs())
    dv = sv[:, None] * ((1 - fx) * (t01 - t00).abs() + fx * (t11 - t10).abs())
    mag_uv = torch.stack(((g.abs() * du).sum(-1), (g.abs() * dv).sum(-1)), -1) * finite[:, None]
    with torch.no_grad():
        mag_out = ms.texture2d(t.abs(), q, boundary)
    return dict(out=out.detach(), mag_out=mag_out, d_uv=q.grad, mag_uv=mag_uv, d_tex=t.grad,
                mag_tex=mag_tex.reshape(Ht, Wt, C))


@pytest.mark.parametrize("boundary", ["wrap", "clamp"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (5, 7), (64, 64), "lattice"])
def test_texture2d(size, C, boundary):
    lattice = size == "lattice"
    tex, uv, cot = _tex_case((4, 8) if lattice else size, C, boundary, lattice)
    want = _tex_reference(tex, uv, cot, boundary)
    t, q = tex.to(DEV).requires_grad_(), uv.to(DEV).requires_grad_()
    out = gs.texture2d(t, q, boundary)
    assert out.shape == (uv.shape[0], C) and torch.equal(out, gs.texture2d(t, q, boundary))
    (out * cot.to(DEV)).sum().backward()
    r = (ms.worst_ratio(out.detach().cpu(), want["out"], want["mag_out"], "out"),
         ms.worst_ratio(q.grad.cpu(), want["d_uv"], want["mag_uv"], "d_uv"),
         ms.worst_ratio(t.grad.cpu(), want["d_tex"], want["mag_tex"], "d_tex"))
    print(f"texture2d {size} C={C} {boundary}: out {r[0]:.4f}, d_uv {r[1]:.4f} (KAPPA_PIXEL {ms.KAPPA_PIXEL}), d_tex {r[2]:.4f}")
    assert r[0] <= 1.0 and r[1] <= ms.KAPPA_PIXEL and r[2] <= 1.0
    if not lattice:
        assert torch.all(out[3:5] == 0) and torch.all(q.grad[3:5] == 0), "a non-finite uv row must give zeros and no gradient"
    # a batch shape in front of the 2, and the sample() form
    shaped = gs.texture2d(t, q.detach().view(-1, 1, 2)[: (uv.shape[0] // 3) * 3].view(-1, 3, 2), boundary)
    assert shaped.shape == (uv.shape[0] // 3, 3, C) and torch.equal(shaped.reshape(-1, C), out[: (uv.shape[0] // 3) * 3].detach())


def test_texture2d_sample_form():
    g = torch.Generator().manual_seed(5)
    tex = torch.rand(5, 7, 3, generator=g)
    uv = torch.rand(500, 2, generator=g) * 3.6 - 1.3
    got = gs.Texture2D(tex.to(DEV)).sample(uv.to(DEV)).cpu()
    want = ms.sample(tex.double(), uv.double())
    assert (got.double() - want).abs().max() <= 1e-4 * float(tex.max())
    const = gs.Texture2D.from_constants((0.2, 0.5, 0.7), device=DEV)
    assert torch.equal(const.sample(uv.to(DEV)).cpu(), torch.tensor([0.2, 0.5, 0.7]).expand(500, 3))


# ------------------------------------------------------------------------------------------------ render_mesh
def _sphere_scene(H, W):
    sv, sf = ref.uv_sphere(8, 16, 0.5)
    c2w, vm = ref.lookat_view(ref.EYE)
    f = 0.5 * 64 / math.tan(math.radians(ref.FOV) * 0.5)
    cam = gs.Camera(torch.as_tensor(c2w, dtype=torch.float32).to(DEV).contiguous(), f, f, 0.5 * W, 0.5 * H, W, H)
    v = torch.as_tensor(sv, dtype=torch.float32).to(DEV)
    faces = torch.as_tensor(sf).to(DEV)
    corner = torch.as_tensor(sv, dtype=torch.float32)[torch.as_tensor(sf)]                      # [F,3,3]
    uvs = torch.stack((torch.atan2(corner[..., 1], corner[..., 0]) / (2 * math.pi) + 0.5,
                       torch.acos((corner[..., 2] / 0.5).clamp(-1, 1)) / math.pi), -1).to(DEV)   # per face-vertex
    return v, faces, uvs, cam


def _materials(kd_size=(5, 7), ks_size=(2, 3)):
    g = torch.Generator().manual_seed(11)
    sc = ms.scene("1x1")
    kd = gs.Texture2D((torch.rand(*kd_size, 3, generator=g) * 0.9 + 0.05).to(DEV))
    ks = gs.Texture2D(torch.rand(*ks_size, 3, generator=g).to(DEV))
    return kd, ks, _env(sc), sc


@pytest.mark.parametrize("size", [(64, 64), (37, 53)])
def test_render_mesh_color(size):
    H, W = size
    v, f, uvs, cam = _sphere_scene(H, W)
    kd, ks, env, sc = _materials()
    vn = gs.vertex_normals(v, f)
    kw = dict(vertex_normals=vn, kd=kd, ks=ks, uvs=uvs, envmap=env, min_visibility=0.3)
    maps = gs.render_mesh(v, f, cam, outputs=("color", "alpha", "normal"), **kw)
    assert sorted(maps) == ["alpha", "color", "normal", "rast"] and maps["color"].shape == (H, W, 3)
    rast = maps["rast"]
    position, uv = gs.interpolate(v, rast, f), gs.interpolate(uvs, rast, f)
    cam_pos = cam.c2w[:, 3].to(DEV)
    direct = gs.shade_pixels(position, maps["normal"], uv, rast, kd, ks, cam_pos, env, min_visibility=0.3)
    assert torch.equal(maps["color"], direct), "render_mesh's colour is not shade_pixels on its own maps"
    assert torch.equal(maps["color"], gs.render_mesh(v, f, cam, outputs=("color", "alpha"), **kw)["color"])
    covered = rast[..., 3] > 0
    assert int(covered.sum()) > 0.1 * H * W and torch.all(maps["color"][~covered] == 0) and bool((maps["color"][covered] > 0).all())
    # the restatement on those maps
    on_maps = dict(H=H, W=W, position=position.cpu().reshape(-1, 3), normal=maps["normal"].cpu().reshape(-1, 3), uv=uv.cpu().reshape(-1, 2),
                   covered=covered.cpu().reshape(-1), kd=kd.data.cpu(), ks=ks.data.cpu(), cam=cam_pos.cpu(), lut=sc["lut"], base=sc["base"],
                   levels=sc["levels"], occlusion="texture", min_visibility=0.3, bend=False)
    want = ms.evaluate(on_maps, torch.zeros(H * W, 3), torch.float64, magnitudes=False)
    r = ms.worst_ratio(maps["color"].cpu().reshape(-1, 3), want["color"], want["mag_color"], "colour")
    print(f"render_mesh {H}x{W}: colour {r:.4f} of 1e-4 x magnitude on {int(covered.sum())} pixels")
    assert r <= 1.0
    # antialias: colour joins the image that goes through the pass
    topo = gs.mesh_edge_topology(f)
    aa = gs.render_mesh(v, f, cam, outputs=("color", "alpha"), antialias=True, topology=topo, **kw)
    vc = gs.meshrender.to_camera_space(v, cam)
    assert torch.equal(aa["color"], gs.antialias(maps["color"], rast, vc, f, cam, topology=topo, cull="back"))
    assert torch.equal(aa["alpha"], gs.antialias(maps["alpha"], rast, vc, f, cam, topology=topo, cull="back"))
    assert bool((aa["color"] != maps["color"]).any())
    # a call without 'color' returns what it returned before, whatever materials it is given
    plain, given = gs.render_mesh(v, f, cam, vertex_normals=vn), gs.render_mesh(v, f, cam, **kw)
    assert sorted(plain) == ["alpha", "depth", "face", "normal", "rast"] == sorted(given)
    for k in plain:
        assert torch.equal(plain[k], given[k]), k


def test_antialias_does_not_depend_on_the_channel_count():
    """a channel's bits are the same whether it is antialiased alone or inside a wider image, forward and backward (the blend is
    explicit FMAs: left to contraction, vectorised channel pairs were fused and an odd last channel was not)"""
    v, f, _, cam = _sphere_scene(64, 64)
    vc = gs.meshrender.to_camera_space(v, cam)
    rast = gs.rasterize_mesh(vc, f, cam, cull="back")
    topo = gs.mesh_edge_topology(f)
    g = torch.Generator().manual_seed(9)
    wide = (torch.rand(64, 64, 5, generator=g) + 0.25).to(DEV)
    cot = torch.randn(64, 64, 5, generator=g).to(DEV)

    def run(channels):
        color = wide[..., channels].contiguous().requires_grad_()
        out = gs.antialias(color, rast, vc, f, cam, topology=topo, cull="back")
        (out * cot[..., channels]).sum().backward()
        return out.detach(), color.grad

    out5, grad5 = run(slice(0, 5))
    assert bool((out5 != wide).any())
    for channels in (slice(0, 3), slice(0, 4), slice(2, 3), slice(4, 5), slice(1, 4)):
        out, grad = run(channels)
        assert torch.equal(out, out5[..., channels]) and torch.equal(grad, grad5[..., channels]), channels


def test_render_mesh_color_arguments_and_constants():
    v, f, uvs, cam = _sphere_scene(64, 64)
    kd, ks, env, _ = _materials()
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("color",))                                          # no materials
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("color",), kd=kd, ks=ks, envmap=env)                # uvs=None with textures larger than 1x1
    with pytest.raises(ValueError):
        gs.render_mesh(v, f, cam, outputs=("color",), kd=kd, ks=ks, uvs=uvs, envmap=env, occlusion="ssao")
    # PrettyShader(occlusion_type='none'): constant materials, no uvs, flat normals, through the model-level pass-through
    const_kd = gs.Texture2D.from_constants((0.7, 0.6, 0.5), device=DEV)
    const_ks = gs.Texture2D.from_constants((0.0, 0.25, 0.0), device=DEV)
    maps = gs.render_mesh(v, f, cam, outputs=("color", "alpha"), normal_type="flat", kd=const_kd, ks=const_ks, envmap=env, occlusion="none")
    covered = maps["rast"][..., 3] > 0
    assert torch.all(maps["color"][covered] > 0) and torch.all(maps["color"][~covered] == 0)
    model = gs.GSplatModel.__new__(gs.GSplatModel)
    via = gs.GSplatModel.render_mesh(model, cam, v, f, outputs=("color", "alpha"), normal_type="flat", kd=const_kd, ks=const_ks, envmap=env,
                                     occlusion="none")
    assert torch.equal(via["color"], maps["color"])


def test_a_texture_is_fitted_through_the_render():
    """sixty Adam steps on a 16x16 kd texture under a fixed environment; without the gradient to kd.data nothing could move"""
    v, f, uvs, cam = _sphere_scene(64, 64)
    _, ks, env, _ = _materials()
    g = torch.Generator().manual_seed(3)
    target_kd = gs.Texture2D((torch.rand(16, 16, 3, generator=g) * 0.6 + 0.2).to(DEV))
    vn = gs.vertex_normals(v, f)
    render = lambda kd: gs.render_mesh(v, f, cam, outputs=("color",), vertex_normals=vn, kd=kd, ks=ks, uvs=uvs, envmap=env)["color"]
    with torch.no_grad():
        target = render(target_kd)
    kd = gs.Texture2D(torch.full((16, 16, 3), 0.5, device=DEV, requires_grad=True))
    opt = torch.optim.Adam([kd.data], lr=0.03)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = (render(kd) - target).abs().mean()
        loss.backward()
        assert kd.data.grad is not None and bool((kd.data.grad != 0).any())
        losses.append(float(loss.detach()))
        opt.step()
    print(f"L1 to the target render {losses[0]:.5f} -> {losses[-1]:.5f} ({losses[-1] / losses[0]:.4f} of its start)")
    assert losses[-1] < 0.1 * losses[0]
