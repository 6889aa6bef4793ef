"""No-GPU checks of the mesh shading restatement tests/meshshade_ref.py (the reference of tests/test_gpu_meshshade.py) and of the
argument validation of its entry points.

  * the wrap lookup against hand-computed values, its period, texel centres, and torch's grid_sample on the circularly padded texture;
  * the pixel arithmetic with occlusion='none' against oracle/torch_ref.shade (the golden-pinned restatement of the per-Gaussian
    shader): diffuse + specular with min_roughness = 0, max_metallic = 1, on pixels with d >= 1e-4, to 1e-12 in float64;
  * every scene the GPU tests use: at most 5 % of the shaded pixels are fragile, every cube face and every mip interval occurs;
  * the restatement evaluated in FLOAT32 ON THE CPU against float64 under the bounds of the GPU tests: an fp32 implementation can
    meet them.  This run sets the one constant, meshshade_ref.KAPPA_PIXEL (the smallest power of two >= 2 x the worst per-pixel
    gradient ratio).  Measured over the five scenes, dense and single-channel cotangents: per-pixel gradients at most 2.91 of
    1e-4 x magnitude, hence KAPPA_PIXEL = 8; forward 0.27, texel gradients 0.112;
  * the share of ill-conditioned pixels (meshshade_ref.ill_conditioned): at most 2 % with the dense cotangent, 12 % with one channel.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr
from tests import meshshade_ref as ms

NAMES = sorted(ms.SCENES)


# ------------------------------------------------------------------------------------------------ the wrap lookup
def _tex23():
    return torch.arange(6, dtype=torch.float64).reshape(2, 3, 1)                  # t[y, x] = 3 y + x


@pytest.mark.parametrize("uv, want", [
    ((0.5, 0.25), 1.0),            # x = 1, y = 0: the texel (0, 1) itself
    ((0.1, 0.25), 0.4),            # x = -0.2: ix0 = -1, fx = 0.8, taps x = 2 and x = 0 of row 0: 2 + 0.8 (0 - 2)
    ((-0.9, 0.25), 0.4),           # the same point one period to the left
    ((2.0, 0.25), 1.0),            # u an integer: u' = 0, x = -0.5, ix0 = -1, fx = 0.5: 2 + 0.5 (0 - 2)
    ((0.5, 0.0), 2.5),             # y = -0.5: iy0 = -1, rows 1 and 0, fy = 0.5: 4 + 0.5 (1 - 4)
    ((0.5, 1.0), 2.5),             # v an integer
    ((5.0 / 6.0, 0.75), 5.0),      # the last texel's centre
    ((0.95, 0.75), 5.0 + 0.35 * (3.0 - 5.0)),   # x = 2.35: taps x = 2 and x = 3 mod 3 = 0 of row 1
])
def test_wrap_lookup_by_hand(uv, want):
    got = ms.texture2d(_tex23(), torch.tensor([uv], dtype=torch.float64), "wrap")
    assert abs(float(got) - want) <= 1e-12


def test_wrap_lookup_period_centres_and_non_finite_rows():
    g = torch.Generator().manual_seed(1)
    tex = torch.rand(5, 7, 3, generator=g, dtype=torch.float64)
    uv = torch.rand(200, 2, generator=g, dtype=torch.float64) * 3.6 - 1.3
    for k in (-3.0, 1.0, 2.0):
        assert (ms.texture2d(tex, uv) - ms.texture2d(tex, uv + k)).abs().max() <= 1e-12
    iy, ix = torch.meshgrid(torch.arange(5), torch.arange(7), indexing="ij")
    centres = torch.stack(((ix.double() + 0.5) / 7, (iy.double() + 0.5) / 5), -1).reshape(-1, 2)
    assert (ms.texture2d(tex, centres) - tex.reshape(-1, 3)).abs().max() <= 1e-14
    assert (ms.texture2d(tex, centres, "clamp") - tex.reshape(-1, 3)).abs().max() <= 1e-14
    bad = torch.tensor([[float("nan"), 0.3], [0.2, float("inf")]], dtype=torch.float64, requires_grad=True)
    tex.requires_grad_()
    out = ms.texture2d(tex, bad)
    out.sum().backward()
    assert torch.all(out == 0) and torch.all(bad.grad == 0) and torch.all(tex.grad == 0)


@pytest.mark.parametrize("size", [(2, 3), (5, 7), (1, 1), (4, 8)])
def test_wrap_lookup_equals_grid_sample_on_the_padded_texture(size):
    Ht, Wt = size
    g = torch.Generator().manual_seed(2)
    tex = torch.rand(Ht, Wt, 3, generator=g, dtype=torch.float64)
    uv = torch.rand(300, 2, generator=g, dtype=torch.float64)                     # [0, 1)
    padded = F.pad(tex.permute(2, 0, 1)[None], (1, 1, 1, 1), mode="circular")     # [1, 3, Ht + 2, Wt + 2]
    x, y = uv[:, 0] * Wt - 0.5 + 1.0, uv[:, 1] * Ht - 0.5 + 1.0                   # pixel coordinates in the padded texture
    grid = torch.stack(((2 * x + 1) / (Wt + 2) - 1, (2 * y + 1) / (Ht + 2) - 1), -1)[None, None]
    want = F.grid_sample(padded, grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].T
    assert (ms.texture2d(tex, uv) - want).abs().max() <= 1e-12


def test_sample_of_a_constant_texture_has_no_uv_gradient():
    tex = torch.tensor([0.2, 0.5, 0.7], dtype=torch.float64).view(1, 1, 3)
    uv = (torch.rand(50, 2, dtype=torch.float64) * 3.6 - 1.3).requires_grad_()
    out = ms.sample(tex, uv)
    out.sum().backward()
    assert torch.all(out == tex.view(1, 3)) and torch.all(uv.grad == 0)


# ------------------------------------------------------------------------------------------------ the pixel arithmetic
def test_pixel_arithmetic_equals_the_per_gaussian_shader():
    sc = ms.scene("64x64 none")
    m = ms.shaded_mask(sc)
    f64 = lambda t: t.double()
    pos, nrm, uv = f64(sc["position"][m]), f64(sc["normal"][m]), f64(sc["uv"][m])
    kd_s, ks_s = ms.sample(f64(sc["kd"]), uv), ms.sample(f64(sc["ks"]), uv)
    levels = [f64(l) for l in sc["levels"]]
    t_diff, t_spec = ms._terms(pos, nrm, uv, f64(sc["kd"]), f64(sc["ks"]), f64(sc["cam"]), f64(sc["lut"]), f64(sc["base"]), levels,
                               "none", 0.0, False)
    args = (pos, nrm, kd_s, ks_s[:, 1:3], f64(sc["cam"]), f64(sc["lut"]), f64(sc["base"]), levels)
    want = sum(tr.shade(*args, min_roughness=0.0, max_metallic=1.0, mode=mode, env_min_r=ms.MIN_R, env_max_r=ms.MAX_R)
               for mode in ("diffuse", "specular"))
    d = (nrm * tr.safe_normalize(f64(sc["cam"]) - pos)).sum(-1)
    keep = d >= 1e-4
    assert int(keep.sum()) > 2000 and int((~keep).sum()) > 100
    assert ((t_diff + t_spec) - want)[keep].abs().max() <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_scenes_are_rarely_fragile_and_cover_every_selection(name):
    sc = ms.scene(name)
    m = ms.shaded_mask(sc)
    share = float(ms.fragile(name)[m].double().mean())
    print(f"{name}: {int(m.sum())} shaded pixels of {m.numel()}, fragile share {share:.4f}")
    assert share <= 0.05
    assert not bool(ms.fragile(name)[~m].any())
    for kind, cap in (("dense", 0.02), ("single", 0.12)):
        ill = ms.ill_conditioned(name, kind)
        print(f"{name} / {kind}: ill-conditioned share {float(ill[m].double().mean()):.4f}")
        assert float(ill[m].double().mean()) <= cap and not bool((ill & ms.fragile(name)).any()) and not bool(ill[~m].any())
    if m.numel() < 1000:
        return
    assert 0.1 < 1.0 - float(sc["covered"].double().mean()) < 0.3                  # about a fifth is empty
    kept = {}
    with torch.no_grad():
        ms._terms(sc["position"][m].double(), sc["normal"][m].double(), sc["uv"][m].double(), sc["kd"].double(), sc["ks"].double(),
                  sc["cam"].double(), sc["lut"].double(), sc["base"].double(), [l.double() for l in sc["levels"]], sc["occlusion"],
                  sc["min_visibility"], sc["bend"], lambda **kw: kept.update(kw))
    assert sorted(tr._select_face(kept["normal"]).unique().tolist()) == list(range(6))
    assert sorted(tr._select_face(kept["refl"]).unique().tolist()) == list(range(6))
    if tuple(sc["ks"].shape[:2]) != (1, 1):
        l0, l1, free = ms.mip_levels(kept["rough"], ms.MIN_R, ms.MAX_R, len(ms.ENV_LEVELS))
        assert sorted(l0.unique().tolist()) == [0, 1] or sorted(l0.unique().tolist()) == [0, 1, 2]
        r = kept["rough"]
        assert bool((r < ms.MIN_R).any()) and bool(((r > ms.MIN_R) & (r < ms.MAX_R)).any()) and bool((r > ms.MAX_R).any())
    if sc["bend"]:
        d0 = (sc["normal"][m] * tr.safe_normalize(sc["cam"] - sc["position"][m])).sum(-1)
        assert 0.25 < float((d0 < 0).double().mean()) < 0.42


# ------------------------------------------------------------------------------------------------ float32 on the CPU under the bounds
def test_float32_on_the_cpu_meets_the_bounds_and_sets_kappa():
    worst = [0.0, 0.0, 0.0]
    for name in NAMES:
        for kind in ("dense", "single"):
            cot, want = ms.reference(name, kind)
            got = ms.evaluate(ms.scene(name), cot, torch.float32, magnitudes=False)
            r = ms.ratios(got, want)
            print(f"{name} / {kind}: forward {r[0]:.3f}, per-pixel gradients {r[1]:.3f}, texel gradients {r[2]:.3f} of 1e-4 x magnitude")
            worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"worst: forward {worst[0]:.3f}, per-pixel {worst[1]:.3f}, texel {worst[2]:.3f}; KAPPA_PIXEL = {ms.KAPPA_PIXEL}")
    assert worst[0] <= 1.0 and worst[2] <= 1.0
    assert ms.KAPPA_PIXEL == ms.smallest_power_of_two_at_least(2.0 * ms.MEASURED_PIXEL) and ms.KAPPA_PIXEL >= 1.0
    assert worst[1] <= ms.KAPPA_PIXEL / 2.0, "the float32 restatement no longer leaves a factor two below KAPPA_PIXEL"


# ------------------------------------------------------------------------------------------------ argument validation
def test_entry_points_validate_before_touching_the_device():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    i64, f32 = ctypes.c_int64, ctypes.c_float
    one = ctypes.c_void_p(64)                                                     # a non-null pointer that is never read
    err = lambda: lib.gs_last_error()
    assert lib.gs_tex2d_fwd(i64(4), 2, 3, 5, 0, one, one, one, None) == -1 and b"C must be in 1..4" in err()
    assert lib.gs_tex2d_fwd(i64(4), 2, 3, 0, 0, one, one, one, None) == -1 and b"C must be in 1..4" in err()
    assert lib.gs_tex2d_fwd(i64(4), 0, 3, 3, 0, one, one, one, None) == -1 and b"texture size" in err()
    assert lib.gs_tex2d_bwd(i64(4), 2, -1, 3, 0, one, one, one, one, one, None) == -1 and b"texture size" in err()
    assert lib.gs_tex2d_fwd(i64(4), 2, 3, 3, 2, one, one, one, None) == -1 and b"boundary" in err()
    assert lib.gs_tex2d_bwd(i64(4), 2, 3, 3, -1, one, one, one, one, one, None) == -1 and b"boundary" in err()
    assert lib.gs_tex2d_fwd(i64(4), 2, 3, 3, 0, None, one, one, None) == -1 and b"null" in err()
    assert lib.gs_tex2d_bwd(i64(4), 2, 3, 3, 0, one, one, one, one, None, None) == -1 and b"null" in err()
    assert lib.gs_tex2d_fwd(i64(-1), 2, 3, 3, 0, one, one, one, None) == -1
    assert lib.gs_tex2d_fwd(i64(0), 2, 3, 3, 0, None, None, None, None) == 0      # P = 0: a no-op
    assert lib.gs_tex2d_bwd(i64(0), 2, 3, 3, 1, None, None, None, None, None, None) == 0

    env = _lib.GsEnv()
    env.lut = 64; env.lut_res = 256; env.base = 64; env.base_res = 16; env.num_levels = 3
    for l, r in enumerate((64, 32, 16)):
        env.levels[l] = 64; env.res[l] = r
    env.min_roughness = 0.08; env.max_roughness = 0.5
    e = ctypes.byref(env)

    def fwd(H=4, W=4, kd=(2, 3), ks=(1, 1), occ=0, rast=one, color=one, env_p=e):
        return lib.gs_meshshade_fwd(H, W, rast, one, one, one, kd[0], kd[1], one, ks[0], ks[1], one, one, env_p, occ, f32(0.0), 0, color, None)

    def bwd(H=4, W=4, kd=(2, 3), ks=(1, 1), occ=0, d_kd=one, eg=None):
        return lib.gs_meshshade_bwd(H, W, one, one, one, one, kd[0], kd[1], one, ks[0], ks[1], one, one, e, occ, f32(0.0), 0, one, one, one,
                                    one, d_kd, one, eg, None)

    assert fwd(H=0) == -1 and b"image size" in err()
    assert fwd(W=-2) == -1 and b"image size" in err()
    assert bwd(H=0) == -1 and b"image size" in err()
    assert fwd(kd=(0, 3)) == -1 and b"texture size" in err()
    assert bwd(ks=(1, 0)) == -1 and b"texture size" in err()
    assert fwd(occ=2) == -1 and b"occlusion" in err()
    assert bwd(occ=-1) == -1 and b"occlusion" in err()
    assert fwd(rast=None) == -1 and b"null" in err()
    assert fwd(color=None) == -1 and b"null" in err()
    assert fwd(env_p=None) == -1 and b"GsEnv" in err()
    assert bwd(eg=None) == -1 and b"null" in err()
    grads = _lib.GsEnvGrad()
    grads.base = 64
    assert bwd(eg=ctypes.byref(grads)) == -1 and b"levels" in err()               # a level's gradient buffer is missing
    for l in range(3):
        grads.levels[l] = 64
    assert bwd(d_kd=None, eg=ctypes.byref(grads)) == -1 and b"null" in err()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.texture2d(torch.rand(2, 3, 3), torch.rand(5, 2))
    with pytest.raises(ValueError):
        gs.texture2d(torch.rand(2, 3, 3), torch.rand(5, 2), boundary_mode="mirror")
    with pytest.raises(GeoSplatHipError):
        gs.Texture2D(torch.rand(2, 3, 4))
    tex = gs.Texture2D.from_constants((0.1, 0.2, 0.3))
    assert tex.data.shape == (1, 1, 3) and (tex.height, tex.width) == (1, 1)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        tex.sample(torch.rand(5, 2))
    env = gs.TextureSplitSum(torch.rand(6, 16, 16, 3), [torch.rand(6, r, r, 3) for r in (64, 32, 16)])
    z = torch.zeros(4, 4, 3)
    with pytest.raises(ValueError):
        gs.shade_pixels(z, z, z[..., :2], torch.zeros(4, 4, 4), tex, tex, torch.zeros(3), env, occlusion="ssao")
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.shade_pixels(z, z, z[..., :2], torch.zeros(4, 4, 4), tex, tex, torch.zeros(3), env)
