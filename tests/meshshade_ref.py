"""Restatement of the mesh shading semantics (geosplatting_amd/meshshade.py, csrc/gs_meshshade.hip; stated in include/geosplat_hip.h)
on oracle/torch_ref.py's dtype-generic pieces (tex2d_linear_clamp, cube_linear, cube_mip_linear, mip_from_roughness, safe_normalize),
plus the wrap lookup and the per-pixel arithmetic.  CPU torch; float64 is the reference, float32 shows what an fp32 implementation can
reach.  Test infrastructure; it shares no code with the kernels.

`evaluate(scene, cot, dtype)` returns the colour, the gradients of sum(cot * colour) by autograd, and the MAGNITUDES the bounds of
tests/test_gpu_meshshade.py are multiples of:
  forward     per element (|l_diff diff| + |l_spec R|) visibility
  per pixel   for d_position, d_normal, d_uv: the sum of the absolute values of six autograd passes, one per (diffuse term |
              specular term) x colour channel, so that neither cross-term nor cross-channel cancellation shrinks the bound
  per texel   for kd, ks, base and the levels: the scatter of the ABSOLUTE cotangent of the sampled value with every tap weight (and,
              for the levels, the trilinear fraction) replaced by 1, each distinct tap of a pixel counted once.  A float32 texel
              coordinate at <= 64 texels carries about 1e-5 of rounding: an ABSOLUTE error of the weight, which no bound proportional
              to a tiny weight can absorb.
`fragile(scene)` flags the pixels where some selection lies within DELTA of switching: a kd or ks texel coordinate or wrap seam (a
dimension of size 1 selects nothing), a LUT cell coordinate, the mip level (the roughness bounds are its integers), a cube texel
coordinate of base or of the levels in use, the cube face (the gap of the two largest |components|, in texels of the largest face in
use), d at 1e-4 (at 0 with the bend) and 1 - ks[0] at min_visibility (both as LUT cells: DELTA / 256).  DELTA = 1e-3 in texel / cell /
level units.

Per-pixel magnitudes are per ELEMENT, with one exception: under a cotangent with a single non-zero colour channel d_position has ONE
non-zero pass (the diffuse term does not depend on the position).  That pass is the projection v - wo (wo . v) of a cotangent onto the
plane across the view direction; a float32 rounding of it is relative to the vector, and nothing else covers a component that happens
to be small.  There, and only there, the magnitude is the largest component of the pixel's vector.  Float32 CPU restatement, worst ratio
to 1e-4 x magnitude before any pixel is flagged as ill-conditioned (below): per element everywhere 279 (d_position, single channel),
13 (d_normal), 5.2 (d_uv), dense 2.2; per vector everywhere 11.3; per element with the one exception 13.

`ill_conditioned(scene, kind)`.  What made single pixels outliers (11.3 on one pixel of '64x64 constants') is not a selection: the
slope of a bilinear patch, (t10 - t00) + fy ((t11 - t01) - (t10 - t00)), crosses zero inside a cell of a random texture, and the
specular direction gradient is a sum of such slopes over two levels and two axes.  Near a zero the float64 gradient itself is not
determined to the tolerance by float32 data: a float32 texel coordinate at <= 64 texels carries 4e-6 of rounding, which moves the slope
by an amount that does not shrink with it.  A pixel is ill-conditioned when perturbing position, normal and uv by PERTURB = 2^-23
relative (one float32 rounding of the inputs; two random draws) moves an element of the FLOAT64 gradients d_position, d_normal or d_uv
by more than 1e-4 of its magnitude, the base tolerance itself.  Its cotangent is zeroed, as on a fragile pixel.  The flag comes from
float64 alone.  Shares of the shaded pixels: at most 1.1 % with the dense cotangent, 2.2 - 10.6 % with the single-channel one
(tests/test_meshshade_cpu.py caps them at 2 % and 12 %; the fragile cap stays 5 %).

Scenes.  ks textures are at most 5 x 7, the 64 x 64 texture is a kd.  A 64 x 64 ks texel is reached by one pixel or none, so its bound
is proportional to that pixel's cotangent of the ks sample, and that cotangent is itself a difference: below min_roughness the roughness
part is a pure FG-LUT slope where neighbouring LUT rows differ by 1e-6 .. 1e-9 of their values, and the metallic part is
sum_c v_spec (kd - 0.04) - v_diff kd.  Tried and measured with the float32 CPU restatement: a 64 x 64 ks with any roughness misses the
texel bound by 583x; with roughness kept in [0.1, 0.98] by 5.5x (dense) and 14.7x (single channel); flagging pixels whose sample
cotangent moves under the perturbation above flags 7 - 15 % of every scene and still leaves 1.75x.  On a small ks texture every texel
sums hundreds of pixels.  The scatter paths of kd and ks are the same device function.

KAPPA_PIXEL is the smallest power of two that is at least twice the worst per-pixel-gradient ratio |fp32 - fp64| / (1e-4 magnitude) of
this restatement evaluated in float32 ON THE CPU over all scenes and both cotangents -- derived from the restatement, never from the
kernel.  Measured (tests/test_meshshade_cpu.py prints them): 2.91, hence 8; forward at most 0.27, texel gradients at most 0.112.
"""
import functools
import math
import os

import numpy as np
import torch

from oracle import torch_ref as tr

DELTA = 1e-3
KAPPA_PIXEL = 8.0
MEASURED_PIXEL, MEASURED_FORWARD, MEASURED_TEXEL = 2.91, 0.27, 0.112     # (float32 CPU run: tests/test_meshshade_cpu.py prints them)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 2-D lookups
def wrap_taps(Ht, Wt, uv):
    """uv [n,2] (finite) -> (idx [4] long tensors of t00 t10 t01 t11, x, y): the wrap lookup's coordinates"""
    up = uv - uv.detach().floor()
    x = up[:, 0] * Wt - 0.5
    y = up[:, 1] * Ht - 0.5
    ix0 = x.detach().floor().long()
    iy0 = y.detach().floor().long()
    jx0, jx1 = torch.remainder(ix0, Wt), torch.remainder(ix0 + 1, Wt)
    jy0, jy1 = torch.remainder(iy0, Ht), torch.remainder(iy0 + 1, Ht)
    return [jy0 * Wt + jx0, jy0 * Wt + jx1, jy1 * Wt + jx0, jy1 * Wt + jx1], x, y


def texture2d(tex, uv, boundary_mode="wrap"):
    """tex [Ht,Wt,C], uv [n,2] -> [n,C]; a non-finite uv row gives zeros and no gradient"""
    Ht, Wt, C = tex.shape
    finite = torch.isfinite(uv).all(-1)
    uvz = torch.where(finite[:, None], uv, torch.zeros_like(uv))
    if boundary_mode == "clamp":
        out = tr.tex2d_linear_clamp(tex, uvz)
    else:
        idx, x, y = wrap_taps(Ht, Wt, uvz)
        fx = (x - x.detach().floor())[:, None]
        fy = (y - y.detach().floor())[:, None]
        flat = tex.reshape(-1, C)
        top = flat[idx[0]] + fx * (flat[idx[1]] - flat[idx[0]])
        bot = flat[idx[2]] + fx * (flat[idx[3]] - flat[idx[2]])
        out = top + fy * (bot - top)
    return torch.where(finite[:, None], out, torch.zeros_like(out))


def sample_coords(Ht, Wt, uv):
    """Texture2D.sample's lookup coordinates"""
    return torch.stack((uv[:, 0] * (1.0 - 1.0 / Wt) + 0.5 / Wt, uv[:, 1] * (1.0 - 1.0 / Ht) + 0.5 / Ht), -1)


def sample(tex, uv):
    return texture2d(tex, sample_coords(tex.shape[0], tex.shape[1], uv), "wrap")


def cube_taps(R, d):
    """d [n,3] -> (idx [4] long tensors, -1 the missing corner; tx, ty texel coordinates): cube_linear's footprint"""
    d = d.detach()
    face = tr._select_face(d)
    x, y = tr._face_coords(d, face)
    tx = (x + 1) * 0.5 * R - 0.5
    ty = (y + 1) * 0.5 * R - 0.5
    ix0, iy0 = tx.floor().long(), ty.floor().long()
    idx = [tr._resolve(face, ix0 + ox, iy0 + oy, R, d.dtype) for (ox, oy) in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return idx, tx, ty


def mip_levels(rough, min_r, max_r, L):
    """-> (l0, l1 (-1: one level), unclamped mip value)"""
    r = rough.detach()
    mip = tr.mip_from_roughness(r, min_r, max_r, L)
    free = torch.where(r < max_r, (r - min_r) / (max_r - min_r) * (L - 2), (r - max_r) / (1.0 - max_r) + (L - 2))
    l0 = mip.clamp(0, L - 1).floor().long().clamp(max=L - 1)
    l1 = torch.where(l0 < L - 1, l0 + 1, torch.full_like(l0, -1))
    return l0, l1, free


# ------------------------------------------------------------------------------------------------ scenes
def fg_lut():
    path = os.path.join(ROOT, "geosplatting_amd", "assets", "fg_lut_256.bin")
    return torch.from_numpy(np.fromfile(path, dtype=np.float32).reshape(256, 256, 2).copy())


SCENES = {
    # name: (H, W, kd size, ks size, occlusion, min_visibility, bend_back_normal, share of normals facing away)
    "1x1": (1, 1, (2, 3), (5, 7), "texture", 0.0, False, 0.0),
    "37x53 textured": (37, 53, (5, 7), (2, 3), "texture", 0.3, False, 0.15),
    "64x64 none": (64, 64, (64, 64), (5, 7), "none", 0.0, False, 0.15),
    "64x64 constants": (64, 64, (1, 1), (1, 1), "texture", 0.0, False, 0.15),
    "37x53 bend": (37, 53, (64, 64), (2, 3), "texture", 0.3, True, 1.0 / 3.0),
}
ENV_LEVELS = (64, 32, 16)
ENV_BASE = 16
MIN_R, MAX_R = 0.08, 0.5


@functools.lru_cache(maxsize=None)
def scene(name):
    """float32 inputs of one G-buffer: random texels (neighbours differ by the order of their values), uv in [-1.3, 2.3], about a fifth
    of the pixels empty, positions on a shell around the camera so that normals and reflections reach every cube face, a few pixels
    with a non-finite position, normal or uv (images of more than one pixel)."""
    H, W, kd_size, ks_size, occlusion, min_vis, bend, away = SCENES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *s: torch.rand(*s, generator=g)
    n = H * W
    cam = torch.tensor([0.1, 0.2, -0.1])
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    position = cam + dirs * (1.0 + 2.0 * rnd(n, 1))
    wo = -dirs
    normal = torch.nn.functional.normalize(wo + 0.8 * torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1), dim=-1)
    flip = rnd(n) < away
    normal = torch.where(flip[:, None], -normal, normal)
    uv = rnd(n, 2) * 3.6 - 1.3
    covered = rnd(n) >= 0.2
    if n == 1:
        covered[:] = True
    bad = torch.zeros(n, dtype=torch.bool)
    if n > 8:
        position[3, 1] = float("nan"); normal[5, 0] = float("inf"); uv[7, 1] = float("nan"); uv[8, 0] = float("-inf")
        bad[[3, 5, 7, 8]] = True
        covered[[3, 5, 7, 8]] = True
    kd = rnd(*kd_size, 3) * 0.9 + 0.05
    ks = rnd(*ks_size, 3)
    if ks_size == (1, 1):
        ks = torch.tensor([0.25, 0.31, 0.6]).view(1, 1, 3)
    else:                                          # roughness below and above the environment's bounds occurs in every textured scene
        ks[0, 0, 1] = 0.02
        ks[-1, -1, 1] = 0.95
    base = rnd(6, ENV_BASE, ENV_BASE, 3) + 0.2
    levels = tuple(rnd(6, r, r, 3) + 0.2 for r in ENV_LEVELS)
    return dict(name=name, H=H, W=W, position=position, normal=normal, uv=uv, covered=covered, bad=bad, kd=kd, ks=ks, cam=cam,
                lut=fg_lut(), base=base, levels=levels, occlusion=occlusion, min_visibility=min_vis, bend=bend)


def cotangents(sc, kind):
    """'dense': a random cotangent in every channel; 'single': channel 1 alone"""
    g = torch.Generator().manual_seed(7 + sc["H"])
    cot = torch.randn(sc["H"] * sc["W"], 3, generator=g)
    if kind == "single":
        cot[:, 0] = 0.0
        cot[:, 2] = 0.0
    return cot


# ------------------------------------------------------------------------------------------------ the shader
def _terms(position, normal, uv, kd, ks, cam, lut, base, levels, occlusion, min_visibility, bend, hook=None):
    """the shaded pixels [m, ...] -> (diffuse term, specular term) [m,3], colour = their sum; `hook` receives the sampled values"""
    kd_s, ks_s = sample(kd, uv), sample(ks, uv)
    rough, metal = ks_s[:, 1:2], ks_s[:, 2:3]
    spec = (1.0 - metal) * 0.04 + kd_s * metal
    diff = kd_s * (1.0 - metal)
    wo = tr.safe_normalize(cam - position)
    d = (normal * wo).sum(-1, keepdim=True)
    if bend:
        normal = torch.where(d.detach() > 0, normal, -normal)
        d = (normal * wo).sum(-1, keepdim=True)
        ndv = d
    else:
        ndv = d.clamp(min=1e-4)
    fg = tr.tex2d_linear_clamp(lut, torch.cat([ndv, rough], -1))
    refl = 2 * d * normal - wo
    l_diff = tr.cube_linear(base, normal)
    l_spec = tr.cube_mip_linear(list(levels), refl, tr.mip_from_roughness(rough[:, 0], MIN_R, MAX_R, len(levels)))
    if hook is not None:
        hook(kd_s=kd_s, ks_s=ks_s, l_diff=l_diff, l_spec=l_spec, normal=normal, refl=refl, d=d, rough=rough[:, 0])
    reflectance = spec * fg[:, 0:1] + fg[:, 1:2]
    vis = (1.0 - ks_s[:, 0:1]).clamp(min=min_visibility) if occlusion == "texture" else torch.ones_like(rough)
    return l_diff * diff * vis, l_spec * reflectance * vis


def shaded_mask(sc):
    finite = torch.isfinite(sc["position"]).all(-1) & torch.isfinite(sc["normal"]).all(-1) & torch.isfinite(sc["uv"]).all(-1)
    return sc["covered"] & finite


def _scatter_abs(size, taps, v):
    """sum of |v| [m,3] over the DISTINCT taps of every pixel -> [size,3]"""
    out = torch.zeros(size, 3, dtype=v.dtype)
    seen = []
    for i in taps:
        ok = i >= 0
        for j in seen:
            ok = ok & (i != j)
        out.index_add_(0, i[ok], v.abs()[ok])
        seen.append(i)
    return out


def evaluate(sc, cot, dtype=torch.float64, magnitudes=True):
    """-> dict(color [n,3], mag_color, grad {...}, mag {...}) for the cotangent `cot` [n,3]; every array flattened over the pixels"""
    m = shaded_mask(sc)
    n = m.numel()
    to = lambda t: t.detach().to(dtype).clone()
    leaves = dict(position=to(sc["position"][m]).requires_grad_(), normal=to(sc["normal"][m]).requires_grad_(),
                  uv=to(sc["uv"][m]).requires_grad_(), kd=to(sc["kd"]).requires_grad_(), ks=to(sc["ks"]).requires_grad_(),
                  base=to(sc["base"]).requires_grad_())
    levels = [to(l).requires_grad_() for l in sc["levels"]]
    kept = {}

    def hook(**kw):
        for k in ("kd_s", "ks_s", "l_diff", "l_spec"):
            kw[k].retain_grad()
        kept.update(kw)

    t_diff, t_spec = _terms(leaves["position"], leaves["normal"], leaves["uv"], leaves["kd"], leaves["ks"], to(sc["cam"]), to(sc["lut"]),
                            leaves["base"], levels, sc["occlusion"], sc["min_visibility"], sc["bend"], hook)
    g = to(cot[m])

    def expand(x):
        out = torch.zeros(n, *x.shape[1:], dtype=dtype)
        out[m] = x.detach()
        return out

    res = dict(color=expand(t_diff + t_spec), mag_color=expand(t_diff.abs() + t_spec.abs()), shaded=m)
    per_pixel = [leaves["position"], leaves["normal"], leaves["uv"]]
    mag = {}
    if magnitudes:
        acc = [torch.zeros_like(x) for x in per_pixel]
        for term in (t_diff, t_spec):
            for c in range(3):
                parts = torch.autograd.grad((g[:, c] * term[:, c]).sum(), per_pixel, retain_graph=True, allow_unused=True)
                for a, p in zip(acc, parts):
                    if p is not None:
                        a += p.abs()
        if int((g != 0).any(0).sum()) == 1:
            # one colour channel: d_position has ONE non-zero pass (the diffuse term does not depend on the position), a vector in
            # the plane across the view direction whose float32 rounding is relative to the vector, not to its smallest component
            acc[0] = acc[0].amax(-1, keepdim=True).expand_as(acc[0])
        mag.update(position=expand(acc[0]), normal=expand(acc[1]), uv=expand(acc[2]))
    for k in ("kd_s", "ks_s", "l_diff", "l_spec"):
        kept[k].grad = None                        # (the six passes above also left their sums in the retained gradients)
    (g * (t_diff + t_spec)).sum().backward()
    zero = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    res["grad"] = dict(position=expand(zero(leaves["position"])), normal=expand(zero(leaves["normal"])), uv=expand(zero(leaves["uv"])),
                       kd=zero(leaves["kd"]), ks=zero(leaves["ks"]), base=zero(leaves["base"]), levels=[zero(l) for l in levels])
    if magnitudes:
        uv = leaves["uv"].detach()
        for name in ("kd", "ks"):
            Ht, Wt = sc[name].shape[:2]
            taps, _, _ = wrap_taps(Ht, Wt, sample_coords(Ht, Wt, uv))
            mag[name] = _scatter_abs(Ht * Wt, taps, kept[name + "_s"].grad).reshape(Ht, Wt, 3)
        taps, _, _ = cube_taps(ENV_BASE, kept["normal"])
        mag["base"] = _scatter_abs(6 * ENV_BASE ** 2, taps, kept["l_diff"].grad).reshape(6, ENV_BASE, ENV_BASE, 3)
        l0, l1, _ = mip_levels(kept["rough"], MIN_R, MAX_R, len(levels))
        mag["levels"] = []
        for l, R in enumerate(ENV_LEVELS):
            use = (l0 == l) | (l1 == l)
            taps, _, _ = cube_taps(R, kept["refl"][use])
            mag["levels"].append(_scatter_abs(6 * R * R, taps, kept["l_spec"].grad[use]).reshape(6, R, R, 3))
    res["mag"] = mag
    return res


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """float64 evaluate() of a scene with the cotangent zeroed on the fragile pixels; computed once, shared, never modified"""
    sc = scene(name)
    cot = cotangents(sc, kind)
    cot[fragile(name)] = 0.0
    cot[ill_conditioned(name, kind)] = 0.0
    return cot, evaluate(sc, cot, torch.float64)


PERTURB = 2.0 ** -23
ILL_SHARE = 1.0


@functools.lru_cache(maxsize=None)
def ill_conditioned(name, kind):
    """bool [n]: pixels whose float64 per-pixel gradient is not determined to the tolerance at float32 precision (module docstring)"""
    sc = scene(name)
    cot = cotangents(sc, kind)
    cot[fragile(name)] = 0.0
    want = evaluate(sc, cot, torch.float64)
    bad = torch.zeros(cot.shape[0], dtype=torch.bool)
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        moved = dict(sc)
        for k in ("position", "normal", "uv"):
            moved[k] = sc[k].double() * (1.0 + PERTURB * (torch.rand(sc[k].shape, generator=g, dtype=torch.float64) * 2 - 1))
        got = evaluate(moved, cot, torch.float64, magnitudes=False)
        for k in ("position", "normal", "uv"):
            bad |= ((got["grad"][k] - want["grad"][k]).abs() > ILL_SHARE * 1e-4 * want["mag"][k]).any(-1)
    return bad & ~fragile(name)


# ------------------------------------------------------------------------------------------------ fragility
def _near_integer(x, delta=DELTA):
    return (x - x.round()).abs() < delta


@functools.lru_cache(maxsize=None)
def fragile(name):
    """bool [n]: shaded pixels where some selection lies within DELTA of switching (module docstring)"""
    sc = scene(name)
    m = shaded_mask(sc)
    kept = {}
    f64 = lambda t: t.double()
    with torch.no_grad():
        _terms(f64(sc["position"][m]), f64(sc["normal"][m]), f64(sc["uv"][m]), f64(sc["kd"]), f64(sc["ks"]), f64(sc["cam"]), f64(sc["lut"]),
               f64(sc["base"]), [f64(l) for l in sc["levels"]], sc["occlusion"], sc["min_visibility"], sc["bend"], lambda **kw: kept.update(kw))
    uv = f64(sc["uv"][m])
    bad = torch.zeros(uv.shape[0], dtype=torch.bool)
    for key in ("kd", "ks"):
        Ht, Wt = sc[key].shape[:2]
        q = sample_coords(Ht, Wt, uv)
        for k, size in ((0, Wt), (1, Ht)):
            if size > 1:
                bad |= _near_integer(q[:, k] * size - 0.5) | _near_integer(q[:, k], DELTA / size)
    d, rough = kept["d"][:, 0], kept["rough"]
    ndv = d if sc["bend"] else d.clamp(min=1e-4)
    bad |= _near_integer(ndv * 256 - 0.5) | _near_integer(rough * 256 - 0.5)
    bad |= (d - (0.0 if sc["bend"] else 1e-4)).abs() < DELTA / 256
    if sc["occlusion"] == "texture":
        bad |= ((1.0 - kept["ks_s"][:, 0]) - sc["min_visibility"]).abs() < DELTA / 256
    L = len(ENV_LEVELS)
    l0, l1, free = mip_levels(rough, MIN_R, MAX_R, L)
    bad |= _near_integer(free) & (free.round() >= 0) & (free.round() <= L - 1)

    def cube(R, dirs, use):
        _, tx, ty = cube_taps(R, dirs)
        a = dirs.abs().sort(-1, descending=True).values
        return use & (_near_integer(tx) | _near_integer(ty) | ((a[:, 0] - a[:, 1]) / a[:, 0] * (R / 2) < DELTA))

    bad |= cube(ENV_BASE, kept["normal"], torch.ones_like(bad))
    for l, R in enumerate(ENV_LEVELS):
        bad |= cube(R, kept["refl"], (l0 == l) | (l1 == l))
    out = torch.zeros(m.numel(), dtype=torch.bool)
    out[m] = bad
    return out


def worst_ratio(got, want, mag, what=""):
    """worst |got - want| / (1e-4 mag) over the elements; an element of magnitude 0 must be exactly 0"""
    err = (got.double() - want).abs()
    assert torch.all(err[mag == 0] == 0), f"{what}: an element of magnitude 0 is not exactly 0"
    nz = mag > 0
    return float((err[nz] / (1e-4 * mag[nz])).max()) if bool(nz.any()) else 0.0


def ratios(got, want):
    """(forward, per-pixel gradients, texel gradients): the worst ratios of an evaluate()-shaped result against the reference"""
    forward = worst_ratio(got["color"], want["color"], want["mag_color"], "colour")
    pixel = max(worst_ratio(got["grad"][k], want["grad"][k], want["mag"][k], k) for k in ("position", "normal", "uv"))
    texel = max([worst_ratio(got["grad"][k], want["grad"][k], want["mag"][k], k) for k in ("kd", "ks", "base")] +
                [worst_ratio(g, w, mg, f"level {l}") for l, (g, w, mg) in
                 enumerate(zip(got["grad"]["levels"], want["grad"]["levels"], want["mag"]["levels"]))])
    return forward, pixel, texel


def smallest_power_of_two_at_least(x):
    return 2.0 ** math.ceil(math.log2(max(x, 2.0 ** -20)))
