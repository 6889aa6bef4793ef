"""Restatement of the environment resampling semantics (geosplatting_amd/envmap.py, csrc/gs_envmap.hip; stated in
include/geosplat_hip.h) on oracle/torch_ref.py's dtype-generic cube lookup (cube_linear, _select_face, _face_coords, _resolve,
_face_point) and the wrap lookup of tests/meshshade_ref.py (texture2d, wrap_taps).  CPU torch; float64 is the reference, float32 shows
what an fp32 implementation can reach.  Test infrastructure; it shares no code with the kernels.

Every op returns {"value", "mag", "grad", "mag_grad"}: the value, the gradient of sum(cot * value) to the texels by autograd, and the
MAGNITUDES the bounds of tests/test_gpu_envmap.py are multiples of:
  forward   per element the sum of the absolute values of the four taps' contributions, sum_i w_i |t_i| (the corner rule's
            redistributed weights for the cube).  With sRGB on: f'(c) times that, plus |f(c)| -- the curve passes an error of its
            argument on with its slope, and rounds its own result.
  texels    the scatter of the ABSOLUTE cotangent with every tap weight replaced by 1, each distinct tap of an element counted once.
            A float32 texel coordinate carries an absolute rounding that no bound proportional to a tiny weight can absorb.
            Where a float64 texel coordinate lies within DELTA = 1e-3 texels of an integer, the cell that holds it is not determined
            by float32 data (the value is: the weights are continuous there), so the taps of BOTH cells are counted: the texels a
            correct float32 lookup may touch.  The conversion cases hit such coordinates by construction (the equator row and the
            phi = 0 column of an odd-sized map under an axis permutation land on texel centres).
The budget of an element is KAPPA x 1e-4 x magnitude; an element of magnitude 0 must be exactly 0.

`face_gap(d, R)` is the distance of a direction from the nearest cube face boundary in texels, (1 - |second| / |largest|) R / 2; an
element is FRAGILE when it is below DELTA: there the seam rule jumps.  Nothing else is fragile.  The conversion cases have no fragile
element (smallest gap 2.2e-3 texels, case (16, 32, 64, rotateY 0.7); tests/test_envmap_cpu.py asserts it); random directions and the
background leave out what is fragile, capped at 2 % (measured: none of either).

KAPPA is the smallest power of two that is at least twice the worst ratio |fp32 - fp64| / (1e-4 magnitude) of this restatement
evaluated in float32 ON THE CPU over all cases, ops, forward and texel gradients -- derived from the restatement, never from the
kernel.  Measured (tests/test_envmap_cpu.py prints them): forward 0.187 (cube -> lat-long), 0.219 (lat-long -> cube), 0.108 (sample),
0.071 (background); texel gradients 0.072, 0.035, 0.006; worst 0.219, hence KAPPA = 0.5.
"""
import functools
import math

import torch

from oracle import torch_ref as tr
from tests import meshshade_ref as mr

DELTA = 1e-3
KAPPA = 0.5
MEASURED_FORWARD, MEASURED_TEXEL = 0.219, 0.072       # (float32 CPU run: tests/test_envmap_cpu.py prints them)
FRAGILE_CAP = 0.02

# (R, H, W, transform): both conversions run on each
CASES = ((2, 4, 8, None), (5, 7, 13, "z_up_to_y_up"), (16, 32, 64, "rotateY 0.7"), (33, 16, 32, "rotateX 0.3 . z_up_to_y_up"))
SAMPLE_R, SAMPLE_N = 16, 4096
BG = dict(R=16, H=37, W=53, fx=41.0, fy=47.0, cx=24.25, cy=20.5)


def transform(name):
    """float32 [3,3] of a case, by the package's own frame methods (their matrices are checked in tests/test_envmap_cpu.py)"""
    from geosplatting_amd.envshade import LatLngEnvMap
    if name is None:
        return None
    m = LatLngEnvMap(torch.zeros(2, 2, 3))
    for step in reversed(name.split(" . ")):
        words = step.split()
        getattr(m, words[0] + "_")(*[float(w) for w in words[1:]])
    return m.transform


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def case_inputs(k):
    """float32 inputs of conversion case k: cube [6,R,R,3], its cotangent [H,W,3], latlng [H,W,3], its cotangent [6,R,R,3]"""
    R, H, W, name = CASES[k]
    return dict(cube=_rand(100 + k, 6, R, R, 3), cot_latlng=_randn(200 + k, H, W, 3), latlng=_rand(300 + k, H, W, 3),
                cot_cube=_randn(400 + k, 6, R, R, 3), transform=transform(name))


@functools.lru_cache(maxsize=None)
def sample_inputs():
    """cube [6,R,R,3], directions [n,3] (random, then a zero row, NaN rows and the six axes), cotangent [n,3]"""
    d = _randn(501, SAMPLE_N, 3) * (0.25 + 4.0 * _rand(502, SAMPLE_N, 1))
    nan = float("nan")
    special = torch.tensor([[0.0, 0.0, 0.0], [nan, 1.0, 0.0], [0.0, nan, nan], [1.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.5, 0.0],
                            [0.0, -1.0, 0.0], [0.0, 0.0, 3.0], [0.0, 0.0, -1.0]])
    d = torch.cat((d, special))
    return dict(cube=_rand(500, 6, SAMPLE_R, SAMPLE_R, 3), dirs=d, cot=_randn(503, d.shape[0], 3))


@functools.lru_cache(maxsize=None)
def background_inputs():
    """cube, c2w [3,4] of a camera that looks off-axis, a transform; intrinsics in BG (fx != fy, off-centre principal point)"""
    eye = torch.tensor([0.3, -0.2, 1.0])
    fwd = torch.nn.functional.normalize(torch.tensor([0.35, 0.4, -0.85]), dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0])), dim=0)
    up = torch.linalg.cross(right, fwd)
    c2w = torch.stack((right, up, -fwd, eye), dim=1).contiguous()          # OpenGL: x right, y up, -z forward
    return dict(cube=_rand(600, 6, BG["R"], BG["R"], 3), c2w=c2w, transform=transform("rotateZ 0.4 . rotateY -1.1"))


# ------------------------------------------------------------------------------------------------ directions and coordinates
def latlng_dirs(H, W, T, dtype):
    """[H W, 3]: the direction of every lat-long texel, row-major, through the transform"""
    gy = torch.linspace(1.0 / H, 1.0 - 1.0 / H, H, dtype=dtype) * math.pi
    gx = torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, dtype=dtype) * math.pi
    gy, gx = torch.meshgrid(gy, gx, indexing="ij")
    st = gy.sin()
    d = torch.stack((st * gx.sin(), gy.cos(), -st * gx.cos()), -1).reshape(-1, 3)
    return d if T is None else d @ T.to(dtype).T


def cube_texel_uv(R, dtype):
    """[6 R R, 2]: the lat-long lookup coordinates of every cube texel, face-major"""
    g = torch.linspace(-1.0 + 1.0 / R, 1.0 - 1.0 / R, R, dtype=dtype)
    gy, gx = torch.meshgrid(g, g, indexing="ij")
    face = torch.arange(6).repeat_interleave(R * R)
    v = tr._face_point(face, gx.reshape(-1).repeat(6), gy.reshape(-1).repeat(6)).to(dtype)
    v = v / v.norm(dim=-1, keepdim=True)
    tu = torch.atan2(v[:, 0], -v[:, 2]) / (2 * math.pi) + 0.5
    tv = torch.acos(v[:, 1].clamp(-1, 1)) / math.pi
    return torch.stack((tu, tv), -1)


def camera_dirs(H, W, fx, fy, cx, cy, c2w, T, dtype):
    i, j = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    v = torch.stack(((0.5 - cx + j) / fx, -(0.5 - cy + i) / fy, -torch.ones_like(i)), -1).reshape(-1, 3)
    d = v @ c2w[:, :3].to(dtype).T
    return d if T is None else d @ T.to(dtype).T


def face_gap(d, R):
    """distance from the nearest face boundary in texels; inf for a direction without a major axis"""
    a = d.detach().double().abs().sort(-1, descending=True).values
    ok = (a[:, 0] > 0) & torch.isfinite(a[:, 0])
    gap = (1.0 - a[:, 1] / a[:, 0].clamp(min=1e-300)) * R / 2.0
    return torch.where(ok, gap, torch.full_like(gap, float("inf")))


def fragile_dirs(d, R):
    return face_gap(d, R) < DELTA


# ------------------------------------------------------------------------------------------------ magnitudes
def _scatter_distinct(size, idx, v):
    """sum over the elements of |v| into every DISTINCT texel of the element's tap list idx [n, k] (negative: no tap) -> [size, C]"""
    idx = idx.sort(-1).values
    keep = idx >= 0
    keep[:, 1:] &= idx[:, 1:] != idx[:, :-1]
    out = torch.zeros(size, v.shape[1], dtype=v.dtype)
    rows = torch.arange(idx.shape[0])[:, None].expand_as(idx)
    out.index_add_(0, idx[keep], v.abs()[rows[keep]])
    return out


def _cells(t):
    """the cells floor(t) a coordinate may fall into: itself, and the neighbour when it is within DELTA of an integer"""
    return [(t - DELTA).floor().long(), (t + DELTA).floor().long()]


def _cube_tap_union(R, d):
    d = d.detach().double()
    face = tr._select_face(d)
    x, y = tr._face_coords(d, face)
    tx, ty = (x + 1) * 0.5 * R - 0.5, (y + 1) * 0.5 * R - 0.5
    taps = [tr._resolve(face, ix + ox, iy + oy, R, torch.float64) for ix in _cells(tx) for iy in _cells(ty)
            for (ox, oy) in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return torch.stack(taps, -1)


def _wrap_tap_union(Ht, Wt, uv):
    uv = uv.detach().double()
    up = uv - uv.floor()
    x, y = up[:, 0] * Wt - 0.5, up[:, 1] * Ht - 0.5
    taps = [torch.remainder(iy + oy, Ht) * Wt + torch.remainder(ix + ox, Wt) for ix in _cells(x) for iy in _cells(y)
            for (ox, oy) in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return torch.stack(taps, -1)


def _cube_forward_mag(cube, d):
    R = cube.shape[1]
    idx, tx, ty = mr.cube_taps(R, d)
    fx, fy = tx - tx.floor(), ty - ty.floor()
    w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    miss = [i < 0 for i in idx]
    spill = sum(torch.where(m, wi, torch.zeros_like(wi)) for wi, m in zip(w, miss)) / 3.0
    flat = cube.detach().reshape(-1, 3).abs()
    mag = sum(torch.where(m, torch.zeros_like(wi), wi + spill)[:, None] * flat[i.clamp(min=0)] for wi, m, i in zip(w, miss, idx))
    return mag


def _wrap_forward_mag(tex, uv):
    Ht, Wt, _ = tex.shape
    idx, x, y = mr.wrap_taps(Ht, Wt, uv.detach())
    fx, fy = x - x.floor(), y - y.floor()
    w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    flat = tex.detach().reshape(-1, 3).abs()
    return sum(wi[:, None] * flat[i] for wi, i in zip(w, idx))


def rgb2srgb(c):
    return torch.where(c <= 0.0031308, c * 12.92, c.clamp(min=0.0031308).pow(1.0 / 2.4) * 1.055 - 0.055)


def _finish(tex, value, mag, cot, tap_union):
    out = {"value": value.detach(), "mag": mag.detach()}
    if cot is not None:
        out["grad"], = torch.autograd.grad((value * cot).sum(), tex)
        out["mag_grad"] = _scatter_distinct(tex.numel() // 3, tap_union, cot.reshape(-1, 3)).reshape(tex.shape)
    return out


# ------------------------------------------------------------------------------------------------ the ops
def sample_cubemap(cube, dirs, cot=None, dtype=torch.float64):
    """cube [6,R,R,3], dirs [n,3], cot [n,3] or None"""
    cube = cube.to(dtype).requires_grad_(cot is not None)
    d = dirs.to(dtype)
    a = d.abs().max(-1).values
    valid = ((a > 0) & torch.isfinite(a))[:, None]                      # no major axis: zeros, no gradient, no taps
    d = torch.where(valid, d, torch.tensor([1.0, 0.0, 0.0], dtype=dtype))
    value = torch.where(valid, tr.cube_linear(cube, d), torch.zeros((), dtype=dtype))
    mag = torch.where(valid, _cube_forward_mag(cube, d), torch.zeros((), dtype=dtype))
    union = None
    if cot is not None:
        union = _cube_tap_union(cube.shape[1], d)
        union[~valid[:, 0]] = -1
    return _finish(cube, value, mag, None if cot is None else cot.to(dtype), union)


def cube_to_latlng(cube, H, W, T=None, cot=None, dtype=torch.float64):
    """-> value [H,W,3] ...; the directions are computed in `dtype`"""
    d = latlng_dirs(H, W, T, dtype)
    out = sample_cubemap(cube, d, None if cot is None else cot.reshape(-1, 3), dtype)
    out["value"], out["mag"] = out["value"].reshape(H, W, 3), out["mag"].reshape(H, W, 3)
    return out


def latlng_to_cube(latlng, R, cot=None, dtype=torch.float64):
    """latlng [H,W,3] -> value [6,R,R,3] ...; the coordinates are computed in `dtype`"""
    tex = latlng.to(dtype).requires_grad_(cot is not None)
    uv = cube_texel_uv(R, dtype)
    value = mr.texture2d(tex, uv, "wrap")
    out = _finish(tex, value, _wrap_forward_mag(tex, uv), None if cot is None else cot.to(dtype).reshape(-1, 3),
                  _wrap_tap_union(tex.shape[0], tex.shape[1], uv) if cot is not None else None)
    out["value"], out["mag"] = out["value"].reshape(6, R, R, 3), out["mag"].reshape(6, R, R, 3)
    return out


def background(cube, H, W, fx, fy, cx, cy, c2w, T=None, srgb=True, dtype=torch.float64):
    """-> value, mag [H,W,3] and `fragile` [H,W] (from the float64 directions)"""
    d = camera_dirs(H, W, fx, fy, cx, cy, c2w, T, dtype)
    out = sample_cubemap(cube, d, None, dtype)
    c, mag = out["value"], out["mag"]
    if srgb:
        slope = torch.where(c <= 0.0031308, torch.full_like(c, 12.92), (1.055 / 2.4) * c.clamp(min=0.0031308).pow(1.0 / 2.4 - 1.0))
        c, mag = rgb2srgb(c), slope * mag + rgb2srgb(c).abs()
    frag = fragile_dirs(camera_dirs(H, W, fx, fy, cx, cy, c2w, T, torch.float64), cube.shape[1])
    return {"value": c.reshape(H, W, 3), "mag": mag.reshape(H, W, 3), "fragile": frag.reshape(H, W)}


# ------------------------------------------------------------------------------------------------ comparison
def worst_ratio(got, want, mag, what="", keep=None):
    """worst |got - want| / (1e-4 mag) over the elements (rows of `keep` only); an element of magnitude 0 must be exactly 0"""
    err = (got.double() - want.double()).abs()
    mag = mag.double()
    if keep is not None:
        sel = keep.reshape(keep.shape + (1,) * (err.ndim - keep.ndim)).expand_as(err)
        err, mag = err[sel], mag[sel]
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert torch.all(err[mag == 0] == 0), f"{what}: an element of magnitude 0 is not exactly 0"
    nz = mag > 0
    return float((err[nz] / (1e-4 * mag[nz])).max()) if bool(nz.any()) else 0.0


def smallest_power_of_two_at_least(x):
    return 2.0 ** math.ceil(math.log2(max(x, 2.0 ** -20)))
