"""float64 restatement of the Monte-Carlo environment shader of csrc/gs_envshade.hip (include/geosplat_hip.h states the semantics),
with per-sample fragile masks and error budgets, and the scenes the shader's tests share (tests/test_envshade_cpu.py,
tests/test_gpu_envshade.py).  Written from the mathematics, in the manner of tests/raytrace_ref.py.

What is EXACT here (computed in uint32 / float32 exactly as the header specifies, so it matches the kernel bit for bit): the PCG
stream, the two table picks, the five uniforms of every iteration, the stratum coordinates ((perm % n) + u) / n, and the bisection over
the CDF tables including the fp32 remainder and width of the chosen cell.  Everything else is float64 from float64 copies of the fp32
inputs: directions, pdfs, the BSDF, the light lookup, the sums.  Visibility comes from raytrace_ref.trace.  Gradients are torch float64
autograd of the per-sample formula with the directions, the pdf sums and V held constant.

Error budgets (u = 2^-24, one fp32 rounding; every constant counts the kernel's operations, none is tuned to what it returns).
  direction of a light sample: the texel coordinate (x + r) / W carries 3 u (remainder, add, divide); phi = (2 c - 1) pi: 2 * 3 u + u,
    times pi (constant and product: 2 u relative) <= 9 pi u; theta = c pi <= 5 pi u; sincosf 2 u each; a component is a product of
    two of them: |d dir| <= (9 pi + 5 pi + 5) u  ->  DIR_LIGHT = 50 u.
  direction of a BSDF sample: the frame of the unit normal (normalise 3 u, basis 5 u), the local direction from sincosf(2 pi u1)
    (argument 3 * 2 pi u = 19 u), two square roots, three products and two sums (5 u), normalise (3 u): 3 * 8 + 19 + 4 + 5 + 3 = 55 u
    ->  DIR_COS = 64 u.  The GGX lobe adds the local view direction (10 u absolute per component), the stretch and its normalise, the
    warp and the reflection (another 30 u), and its tangent T1 = unit(-Vh.y, Vh.x, 0) turns by 10 u / |wo_l.xy| when the viewer is
    near the normal (the stretch by alpha cancels in the ratio); the half vector is ill-conditioned at the rim of the sampling disk
    and for a small alpha (see `sample`: h_cond)  ->  DIR_GGX = (128 + 16 / max(|wo_l.xy|, 1e-3) + h_cond) u.
  pdf of the light at a given direction: acosf 2 u theta, v = theta / pi 2 u, sinf(v pi) argument 4 u theta: relative
    4 u theta |cot theta| + 2 u, weight 5 u  ->  relative (8 + 13 |cot theta|) u, cot capped where the 1e-4 clamp holds.
  pdf of the GGX lobe: D = a2 / (pi d^2), d = (c a2 - c) c + 1 with c = n.h rounded to fp32 near 1: the absolute error of c (6 u from a
    normalise and a dot product, more at grazing half vectors where |wo + wi| = 2 wo.h is small) enters d twice: d d <= 2 * 6 u / max(wo.h,
    0.05) + 4 u, and D doubles it again.  This is the known cancellation: relative (32 + 64 / (d max(wo.h, 0.05))) u.  At roughness
    0.08 (a2 = 4.1e-5, d >= a2) that is up to 7 % of a sample on the peak of the lobe -- far looser than a 1e-4 relative contract,
    because no fp32 evaluation of d through c can do better: the rounding of c alone (u) is 0.3 % of d = a2 there.
  pdf of the cosine lobe: 4 u absolute.
  specular BSDF: the same D with clamped a2 >= 4.1e-5 (d from c = clamp(n.h)), two lambdas (8 u each relative to 1 + lambda), Fresnel
    (pow5 of a difference: 12 u), the quotient 4 u  ->  relative (48 + 64 / (d max(wo.h, 0.05))) u.  Lambert: 4 u / pi absolute.
  a sample's term t = bsdf L V w, w = 1 / (n^2 max(pdf_sum, 1e-4)): relative rel(bsdf) + rel(pdf_sum) + 6 u; an output element over S
    samples: sum_s |t_s| rel_s + (S + 8) u sum_s |t_s|  -- the scale is sum |t|, not |sum t|.
  gradients: the same per sample and per factor of the specular product (F, D, G, 1 / n.wo each differentiated with the others held),
    the D factor with three times its cancellation term (d^3); light_grad per texel with the scale = the sum of absolute adds.

FRAGILE samples -- an fp32 rounding may legitimately flip a discrete decision: the lobe choice (|u - pDiffuse| within the error of
pDiffuse, 64 u), pDiffuse against 1e-4, a mixture weight against 1e-6, n.wo or n.wi against 1e-6 (pdf) and 1e-4 (specular gate), the
local view against the horizon, Vh.z against 0.9999 (within (4 + 16 |Vh.xy|) u), a texel coordinate within 8 u size of a texel edge, and a shadow ray that
raytrace_ref marks fragile_any; for the gradients also a clamped cosine within 16 u of either clamp end.  A point is fragile when
any of its samples is."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import raytrace_ref

U24 = 2.0 ** -24
ONE_BELOW = np.float32(0.99999994)
BSDFS = ("pbr", "diffuse", "white")
CAMERA = np.array([0.0, 0.0, 3.0], dtype=np.float32)
TMAX = 1e16
DIR_LIGHT, DIR_COS = 50.0, 64.0
PCG_MUL, PCG_INC = np.uint32(747796405), np.uint32(2891336453)


# ---- the exact part ----------------------------------------------------------------------------------------------------------------
def pcg_out(s: np.ndarray) -> np.ndarray:
    s = np.asarray(s, dtype=np.uint32)
    with np.errstate(over="ignore"):
        w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


def pcg_step(s: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(s, dtype=np.uint32) * PCG_MUL + PCG_INC


def stream(seed: int, P: int, T: int, nn: int):
    """(light table [P], bsdf table [P], uniforms [P, nn, 5] float32) of points 0 .. P - 1"""
    s = pcg_out(np.full(P, seed, np.uint32)) ^ pcg_out(np.arange(P, dtype=np.uint32))
    lt = pcg_out(s) % np.uint32(T); s = pcg_step(s)
    bt = pcg_out(s) % np.uint32(T); s = pcg_step(s)
    u = np.empty((P, nn, 5), np.float32)
    for i in range(nn):
        for k in range(5):
            u[:, i, k] = (pcg_out(s) & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
            s = pcg_step(s)
    return lt.astype(np.int64), bt.astype(np.int64), u


def strata(perm: np.ndarray, n: int, ua: np.ndarray, ub: np.ndarray):
    """fp32 ((perm % n) + ua) / n, ((perm / n) + ub) / n as the kernel rounds them"""
    inv = np.float32(1.0) / np.float32(n)
    return ((perm % n).astype(np.float32) + ua) * inv, ((perm // n).astype(np.float32) + ub) * inv


def search_steps(size: int) -> int:
    c = 0
    while (1 << c) < size - 1:
        c += 1
    return c + 1


def cdf_pick(cdf: np.ndarray, x: np.ndarray):
    """cdf [..., size] float32 (one table per element of x, or one shared 1-D table), x [...] float32 -> (index, fp32 offset, fp32 width)"""
    x = np.minimum(x.astype(np.float32), ONE_BELOW)
    size = cdf.shape[-1]
    table = np.broadcast_to(cdf, x.shape + (size,))
    take = lambda i: np.take_along_axis(table, i[..., None], -1)[..., 0]
    lo, hi = np.zeros(x.shape, np.int64), np.full(x.shape, size - 1, np.int64)
    for _ in range(search_steps(size)):
        mid = (lo + hi) // 2
        c = take(mid)
        lo = np.where(x >= c, mid, lo)
        hi = np.where(x < c, mid, hi)
    below = np.where(hi == 0, np.float32(0), take(np.maximum(hi - 1, 0))).astype(np.float32)
    width = np.where(hi == 0, take(hi), take(hi) - below).astype(np.float32)
    off = np.where(hi == 0, x, x - below).astype(np.float32)
    return hi, off, width


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_mesh(occluder: bool = True):
    v, f = raytrace_ref.mesh("ico2")
    if not occluder:
        return v, f
    tri = np.array([[-1.6, 1.5, -1.3], [1.7, 1.45, -0.9], [0.1, 1.55, 1.8]], dtype=np.float32)
    return np.concatenate([v, tri]), np.concatenate([f, [[v.shape[0], v.shape[0] + 1, v.shape[0] + 2]]])


@functools.lru_cache(maxsize=None)
def env_map(name: str):
    """(light [H,W,3], pdf [H,W], rows [H], cols [H,W]) float32: random positive radiance, one texel x 200, one row of zeros; the
    tables by `compute_pdf` below"""
    H, W = {"16x32": (16, 32), "5x7": (5, 7)}[name]
    rng = np.random.default_rng(7 + H)
    light = rng.uniform(0.05, 1.0, (H, W, 3)).astype(np.float32)
    light[H // 4, (2 * W) // 3] *= 200.0
    light[H - 2] = 0.0
    return (light,) + compute_pdf(light)


def compute_pdf(light: np.ndarray):
    """TextureLatLng.compute_pdf_ in fp32 numpy, the same operations (the sums' order may differ from torch's: compare with a tolerance)"""
    H, W = light.shape[:2]
    y = ((np.arange(H, dtype=np.float32) + np.float32(0.5)) / np.float32(H))[:, None]
    pdf = np.maximum(light.max(-1), np.float32(1e-3)) * np.sin(y * np.float32(np.pi)).astype(np.float32)
    pdf = (pdf / pdf.sum(dtype=np.float32)).astype(np.float32)
    cols = np.cumsum(pdf, 1, dtype=np.float32)
    rows = np.cumsum(np.repeat(cols[:, -1:], W, 1), 0, dtype=np.float32)
    cols = cols / np.where(cols[:, -1:] > 0, cols[:, -1:], np.float32(1))
    rows = rows / np.where(rows[-1:] > 0, rows[-1:], np.float32(1))
    return pdf, np.ascontiguousarray(rows[:, 0]).astype(np.float32), cols.astype(np.float32)


@functools.lru_cache(maxsize=None)
def points(P: int):
    """Every third MGAdapter Gaussian of the bumpy icosphere(2), the first P of them: dict of fp32 arrays pos, nrm (bent towards the
    camera as splat_mc bends them), ro (= pos + unbent normal * 1e-5), kd, ks (occlusion factor, roughness, metallic)"""
    from oracle import mesh_ref
    v, f = raytrace_ref.mesh("ico2")
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    means, _, _, _, normals = mesh_ref.mesh_to_splats(vt, ft, mesh_ref.vertex_normals(vt, ft))
    pos = np.roll(means.numpy()[::3], -2, 0)[:P].astype(np.float32)                       # (the first point sees the sky)
    nrm0 = np.roll(normals.numpy()[::3], -2, 0)[:P].astype(np.float32)
    lookat = np.array([0.0, 0.0, -1.0], np.float32)
    bend = (nrm0 * lookat).sum(-1, keepdims=True) > 1e-3
    nrm = np.where(bend, -nrm0, nrm0).astype(np.float32)
    ro = (pos + nrm0 * np.float32(1e-5)).astype(np.float32)
    rng = np.random.default_rng(11)
    N = 214
    kd = rng.uniform(0.05, 0.95, (N, 3)).astype(np.float32)
    rough = rng.uniform(0.08, 1.0, N).astype(np.float32)
    metal = rng.uniform(0.0, 1.0, N).astype(np.float32)
    occ = np.where(rng.random(N) < 0.3, rng.uniform(0.0, 0.6, N), 0.0).astype(np.float32)
    rough[[0, 5]] = np.float32(0.08); rough[7] = 1.0
    metal[[0, 3]] = 0.0; metal[[1, 4]] = 1.0
    ks = np.stack([occ, rough, metal], -1).astype(np.float32)
    return dict(pos=pos, nrm=nrm, ro=ro, kd=kd[:P].copy(), ks=ks[:P].copy())


@functools.lru_cache(maxsize=None)
def perms(n: int, T: int = 7):
    rng = np.random.default_rng(100 + n)
    return np.stack([rng.permutation(n * n) for _ in range(T)]).astype(np.int32)


POINT_COUNTS = (1, 65, 214)
MAPS = ("16x32", "5x7")
SAMPLES_X = (1, 3, 4)
SEED = 3                # chosen from the restatement alone: with 65 points one fragile point is already over the 1 % cap (test_envshade_cpu)
# the combinations the GPU tests run: every P, map and n occurs, not the full product (each costs a float64 evaluation)
CASES = ((214, "16x32", 4), (65, "5x7", 3), (1, "16x32", 1), (65, "16x32", 1), (214, "5x7", 4), (1, "5x7", 3))


# ---- float64 sampling --------------------------------------------------------------------------------------------------------------
def _unit(a):
    l = np.sqrt((a * a).sum(-1, keepdims=True))
    return np.where(l > 0, a / np.where(l > 0, l, 1.0), 0.0)


def _basis(n):
    sign = np.copysign(1.0, n[..., 2])
    a = -1.0 / (sign + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    b1 = np.stack([1.0 + sign * n[..., 0] ** 2 * a, sign * b, -sign * n[..., 0]], -1)
    b2 = np.stack([b, sign + n[..., 1] ** 2 * a, -n[..., 1]], -1)
    return b1, b2


def _luma(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _clampc(c):
    return np.clip(c, 1e-4, 1.0 - 1e-4)


def point_setup(pt: dict, view=CAMERA) -> dict:
    """the per-point constants in float64: wo, the frame, the local view, alpha and the lobe probabilities, and the point's own
    fragile flag (decisions that do not depend on the sample)"""
    pos, n, kd, ks = (pt[k].astype(np.float64) for k in ("pos", "nrm", "kd", "ks"))
    to_view = view.astype(np.float64) - pos
    wo = _unit(to_view)
    fw = _unit(n)
    fu, fv = _basis(fw)
    wol = np.stack([(wo * fu).sum(-1), (wo * fv).sum(-1), (wo * fw).sum(-1)], -1)
    woln = _unit(wol)
    alpha = ks[:, 1] ** 2
    m = ks[:, 2]
    f0 = 0.04 * (1.0 - m)[:, None] + kd * m[:, None]
    wd = (1.0 - m) * _luma(kd)
    s = (1.0 - _clampc(woln[:, 2])) ** 5
    wsp = np.where(woln[:, 2] > 0, _luma(f0 * (1.0 - s)[:, None] + s[:, None]), 0.0)
    tot = wd + wsp
    pD = np.where(tot > 0, wd / np.where(tot > 0, tot, 1.0), 1.0)
    al = alpha
    vh = _unit(np.stack([al * woln[:, 0], al * woln[:, 1], woln[:, 2]], -1))
    # pDiffuse is exactly 0 (no diffuse weight) or exactly 1 (no specular weight) in fp32 as here; otherwise its relative error, and
    # that of 1 - pDiffuse = wsp / (wd + wsp), is 64 u, and the kernel's 1 - fl(pDiffuse) adds 2 u absolute
    e = 64.0 * U24
    nv = (n * wo).sum(-1)
    inexact = (wd > 0) & (wsp > 0)
    # Vh.z at 0.9999 is stationary in the tangential components: their 16 u enter scaled by |Vh.xy| = 0.014, the normalise adds 4 u
    e_vh = (4.0 + 16.0 * np.sqrt(vh[:, 0] ** 2 + vh[:, 1] ** 2)) * U24
    pS = 1.0 - pD
    frag = ((inexact & ((np.abs(pD - 1e-4) <= e * pD) | (np.abs(pD - 1e-6) <= e * pD) | (np.abs(pS - 1e-6) <= e * pS + 2.0 * U24) | (pS <= 2.0 * U24))) |
            (np.abs(woln[:, 2]) <= e) | (np.abs(wol[:, 2]) <= e) | (np.abs(vh[:, 2] - 0.9999) <= e_vh) |
            (np.abs(nv - 1e-6) <= e) | (np.abs(nv - 1e-4) <= e))
    return dict(pos=pos, n=n, kd=kd, ks=ks, wo=wo, fw=fw, fu=fu, fv=fv, wol=wol, woln=woln, alpha=alpha, pD=pD, vh=vh, nv=nv, fragile=frag,
                wo_len=np.sqrt((to_view ** 2).sum(-1)))


def _ndf(a2, c):
    d = (c * a2 - c) * c + 1.0
    return a2 / (d * d * np.pi), d


def _g1(a2, c):
    c2 = c * c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, 2.0 / (1.0 + np.sqrt(1.0 + a2 * np.maximum(1.0 - c2, 0.0) / c2)), 0.0)


def ggx_pdf(ps: dict, wi: np.ndarray):
    """VNDF pdf with the reflection Jacobian for directions wi [P,S,3]; also its relative budget in units of u and a fragile mask"""
    wil = np.stack([(wi * ps["fu"][:, None]).sum(-1), (wi * ps["fv"][:, None]).sum(-1), (wi * ps["fw"][:, None]).sum(-1)], -1)
    wol = ps["wol"][:, None, :]
    ok = (wol[..., 2] > 0) & (wil[..., 2] > 0)
    m = _unit(wil + wol)
    vh = (m * wol).sum(-1)
    a2 = (ps["alpha"] ** 2)[:, None]
    D, d = _ndf(a2, m[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = _g1(a2, wol[..., 2]) * D * np.maximum(0.0, vh) / wol[..., 2] / (4.0 * vh)
        rel = 32.0 + 64.0 / (np.maximum(d, 1e-300) * np.maximum(vh, 0.05))
    frag = np.abs(wil[..., 2]) <= 16.0 * U24
    return np.where(ok, pdf, 0.0), np.where(ok, rel, 0.0), frag


def _texel(coord, size):
    return np.clip(np.floor(np.clip(coord * size, 0.0, None)), 0, size - 1).astype(np.int64)


def light_pdf(env, wi: np.ndarray):
    """(pdf [.,.], texel x, texel y, relative budget in u, fragile) of directions wi"""
    _, pdf, _, _ = env
    H, W = pdf.shape
    u = np.arctan2(wi[..., 0], -wi[..., 2]) / (2.0 * np.pi) + 0.5
    theta = np.arccos(np.clip(wi[..., 1], -1.0, 1.0))
    v = theta / np.pi
    tx, ty = _texel(u, W), _texel(v, H)
    sin_t = np.maximum(np.sin(theta), 1e-4)
    val = pdf.astype(np.float64)[ty, tx] * (W * H / (2.0 * np.pi ** 2 * sin_t))
    rel = 8.0 + 13.0 * np.abs(np.cos(theta)) / sin_t
    edge = lambda c, size: (np.abs(c * size - np.round(c * size)) <= 8.0 * U24 * size) & (np.round(c * size) > 0) & (np.round(c * size) < size)
    return val, tx, ty, rel, edge(u, W) | edge(v, H)


def sample(pt: dict, env, n: int, seed: int, T_perms: np.ndarray) -> dict:
    """The 2 n^2 sample directions of every point in float64 and what the pdf of a BSDF sample needs from its generation:
    dirs [P,S,3], budget [P,S] (absolute, per component), fragile [P,S], search texel [P,nn,2], lobe [P,nn] (0 cosine, 1 GGX,
    2 the normal itself, 3 the zero direction), own [P,nn] (the sampled lobe's own pdf before the mixture weight), own_rel [P,nn]"""
    light, pdf, rows, cols = env
    H, W = pdf.shape
    P, nn = pt["pos"].shape[0], n * n
    ps = point_setup(pt)
    lt, bt, u = stream(seed, P, T_perms.shape[0], nn)
    pl, pb = T_perms[lt].astype(np.int64), T_perms[bt].astype(np.int64)                   # [P,nn]
    lx, ly = strata(pl, n, u[..., 0], u[..., 1])
    bx, by = strata(pb, n, u[..., 2], u[..., 3])
    u3 = u[..., 4].astype(np.float64)
    # light: row, then column of that row
    y, offy, wy = cdf_pick(rows, ly)
    x, offx, wx = cdf_pick(cols[y], lx)
    with np.errstate(divide="ignore", invalid="ignore"):
        ry = np.fmin(offy.astype(np.float64) / wy.astype(np.float64), float(ONE_BELOW))
        rx = np.fmin(offx.astype(np.float64) / wx.astype(np.float64), float(ONE_BELOW))
    phi = (((x + rx) / W) * 2.0 - 1.0) * np.pi
    theta = ((y + ry) / H) * np.pi
    dl = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1)
    # bsdf
    pD = ps["pD"][:, None]
    fu, fv, fw = ps["fu"][:, None], ps["fv"][:, None], ps["fw"][:, None]
    bx64, by64 = bx.astype(np.float64), by.astype(np.float64)
    diffuse = u3 < pD
    ph = 2.0 * np.pi * bx64
    ct, st = np.sqrt(by64), np.sqrt(1.0 - by64)
    d_cos = _unit(fu * (np.cos(ph) * st)[..., None] + fv * (np.sin(ph) * st)[..., None] + fw * ct[..., None])
    own_cos = np.maximum(1e-6, ct / np.pi)
    o = ps["woln"][:, None, :]
    al = ps["alpha"][:, None]
    a2 = al * al
    vh = ps["vh"][:, None, :]
    t1 = np.where(vh[..., 2:3] < 0.9999, _unit(np.stack([-vh[..., 1], vh[..., 0], np.zeros_like(vh[..., 0])], -1)), np.array([1.0, 0.0, 0.0]))
    t2 = np.cross(vh, t1)
    ph2 = 2.0 * np.pi * by64
    r = np.sqrt(bx64)
    p1 = r * np.cos(ph2)
    s = 0.5 * (1.0 + vh[..., 2])
    p2 = (1.0 - s) * np.sqrt(1.0 - p1 * p1) + s * (r * np.sin(ph2))
    nh = t1 * p1[..., None] + t2 * p2[..., None] + vh * np.sqrt(np.maximum(0.0, 1.0 - p1 * p1 - p2 * p2))[..., None]
    h_long = np.stack([al * nh[..., 0], al * nh[..., 1], np.maximum(0.0, nh[..., 2])], -1)
    h = _unit(h_long)
    # conditioning of the half vector: the height q = sqrt(1 - p1^2 - p2^2) on the hemisphere loses 2 u / q at the rim of the disk, the
    # components across it carry 20 u alpha; normalising the (short, for a small alpha) stretched vector divides both by its length,
    # the reflection doubles them
    q = np.sqrt(np.maximum(0.0, 1.0 - p1 * p1 - p2 * p2))
    h_cond = 2.0 * (20.0 * al + 2.0 / np.maximum(q, 1e-4)) / np.maximum(np.sqrt((h_long ** 2).sum(-1)), 1e-6)
    oh = (o * h).sum(-1)
    D, dd = _ndf(a2, h[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        own_ggx = _g1(a2, o[..., 2]) * D * np.maximum(0.0, oh) / o[..., 2] / (4.0 * oh)
        own_ggx_rel = 32.0 + 64.0 / (np.maximum(dd, 1e-300) * np.maximum(oh, 0.05))
    l = h * (2.0 * oh)[..., None] - o
    d_ggx = _unit(fu * l[..., 0:1] + fv * l[..., 1:2] + fw * l[..., 2:3])
    below = ~(o[..., 2] > 0)
    lobe = np.where(diffuse, np.where(pD < 1e-4, 2, 0), np.where(below, 3, 1)) * np.ones((P, nn), np.int64)
    n_raw = np.broadcast_to(ps["n"][:, None, :], (P, nn, 3))
    db = np.select([(lobe == 0)[..., None], (lobe == 1)[..., None], (lobe == 2)[..., None]], [d_cos, d_ggx, n_raw], 0.0)
    own = np.select([lobe == 0, lobe == 1, lobe == 2], [own_cos, own_ggx, np.ones_like(own_cos)], 0.0)
    own_rel = np.select([lobe == 0, lobe == 1], [np.full_like(own_cos, 8.0), own_ggx_rel], 0.0)
    xy = np.sqrt(ps["woln"][:, 0] ** 2 + ps["woln"][:, 1] ** 2)[:, None]
    b_budget = np.select([lobe == 0, lobe == 1], [np.full_like(own_cos, DIR_COS), 128.0 + 16.0 / np.maximum(xy, 1e-3) + h_cond], 0.0) * U24
    dirs = np.stack([dl, db], 2).reshape(P, 2 * nn, 3)
    budget = np.stack([np.full((P, nn), DIR_LIGHT * U24), b_budget], 2).reshape(P, 2 * nn)
    frag_b = (np.abs(u3 - pD) <= 64.0 * U24) | ps["fragile"][:, None]
    fragile = np.stack([np.broadcast_to(ps["fragile"][:, None], (P, nn)), frag_b], 2).reshape(P, 2 * nn)
    return dict(dirs=dirs, budget=budget, fragile=fragile, texel=np.stack([x, y], -1), lobe=lobe, own=own, own_rel=own_rel, ps=ps,
                uniforms=u, tables=(lt, bt))


def pdf_sums(pt: dict, env, smp: dict, dirs: np.ndarray):
    """pdf_light + pdf_bsdf of every slot, evaluated at `dirs` [P,S,3] (the restatement's own or the kernel's logged ones): the light
    pdf and the mixture's other lobe from the direction, a BSDF sample's own lobe from its generation.  -> (pdf_sum [P,S], absolute
    budget [P,S], fragile [P,S], texel index [P,S])"""
    ps = smp["ps"]
    P, S = dirs.shape[:2]
    nn = S // 2
    pD = ps["pD"][:, None]
    pS = 1.0 - pD
    n = ps["n"][:, None, :]
    pl, tx, ty, rel_l, frag = light_pdf(env, dirs)
    nl = (n * dirs).sum(-1)
    nv = ps["nv"][:, None]
    gp, gp_rel, gp_frag = ggx_pdf(ps, dirs)
    cosp = np.maximum(nl, 0.0) / np.pi
    mixw = lambda w: np.where(w > 1e-6, w, 0.0)
    # a direction the light produced
    horizon = np.minimum(nv, nl) < 1e-6
    pb_l = np.where(pD > 0, cosp * mixw(pD), 0.0) + np.where(pS > 0, gp * mixw(1.0 - pD), 0.0)
    bud_l = np.where(pD > 0, 4.0 * U24 * mixw(pD), 0.0) + np.where(pS > 0, gp * mixw(1.0 - pD) * gp_rel * U24, 0.0)
    pb_l, bud_l = np.where(horizon, 1.0, pb_l), np.where(horizon, 0.0, bud_l)
    frag_l = (np.abs(nl - 1e-6) <= 16.0 * U24) | (gp_frag & ~horizon & (pS > 0))
    # a direction the BSDF produced
    lobe = np.repeat(smp["lobe"], 2, 1)
    own, own_rel = np.repeat(smp["own"], 2, 1), np.repeat(smp["own_rel"], 2, 1)
    pb_b = np.select([lobe == 0, lobe == 1, lobe == 2], [
        own * pD + np.where(pS > 0, gp * mixw(1.0 - pD), 0.0),
        own * (1.0 - pD) + np.where(pD > 0, cosp * mixw(pD), 0.0),
        np.ones_like(own)], 0.0)
    bud_b = np.select([lobe == 0, lobe == 1], [
        own * pD * (own_rel + 66.0) * U24 + np.where(pS > 0, gp * mixw(1.0 - pD) * gp_rel * U24, 0.0),
        own * (1.0 - pD) * (own_rel + 66.0) * U24 + np.where(pD > 0, 4.0 * U24 * mixw(pD), 0.0)], 0.0)
    frag_b = np.where(lobe == 0, gp_frag & (pS > 0), False)
    odd = (np.arange(S) % 2 == 1)[None, :]
    pb = np.where(odd, pb_b, pb_l)
    total = pl + pb
    budget = pl * rel_l * U24 + np.where(odd, bud_b, bud_l) + 2.0 * U24 * np.abs(total)
    return total, budget, frag | np.where(odd, frag_b, frag_l), ty * env[1].shape[1] + tx


# ---- float64 shading (torch: autograd gives the reference gradients) ---------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _tunit(a):
    l = (a * a).sum(-1, keepdim=True).sqrt()
    return torch.where(l > 0, a / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(a))


def bsdf_terms(pos, n, kd, ks, wi, bsdf: str, only=None, view=CAMERA):
    """Lambert value [P,S] and specular [P,S,3] for per-sample copies of the point attributes ([P,S,3] each).  only in (None, 'lam', 'F',
    'D', 'G', 'k'): differentiate through that factor alone (the others detached) -- the per-factor scales of the gradient budgets.
    Also the relative budget of the specular value in u [P,S], the D factor's cancellation term [P,S], and the fragile masks."""
    att = lambda name, x: x if only in (None, name) else x.detach()
    lam = att("lam", ((n * wi).sum(-1) / np.pi).clamp_min(0.0))
    wo = _tunit(_t(view) - pos)
    alpha = ks[..., 1] ** 2
    amin = 0.08 ** 2
    al = torch.where(alpha > amin, alpha, torch.full_like(alpha, amin)).clamp_max(1.0)
    a2 = al * al
    h = _tunit(wo + wi)
    nv, nl, vh, nh = (wo * n).sum(-1), (wi * n).sum(-1), (wo * h).sum(-1), (n * h).sum(-1)
    col = (0.04 * (1.0 - ks[..., 2:3]) + kd * ks[..., 2:3]) * (1.0 - ks[..., 0:1])
    cl = lambda c: c.clamp(1e-4, 1.0 - 1e-4)
    c = cl(nh)
    d = (c * a2 - c) * c + 1.0
    D = att("D", a2 / (d * d * np.pi))
    lam_f = lambda x: 0.5 * (torch.sqrt(1.0 + a2 * ((1.0 - cl(x) ** 2) / cl(x) ** 2)) - 1.0)
    G = att("G", 1.0 / (1.0 + lam_f(nv) + lam_f(nl)))
    s = (1.0 - cl(vh)) ** 5
    F = att("F", col * (1.0 - s)[..., None] + s[..., None])
    k = att("k", 0.25 / nv)
    front = (nv > 1e-4) & (nl > 1e-4)
    spec = torch.where(front[..., None], F * (D * G * k)[..., None], torch.zeros_like(F))
    if bsdf != "pbr":
        spec = torch.zeros_like(spec)
    with torch.no_grad():
        cancel = 64.0 / (d * vh.clamp_min(0.05))
        e = 16.0 * U24
        near = lambda x, t: (x - t).abs() <= e
        frag_val = (near(nv, 1e-4) | near(nl, 1e-4)) if bsdf == "pbr" else torch.zeros_like(front)
        frag_grad = near(nl, 0.0)
        if bsdf == "pbr":
            for x in (nv, nl, vh, nh):
                frag_grad = frag_grad | ((near(x, 1e-4) | near(x, 1.0 - 1e-4)) & front)
    return lam, spec, 48.0 + cancel, cancel, frag_val.numpy(), (frag_val | frag_grad).numpy()


def shade(pt: dict, env, smp: dict, dirs: np.ndarray, vis: np.ndarray, bsdf: str, shadow_scale: float, n_samples_x: int,
          d_diff: np.ndarray = None, d_spec: np.ndarray = None) -> dict:
    """The outputs for given sample directions [P,S,3] and visibilities [P,S] (0 / 1), in float64, with budgets and fragile masks;
    with d_diff / d_spec [P,3] also the five gradients and theirs."""
    light = env[0].astype(np.float64)
    P, S = dirs.shape[:2]
    nn = n_samples_x * n_samples_x
    psum, psum_budget, frag_pdf, texel = pdf_sums(pt, env, smp, dirs)
    L = _t(light.reshape(-1, 3)[texel])                                                          # [P,S,3]
    w = 1.0 / (nn * np.maximum(psum, 1e-4))
    rel_w = psum_budget / np.maximum(psum, 1e-4) + 6.0 * U24
    V = vis * shadow_scale + (1.0 - shadow_scale)
    exp = lambda k: _t(pt[k])[:, None, :].expand(P, S, 3).clone().requires_grad_(d_diff is not None)
    wi = _t(dirs)
    out = {}
    leaves = [exp(k) for k in ("pos", "nrm", "kd", "ks")]
    lam, spec, rel_s, cancel, frag_val, frag_grad = bsdf_terms(*leaves, wi, bsdf)
    c, shadow = _t(V * w), _t((1.0 - V) * w)
    t_diff = lam[..., None] * L * c[..., None]
    t_spec = spec * L * c[..., None]
    t_resi = torch.stack([lam * shadow, spec.mean(-1) * shadow], -1)
    rel_d = _t(rel_w)[..., None] + 4.0 * U24 / np.pi / lam.detach().clamp_min(1e-300)[..., None] * (lam.detach() > 0)[..., None]
    rel_sp = (_t(rel_w) + rel_s.detach() * U24)[..., None]
    acc = (S + 8.0) * U24
    with torch.no_grad():
        out["diff"], out["spec"], out["resi"] = t_diff.sum(1).numpy(), t_spec.sum(1).numpy(), t_resi.sum(1).numpy()
        out["diff_budget"] = ((t_diff.abs() * rel_d).sum(1) + acc * t_diff.abs().sum(1)).numpy()
        out["spec_budget"] = ((t_spec.abs() * rel_sp).sum(1) + acc * t_spec.abs().sum(1)).numpy()
        r_abs = t_resi.abs()
        r_rel = torch.stack([rel_d[..., 0], rel_sp[..., 0] + 4.0 * U24], -1)
        out["resi_budget"] = ((r_abs * r_rel).sum(1) + acc * r_abs.sum(1)).numpy()
        out["terms"] = (t_diff.numpy(), t_spec.numpy(), t_resi.numpy())
    out["pdf_sum"], out["pdf_sum_budget"], out["texel"] = psum, psum_budget, texel
    out["fragile_sample"] = smp["fragile"] | frag_pdf | frag_val
    out["fragile"] = out["fragile_sample"].any(1)
    out["fragile_grad"] = (out["fragile_sample"] | frag_grad).any(1)
    if d_diff is None:
        return out
    gd, gs = _t(d_diff)[:, None, :], _t(d_spec)[:, None, :]
    # light_grad: per sample, scattered to its texel
    with torch.no_grad():
        gl = (gd * lam[..., None] + gs * spec) * c[..., None]
        rel_gl = torch.maximum(rel_d, rel_sp)
        lg = np.zeros((light.shape[0] * light.shape[1], 3))
        lg_abs, lg_bud, cnt = np.zeros_like(lg), np.zeros_like(lg), np.zeros(lg.shape[0])
        live = (pt.get("mask", np.ones(P, np.float32)) > 0)[:, None] & np.ones((P, S), bool)
        tex = texel[live]
        np.add.at(lg, tex, gl.numpy()[live])
        np.add.at(lg_abs, tex, gl.abs().numpy()[live])
        np.add.at(lg_bud, tex, (gl.abs() * rel_gl).numpy()[live])
        np.add.at(cnt, tex, 1.0)
        out["d_light"] = lg.reshape(light.shape)
        out["d_light_budget"] = (lg_bud + ((cnt + 8.0) * U24)[:, None] * lg_abs).reshape(light.shape)
    # point gradients: the sum of the per-factor passes is the gradient, the sum of their absolute values its scale
    grads = [np.zeros((P, 3)) for _ in range(4)]
    buds = [np.zeros((P, 3)) for _ in range(4)]
    for only in ("lam", "F", "D", "G", "k"):
        if bsdf != "pbr" and only != "lam":
            continue
        lv = [exp(k) for k in ("pos", "nrm", "kd", "ks")]
        lam_o, spec_o, _, _, _, _ = bsdf_terms(*lv, wi, bsdf, only=only)
        obj = ((gd * lam_o[..., None] * L + gs * spec_o * L) * c[..., None]).sum()
        gv = torch.autograd.grad(obj, lv, allow_unused=True)
        rel = _t(rel_w) + (48.0 + (3.0 * cancel if only == "D" else 0.0 * cancel)) * U24
        for k in range(4):
            g = torch.zeros(P, S, 3, dtype=torch.float64) if gv[k] is None else gv[k]
            grads[k] += g.sum(1).numpy()
            buds[k] += ((g.abs() * rel[..., None]).sum(1) + acc * g.abs().sum(1)).numpy()
    for name, g, b in zip(("d_pos", "d_nrm", "d_kd", "d_ks"), grads, buds):
        out[name], out[name + "_budget"] = g, b
    out["fragile_grad"] = (out["fragile_sample"] | frag_grad).any(1)
    return out


def direction_slack(pt: dict, env, smp: dict, vis: np.ndarray, bsdf: str, shadow_scale: float, n_samples_x: int, base: dict) -> dict:
    """What the END-TO-END comparison adds to the budgets of `base` = shade(... smp["dirs"] ...): the kernel's directions differ from
    the restatement's by up to smp["budget"] per component, and a sample's term follows its direction.  First order: the term's change
    when the direction moves by sqrt(3) budget along each of two tangents, summed (either sign, any direction in the tangent plane
    is within twice that sum).  A sample whose texel changes under the move contributes its whole change: that is what can happen."""
    d = smp["dirs"]
    t1, t2 = _basis(d)
    step = (np.sqrt(3.0) * smp["budget"])[..., None]
    add = [0.0, 0.0, 0.0]
    for t in (t1, t2):
        moved = shade(pt, env, smp, _unit(d + step * t), vis, bsdf, shadow_scale, n_samples_x)
        for k in range(3):
            add[k] = add[k] + 2.0 * np.abs(moved["terms"][k] - base["terms"][k]).sum(1)
    return dict(diff=add[0], spec=add[1], resi=add[2])


def visibility(pt: dict, dirs32: np.ndarray, occluder: bool = True):
    """(vis [P,S] 0 / 1, fragile_any [P,S]) of the shadow rays (ro, dirs32) by raytrace_ref.trace, tmin = 0, tmax = 1e16"""
    v, f = scene_mesh(occluder)
    P, S = dirs32.shape[:2]
    o = np.ascontiguousarray(np.broadcast_to(pt["ro"][:, None, :], (P, S, 3))).reshape(-1, 3)
    r = raytrace_ref.trace(v, f, o, np.ascontiguousarray(dirs32.reshape(-1, 3)), 0.0, TMAX)
    return 1.0 - r["occluded"].reshape(P, S).astype(np.float64), r["fragile_any"].reshape(P, S)


@functools.lru_cache(maxsize=None)
def expected(P: int, map_name: str, n: int, bsdf: str = "pbr", shadow_scale: float = 1.0, seed: int = SEED):
    """The end-to-end restatement of one case: (samples, outputs) -- computed once per process and shared (do not modify)"""
    pt, env = points(P), env_map(map_name)
    smp = sample(pt, env, n, seed, perms(n))
    vis, frag_ray = visibility(pt, smp["dirs"].astype(np.float32))
    out = shade(pt, env, smp, smp["dirs"], vis, bsdf, shadow_scale, n)
    out["vis"], out["fragile_ray"] = vis, frag_ray
    out["fragile_grad"] = out["fragile_grad"] | frag_ray.any(1)
    out["fragile_sample"] = out["fragile_sample"] | frag_ray
    out["fragile"] = out["fragile_sample"].any(1)
    return smp, out


def fragile_share(P: int, map_name: str, n: int, bsdf: str = "pbr") -> float:
    """the share of points the GPU comparisons leave out, gradients included (the wider of the two masks)"""
    return float(expected(P, map_name, n, bsdf)[1]["fragile_grad"].mean())
