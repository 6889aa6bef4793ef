"""TEST INFRASTRUCTURE -- CPU torch restatement of the reference's mesh -> Gaussians step (parity pinned by
tests/golden/ref_mgadapter.npz and ref_math.npz, which were produced by the reference's own functions:
scripts/make_golden.py).  Works in float32 and float64 (the float64 run is the autograd reference of
tests/test_gpu_mesh.py).  Nothing under geosplatting_amd/ imports this file.

Follows, statement by statement:
  safe_normalize      rfstudio/graphics/math.py:119-125
  rot2quat            rfstudio/graphics/math.py:246-278
  random_quaternion   rfstudio/graphics/math.py:59-72
  vertex_normals      rfstudio/graphics/_mesh/_triangle_mesh.py:588-615
  bary2gs / make      rfstudio/model/geosplat.py:390-424 / :426-472   (MGAdapter, default ratios :381-388)
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor


def safe_normalize(v: Tensor) -> Tensor:
    """rfstudio/graphics/math.py:119-125"""
    l = v.norm(dim=-1, keepdim=True)
    return torch.where(l < 1e-6, torch.tensor([0.0, 0.0, 1.0], dtype=v.dtype, device=v.device), v / l.clamp_min(1e-6))


def rot2quat(rots: Tensor, masked_sqrt: bool = False) -> Tensor:
    """Rotation matrices [*,3,3] -> quaternions wxyz [*,4]; best-conditioned branch of the four
    candidates (semantics of rfstudio/graphics/math.py:246-278).  masked_sqrt: same values, but a candidate with q <= 0 -- never the
    selected one -- is kept out of the square root, whose autograd there is 0 * inf = NaN (the kernels differentiate the selected
    candidate only); for float32 runs, where a q of a non-selected candidate rounds to <= 0 now and then."""
    m = rots.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    q = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1)
    q_abs = torch.where(q > 0, torch.sqrt(torch.where(q > 0, q, torch.ones_like(q))), torch.zeros_like(q)) if masked_sqrt \
        else torch.sqrt(q.clamp_min(0.0))
    cand = torch.stack([
        torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], -1),
    ], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = q_abs.argmax(-1)
    out = cand[torch.arange(cand.shape[0]), best]
    return out.reshape(rots.shape[:-2] + (4,))


def random_quaternion(n: int, gen: torch.Generator) -> Tensor:
    """rfstudio/graphics/math.py:59-72"""
    u = torch.rand(n, generator=gen); v = torch.rand(n, generator=gen) * (2 * math.pi)
    w = torch.rand(n, generator=gen) * (2 * math.pi)
    return torch.stack([torch.sqrt(1 - u) * torch.sin(v), torch.sqrt(1 - u) * torch.cos(v),
                        torch.sqrt(u) * torch.sin(w), torch.sqrt(u) * torch.cos(w)], -1)


def vertex_normals(vertices: Tensor, faces: Tensor) -> Tensor:
    """Area-weighted vertex normals (rfstudio/graphics/_mesh/_triangle_mesh.py:588-615)."""
    p = vertices[faces]                                     # [F,3,3]
    fn = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
    n = torch.zeros_like(vertices)
    n.index_add_(0, faces.reshape(-1), fn[:, None, :].expand(-1, 3, -1).reshape(-1, 3))
    return n / n.norm(dim=-1, keepdim=True)


def _bary2gs(p0, p1, area, normals, max_scale_ratio, g_scale_ratio=1.6, masked_sqrt=False):
    """rfstudio/model/geosplat.py:390-424"""
    means = (p0 + p1) / 2
    max_rots = p1 - means
    max_scales = max_rots.norm(dim=-1, keepdim=True).clamp(min=1e-10)
    min_scales = area / 4 / max_scales
    max_rots = max_rots / max_scales
    scales = torch.cat(((g_scale_ratio * max_scale_ratio * max_scales).log(),
                        (g_scale_ratio / max_scale_ratio * min_scales).log(),
                        torch.full_like(max_scales, -10.0)), dim=-1)
    min_rots = torch.cross(normals, max_rots, dim=-1)
    quats = rot2quat(torch.stack((max_rots, min_rots, normals), dim=-1), masked_sqrt)
    opac = torch.full_like(means[:, :1], 0.99).logit()
    return means, scales, quats, opac


def mesh_to_splats(vertices: Tensor, faces: Tensor, vnormals: Tensor, masked_sqrt: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """MGAdapter.make with its default ratios (rfstudio/model/geosplat.py:381-388,426-472):
    two rings of three Gaussians per face, colours = interpolated shading normals.
    Returns (means[6F,3], log_scales[6F,3], quats_wxyz[6F,4], logit_opacities[6F,1], shading_normals[6F,3]);
    row = part * F + face."""
    scale_ratio = (0.5, 1.3); l_scale_ratio = (1.0 / 3.0, 3.0); bias = (-1.0 / 24.0, 0.0)
    p0, p1, p2 = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    vn0, vn1, vn2 = vnormals[faces[:, 0]], vnormals[faces[:, 1]], vnormals[faces[:, 2]]
    fn = torch.cross(p1 - p0, p2 - p0, dim=-1)
    area = fn.norm(dim=-1, keepdim=True).clamp(min=1e-10) / 2
    fn = safe_normalize(fn)
    parts, shading = [], []
    for u_coeff, a_coeff, s_ratio in zip([1 / 9 + bias[0], 2 / 9 + bias[1]],
                                         [1 / 4 * l_scale_ratio[0], 1 / 12 * l_scale_ratio[1]], scale_ratio):
        u0 = p0 * (1 - 2 * u_coeff) + (p1 + p2) * u_coeff
        u1 = p1 * (1 - 2 * u_coeff) + (p2 + p0) * u_coeff
        u2 = p2 * (1 - 2 * u_coeff) + (p0 + p1) * u_coeff
        n0 = vn0 * (1 - 2 * u_coeff) + (vn1 + vn2) * u_coeff
        n1 = vn1 * (1 - 2 * u_coeff) + (vn2 + vn0) * u_coeff
        n2 = vn2 * (1 - 2 * u_coeff) + (vn0 + vn1) * u_coeff
        a = area * a_coeff
        for (a0, a1, na, nb) in ((u0, u1, n0, n1), (u1, u2, n1, n2), (u2, u0, n2, n0)):
            parts.append(_bary2gs(a0, a1, a, fn, s_ratio, masked_sqrt=masked_sqrt))
            shading.append(safe_normalize((na + nb) / 2))
    means, scales, quats, opac = (torch.cat([p[i] for p in parts], 0) for i in range(4))
    normals = torch.cat(shading, 0)
    return means, scales, quats, opac, normals


def mesh_to_splats_set(vertices: Tensor, faces: Tensor, vnormals: Tensor):
    """Same, returned as (object with .means/.scales/.quats/.opacities/.colors/.num, shading_normals) -- the shape of
    the product's ``geosplatting_amd.mesh.mesh_to_splats`` result, for side-by-side comparisons in the tests."""
    from types import SimpleNamespace
    means, scales, quats, opac, normals = mesh_to_splats(vertices, faces, vnormals)
    return SimpleNamespace(means=means, scales=scales, quats=quats, opacities=opac, colors=normals.clone(),
                           num=means.shape[0]), normals


def scene_builder(vertices: Tensor, faces: Tensor):
    """``mesh_to_splats_fn`` argument of geosplatting_amd.synthetic.sphere_scene for suites without a GPU."""
    return mesh_to_splats(vertices, faces, vertex_normals(vertices, faces))


# ------------------------------------------------------------------------------------------------ per-element error budgets
# Units of 2^-24 (float32 unit roundoff), first order, computed in float64 from the float64 intermediates -- the rules of
# oracle/flexicubes_ref.py: a cross product is charged by the sum of the sizes of its products (a sliver's normal is a small
# difference of large products), a vertex collecting n contributions through atomics by sum(own bounds) + (n - 1) sum |c|.
def _cross_b(a, ea, b, eb):
    """a x b for arrays [..., 3] with bounds: value, bound, sum of the sizes of the products"""
    import numpy as np
    i1, i2 = [1, 2, 0], [2, 0, 1]
    v = a[..., i1] * b[..., i2] - a[..., i2] * b[..., i1]
    m = np.abs(a[..., i1] * b[..., i2]) + np.abs(a[..., i2] * b[..., i1])
    e = (ea[..., i1] * np.abs(b[..., i2]) + np.abs(a[..., i1]) * eb[..., i2] + ea[..., i2] * np.abs(b[..., i1])
         + np.abs(a[..., i2]) * eb[..., i1] + m + np.abs(v))
    return v, e, m


def vertex_normals_budget(vertices, faces, v_vnormals=None):
    """float64 `vertex_normals` on float32 vertices, its gradient for the cotangent v_vnormals, and budgets: dict(vnormals,
    vnormals_budget, valence, g_vertices, g_vertices_budget, g_vertices_n).  A vertex on no face has no normal in the restatement
    (0 / 0): `isolated` marks it; there the value is the fixing constant (0, 0, 1) of compute_vertex_normals(fix=True), budget 0, and
    the gradient has no contribution."""
    import numpy as np
    x32 = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))
    f = np.asarray(faces, dtype=np.int64)
    V, F = x32.shape[0], f.shape[0]
    x = x32.astype(np.float64)
    valence = np.bincount(f.reshape(-1), minlength=V)
    out = dict(valence=valence, isolated=valence == 0)
    p = x[f]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    fn, e_fn, _ = _cross_b(e1, np.abs(e1), e2, np.abs(e2))
    sc = lambda idx, val: np.stack([np.bincount(idx, val[:, k], V) for k in range(3)], -1)
    rep = lambda a: np.repeat(a[:, None, :], 3, 1).reshape(-1, 3)
    fl = f.reshape(-1)
    raw = sc(fl, rep(fn))
    n_c = sc(fl, rep((fn != 0).astype(np.float64)))
    e_raw = sc(fl, rep(e_fn)) + np.maximum(n_c - 1, 0) * sc(fl, rep(np.abs(fn)))
    l = np.sqrt((raw * raw).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = raw / l
        e_l = (np.abs(n) * e_raw).sum(-1, keepdims=True) + 3 * l
        e_n = e_raw / l + np.abs(n) * (e_l / l + 1)
    iso = (valence == 0)[:, None]                                          # compute_vertex_normals(fix=True): the constant (0, 0, 1), exactly
    n, e_n = np.where(iso, np.array([0.0, 0.0, 1.0]), n), np.where(iso, 0.0, e_n)
    out.update(vnormals=n, vnormals_budget=e_n, raw_len=l[:, 0])
    if v_vnormals is None:
        return out
    a = np.asarray(v_vnormals, dtype=np.float32).astype(np.float64)
    xt = torch.from_numpy(x).requires_grad_(True)
    ft = torch.from_numpy(f)
    live = torch.from_numpy(valence > 0)
    (vertex_normals(xt, ft)[live] * torch.from_numpy(a)[live]).sum().backward()
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (n * a).sum(-1, keepdims=True)
        e_d = (e_n * np.abs(a) + 2 * np.abs(n * a)).sum(-1, keepdims=True)
        g = (a - n * d) / l
        e_g = (e_n * np.abs(d) + np.abs(n) * e_d + 2 * np.abs(n * d) + np.abs(a) + np.abs(a - n * d)) / l + np.abs(g) * (e_l / l + 1)
    g, e_g = np.where(valence[:, None] > 0, g, 0.0), np.where(valence[:, None] > 0, e_g, 0.0)
    gf = g[f].sum(1)                                                      # [F, 3]: the sum over the face's corners
    e_gf = e_g[f].sum(1) + 2 * np.abs(g[f]).sum(1)
    g1, e_g1, m1 = _cross_b(e2, np.abs(e2), gf, e_gf)
    g2, e_g2, m2 = _cross_b(gf, e_gf, e1, np.abs(e1))
    c = np.stack((-(g1 + g2), g1, g2), 1).reshape(-1, 3)                  # contribution of the face to its corners 0, 1, 2
    e_c = np.stack((e_g1 + e_g2 + np.abs(g1) + np.abs(g2), e_g1, e_g2), 1).reshape(-1, 3)
    m_c = np.stack((m1 + m2, m1, m2), 1).reshape(-1, 3)
    cnt = sc(fl, ((c != 0) | (e_c > 0)).astype(np.float64))
    bud = np.where(cnt > 0, sc(fl, e_c) + np.maximum(cnt - 1, 0) * sc(fl, m_c), 0.0)
    gv = xt.grad.numpy()
    hand = sc(fl, c)
    assert np.allclose(hand, gv, rtol=1e-7, atol=1e-9 * max(float(np.abs(c).max(initial=0)), 1e-300)), "hand-derived gradient != autograd"
    out.update(g_vertices=gv, g_vertices_budget=bud, g_vertices_n=cnt)
    return out


class _B:
    """a float64 array with a first-order bound (units of 2^-24) on what a float32 evaluation of the same operations may differ by:
    every operation propagates its operands' bounds and adds one rounding of its result"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        import numpy as np
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    @staticmethod
    def lift(x):
        return x if isinstance(x, _B) else _B(float(x))

    def __add__(self, o):
        import numpy as np
        o = _B.lift(o); v = self.v + o.v
        return _B(v, self.e + o.e + np.abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        import numpy as np
        o = _B.lift(o); v = self.v - o.v
        return _B(v, self.e + o.e + np.abs(v))

    def __rsub__(self, o):
        return _B.lift(o) - self

    def __neg__(self):
        return _B(-self.v, self.e)

    def __mul__(self, o):
        import numpy as np
        o = _B.lift(o); v = self.v * o.v
        return _B(v, self.e * np.abs(o.v) + np.abs(self.v) * o.e + np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        import numpy as np
        o = _B.lift(o); v = self.v / o.v
        return _B(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + np.abs(v))

    def sqrt(self):
        import numpy as np
        s = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _B(s, np.where(s > 0, self.e * 0.5 / s, 0.0) + 2 * s)

    def log(self):
        import numpy as np
        l = np.log(self.v)
        return _B(l, self.e / np.abs(self.v) + 2 * np.abs(l) + 2)          # logf: two roundings of the result, absolute near log 1 = 0

    def val(self):
        return self.v

    @staticmethod
    def where(m, a, b):
        import numpy as np
        a, b = _B.lift(a), _B.lift(b)
        return _B(np.where(m, a.v, b.v), np.where(m, a.e, b.e))

    def clamp_min(self, c):
        return _B.where(self.v < c, c, self)


class _Dual:
    """the kernels' dual numbers (csrc/gs_mesh.hip) over _B: value and one tangent, operator for operator"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v = _B.lift(v); self.d = _B(0.0) if d is None else _B.lift(d)

    @staticmethod
    def lift(x):
        return x if isinstance(x, _Dual) else _Dual(x)

    def __add__(self, o):
        o = _Dual.lift(o); return _Dual(self.v + o.v, self.d + o.d)
    __radd__ = __add__

    def __sub__(self, o):
        o = _Dual.lift(o); return _Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return _Dual.lift(o) - self

    def __neg__(self):
        return _Dual(-self.v, -self.d)

    def __mul__(self, o):
        if not isinstance(o, _Dual):
            return _Dual(self.v * o, self.d * o)
        return _Dual(self.v * o.v, self.d * o.v + self.v * o.d)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, _Dual):
            return _Dual(self.v / o, self.d / o)
        q = self.v / o.v
        return _Dual(q, (self.d - q * o.d) / o.v)

    def sqrt(self):
        s = self.v.sqrt(); return _Dual(s, self.d * 0.5 / s)

    def log(self):
        return _Dual(self.v.log(), self.d / self.v)

    def val(self):
        return self.v.v

    @staticmethod
    def where(m, a, b):
        a, b = _Dual.lift(a), _Dual.lift(b)
        return _Dual(_B.where(m, a.v, b.v), _B.where(m, a.d, b.d))

    def clamp_min(self, c):
        return _Dual.where(self.val() < c, _Dual(c), self)


def _face_chain(T, P, VN):
    """mgadapter_face of csrc/gs_mesh.hip over the number type T (_B or _Dual), operation for operation: P, VN [3][3] of T ->
    (means, scales [6][3], quats [6][4], normals [6][3], selected rot2quat candidate [6] of int arrays)"""
    import numpy as np
    cst = lambda x: T.lift(_B(float(x), abs(float(x))))                  # a constant the kernel holds rounded to float32
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    norm = lambda a: (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]).sqrt()

    def safe_normalize(v):
        l = norm(v)
        small = l.val() < 1e-6
        lc = l.clamp_min(1e-6)
        return [T.where(small, c, v[k] / lc) for k, c in enumerate((0.0, 0.0, 1.0))]

    def rot2quat(m):
        qq = [1.0 + m[0][0] + m[1][1] + m[2][2], 1.0 + m[0][0] - m[1][1] - m[2][2], 1.0 - m[0][0] + m[1][1] - m[2][2],
              1.0 - m[0][0] - m[1][1] + m[2][2]]
        qa = [T.where(q.val() > 0, T.where(q.val() > 0, q, 1.0).sqrt(), 0.0) for q in qq]
        best = np.argmax(np.stack([np.broadcast_to(q.val(), np.broadcast_shapes(*[x.val().shape for x in qa])) for q in qa]), 0)
        cands = [[qa[0] * qa[0], m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]],
                 [m[2][1] - m[1][2], qa[1] * qa[1], m[1][0] + m[0][1], m[0][2] + m[2][0]],
                 [m[0][2] - m[2][0], m[1][0] + m[0][1], qa[2] * qa[2], m[1][2] + m[2][1]],
                 [m[1][0] - m[0][1], m[2][0] + m[0][2], m[2][1] + m[1][2], qa[3] * qa[3]]]
        pick = lambda xs: T.where(best == 0, xs[0], T.where(best == 1, xs[1], T.where(best == 2, xs[2], xs[3])))
        den = 2.0 * pick(qa).clamp_min(0.1)
        return [pick([cands[b][i] for b in range(4)]) / den for i in range(4)], best

    def bary2gs(a0, a1, area, fnn, s_ratio):
        mean = [(a0[k] + a1[k]) / 2.0 for k in range(3)]
        mr = [a1[k] - mean[k] for k in range(3)]
        ms = norm(mr).clamp_min(1e-10)
        mins = area / 4.0 / ms
        mr = [mr[k] / ms for k in range(3)]
        scale = [(cst(1.6 * s_ratio) * ms).log(), (cst(1.6 / s_ratio) * mins).log(), T.lift(-10.0)]
        minr = cross(fnn, mr)
        R = [[mr[k], minr[k], fnn[k]] for k in range(3)]
        quat, best = rot2quat(R)
        return mean, scale, quat, best

    e1 = [P[1][k] - P[0][k] for k in range(3)]; e2 = [P[2][k] - P[0][k] for k in range(3)]
    fn = cross(e1, e2)
    area = norm(fn).clamp_min(1e-10) / 2.0
    fnn = safe_normalize(fn)
    u_c = (1.0 / 9.0 - 1.0 / 24.0, 2.0 / 9.0)
    a_c = (0.25 * (1.0 / 3.0), (1.0 / 12.0) * 3.0)
    s_r = (0.5, 1.3)
    means, scales, quats, normals, bests = [], [], [], [], []
    for ring in range(2):
        u, c0 = cst(u_c[ring]), cst(1.0 - 2.0 * u_c[ring])
        U = [[P[i][k] * c0 + (P[(i + 1) % 3][k] + P[(i + 2) % 3][k]) * u for k in range(3)] for i in range(3)]
        Nn = [[VN[i][k] * c0 + (VN[(i + 1) % 3][k] + VN[(i + 2) % 3][k]) * u for k in range(3)] for i in range(3)]
        a = area * cst(a_c[ring])
        for e in range(3):
            i0, i1 = e, (e + 1) % 3
            m, s, q, b = bary2gs(U[i0], U[i1], a, fnn, s_r[ring])
            means.append(m); scales.append(s); quats.append(q); bests.append(b)
            normals.append(safe_normalize([(Nn[i0][k] + Nn[i1][k]) / 2.0 for k in range(3)]))
    return means, scales, quats, normals, bests


def mesh_to_splats_budget(vertices, faces, vnormals, cot=None, quat_sign=None):
    """float64 `mesh_to_splats` on float32 inputs with budgets, forward and (for the cotangents cot = (v_means, v_scales, v_quats,
    v_normals), rows part * F + face) backward.  quat_sign [6F, 1] (+-1) multiplies the reference's quaternions and their cotangent:
    rot2quat picks one of four candidates by value and a float32 evaluation may pick another, which is the same rotation with the
    opposite sign.  The forward budgets come from evaluating csrc/gs_mesh.hip's operations on (value, bound) pairs; the gradient's from
    the same operations on the kernels' dual numbers over such pairs: a face's contribution to one input coordinate is the dot product
    of the 78 output tangents with the cotangents (own bound + 77 sum |g d|), and a vertex collects its faces' contributions through
    atomics (sum of own bounds + (valence - 1) sum |g d|).  Returns dict(means, scales, quats, normals [+ _budget], candidates [6F],
    g_vertices, g_vnormals [+ _budget, _n])."""
    import numpy as np
    x = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    vn = np.asarray(vnormals, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64)
    V, F = x.shape[0], f.shape[0]
    xt, nt, ft = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(vn).requires_grad_(True), torch.from_numpy(f)
    means, scales, quats, _, normals = mesh_to_splats(xt, ft, nt)
    sign = torch.ones(6 * F, 1, dtype=torch.float64) if quat_sign is None else torch.from_numpy(np.asarray(quat_sign, dtype=np.float64).reshape(-1, 1))
    quats = quats * sign
    P = [[_B(x[f[:, i], k]) for k in range(3)] for i in range(3)]
    N = [[_B(vn[f[:, i], k]) for k in range(3)] for i in range(3)]
    bm, bs, bq, bn, best = _face_chain(_B, P, N)
    cat = lambda parts, w, attr: np.concatenate([np.stack([np.broadcast_to(getattr(p[k], attr), (F,)) for k in range(w)], -1) for p in parts], 0)
    out = dict(candidates=np.concatenate(best), means=means.detach().numpy(), scales=scales.detach().numpy(), quats=quats.detach().numpy(),
               normals=normals.detach().numpy(), means_budget=cat(bm, 3, "e"), scales_budget=cat(bs, 3, "e"), quats_budget=cat(bq, 4, "e"),
               normals_budget=cat(bn, 3, "e"))
    assert np.allclose(cat(bm, 3, "v"), out["means"], atol=1e-12) and np.allclose(cat(bn, 3, "v"), out["normals"], atol=1e-9)
    assert np.allclose(cat(bq, 4, "v") * sign.numpy() * np.sign((cat(bq, 4, "v") * sign.numpy() * out["quats"]).sum(-1, keepdims=True)), out["quats"], atol=1e-7)
    if cot is None:
        return out
    gm, gs, gq, gn = (np.asarray(c, dtype=np.float32).astype(np.float64) for c in cot)
    gq = gq * sign.numpy()
    ((means * torch.from_numpy(gm)).sum() + (scales * torch.from_numpy(gs)).sum() + (quats * torch.from_numpy(gq / sign.numpy())).sum()
     + (normals * torch.from_numpy(gn)).sum()).backward()
    eye = np.eye(18)[:, :, None]                                           # [direction, input coordinate, 1]: one-hot tangents
    DP = [[_Dual(P[i][k], _B(np.broadcast_to(eye[:, i * 3 + k], (18, F)).copy())) for k in range(3)] for i in range(3)]
    DN = [[_Dual(N[i][k], _B(np.broadcast_to(eye[:, 9 + i * 3 + k], (18, F)).copy())) for k in range(3)] for i in range(3)]
    dm, ds, dq, dn, _ = _face_chain(_Dual, DP, DN)
    acc, e_acc, m_acc = np.zeros((18, F)), np.zeros((18, F)), np.zeros((18, F))
    for part in range(6):
        rows = slice(part * F, (part + 1) * F)
        for outs, g in ((dm[part], gm[rows]), (ds[part], gs[rows]), (dn[part], gn[rows]), (dq[part], gq[rows])):
            for k, o in enumerate(outs):
                t = g[:, k][None] * o.d.v
                acc += t; e_acc += np.abs(g[:, k])[None] * o.d.e + np.abs(t); m_acc += np.abs(t)
    e_acc = e_acc + 77 * m_acc
    flat = np.broadcast_to(f.T[:, None, :] * 3 + np.arange(3)[None, :, None], (3, 3, F)).reshape(9, F)     # [corner * 3 + k, F] -> 3 vid + k
    for name, lo, ref in (("g_vertices", 0, xt.grad.numpy()), ("g_vnormals", 9, nt.grad.numpy())):
        c, e_c, m_c = acc[lo:lo + 9].reshape(-1), e_acc[lo:lo + 9].reshape(-1), m_acc[lo:lo + 9].reshape(-1)
        idx = flat.reshape(-1)
        cnt = np.bincount(idx, ((c != 0) | (e_c > 0)).astype(np.float64), 3 * V)
        bud = np.where(cnt > 0, np.bincount(idx, e_c, 3 * V) + np.maximum(cnt - 1, 0) * np.bincount(idx, m_c, 3 * V), 0.0)
        hand = np.bincount(idx, c, 3 * V).reshape(V, 3)
        assert np.allclose(hand, ref, rtol=1e-6, atol=1e-9 * max(float(np.abs(c).max(initial=0)), 1e-300)), f"dual-number {name} != autograd"
        out.update({name: ref, name + "_budget": bud.reshape(V, 3), name + "_n": cnt.reshape(V, 3)})
    return out
