"""TEST INFRASTRUCTURE (CPU only): the surfel projection of csrc/gs_surfel.hip and the SH colours of csrc/gs_sh_dev.h, restated
operation for operation over two number types:

  * (value, bound) pairs -- `_B` of oracle/mesh_ref.py: float64 values with a first-order running-error bound in units of 2^-24 that
    charges one rounding per operation.  `1.0f / x`, `1.0f / sqrtf(x)` and `rsqrtf` are charged three roundings: the kernels whose
    results are only gradients are compiled with contraction on and may use v_rcp_f32 / v_rsq_f32 (1 ulp).  A fused multiply-add only
    removes a rounding, so the bound holds either way.  A literal the kernel holds rounded to float32 carries a bound of its own size.
  * numpy float32 (`_F`): the same chains as an all-float32 evaluation, which tests/test_surfel_project_cpu.py measures against the
    bound.

The chains are written ONCE over a small table of operations (`_OB` / `_OF`), so both restatements are the same statements.

  project_fwd_budget   surfel_project: quat_to_rotmat_exact, surfel_cam_mean, surfel_cam_rot, M, d, f, means2d, the extents -> value
                       and bound of the nine ray-transform entries, means2d, depth and the normal, and the float64 decisions (the two
                       depth culls, d == 0, the radius, radius_clip, the four screen tests, the tile rectangle, the normal's sign),
                       each with its margin in units of the bound of the quantity compared.  The values are asserted equal to
                       tests/surfel_ref.py::project in float64.
  project_bwd_budget   surfel_project_bwd_kernel, statement for statement, with the SH backward (sh_color_bwd_row) when a degree is
                       given.  The normal's sign is an INPUT (the sign the GPU stored).  The values are asserted equal to torch float64
                       autograd of surfel_ref.project (+ surfel_ref.sh_colors) under the same cotangents and the same flip.
  sh_fwd_budget        sh_dir, sh_basis<DEG>, sh_color_deg and the clamp rule: colour, bound, margin of c + 0.5 against 0.
  *_f32                the float32 restatements.

Scenes (budget_scene): Gaussians placed per regime in the camera space of the view and mapped back through it, culled rows
interleaved in one random order; a Gaussian with any decision margin below 2 * kappa bounds is drawn again at construction, so no
Gaussian is ever excluded from a check.  The one exception is the normal's sign, which the reference takes from the GPU.
"""
import functools
import math

import numpy as np
import torch

from oracle.mesh_ref import _B, rot2quat
from tests import surfel_ref
from tests.util import SH_KAPPA, SURFEL_PROJ_KAPPA

EPS32 = 2.0 ** -24
TILE = 16
FAR = 2048.0                                # every near / far plane is exact in float32
SF_MAX_RADIUS = 16777216.0
RADIUS_BIG = 1024
MARGIN_KAPPA = max(SURFEL_PROJ_KAPPA, SH_KAPPA)    # the builders redraw below 2 * MARGIN_KAPPA bounds


# ------------------------------------------------------------------------------------------------ the two number types
class _F:
    """numpy float32, operator for operator"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float32)

    @staticmethod
    def lift(x):
        return x if isinstance(x, _F) else _F(np.float32(x))

    def __add__(self, o):
        return _F(self.v + _F.lift(o).v)
    __radd__ = __add__

    def __sub__(self, o):
        return _F(self.v - _F.lift(o).v)

    def __rsub__(self, o):
        return _F(_F.lift(o).v - self.v)

    def __neg__(self):
        return _F(-self.v)

    def __mul__(self, o):
        return _F(self.v * _F.lift(o).v)
    __rmul__ = __mul__


class _OB:
    """operations over _B"""
    @staticmethod
    def inp(a):                                  # a float32 input: exact
        return _B(np.asarray(a, dtype=np.float32).astype(np.float64))

    @staticmethod
    def cst(x):                                  # a literal held rounded to float32
        return _B(np.float64(x), np.float64(abs(x)))

    @staticmethod
    def rcp(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = 1.0 / x.v
            return _B(v, np.abs(v) * x.e / np.abs(x.v) + 3.0 * np.abs(v))

    @staticmethod
    def rsqrt(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = 1.0 / np.sqrt(x.v)
            return _B(v, 0.5 * np.abs(v) * x.e / np.abs(x.v) + 3.0 * np.abs(v))

    @staticmethod
    def sqrt(x):
        return x.sqrt()

    @staticmethod
    def vabs(x):
        return _B(np.abs(x.v), x.e)

    @staticmethod
    def vmax(a, b):                              # max is 1-Lipschitz in each argument and rounds nothing
        a, b = _B.lift(a), _B.lift(b)
        return _B(np.maximum(a.v, b.v), np.maximum(a.e, b.e))

    @staticmethod
    def where(m, a, b):
        return _B.where(m, a, b)

    @staticmethod
    def val(x):
        return x.v


class _OF:
    """operations over _F"""
    @staticmethod
    def inp(a):
        return _F(a)

    @staticmethod
    def cst(x):
        return _F(np.float32(x))

    @staticmethod
    def rcp(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _F(np.float32(1.0) / x.v)

    @staticmethod
    def rsqrt(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _F(np.float32(1.0) / np.sqrt(x.v))

    @staticmethod
    def sqrt(x):
        return _F(np.sqrt(x.v))

    @staticmethod
    def vabs(x):
        return _F(np.abs(x.v))

    @staticmethod
    def vmax(a, b):
        return _F(np.maximum(_F.lift(a).v, _F.lift(b).v))

    @staticmethod
    def where(m, a, b):
        return _F(np.where(m, _F.lift(a).v, _F.lift(b).v))

    @staticmethod
    def val(x):
        return x.v


# ------------------------------------------------------------------------------------------------ the chains
def _cam(O, viewmat, K):
    vm, K = np.asarray(viewmat, np.float32), np.asarray(K, np.float32)
    return dict(R=[O.inp(vm[i, j]) for i in range(3) for j in range(3)], t=[O.inp(vm[i, 3]) for i in range(3)],
                fx=O.inp(K[0, 0]), fy=O.inp(K[1, 1]), cx=O.inp(K[0, 2]), cy=O.inp(K[1, 2]))


def _cols(O, a):
    a = np.asarray(a, np.float32)
    return [O.inp(a[:, k]) for k in range(a.shape[1])]


def _frame(O, cam, mean, quat):
    """surfel_cam_mean, surfel_cam_rot (quat_to_rotmat_exact) and the sum surfel_normal_sign tests"""
    R, t = cam["R"], cam["t"]
    mc = [((R[3 * i] * mean[0] + R[3 * i + 1] * mean[1]) + R[3 * i + 2] * mean[2]) + t[i] for i in range(3)]
    qw, qx, qy, qz = quat
    n2 = ((qx * qx + qy * qy) + qz * qz) + qw * qw
    inv = O.rsqrt(n2)
    x, y, z, w = qx * inv, qy * inv, qz * inv, qw * inv
    x2, y2, z2 = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    Rq = [1.0 - 2.0 * (y2 + z2), 2.0 * (xy - wz), 2.0 * (xz + wy),
          2.0 * (xy + wz), 1.0 - 2.0 * (x2 + z2), 2.0 * (yz - wx),
          2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (x2 + y2)]
    Rc = [(R[3 * i] * Rq[j] + R[3 * i + 1] * Rq[3 + j]) + R[3 * i + 2] * Rq[6 + j] for i in range(3) for j in range(3)]
    dot = (Rc[2] * mc[0] + Rc[5] * mc[1]) + Rc[8] * mc[2]
    return mc, Rc, dot


def _fwd_chain(O, cam, mean, quat, s0, s1):
    """surfel_project up to the radius: dict(mc, Rc, dot, M [9], d, mx, my, ex, ey, pre = 3 sqrt(max(1e-4, max(ex, ey))))"""
    mc, Rc, dot = _frame(O, cam, mean, quat)
    Hm = [None] * 9
    for i in range(3):
        Hm[3 * i], Hm[3 * i + 1], Hm[3 * i + 2] = s0 * Rc[3 * i], s1 * Rc[3 * i + 1], mc[i]
    M0 = [cam["fx"] * Hm[j] + cam["cx"] * Hm[6 + j] for j in range(3)]
    M1 = [cam["fy"] * Hm[3 + j] + cam["cy"] * Hm[6 + j] for j in range(3)]
    M2 = [Hm[6 + j] for j in range(3)]
    d = (M2[0] * M2[0] + M2[1] * M2[1]) - M2[2] * M2[2]
    f = O.rcp(d)
    mx = f * ((M0[0] * M2[0] + M0[1] * M2[1]) - M0[2] * M2[2])
    my = f * ((M1[0] * M2[0] + M1[1] * M2[1]) - M1[2] * M2[2])
    ex = mx * mx - f * ((M0[0] * M0[0] + M0[1] * M0[1]) - M0[2] * M0[2])
    ey = my * my - f * ((M1[0] * M1[0] + M1[1] * M1[1]) - M1[2] * M1[2])
    ext = O.vmax(ex, ey)
    pre = 3.0 * O.sqrt(O.vmax(O.cst(1e-4), ext))
    return dict(mc=mc, Rc=Rc, dot=dot, M=M0 + M1 + M2, d=d, mx=mx, my=my, ex=ex, ey=ey, ext=ext, pre=pre)


def _bwd_chain(O, cam, mean, quat, s0, s1, sgn, vM, vm2, vdepth, vn):
    """surfel_project_bwd_kernel without its colour part: (v_mean [3], g_quats [4], gs0, gs1).  sgn: array of +-1."""
    R = cam["R"]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    mc, Rc, _ = _frame(O, cam, mean, quat)
    M0, M1, M2 = [], [], []
    for j in range(3):
        h0 = s0 * Rc[0] if j == 0 else s1 * Rc[1] if j == 1 else mc[0]
        h1 = s0 * Rc[3] if j == 0 else s1 * Rc[4] if j == 1 else mc[1]
        h2 = s0 * Rc[6] if j == 0 else s1 * Rc[7] if j == 1 else mc[2]
        M0.append(fx * h0 + cx * h2); M1.append(fy * h1 + cy * h2); M2.append(h2)
    vM0, vM1, vM2 = list(vM[0:3]), list(vM[3:6]), list(vM[6:9])
    vmx, vmy = vm2
    d = M2[0] * M2[0] + M2[1] * M2[1] - M2[2] * M2[2]
    f = O.rcp(d)
    mx = f * (M0[0] * M2[0] + M0[1] * M2[1] - M0[2] * M2[2])
    my = f * (M1[0] * M2[0] + M1[1] * M2[1] - M1[2] * M2[2])
    vd = -(vmx * mx + vmy * my) * f
    for j in range(3):
        t = -f if j == 2 else f
        vM0[j] = vM0[j] + vmx * t * M2[j]
        vM1[j] = vM1[j] + vmy * t * M2[j]
        vM2[j] = vM2[j] + (t * (vmx * M0[j] + vmy * M1[j]) + 2.0 * vd * (-M2[j] if j == 2 else M2[j]))
    vH = [None] * 9
    for j in range(3):
        vH[j] = fx * vM0[j]
        vH[3 + j] = fy * vM1[j]
        vH[6 + j] = cx * vM0[j] + cy * vM1[j] + vM2[j]
    v_mc = [vH[2], vH[5], vH[8]]
    if vdepth is not None:
        v_mc[2] = v_mc[2] + vdepth
    neg = np.asarray(sgn) < 0
    vRc = [None] * 9
    for i in range(3):
        vRc[3 * i] = s0 * vH[3 * i]
        vRc[3 * i + 1] = s1 * vH[3 * i + 1]
        vRc[3 * i + 2] = O.where(neg, -vn[i], vn[i])                      # sgn * v_normals: exact
    gs0 = vH[0] * Rc[0] + vH[3] * Rc[3] + vH[6] * Rc[6]
    gs1 = vH[1] * Rc[1] + vH[4] * Rc[4] + vH[7] * Rc[7]
    v_mean = [R[i] * v_mc[0] + R[3 + i] * v_mc[1] + R[6 + i] * v_mc[2] for i in range(3)]
    v_Rq = [R[i] * vRc[j] + R[3 + i] * vRc[3 + j] + R[6 + i] * vRc[6 + j] for i in range(3) for j in range(3)]
    qw, qx, qy, qz = quat
    inv = O.rsqrt(qx * qx + qy * qy + qz * qz + qw * qw)
    w, xq, yq, zq = qw * inv, qx * inv, qy * inv, qz * inv
    VR = lambda i, j: v_Rq[3 * i + j]
    vqn = [2.0 * (xq * (VR(2, 1) - VR(1, 2)) + yq * (VR(0, 2) - VR(2, 0)) + zq * (VR(1, 0) - VR(0, 1))),
           2.0 * (-2.0 * xq * (VR(1, 1) + VR(2, 2)) + yq * (VR(1, 0) + VR(0, 1)) + zq * (VR(2, 0) + VR(0, 2)) + w * (VR(2, 1) - VR(1, 2))),
           2.0 * (xq * (VR(1, 0) + VR(0, 1)) - 2.0 * yq * (VR(0, 0) + VR(2, 2)) + zq * (VR(2, 1) + VR(1, 2)) + w * (VR(0, 2) - VR(2, 0))),
           2.0 * (xq * (VR(2, 0) + VR(0, 2)) + yq * (VR(2, 1) + VR(1, 2)) - 2.0 * zq * (VR(0, 0) + VR(1, 1)) + w * (VR(1, 0) - VR(0, 1)))]
    qn = [w, xq, yq, zq]
    dotp = vqn[0] * qn[0] + vqn[1] * qn[1] + vqn[2] * qn[2] + vqn[3] * qn[3]
    g_quats = [(vqn[k] - dotp * qn[k]) * inv for k in range(4)]
    return v_mean, g_quats, gs0, gs1


# ----- gs_sh_dev.h
def _sh_campos(O, cam):
    R, t = cam["R"], cam["t"]
    return [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]


def _sh_dir(O, cam, mean):
    cp = _sh_campos(O, cam)
    dx, dy, dz = mean[0] - cp[0], mean[1] - cp[1], mean[2] - cp[2]
    inorm = O.rsqrt(dx * dx + dy * dy + dz * dz)
    return dx * inorm, dy * inorm, dz * inorm, inorm


def _sh_basis(O, deg, x, y, z):
    c = O.cst
    b = [c(0.2820947917738781)]
    if deg >= 1:
        b += [c(-0.48860251190292) * y, c(0.48860251190292) * z, c(-0.48860251190292) * x]
    if deg >= 2:
        z2, fTmp0B, fC1, fS1 = z * z, c(-1.092548430592079) * z, x * x - y * y, 2.0 * x * y
        b += [c(0.5462742152960395) * fS1, fTmp0B * y, c(0.9461746957575601) * z2 - c(0.3153915652525201), fTmp0B * x,
              c(0.5462742152960395) * fC1]
        if deg >= 3:
            fTmp0C, fTmp1B = c(-2.285228997322329) * z2 + c(0.4570457994644658), c(1.445305721320277) * z
            fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
            b += [c(-0.5900435899266435) * fS2, fTmp1B * fS1, fTmp0C * y, z * (c(1.865881662950577) * z2 - c(1.119528997770346)),
                  fTmp0C * x, fTmp1B * fC1, c(-0.5900435899266435) * fC2]
    return b


def _sh_basis_vjp(O, deg, x, y, z, vb):
    c = O.cst
    vx = vy = vz = None
    if deg >= 1:
        C1 = c(0.48860251190292)
        vx, vy, vz = -C1 * vb[3], -C1 * vb[1], C1 * vb[2]                  # 0 + . is exact
    if deg >= 2:
        A, B = c(1.092548430592079), c(0.5462742152960395)
        vx = vx + (A * y * vb[4] - A * z * vb[7] + 2.0 * B * x * vb[8])
        vy = vy + (A * x * vb[4] - A * z * vb[5] - 2.0 * B * y * vb[8])
        vz = vz + (-A * y * vb[5] + 2.0 * c(0.9461746957575601) * z * vb[6] - A * x * vb[7])
        if deg >= 3:
            E, F, G, H0 = c(-0.5900435899266435), c(1.445305721320277), c(-2.285228997322329), c(0.4570457994644658)
            xx, yy, zz = x * x, y * y, z * z
            fTmp0C = G * zz + H0
            vx = vx + (E * 6.0 * x * y * vb[9] + F * 2.0 * y * z * vb[10] + fTmp0C * vb[13] + F * 2.0 * x * z * vb[14]
                       + E * 3.0 * (xx - yy) * vb[15])
            vy = vy + (E * 3.0 * (xx - yy) * vb[9] + F * 2.0 * x * z * vb[10] + fTmp0C * vb[11] - F * 2.0 * y * z * vb[14]
                       - E * 6.0 * x * y * vb[15])
            vz = vz + (F * 2.0 * x * y * vb[10] + 2.0 * G * z * y * vb[11]
                       + (3.0 * c(1.865881662950577) * zz - c(1.119528997770346)) * vb[12] + 2.0 * G * z * x * vb[13]
                       + F * (xx - yy) * vb[14])
    return vx, vy, vz


def _sh_color_chain(O, cam, deg, mean, co):
    """sh_color_deg on the row co[k][ch]: (c [3] before the + 0.5, c + 0.5 [3], basis, (x, y, z, inorm))"""
    nb = (deg + 1) ** 2
    zero = O.inp(np.zeros_like(O.val(mean[0]), dtype=np.float32))
    x, y, z, inorm = _sh_dir(O, cam, mean) if deg >= 1 else (zero, zero, zero, zero)
    b = _sh_basis(O, deg, x, y, z)
    c = []
    for ch in range(3):
        acc = b[0] * co[0][ch]
        for k in range(1, nb):
            acc = acc + b[k] * co[k][ch]
        c.append(acc)
    return c, [a + 0.5 for a in c], b, (x, y, z, inorm)


def _sh_bwd_chain(O, cam, deg, mean, co, v_rgb):
    """sh_color_bwd_row of a visible Gaussian: (g [nb][3], direction term [3] or None, passes [3] bool)"""
    nb = (deg + 1) ** 2
    c, c5, b, (x, y, z, inorm) = _sh_color_chain(O, cam, deg, mean, co)
    passes = [O.val(a) >= 0 for a in c5]
    vc = [O.where(passes[ch], v_rgb[ch], 0.0) for ch in range(3)]
    g = [[b[k] * vc[ch] for ch in range(3)] for k in range(nb)]
    if deg == 0:
        return g, None, passes
    vb = [co[k][0] * vc[0] + co[k][1] * vc[1] + co[k][2] * vc[2] for k in range(nb)]
    vx, vy, vz = _sh_basis_vjp(O, deg, x, y, z, vb)
    dotp = vx * x + vy * y + vz * z
    return g, [(vx - dotp * x) * inorm, (vy - dotp * y) * inorm, (vz - dotp * z) * inorm], passes


def _sh_rows(O, coeffs, nb):
    co = np.asarray(coeffs, np.float32)
    return [[O.inp(co[:, k, ch]) for ch in range(3)] for k in range(nb)]


# ------------------------------------------------------------------------------------------------ forward: values, bounds, decisions
def _margin(a, b):
    """|a - b| in units of a's bound (inf where the bound is 0 and the two differ)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.abs(a.v - b)
        return np.where(a.e > 0, gap / (EPS32 * a.e), np.where(gap > 0, np.inf, 0.0))


CULL_NAMES = ("kept", "near", "far", "d0", "clip", "left", "right", "top", "bottom")


def project_fwd_budget(means, quats, scales, viewmat, K, W, H, near, far=FAR, radius_clip=0.0, tile_size=TILE, check=True):
    """float64 surfel_project of all N rows with bounds and decisions.  dict:
      M, means2d, depths, normal (unsigned: Rc[:, 2]) [+ _e: bounds in units of 2^-24], dot, dot_e (the sum whose sign flips the normal),
      valid, culled_by (index into CULL_NAMES: the FIRST failing test, in the kernel's order), radii, rect [N,4], tiles,
      margins {name: [N]} and `margin` [N]: the margin that decides the row's fate -- for a kept row the least of all, for a culled row
      that of the test that culls it (and of the radius where a test uses it) -- in units of the bound of the quantity compared."""
    O = _OB
    cam = _cam(O, viewmat, K)
    sc = np.asarray(scales, np.float32)
    fw = _fwd_chain(O, cam, _cols(O, means), _cols(O, quats), O.inp(sc[:, 0]), O.inp(sc[:, 1]))
    N = len(sc)
    z, d, mx, my, ext = fw["mc"][2], fw["d"], fw["mx"], fw["my"], fw["ext"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pre = fw["pre"].v
        radius_f = np.minimum(np.ceil(pre), SF_MAX_RADIUS)
        # the radius changes where ext crosses (m / 3)^2 for an integer m; below the 1e-4 floor it cannot (3 sqrt(1e-4) = 0.03).  The
        # square root and the product by 3 add 4 roundings of the threshold.
        hi_t = (radius_f / 3.0) ** 2
        lo_t = ((radius_f - 1.0) / 3.0) ** 2
        m_hi = (hi_t - ext.v) / (EPS32 * (ext.e + 4.0 * hi_t))
        m_lo = np.where(radius_f >= 2.0, (ext.v - lo_t) / (EPS32 * (ext.e + 4.0 * lo_t)), np.inf)
        m_radius = np.where(np.ceil(pre) < SF_MAX_RADIUS, np.minimum(m_hi, m_lo), 0.0)
        # A radius of thousands of pixels (a surfel whose plane nearly contains the camera: f = 1 / d with d a small difference) is a
        # rounded-up number whose float32 error exceeds 1: no evaluation decides it.  From RADIUS_BIG on, an undecided radius is not
        # redrawn; it is carried as a number with a bound (that of 3 sqrt(ext), plus 1 for the ceil) into the screen tests and the tile
        # rectangle, whose margins then say whether THEY are decided, and the test checks such a radius against that bound.
        radius_exact = m_radius >= 2 * MARGIN_KAPPA
        m_radius = np.where(~radius_exact & (radius_f >= RADIUS_BIG), np.inf, m_radius)
        rB = _B(radius_f, np.where(radius_exact, 0.0, fw["pre"].e + 2.0 ** 24))
        left, right, top, bottom = mx + rB, mx - rB, my + rB, my - rB
        fails = [z.v < near, z.v > far, d.v == 0.0, ~(radius_f > radius_clip), ~(left.v > 0.0), ~(right.v < W), ~(top.v > 0.0),
                 ~(bottom.v < H)]
        marg = dict(near=_margin(z, near), far=_margin(z, far), d0=_margin(d, 0.0), radius=m_radius, left=_margin(left, 0.0),
                    right=_margin(right, float(W)), top=_margin(top, 0.0), bottom=_margin(bottom, float(H)))
        culled_by = np.zeros(N, np.int64)
        for i in range(len(fails) - 1, -1, -1):
            culled_by = np.where(fails[i], i + 1, culled_by)
        valid = culled_by == 0
        # tile_range_exact
        ts = float(tile_size)
        tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
        tr = rB / ts
        tx, ty = mx / ts, my / ts
        edges = [tx - tr, ty - tr, tx + tr, ty + tr]
        grid = [tw, th, tw, th]
        rect, m_edge = [], np.full(N, np.inf)
        for k, (e, g) in enumerate(zip(edges, grid)):
            r = np.floor(e.v) if k < 2 else np.ceil(e.v)
            rect.append(np.clip(np.nan_to_num(r, nan=0.0, posinf=g, neginf=0.0), 0, g).astype(np.int64))
            near_int = np.round(e.v)
            on_grid = (near_int >= 0) & (near_int <= g)                   # beyond it the clamp decides, not the rounding
            m_edge = np.minimum(m_edge, np.where(on_grid, _margin(e, near_int), np.inf))
        marg["tile"] = m_edge
        rect = np.stack(rect, -1)
        tiles = np.where(valid, (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), -1)
        kept_margin = np.minimum.reduce([marg[k] for k in ("near", "far", "d0", "radius", "left", "right", "top", "bottom", "tile")])
        own = np.stack([kept_margin, marg["near"], marg["far"], marg["d0"], marg["radius"]]
                       + [np.minimum(marg[k], marg["radius"]) for k in ("left", "right", "top", "bottom")], 0)
        margin = own[culled_by, np.arange(N)]
        marg["sign"] = _margin(fw["dot"], 0.0)
    stack = lambda xs, f: np.stack([f(x) for x in xs], -1)
    out = dict(M=stack(fw["M"], lambda x: x.v), M_e=stack(fw["M"], lambda x: x.e), means2d=np.stack((mx.v, my.v), -1),
               means2d_e=np.stack((mx.e, my.e), -1), depths=z.v, depths_e=z.e, normal=stack([fw["Rc"][2], fw["Rc"][5], fw["Rc"][8]], lambda x: x.v),
               normal_e=stack([fw["Rc"][2], fw["Rc"][5], fw["Rc"][8]], lambda x: x.e), dot=fw["dot"].v, dot_e=fw["dot"].e, valid=valid,
               culled_by=culled_by, radii=radius_f.astype(np.int64), radius_exact=radius_exact, pre=fw["pre"].v, pre_e=fw["pre"].e, rect=rect, tiles=tiles, margins=marg, margin=margin, d=d.v,
               ext=np.stack((fw["ex"].v, fw["ey"].v), -1), M2sq=sum(fw["M"][6 + j].v ** 2 for j in range(3)))
    if check:
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
        with torch.no_grad():
            pr = surfel_ref.project(t(means), t(quats), t(scales), t(viewmat), t(K), W, H, near=near, far=far, radius_clip=radius_clip,
                                    tile_size=tile_size)
        v = valid
        assert np.array_equal(pr["valid"].numpy(), v), "restatement != surfel_ref.project (valid)"
        same = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12 * max(float(np.abs(b).max(initial=0.0)), 1e-300))
        front = (z.v >= near) & (z.v <= far)
        assert same(out["M"][front].reshape(-1, 9), pr["M"].numpy()[front].reshape(-1, 9)), "restatement != surfel_ref.project (M)"
        for i in np.nonzero(v)[0][:: max(1, int(v.sum()) // 4000)]:                            # row by row: each at its own scale
            assert same(out["M"][i], pr["M"].numpy()[i].reshape(9)) and same(out["means2d"][i], pr["means2d"].numpy()[i]), i
        assert same(out["depths"][v], pr["depths"].numpy()[v]), "depths"
        flip = np.where(out["dot"] > 0, -1.0, 1.0)[:, None]
        assert same((flip * out["normal"])[v], pr["normals"].numpy()[v]), "normals"
        assert np.array_equal(out["radii"][v & radius_exact], pr["radii"].numpy()[v & radius_exact]) and np.array_equal(rect[v], pr["rect"].numpy()[v]), "radii / rect"
    return out


def project_fwd_f32(means, quats, scales, viewmat, K):
    """the float32 restatement of the forward's values: dict(M [N,9], means2d [N,2], depths [N], normal [N,3] unsigned, dot [N])"""
    O = _OF
    sc = np.asarray(scales, np.float32)
    fw = _fwd_chain(O, _cam(O, viewmat, K), _cols(O, means), _cols(O, quats), O.inp(sc[:, 0]), O.inp(sc[:, 1]))
    st = lambda xs: np.stack([x.v for x in xs], -1)
    return dict(M=st(fw["M"]), means2d=st([fw["mx"], fw["my"]]), depths=fw["mc"][2].v, normal=st([fw["Rc"][2], fw["Rc"][5], fw["Rc"][8]]),
                dot=fw["dot"].v)


# ------------------------------------------------------------------------------------------------ SH forward
def sh_fwd_budget(deg, means, viewmat, K, coeffs, check=True):
    """SH colours of all rows (coeffs [N, >= (deg+1)^2, 3] float32): dict(rgb, rgb_e [N,3] (clamped channels: exactly 0, bound 0),
    c5 (= c + 0.5), clamped [N,3] bool, margin [N,3] of c + 0.5 against 0 in units of its bound, n_clamped [N])"""
    O = _OB
    nb = (deg + 1) ** 2
    cam = _cam(O, viewmat, K)
    c, c5, _, _ = _sh_color_chain(O, cam, deg, _cols(O, means), _sh_rows(O, coeffs, nb))
    v5, e5 = np.stack([a.v for a in c5], -1), np.stack([a.e for a in c5], -1)
    clamped = ~(v5 >= 0)
    out = dict(rgb=np.where(clamped, 0.0, v5), rgb_e=np.where(clamped, 0.0, e5), c5=v5, clamped=clamped,
               margin=np.stack([_margin(a, 0.0) for a in c5], -1), n_clamped=clamped.sum(-1),
               size=sum(np.abs(a.v) for a in c) / 3.0)
    if check:
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
        vm = t(viewmat)
        want = surfel_ref.sh_colors(deg, t(means), -(vm[:3, :3].T @ vm[:3, 3]), t(coeffs)).numpy()
        scale = np.abs(np.asarray(coeffs, np.float64)[:, :nb]).sum((1, 2))[:, None] + 0.5
        assert (np.abs(out["rgb"] - want) <= 1e-12 * scale).all(), "SH restatement != surfel_ref.sh_colors"
    return out


def sh_fwd_f32(deg, means, viewmat, K, coeffs):
    """float32 restatement: rgb [N,3] = fmaxf(c + 0.5, 0)"""
    O = _OF
    _, c5, _, _ = _sh_color_chain(O, _cam(O, viewmat, K), deg, _cols(O, means), _sh_rows(O, coeffs, (deg + 1) ** 2))
    return np.maximum(np.stack([a.v for a in c5], -1), np.float32(0.0))


# ------------------------------------------------------------------------------------------------ backward
GRAD_NAMES = ("g_means", "g_quats", "g_scales", "g_opacities", "g_colors")


def _bwd_any(O, means, quats, scales, viewmat, K, gids, sgn, cot, sh):
    """the backward of the visible rows `gids` over the number type of O.  cot: dict(v_ray_transforms [V,9], v_means2d [V,2],
    v_depths [V] or None, v_normals [V,3], v_opacities [V], v_colors [V,Dc]); sh: None or (degree, coeffs [N,K,3]).
    Returns lists of numbers: v_mean_proj [3], dir [3] or None, g_quats [4], gs0, gs1, g_sh [nb][3] or None."""
    gids = np.asarray(gids, np.int64)
    cam = _cam(O, viewmat, K)
    mean, quat = _cols(O, np.asarray(means, np.float32)[gids]), _cols(O, np.asarray(quats, np.float32)[gids])
    sc = np.asarray(scales, np.float32)[gids]
    vdepth = None if cot.get("v_depths") is None else O.inp(cot["v_depths"])
    v_mean, g_quats, gs0, gs1 = _bwd_chain(O, cam, mean, quat, O.inp(sc[:, 0]), O.inp(sc[:, 1]), sgn, _cols(O, cot["v_ray_transforms"]),
                                           _cols(O, cot["v_means2d"]), vdepth, _cols(O, cot["v_normals"]))
    g_sh = dirt = None
    if sh is not None:
        deg, coeffs = sh
        g_sh, dirt, _ = _sh_bwd_chain(O, cam, deg, mean, _sh_rows(O, np.asarray(coeffs, np.float32)[gids], (deg + 1) ** 2),
                                      _cols(O, cot["v_colors"]))
    return v_mean, dirt, g_quats, gs0, gs1, g_sh


def _scatter(N, gids, a):
    out = np.zeros((N,) + a.shape[1:], a.dtype)
    out[gids] = a
    return out


def project_bwd_budget(means, quats, scales, viewmat, K, gids, sgn, cot, sh=None, check=True):
    """float64 surfel_project_bwd_kernel with budgets, scattered to [N, ...] (invisible rows: value 0, budget 0).  dict name ->
    (value, budget): g_means (with SH: the projection term plus the SH direction term, the sum of both budgets and the rounding of
    the sum), g_means_proj, g_means_dir, g_quats, g_scales, g_opacities, g_colors (plain colours: copies) or g_sh [N, K, 3].
    The values are asserted equal to float64 autograd of tests/surfel_ref.py under the same cotangents with the same flip."""
    O = _OB
    N, gids = len(means), np.asarray(gids, np.int64)
    V = len(gids)
    v_mean, dirt, g_quats, gs0, gs1, g_sh = _bwd_any(O, means, quats, scales, viewmat, K, gids, sgn, cot, sh)
    full = lambda xs: [_B(np.broadcast_to(x.v, (V,)).copy(), np.broadcast_to(x.e, (V,)).copy()) for x in xs]
    pack = lambda xs: (_scatter(N, gids, np.stack([x.v for x in full(xs)], -1)), _scatter(N, gids, np.stack([x.e for x in full(xs)], -1)))
    out = dict(g_means_proj=pack(v_mean), g_quats=pack(g_quats))
    zero = _B(np.zeros(V))
    out["g_scales"] = pack([gs0, gs1, zero])
    out["g_means"] = pack([a + b for a, b in zip(v_mean, dirt)]) if dirt is not None else out["g_means_proj"]
    out["g_means_dir"] = pack(dirt) if dirt is not None else (np.zeros((N, 3)), np.zeros((N, 3)))
    vo = np.asarray(cot["v_opacities"], np.float32).astype(np.float64)
    out["g_opacities"] = (_scatter(N, gids, vo), np.zeros(N))
    if sh is None:
        vc = np.asarray(cot["v_colors"], np.float32).astype(np.float64)
        out["g_colors"] = (_scatter(N, gids, vc), np.zeros((N, vc.shape[1])))
    else:
        deg, coeffs = sh
        Kc, nb = np.asarray(coeffs).shape[1], (deg + 1) ** 2
        gv, ge = np.zeros((N, Kc, 3)), np.zeros((N, Kc, 3))
        for k in range(nb):
            v, e = pack(g_sh[k])
            gv[:, k], ge[:, k] = v, e
        out["g_sh"] = (gv, ge)
    if check:
        _check_autograd(out, means, quats, scales, viewmat, K, gids, sgn, cot, sh)
    return out


def _check_autograd(out, means, quats, scales, viewmat, K, gids, sgn, cot, sh):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
    lv = {k: t(v).requires_grad_(True) for k, v in dict(means=means, quats=quats, scales=scales).items()}
    vm, Kt = t(viewmat), t(K)
    ids = torch.from_numpy(np.asarray(gids, np.int64))
    pr = surfel_ref.project(lv["means"], lv["quats"], lv["scales"], vm, Kt, 10, 10)
    # the reference's normal is +-Rc[:, 2] by its own float64 flip: undo that and apply the sign handed in
    ref_sgn = torch.where(((vm[:3, :3] @ surfel_ref.quat_rotation(lv["quats"].detach()))[:, :, 2] * pr["normals"].detach()).sum(-1) < 0, -1.0, 1.0)
    normals = (torch.from_numpy(np.asarray(sgn, np.float64)) * ref_sgn[ids])[:, None] * pr["normals"][ids]
    loss = (pr["M"][ids].reshape(-1, 9) * t(cot["v_ray_transforms"])).sum() + (pr["means2d"][ids] * t(cot["v_means2d"])).sum() \
        + (normals * t(cot["v_normals"])).sum()
    if cot.get("v_depths") is not None:
        loss = loss + (pr["depths"][ids] * t(cot["v_depths"])).sum()
    if sh is not None:
        deg, coeffs = sh
        lv["sh"] = t(coeffs).requires_grad_(True)
        campos = -(vm[:3, :3].T @ vm[:3, 3])
        loss = loss + (surfel_ref.sh_colors(deg, lv["means"][ids], campos, lv["sh"][ids]) * t(cot["v_colors"])).sum()
    loss.backward()
    pairs = [("g_means", lv["means"].grad), ("g_quats", lv["quats"].grad), ("g_scales", lv["scales"].grad)]
    if sh is not None:
        pairs.append(("g_sh", lv["sh"].grad))
    for name, auto in pairs:
        auto = np.zeros(out[name][0].shape) if auto is None else auto.numpy()
        hand, bud = out[name]
        # both sides are float64 evaluations of chains whose float32 error the budget bounds: they may differ by 2^-29 of it
        ok = np.abs(hand - auto) <= 1e-6 * EPS32 * bud + 1e-13 * np.abs(auto)
        assert ok.all(), f"restatement != autograd ({name}): {np.argwhere(~ok)[0]}, {hand[~ok][0]} vs {auto[~ok][0]}"


def project_bwd_f32(means, quats, scales, viewmat, K, gids, sgn, cot, sh=None):
    """float32 restatement of the backward, scattered to [N, ...]: dict name -> array (names of project_bwd_budget)"""
    O = _OF
    N, gids = len(means), np.asarray(gids, np.int64)
    V = len(gids)
    v_mean, dirt, g_quats, gs0, gs1, g_sh = _bwd_any(O, means, quats, scales, viewmat, K, gids, sgn, cot, sh)
    pack = lambda xs: _scatter(N, gids, np.stack([np.broadcast_to(x.v, (V,)) for x in xs], -1))
    out = dict(g_means_proj=pack(v_mean), g_quats=pack(g_quats), g_scales=pack([gs0, gs1, _F(np.zeros(V))]))
    out["g_means"] = pack([a + b for a, b in zip(v_mean, dirt)]) if dirt is not None else out["g_means_proj"]
    out["g_opacities"] = _scatter(N, gids, np.asarray(cot["v_opacities"], np.float32))
    if sh is None:
        out["g_colors"] = _scatter(N, gids, np.asarray(cot["v_colors"], np.float32))
    else:
        deg, coeffs = sh
        Kc = np.asarray(coeffs).shape[1]
        g = np.zeros((N, Kc, 3), np.float32)
        for k in range((deg + 1) ** 2):
            g[:, k] = pack(g_sh[k])
        out["g_sh"] = g
    return out


# ------------------------------------------------------------------------------------------------ scenes
def camera(index):
    """the two cameras: roll, fx != fy, cx and cy well off centre, W and H no multiples of the tile size; the second with radius_clip 3.
    The first stands away from the world origin, so a camera-space centre is a difference of numbers of size 1 and carries an absolute
    error of about 3e-7, which d = |M2.xy|^2 - z^2 and the extents magnify by 1 / z: closer than 1/4 the radius of a surfel is not
    decided with a margin.  The second stands AT the origin
    (t = 0: the centre is a rotation of the mean, with a relative error), so its near plane is 2^-11 and its rows reach from 1e-3 to
    1e3 from the camera."""
    from tests.util import proj_camera
    if index == 0:
        return dict(proj_camera(0.35, -0.2, 0.3, (0.4, -0.3, -1.2), 203, 131, 170.0, 150.0, 72.0, 81.0), radius_clip=0.0, near=0.25, far=FAR)
    return dict(proj_camera(-0.6, 0.25, -0.45, (0.0, 0.0, 0.0), 147, 189, 205.0, 236.0, 96.0, 61.0), radius_clip=3.0, near=2.0 ** -11, far=FAR)


REGIMES = ("plain", "near", "far", "dsmall", "edge", "flip", "floor", "large", "off", "straddle", "qnorm", "ratio", "scales", "range", "behind")


def _frames_from_normal(r, n):
    """camera-space rotations [n,3,3] whose third column is the given unit normal, with a random spin about it"""
    k = len(n)
    a = r.randn(k, 3)
    t1 = np.cross(n, a); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(n, t1)
    return np.stack((t1, t2, n), -1)


def _regime_rows(r, name, n, cam):
    """n candidate surfels of one regime in CAMERA space: (centre [n,3], rotation [n,3,3], scales [n,2], quaternion scale [n])"""
    Km, W, H = cam["K"].astype(np.float64), cam["W"], cam["H"]
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    f = math.sqrt(fx * fy)
    z = r.uniform(2.0, 6.0, n)
    px, py = r.uniform(0.05 * W, 0.95 * W, n), r.uniform(0.05 * H, 0.95 * H, n)
    sig = r.uniform(1.5, 8.0, (n, 2))
    qs = np.ones(n)
    view_n = None                                       # |n . view|, drawn below
    facing = r.uniform(0.3, 1.0, n) * np.where(r.rand(n) < 0.5, -1.0, 1.0)
    lu = lambda a, b, *s: np.exp(r.uniform(math.log(a), math.log(b), *s))
    NEAR = cam["near"]
    if name == "near":
        z = NEAR * (1.0 + lu(1e-4, 0.5, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0))
    elif name == "far":
        z = FAR * (1.0 + lu(1e-4, 0.5, n) * np.where(np.arange(n) % 2 == 0, -1.0, 1.0))
    elif name == "edge":
        facing = r.uniform(-0.05, 0.05, n)
        facing[:12] = lu(1e-9, 1e-6, 12) * np.sign(facing[:12])          # n . c within a few bounds of 0: the stored sign decides
    elif name == "floor":
        sig = lu(1e-4, 3e-3, (n, 2))
        px, py = r.uniform(4.0, 45.0, n), r.uniform(4.0, 45.0, n)
    elif name == "large":
        sig = r.uniform(0.4, 2.0, (n, 1)) * max(W, H) * r.uniform(0.7, 1.4, (n, 2))
        facing = r.uniform(0.6, 1.0, n) * np.sign(facing)
    elif name in ("off", "straddle"):
        s = r.uniform(2.0, 10.0, n)
        sig = s[:, None] * r.uniform(0.9, 1.1, (n, 2))
        facing = r.uniform(0.8, 1.0, n) * np.sign(facing)
        dist = 3.0 * s * (r.uniform(1.4, 3.0, n) if name == "off" else r.uniform(0.2, 0.6, n))
        side = np.arange(n) % 4
        px = np.where(side == 0, -dist, np.where(side == 1, W + dist, px))
        py = np.where(side == 2, -dist, np.where(side == 3, H + dist, py))
    elif name == "qnorm":
        qs = lu(1e-3, 1e3, n); qs[0], qs[1] = 1e-3, 1e3
    elif name == "ratio":
        big = r.uniform(4.0, 30.0, n)
        ratio = lu(1e-3, 1.0, n); ratio[0] = 1e-3
        sig = np.where((np.arange(n) % 2 == 0)[:, None], np.stack((big, big * ratio), -1), np.stack((big * ratio, big), -1))
    elif name == "range":
        z = lu(2.0 * NEAR, 1e3, n); z[0], z[1] = 2.05 * NEAR, 0.98e3
    elif name == "behind":
        z = -lu(1e-3, 1e2, n)
    centre = np.stack(((px - cx) / fx * z, (py - cy) / fy * z, z), -1)
    view = centre / np.linalg.norm(centre, axis=1, keepdims=True)
    # normal = facing * view + sqrt(1 - facing^2) * (a unit vector across the view ray)
    a = np.cross(view, r.randn(n, 3)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    nrm = facing[:, None] * view + np.sqrt(1.0 - facing ** 2)[:, None] * a
    Rc = _frames_from_normal(r, nrm)
    scales = sig * np.abs(z)[:, None] / f
    if name == "scales":
        scales = lu(1e-4, 10.0, (n, 1)) * r.uniform(0.7, 1.4, (n, 2)); scales[0, 0], scales[1, 1] = 1e-4, 10.0
    elif name == "dsmall":
        # d = (s0 Rc20)^2 + (s1 Rc21)^2 - z^2 with |d| / |M2|^2 = rho: the plane of the surfel nearly contains the camera
        rho = lu(1e-3, 1e-1, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        A = z * z * (1.0 + rho) / (1.0 - rho)
        phi = r.uniform(0.3, 1.2, n)
        lo = 0.2                                                  # keep both in-plane axes well off the image plane
        ok = (np.abs(Rc[:, 2, 0]) > lo) & (np.abs(Rc[:, 2, 1]) > lo)
        Rc[~ok] = _frames_from_normal(r, nrm[~ok])
        with np.errstate(divide="ignore"):
            scales = np.stack((np.sqrt(A) * np.cos(phi) / np.abs(Rc[:, 2, 0]), np.sqrt(A) * np.sin(phi) / np.abs(Rc[:, 2, 1])), -1)
        scales = np.where(np.isfinite(scales), scales, 1.0)
    return centre, Rc, scales, qs


def _qmul(a, b):
    return np.stack((a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(-1),
                     a[:, 0] * b[:, 1] + b[:, 0] * a[:, 1] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] + b[:, 0] * a[:, 2] + a[:, 3] * b[:, 1] - a[:, 1] * b[:, 3],
                     a[:, 0] * b[:, 3] + b[:, 0] * a[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]), -1)


def _to_world(cam, centre, Rc, scales, qs):
    vm = cam["viewmat"].astype(np.float64)
    Rcw = vm[:3, :3]
    means = (centre - vm[:3, 3]) @ Rcw                                       # Rcw^T (c - t)
    Rw = np.einsum("ji,njk->nik", Rcw, Rc)
    q = rot2quat(torch.from_numpy(Rw)).numpy() * qs[:, None]
    sc3 = np.concatenate((scales, np.ones((len(scales), 1))), -1)
    return means.astype(np.float32), q.astype(np.float32), sc3.astype(np.float32)


def _regime_ok(name, i, fwd, sc3, cam):
    """row by row: does the reference see the candidate in its regime?  (i: index within the regime's draw)"""
    W, H = cam["W"], cam["H"]
    valid, by = fwd["valid"], fwd["culled_by"]
    cb = lambda nm: by == CULL_NAMES.index(nm)
    clip = cam["radius_clip"]
    if name == "near":
        return np.where(i % 2 == 0, valid, cb("near"))
    if name == "far":
        return np.where(i % 2 == 0, valid, cb("far"))
    if name == "floor":
        small = (fwd["radii"] == 1) & (fwd["ext"].max(-1) < 1e-4)
        return small & (cb("clip") if clip >= 1 else valid)
    if name == "large":
        return valid & (fwd["radii"] > max(W, H))
    if name == "off":
        return by == 5 + i % 4
    if name == "straddle":
        mx, my, rr = fwd["means2d"][:, 0], fwd["means2d"][:, 1], fwd["radii"]
        out = np.where(i % 4 == 0, mx < 0, np.where(i % 4 == 1, mx > W, np.where(i % 4 == 2, my < 0, my > H)))
        return valid & out
    if name == "behind":
        return cb("near")
    if name == "dsmall":
        rho = fwd["d"] / fwd["M2sq"]
        return valid & (np.abs(rho) < 0.12) & (np.sign(rho) == np.where(i % 2 == 0, 1.0, -1.0))
    return valid


@functools.lru_cache(maxsize=None)
def budget_scene(cam_index, n_per=100, seed=0):
    """One scene per camera.  dict(means, quats, scales, opacities (float32), regime [N] (index into REGIMES), slot [N] (index within the
    regime's draw: parity / side), cam, fwd (project_fwd_budget of the finished scene))."""
    cam = camera(cam_index)
    r = np.random.RandomState(4000 + 17 * cam_index + seed)
    rows = {k: [] for k in ("means", "quats", "scales", "regime", "slot")}
    for ri, name in enumerate(REGIMES):
        n = 64 if name == "behind" else 128 if name in ("off", "straddle") else n_per
        have = np.zeros(n, bool)
        keep = [None] * n
        for attempt in range(60):
            centre, Rc, sc, qs = _regime_rows(r, name, n, cam)
            m, q, s3 = _to_world(cam, centre, Rc, sc, qs)
            fwd = project_fwd_budget(m, q, s3, cam["viewmat"], cam["K"], cam["W"], cam["H"], cam["near"], cam["far"], cam["radius_clip"], check=False)
            ok = _regime_ok(name, np.arange(n), fwd, s3, cam) & (fwd["margin"] >= 2 * MARGIN_KAPPA) & np.isfinite(fwd["M"]).all(-1)
            for i in np.nonzero(ok & ~have)[0]:
                keep[i] = (m[i], q[i], s3[i]); have[i] = True
            if have.all():
                break
        assert have.all(), (cam_index, name, int(have.sum()))
        for i in range(n):
            rows["means"].append(keep[i][0]); rows["quats"].append(keep[i][1]); rows["scales"].append(keep[i][2])
            rows["regime"].append(ri); rows["slot"].append(i)
    order = r.permutation(len(rows["regime"]))
    sc = {k: np.asarray(v)[order] for k, v in rows.items()}
    sc["means"], sc["quats"], sc["scales"] = (np.ascontiguousarray(sc[k], np.float32) for k in ("means", "quats", "scales"))
    sc["opacities"] = r.uniform(0.05, 1.0, len(order)).astype(np.float32)
    sc["cam"] = cam
    sc["fwd"] = project_fwd_budget(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], cam["W"], cam["H"],
                                   cam["near"], cam["far"], cam["radius_clip"])
    assert (sc["fwd"]["margin"] >= 2 * MARGIN_KAPPA).all()
    assert len(order) <= 3000
    return sc


def regime_counts(sc):
    """how many rows of the finished scene the reference sees in each regime (and sub-case)"""
    fwd, cam = sc["fwd"], sc["cam"]
    reg = lambda nm: sc["regime"] == REGIMES.index(nm)
    ok = {nm: _regime_ok(nm, sc["slot"], fwd, sc["scales"], cam) & reg(nm) for nm in REGIMES}
    slot, valid = sc["slot"], fwd["valid"]
    mc = sc["means"].astype(np.float64) @ cam["viewmat"][:3, :3].astype(np.float64).T + cam["viewmat"][:3, 3].astype(np.float64)
    cosv = np.abs(fwd["dot"]) / np.linalg.norm(mc, axis=1)
    out = dict(plain=ok["plain"].sum(), near_kept=(ok["near"] & valid).sum(), near_culled=(ok["near"] & ~valid).sum(),
               far_kept=(ok["far"] & valid).sum(), far_culled=(ok["far"] & ~valid).sum(),
               dsmall_pos=(ok["dsmall"] & (fwd["d"] > 0)).sum(), dsmall_neg=(ok["dsmall"] & (fwd["d"] < 0)).sum(),
               dsmall_1e3=(ok["dsmall"] & (np.abs(fwd["d"] / fwd["M2sq"]) < 3e-3)).sum() * 4,
               edge=(ok["edge"] & (cosv < 0.05)).sum(), flipped=(ok["flip"] & (fwd["dot"] > 0)).sum(),
               unflipped=(ok["flip"] & (fwd["dot"] <= 0)).sum(), floor=ok["floor"].sum(), large=ok["large"].sum(),
               qnorm=ok["qnorm"].sum(), ratio=ok["ratio"].sum(), scales=ok["scales"].sum(), range=ok["range"].sum(), behind=ok["behind"].sum())
    for s, side in enumerate(("left", "right", "top", "bottom")):
        out["off_" + side] = (ok["off"] & (slot % 4 == s)).sum()
        out["straddle_" + side] = (ok["straddle"] & (slot % 4 == s)).sum()
    qn = np.linalg.norm(sc["quats"][reg("qnorm")].astype(np.float64), axis=1)
    rt = sc["scales"][reg("ratio"), 0].astype(np.float64) / sc["scales"][reg("ratio"), 1]
    ss = sc["scales"][reg("scales"), :2]
    dist = np.linalg.norm(mc[valid], axis=1)
    spans = dict(qnorm=(qn.min() < 2e-3 and qn.max() > 5e2), ratio=(rt.min() < 3e-3 and rt.max() > 3e2), scales=(ss.min() < 3e-4 and ss.max() > 3.0),
                 range=(dist.min() < 4.0 * cam["near"] and dist.max() > 3e2), interleaved=int((~valid[:-1] & valid[1:]).sum()) > 50)
    return {k: int(v) for k, v in out.items()}, spans


def assert_regimes(sc):
    counts, spans = regime_counts(sc)
    low = {k: v for k, v in counts.items() if v < 20}
    assert not low, ("regimes with fewer than 20 rows", low)
    assert all(spans.values()), spans
    return counts


# ----- SH inputs
@functools.lru_cache(maxsize=None)
def sh_inputs(cam_index, deg, seed=0, scene="surfel"):
    """coefficients [N,16,3] float32 for the rows of a scene, tuned on the float64 evaluation at degree `deg`: rows of magnitude
    1e-3 .. 10; every third row has one, two or three channels clamped with a clear margin; every third is unclamped with c + 0.5 small;
    the rest is as drawn.  Every row ends with a margin of at least 2 * MARGIN_KAPPA bounds on all three channels.  (The entries
    k >= (deg+1)^2 are random and must never be read.)  Returns (coeffs, sh_fwd_budget of them)."""
    if scene == "surfel":
        sc = budget_scene(cam_index)
        means, vm, K = sc["means"], sc["cam"]["viewmat"], sc["cam"]["K"]
    else:
        s3 = _yaw_scene()
        means, vm, K = s3["means"], s3["views"][0]["viewmat"], s3["views"][0]["K"]
    N = len(means)
    r = np.random.RandomState(9000 + 31 * cam_index + 7 * deg + seed)
    mag = np.exp(r.uniform(math.log(1e-3), math.log(10.0), N))
    co = (mag[:, None, None] * r.randn(N, 16, 3)).astype(np.float32)
    kind = np.arange(N) % 3
    b0 = 0.2820947917738781
    target = np.zeros((N, 3))
    tuned = np.zeros((N, 3), bool)
    n_cl = 1 + (np.arange(N) // 3) % 3
    for ch in range(3):
        tuned[:, ch] = (kind == 1) | ((kind == 0) & (ch < n_cl))
    grow = np.ones((N, 3))
    for attempt in range(8):
        fw = sh_fwd_budget(deg, means, vm, K, co, check=False)
        size = 3.0 * fw["size"][:, None] + 0.5
        if attempt == 0:
            u = r.uniform(size=(N, 3))
            base = np.where((kind == 0)[:, None], -(0.05 + 0.95 * u), 10.0 ** (-3.0 + u))
        bad = fw["margin"] < 2 * MARGIN_KAPPA
        if attempt > 0 and not bad.any():
            break
        grow = np.where(bad & (attempt > 0), grow * 4.0, grow)
        target = base * grow * size
        fix = tuned & (bad | (attempt == 0))
        rest = fw["c5"] - b0 * co[:, 0, :].astype(np.float64)
        co[:, 0, :] = np.where(fix, ((target - rest) / b0), co[:, 0, :]).astype(np.float32)
        # an untuned row inside the band: move it out the same way
        fix2 = ~tuned & bad
        co[:, 0, :] = np.where(fix2, ((np.sign(fw["c5"]) * np.abs(base) * grow * size - rest) / b0), co[:, 0, :]).astype(np.float32)
    fw = sh_fwd_budget(deg, means, vm, K, co)
    assert (fw["margin"] >= 2 * MARGIN_KAPPA).all(), (deg, int((fw["margin"] < 2 * MARGIN_KAPPA).sum()))
    return co, fw


@functools.lru_cache(maxsize=None)
def _yaw_scene():
    from tests import util
    return util.PROJ_BUDGET_SCENES["yaw"]()


def assert_clamp_patterns(fw, visible):
    """0, 1, 2 and 3 clamped channels: at least 20 visible rows each; and some unclamped c + 0.5 are small"""
    n = np.bincount(fw["n_clamped"][visible], minlength=4)
    assert (n >= 20).all(), n
    small = (~fw["clamped"][visible]) & (fw["c5"][visible] < 0.02 * (1.0 + fw["size"][visible][:, None] * 3.0))
    assert small.sum() >= 20, int(small.sum())
    return n


# ----- cotangents
COTANGENTS = ("dense", "decades", "rows0", "only_v_ray_transforms", "only_v_means2d", "only_v_depths", "only_v_normals", "only_v_opacities",
              "only_v_colors")
COT_COLUMNS = (("v_ray_transforms", 9), ("v_means2d", 2), ("v_depths", 1), ("v_normals", 3), ("v_opacities", 1), ("v_colors", None))


def cotangents(kind, V, Dc, seed, with_depth=True):
    """the six incoming gradients of the backward as float32 arrays; v_depths None without a depth channel"""
    r = np.random.RandomState(7000 + seed)
    out = {}
    for name, w in COT_COLUMNS:
        w = Dc if w is None else w
        a = r.uniform(-1, 1, (V, w))
        if kind == "decades":
            a = np.sign(a) * 10.0 ** r.uniform(-3, 3, (V, w))
        if kind.startswith("only_") and kind != "only_" + name:
            a[:] = 0.0
        if kind == "rows0":
            a[3::7] = 0.0
        out[name] = a.astype(np.float32)
    assert kind in COTANGENTS, kind
    out["v_depths"] = out["v_depths"][:, 0] if with_depth else None
    out["v_opacities"] = out["v_opacities"][:, 0]
    return out
