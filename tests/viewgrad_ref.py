"""TEST INFRASTRUCTURE (CPU only): the gradient of the view matrix as gs_project_bwd_view forms it (csrc/gs_project.hip:
project_bwd_view_kernel, on project_bwd_one of csrc/gs_project_dev.h and sh_color_bwd_row of csrc/gs_sh_dev.h), restated operation for
operation ONCE over the small operation tables of tests/surfel_project_ref.py and evaluated with two number types:

  * `_B` of oracle/mesh_ref.py -- float64 values with a first-order running-error bound in units of 2^-24 that charges one rounding
    per operation; v_rcp_f32 / v_rsq_f32 (and `1.0f / sqrtf`) are charged three.  Contraction only removes roundings.
  * numpy float32 (`_F`), which tests/test_viewgrad_cpu.py measures against the bound.

The chain takes the STORED conics and compensations as inputs (the same-stored-state principle of tests/test_gpu_project_budget.py),
the visible set as given, and decides the tan-fov clamp routes from its own values (the scenes of tests/util.py keep every decision
1e-3 away from its threshold).  Literals the kernel holds in float32 (0.3f, 1e-6f) enter as those floats.

  view_contributions   per visible Gaussian the twelve numbers c_n[12], row-major [3][4] = (c_R | c_t), and their bounds b_n[12]:
                           c_t = v_mc,   c_R = v_mc m^T + (v_Cc + v_Cc^T) (R cov)
                           SH degree >= 1 (v_dir = the direction term sh_color_bwd_row adds to v_mean):
                           c_t += R v_dir,   c_R[i][j] += t[i] v_dir[j]
  view_reference       (want [16], budget [16]) of v_viewmat: want = sum_n c_n (float64), budget B = sum_n b_n + |sum_n c_n| in units
                       of 2^-24 -- the second term is the ONE final rounding to fp32.  Only a wide (fp64) accumulation can meet it: an
                       fp32 running sum over N terms errs by up to N roundings of the partial sums.  The last row has want 0, budget 0;
                       a zero budget means exactly zero (all culled, zero cotangents).
  view_f32             the same sum from the all-float32 contributions, accumulated in float64 and rounded once.
  autograd_contributions
                       the arbiter: torch float64 autograd of the restated forward -- means2d, conic, opacity * comp (classic:
                       opacity), depth, plus surfel_ref.sh_colors with campos = -R^T t -- under the same cotangents, with EVERY
                       Gaussian given its own copy of the view matrix as a leaf, so one backward yields all c_n.  The forward is the
                       function the kernel differentiates (the twelve entries R, t as the forward reads them, not inverse(viewmat)).
                       sqrt in the compensation carries gsplat's own vjp, 0.5 / (comp + 1e-6), which is what project_bwd_one computes.
                       It also returns its float64 conics / compensations: check_against_autograd runs the `_B` chain on THOSE and
                       asserts |c_B - c_autograd| <= AUTOGRAD_BAR * 2^-24 * b_n for every element (b_n = 0: both exactly 0).

VIEWGRAD_KAPPA follows the project's rule for a rigorous bound, with one restriction: it is the smallest power of two that is at least
4 x (a), where (a) is the worst ratio of view_f32 against (want, budget) on the CPU over every scene, view, mode, SH degree and
cotangent kind of tests/test_viewgrad_cpu.py (the CPU bar is kappa / 2).  (b), the worst ratio of the kernel on an MI355X, is recorded
beside it and NOT used to set kappa: if (b) exceeds kappa the kernel is wrong or the bound misses an operation.
    (a) = 0.343  ('yaw' cut to its first visible Gaussian, antialiased; one term has no statistical slack against its bound.
                  The other prefix sizes: 0.15 at 65 Gaussians, 0.08 at 256, 0.03 at 769; the whole scenes 0.011 .. 0.035)
                  -> 4 x (a) = 1.37 -> kappa = 2, CPU bar 1
    (b) = the table in the docstring of tests/test_gpu_viewgrad.py
"""
import functools

import numpy as np
import torch

from oracle import torch_ref as tr
from tests import surfel_ref
from tests import util
from tests.surfel_project_ref import _OB, _OF, _cam, _cols, _sh_bwd_chain, _sh_rows

EPS32 = 2.0 ** -24
VIEWGRAD_KAPPA = 2.0
# float64 roundings are 2^-29 of float32's; the autograd route goes through the explicit inverse of the 2 x 2 covariance, whose
# cancellation (aniso regime: b^2 > 0.99 a c, scale ratios of 1e-4) may cost it up to ~2^23 of that advantage.  2^-6 of the fp32 bound
# is still three to five orders below what a wrong formula shows (see the bite table of tests/test_gpu_viewgrad.py).
AUTOGRAD_BAR = 2.0 ** -6
LIT_03 = np.float32(0.3)
LIT_1EM6 = np.float32(1e-6)
EPS2D = np.float32(0.3)


# ------------------------------------------------------------------------------------------------ the chain, written once
def _clamp_route(O, r, lim_pos, lim_neg):
    """fminf(lim_pos, fmaxf(-lim_neg, r)) and whether r passed unclamped (the kernel's own test: r <= lim_pos && r >= -lim_neg)"""
    rv, lp, ln = O.val(r), O.val(lim_pos), O.val(lim_neg)
    inside = (rv <= lp) & (rv >= -ln)
    return O.where(rv > lp, lim_pos, O.where(rv < -ln, -lim_neg, r)), inside


def _view_chain(O, cam, W, H, mean, quat, scale, opacity, conic, comp, vm2, vcon, vop, vdepth, classic, sh=None):
    """project_bwd_one up to (v_mc, v_Cc, T1), then the view terms of project_bwd_view_kernel: the list c[12]"""
    R, t = cam["R"], cam["t"]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    Wf, Hf, eps2d = O.inp(np.float32(W)), O.inp(np.float32(H)), O.inp(EPS2D)
    ia, ib, ic = conic
    if classic:                                                  # project_bwd_one with comp = 1 and opacity = 0
        zero = O.inp(np.zeros_like(O.val(vop), dtype=np.float32))
        opacity, comp = zero, zero + 1.0
    v_comp = vop * opacity
    mc = [R[3 * i] * mean[0] + R[3 * i + 1] * mean[1] + R[3 * i + 2] * mean[2] + t[i] for i in range(3)]
    qw, qx, qy, qz = quat
    inv = O.rsqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    x, y, z, w = qx * inv, qy * inv, qz * inv, qw * inv
    x2, y2, z2, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    Rq = [1.0 - 2.0 * (y2 + z2), 2.0 * (xy - wz), 2.0 * (xz + wy),
          2.0 * (xy + wz), 1.0 - 2.0 * (x2 + z2), 2.0 * (yz - wx),
          2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (x2 + y2)]
    M = [Rq[3 * i + j] * scale[j] for i in range(3) for j in range(3)]
    cov = [M[3 * i] * M[3 * j] + M[3 * i + 1] * M[3 * j + 1] + M[3 * i + 2] * M[3 * j + 2] for i in range(3) for j in range(3)]
    T1 = [R[3 * i] * cov[j] + R[3 * i + 1] * cov[3 + j] + R[3 * i + 2] * cov[6 + j] for i in range(3) for j in range(3)]
    Cc = [T1[3 * i] * R[3 * j] + T1[3 * i + 1] * R[3 * j + 1] + T1[3 * i + 2] * R[3 * j + 2] for i in range(3) for j in range(3)]
    # conic = inverse(cov2d_blur)
    ga, gb, gc = vcon[0], 0.5 * vcon[1], vcon[2]
    p00, p01 = ia * ga + ib * gb, ia * gb + ib * gc
    p10, p11 = ib * ga + ic * gb, ib * gb + ic * gc
    G = [-(p00 * ia + p01 * ib), -(p00 * ib + p01 * ic), -(p10 * ia + p11 * ib), -(p10 * ib + p11 * ic)]
    det_conic = ia * ic - ib * ib
    v_sqr_comp = v_comp * 0.5 * O.rcp(comp + O.inp(LIT_1EM6))
    om = 1.0 - comp * comp
    G[0] = G[0] + v_sqr_comp * (om * ia - eps2d * det_conic)
    G[1] = G[1] + v_sqr_comp * (om * ib)
    G[2] = G[2] + v_sqr_comp * (om * ib)
    G[3] = G[3] + v_sqr_comp * (om * ic - eps2d * det_conic)
    # perspective projection
    X, Y, Z = mc
    rfx, rfy = O.rcp(fx), O.rcp(fy)
    lit03 = O.inp(LIT_03)
    tan_fovx, tan_fovy = 0.5 * Wf * rfx, 0.5 * Hf * rfy
    lim_x_pos, lim_x_neg = (Wf - cx) * rfx + lit03 * tan_fovx, cx * rfx + lit03 * tan_fovx
    lim_y_pos, lim_y_neg = (Hf - cy) * rfy + lit03 * tan_fovy, cy * rfy + lit03 * tan_fovy
    rz = O.rcp(Z)
    rz2 = rz * rz
    rz3 = rz2 * rz
    cxr, in_x = _clamp_route(O, X * rz, lim_x_pos, lim_x_neg)
    cyr, in_y = _clamp_route(O, Y * rz, lim_y_pos, lim_y_neg)
    tx, ty = Z * cxr, Z * cyr
    J = [fx * rz, 0.0, -fx * tx * rz2, 0.0, fy * rz, -fy * ty * rz2]
    GJ = [G[2 * i] * J[j] + G[2 * i + 1] * J[3 + j] for i in range(2) for j in range(3)]
    v_Cc = [J[i] * GJ[j] + J[3 + i] * GJ[3 + j] for i in range(3) for j in range(3)]
    JC = [J[3 * i] * Cc[j] + J[3 * i + 1] * Cc[3 + j] + J[3 * i + 2] * Cc[6 + j] for i in range(2) for j in range(3)]
    JCt = [J[3 * i] * Cc[3 * j] + J[3 * i + 1] * Cc[3 * j + 1] + J[3 * i + 2] * Cc[3 * j + 2] for i in range(2) for j in range(3)]
    v_J = [(G[2 * i] * JCt[j] + G[2 * i + 1] * JCt[3 + j]) + (G[i] * JC[j] + G[2 + i] * JC[3 + j]) for i in range(2) for j in range(3)]
    v_mc = [fx * rz * vm2[0], fy * rz * vm2[1], -(fx * X * vm2[0] + fy * Y * vm2[1]) * rz2]
    v_mc[0] = O.where(in_x, v_mc[0] + (-fx * rz2 * v_J[2]), v_mc[0])
    v_mc[2] = O.where(in_x, v_mc[2], v_mc[2] + (-fx * rz3 * v_J[2] * tx))
    v_mc[1] = O.where(in_y, v_mc[1] + (-fy * rz2 * v_J[5]), v_mc[1])
    v_mc[2] = O.where(in_y, v_mc[2], v_mc[2] + (-fy * rz3 * v_J[5] * ty))
    v_mc[2] = v_mc[2] + (-fx * rz2 * v_J[0] - fy * rz2 * v_J[4] + 2.0 * fx * tx * rz3 * v_J[2] + 2.0 * fy * ty * rz3 * v_J[5])
    if vdepth is not None:
        v_mc[2] = v_mc[2] + vdepth
    # the view terms
    c = [None] * 12
    for i in range(3):
        s = [v_Cc[3 * i + k] + v_Cc[3 * k + i] for k in range(3)]
        for j in range(3):
            c[4 * i + j] = v_mc[i] * mean[j] + (s[0] * T1[j] + s[1] * T1[3 + j] + s[2] * T1[6 + j])
        c[4 * i + 3] = v_mc[i]
    if sh is not None:
        deg, co, v_rgb = sh
        _, vd, _ = _sh_bwd_chain(O, cam, deg, mean, co, v_rgb)
        if vd is not None:
            for i in range(3):
                for j in range(3):
                    c[4 * i + j] = c[4 * i + j] + t[i] * vd[j]
                c[4 * i + 3] = c[4 * i + 3] + (R[3 * i] * vd[0] + R[3 * i + 1] * vd[1] + R[3 * i + 2] * vd[2])
    return c


def _inputs(O, sc, vw, gids, conics, comps, cot, sh, exact_state=False):
    vm2, vc, vo, vd = cot
    g = np.asarray(gids)
    st = O.inp
    if exact_state:                                              # float64 conics / compensations of the autograd forward: `_B` only
        from oracle.mesh_ref import _B
        st = lambda a: _B(np.asarray(a, np.float64))
    args = dict(mean=_cols(O, sc["means"][g]), quat=_cols(O, sc["quats"][g]), scale=_cols(O, sc["scales"][g]),
                opacity=O.inp(sc["opacities"][g]), conic=[st(np.asarray(conics)[:, k]) for k in range(3)], comp=st(comps),
                vm2=_cols(O, vm2), vcon=_cols(O, vc), vop=O.inp(vo), vdepth=None if vd is None else O.inp(vd))
    if sh is not None:
        deg, coeffs, v_rgb = sh
        args["sh"] = (deg, _sh_rows(O, np.asarray(coeffs)[g], (deg + 1) ** 2), _cols(O, v_rgb))
    return args


def view_contributions(sc, vw, gids, conics, comps, cot, classic=False, sh=None, exact_state=False):
    """(c [V,12] float64, b [V,12] in units of 2^-24).  sh = (degree, coeffs [N,K,3], v_rgb [V,3]) or None."""
    O = _OB
    V = len(gids)
    if V == 0:
        return np.zeros((0, 12)), np.zeros((0, 12))
    c = _view_chain(O, _cam(O, vw["viewmat"], vw["K"]), vw["W"], vw["H"], classic=classic,
                    **_inputs(O, sc, vw, gids, conics, comps, cot, sh, exact_state))
    val = np.stack([np.broadcast_to(a.v, (V,)) for a in c], 1)
    err = np.stack([np.broadcast_to(a.e, (V,)) for a in c], 1)
    return val, err


def contributions_f32(sc, vw, gids, conics, comps, cot, classic=False, sh=None):
    O = _OF
    V = len(gids)
    if V == 0:
        return np.zeros((0, 12), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        c = _view_chain(O, _cam(O, vw["viewmat"], vw["K"]), vw["W"], vw["H"], classic=classic,
                        **_inputs(O, sc, vw, gids, conics, comps, cot, sh))
    return np.stack([np.broadcast_to(a.v, (V,)) for a in c], 1).astype(np.float32)


def _as16(v12):
    out = np.zeros(16, v12.dtype)
    out[:12] = v12
    return out


def view_reference(sc, vw, gids, conics, comps, cot, classic=False, sh=None):
    """(want [16] float64, budget [16] in units of 2^-24, (c, b)) of v_viewmat, row-major 4 x 4"""
    c, b = view_contributions(sc, vw, gids, conics, comps, cot, classic, sh)
    want = c.sum(0)
    return _as16(want), _as16(b.sum(0) + np.abs(want)), (c, b)


def view_f32(sc, vw, gids, conics, comps, cot, classic=False, sh=None):
    c = contributions_f32(sc, vw, gids, conics, comps, cot, classic, sh)
    return _as16(c.astype(np.float64).sum(0).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the arbiter
class _SqrtGsplat(torch.autograd.Function):
    """sqrt with gsplat's vjp of the compensation: v_x = v_s * 0.5 / (s + 1e-6f)"""
    @staticmethod
    def forward(ctx, x):
        s = torch.sqrt(x)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return g * 0.5 / (s + float(LIT_1EM6))


def autograd_contributions(sc, vw, gids, cot, classic=False, sh=None):
    """(c [V,12], conics [V,3], comps [V]) in float64: one view-matrix leaf per Gaussian, one backward"""
    dt = torch.float64
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dt)
    g = np.asarray(gids)
    V = len(g)
    vm2, vc, vo, vd = cot
    means, quats, scales, opac = T(sc["means"][g]), T(sc["quats"][g]), T(sc["scales"][g]), T(sc["opacities"][g])
    K = vw["K"].astype(np.float64)
    fx, fy, cx, cy, W, H = K[0, 0], K[1, 1], K[0, 2], K[1, 2], float(vw["W"]), float(vw["H"])
    vm = T(vw["viewmat"][:3]).expand(V, 3, 4).clone().requires_grad_(True)
    R, t = vm[:, :, :3], vm[:, :, 3]
    mc = (R @ means[:, :, None])[..., 0] + t
    Rq = tr.quat_to_rotmat(quats)
    M = Rq * scales[:, None, :]
    covc = R @ (M @ M.transpose(-1, -2)) @ R.transpose(-1, -2)
    x, y, z = mc.unbind(-1)
    l3 = float(LIT_03)
    lim = lambda a, f, n: torch.full_like(z, a / f + l3 * 0.5 * n / f)
    rz = 1.0 / z
    rz2 = rz * rz
    tx = z * torch.minimum(lim(W - cx, fx, W), torch.maximum(-lim(cx, fx, W), x * rz))
    ty = z * torch.minimum(lim(H - cy, fy, H), torch.maximum(-lim(cy, fy, H), y * rz))
    zero = torch.zeros_like(z)
    J = torch.stack([fx * rz, zero, -fx * tx * rz2, zero, fy * rz, -fy * ty * rz2], -1).reshape(-1, 2, 3)
    cov2d = J @ covc @ J.transpose(-1, -2)
    eps2d = float(EPS2D)
    det_orig = cov2d[:, 0, 0] * cov2d[:, 1, 1] - cov2d[:, 0, 1] * cov2d[:, 1, 0]
    c00, c11, c01, c10 = cov2d[:, 0, 0] + eps2d, cov2d[:, 1, 1] + eps2d, cov2d[:, 0, 1], cov2d[:, 1, 0]
    det = c00 * c11 - c01 * c10
    comp = _SqrtGsplat.apply(torch.clamp(det_orig / det, min=0.0))
    conics = torch.stack([c11 / det, -c01 / det, c00 / det], -1)
    means2d = torch.stack([fx * x * rz + cx, fy * y * rz + cy], -1)
    loss = (means2d * T(vm2)).sum() + (conics * T(vc)).sum() + ((opac if classic else opac * comp) * T(vo)).sum()
    if vd is not None:
        loss = loss + (z * T(vd)).sum()
    if sh is not None:
        deg, coeffs, v_rgb = sh
        campos = -(R.transpose(-1, -2) @ t[:, :, None])[..., 0]
        loss = loss + (surfel_ref.sh_colors(deg, means, campos, T(np.asarray(coeffs)[g])) * T(v_rgb)).sum()
    loss.backward()
    return vm.grad.reshape(V, 12).numpy(), conics.detach().numpy(), comp.detach().numpy()


def check_against_autograd(sc, vw, gids, cot, classic=False, sh=None):
    """asserts the `_B` chain, run on the autograd forward's own float64 conics / compensations, equal to float64 autograd; returns
    the worst |c_B - c_autograd| / (2^-24 b)"""
    want, conics, comps = autograd_contributions(sc, vw, gids, cot, classic, sh)
    c, b = view_contributions(sc, vw, gids, conics, comps, cot, classic, sh, exact_state=True)
    assert np.isfinite(c).all() and np.isfinite(b).all() and np.isfinite(want).all()
    dead = b == 0
    assert not c[dead].any() and not want[dead].any()
    ratio = np.abs(c - want)[~dead] / (EPS32 * b[~dead])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= AUTOGRAD_BAR, f"view terms differ from float64 autograd: worst ratio {worst:.3g} of the fp32 bound"
    return worst


# ------------------------------------------------------------------------------------------------ scenes, cotangents, SH inputs
VIEWS = (("yaw", 0), ("tilt_clip", 0), ("orbit8", 0), ("orbit8", 5))
MODES = (False, True)                       # classic
SH_DEGREES = (None, 0, 3)


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = util.PROJ_BUDGET_SCENES[name]()
    return sc, [util.proj_scene_forward(sc, vi) for vi in range(len(sc["views"]))]


VIEW_BLOCK = 256                            # GS_VIEW_BLOCK of csrc/gs_project.hip: Gaussians per workgroup, one partial row each
PREFIX_SIZES = (1, 63, 64, 65, VIEW_BLOCK - 1, VIEW_BLOCK, VIEW_BLOCK + 1, 3 * VIEW_BLOCK + 1)


def prefix(name, vi, n):
    """the first n Gaussians of a scene as a scene of their own: (scene, gaussian_ids, conics, compensations) of view vi"""
    sc, fwd = scene(name)
    m = fwd[vi]
    keep = m["gaussian_ids"] < n
    sub = dict(sc, means=sc["means"][:n], quats=sc["quats"][:n], scales=sc["scales"][:n], opacities=sc["opacities"][:n])
    return sub, m["gaussian_ids"][keep], m["conics"][keep], m["compensations"][keep]


def one_visible_size(name="yaw", vi=0):
    """the smallest prefix of a scene with exactly one visible Gaussian"""
    return int(scene(name)[1][vi]["gaussian_ids"][0]) + 1


def sh_inputs(sc, vi, deg, K=None, seed=0):
    """SH coefficients [N, K, 3] of a scene for one view: random in [-0.5, 0.5], with the DC term of every Gaussian whose colour is
    within 1e-3 of the clamp at 0 (any channel, float64) pushed away, so that float32 and float64 take the same clamp decisions"""
    N = sc["means"].shape[0]
    K = (deg + 1) ** 2 if K is None else K
    r = np.random.RandomState(500 + 31 * seed + 7 * deg + vi)
    co = r.uniform(-0.5, 0.5, (N, K, 3)).astype(np.float32)
    vm = sc["views"][vi]["viewmat"].astype(np.float64)
    campos = -vm[:3, :3].T @ vm[:3, 3]
    for _ in range(8):
        c5 = surfel_ref.sh_colors(deg, torch.tensor(sc["means"].astype(np.float64)), torch.tensor(campos), torch.tensor(co.astype(np.float64)))
        raw = (surfel_ref.sh_basis(deg, torch.nn.functional.normalize(torch.tensor(sc["means"].astype(np.float64)) - torch.tensor(campos), dim=-1))[..., None]
               * torch.tensor(co.astype(np.float64))[:, :(deg + 1) ** 2]).sum(-2).numpy() + 0.5
        near = np.abs(raw) < 1e-3
        if not near.any():
            break
        co[:, 0, :] = np.where(near, co[:, 0, :] + np.float32(0.05), co[:, 0, :])
    assert not near.any()
    return co


def cotangents(kind, V, seed, with_rgb):
    """util.proj_budget_cotangents plus colour cotangents [V,3] (None without SH) with the same all-zero rows"""
    cot = util.proj_budget_cotangents(kind, V, seed)
    rgb = None
    if with_rgb:
        rgb = np.random.RandomState(seed + 99).uniform(-1, 1, (V, 3)).astype(np.float32)
        if kind == "opacity":
            rgb[:] = 0.0
        rgb[3::7] = 0.0
    return cot, rgb


# ------------------------------------------------------------------------------------------------ the pose-recovery case
# tests/test_gpu_viewgrad.py::test_pose_recovery and scripts/poseopt_reference.py (the same loop on the CPU oracle, with the view
# gradient from view_reference in float64) share the scene, the perturbation, the two error measures and the optimiser settings.
# POSE_LR / POSE_STEPS were chosen with that script: see its docstring for the sweep.
POSE_N, POSE_W, POSE_H, POSE_SH = 3000, 97, 61, 1
POSE_DISTANCE = 3.0
POSE_TURN_DEG, POSE_SHIFT = 1.5, 0.03 * POSE_DISTANCE
POSE_LR, POSE_STEPS = 1e-2, 60


def pose_scene(device=None):
    """(GaussianSet, true Camera, start c2w [3,4]): 3000 Gaussians of GaussianSet.random (SH degree 1) with seeded random colours
    and first-order coefficients in place of its constant grey (a grey cloud has nothing to register against), opacity 0.5; the
    start pose is the true one turned by 1.5 degrees about an oblique axis and shifted by 3 % of the camera distance, camera-local"""
    import math

    import geosplatting_amd as gs
    g = torch.Generator().manual_seed(21)
    s = gs.GaussianSet.random(POSE_N, sh_degree=POSE_SH, random_scale=1.0, generator=g)
    s.colors = torch.rand(POSE_N, 3, generator=g)
    s.shs = torch.randn(POSE_N, 3, 3, generator=g) * 0.2
    s.opacities = torch.zeros(POSE_N, 1)
    cam = gs.orbit_cameras(8, POSE_DISTANCE, 20.0, POSE_W, POSE_H, focal=80.0)[3]
    axis = torch.tensor([0.48, -0.6, 0.64], dtype=torch.float64)
    a = math.radians(POSE_TURN_DEG)
    Kx = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    Rp = torch.eye(3, dtype=torch.float64) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)
    tp = torch.tensor([0.6, 0.64, -0.48], dtype=torch.float64) * POSE_SHIFT
    c = cam.c2w.double()
    start = torch.cat((c[:, :3] @ Rp, c[:, :3] @ tp[:, None] + c[:, 3:4]), dim=-1).float()
    if device is not None:
        s, cam, start = s.to(device), cam.to(device), start.to(device)
    return s, cam, start


def pose_errors(c2w, c2w_true):
    """(rotation error in degrees, translation error) of a pose [3,4] against the true one"""
    c2w, c2w_true = c2w.detach().double().cpu(), c2w_true.detach().double().cpu()
    cosang = ((c2w[:, :3].T @ c2w_true[:, :3]).trace() - 1.0) / 2.0
    return float(torch.rad2deg(torch.arccos(cosang.clamp(-1.0, 1.0)))), float((c2w[:, 3] - c2w_true[:, 3]).norm())
