"""GPU: the gradient of the view matrix -- gs_project_bwd_view (csrc/gs_project.hip), its autograd wiring in rasterization() /
rasterization_3dgs(), camera-pose refinement on it (geosplatting_amd/poseopt.py) and GSplatTrainer(pose_opt=True).

The reference and its budget are tests/viewgrad_ref.py (validated against float64 autograd without a GPU in
tests/test_viewgrad_cpu.py): |v_viewmat - want| <= VIEWGRAD_KAPPA * 2^-24 * B per element, B = sum_n b_n + |sum_n c_n|; a zero budget
(the last row, an all-culled scene, zero cotangents) means exactly zero.  Both sides read the same stored state: the reference is fed
the conics and compensations the GPU forward stored.

(b) of VIEWGRAD_KAPPA -- worst ratio |got - want| / (2^-24 B) seen on an MI355X (kappa = 2; (a), the float32 restatement on the
CPU, is 0.343):
    gs_project_bwd_view, the four scenes / views, plain colours and SH degree 0, antialiased          0.039
    ... SH degree 3, antialiased                                                                     0.039
    ... GS_PROJ_CLASSIC: plain and SH degree 0   0.032        SH degree 3                             0.025
    reduction edges, first n Gaussians of 'yaw': one visible Gaussian 0.177 | n = 63: 0.115 | 64: 0.137 | 65: 0.142 |
        255: 0.078 | 256: 0.075 | 257: 0.077 | 769: 0.025                      (n = 1: nothing visible, exact zeros)
    through autograd (rasterization / rasterization_3dgs, every combination of test 4)               0.034
The parameter gradients equalled gs_project_bwd_ex bit for bit in every case, for both accumulate values.
The tests bite.  Each of these one-line changes of project_bwd_view_kernel / project_view_sum_kernel, built into a scratch library
that is never committed, was run against this file on an MI355X:
(tests 1 and 2 and the all-culled test: 18 cases; ratios against the budget, the bar is kappa = 2):
    1. the covariance term dropped from c_R             16 of 18 fail (all but the two with nothing visible): whole scenes 6.8 .. 15,
                                                        the edge sizes up to 4 303
    2. v_Cc not symmetrised (v_Cc for v_Cc + v_Cc^T)     16 fail: whole scenes 3.4 .. 7.6, edge sizes up to 2 152
    3. the t[i] v_dir[j] term dropped                   only SH degree 3 fails, 15 .. 108 (edge sizes up to 12 587); plain colours and
                                                        SH degree 0 pass inside the same tests with their usual 0.005 .. 0.039
    4. R v_dir written with R^T                         only SH degree 3 fails, 10 .. 38 (edge sizes up to 1 888); the rest as in 3.
    5. the last PARTIAL workgroup's row skipped by      every N that is no multiple of 256 fails, 68 .. 1 699 on the whole scenes
       the sum kernel                                   (N = 3 000 / 2 300), up to 1.7e6 on the edge sizes; n = 256 passes (0.075)
    6. culled Gaussians not masked out of the sum       16 fail, 1 143 .. 64 223 (they were given the cotangents of a valid slot)
Run with -s to print the ratios.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import util
from tests import viewgrad_ref as vr
from tests.ws_poison import GUARD, poisoned

pytestmark = pytest.mark.gpu

TILE = 16
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print()
    for k in sorted(WORST):
        print(f"    {k:34s} worst ratio {WORST[k]:6.3f}")


def _R():
    return importlib.import_module("geosplatting_amd.rasterization")


def _note(label, r):
    WORST[label] = max(WORST.get(label, 0.0), r)


def _dev(cuda, sc):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda)
    return dict(means=t(sc["means"]), quats=t(sc["quats"]), scales=t(sc["scales"]), opac=t(sc["opacities"]))


def _forward(cuda, sc, vi, classic, coeffs, deg):
    """GPU projection forward: (x, (viewmat, K), gids, conics, comps, V, host copies of the stored state)"""
    vw = sc["views"][vi]
    x = _dev(cuda, sc)
    vm, K = torch.tensor(vw["viewmat"], device=cuda), torch.tensor(vw["K"], device=cuda)
    colors = torch.tensor(util.scene_colors(sc, 3) if deg is None else coeffs, device=cuda)
    pr = _R()._project_stage(x["means"], x["quats"], x["scales"], x["opac"], colors, vm, K, vw["W"], vw["H"], TILE, 0.3, util.PROJ_NEAR,
                             1e10, sc["radius_clip"], sh_degree=deg, classic=classic)
    torch.cuda.synchronize()
    V = int(pr.host_counts[0])
    gids, conics, comps = pr.bufs[0], pr.bufs[4], pr.bufs[5]
    host = dict(gids=gids[:V].cpu().numpy(), conics=conics[:V].cpu().numpy(), comps=comps[:V].cpu().numpy())
    return x, (vm, K), gids, conics, comps, V, host


def _packed(cuda, cot, rgb, stride, rows=None, fill=0.0):
    """v_packed [rows, stride] {xy, conic(3), opacity, colours(3), padding}: the cotangents in the first V rows, `fill` elsewhere"""
    vm2, vc, vo, _ = cot
    V = len(vo)
    vp = np.full((V if rows is None else rows, stride), fill, np.float32)
    vp[:V, 0:2] = vm2; vp[:V, 2:5] = vc; vp[:V, 5] = vo
    vp[:V, 6:9] = rgb
    return torch.tensor(vp, device=cuda)


def _outs(cuda, N, K, fill):
    f = lambda *s: torch.full(s, fill, dtype=torch.float32, device=cuda)
    return [f(N, 3), f(N, 4), f(N, 3), f(N), f(N, 3), f(N, max(K, 1), 3)]


class _Call:
    """one (scene, view, mode, SH) on the device, ready to be called through gs_project_bwd_ex and gs_project_bwd_view"""

    def __init__(self, cuda, sc, vi, classic, deg, K=None):
        from geosplatting_amd import _lib as L
        self.L, self.lib, self.cuda = L, L.lib(), cuda
        self.sc, self.vw, self.classic, self.deg = sc, sc["views"][vi], classic, deg
        self.N = sc["means"].shape[0]
        self.coeffs = None if deg is None else vr.sh_inputs(sc, vi, deg, K=K)
        self.K = 0 if deg is None else self.coeffs.shape[1]
        self.x, (self.vm, self.Km), self.gids, self.conics, self.comps, self.V, self.host = _forward(cuda, sc, vi, classic, self.coeffs, deg)
        self.co = None if deg is None else torch.tensor(self.coeffs, device=cuda)
        self.stride = self.lib.gs_raster_grad_stride(3)

    def _common(self, vp, stride, vd):
        L, x, vw = self.L, self.x, self.vw
        return (self.N, self.V, 3, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]), L.ptr(self.vm), L.ptr(self.Km),
                vw["W"], vw["H"], L.f32(0.3), L.ptr(self.gids), L.ptr(self.conics), L.ptr(self.comps), L.ptr(vp), stride, L.ptr(vd),
                L.ptr(self.co), self.K, -1 if self.deg is None else self.deg, 1 if self.classic else 0)

    def _grads(self, o):
        L = self.L
        sh = self.deg is not None
        return (L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), None if sh else L.ptr(o[4]), L.ptr(o[5]) if sh else None)

    def ex(self, vp, vd, o, acc, stride=None):
        L = self.L
        args = self._common(vp, self.stride if stride is None else stride, vd) + self._grads(o)
        L.check(self.lib.gs_project_bwd_ex(*args, acc, L.stream()), "gs_project_bwd_ex")

    def view(self, vp, vd, o, acc, out16, stride=None, ws=None):
        L = self.L
        nbytes = self.lib.gs_project_bwd_view_ws_bytes(self.N)
        ws = L.workspace(nbytes, self.cuda) if ws is None else ws
        args = self._common(vp, self.stride if stride is None else stride, vd) + self._grads(o)
        L.check(self.lib.gs_project_bwd_view(*args, acc, L.ptr(out16), L.ptr(ws), nbytes, L.stream()), "gs_project_bwd_view")

    def reference(self, cot, rgb):
        sh = None if self.deg is None else (self.deg, self.coeffs, rgb)
        return vr.view_reference(self.sc, self.vw, self.host["gids"], self.host["conics"], self.host["comps"], cot, self.classic, sh)[:2]


def _bits_equal(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


def _check_case(c, label, kind, seed, rows=None, fill=0.0, stride=None):
    """one cotangent kind through both entry points: v_viewmat within budget (a plain write over garbage, also with accumulate = 1),
    the parameter gradients bit for bit those of gs_project_bwd_ex for both accumulate values"""
    cuda = c.cuda
    cot, rgb = vr.cotangents(kind, c.V, seed, with_rgb=True)
    rgb_ref = None if c.deg is None else rgb
    vp = _packed(cuda, cot, rgb, c.stride if stride is None else stride, rows=rows, fill=fill)
    vd = None
    if cot[3] is not None:
        vd = torch.full((c.V if rows is None else rows,), fill, dtype=torch.float32, device=cuda)
        vd[:c.V] = torch.tensor(cot[3], device=cuda)
    want, bud = c.reference(cot, rgb_ref)
    got = []
    for acc in (0, 1):
        base = 123.0 if acc == 0 else 0.25
        a, b = _outs(cuda, c.N, c.K, base), _outs(cuda, c.N, c.K, base)
        out16 = torch.full((16,), float("nan") if acc == 0 else 77.0, device=cuda)
        c.ex(vp, vd, a, acc, stride)
        c.view(vp, vd, b, acc, out16, stride)
        torch.cuda.synchronize()
        assert _bits_equal(a, b), (label, kind, "accumulate", acc)
        got.append(out16.cpu().numpy())
    assert got[0].view(np.int32).tobytes() == got[1].view(np.int32).tobytes(), (label, kind)      # always a plain write
    assert not got[0][12:].any()
    r = util.assert_within_budget(f"{label} {kind}", got[0], want, bud, vr.VIEWGRAD_KAPPA)
    _note(label.split()[0], r)
    return got[0], want, bud


# ------------------------------------------------------------------------------------------------ 1. ABI level, per element
@pytest.mark.parametrize("classic", vr.MODES)
@pytest.mark.parametrize("name,vi", vr.VIEWS)
def test_view_gradient_within_budget(cuda, name, vi, classic):
    sc, _ = vr.scene(name)
    for deg in vr.SH_DEGREES:
        c = _Call(cuda, sc, vi, classic, deg)
        assert c.V > 1000
        for kind in util.PROJ_COTANGENTS:
            got, want, _ = _check_case(c, f"abi{'_classic' if classic else ''}{'' if deg is None else '_sh%d' % deg} {name}/{vi}", kind, 11 + vi)
            assert np.abs(got[:12]).min() > 0 or (kind == "opacity" and classic)


def test_arguments(cuda):
    """v_viewmat NULL, a short workspace and a NULL workspace are errors; the size comes from the layout (12 doubles per 256)"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    assert lib.gs_project_bwd_view_ws_bytes(0) == 96 and lib.gs_project_bwd_view_ws_bytes(256) == 96
    assert lib.gs_project_bwd_view_ws_bytes(257) == 192 and lib.gs_project_bwd_view_ws_bytes(1966080) == 7680 * 96
    sc, _, _, _ = vr.prefix("yaw", 0, 65)
    c = _Call(cuda, sc, 0, False, None)
    cot, rgb = vr.cotangents("dense", c.V, 1, with_rgb=True)
    vp = _packed(cuda, cot, rgb, c.stride)
    o = _outs(cuda, c.N, 0, 0.0)
    out16 = torch.zeros(16, device=cuda)
    ws = L.workspace(96, cuda)
    args = c._common(vp, c.stride, None) + c._grads(o)
    assert lib.gs_project_bwd_view(*args, 0, None, L.ptr(ws), 96, L.stream()) == -1 and b"NULL" in lib.gs_last_error()
    assert lib.gs_project_bwd_view(*args, 0, L.ptr(out16), None, 96, L.stream()) == -1
    assert lib.gs_project_bwd_view(*args, 0, L.ptr(out16), L.ptr(ws), 95, L.stream()) != 0 and b"workspace" in lib.gs_last_error()


# ------------------------------------------------------------------------------------------------ 2. reduction edges
@pytest.mark.parametrize("n", vr.PREFIX_SIZES + (0,))
def test_reduction_edges(cuda, n):
    """the first n Gaussians of 'yaw' (0: the prefix with exactly one visible Gaussian), B = 256 Gaussians per workgroup: a single
    wave, one short of / exactly / one past a wave and a workgroup, three workgroups and one Gaussian; capacity rows and padding
    columns of v_packed (and the rows of v_depths beyond V) hold NaN and are never read"""
    n = n or vr.one_visible_size()
    sc, gid, _, _ = vr.prefix("yaw", 0, n)
    for classic, deg in ((False, None), (True, 3)):
        c = _Call(cuda, sc, 0, classic, deg)
        assert np.array_equal(c.host["gids"], gid)
        assert n != vr.one_visible_size() or c.V == 1
        for kind in ("dense", "depth"):
            _check_case(c, f"edge n={n}", kind, 7, rows=n, fill=np.nan, stride=24)


def test_nothing_visible_writes_zeros(cuda):
    """V = 0 (every Gaussian culled) and N = 0: sixteen exact zeros over garbage"""
    sc, _ = vr.scene("yaw")
    c = _Call(cuda, sc, 0, False, 3)
    c.V = 0
    vp = torch.full((c.N, c.stride), float("nan"), device=cuda)
    for N in (c.N, 0):
        c.N = N
        o = _outs(cuda, max(N, 1), c.K, 5.0)
        out16 = torch.full((16,), float("nan"), device=cuda)
        c.view(vp, None, o, 0, out16)
        torch.cuda.synchronize()
        assert not out16.cpu().numpy().any()
        if N:
            assert not any(t.any() for t in o[:4]) and not o[5].any()


# ------------------------------------------------------------------------------------------------ 3. reproducible, workspace contract
def test_reproducible_under_poisoned_workspace(cuda):
    """two calls give identical bits; so does a call whose workspace was pre-filled with NaN, with 0xFF or with what a previous call
    left; the guard bytes around the workspace stay intact (tests/ws_poison.py checks them on exit)"""
    from geosplatting_amd import _lib as L
    sc, _, _, _ = vr.prefix("yaw", 0, 3 * vr.VIEW_BLOCK + 1)
    c = _Call(cuda, sc, 0, False, 3)
    cot, rgb = vr.cotangents("depth", c.V, 3, with_rgb=True)
    vp = _packed(cuda, cot, rgb, c.stride)
    vd = torch.tensor(cot[3], device=cuda)
    nbytes = c.lib.gs_project_bwd_view_ws_bytes(c.N)
    assert nbytes == 4 * 96

    def run(ws=None):
        o, out16 = _outs(cuda, c.N, c.K, 9.0), torch.full((16,), float("nan"), device=cuda)
        c.view(vp, vd, o, 0, out16, ws=ws)
        torch.cuda.synchronize()
        return [t.clone() for t in o] + [out16]

    first = run()
    assert np.isfinite(first[-1].cpu().numpy()).all() and first[-1][:12].abs().min() > 0
    assert _bits_equal(first, run())
    block = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=cuda)
    block.view(torch.float32)[:] = float("nan")
    marks = block.clone()
    assert _bits_equal(first, run(ws=block[GUARD:GUARD + nbytes]))
    assert torch.equal(block[:GUARD], marks[:GUARD]) and torch.equal(block[GUARD + nbytes:], marks[GUARD + nbytes:])
    for mode in ("ones", "zero", "recycle"):
        with poisoned(mode) as p:
            assert _bits_equal(first, run())
        assert p.sizes == [nbytes]


# ------------------------------------------------------------------------------------------------ 4. autograd level
@pytest.mark.parametrize("deg", [None, 2])
@pytest.mark.parametrize("render_mode", ["RGB", "RGB+ED"])
@pytest.mark.parametrize("means2d_grad", [False, True])
@pytest.mark.parametrize("fn", ["rasterization", "rasterization_3dgs"])
def test_autograd_view_gradient(cuda, monkeypatch, fn, means2d_grad, render_mode, deg):
    """viewmats.requires_grad_() -> viewmats.grad [1,4,4], last row 0, within budget of the reference fed with that run's own v_packed
    and stored state.  The other gradients are bit for bit what the same projection backward gives without the view gradient ON
    THE SAME v_packed (the compositor's backward adds with float atomics, so two separate backward passes never promised equal
    bits); a second whole run with viewmats.requires_grad_(False) asks for exactly today's scratch and agrees to 1e-4 of the largest entry."""
    import geosplatting_amd as gs
    from geosplatting_amd import _lib as L
    R = _R()
    lib = L.lib()
    sc, _ = vr.scene("yaw")
    vw = sc["views"][0]
    classic = fn == "rasterization_3dgs"
    W, H = vw["W"], vw["H"]
    coeffs = None if deg is None else vr.sh_inputs(sc, 0, deg)
    colors = util.scene_colors(sc, 3) if deg is None else coeffs
    g = torch.Generator().manual_seed(5)
    D = 3 + (render_mode != "RGB")
    wr, wa = (torch.rand(1, H, W, D, generator=g) * 2 - 1).to(cuda), (torch.rand(1, H, W, 1, generator=g) * 2 - 1).to(cuda)
    captured = []
    real = R._project_backward

    def spy(saved, cfg, st, v_packed, want_viewmat=False):
        captured.append((saved, cfg, dict(st), v_packed.clone(), want_viewmat))
        return real(saved, cfg, st, v_packed, want_viewmat)

    monkeypatch.setattr(R, "_project_backward", spy)

    def run(view_grad):
        leaf = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda).requires_grad_(True)
        x = [leaf(sc["means"]), leaf(sc["quats"]), leaf(sc["scales"]), leaf(sc["opacities"]), leaf(colors)]
        vm = torch.tensor(vw["viewmat"], device=cuda)[None].requires_grad_(view_grad)
        with poisoned("ones") as p:
            render, alpha, meta = getattr(gs, fn)(*x, vm, torch.tensor(vw["K"], device=cuda)[None], W, H, near_plane=util.PROJ_NEAR,
                                                  radius_clip=sc["radius_clip"], sh_degree=deg, render_mode=render_mode,
                                                  rasterize_mode="classic" if classic else "antialiased", means2d_grad=means2d_grad)
            ((render * wr).sum() + (alpha * wa).sum()).backward()
        return x, vm, meta, p.sizes

    x, vm, meta, sizes = run(True)
    saved, cfg, st, v_packed, asked = captured[-1]
    assert asked and vm.grad is not None and vm.grad.shape == (1, 4, 4) and not vm.grad[0, 3].any()
    V, depth_channel = cfg[3], cfg[4]
    assert depth_channel == (render_mode != "RGB") and V > 1000
    vp = v_packed.cpu().numpy()
    cot = (vp[:, 0:2].copy(), vp[:, 2:5].copy(), vp[:, 5].copy(), vp[:, 9].copy() if depth_channel else None)
    host = {k: st[k].cpu().numpy() for k in ("gaussian_ids_i32", "conics", "compensations")}
    sh = None if deg is None else (deg, coeffs, vp[:, 6:9].copy())
    want, bud, _ = vr.view_reference(sc, vw, host["gaussian_ids_i32"], host["conics"], host["compensations"], cot, classic, sh)
    r = util.assert_within_budget(f"autograd {fn} m2d={means2d_grad} {render_mode} sh={deg}", vm.grad.reshape(16).cpu().numpy(), want, bud,
                                  vr.VIEWGRAD_KAPPA)
    _note("autograd", r)
    plain = real(saved, cfg, st, v_packed, False)
    assert plain[5] is None
    for leaf_t, gr in zip(x, plain[:5]):
        assert torch.equal(leaf_t.grad.view(torch.int32), gr.view(torch.int32))
    # the same call with the view matrix as data: no gradient, today's launches and scratch requests
    x2, vm2, meta2, sizes2 = run(False)
    assert vm2.grad is None and captured[-1][4] is False
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    N, I = sc["means"].shape[0], int(meta["flatten_ids"].shape[0])
    today = [lib.gs_project_ws_bytes(N), max(lib.gs_isect_bin_ws_bytes(V, I, tw, th), 1), lib.gs_raster_ws_bytes(I, V, W, H, TILE)]
    assert sizes2 == today and sizes == today + [lib.gs_project_bwd_view_ws_bytes(N)]
    for a, b in zip(x, x2):
        assert float((a.grad - b.grad).abs().max()) <= 1e-4 * float(b.grad.abs().max())


# ------------------------------------------------------------------------------------------------ 5. pose recovery
def _pose_loop(cuda, detach):
    import geosplatting_amd as gs
    s, cam, start = vr.pose_scene(cuda)
    model = gs.GSplatModel(gaussians=s, sh_degree=vr.POSE_SH, rasterize_mode="classic", background_color="black", training=False)
    black = torch.zeros(3, device=cuda)
    with torch.no_grad():
        target = model.render_rgb(cam, black)
    deltas = gs.CameraPoseDeltas(1, device=cuda)
    opt = torch.optim.Adam(deltas.parameters(), lr=vr.POSE_LR)
    losses = []
    for _ in range(vr.POSE_STEPS):
        opt.zero_grad()
        c2w = deltas.apply(start, 0)
        moved = gs.Camera(c2w.detach() if detach else c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
        loss = (model.render_rgb(moved, black) - target).square().mean()
        if loss.requires_grad:
            loss.backward()
        opt.step()
        losses.append(loss.detach())
    return deltas, start, cam, [float(l) for l in losses]


def test_pose_recovery(cuda):
    """3 000 Gaussians of GaussianSet.random (SH degree 1, 'classic'), 97 x 61, one camera: the target is rendered at the true pose,
    the start pose is turned 1.5 degrees about an oblique axis and shifted by 3 % of the camera distance; only the nine pose numbers
    are optimised, Adam (lr POSE_LR) on a plain MSE for POSE_STEPS steps.  Conditions: the loss falls, the rotation and the
    translation error both end below half of where they began (1.5 deg, 0.09), and with the view gradient disconnected the pose does
    not move at all.  Learning rate and step count come from scripts/poseopt_reference.py, the same loop on the CPU oracle with the
    view gradient of tests/viewgrad_ref.py in float64, which ends at 0.120 deg / 0.0041 (loss 9.99e-3 -> 3.69e-6).
    On an MI355X: loss 9.987e-3 -> 3.691e-6, rotation 1.500 -> 0.119 deg, translation 0.0900 -> 0.0041."""
    deltas, start, cam, losses = _pose_loop(cuda, detach=False)
    r0, t0 = vr.pose_errors(start, cam.c2w)
    r1, t1 = vr.pose_errors(deltas.apply(start, 0), cam.c2w)
    print(f"\n  pose recovery: loss {losses[0]:.3e} -> {losses[-1]:.3e}; rotation {r0:.3f} -> {r1:.3f} deg; translation {t0:.4f} -> {t1:.4f}")
    assert abs(r0 - vr.POSE_TURN_DEG) < 1e-3 and abs(t0 - vr.POSE_SHIFT) < 1e-5
    assert losses[-1] < losses[0]
    assert r1 < 0.5 * r0 and t1 < 0.5 * t0
    still, start, cam, _ = _pose_loop(cuda, detach=True)
    assert not still.deltas.any() and still.deltas.grad is None


# ------------------------------------------------------------------------------------------------ 6. trainer
TRAINER_FIELDS = dict(warmup_length=2, refine_every=2, reset_alpha_every=100, sh_degree_interval=2, stop_split_at=100)


def _trainer_case(cuda, **kw):
    import geosplatting_amd as gs
    gen = torch.Generator().manual_seed(31)
    n = 300
    hidden = gs.GaussianSet(means=(torch.rand(n, 3, generator=gen) - 0.5) * 1.2, scales=torch.log(0.03 + 0.07 * torch.rand(n, 3, generator=gen)),
                            quats=torch.randn(n, 4, generator=gen), opacities=torch.full((n, 1), 2.0), colors=torch.rand(n, 3, generator=gen),
                            shs=torch.randn(n, 3, 3, generator=gen) * 0.05).to(cuda)
    cam = gs.orbit_cameras(4, 3.0, 20.0, 64, 48, focal=70.0)[1]
    with torch.no_grad():
        gt = gs.GSplatModel(gaussians=hidden, sh_degree=1, training=False, background_color="black").render_rgba(cam).clamp(0, 1)
    model = gs.GSplatModel(num_random=1200, random_scale=0.8, sh_degree=1, prepare_densification=True, device=cuda,
                           generator=torch.Generator().manual_seed(32), background_color="black")
    trainer = gs.GSplatTrainer(generator=torch.Generator(device=cuda).manual_seed(33), **TRAINER_FIELDS, **kw)
    trainer.setup(model, dataset_size=1)
    return model, trainer, cam, gt


def test_trainer_pose_opt(cuda):
    """GSplatTrainer(pose_opt=True): three train_steps change "poses"; the Gaussian-count logic and mutate_adam keep working across the
    densify event of step 4 (the pose optimizer is no Gaussian field: untouched by it)"""
    model, trainer, cam, gt = _trainer_case(cuda, pose_opt=True, pose_lr=1e-3)
    assert set(trainer.optimizers) == {"means", "scales", "quats", "colors", "opacities", "shs", "poses"}
    assert trainer.optimizers["poses"].defaults["weight_decay"] == trainer.pose_reg == 1e-6
    assert trainer.pose_deltas.deltas.shape == (1, 9) and not trainer.pose_deltas.deltas.any()
    for step in (1, 2, 3):
        trainer.train_step(model, cam, gt, curr_step=step, camera_index=0)
    d3 = trainer.pose_deltas.deltas.detach().clone()
    assert torch.isfinite(d3).all() and (d3[0, [0, 1, 2, 4, 5, 8]] != 0).all()
    n_before = len(model.gaussians)
    trainer.train_step(model, cam, gt, curr_step=4, camera_index=0)
    assert trainer.refined == [(4, "densify")] and len(model.gaussians) != n_before
    n = len(model.gaussians)
    for name in ("means", "scales", "quats", "colors", "opacities", "shs"):
        opt = trainer.optimizers[name]
        (p,) = opt.param_groups[0]["params"]
        assert p is getattr(model.gaussians, name) and p.shape[0] == n and opt.state[p]["exp_avg"].shape == p.shape
    (pp,) = trainer.optimizers["poses"].param_groups[0]["params"]
    assert pp is trainer.pose_deltas.deltas and trainer.optimizers["poses"].state[pp]["exp_avg"].shape == (1, 9)
    loss, _ = trainer.train_step(model, cam, gt, curr_step=5, camera_index=0)
    assert torch.isfinite(loss) and not torch.equal(trainer.pose_deltas.deltas.detach(), d3)
    # without an index the step renders through the camera as given and the poses stay
    d5 = trainer.pose_deltas.deltas.detach().clone()
    trainer.train_step(model, cam, gt, curr_step=7)
    assert trainer.pose_deltas.deltas.grad is None or not trainer.pose_deltas.deltas.grad.any()
    assert float((trainer.pose_deltas.deltas.detach() - d5).abs().max()) <= 1e-6 * float(d5.abs().max())     # (weight decay alone)


def test_trainer_without_pose_opt_is_the_parent_path(cuda, monkeypatch):
    """pose_opt=False given explicitly, with a camera_index passed, against the default: no pose state, no "poses" optimizer, the
    model receives the caller's own Camera object in every step, the loss of the first step -- a forward alone -- is the default
    trainer's bit for bit and the next two agree to 1e-5.  Past the first backward, bits are not a property the parent has: the
    compositor's backward adds with float atomics, Adam's first steps have the size of the learning rate whatever the gradient's
    size, and a gradient at noise level flips its sign.  On an MI355X two runs of the DEFAULT trainer end 5.6e-3 (of the largest
    entry) apart after three steps, and the explicit run 5.6e-3 and 5.5e-3 from them; the three losses were the same bits in all
    runs.  So the parameters are compared three ways and the explicit run may be no farther from a default run than twice what the
    two default runs are from each other."""
    import geosplatting_amd as gs
    runs = []
    for kw, idx in ((dict(), None), (dict(), None), (dict(pose_opt=False), 0)):
        model, trainer, cam, gt = _trainer_case(cuda, **kw)
        assert trainer.pose_deltas is None and "poses" not in trainer.optimizers
        assert sorted(trainer.optimizers) == ["colors", "means", "opacities", "quats", "scales", "shs"]
        seen = []
        real = gs.GSplatModel.render_layers
        monkeypatch.setattr(gs.GSplatModel, "render_layers", lambda self, camera, _r=real, _s=seen: (_s.append(camera), _r(self, camera))[1])
        losses = []
        for step in (1, 2, 3):
            if idx is None:
                loss, _ = trainer.train_step(model, cam, gt, curr_step=step)
            else:
                loss, _ = trainer.train_step(model, cam, gt, curr_step=step, camera_index=idx)
            losses.append(loss.clone())
        monkeypatch.setattr(gs.GSplatModel, "render_layers", real)
        assert all(c is cam for c in seen) and len(seen) == 3
        runs.append((losses, {k: v.detach().clone() for k, v in model.gaussians.parameters().items()}))
    (la, pa), (lb, pb), (lc, pc) = runs
    assert torch.equal(la[0].view(torch.int32), lb[0].view(torch.int32)) and torch.equal(la[0].view(torch.int32), lc[0].view(torch.int32))
    assert sorted(pa) == sorted(pb) == sorted(pc)
    far = lambda p, q: max(float((p[k] - q[k]).abs().max()) / float(p[k].abs().max()) for k in p)
    print(f"\n  parameters after three steps, largest relative distance: default/default {far(pa, pb):.2e}, "
          f"explicit/default {far(pa, pc):.2e} and {far(pb, pc):.2e}; losses {[float(l) for l in la]} {[float(l) for l in lc]}")
    assert max(far(pa, pc), far(pb, pc)) <= 2.0 * far(pa, pb) + 1e-6
    for a, b, c in zip(la, lb, lc):
        assert abs(float(a) - float(c)) <= 1e-5 * abs(float(a)) and abs(float(a) - float(b)) <= 1e-5 * abs(float(a))
