"""GPU: every entry point that inlines the projection backward (project_bwd_one, csrc/gs_project_dev.h) against the oracle, ELEMENT BY
ELEMENT, within the oracle's error budget (oracle.project_bwd_budget, a running-error bound validated against float64 autograd in
tests/test_oracle_cpu.py): |got - want| <= kappa * 2^-24 * budget for every gradient of every Gaussian, culled ones (budget 0: exactly
0) included, on scenes built to drive the stage's regimes (tests/util.py PROJ_BUDGET_SCENES: near plane, the four routes of the
tan-fov clamp, tiny / anisotropic / isotropic / flat Gaussians, quaternion norms from 1e-3 to 1e3, culled rows interleaved), each
under dense, geometry-only, opacity-only and with-depth cotangents with all-zero rows.

Both sides read the SAME stored state: the oracle is fed the conics and compensations the GPU forward stored (for the tail kernels:
the fields of vis_records), so the budget needs no stored-state term.

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X (kappa = util.PROJ_BUDGET_KAPPA = 4; the budget is a rigorous bound, so a
correct kernel stays below 1 even with v_rcp_f32 / v_rsq_f32 and contraction on):
                                            v_means   v_quats   v_scales   v_opacities
    gs_project_bwd (accumulate 0 and 1)        0.51      0.07       0.20          0.00
    gs_project_bwd_cap                         0.51      0.07       0.17          0.00
    gs_project_bwd_ex, GS_PROJ_CLASSIC         0.45      0.07       0.17          0.00
    gs_tail_bwd (exact and counts_dev)         0.54      0.06       0.19          0.00
    gs_tail_bwd_multi, n = 1, 2, 3, 5, 8       0.35      0.04       0.18          0.41
    gs_tail_bwd_multi_parts, 1 then 2          0.35      0.03       0.16          0.41
    ... background launches 3 + 3 + 2          0.35      0.03       0.18          0.45
(v_opacities of one view is the single product v_op * comp: the same bits.)  gs_project_bwd_ex with sh_degree = -1, flags = 0 equals
gs_project_bwd bit for bit, and the forward's stored conics / compensations equal the oracle's bit for bit in every regime.

The tests bite: each of these one-line changes of project_bwd_one, built into a scratch library and never committed, was seen to fail
the tests of every entry point here on the MI355X -- except where noted below -- and, made in the oracle's C instead, fails
test_project_bwd_budget_vs_float64_autograd (ratios against the budget; the bar is kappa):
    1. the branches of the y clamp swapped                          v_means, every regime, ratios 2e4 .. 1e5
    2. gb = v_cb instead of 0.5f * v_cb                              v_means first (flat, isotropic, anisotropic), 1.5e4 .. 9e4
    3. `- eps2d * det_conic` dropped from G[3] only                  tiny regime (comp -> 0) 7e5 .. 1.4e6, anisotropic / flat 1.4e4 .. 2e4;
                                                                     the classic test passes, as it must (no compensation gradient)
    4. rz2 for rz3 in the clamped-route term of v_mc[2]             clamp_x / clamp_xy regimes only, v_means z, ratios 20 .. 470 (observed under a bar of 16)
    5. vqn[k] * inv without the `- dotp * qn[k]` projection         v_quats, quaternion-norm regime first, 7e4 .. 1.2e5
Run with -s to print the ratios of every gradient.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import oracle
from tests import util

pytestmark = pytest.mark.gpu

SCENES = list(util.PROJ_BUDGET_SCENES)
SINGLE = [s for s in SCENES if s != "orbit8"]
NAMES = ("v_means", "v_quats", "v_scales", "v_opacities")
TILE = 16
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module's tests: the worst ratio per entry point and gradient over whatever ran (shown with -s)"""
    yield
    print()
    for ep in sorted({k[0] for k in WORST}):
        print(f"    {ep:14s}" + "   ".join(f"{nm} {WORST.get((ep, nm), 0.0):6.2f}" for nm in NAMES))


def _R():
    return importlib.import_module("geosplatting_amd.rasterization")      # (the package attribute of that name is the function)


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = util.PROJ_BUDGET_SCENES[name]()
    fwd = [util.proj_scene_forward(sc, vi) for vi in range(len(sc["views"]))]          # asserts regimes and margins
    return sc, fwd


def _dev(cuda, sc):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda)
    return dict(means=t(sc["means"]), quats=t(sc["quats"]), scales=t(sc["scales"]), opac=t(sc["opacities"]))


def _view_dev(cuda, vw):
    vm = torch.tensor(vw["viewmat"], device=cuda); K = torch.tensor(vw["K"], device=cuda)
    R, t = vw["viewmat"][:3, :3].astype(np.float64), vw["viewmat"][:3, 3].astype(np.float64)
    return vm, K, torch.tensor((-R.T @ t).astype(np.float32), device=cuda)


def _forward(cuda, name, vi, D, classic=False):
    """GPU projection forward of a view: (x, view tensors, gids, conics, comps, counts (device), V, host copies); the visible set is
    the oracle's"""
    sc, fwd = _scene(name)
    vw = sc["views"][vi]
    x = _dev(cuda, sc)
    vm, K, _ = _view_dev(cuda, vw)
    colors = torch.tensor(util.scene_colors(sc, D), device=cuda)
    pr = _R()._project_stage(x["means"], x["quats"], x["scales"], x["opac"], colors, vm, K, vw["W"], vw["H"], TILE, 0.3, util.PROJ_NEAR,
                             1e10, sc["radius_clip"], classic=classic)
    torch.cuda.synchronize()
    V = int(pr.host_counts[0])
    gids, conics, comps, counts = pr.bufs[0], pr.bufs[4], pr.bufs[5], pr.bufs[10]
    host = dict(gids=gids[:V].cpu().numpy(), conics=conics[:V].cpu().numpy(), comps=comps[:V].cpu().numpy())
    assert np.array_equal(host["gids"], fwd[vi]["gaussian_ids"])
    same = np.array_equal(host["conics"], fwd[vi]["conics"]) and np.array_equal(host["comps"], fwd[vi]["compensations"])
    assert same                                  # project_exact is the bit-exact twin of the oracle's project_one, in every regime
    return x, (vm, K), gids, conics, comps, counts, V, host


def _oracle(sc, vw, host, cot, classic=False):
    vm2, vc, vo, vd = cot
    return oracle.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], sc["opacities"], vw["viewmat"], vw["K"], vw["W"], vw["H"],
                                     host["gids"], host["conics"], host["comps"], vm2, vc, vo, v_depths=vd, classic=classic)


def _check(label, got, want, bud, times=1.0, dead=None):
    """the four gradient arrays against times * (want, budget); `dead` rows (culled, or every cotangent zero) are exactly 0"""
    for nm, g, w, b in zip(NAMES, got, want, bud):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert np.isfinite(g).all(), (label, nm)
        if dead is not None:
            assert not g[dead].any() and not np.asarray(b)[dead].any(), (label, nm)
        r = util.assert_within_budget(f"{label} {nm}", g, times * w.astype(np.float64), times * b, util.PROJ_BUDGET_KAPPA)
        key = (label.split()[0], nm)
        WORST[key] = max(WORST.get(key, 0.0), r)


def _packed(cuda, cot, D, stride, rows=None, seed=0, fill=0.0):
    """v_packed [rows, stride] {xy, conic(3), opacity, colours(D), padding}: the cotangents in the first V rows, `fill` elsewhere
    (padding columns and capacity rows), colours random"""
    vm2, vc, vo, _ = cot
    V = len(vo)
    vp = np.full((V if rows is None else rows, stride), fill, np.float32)
    vp[:V, 0:2] = vm2; vp[:V, 2:5] = vc; vp[:V, 5] = vo
    vp[:V, 6:6 + D] = np.random.RandomState(seed).uniform(-1, 1, (V, D)).astype(np.float32)
    return torch.tensor(vp, device=cuda), vp


def _outs(cuda, N, D, fill):
    f = lambda *s: torch.full(s, fill, dtype=torch.float32, device=cuda)
    return [f(N, 3), f(N, 4), f(N, 3), f(N), f(N, max(D, 1))]


def _dead_rows(N, gids):
    dead = np.ones(N, bool); dead[gids] = False
    dead[gids[3::7]] = True
    return dead


@pytest.mark.parametrize("D,stride", [(3, 0), (5, 24)])
@pytest.mark.parametrize("scene", SINGLE)
def test_project_bwd_within_budget(cuda, scene, D, stride):
    """gs_project_bwd: accumulate = 0 over garbage (every row written, culled rows exactly 0), accumulate = 1 twice over zeros (twice
    the gradient within twice the budget), v_depths null and non-null, D = 3 with the default record stride and D = 5 with an explicit
    one (padding columns hold NaN: never read); v_colors is a pure gather, bit-exact"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc, _ = _scene(scene)
    vw = sc["views"][0]
    x, (vm, K), gids, conics, comps, _, V, host = _forward(cuda, scene, 0, D)
    N = sc["means"].shape[0]
    st = stride or lib.gs_raster_grad_stride(D)
    dead = _dead_rows(N, host["gids"])
    for kind in util.PROJ_COTANGENTS:
        cot = util.proj_budget_cotangents(kind, V, seed=3 + D)
        vp, vph = _packed(cuda, cot, D, st, seed=D, fill=np.nan)
        vd = None if cot[3] is None else torch.tensor(cot[3], device=cuda)
        want, bud = _oracle(sc, vw, host, cot)
        call = lambda o, acc: L.check(lib.gs_project_bwd(
            N, V, D, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]), L.ptr(vm), L.ptr(K), vw["W"], vw["H"],
            L.f32(0.3), L.ptr(gids), L.ptr(conics), L.ptr(comps), L.ptr(vp), stride, L.ptr(vd), L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]),
            L.ptr(o[3]), L.ptr(o[4]), acc, L.stream()), "gs_project_bwd")
        o = _outs(cuda, N, D, 123.0)
        call(o, 0)
        torch.cuda.synchronize()
        _check(f"bwd {scene}/{kind} D={D}", o[:4], want, bud, dead=dead)
        col = o[4].cpu().numpy()
        want_col = np.zeros((N, D), np.float32); want_col[host["gids"]] = vph[:, 6:6 + D]
        assert col.view(np.int32).tobytes() == want_col.view(np.int32).tobytes()
        o2 = _outs(cuda, N, D, 0.0)
        call(o2, 1); call(o2, 1)
        torch.cuda.synchronize()
        _check(f"bwd_acc {scene}/{kind} D={D}", o2[:4], want, bud, times=2.0, dead=dead)


@pytest.mark.parametrize("scene", SINGLE)
def test_project_bwd_ex_within_budget(cuda, scene):
    """gs_project_bwd_ex: with sh_degree = -1, flags = 0 it IS gs_project_bwd (bit for bit); with GS_PROJ_CLASSIC against the oracle's
    classic mode (v_opacities = v_opacity_packed exactly, no compensation gradient)"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc, _ = _scene(scene)
    vw = sc["views"][0]
    D = 3
    N = sc["means"].shape[0]
    st = lib.gs_raster_grad_stride(D)
    for classic in (False, True):
        x, (vm, K), gids, conics, comps, _, V, host = _forward(cuda, scene, 0, D, classic=classic)
        dead = _dead_rows(N, host["gids"])
        for kind in util.PROJ_COTANGENTS:
            cot = util.proj_budget_cotangents(kind, V, seed=17)
            vp, _ = _packed(cuda, cot, D, st, seed=1)
            vd = None if cot[3] is None else torch.tensor(cot[3], device=cuda)
            o = _outs(cuda, N, D, 123.0)
            L.check(lib.gs_project_bwd_ex(N, V, D, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]), L.ptr(vm),
                                          L.ptr(K), vw["W"], vw["H"], L.f32(0.3), L.ptr(gids), L.ptr(conics), L.ptr(comps), L.ptr(vp), st,
                                          L.ptr(vd), None, 0, -1, 1 if classic else 0, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]),
                                          L.ptr(o[4]), None, 0, L.stream()), "gs_project_bwd_ex")
            torch.cuda.synchronize()
            if classic:
                want, bud = _oracle(sc, vw, host, cot, classic=True)
                _check(f"ex_classic {scene}/{kind}", o[:4], want, bud, dead=dead)
                assert np.array_equal(o[3].cpu().numpy()[host["gids"]], cot[2])
            else:
                p = _outs(cuda, N, D, 55.0)
                L.check(lib.gs_project_bwd(N, V, D, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]), L.ptr(vm),
                                           L.ptr(K), vw["W"], vw["H"], L.f32(0.3), L.ptr(gids), L.ptr(conics), L.ptr(comps), L.ptr(vp), st,
                                           L.ptr(vd), L.ptr(p[0]), L.ptr(p[1]), L.ptr(p[2]), L.ptr(p[3]), L.ptr(p[4]), 0, L.stream()),
                        "gs_project_bwd")
                torch.cuda.synchronize()
                for a, b in zip(o, p):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("scene", SINGLE)
def test_project_bwd_cap_within_budget(cuda, scene):
    """gs_project_bwd_cap: the count read on the device, buffers sized V_cap = N; the capacity rows behind V hold NaN in v_packed and
    v_depths and the ids of culled Gaussians in gaussian_ids: nothing from beyond V may reach the output"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc, _ = _scene(scene)
    vw = sc["views"][0]
    D = 3
    N = sc["means"].shape[0]
    st = lib.gs_raster_grad_stride(D)
    x, (vm, K), gids, conics, comps, counts, V, host = _forward(cuda, scene, 0, D)
    dead = _dead_rows(N, host["gids"])
    culled = np.setdiff1d(np.arange(N), host["gids"]).astype(np.int32)
    assert 0 < len(culled) == N - V
    gids = gids.clone(); gids[V:] = torch.tensor(culled, device=cuda)
    conics = conics.clone(); conics[V:] = float("nan")
    comps = comps.clone(); comps[V:] = float("nan")
    for kind in util.PROJ_COTANGENTS:
        cot = util.proj_budget_cotangents(kind, V, seed=29)
        vp, _ = _packed(cuda, cot, D, st, rows=N, seed=2, fill=np.nan)
        vp[:V, 6 + D:] = 0.0
        vd = None
        if cot[3] is not None:
            vd = torch.full((N,), float("nan"), device=cuda); vd[:V] = torch.tensor(cot[3], device=cuda)
        want, bud = _oracle(sc, vw, host, cot)
        o = _outs(cuda, N, D, 123.0)
        L.check(lib.gs_project_bwd_cap(N, L.ptr(counts), D, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]),
                                       L.ptr(vm), L.ptr(K), vw["W"], vw["H"], L.f32(0.3), L.ptr(gids), L.ptr(conics), L.ptr(comps),
                                       L.ptr(vp), st, L.ptr(vd), L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.ptr(o[4]), 0,
                                       L.stream()), "gs_project_bwd_cap")
        torch.cuda.synchronize()
        _check(f"bwd_cap {scene}/{kind}", o[:4], want, bud, dead=dead)
        assert np.isfinite(o[4].cpu().numpy()).all()


# ----------------------------------------------------------------------------- the engine's tail kernels
def _env(cuda, seed=3, res=(64, 32, 16)):
    import geosplatting_amd as gs
    from geosplatting_amd.shading import _make_env
    g = torch.Generator().manual_seed(seed)
    levels = [(torch.rand(6, r, r, 3, generator=g) + 0.05).to(cuda) for r in res]
    base = (torch.rand(6, 16, 16, 3, generator=g) + 0.05).to(cuda)
    env = gs.TextureSplitSum(base, levels)
    return env, _make_env(gs.get_fg_lut(cuda), env)


def _shading_inputs(cuda, N):
    g = torch.Generator().manual_seed(5)
    return (torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(cuda), torch.rand(N, 3, generator=g).to(cuda),
            torch.rand(N, 2, generator=g).to(cuda))


def _front(cuda, name, vi, x, sh, e, mode):
    """gs_front_fwd of a view: (Front, V, host copies of the stored state the tail kernels read from vis_records)"""
    from geosplatting_amd import front as F
    sc, fwd = _scene(name)
    vw = sc["views"][vi]
    vm, K, cam_pos = _view_dev(cuda, vw)
    fr = F.front_stage(x["means"], x["quats"], x["scales"], x["opac"], sh[0], sh[1], sh[2], vm, K, cam_pos, e, vw["W"], vw["H"], 0.1, 1.0,
                       mode, near=util.PROJ_NEAR, radius_clip=sc["radius_clip"], want_packed_index=True)
    torch.cuda.synchronize()
    V = int(fr.host_counts[0])
    vis = fr.vis[:V].cpu().numpy()
    host = dict(gids=np.ascontiguousarray(vis[:, 13]).view(np.int32), comps=np.ascontiguousarray(vis[:, 12]),
                conics=np.stack([np.float32(2.0) * vis[:, 2], vis[:, 3], np.float32(2.0) * vis[:, 4]], 1).astype(np.float32))
    assert np.array_equal(host["gids"], fwd[vi]["gaussian_ids"])
    return fr, V, host, (vm, K, cam_pos)


def _grad_bufs(cuda, N, env, fill=0.0):
    from geosplatting_amd import _lib as L
    z = lambda *s: torch.full(s, fill, dtype=torch.float32, device=cuda)
    t = dict(means=z(N, 3), quats=z(N, 4), scales=z(N, 3), opac=z(N), normals=z(N, 3), kd=z(N, 3), ks=z(N, 2))
    tb, tl = torch.zeros_like(env.base), [torch.zeros_like(l) for l in env.levels]
    eg = L.GsEnvGrad(); eg.base = tb.data_ptr()
    for i, l in enumerate(tl):
        eg.levels[i] = l.data_ptr()
    return t, [tb] + tl, eg


def _shading_silent(t, texels, what):
    for k in ("normals", "kd", "ks"):
        assert not t[k].any(), (what, k)
    for a in texels:
        assert not a.any(), what


@pytest.mark.parametrize("mode", ["pbr", "diffuse"])
@pytest.mark.parametrize("scene", SINGLE)
def test_tail_bwd_within_budget(cuda, scene, mode):
    """gs_tail_bwd, exact form and counts_dev form (capacity rows of v_packed hold NaN): with zero colour cotangents only the
    projection half contributes to v_means / v_quats / v_scales / v_opacities, and the shading outputs and texel gradients are
    exactly 0 (the shading half keeps its own tests)"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd import front as F
    from geosplatting_amd.shading import _MODE
    lib = L.lib()
    sc, _ = _scene(scene)
    vw = sc["views"][0]
    N = sc["means"].shape[0]
    x = _dev(cuda, sc); sh = _shading_inputs(cuda, N)
    env, e = _env(cuda)
    fr, V, host, (vm, K, cam_pos) = _front(cuda, scene, 0, x, sh, e, _MODE[mode])
    dead = _dead_rows(N, host["gids"])
    st = lib.gs_raster_grad_stride(3)
    for kind in ("dense", "geometry", "opacity"):
        cot = util.proj_budget_cotangents(kind, V, seed=41)
        want, bud = _oracle(sc, vw, host, cot)
        for form in ("exact", "counts"):
            vp, _ = _packed(cuda, cot, 0, st, rows=V if form == "exact" else N, fill=np.nan if form == "counts" else 0.0)
            vp[:V, 6:] = 0.0
            t, texels, eg = _grad_bufs(cuda, N, env)
            F.tail_stage(V if form == "exact" else N, None if form == "exact" else fr.counts, x["means"], x["quats"], x["scales"], x["opac"],
                         sh[0], sh[1], sh[2], vm, K, cam_pos, e, eg, vw["W"], vw["H"], 0.1, 1.0, _MODE[mode], fr.vis, vp, t["means"],
                         t["quats"], t["scales"], t["opac"], t["normals"], t["kd"], t["ks"])
            torch.cuda.synchronize()
            _check(f"tail_{form} {scene}/{kind} {mode}", [t["means"], t["quats"], t["scales"], t["opac"]], want, bud, dead=dead)
            _shading_silent(t, texels, (form, kind))


def test_tail_multi_within_budget(cuda):
    """gs_tail_bwd_multi / gs_tail_bwd_multi_parts over n = 1, 2, 3, 5, 8 different cameras of one scene (every lanes-per-Gaussian
    variant; Gaussians visible in all, some or none of the views), parts = 3, then 1 followed by 2, then background launches (7)
    accumulated: want = the sum over the views of the oracle's gradients; budget = the sum of the per-view budgets plus
    3 * sum_v |g_v| for the three levels of the eight-lane tree sum"""
    from geosplatting_amd import front as F
    from geosplatting_amd.shading import _MODE
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc, _ = _scene("orbit8")
    N = sc["means"].shape[0]
    x = _dev(cuda, sc); sh = _shading_inputs(cuda, N)
    env, e = _env(cuda)
    M = _MODE["pbr"]
    st = lib.gs_raster_grad_stride(3)
    views, per_view, seen = [], [], np.zeros(N, int)
    for vi, vw in enumerate(sc["views"]):
        fr, V, host, (vm, K, cam_pos) = _front(cuda, "orbit8", vi, x, sh, e, M)
        cot = util.proj_budget_cotangents(("dense", "geometry", "opacity")[vi % 3], V, seed=60 + vi)
        vp, _ = _packed(cuda, cot, 0, st)
        views.append((vm, K, cam_pos, fr.vis, vp, fr.packed_index, vw["W"], vw["H"]))
        per_view.append(_oracle(sc, vw, host, cot))
        seen[host["gids"]] += 1
    assert (seen == 0).sum() > 20 and (seen == 8).sum() > 500 and ((seen > 0) & (seen < 8)).sum() > 200

    def expect(idx):
        want = [sum(per_view[i][0][k].astype(np.float64) for i in idx) for k in range(4)]
        mag = [sum(np.abs(per_view[i][0][k].astype(np.float64)) for i in idx) for k in range(4)]
        bud = [sum(per_view[i][1][k] for i in idx) + 3.0 * mag[k] for k in range(4)]
        return want, bud

    def multi(vs, t, eg, accumulate, parts):
        F.tail_multi_stage(vs, x["means"], x["quats"], x["scales"], x["opac"], sh[0], sh[1], sh[2], e, eg, 0.1, 1.0, M, t["means"], t["quats"],
                           t["scales"], t["opac"], t["normals"], t["kd"], t["ks"], accumulate=accumulate, parts=parts)

    def done(label, t, texels, idx):
        torch.cuda.synchronize()
        want, bud = expect(idx)
        _check(label, [t["means"], t["quats"], t["scales"], t["opac"]], want, bud, dead=seen == 0)
        _shading_silent(t, texels, label)

    for n in (1, 2, 3, 5, 8):
        t, texels, eg = _grad_bufs(cuda, N, env, fill=123.0)                      # accumulate = 0 must overwrite
        multi(views[:n], t, eg, False, 3)
        done(f"multi n={n}", t, texels, range(n))
    t, texels, eg = _grad_bufs(cuda, N, env, fill=123.0)
    multi(views, t, eg, False, 1)
    multi(views, t, eg, False, 2)
    done("multi_parts 1+2", t, texels, range(8))
    t, texels, eg = _grad_bufs(cuda, N, env, fill=123.0)
    multi(views[:3], t, eg, False, 7)
    multi(views[3:6], t, eg, True, 7)
    multi(views[6:], t, eg, True, 3)
    done("multi_bg 3+3+2", t, texels, range(8))
