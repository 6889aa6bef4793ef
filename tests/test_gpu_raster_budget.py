"""GPU: every compositor backward entry point against the oracle, ELEMENT BY ELEMENT, within the oracle's error budget
(oracle.raster_bwd_budget, validated against float64 autograd in tests/test_oracle_cpu.py): |got - want| <= kappa * 2^-24 * budget
for every packed gradient of every visible Gaussian, on scenes built to drive the kernels' capacity and assist branches (tests/util.py:
deep stack, opaque veil, speckle, ragged image), each under dense, alpha-only and sparse cotangents.

The forward is bit-identical to the oracle (tests/test_gpu_rasterizer.py), so both sides read the same alphas / last_ids and the
oracle is fed the GPU's own projected per-Gaussian inputs.

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X over the four scenes and three cotangents (kappa = util.BUDGET_KAPPA = 16):
    gs_raster_bwd          D = 1: 1.57   2: 1.79   3: 1.70   4: 1.81   14: 1.68   32: 1.84
    gs_raster_bwd_acc      D = 3: 1.99   14: 1.82          gs_raster_bwd_acc_cap   D = 3: 1.63
    gs_raster_bwd_tone_acc          none 2.21   naive 1.77   aces 3.31
    cull-log pair (tone_log)        none 1.74   naive 1.89   aces 3.31   (the same with -DGS_LOG_ASSIST_MAX=0 / =64, and within
                                    2.21 with -DGS_BWD_LOG_EXACT_MATH)
(aces: the oracle's tone-mapping derivative and the kernel's differ by an ulp or two in the cotangent itself.)  Run with -s to print
the ratios of every gradient and the measured scene properties.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import oracle
from tests import util

pytestmark = pytest.mark.gpu

SCENES = list(util.BUDGET_SCENES)
KINDS = ["dense", "alpha", "sparse"]
TILE = 16


def _R():
    return importlib.import_module("geosplatting_amd.rasterization")      # (the package attribute of that name is the function)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """the scene, with its branch-driving properties asserted on the oracle's forward (so that a later change of the scene or of a
    constant cannot silently stop covering the branch)"""
    sc = util.BUDGET_SCENES[name]()
    W, H = sc["W"], sc["H"]
    m = oracle.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], util.scene_colors(sc, 3), sc["viewmat"], sc["K"],
                             W, H, background=sc["background"])
    st = util.raster_pair_stats(W, H, m["means2d"], m["conics"], m["opacities"], m["isect_offsets"], m["flatten_ids"], m["last_ids"])
    print(f"\n  scene {name} {W}x{H}: {len(m['gaussian_ids'])} visible, {len(m['flatten_ids'])} intersections, {st}")
    if name == "deep_stack":      # long walks, many dense batches, pair buffers overflowing (GS_PAIR_CAP 448, GS_LOG_PAIR_CAP 790)
        assert st["max_list"] > 4096 and st["max_live_per64"] > 790, st
    elif name == "veil":          # termination at many depths inside one quadrant; alpha at the 0.999 clamp
        assert st["max_distinct_last"] >= 8 and st["clamped_live"] > 0, st
    elif name == "speckle":       # a batch of some quadrant touches at most 16 pixels (GS_LOG_ASSIST_MAX)
        assert st["min_busy_pixels"] is not None and st["min_busy_pixels"] <= 16, st
    elif name == "ragged":        # empty tiles beside heavy ones
        assert st["min_list"] == 0 and st["max_list"] > 2000, st
    return sc


def _bg(sc, D):
    return None if sc["background"] is None else np.resize(sc["background"], D).astype(np.float32)


def _project(cuda, sc, D):
    t = lambda a: torch.tensor(a, device=cuda)
    return _R()._project_stage(t(sc["means"]), t(sc["quats"]), t(sc["scales"]), t(sc["opacities"]), t(util.scene_colors(sc, D)),
                               t(sc["viewmat"]), t(sc["K"]), sc["W"], sc["H"], TILE, 0.3, 0.01, 1e10, 0.0)


@functools.lru_cache(maxsize=None)
def _forward(name, D, with_bg, user=""):
    """GPU forward (exact counts) of a scene at D channels: (state, V, I, render, alphas, host copies of the compositor inputs); one
    per `user`, so that no test's workspace has seen another test's forwards"""
    R = _R()
    sc = _scene(name)
    cuda = torch.device("cuda:0")
    bg = _bg(sc, D) if with_bg else None
    state, V, I, D_, whs = R._bin_stage(_project(cuda, sc, D))
    state = R._prepare_stage(state, V, I, D_, whs)
    render, alphas, st, _, _ = R._composite_stage(state, V, I, D_, whs, None if bg is None else torch.tensor(bg, device=cuda))
    torch.cuda.synchronize()
    host = dict(means2d=st["means2d"].cpu().numpy(), conics=st["conics"].cpu().numpy(), opacities=st["opacities"].cpu().numpy(),
                colors=st["colors"].cpu().numpy(), offsets=st["isect_offsets"].cpu().numpy().reshape(-1),
                flatten_ids=st["flatten_ids"].cpu().numpy(), alphas=alphas.cpu().numpy(), last_ids=st["last_ids"].cpu().numpy(),
                render=render.cpu().numpy(), bg=bg)
    # the forward the budget relies on: the oracle's, bit for bit, on the same inputs
    r, a, last, _, _ = oracle.raster_fwd(sc["W"], sc["H"], TILE, host["means2d"], host["conics"], host["opacities"], host["colors"],
                                         host["offsets"], host["flatten_ids"], bg)
    assert np.array_equal(last, host["last_ids"]) and np.array_equal(a, host["alphas"])
    bad = np.argwhere(r.view(np.int32) != host["render"].view(np.int32))
    assert len(bad) == 0, (f"render differs from the oracle's in {len(bad)} values, first {[tuple(b) for b in bad[:4]]}: "
                           f"got {[host['render'][tuple(b)] for b in bad[:4]]} want {[r[tuple(b)] for b in bad[:4]]}")
    return st, V, I, render, alphas, host


def _check(label, sc, host, v_packed, v_render, v_alpha, D, V):
    """v_packed [>= V, stride] (GPU) against the oracle's gradients and budget for the cotangents (v_render, v_alpha); returns the
    worst ratio"""
    vp = v_packed.cpu().numpy()
    assert not vp[V:].any()                                          # capacity rows beyond the visible set stay untouched
    vp = vp[:V]
    (g_m, g_c, g_col, g_o), (b_m, b_c, b_col, b_o) = oracle.raster_bwd_budget(
        sc["W"], sc["H"], TILE, host["means2d"], host["conics"], host["opacities"], host["colors"], host["offsets"],
        host["flatten_ids"], host["alphas"], host["last_ids"], v_render, v_alpha, background=host["bg"])
    assert float(np.abs(g_o).max()) > 0
    worst = 0.0
    for nm, got, want, bud in (("v_means2d", vp[:, 0:2], g_m, b_m), ("v_conics", vp[:, 2:5], g_c, b_c),
                               ("v_opacities", vp[:, 5], g_o, b_o), ("v_colors", vp[:, 6:6 + D], g_col, b_col)):
        worst = max(worst, util.assert_within_budget(f"{label} {nm}", got, want, bud))
    return worst


@pytest.mark.parametrize("D", [1, 2, 3, 4, 14, 32])
@pytest.mark.parametrize("scene", SCENES)
def test_raster_bwd_within_budget(cuda, scene, D):
    """gs_raster_bwd (what rasterization().backward() runs), every channel-count template, with the scene's background"""
    sc = _scene(scene)
    st, V, I, render, alphas, host = _forward(scene, D, True)
    bg = None if host["bg"] is None else torch.tensor(host["bg"], device=cuda)
    for kind in KINDS:
        vr, va = util.budget_cotangents(kind, sc["H"], sc["W"], D, seed=D)
        vp = _R()._raster_backward(sc["W"], sc["H"], TILE, D, V, I, st, bg, alphas, torch.tensor(vr, device=cuda),
                                   torch.tensor(va, device=cuda))
        torch.cuda.synchronize()
        _check(f"bwd D={D} {scene}/{kind}", sc, host, vp, vr, va, D, V)


@pytest.mark.parametrize("D", [3, 14])
@pytest.mark.parametrize("scene", SCENES)
def test_raster_bwd_acc_within_budget(cuda, scene, D):
    """gs_raster_bwd_acc: adds into a v_packed that already holds something (here: a first call with the same cotangents, so the
    result is twice the gradient)"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc = _scene(scene)
    st, V, I, render, alphas, host = _forward(scene, D, True)
    W, H = sc["W"], sc["H"]
    bg = None if host["bg"] is None else torch.tensor(host["bg"], device=cuda)
    rws = st["raster_ws"]
    for kind in KINDS:
        vr, va = util.budget_cotangents(kind, H, W, D, seed=30 + D)
        tvr, tva = torch.tensor(vr, device=cuda), torch.tensor(va, device=cuda)
        vp = torch.zeros(V, lib.gs_raster_grad_stride(D), device=cuda)
        for _ in range(2):
            L.check(lib.gs_raster_bwd_acc(W, H, TILE, D, V, L.ptr(st["colors"]), L.ptr(bg), L.i64(I), L.ptr(st["isect_offsets"]),
                                          L.ptr(alphas), L.ptr(st["last_ids"]), L.ptr(tvr), L.ptr(tva), L.ptr(vp), L.ptr(rws),
                                          C.c_size_t(rws.numel()), L.stream()), "gs_raster_bwd_acc")
        torch.cuda.synchronize()
        _check(f"acc D={D} {scene}/{kind}", sc, host, vp, 2.0 * vr, 2.0 * va, D, V)


@pytest.mark.parametrize("scene", SCENES)
def test_raster_bwd_acc_cap_within_budget(cuda, scene):
    """gs_raster_bwd_acc_cap: the capacity protocol (counts on the device, buffers sized V_cap = N and I_cap = I + 777), D = 3"""
    from geosplatting_amd import _lib as L
    R = _R()
    lib = L.lib()
    sc = _scene(scene)
    W, H, D = sc["W"], sc["H"], 3
    _, V, I, _, _, host = _forward(scene, D, True)
    bg = None if host["bg"] is None else torch.tensor(host["bg"], device=cuda)
    status = torch.zeros(3, dtype=torch.int64, device=cuda)
    state, Vc, Ic, D_, whs = R._bin_stage_cap(_project(cuda, sc, D), I + 777, status, want_ids=False)
    state = R._prepare_stage_cap(state, Vc, Ic, D_, whs)
    render, alphas, st = R._composite_stage_cap(state, Vc, Ic, D_, whs, bg)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and Ic > I and Vc >= V
    assert np.array_equal(alphas.cpu().numpy(), host["alphas"]) and np.array_equal(st["last_ids"].cpu().numpy(), host["last_ids"])
    rws = st["raster_ws"]
    for kind in KINDS:
        vr, va = util.budget_cotangents(kind, H, W, D, seed=40)
        tvr, tva = torch.tensor(vr, device=cuda), torch.tensor(va, device=cuda)
        vp = torch.zeros(Vc, lib.gs_raster_grad_stride(D), device=cuda)
        L.check(lib.gs_raster_bwd_acc_cap(W, H, TILE, D, Vc, L.ptr(st["colors"]), L.ptr(bg), L.i64(Ic), L.ptr(st["counts"]),
                                          L.ptr(st["isect_offsets"]), L.ptr(alphas), L.ptr(st["last_ids"]), L.ptr(tvr), L.ptr(tva),
                                          L.ptr(vp), L.ptr(rws), C.c_size_t(rws.numel()), L.stream()), "gs_raster_bwd_acc_cap")
        torch.cuda.synchronize()
        _check(f"acc_cap {scene}/{kind}", sc, host, vp, vr, va, D, V)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("scene", SCENES)
def test_raster_bwd_tone_within_budget(cuda, scene, log):
    """gs_raster_bwd_tone_acc (log=False) and the engine's cull-log pair gs_raster_composite_tone_log + gs_raster_bwd_tone_log_acc
    (log=True: hardware exp2 and one Newton step, assisted walk trips) for tone mapping none / naive / aces, D = 3, no background;
    the oracle's cotangents come from oracle.tonemap_bwd of the same image cotangent"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc = _scene(scene)
    W, H, D = sc["W"], sc["H"], 3
    st, V, I, render, alphas, host = _forward(scene, D, False, "log" if log else "tone")
    exposure = torch.tensor([1.3], device=cuda)
    rws = st["raster_ws"]
    offs = L.ptr(st["isect_offsets"])
    rgba = np.concatenate([host["render"], host["alphas"][..., None]], -1)
    for tone, mode in (("none", 0), ("naive", 1), ("aces", 2)):
        img = torch.empty(H, W, 4, device=cuda)
        if log:                      # the backward reads the log of exactly this forward
            log_ws = torch.empty(lib.gs_raster_log_ws_bytes(L.i64(I), W, H, TILE), dtype=torch.uint8, device=cuda)
            r2, a2 = torch.empty_like(render), torch.empty_like(alphas)
            last2 = torch.empty_like(st["last_ids"])
            L.check(lib.gs_raster_composite_tone_log(W, H, TILE, V, L.ptr(st["colors"]), L.i64(I), None, offs, L.ptr(r2), L.ptr(a2),
                                                     L.ptr(last2), mode, L.ptr(exposure), L.ptr(img), L.ptr(rws), C.c_size_t(rws.numel()),
                                                     L.ptr(log_ws), C.c_size_t(log_ws.numel()), L.stream()), "gs_raster_composite_tone_log")
            torch.cuda.synchronize()
            assert torch.equal(r2, render) and torch.equal(a2, alphas) and torch.equal(last2, st["last_ids"])
        for kind in KINDS:
            vr, va = util.budget_cotangents(kind, H, W, D, seed=50 + mode)
            v_img = np.concatenate([vr, va[..., None]], -1)
            tv = torch.tensor(v_img, device=cuda)
            vp = torch.zeros(V, lib.gs_raster_grad_stride(D), device=cuda)
            v_exp = torch.zeros(1, device=cuda)
            if log:
                L.check(lib.gs_raster_bwd_tone_log_acc(W, H, TILE, V, L.ptr(st["colors"]), L.i64(I), None, offs, L.ptr(render), L.ptr(alphas),
                                                       L.ptr(st["last_ids"]), mode, L.ptr(exposure), L.ptr(tv), L.ptr(vp), L.ptr(v_exp),
                                                       L.ptr(rws), C.c_size_t(rws.numel()), L.ptr(log_ws), C.c_size_t(log_ws.numel()),
                                                       L.stream()), "gs_raster_bwd_tone_log_acc")
            else:
                L.check(lib.gs_raster_bwd_tone_acc(W, H, TILE, V, L.ptr(st["colors"]), L.i64(I), None, offs, L.ptr(render), L.ptr(alphas),
                                                   L.ptr(st["last_ids"]), mode, L.ptr(exposure), L.ptr(tv), L.ptr(vp), L.ptr(v_exp),
                                                   L.ptr(rws), C.c_size_t(rws.numel()), L.stream()), "gs_raster_bwd_tone_acc")
            torch.cuda.synchronize()
            v_rgba, _ = oracle.tonemap_bwd(rgba, 1.3, v_img, tone)
            _check(f"{'log' if log else 'tone'} {tone} {scene}/{kind}", sc, host, vp, v_rgba[..., :3], v_rgba[..., 3], D, V)
