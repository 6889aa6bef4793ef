"""GPU: every entry point that inlines the split-sum shading backward (S1..S3: csrc/gs_shade_dev.h, gs_shade.hip, the shading half of
gs_front.hip) against the oracle, ELEMENT BY ELEMENT, within the oracle's error budget (oracle.shade_bwd_budget, a running-error bound
validated against float64 autograd in tests/test_oracle_cpu.py): |got - want| <= kappa * 2^-24 * budget for every element of v_means,
v_normals, v_kd, v_ks and of every texel-gradient array -- rows with an all-zero colour cotangent and texels no footprint touches
(budget 0: exactly 0) included -- on scenes built to drive the stage's branches (tests/util.py SHADE_BUDGET_SCENES: every cube face,
edge from both sides and corner at every level in use, axis-aligned and zero directions, the FG-LUT clamps, back-facing / grazing /
0 < d < 1e-6 views, the mean at the camera, |mean - camera| from 1e-3 to 1e3, roughness below / on / between / above the environment's
bounds, pile-ups of hundreds of footprints on a few texels), under dense, single-channel and six-decade cotangents.  A texel element
that collects n contributions in an order nobody controls (LDS atomics, the block flush, HBM atomics, the XCD fold) is budgeted
sum(own bounds) + (n - 1) * sum |contribution|.

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X (kappa = util.SHADE_BUDGET_KAPPA = 4, the smallest power of two that is at
least 4 x the worst figure below):
                                              v_means  v_normals   v_kd   v_ks   texels
    gs_shade_bwd, accumulate 0 (over a pattern)   0.00      0.00   0.00   0.00     0.97
    gs_shade_bwd, accumulate 1 twice              0.00      0.00   0.00   0.00     0.04
    ... with the XCD-private workspace            0.00      0.00   0.00   0.00     0.95 / 0.01
    gs_shade_bwd, grid stride (n_iter = 2)        0.00      0.00   0.00   0.00     0.01
    gs_tail_bwd (exact and counts_dev)            0.00      0.00   0.00   0.00     0.03
    gs_tail_bwd_multi, n = 1, 2, 3, 5, 8          0.01      0.09   0.41   0.05     0.04
    gs_tail_bwd_multi_parts, 1 then 2             0.01      0.08   0.41   0.03     0.04
    ... background launches 3 + 3 + 2             0.01      0.08   0.41   0.03     0.03
    ... the three with gs_tail_priv_reduce (pbr)  0.01      0.02   0.41   0.05     0.01
The per-Gaussian gradients of gs_shade_bwd and gs_tail_bwd (shade_one<true>, contraction off) equal the oracle's bit for bit in every
regime; only the order of the texel sums differs, and single launches of the two are held to TEXEL_ORDER_BAR = 2 budgets on the
texels instead of kappa (see there).  The lean pair path (contracted, v_rcp_f32) stays below half the budget.  The 0.97 is the pattern
case, and it alone sets kappa: a texel that collects n contributions on top of a pattern value p is charged n |p| + sum |contribution|
more on the test's side (each of the n additions may round a sum that holds p; a worst-case bound like the oracle's, which nothing on
the CPU validates); over zeros the texels stay at 0.04.  The CPU side (tests/test_oracle_cpu.py, oracle against float64 autograd, bar
kappa / 2): worst 0.28.

The forward is not under test here, but gs_shade_fwd was seen to equal oracle.shade_fwd bit for bit in every scene and mode
(test_shade_bwd_within_budget asserts it).

Whether the tests bite.  Each one-line change below was built into a scratch library and this module, test_gpu_shading.py::
test_shade_fwd_bwd ("old A", max norm 1e-4) and test_gpu_front.py::test_tail_multi_equals_sum_of_view_tails ("old B", max norm 1e-5)
were run against it on an MI355X (first failing element of each test; the unchanged library passes all 18):
 1. cube_fetch_vjp: `vc` without `sgn_c` -- FAILS test_tail_multi_within_budget[pbr] (v_means, ratio 20 477) and [diffuse] (v_normals,
    879 537: the sign of the component flips); the other new tests do not run that function and pass.  Old A passes (does not run
    it), old B fails in all three modes (relative 0.11 / 1.7).
 2. cube_footprint: corner weight `/ 4.0f` -- FAILS every test_shade_bwd_within_budget case (corner texels, ratio 12 .. 290),
    test_shade_bwd_grid_stride (4.5), test_tail_bwd_within_budget (29 / 677) and test_tail_multi_within_budget (23 / 437).  Old A
    fails, in the specular modes only just (v_levels[1] 1.2e-4 against 1e-4; v_base 1.6e-2 in diffuse); old B passes (both of its
    sides share the footprint).
 3. shade_pair_post: no `p.clamped` test on v_mip -- FAILS test_tail_multi_within_budget[pbr]: a Gaussian of the 'r == 1 exactly'
    regime gets v_ks[0] = -0.236 where the gradient and its budget are exactly 0 (ratio inf).  Old A and old B pass.
 4. tex2d_linear_clamp2: `d_du` not zeroed under `cx` -- FAILS test_shade_bwd_within_budget in the pbr and specular cases (v_means,
    ratio 1 465 .. 33 239), test_shade_bwd_grid_stride (2 473), test_tail_bwd_within_budget[pbr] (838) and
    test_tail_multi_within_budget[pbr] (536); the diffuse cases do not use the LUT and pass.  Old A fails in pbr and specular
    (v_means 5.4e-2); old B passes (both of its sides share the lookup).
 5. shade_pair_post: `p.d >= 1e-6f` -> `> 0.0f` -- passes everything, with the 'tiny_d' regime (0 < d < 1e-6) in every scene.  The
    change cannot be observed: for such a d the forward clamps ndv to 1e-6, the LUT coordinate 1e-6 * 256 - 0.5 is below 0, `cx` holds
    and d_du is 0, so the v_ndv that the test gates is exactly 0 on both sides of it.  It would show only together with change 4.
 6. cube_scatter_wave_tagged: the second row pair with the first row's weights -- FAILS test_tail_bwd_within_budget[pbr] and
    test_tail_multi_within_budget[pbr] (a texel of the 64^2 level, got 0.088 for 0.0014, ratio 39 283 in both).  The diffuse cases keep
    their 16^2 base in LDS and gs_shade_bwd scatters through cube_scatter_wave: those pass.  Old A and old B pass (old B's two sides
    share the scatter).
Run with -s to print the ratios of every gradient.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import util
from tests import test_gpu_project_budget as PB

pytestmark = pytest.mark.gpu

NAMES = ("v_means", "v_normals", "v_kd", "v_ks", "texels")
CASES = [(nm, mode) for nm, spec in util.SHADE_BUDGET_SCENES.items() for mode in spec["modes"]]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module's tests: the worst ratio per entry point and gradient over whatever ran (shown with -s)"""
    yield
    print()
    for ep in sorted({k[0] for k in WORST}):
        print(f"    {ep:16s}" + "   ".join(f"{nm} {WORST.get((ep, nm), 0.0):6.2f}" for nm in NAMES))


@functools.lru_cache(maxsize=None)
def _scene(name, mode):
    sc = util.shade_budget_scene(name, mode, **util.SHADE_BUDGET_SCENES[name]["kw"])
    util.shade_scene_check(sc)                                       # asserts regimes and margins
    return sc


@functools.lru_cache(maxsize=None)
def _want(name, mode, kind, seed):
    sc = _scene(name, mode)
    cot = util.shade_budget_cotangents(kind, len(sc["regime"]), seed)
    want, bud = _oracle(sc, cot, pool=True)
    _, tb = oracle.shade_pool_texels([(want, bud)])
    pool = (bud["abs"], bud["n"])
    bud = dict(bud, v_levels=tb[:-1], v_base=tb[-1])
    return cot, (want, bud, pool)


def _oracle(sc, cot, cam_pos=None, pool=False):
    return oracle.shade_bwd_budget(sc["means"], sc["normals"], sc["kd"], sc["ks"], sc["cam_pos"] if cam_pos is None else cam_pos,
                                   sc["lut"], sc["base"], sc["levels"], cot, mode=sc["mode"], pool=pool, **sc["opts"])


def _texels(x):
    return list(x["v_levels"]) + [x["v_base"]]


def _env(cuda, sc):
    import geosplatting_amd as gs
    from geosplatting_amd.shading import _make_env
    t = lambda a: torch.tensor(a, device=cuda)
    o = sc["opts"]
    env = gs.TextureSplitSum(t(sc["base"]), [t(l) for l in sc["levels"]], o["env_min_roughness"], o["env_max_roughness"])
    lut = t(sc["lut"]).reshape(1, 256, 256, 2).contiguous()
    return env, lut, _make_env(lut, env)


def _texel_bufs(cuda, env, pattern=None):
    """texel-gradient buffers ([levels..., base] order) and the GsEnvGrad over them, zero or pre-filled with `pattern` arrays"""
    from geosplatting_amd import _lib as L
    shapes = [l.shape for l in env.levels] + [env.base.shape]
    bufs = [torch.zeros(s, device=cuda) if pattern is None else torch.tensor(p, device=cuda) for s, p in zip(shapes, pattern or shapes)]
    eg = L.GsEnvGrad(); eg.base = bufs[-1].data_ptr()
    for i, b in enumerate(bufs[:-1]):
        eg.levels[i] = b.data_ptr()
    return bufs, eg


def _record(label, nm, r):
    key = (label.split()[0], nm)
    WORST[key] = max(WORST.get(key, 0.0), r)


def _check_rows(label, got, want, bud, times=1.0, dead=None, extra=None):
    """the four per-Gaussian arrays against times * (want, budget) (+ `extra` budget); `dead` rows are exactly 0"""
    for i, nm in enumerate(NAMES[:4]):
        g = got[i].cpu().numpy()
        w = want[nm] if isinstance(want, dict) else want[i]
        b = bud[nm] if isinstance(bud, dict) else bud[i]
        assert np.isfinite(g).all(), (label, nm)
        if dead is not None:
            assert not g[dead].any() and not np.asarray(b)[dead].any(), (label, nm)
        b = times * np.asarray(b) + (0.0 if extra is None else extra[i])
        _record(label, nm, util.assert_within_budget(f"{label} {nm}", g, times * np.asarray(w, np.float64), b, util.SHADE_BUDGET_KAPPA))


# gs_shade_bwd and gs_tail_bwd form every texel contribution with the oracle's bits (contraction off), so one launch differs from the
# oracle only in the ORDER of a texel's n additions.  Any order rounds at most n - 1 times (n on top of a pattern), each time a partial
# sum no larger than |p| + sum |contribution|: either side lies within the element's budget of the exact sum, the two within twice
# the budget of each other.  Single launches of these entry points are therefore held to 2, not to kappa.
TEXEL_ORDER_BAR = 2.0


def _check_texels(label, got, want, bud, times=1.0, pattern=None, pool=None, bar=util.SHADE_BUDGET_KAPPA):
    """texel arrays against times * (want, budget), within `bar` budgets; with a pattern p (and pool = the oracle's per-element
    (sum |contribution|, n)): p + gradient, where each of the n additions may round a sum that holds p -- n |p| + sum |contribution|
    more -- and a texel no footprint touches keeps the pattern's bits"""
    assert bar <= util.SHADE_BUDGET_KAPPA
    for i, (g, w, b) in enumerate(zip(got, want, bud)):
        g = g.cpu().numpy(); w = times * np.asarray(w, np.float64); b = times * np.asarray(b)
        if times > 1.0:
            b = b + np.abs(w)                                       # the second launch adds onto the first launch's sum
        if pattern is not None:
            p = pattern[i]
            assert g[b == 0].view(np.int32).tobytes() == p[b == 0].view(np.int32).tobytes(), (label, i)
            b = np.where(b > 0, b + pool[1][i] * np.abs(p) + pool[0][i], 0.0)
            w = w + p
        _record(label, "texels", util.assert_within_budget(f"{label} texels[{i}]", g, w, b, bar))


def _pattern(sc, seed=9):
    r = np.random.RandomState(seed)
    return [r.uniform(-2, 2, a.shape).astype(np.float32) for a in list(sc["levels"]) + [sc["base"]]]


def _shade_bwd(cuda, sc, x, e, eg, cot_dev, outs, accumulate, priv):
    from geosplatting_amd import _lib as L
    from geosplatting_amd.shading import _MODE
    lib = L.lib()
    o = sc["opts"]
    M = _MODE[sc["mode"]]
    ws_bytes = lib.gs_shade_bwd_ws_bytes(C.byref(e), M) if priv else 0
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=cuda) if ws_bytes else None
    L.check(lib.gs_shade_bwd(x["means"].shape[0], L.ptr(x["means"]), L.ptr(x["normals"]), L.ptr(x["kd"]), L.ptr(x["ks"]), L.ptr(x["cam"]),
                             L.f32(o["min_roughness"]), L.f32(o["max_metallic"]), M, C.byref(e), L.ptr(cot_dev), L.ptr(outs[0]),
                             L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(outs[3]), C.byref(eg), accumulate, L.ptr(ws), C.c_size_t(ws_bytes),
                             L.stream()), "gs_shade_bwd")
    torch.cuda.synchronize()
    return ws_bytes


def _dev(cuda, sc):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda)
    return dict(means=t(sc["means"]), normals=t(sc["normals"]), kd=t(sc["kd"]), ks=t(sc["ks"]), cam=t(sc["cam_pos"]))


def _outs(cuda, N, fill):
    f = lambda *s: torch.full(s, fill, dtype=torch.float32, device=cuda)
    return [f(N, 3), f(N, 3), f(N, 3), f(N, 2)]


@pytest.mark.parametrize("scene,mode", CASES)
def test_shade_bwd_within_budget(cuda, scene, mode):
    """gs_shade_bwd: accumulate = 0 over garbage-filled outputs and pattern-filled texel buffers (every row written, dead rows exactly
    0, the texels pattern + gradient, untouched texels the pattern's bits), accumulate = 1 twice over zeros (twice the gradient within
    twice the budget), with and without the XCD-private workspace; and the forward's colours equal the oracle's bit for bit"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd.shading import _MODE
    sc = _scene(scene, mode)
    N = len(sc["regime"])
    x = _dev(cuda, sc)
    env, lut, e = _env(cuda, sc)
    o = sc["opts"]
    col = torch.empty(N, 3, device=cuda)
    L.check(L.lib().gs_shade_fwd(N, L.ptr(x["means"]), L.ptr(x["normals"]), L.ptr(x["kd"]), L.ptr(x["ks"]), L.ptr(x["cam"]),
                                 L.f32(o["min_roughness"]), L.f32(o["max_metallic"]), _MODE[mode], C.byref(e), L.ptr(col), L.stream()),
            "gs_shade_fwd")
    ref = oracle.shade_fwd(sc["means"], sc["normals"], sc["kd"], sc["ks"], sc["cam_pos"], sc["lut"], sc["base"], sc["levels"], mode=mode, **o)
    fwd_diff = np.abs(col.cpu().numpy().astype(np.float64) - ref).max()
    print(f"\n  forward {scene}/{mode}: max |diff| {fwd_diff:.3e}")
    assert col.cpu().numpy().view(np.int32).tobytes() == ref.view(np.int32).tobytes()      # the contraction-off forward IS the oracle's
    for kind in util.SHADE_COTANGENTS:
        cot, (want, bud, pool) = _want(scene, mode, kind, 3)
        dead = ~cot.any(1)
        cd = torch.tensor(cot, device=cuda)
        for priv in (False, True):
            tag = "priv" if priv else "plain"
            pat = _pattern(sc)
            tex, eg = _texel_bufs(cuda, env, pat)
            outs = _outs(cuda, N, 123.0)
            ws_bytes = _shade_bwd(cuda, sc, x, e, eg, cd, outs, 0, priv)
            if priv and not ws_bytes:
                continue                                             # no level beyond LDS: the same launch as without
            _check_rows(f"shade_{tag} {scene}/{mode}/{kind}", outs, want, bud, dead=dead)
            _check_texels(f"shade_{tag} {scene}/{mode}/{kind}", tex, _texels(want), _texels(bud), pattern=pat, pool=pool, bar=TEXEL_ORDER_BAR)
            tex, eg = _texel_bufs(cuda, env)
            outs = _outs(cuda, N, 0.0)
            _shade_bwd(cuda, sc, x, e, eg, cd, outs, 1, priv)
            _shade_bwd(cuda, sc, x, e, eg, cd, outs, 1, priv)
            _check_rows(f"shade_{tag}_acc {scene}/{mode}/{kind}", outs, want, bud, times=2.0, dead=dead)
            _check_texels(f"shade_{tag}_acc {scene}/{mode}/{kind}", tex, _texels(want), _texels(bud), times=2.0)


def test_shade_bwd_grid_stride(cuda):
    """N beyond what the persistent blocks of gs_shade_bwd cover in one trip: the library's own launch plan
    (gs_shade_bwd_plan_blocks) caps the blocks for the env3 environment, the env3 scene is tiled past blocks * threads, and the plan
    for that N is asserted to stride (n_iter = 2) -- every row and every texel within budget"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd.shading import _MODE
    sc0 = _scene("env3", "pbr")
    _, _, e0 = env_keep = _env(cuda, sc0)
    bt = C.c_int(0)
    cap = L.lib().gs_shade_bwd_plan_blocks(C.byref(e0), _MODE["pbr"], 2 ** 30, C.byref(bt)) * bt.value
    assert 0 < cap < 2 ** 20, cap                                    # the plan caps its blocks (and a tiled scene stays small)
    n0 = len(sc0["regime"])
    reps = cap // n0 + 2
    sc = dict(sc0)
    for k in ("means", "normals", "kd", "ks"):
        sc[k] = np.tile(sc0[k], (reps, 1))
    N = n0 * reps
    assert L.lib().gs_shade_bwd_plan_blocks(C.byref(e0), _MODE["pbr"], N, C.byref(bt)) * bt.value == cap and (N + cap - 1) // cap == 2
    cot = util.shade_budget_cotangents("dense", N, 5)
    want, bud = _oracle(sc, cot)
    x = _dev(cuda, sc)
    env, lut, e = _env(cuda, sc)
    tex, eg = _texel_bufs(cuda, env)
    outs = _outs(cuda, N, 123.0)
    _shade_bwd(cuda, sc, x, e, eg, torch.tensor(cot, device=cuda), outs, 0, False)
    _check_rows("shade_stride env3/pbr/dense", outs, want, bud, dead=~cot.any(1))
    _check_texels("shade_stride env3/pbr/dense", tex, _texels(want), _texels(bud), bar=TEXEL_ORDER_BAR)


# ----------------------------------------------------------------------------- the engine's tail kernels
@functools.lru_cache(maxsize=None)
def _tail_scene(mode):
    """shading inputs for the Gaussians of the projection scene 'orbit8' (culled Gaussians interleaved with visible ones): the
    direction regimes are built for the first camera, the selection margins hold for all eight"""
    ps, _ = PB._scene("orbit8")
    cams = []
    for vw in ps["views"]:
        R, t = vw["viewmat"][:3, :3].astype(np.float64), vw["viewmat"][:3, 3].astype(np.float64)
        cams.append((-R.T @ t).astype(np.float32))
    sc = util.shade_budget_scene("tail", mode, n_per=30, n_pile=100, seed=5, geometry=(ps["means"], cams))
    util.shade_scene_check(sc)
    return ps, sc, cams


def _grad_bufs(cuda, N, env, fill=0.0):
    z = lambda *s: torch.full(s, fill, dtype=torch.float32, device=cuda)
    t = dict(means=z(N, 3), quats=z(N, 4), scales=z(N, 3), opac=z(N), normals=z(N, 3), kd=z(N, 3), ks=z(N, 2))
    tex, eg = _texel_bufs(cuda, env)
    return t, tex, eg


def _view_cot(N, gids, kind, seed):
    """per-Gaussian colour cotangents of a view: zero for the Gaussians the view does not see"""
    cot = util.shade_budget_cotangents(kind, N, seed)
    eff = np.zeros_like(cot); eff[gids] = cot[gids]
    return eff


def _vpacked(cuda, gids, cot, st, rows, fill):
    V = len(gids)
    vp = np.full((rows, st), fill, np.float32)
    vp[:V] = 0.0
    vp[:V, 6:9] = cot[gids]
    return torch.tensor(vp, device=cuda)


@pytest.mark.parametrize("mode", ["pbr", "diffuse"])
def test_tail_bwd_within_budget(cuda, mode):
    """gs_tail_bwd, exact form and counts_dev form (capacity rows of v_packed hold NaN), with non-zero colour cotangents and zero
    geometry cotangents: v_normals / v_kd / v_ks and the texel gradients against the shading budget, v_means against the sum of the
    shading and projection oracles within the sum of both budgets; Gaussians the view culls are exactly 0"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd import front as F
    from geosplatting_amd.shading import _MODE
    lib = L.lib()
    ps, sc, cams = _tail_scene(mode)
    vw = ps["views"][0]
    N = len(sc["regime"])
    x = PB._dev(cuda, ps)
    sh = tuple(torch.tensor(sc[k], device=cuda) for k in ("normals", "kd", "ks"))
    env, lut, e = _env(cuda, sc)
    o = sc["opts"]
    fr, V, host, (vm, K, cam_pos) = PB._front(cuda, "orbit8", 0, x, sh, e, _MODE[mode])
    st = lib.gs_raster_grad_stride(3)
    zero_geo = (np.zeros((V, 2), np.float32), np.zeros((V, 3), np.float32), np.zeros(V, np.float32), None)
    pw, pb = PB._oracle(ps, vw, host, zero_geo)
    for kind in util.SHADE_COTANGENTS:
        cot = _view_cot(N, host["gids"], kind, 21)
        want, bud = _oracle(sc, cot, cam_pos=cams[0])
        want = dict(want); bud = dict(bud)
        want["v_means"] = want["v_means"].astype(np.float64) + pw[0]; bud["v_means"] = bud["v_means"] + pb[0]
        for form in ("exact", "counts"):
            vp = _vpacked(cuda, host["gids"], cot, st, V if form == "exact" else N, np.nan)
            t, tex, eg = _grad_bufs(cuda, N, env)
            F.tail_stage(V if form == "exact" else N, None if form == "exact" else fr.counts, x["means"], x["quats"], x["scales"], x["opac"],
                         sh[0], sh[1], sh[2], vm, K, cam_pos, e, eg, vw["W"], vw["H"], o["min_roughness"], o["max_metallic"], _MODE[mode],
                         fr.vis, vp, t["means"], t["quats"], t["scales"], t["opac"], t["normals"], t["kd"], t["ks"])
            torch.cuda.synchronize()
            label = f"tail_{form} {mode}/{kind}"
            _check_rows(label, [t["means"], t["normals"], t["kd"], t["ks"]], want, bud, dead=~cot.any(1))
            _check_texels(label, tex, _texels(want), _texels(bud), bar=TEXEL_ORDER_BAR)
            for k in ("quats", "scales", "opac"):
                assert not t[k].any(), (label, k)


@pytest.mark.parametrize("mode", ["pbr", "diffuse"])
def test_tail_multi_within_budget(cuda, mode):
    """gs_tail_bwd_multi / gs_tail_bwd_multi_parts (the lean pair path) over n = 1, 2, 3, 5, 8 cameras (every lanes-per-Gaussian
    variant), parts = 3, then 1 followed by 2, then background launches accumulated, with and without the XCD-private workspace
    folded by gs_tail_priv_reduce ('pbr' only: in 'diffuse' the 16^2 base lives in LDS, there is no private copy and the library hands
    out no workspace -- asserted): want = the sum over the views; budget = the sum of the per-view budgets + 3 * sum_v |g_v| for the
    group tree sum; a texel pools the contributions of all views under the (n - 1) rule"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd import front as F
    from geosplatting_amd.shading import _MODE
    lib = L.lib()
    ps, sc, cams = _tail_scene(mode)
    N = len(sc["regime"])
    x = PB._dev(cuda, ps)
    sh = tuple(torch.tensor(sc[k], device=cuda) for k in ("normals", "kd", "ks"))
    env, lut, e = _env(cuda, sc)
    o = sc["opts"]
    M = _MODE[mode]
    st = lib.gs_raster_grad_stride(3)
    views, per_view, seen = [], [], np.zeros(N, int)
    for vi, vw in enumerate(ps["views"]):
        fr, V, host, (vm, K, cam_pos) = PB._front(cuda, "orbit8", vi, x, sh, e, M)
        cot = _view_cot(N, host["gids"], util.SHADE_COTANGENTS[vi % 3], 60 + vi)
        vp = _vpacked(cuda, host["gids"], cot, st, V, 0.0)
        views.append((vm, K, cam_pos, fr.vis, vp, fr.packed_index, vw["W"], vw["H"]))
        per_view.append(_oracle(sc, cot, cam_pos=cams[vi], pool=True))
        seen[host["gids"]] += cot[host["gids"]].any(1)
    keys = ("v_means", "v_normals", "v_kd", "v_ks")

    def expect(idx):
        want = [sum(per_view[i][0][k].astype(np.float64) for i in idx) for k in keys]
        mag = [sum(np.abs(per_view[i][0][k].astype(np.float64)) for i in idx) for k in keys]
        bud = [sum(per_view[i][1][k] for i in idx) + 3.0 * m for k, m in zip(keys, mag)]
        return want, bud, oracle.shade_pool_texels([per_view[i] for i in idx])

    def multi(vs, t, eg, accumulate, parts, priv=None):
        F.tail_multi_stage(vs, x["means"], x["quats"], x["scales"], x["opac"], sh[0], sh[1], sh[2], e, eg, o["min_roughness"], o["max_metallic"],
                           M, t["means"], t["quats"], t["scales"], t["opac"], t["normals"], t["kd"], t["ks"], accumulate=accumulate,
                           parts=parts, priv=priv)

    def done(label, t, tex, idx):
        torch.cuda.synchronize()
        want, bud, (tw, tb) = expect(idx)
        seen_idx = np.zeros(N, bool)
        for i in idx:
            seen_idx |= np.abs(per_view[i][0]["v_kd"]).sum(1) + per_view[i][1]["v_kd"].sum(1) > 0
        _check_rows(label, [t["means"], t["normals"], t["kd"], t["ks"]], want, bud)
        for a in (t["normals"], t["kd"], t["ks"]):
            assert not a.cpu().numpy()[~seen_idx].any(), label
        _check_texels(label, tex, tw, tb)

    for use_priv in (False, True):
        tag = "multi_priv" if use_priv else "multi"
        for n in (1, 2, 3, 5, 8):
            priv = F.tail_priv_alloc(e, M, cuda) if use_priv else None
            if use_priv and priv is None:
                assert mode == "diffuse"                             # no level beyond LDS: nothing more to run
                return
            t, tex, eg = _grad_bufs(cuda, N, env, fill=123.0)
            multi(views[:n], t, eg, False, 3, priv)
            F.tail_priv_reduce(e, eg, M, priv)
            done(f"{tag} n={n} {mode}", t, tex, range(n))
        priv = F.tail_priv_alloc(e, M, cuda) if use_priv else None
        t, tex, eg = _grad_bufs(cuda, N, env, fill=123.0)
        multi(views, t, eg, False, 1, priv)
        multi(views, t, eg, False, 2, priv)
        F.tail_priv_reduce(e, eg, M, priv)
        done(f"{tag}_parts 1+2 {mode}", t, tex, range(8))
        priv = F.tail_priv_alloc(e, M, cuda) if use_priv else None
        t, tex, eg = _grad_bufs(cuda, N, env, fill=123.0)
        multi(views[:3], t, eg, False, 7, priv)
        multi(views[3:6], t, eg, True, 7, priv)
        multi(views[6:], t, eg, True, 3, priv)
        F.tail_priv_reduce(e, eg, M, priv)
        done(f"{tag}_bg 3+3+2 {mode}", t, tex, range(8))
