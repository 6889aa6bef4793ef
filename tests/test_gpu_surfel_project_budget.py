"""GPU: the surfel projection (gs_surfel_project_fwd / gs_surfel_project_bwd, csrc/gs_surfel.hip) and the SH colours both projections
inline (csrc/gs_sh_dev.h), ELEMENT BY ELEMENT against the float64 reference and running-error budgets of tests/surfel_project_ref.py:
|got - want| <= kappa * 2^-24 * budget for every element (kappa = util.SURFEL_PROJ_KAPPA; util.SH_KAPPA for SH colours and g_sh), a
budget of 0 meaning exactly `want`.  The C entries are called directly, so nothing downstream consumes a count a wrong kernel made;
every output is pre-filled with a NaN / sentinel pattern.

No element is excluded.  Two things are taken from the GPU instead of decided by the reference, both because no float32 evaluation
decides them: the normal's sign where |n . c| is within its bound of 0 (elsewhere it must equal the reference's), and a radius of
RADIUS_BIG pixels or more whose rounding-up the bound cannot decide (a surfel whose plane nearly contains the camera: radii of 1e3
to 1e6); such a radius is checked against 3 sqrt(ext) within its bound plus the 1 of the ceil, every other radius exactly.

gs_surfel_project_bwd takes ONE row length (`stride`) for all six incoming gradients, so "separate arrays" are six allocations of
[V, 9] with the gradient in the leading columns and NaN behind (its header speaks of "their own row length": one shared by all).

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X (both constants are 4; the budgets are rigorous running-error bounds, so a
correct kernel stays near or below 1 whatever the compiler contracts or approximates):
    gs_surfel_project_fwd, both cameras, depth_channel 0 / 1, every colour mode
        ray_transforms 0.70   means2d 0.30   depths 0.70   normals 0.36   undecided big radii 0.16   SH colours 1.00 (0.996)
    ... on the 131 372 jittered rows of the compaction scene
        ray_transforms 0.85   means2d 0.52   depths 0.85   normals 0.36   undecided big radii 0.21
    gs_surfel_project_bwd, plain colours, Cn = 1 / 3 / 4, packed and separate gradients, every cotangent kind
        g_means 0.50   g_quats 0.30   g_scales 0.28   g_opacities, g_colors 0 (copies)
    gs_surfel_project_bwd, SH degrees 0..3 in the five coefficient layouts
        g_means 0.55 (direction term alone 0.27)   g_quats 0.34   g_scales 0.28   g_sh 0.93
    gs_project_fwd_vis_ex / gs_project_bwd_ex with SH, flags 0
        colours 0.99   g_sh_coeffs 0.93   v_means 0.64   v_quats 0.07   v_scales 0.20   v_opacities 0.00
    ... GS_PROJ_CLASSIC
        colours 0.99   g_sh_coeffs 0.93   v_means 0.54   v_quats 0.06   v_scales 0.15   v_opacities 0.00
    rasterization_2dgs, loss on the depth channel, gradients of the leaves against the recorded v_packed
        g_means 0.47   g_quats 0.21   g_scales 0.25
The compaction itself (ids, counts, untouched rows, prefixes bit for bit) is exact at every size; no test of this module exposed a
defect in a kernel or in the wrapper.

The tests bite.  Each change below (arithmetic only: no address, index, loop bound or launch size) was built into a scratch copy
of the library, never committed, and run once on the MI355X against this module ("new") and against tests/test_gpu_surfels.py
("old", the 1e-4 max-norm tests).  First failing element of "new", its ratio, and what "old" did:
    1. `t = j == 2 ? -f : f` -> `f` (means2d block)        bwd g_means[659, 1] got -136.2 want 44.7, ratio 1.6e6; 16 tests fail.
                                                           old: 26 of 30 fail (means 3.2e-2)
    2. vRc[.., 2] = v_normals without `sgn`                bwd g_quats[70, 1] got -2.2518 want 2.2504, ratio 1.8e6; 14 fail.
                                                           old: 26 fail (quats 0.53)
    3. g_quats without the `dotp * qn[k]` projection       bwd g_quats[1394, 0] got 0.0575 want -0.879, ratio 4.4e5; 16 fail.
                                                           old: 26 fail (quats 0.98)
    4. vH row 2 without the `cam.cy * vM1[j]` term         bwd g_means[301, 2] got 11.70 want -57.70, ratio 2.2e6; 16 fail.
                                                           old: 26 fail (means 0.26, quats 0.39)
    5. the clamp rule of sh_color_bwd_row dropped          bwd_sh g_sh[0, 0, 0] got 0.2039 want 0 (budget 0: ratio inf), then
                                                           g_means[825, 1] ratio 3.7e4; all 8 surfel SH tests and all 8 of the 3DGS
                                                           entry fail.  old: 10 fail (means 9.4e-3; degree 2 only)
    6. `- F * 2.f * y * z * vb[14]` -> `+` (degree 3)      bwd_sh g_means[953, 1] got -10.01 want -7.34, ratio 4.0e4; the four degree-3
                                                           tests (two surfel, two 3DGS) fail and nothing else.
                                                           old: PASSES, all 30 -- it never runs degree 3
    7. surfels.py: `_off(v_packed, 15 + Cn - 1)` -> `15 + Cn`   wrapper g_means[192, 2] got 1.0035 want -3.4500, ratio 3.1e6
                                                           (test_wrapper_routes_packed_columns, both modes; the C-entry tests
                                                           cannot see the wrapper and pass).  old: 23 of 61 fail (means 2.5e-2;
                                                           tests/test_gpu_surfel_budget.py, which stops at the compositor, passes)
Every change is detected; 6 is the one the suite could not see before.  Run with -s to print the ratios of every output.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import surfel_project_ref as R
from tests import util

pytestmark = pytest.mark.gpu

WORST = {}
F_PAT, I_PAT = 0x7FC0BEEF, -0x5EADBEE          # a quiet NaN with a payload; a negative id / radius / tile count
THR = 2 * R.MARGIN_KAPPA


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print()
    for ep in sorted({k[0] for k in WORST}):
        print(f"    {ep:22s}" + "   ".join(f"{k[1]} {v:5.2f}" for k, v in sorted(WORST.items()) if k[0] == ep))


def _sf_block():
    """SF_BLOCK, read from the source the library was built from"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geosplatting_amd", "csrc", "gs_surfel.hip")).read()
    block = int(re.search(r"^#define SF_BLOCK (\d+)", src, re.M).group(1))
    assert block % 64 == 0
    return block


SF_BLOCK = _sf_block()

# on the reference alone, at import: every regime of both scenes and every clamp pattern of every degree holds at least 20 rows, so a
# later change of a constant cannot silently stop covering one
for _ci in (0, 1):
    R.assert_regimes(R.budget_scene(_ci))
    for _deg in range(4):
        R.assert_clamp_patterns(R.sh_inputs(_ci, _deg)[1], R.budget_scene(_ci)["fwd"]["valid"])


def _check(ep, name, got, want, bud, kappa=None):
    kappa = (util.SH_KAPPA if name in ("sh_colors", "g_sh") else util.SURFEL_PROJ_KAPPA) if kappa is None else kappa
    r = util.assert_within_budget(f"{ep} {name}", got, want, bud, kappa)
    WORST[(ep, name)] = max(WORST.get((ep, name), 0.0), r)


def _pat(cuda, shape, dtype):
    t = torch.full(shape, F_PAT if dtype == torch.float32 else I_PAT, dtype=torch.int32, device=cuda)
    return t.view(torch.float32) if dtype == torch.float32 else t


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dev(cuda, *arrays):
    return [None if a is None else torch.tensor(np.ascontiguousarray(a), device=cuda) for a in arrays]


def _forward(cuda, x, N, cam, Dc, colors, sh, depth_channel):
    """gs_surfel_project_fwd on the first N rows of the device tensors x over patterned outputs: dict of host arrays (whole capacity
    rows) and V, I.  sh: None or (degree, device coefficients [>= N, K, 3], K)."""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    f32, i32 = torch.float32, torch.int32
    Cn = Dc + depth_channel
    cap = max(N, 1)
    o = dict(gaussian_ids=_pat(cuda, (cap,), i32), radii=_pat(cuda, (cap,), i32), means2d=_pat(cuda, (cap, 2), f32),
             depths=_pat(cuda, (cap,), f32), ray_transforms=_pat(cuda, (cap, 9), f32), normals=_pat(cuda, (cap, 3), f32),
             opacities=_pat(cuda, (cap,), f32), colors=_pat(cuda, (cap, Cn), f32), tiles=_pat(cuda, (cap,), i32))
    ws_bytes = lib.gs_surfel_project_ws_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    counts = torch.full((2,), -7, dtype=torch.int64, device=cuda)
    vm, K = _dev(cuda, cam["viewmat"], cam["K"])
    L.check(lib.gs_surfel_project_fwd(N, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opacities"]),
                                      None if sh else L.ptr(colors), Dc, L.ptr(sh[1]) if sh else None, sh[2] if sh else 0,
                                      sh[0] if sh else -1, depth_channel, L.ptr(vm), L.ptr(K), cam["W"], cam["H"], R.TILE,
                                      L.f32(cam["near"]), L.f32(cam["far"]), L.f32(cam["radius_clip"]), L.ptr(o["gaussian_ids"]),
                                      L.ptr(o["radii"]), L.ptr(o["means2d"]), L.ptr(o["depths"]), L.ptr(o["ray_transforms"]),
                                      L.ptr(o["normals"]), L.ptr(o["opacities"]), L.ptr(o["colors"]), L.ptr(o["tiles"]), L.ptr(ws),
                                      ws_bytes, L.ptr(counts), L.stream()), "gs_surfel_project_fwd")
    torch.cuda.synchronize()
    V, I = (int(c) for c in counts.tolist())
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out.update(V=V, I=I)
    return out


def _untouched(out, V):
    for k, a in out.items():
        if isinstance(a, np.ndarray):
            assert (_bits(a[V:]) == (I_PAT if a.dtype == np.int32 else F_PAT)).all(), f"rows >= V of {k} were written"


@functools.lru_cache(maxsize=None)
def _scene_dev(ci):
    sc = R.budget_scene(ci)
    R.assert_regimes(sc)                                                  # on the reference alone
    return sc


def _x(cuda, sc):
    m, q, s, o = _dev(cuda, sc["means"], sc["quats"], sc["scales"], sc["opacities"])
    return dict(means=m, quats=q, scales=s, opacities=o)


def _stored_sign(sc, out, gids):
    """the sign the forward stored with each normal (+1: Rc[:, 2] as it is), checked against the reference's where that is decided"""
    fwd = sc["fwd"]
    sgn = np.where((out["normals"][:len(gids)].astype(np.float64) * fwd["normal"][gids]).sum(-1) < 0, -1.0, 1.0)
    decided = fwd["margins"]["sign"][gids] >= THR
    assert np.array_equal(sgn[decided], np.where(fwd["dot"][gids] > 0, -1.0, 1.0)[decided])
    return sgn


def _check_forward(ep, sc, out, N=None):
    """everything of a forward run that does not depend on the colours; returns (gids, stored sign)"""
    fwd = sc["fwd"]
    N = len(sc["means"]) if N is None else N
    gids = np.nonzero(fwd["valid"][:N])[0]
    V = len(gids)
    assert out["V"] == V and out["I"] == int(fwd["tiles"][gids].sum())
    assert np.array_equal(out["gaussian_ids"][:V], gids)
    exact = fwd["radius_exact"][gids]
    assert np.array_equal(out["radii"][:V][exact], fwd["radii"][gids][exact])
    # an undecided big radius: ceil(3 sqrt(ext)) lies within 1 of 3 sqrt(ext); what is left of the difference is 3 sqrt(ext)'s own error
    pre, big = fwd["pre"][gids][~exact], out["radii"][:V][~exact].astype(np.float64)
    _check(ep, "radii_big", pre + np.sign(big - pre) * np.maximum(np.abs(big - pre) - 1.0, 0.0), pre, fwd["pre_e"][gids][~exact])
    assert np.array_equal(out["tiles"][:V], fwd["tiles"][gids])
    assert _bits(out["opacities"][:V]).tobytes() == _bits(sc["opacities"][gids]).tobytes()
    _check(ep, "ray_transforms", out["ray_transforms"][:V], fwd["M"][gids], fwd["M_e"][gids])
    _check(ep, "means2d", out["means2d"][:V], fwd["means2d"][gids], fwd["means2d_e"][gids])
    _check(ep, "depths", out["depths"][:V], fwd["depths"][gids], fwd["depths_e"][gids])
    sgn = _stored_sign(sc, out, gids)
    _check(ep, "normals", out["normals"][:V], sgn[:, None] * fwd["normal"][gids], fwd["normal_e"][gids])
    _untouched(out, V)
    return gids, sgn


def _sh_layouts(deg):
    nb = (deg + 1) ** 2
    return [nb] if nb == 16 else [nb, 16]


@pytest.mark.parametrize("depth_channel", [0, 1])
@pytest.mark.parametrize("ci", [0, 1])
def test_forward_per_element(cuda, ci, depth_channel):
    sc = _scene_dev(ci)
    cam, N = sc["cam"], len(sc["means"])
    x = _x(cuda, sc)
    rs = np.random.RandomState(5 + ci)
    for Dc in ((1, 3, 4) if depth_channel == 0 else (0, 1, 3)):
        colors = rs.uniform(-1, 1, (N, Dc)).astype(np.float32)
        out = _forward(cuda, x, N, cam, Dc, _dev(cuda, colors)[0] if Dc else None, None, depth_channel)
        gids, _ = _check_forward("fwd", sc, out)
        V = len(gids)
        assert _bits(out["colors"][:V, :Dc]).tobytes() == _bits(colors[gids]).tobytes()
        if depth_channel:
            assert _bits(out["colors"][:V, Dc]).tobytes() == _bits(out["depths"][:V]).tobytes()
    for deg in range(4):
        co, shf = R.sh_inputs(ci, deg)
        R.assert_clamp_patterns(shf, sc["fwd"]["valid"])
        for Kc in _sh_layouts(deg):
            cd = _dev(cuda, co[:, :Kc])[0]
            out = _forward(cuda, x, N, cam, 3, None, (deg, cd, Kc), depth_channel)
            gids, _ = _check_forward("fwd_sh", sc, out)
            V = len(gids)
            _check("fwd_sh", "sh_colors", out["colors"][:V, :3], shf["rgb"][gids], shf["rgb_e"][gids])
            assert not out["colors"][:V, :3][shf["clamped"][gids]].any()
            if depth_channel:
                assert _bits(out["colors"][:V, 3]).tobytes() == _bits(out["depths"][:V]).tobytes()
            if Kc == 16:                                                 # the scalar-load route: a base pointer one float into a buffer
                buf = torch.zeros(N * 48 + 8, dtype=torch.float32, device=cuda)
                view = buf[1:1 + N * 48].view(N, 16, 3)
                view.copy_(cd)
                assert view.data_ptr() % 16 == 4
                out2 = _forward(cuda, x, N, cam, 3, None, (deg, view, 16), depth_channel)
                assert _bits(out2["colors"]).tobytes() == _bits(out["colors"]).tobytes()


# ----------------------------------------------------------------------------- compaction
BIG_N = 2 * 65536 + 300
PREFIXES = (1, 63, 64, 65, 255, 256, 257, 65536, 65537, BIG_N)


@functools.lru_cache(maxsize=None)
def _big_scene(first_last_kept):
    """the budget scene of camera 0 tiled to BIG_N rows with jittered means, rebuilt until every row is decided; one run of SF_BLOCK
    culled rows aligned to a block, one of 64 aligned to a wave, one fully visible block; the first and the last row culled or kept"""
    base = R.budget_scene(0)
    cam = base["cam"]
    r = np.random.RandomState(77)
    n0 = len(base["means"])
    src = np.arange(BIG_N) % n0
    vis_rows, cul_rows = np.nonzero(base["fwd"]["valid"])[0], np.nonzero(~base["fwd"]["valid"])[0]
    plain = np.nonzero(base["fwd"]["valid"] & (base["regime"] == R.REGIMES.index("plain")))[0]
    blk = SF_BLOCK
    b0, b1, w0 = 37 * blk, 211 * blk, 90 * blk + 128                       # culled block, visible block, culled wave
    src[b0:b0 + blk] = cul_rows[np.arange(blk) % len(cul_rows)]
    src[w0:w0 + 64] = cul_rows[np.arange(64) % len(cul_rows)]
    src[b1:b1 + blk] = plain[np.arange(blk) % len(plain)]
    ends = plain[:2] if first_last_kept else cul_rows[:2]
    src[0], src[-1] = ends
    means = base["means"][src].copy()
    fixed = np.zeros(BIG_N, bool)
    fixed[:n0] = True                                                      # the first copy is the scene itself
    jit = lambda k: (1.0 + 2e-3 * r.uniform(-1, 1, (k, 3))).astype(np.float32)
    todo = ~fixed
    for attempt in range(5):
        trial = means.copy()
        trial[todo] = base["means"][src[todo]] * jit(int(todo.sum()))
        fwd = R.project_fwd_budget(trial, base["quats"][src], base["scales"][src], cam["viewmat"], cam["K"], cam["W"], cam["H"],
                                   cam["near"], cam["far"], cam["radius_clip"], check=False)
        same_fate = fwd["valid"] == base["fwd"]["valid"][src]
        good = todo & (fwd["margin"] >= THR) & same_fate
        means[good] = trial[good]
        todo &= ~good
        if attempt >= 3:                                                   # what is left keeps the mean of its source row
            means[todo] = base["means"][src[todo]]
            todo[:] = False
        if not todo.any():
            break
    sc = dict(means=means, quats=base["quats"][src].copy(), scales=base["scales"][src].copy(), opacities=base["opacities"][src].copy(),
              cam=cam, src=src)
    sc["fwd"] = R.project_fwd_budget(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], cam["W"], cam["H"], cam["near"],
                                     cam["far"], cam["radius_clip"], check=False)
    v = sc["fwd"]["valid"]
    assert (sc["fwd"]["margin"] >= THR).all()
    assert 0.15 < 1.0 - v.mean() < 0.3 and int((~v[:-1] & v[1:]).sum()) > 5000      # culled rows interleaved
    assert not v[b0:b0 + blk].any() and not v[w0:w0 + 64].any() and v[b1:b1 + blk].all()
    assert v[0] == v[-1] == first_last_kept
    return sc


@pytest.mark.parametrize("first_last_kept", [False, True])
def test_compaction_exact(cuda, first_last_kept):
    """every prefix of one scene of 2 * 65 536 + 300 rows: surfel_scan_kernel with per = 1, 2 and 3 block totals per thread and a ragged
    last thread.  The per-Gaussian arithmetic does not depend on N, so the outputs of the prefix n are, bit for bit, the largest run's
    restricted to ids < n"""
    sc = _big_scene(first_last_kept)
    cam, fwd = sc["cam"], sc["fwd"]
    per = lambda n: -(-(-(-n // SF_BLOCK)) // SF_BLOCK)
    assert sorted({per(n) for n in PREFIXES}) == [1, 2, 3] and (-(-BIG_N // SF_BLOCK)) % per(BIG_N) != 0
    x = _x(cuda, sc)
    colors = np.random.RandomState(3).uniform(-1, 1, (BIG_N, 3)).astype(np.float32)
    cd = _dev(cuda, colors)[0]
    big = _forward(cuda, x, BIG_N, cam, 3, cd, None, 1)
    gids, _ = _check_forward("fwd_big", sc, big)
    assert (np.diff(big["gaussian_ids"][:big["V"]]) > 0).all()
    for n in PREFIXES[:-1]:
        out = _forward(cuda, x, n, cam, 3, cd, None, 1)
        Vn = int(np.searchsorted(gids, n))
        assert out["V"] == Vn == int(fwd["valid"][:n].sum()) and out["I"] == int(fwd["tiles"][gids[:Vn]].sum()), n
        for k, a in out.items():
            if isinstance(a, np.ndarray):
                assert _bits(a[:Vn]).tobytes() == _bits(big[k][:Vn]).tobytes(), (n, k)
        _untouched(out, Vn)


def test_compaction_empty(cuda):
    """N = 0 returns counts {0, 0}; 300 rows all culled give V = 0 and leave every output untouched"""
    base = R.budget_scene(0)
    cul = np.nonzero(~base["fwd"]["valid"])[0]
    rows = cul[np.arange(300) % len(cul)]
    sc = {k: base[k][rows] for k in ("means", "quats", "scales", "opacities")}
    x = _x(cuda, sc)
    colors = _dev(cuda, np.zeros((300, 3), np.float32))[0]
    out = _forward(cuda, x, 300, base["cam"], 3, colors, None, 0)
    assert (out["V"], out["I"]) == (0, 0)
    _untouched(out, 0)
    out = _forward(cuda, x, 0, base["cam"], 3, colors, None, 0)
    assert (out["V"], out["I"]) == (0, 0)
    _untouched(out, 0)


# ----------------------------------------------------------------------------- backward
COLS = dict(v_ray_transforms=0, v_means2d=9, v_normals=12, v_opacities=11, v_colors=15)


def _backward(cuda, x, N, cam, gids_dev, V, cot, Dc, depth_channel, layout, sh=None, g_sh_view=None):
    """gs_surfel_project_bwd over garbage outputs.  layout 'packed': columns of one [V, gs_surfel_grad_stride()] matrix at the wrapper's
    offsets, NaN in every other column; 'separate': six arrays of row length 9.  sh: (degree, device coefficients, K);
    g_sh_view: the output tensor for g_sh (a view of a larger buffer), else a fresh one.  Returns host arrays."""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    Cn = Dc + depth_channel
    cols = dict(COLS, v_depths=15 + Cn - 1)
    width = dict(v_ray_transforms=9, v_means2d=2, v_depths=1, v_normals=3, v_opacities=1, v_colors=Dc)
    names = ("v_ray_transforms", "v_means2d", "v_depths", "v_normals", "v_opacities", "v_colors")
    as2d = lambda a: a.reshape(V, -1)
    if layout == "packed":
        stride = lib.gs_surfel_grad_stride()
        assert stride >= 15 + Cn
        m = np.full((V, stride), np.nan, np.float32)
        for k in names:
            if cot[k] is not None and width[k]:
                m[:, cols[k]:cols[k] + width[k]] = as2d(cot[k])
        md = _dev(cuda, m)[0]
        ptrs = {k: (None if cot[k] is None else torch_ptr(md, cols[k])) for k in names}
        hold = [md]
    else:
        stride, hold, ptrs = 9, [], {}
        for k in names:
            if cot[k] is None:
                ptrs[k] = None
                continue
            m = np.full((V, stride), np.nan, np.float32)
            if width[k]:
                m[:, :width[k]] = as2d(cot[k])
            hold.append(_dev(cuda, m)[0])
            ptrs[k] = torch_ptr(hold[-1], 0)
    g = lambda *s: torch.full(s, 123.0, dtype=torch.float32, device=cuda)
    o = dict(g_means=g(N, 3), g_quats=g(N, 4), g_scales=g(N, 3), g_opacities=g(N))
    if sh:
        o["g_sh"] = g(N, sh[2], 3) if g_sh_view is None else g_sh_view
    else:
        o["g_colors"] = g(N, max(Dc, 1))
    L.check(lib.gs_surfel_project_bwd(N, V, Dc, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(sh[1]) if sh else None,
                                      sh[2] if sh else 0, sh[0] if sh else -1, *_dev_cam(cuda, cam), L.ptr(gids_dev), ptrs["v_ray_transforms"],
                                      ptrs["v_means2d"], ptrs["v_depths"], ptrs["v_normals"], ptrs["v_opacities"], ptrs["v_colors"], stride,
                                      L.ptr(o["g_means"]), L.ptr(o["g_quats"]), L.ptr(o["g_scales"]), L.ptr(o["g_opacities"]),
                                      None if sh else L.ptr(o["g_colors"]), L.ptr(o["g_sh"]) if sh else None, L.stream()),
            "gs_surfel_project_bwd")
    torch.cuda.synchronize()
    del hold
    return {k: v.cpu().numpy() for k, v in o.items()}


def torch_ptr(t, col):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * col)


_CAM_DEV = {}


def _dev_cam(cuda, cam):
    from geosplatting_amd import _lib as L
    key = id(cam)
    if key not in _CAM_DEV:
        _CAM_DEV[key] = _dev(cuda, cam["viewmat"], cam["K"])
    return [L.ptr(t) for t in _CAM_DEV[key]]


def _check_backward(ep, ref, got, N, gids, kind, sh_clamped=None, deg=None):
    dead = np.ones(N, bool); dead[gids] = False
    if kind == "rows0":
        dead[gids[3::7]] = True
    for name in ("g_means", "g_quats", "g_scales", "g_opacities") + (("g_sh",) if "g_sh" in got else ("g_colors",)):
        want, bud = ref[name]
        g = got[name]
        if name == "g_colors" and want.shape[1] == 0:
            continue
        assert not g[dead].any(), (ep, name, "dead rows")
        _check(ep, name, g.reshape(want.shape), want, bud)
    assert not got["g_scales"][:, 2].any()
    assert _bits(got["g_opacities"]).tobytes() == _bits(ref["g_opacities"][0].astype(np.float32)).tobytes()
    if "g_colors" in got and ref["g_colors"][0].shape[1]:
        assert _bits(got["g_colors"]).tobytes() == _bits(ref["g_colors"][0].astype(np.float32)).tobytes()
    if kind == "only_v_depths":
        assert not got["g_quats"].any() and not got["g_scales"].any()
    if kind == "only_v_opacities":
        assert not got["g_means"].any() and not got["g_quats"].any() and not got["g_scales"].any()
    if "g_sh" in got:
        assert not got["g_sh"][:, (deg + 1) ** 2:].any()
        assert not got["g_sh"][gids][:, :(deg + 1) ** 2][np.broadcast_to(sh_clamped[:, None, :], (len(gids), (deg + 1) ** 2, 3))].any()


@functools.lru_cache(maxsize=None)
def _fwd_state(ci):
    """V, gaussian_ids and the normal's sign from the GPU forward of the scene (plain colours; the colours do not enter them)"""
    cuda = torch.device("cuda:0")
    sc = _scene_dev(ci)
    x = _x(cuda, sc)
    N = len(sc["means"])
    out = _forward(cuda, x, N, sc["cam"], 1, _dev(cuda, np.zeros((N, 1), np.float32))[0], None, 0)
    gids, sgn = _check_forward("fwd", sc, out)
    return x, gids, sgn, _dev(cuda, gids.astype(np.int32))[0]


@pytest.mark.parametrize("Dc,depth_channel", [(0, 1), (3, 0), (3, 1)])
@pytest.mark.parametrize("ci", [0, 1])
def test_backward_per_element(cuda, ci, Dc, depth_channel):
    """plain colours, Cn = 1, 3 and 4 composited channels (v_depths NULL without a depth channel), every cotangent kind, both layouts"""
    sc = _scene_dev(ci)
    cam, N = sc["cam"], len(sc["means"])
    x, gids, sgn, gd = _fwd_state(ci)
    V = len(gids)
    for i, kind in enumerate(R.COTANGENTS):
        if kind == "only_v_depths" and not depth_channel or kind == "only_v_colors" and not Dc:
            continue
        cot = R.cotangents(kind, V, Dc, seed=100 * ci + 10 * Dc + i, with_depth=bool(depth_channel))
        ref = R.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], gids, sgn, cot, check=False)
        for layout in ("packed", "separate"):
            got = _backward(cuda, x, N, cam, gd, V, cot, Dc, depth_channel, layout)
            _check_backward("bwd", ref, got, N, gids, kind)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("ci", [0, 1])
def test_backward_sh_per_element(cuda, ci, deg):
    """SH colours in four layouts: K = (deg+1)^2; K = 16; K = 4 (degrees 0 and 1); K = 16 from a base pointer one float into a larger
    buffer, for sh_coeffs and for g_sh in turn (sh_row_vec false on the forward side, then on the backward side)"""
    sc = _scene_dev(ci)
    cam, N = sc["cam"], len(sc["means"])
    x, gids, sgn, gd = _fwd_state(ci)
    V = len(gids)
    co, shf = R.sh_inputs(ci, deg)
    nb = (deg + 1) ** 2
    clamped = shf["clamped"][gids]
    layouts = [("K=nb", nb, 1), ("K=16", 16, 0)] + ([("K=4", 4, 0)] if deg <= 1 and nb != 4 else []) + [("co+1", 16, 0), ("g+1", 16, 0)]
    for i, kind in enumerate(R.COTANGENTS):
        refs = {}
        for label, Kc, dc in layouts:
            if kind == "only_v_depths" and not dc:
                continue
            if dc not in refs:
                cot = R.cotangents(kind, V, 3, seed=300 * ci + 20 * deg + i, with_depth=bool(dc))
                refs[dc] = (cot, R.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], gids, sgn, cot,
                                                      sh=(deg, co[:, :16]), check=False))
            cot, ref = refs[dc]
            ref = dict(ref, g_sh=(ref["g_sh"][0][:, :Kc], ref["g_sh"][1][:, :Kc]))
            ch = np.ascontiguousarray(co[:, :Kc])
            if label == "co+1":
                buf = torch.zeros(N * Kc * 3 + 8, dtype=torch.float32, device=cuda)
                cd = buf[1:1 + N * Kc * 3].view(N, Kc, 3)
                cd.copy_(torch.tensor(ch))
                assert cd.data_ptr() % 16 == 4 and cd.is_contiguous()
            else:
                cd = _dev(cuda, ch)[0]
            gv = None
            if label == "g+1":
                gbuf = torch.full((N * Kc * 3 + 8,), 123.0, dtype=torch.float32, device=cuda)
                gv = gbuf[1:1 + N * Kc * 3].view(N, Kc, 3)
                assert gv.data_ptr() % 16 == 4
            got = _backward(cuda, x, N, cam, gd, V, cot, 3, dc, "packed" if i % 2 == 0 else "separate", sh=(deg, cd, Kc), g_sh_view=gv)
            if gv is not None:
                edge = gbuf.cpu().numpy()
                assert (edge[:1] == 123.0).all() and (edge[1 + N * Kc * 3:] == 123.0).all()       # nothing outside the view
            _check_backward("bwd_sh", ref, got, N, gids, kind, clamped, deg)
            # g_means is the projection term plus the SH direction term: the direction term alone, within the sum of both budgets
            if kind == "only_v_colors":
                dv, de = ref["g_means_dir"]
                _check("bwd_sh", "g_means_dir", got["g_means"], dv, ref["g_means"][1])


# ----------------------------------------------------------------------------- the 3DGS entry with SH
@pytest.mark.parametrize("classic", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_3dgs_entry_sh(cuda, deg, classic):
    """gs_project_fwd_vis_ex / gs_project_bwd_ex on the 'yaw' scene of util.PROJ_BUDGET_SCENES with SH colours, flags 0 and
    GS_PROJ_CLASSIC, K = (deg+1)^2 and 16: colours and g_sh_coeffs per element against the SH budget (g_sh fully written with
    accumulate = 1 too), culled rows exactly 0, v_means against oracle.project_bwd_budget plus the SH direction term within the sum
    of both budgets, v_quats / v_scales / v_opacities within the projection budget alone"""
    import importlib
    import oracle
    from geosplatting_amd import _lib as L
    Rz = importlib.import_module("geosplatting_amd.rasterization")
    lib = L.lib()
    sc = R._yaw_scene()
    fwd = util.proj_scene_forward(sc, 0)
    vw = sc["views"][0]
    N = len(sc["means"])
    co, shf = R.sh_inputs(0, deg, scene="yaw")
    nb = (deg + 1) ** 2
    x = dict(zip(("means", "quats", "scales", "opac"), _dev(cuda, sc["means"], sc["quats"], sc["scales"], sc["opacities"])))
    vm, K = _dev(cuda, vw["viewmat"], vw["K"])
    st = lib.gs_raster_grad_stride(3)
    for Kc in _sh_layouts(deg):
        cd = _dev(cuda, co[:, :Kc])[0]
        pr = Rz._project_stage(x["means"], x["quats"], x["scales"], x["opac"], cd, vm, K, vw["W"], vw["H"], 16, 0.3, util.PROJ_NEAR, 1e10,
                               sc["radius_clip"], sh_degree=deg, classic=classic)
        torch.cuda.synchronize()
        V = int(pr.host_counts[0])
        gids_d, conics, comps, colors_p = pr.bufs[0], pr.bufs[4], pr.bufs[5], pr.bufs[7]
        gids = gids_d[:V].cpu().numpy()
        assert np.array_equal(gids, fwd["gaussian_ids"])
        assert R.assert_clamp_patterns(shf, np.isin(np.arange(N), gids)) is not None
        ep = "3dgs_classic" if classic else "3dgs"
        rgb = colors_p[:V].cpu().numpy()
        _check(ep, "sh_colors", rgb, shf["rgb"][gids], shf["rgb_e"][gids])
        assert not rgb[shf["clamped"][gids]].any()
        host = dict(gids=gids, conics=conics[:V].cpu().numpy(), comps=comps[:V].cpu().numpy())
        for i, kind in enumerate(("dense", "depth")):
            cotp = util.proj_budget_cotangents(kind, V, seed=50 + i)
            vcol = R.cotangents("rows0" if i else "decades", V, 3, seed=60 + deg)["v_colors"]
            vcol[3::7] = 0.0
            vp = np.zeros((V, st), np.float32)
            vp[:, 0:2], vp[:, 2:5], vp[:, 5], vp[:, 6:9] = cotp[0], cotp[1], cotp[2], vcol
            vpd, vd = _dev(cuda, vp, cotp[3])
            want, bud = oracle.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], sc["opacities"], vw["viewmat"], vw["K"], vw["W"],
                                                  vw["H"], gids, host["conics"], host["comps"], cotp[0], cotp[1], cotp[2], v_depths=cotp[3],
                                                  classic=classic)
            # the SH half alone: the surfel reference's SH chain with every other cotangent zero
            zc = dict(v_ray_transforms=np.zeros((V, 9), np.float32), v_means2d=np.zeros((V, 2), np.float32), v_depths=None,
                      v_normals=np.zeros((V, 3), np.float32), v_opacities=np.zeros(V, np.float32), v_colors=vcol)
            shref = R.project_bwd_budget(sc["means"], np.tile(np.float32([1, 0, 0, 0]), (N, 1)), np.ones((N, 3), np.float32), vw["viewmat"],
                                         vw["K"], gids, np.ones(V), zc, sh=(deg, co[:, :Kc]), check=False)
            dead = np.ones(N, bool); dead[gids] = False
            for acc in (0, 1):
                f = lambda *s: torch.full(s, 0.0 if acc else 123.0, dtype=torch.float32, device=cuda)
                o = [f(N, 3), f(N, 4), f(N, 3), f(N)]
                g_sh = _pat(cuda, (N, Kc, 3), torch.float32)
                L.check(lib.gs_project_bwd_ex(N, V, 3, L.ptr(x["means"]), L.ptr(x["quats"]), L.ptr(x["scales"]), L.ptr(x["opac"]), L.ptr(vm),
                                              L.ptr(K), vw["W"], vw["H"], L.f32(0.3), L.ptr(gids_d), L.ptr(conics), L.ptr(comps), L.ptr(vpd),
                                              st, L.ptr(vd), L.ptr(cd), Kc, deg, 1 if classic else 0, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]),
                                              L.ptr(o[3]), None, L.ptr(g_sh), acc, L.stream()), "gs_project_bwd_ex")
                torch.cuda.synchronize()
                gs = g_sh.cpu().numpy()
                assert not (_bits(gs) == F_PAT).any(), "g_sh_coeffs not fully written"
                assert not gs[dead].any() and not gs[:, nb:].any()
                _check(ep, "g_sh", gs, *shref["g_sh"])
                assert not gs[gids][:, :nb][np.broadcast_to(shf["clamped"][gids][:, None, :], (V, nb, 3))].any()
                got = [t.cpu().numpy() for t in o]
                for nm, g, w, b in zip(("v_means", "v_quats", "v_scales", "v_opacities"), got, want, bud):
                    assert not g[dead].any(), nm
                    w, b = w.astype(np.float64), np.asarray(b, np.float64)
                    if nm == "v_means":
                        dv, de = shref["g_means_dir"]
                        w, b = w + dv, b + de + np.abs(w + dv)
                    _check(ep, nm, g, w, b, kappa=max(util.PROJ_BUDGET_KAPPA, util.SH_KAPPA) if nm == "v_means" else util.PROJ_BUDGET_KAPPA)


# ----------------------------------------------------------------------------- the wrapper's routing of the packed columns
@pytest.mark.parametrize("render_mode", ["D", "RGB+D"])
def test_wrapper_routes_packed_columns(cuda, monkeypatch, render_mode):
    """rasterization_2dgs under a loss on the depth channel alone: the compositor's v_packed is recorded on its way to the projection
    backward, the reference reads its columns at the offsets the header documents (v_depths = the last colour column, 15 + C - 1), and
    every element of the leaves' gradients is checked against it"""
    from geosplatting_amd import surfels as S
    sc = _scene_dev(0)
    cam, fwd = sc["cam"], sc["fwd"]
    rows = np.nonzero(fwd["valid"] & np.isin(sc["regime"], [R.REGIMES.index(k) for k in ("plain", "flip", "ratio", "qnorm")]))[0]
    sub = {k: np.ascontiguousarray(sc[k][rows]) for k in ("means", "quats", "scales", "opacities")}
    N = len(rows)
    colors = np.random.RandomState(2).uniform(0, 1, (N, 3)).astype(np.float32)
    leaves = [t.requires_grad_(True) for t in _dev(cuda, sub["means"], sub["quats"], sub["scales"], sub["opacities"], colors)]
    vm, K = _dev(cuda, cam["viewmat"], cam["K"])
    seen = {}
    real = S._raster_bwd

    def spy(*a, **k):
        out = real(*a, **k)
        seen["v_packed"] = out[0].detach().clone()
        return out
    monkeypatch.setattr(S, "_raster_bwd", spy)
    render, _, _, _, _, _, meta = S.rasterization_2dgs(*leaves, vm[None], K[None], cam["W"], cam["H"], near_plane=cam["near"],
                                                       far_plane=cam["far"], render_mode=render_mode)
    cot = torch.tensor(np.random.RandomState(4).uniform(-1, 1, (cam["H"], cam["W"])).astype(np.float32), device=cuda)
    (render[0, ..., -1] * cot).sum().backward()
    torch.cuda.synchronize()
    gids = meta["gaussian_ids"].cpu().numpy()
    assert np.array_equal(gids, np.arange(N))                              # every row of the subset is visible
    Dc = 0 if render_mode == "D" else 3
    Cn = Dc + 1
    vp = seen["v_packed"].cpu().numpy()
    c = dict(v_ray_transforms=vp[:, 0:9], v_means2d=vp[:, 9:11], v_opacities=vp[:, 11], v_normals=vp[:, 12:15], v_colors=vp[:, 15:15 + Dc],
             v_depths=vp[:, 15 + Cn - 1])
    assert np.abs(c["v_depths"]).max() > 0
    sgn = np.where((meta["normals"].cpu().numpy().astype(np.float64) * fwd["normal"][rows]).sum(-1) < 0, -1.0, 1.0)
    ref = R.project_bwd_budget(sub["means"], sub["quats"], sub["scales"], cam["viewmat"], cam["K"], gids, sgn, c, check=False)
    for name, leaf in zip(("g_means", "g_quats", "g_scales", "g_opacities"), leaves):
        _check("wrapper", name, leaf.grad.cpu().numpy(), *ref[name])
    if Dc:
        assert _bits(leaves[4].grad.cpu().numpy()).tobytes() == _bits(vp[:, 15:18]).tobytes()
