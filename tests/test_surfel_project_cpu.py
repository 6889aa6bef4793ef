"""CPU: the reference of tests/test_gpu_surfel_project_budget.py checked on its own (tests/surfel_project_ref.py).

  * the restatement over (value, bound) numbers equals tests/surfel_ref.py::project in float64, and its hand-derived backward equals
    float64 autograd of surfel_ref.project (+ surfel_ref.sh_colors) -- both assertions live inside the reference's functions and run
    here over both scenes, plain colours and SH degrees 0..3, and every cotangent kind;
  * every regime of the scenes and every clamp pattern of the SH inputs holds at least 20 rows, on the reference alone;
  * the float32 restatement of the same chains lies within kappa / 2 budgets of float64 for EVERY element, forward and backward
    (kappa = util.SURFEL_PROJ_KAPPA, util.SH_KAPPA for the colours and g_sh): measurement (a) of the constants.

Worst ratio |float32 - float64| / (2^-24 budget) per output (run with -s):
    forward   ray_transforms 0.70   means2d 0.30   depths 0.70   normals 0.36   SH colours 1.00 (0.996)
    backward  g_means 0.55 (projection term alone 0.47)   g_quats 0.29   g_scales 0.27   g_sh 0.93   g_opacities / g_colors 0 (copies)
"""
import functools

import numpy as np
import pytest

from tests import surfel_project_ref as R
from tests import util

WORST = {}
SH_OUTPUTS = ("sh_colors", "g_sh")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for k in sorted(WORST):
        print(f"    {k:16s} {WORST[k]:7.3f}")


def _ratio(name, got, want, bud):
    kappa = util.SH_KAPPA if name in SH_OUTPUTS else util.SURFEL_PROJ_KAPPA
    r = util.assert_within_budget(name, got, want, bud, kappa / 2)
    WORST[name] = max(WORST.get(name, 0.0), r)


@functools.lru_cache(maxsize=None)
def _visible(ci):
    sc = R.budget_scene(ci)
    gids = np.nonzero(sc["fwd"]["valid"])[0]
    return sc, gids, np.where(sc["fwd"]["dot"][gids] > 0, -1.0, 1.0)


@pytest.mark.parametrize("ci", [0, 1])
def test_regimes_and_forward(ci):
    """budget_scene asserts restatement == surfel_ref.project and the margins of every row; here the regime counts and float32"""
    sc, gids, _ = _visible(ci)
    cam, fwd = sc["cam"], sc["fwd"]
    counts = R.assert_regimes(sc)
    print(counts)
    assert cam["W"] % R.TILE and cam["H"] % R.TILE and cam["K"][0, 0] != cam["K"][1, 1]
    assert abs(cam["K"][0, 2] - cam["W"] / 2) > 10 and abs(cam["K"][1, 2] - cam["H"] / 2) > 10
    assert (fwd["margins"]["sign"][gids] < 2 * R.MARGIN_KAPPA).sum() >= 5        # the sign is the GPU's to decide on some rows
    assert (~fwd["radius_exact"][gids]).sum() >= 20 and (fwd["radii"][gids][~fwd["radius_exact"][gids]] >= R.RADIUS_BIG).all()
    f = R.project_fwd_f32(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"])
    for name, key in (("ray_transforms", "M"), ("means2d", "means2d"), ("depths", "depths"), ("normals", "normal")):
        _ratio(name, f[key][gids], fwd[key][gids], fwd[key + "_e"][gids])
    # the float32 evaluation takes every decision as float64 does (this is what the margins are for)
    assert np.array_equal((f["dot"] > 0)[gids][fwd["margins"]["sign"][gids] >= 2 * R.MARGIN_KAPPA],
                          (fwd["dot"] > 0)[gids][fwd["margins"]["sign"][gids] >= 2 * R.MARGIN_KAPPA])


@pytest.mark.parametrize("deg", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("ci", [0, 1])
def test_backward_and_sh(ci, deg):
    sc, gids, sgn = _visible(ci)
    cam = sc["cam"]
    sh = None
    if deg is not None:
        co, shf = R.sh_inputs(ci, deg)                                           # asserts restatement == surfel_ref.sh_colors
        sh = (deg, co)
        print(R.assert_clamp_patterns(shf, sc["fwd"]["valid"]))
        rgb = R.sh_fwd_f32(deg, sc["means"], cam["viewmat"], cam["K"], co)
        _ratio("sh_colors", rgb[gids], shf["rgb"][gids], shf["rgb_e"][gids])
        assert not rgb[gids][shf["clamped"][gids]].any()
        mag = np.abs(co).max((1, 2))
        assert mag.min() < 1e-2 and mag.max() > 10.0
    for i, kind in enumerate(R.COTANGENTS):
        cot = R.cotangents(kind, len(gids), 3, seed=10 * ci + i)
        ref = R.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], gids, sgn, cot, sh)   # asserts == autograd
        f = R.project_bwd_f32(sc["means"], sc["quats"], sc["scales"], cam["viewmat"], cam["K"], gids, sgn, cot, sh)
        for name in ("g_means", "g_means_proj", "g_quats", "g_scales", "g_opacities") + (("g_sh",) if sh else ("g_colors",)):
            _ratio(name, f[name], *ref[name])
        assert not ref["g_scales"][1][:, 2].any() and not f["g_scales"][:, 2].any()
        if kind == "rows0":
            dead = np.ones(len(sc["means"]), bool); dead[gids] = False; dead[gids[3::7]] = True
            for name in ("g_means", "g_quats", "g_scales"):
                assert not ref[name][1][dead].any() and not f[name][dead].any()
        if kind == "only_v_depths":
            assert not ref["g_quats"][1].any() and not ref["g_scales"][1].any()
            # three products per row: R[2, i] * v_depth (the zero terms of the sum add nothing)
            want = cam["viewmat"][2, :3].astype(np.float64)[None] * cot["v_depths"].astype(np.float64)[:, None]
            assert np.allclose(ref["g_means_proj"][0][gids], want, rtol=1e-14, atol=0)
        if kind == "only_v_opacities":
            for name in ("g_means", "g_quats", "g_scales"):
                assert not ref[name][1].any()
            assert f["g_opacities"][gids].tobytes() == cot["v_opacities"].tobytes()
        if sh:
            assert not ref["g_sh"][1][:, (deg + 1) ** 2:].any()
            assert not ref["g_sh"][1][gids][np.broadcast_to(shf["clamped"][gids][:, None, :], ref["g_sh"][1][gids].shape)].any()
