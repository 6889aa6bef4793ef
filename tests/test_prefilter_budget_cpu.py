"""The split-sum prefilter's float64 reference and its error budgets, without a GPU: the float32 oracle (oracle/gs_oracle_splitsum.c,
first half) against the float64 restatement (second half) per texel, within kappa / 2; adjointness of the float64 operators; the
share of texels that own a pair in doubt; the empty lobes (0 / 0) of the small non-pyramid configurations; the scenes' own
properties; and one deliberately wrong result that the per-texel budget catches and the max-norm criterion does not.

Measurement (a) of the constants in tests/util.py (worst |oracle32 - float64| / (2^-24 budget) per configuration, printed by the
tests): specular forward 2.77 (the 16^2 level of the 64^2 pyramid, roughness 1.0; single levels up to 1.39), backward 0.63;
diffuse 0.72; mip forward 0.73, mip backward 0.08.
"""
import numpy as np
import pytest

import oracle
from tests import util
from tests.util import (PREFILTER_COTANGENTS, PREFILTER_DOUBT_CAP, PREFILTER_LIN_KAPPA, PREFILTER_SCENES, PREFILTER_SPEC_KAPPA,
                        assert_prefilter_budget, assert_within_budget, prefilter_cotangent, prefilter_reference, prefilter_scene)

# every (R, roughness) of tests/test_gpu_prefilter_budget.py the CPU can afford (R <= 64), the levels of a 64^2 pyramid included
SPEC_CONFIGS = ((16, 1.0), (16, 0.5), (32, 0.29), (32, 0.5), (64, 0.08), (64, 0.29), (64, 0.395), (24, 0.5))
# configurations with empty lobes (the reference's 16x16 culling tiles cull every pair of a narrow lobe): (R, roughness, NaN texels)
NAN_CONFIGS = ((16, 0.3, 790), (48, 0.08, 1278), (48, 0.2, 570))


def _level32(cubemap, ref, roughness):
    raw = oracle.specular_cubemap_fwd(cubemap, ref["bounds"], roughness, ref["ct"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return raw[..., :3] / raw[..., 3:], raw[..., 3:]


def test_scenes_and_cotangents_hold_their_properties():
    for R in (16, 24, 48, 64, 128):
        for k in PREFILTER_SCENES:
            c = prefilter_scene(k, R)
            assert c.shape == (6, R, R, 3) and c.dtype == np.float32 and np.isfinite(c).all()
        for k in PREFILTER_COTANGENTS:
            v = prefilter_cotangent(k, R)
            assert v.shape == (6, R, R, 3) and v.dtype == np.float32
        sun, flat = prefilter_scene("sun", R), prefilter_scene("flat", R)
        hot = (sun != flat).any(-1)
        assert sorted(zip(*np.nonzero(hot))) == sorted(util.prefilter_sun_texels(R))
        assert sun.max() / np.median(sun) >= 1e4
        sp = prefilter_cotangent("sparse", R)
        assert sorted(zip(*np.nonzero((sp != 0).any(-1)))) == sorted(util.prefilter_sparse_texels(R))
        assert (prefilter_scene("dark", R)[5] == 0).all()


@pytest.mark.parametrize("R,roughness", SPEC_CONFIGS)
def test_oracle32_specular_within_half_kappa(R, roughness):
    """forward for every scene, backward for every cotangent; no empty lobe in these configurations; a dark output whose whole lobe
    is zero is exactly 0; a gradient no cotangent reaches is exactly 0 (budget 0)"""
    ref = prefilter_reference(R, roughness)
    assert not ref["has_nan"]
    print(f"\n  R={R} roughness={roughness}: doubt share fwd {ref['fwd_doubt'].mean():.4f} bwd {ref['bwd_doubt'].mean():.4f}")
    assert ref["fwd_doubt"].mean() <= PREFILTER_DOUBT_CAP and ref["bwd_doubt"].mean() <= PREFILTER_DOUBT_CAP
    wsum = None
    for k in PREFILTER_SCENES:
        got, wsum = _level32(prefilter_scene(k, R), ref, roughness)
        assert_prefilter_budget(f"fwd {k}", got, *ref["fwd"][k], kappa=PREFILTER_SPEC_KAPPA / 2)
    if roughness < 0.3:
        assert (ref["fwd"]["dark"][1] == 0).any()
    for k in PREFILTER_COTANGENTS:
        v = prefilter_cotangent(k, R)
        got = oracle.specular_cubemap_bwd(ref["bounds"], (v / wsum).astype(np.float32), roughness, ref["ct"])
        assert_within_budget(f"bwd {k}", got, *ref["bwd"][k], kappa=PREFILTER_SPEC_KAPPA / 2)
    zero = (ref["bwd"]["sparse"][1] == 0).mean()
    print(f"  sparse cotangent: {zero:.4f} of the gradient elements have budget 0")
    if roughness < 0.3:                                            # (a wide lobe reaches every texel from ten sources)
        assert zero > (0.99 if (R, roughness) == (64, 0.08) else 0.5)


@pytest.mark.parametrize("R,roughness,n_nan", NAN_CONFIGS)
def test_empty_lobes_are_nan_on_both_sides(R, roughness, n_nan):
    ref = prefilter_reference(R, roughness)
    assert ref["has_nan"] and "bwd" not in ref
    print(f"\n  R={R} roughness={roughness}: doubt share fwd {ref['fwd_doubt'].mean():.4f}")
    assert ref["fwd_doubt"].mean() <= PREFILTER_DOUBT_CAP
    for k in PREFILTER_SCENES:
        want, bud = ref["fwd"][k]
        nan = np.isnan(want).all(-1)
        assert int(nan.sum()) == n_nan and np.array_equal(np.isnan(want).any(-1), nan)
        got, _ = _level32(prefilter_scene(k, R), ref, roughness)
        assert_prefilter_budget(f"fwd {k}", got, want, bud, kappa=PREFILTER_SPEC_KAPPA / 2, nan_expected=True)
    print(f"  empty lobes: {n_nan} of {6 * R * R} texels")


def test_oracle32_diffuse_and_mips_within_half_kappa():
    half = PREFILTER_LIN_KAPPA / 2
    for k in PREFILTER_SCENES:
        c = prefilter_scene(k, 16)
        assert_within_budget(f"diffuse fwd {k}", oracle.diffuse_cubemap_fwd(c), *oracle.diffuse_budget(c), kappa=half)
        for R in (64, 32):
            c = prefilter_scene(k, R)
            assert_within_budget(f"mip fwd {R} {k}", oracle.cubemap_mip_fwd(c), *oracle.cubemap_mip_fwd_budget(c), kappa=half)
    for k in PREFILTER_COTANGENTS:
        v = prefilter_cotangent(k, 16)
        assert_within_budget(f"diffuse bwd {k}", oracle.diffuse_cubemap_bwd(v), *oracle.diffuse_budget(v, backward=True), kappa=half)
        for R in (16, 8):
            v = prefilter_cotangent(k, R)
            want, bud = oracle.cubemap_mip_bwd_budget(v)
            assert_within_budget(f"mip bwd {R} {k}", oracle.cubemap_mip_bwd(v), want, bud, kappa=half)
            if k == "sparse":
                assert (bud == 0).mean() > 0.9


def test_float64_operators_are_adjoint():
    """<fwd64(x), v> = <x, bwd64(v)> to 1e-12 for the specular and the diffuse operator (HDR map, spiked cotangent)"""
    for R, roughness in ((16, 1.0), (32, 0.29), (64, 0.08)):
        ref = prefilter_reference(R, roughness)
        x = prefilter_scene("sun", R).astype(np.float64); v = prefilter_cotangent("spiked", R).astype(np.float64)
        a = (ref["fwd"]["sun"][0] * v).sum(); b = (x * ref["bwd"]["spiked"][0]).sum()
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (R, roughness, a, b)
    x = prefilter_scene("sun", 16); v = prefilter_cotangent("spiked", 16)
    a = (oracle.diffuse_budget(x)[0] * v).sum(); b = (x * oracle.diffuse_budget(v, backward=True)[0]).sum()
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (a, b)


def test_oracle32_pyramid_within_half_kappa():
    """oracle.as_splitsum / as_splitsum_bwd at 64^2 (levels 64 / 32 / 16 at roughness 0.08 / 0.5 / 1.0): the forward cut loose per
    stage on the oracle's own float32 mips, the backward with propagated budgets"""
    for k in ("flat", "sun"):
        cube = prefilter_scene(k, 64)
        base, levels, saved = oracle.as_splitsum(cube)
        mips = [cube, oracle.cubemap_mip_fwd(cube)]
        mips.append(oracle.cubemap_mip_fwd(mips[-1]))
        mip_refs, base_ref, level_refs = util.prefilter_pyramid_forward_reference(mips)
        for i, (want, bud) in enumerate(mip_refs):
            assert_within_budget(f"{k} mip {i + 1}", mips[i + 1], want, bud, kappa=PREFILTER_LIN_KAPPA / 2)
        assert_within_budget(f"{k} base", base, *base_ref, kappa=PREFILTER_LIN_KAPPA / 2)
        for i, (want, bud) in enumerate(level_refs):
            assert_prefilter_budget(f"{k} level {i}", levels[i], want, bud, kappa=PREFILTER_SPEC_KAPPA / 2)
    for k in ("dense", "sparse"):
        vb = prefilter_cotangent(k, 16, seed=5)
        vl = [prefilter_cotangent(k, R, seed=6 + i) for i, R in enumerate((64, 32, 16))]
        want, bud = util.prefilter_pyramid_backward_reference(vb, vl)
        assert_within_budget(f"pyramid bwd {k}", oracle.as_splitsum_bwd(saved, vb, vl), want, bud, kappa=PREFILTER_SPEC_KAPPA / 2)


def test_a_wrong_dark_texel_next_to_the_sun_fails_the_budget_and_passes_max_norm():
    """The reference level of the 'sun' scene at R = 32, roughness 0.29, with ONE pair weight perturbed by 1 % in ONE output texel:
    a dark output within 8 texels of the lone sun texel whose lobe holds no sun texel (a 1 % error of one pair weight of an output
    that does see the sun is below what float32 resolves there, in the budget and in fact).  Its own weight, the largest of its
    lobe, is the one perturbed; of these outputs the test takes the one where that shows best against the budget: 30 x 2^-24
    budget, about the most a 1 % error of ONE weight reaches at any roughness -- the 6 / d conditioning of the weights bounds it.
    Today's criterion (tests/test_gpu_shading.py: 1e-5 of the largest element for tiled against direct, 1e-4 against the oracle)
    accepts it by a factor of twenty -- the largest element is a sunlit one; the per-texel budget refuses it."""
    R, roughness = 32, 0.29
    ref = prefilter_reference(R, roughness)
    want, bud = ref["fwd"]["sun"]
    sun = prefilter_scene("sun", R)
    s, y, x = util.prefilter_sun_texels(R)[-1]
    maps = np.zeros((6, R, R, 1), np.float32)
    for t in util.prefilter_sun_texels(R):
        maps[t] = 1.0
    sees_sun = oracle.specular_fwd_budget(maps, ref["bounds"], roughness, ref["ct"])[0][..., 0] > 0
    assert sees_sun[s, y, x + 1] and sees_sun[s, y - 1, x]
    best = (0.0, None, None)
    for yo in range(y - 8, y + 9):
        for xo in range(x - 8, x + 9):
            o = (s, yo, xo)
            if sees_sun[o]:
                continue
            maps[:] = 0.0; maps[o] = 1.0
            share = oracle.specular_fwd_budget(maps, ref["bounds"], roughness, ref["ct"])[0][o][0]    # w(o, o) / W_o
            delta = 0.01 * share * (sun[o].astype(np.float64) - want[o])                              # first order in the weight
            best = max(best, (float((np.abs(delta) / (util.EPS32 * bud[o])).max()), o, delta), key=lambda b: b[0])
    ratio, o, delta = best
    print(f"\n  output {o}, {max(abs(o[1] - y), abs(o[2] - x))} texels from the sun: 1 % of its own weight = {ratio:.1f} x 2^-24 budget")
    assert (sun[o] < 2.0).all() and ratio > 1.5 * PREFILTER_SPEC_KAPPA
    got = want.copy()
    got[o] += delta
    assert 0 < util.rel_err(got, want) < 1e-6                                                     # passes max-norm ten times over
    assert_prefilter_budget("unperturbed", want, want, bud, kappa=PREFILTER_SPEC_KAPPA)
    with pytest.raises(AssertionError, match="ratio"):
        assert_prefilter_budget("perturbed", got, want, bud, kappa=PREFILTER_SPEC_KAPPA)
