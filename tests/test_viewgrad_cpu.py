"""No GPU: the reference of the view-matrix gradient (tests/viewgrad_ref.py) is right and its bound is honest.

For util.PROJ_BUDGET_SCENES 'yaw' and 'tilt_clip' (view 0) and two views of 'orbit8', antialiased and classic, SH degree None, 0 and
3, under every kind of util.PROJ_COTANGENTS:
  * the `_B` chain equals torch float64 autograd of the restated forward, one view-matrix leaf per Gaussian (the arbiter of the
    formulas: viewgrad_ref.check_against_autograd);
  * the all-float32 restatement of the same chain, summed wide and rounded once, lies within (VIEWGRAD_KAPPA / 2) * 2^-24 * B of the
    float64 sum, element by element, B = sum_n b_n + |sum_n c_n|; the last row is exactly 0 on both sides;
  * zero budgets mean exact zeros: an all-culled view and all-zero cotangents.
Worst ratios seen are in the docstring of tests/viewgrad_ref.py ((a) of VIEWGRAD_KAPPA).  Run with -s to print them.
"""
import numpy as np
import pytest

from tests import util
from tests import viewgrad_ref as vr

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for k in sorted(WORST, key=str):
        print(f"    {str(k):40s} f32 / bound {WORST[k][0]:6.3f}    _B vs autograd {WORST[k][1]:9.2e}")


def _case(name, vi, classic, deg, kind):
    sc, fwd = vr.scene(name)
    vw, m = sc["views"][vi], fwd[vi]
    gid = m["gaussian_ids"]
    cot, rgb = vr.cotangents(kind, len(gid), seed=11 + vi, with_rgb=deg is not None)
    sh = None if deg is None else (deg, vr.sh_inputs(sc, vi, deg), rgb)
    return sc, vw, gid, m["conics"], m["compensations"], cot, classic, sh


@pytest.mark.parametrize("deg", vr.SH_DEGREES)
@pytest.mark.parametrize("classic", vr.MODES)
@pytest.mark.parametrize("name,vi", vr.VIEWS)
def test_view_terms_equal_autograd_and_f32_within_bound(name, vi, classic, deg):
    for kind in util.PROJ_COTANGENTS:
        sc, vw, gid, conics, comps, cot, classic, sh = _case(name, vi, classic, deg, kind)
        assert len(gid) > 1000
        worst_auto = vr.check_against_autograd(sc, vw, gid, cot, classic, sh)
        want, bud, (c, b) = vr.view_reference(sc, vw, gid, conics, comps, cot, classic, sh)
        dead = np.zeros(len(gid), bool); dead[3::7] = True
        assert not c[dead].any() and not b[dead].any()                  # a visible Gaussian with an all-zero cotangent row: exactly 0
        assert not want[12:].any() and not bud[12:].any()
        assert np.abs(want[:12]).min() > 0 or kind == "opacity" and classic      # (classic: opacity cotangents reach no view entry)
        got = vr.view_f32(sc, vw, gid, conics, comps, cot, classic, sh)
        r = util.assert_within_budget(f"{name}/{vi} classic={classic} sh={deg} {kind}", got, want, bud, vr.VIEWGRAD_KAPPA / 2)
        key = (name, vi, classic, deg)
        old = WORST.get(key, (0.0, 0.0))
        WORST[key] = (max(old[0], r), max(old[1], worst_auto))


@pytest.mark.parametrize("n", vr.PREFIX_SIZES + (0,))
def test_prefix_scenes_f32_within_bound(n):
    """the first n Gaussians of 'yaw' (the reduction-edge sizes of tests/test_gpu_viewgrad.py; 0 stands for the prefix with exactly
    one visible Gaussian): with few terms the bound has no statistical slack, so these set (a)"""
    n = n or vr.one_visible_size()
    sub, gid, conics, comps = vr.prefix("yaw", 0, n)
    vw = sub["views"][0]
    for classic in vr.MODES:
        for deg in (None, 3):
            for kind in util.PROJ_COTANGENTS:
                cot, rgb = vr.cotangents(kind, len(gid), seed=7, with_rgb=deg is not None)
                sh = None if deg is None else (deg, vr.sh_inputs(sub, 0, deg), rgb)
                vr.check_against_autograd(sub, vw, gid, cot, classic, sh)
                want, bud, _ = vr.view_reference(sub, vw, gid, conics, comps, cot, classic, sh)
                got = vr.view_f32(sub, vw, gid, conics, comps, cot, classic, sh)
                r = util.assert_within_budget(f"yaw[:{n}] classic={classic} sh={deg} {kind}", got, want, bud, vr.VIEWGRAD_KAPPA / 2)
                key = (f"yaw[:{n}]", 0, classic, deg)
                WORST[key] = (max(WORST.get(key, (0.0, 0.0))[0], r), 0.0)


def test_zero_budget_means_exactly_zero():
    sc, fwd = vr.scene("yaw")
    vw, m = sc["views"][0], fwd[0]
    gid = m["gaussian_ids"]
    V = len(gid)
    zeros = (np.zeros((V, 2), np.float32), np.zeros((V, 3), np.float32), np.zeros(V, np.float32), np.zeros(V, np.float32))
    sh = (3, vr.sh_inputs(sc, 0, 3), np.zeros((V, 3), np.float32))
    want, bud, _ = vr.view_reference(sc, vw, gid, m["conics"], m["compensations"], zeros, False, sh)
    assert not want.any() and not bud.any()
    assert not vr.view_f32(sc, vw, gid, m["conics"], m["compensations"], zeros, False, sh).any()
    none = np.zeros(0, np.int32)                                        # an all-culled view
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), None)
    want, bud, _ = vr.view_reference(sc, vw, none, np.zeros((0, 3), np.float32), np.zeros(0, np.float32), empty)
    assert want.shape == (16,) and not want.any() and not bud.any()


def test_classic_has_no_compensation_gradient():
    """GS_PROJ_CLASSIC: opacity cotangents alone reach the view matrix through nothing"""
    sc, fwd = vr.scene("tilt_clip")
    vw, m = sc["views"][0], fwd[0]
    gid = m["gaussian_ids"]
    cot, _ = vr.cotangents("opacity", len(gid), seed=5, with_rgb=False)
    want, bud, _ = vr.view_reference(sc, vw, gid, m["conics"], m["compensations"], cot, True, None)
    assert not want.any() and not bud.any()
    want, _, _ = vr.view_reference(sc, vw, gid, m["conics"], m["compensations"], cot, False, None)
    assert np.abs(want[:12]).min() > 0
