"""GPU: both surfel compositor kernels of csrc/gs_surfel.hip, every launchable instantiation <C, DIST> at tile sizes 8 and 16, against the
float64 per-pair restatement (tests/surfel_ref.py composite_pairs), ELEMENT BY ELEMENT:

    |got - want| <= kappa * 2^-24 * B      for every element of v_packed[:, :15 + C] and of v_densify,

kappa = tests.util.SURFEL_BUDGET_KAPPA (measured on the CPU from the restatement itself in float32: tests/test_surfel_cpu.py), B below.  The stages
are called directly (surfels._project_bin, _raster_fwd, _raster_bwd) and the restatement is fed the GPU's own projected fp32 tensors,
flatten_ids and tile offsets, so projection and binning differences drop out.  An element with B = 0 (no kept pixel reaches the surfel,
or only zero cotangents do) must be exactly 0, and so must the pad columns 15 + C .. SF_REC - 1.  Pixels inside the restatement's
decision bands are left out through masked cotangents; the caps (1 % of the pixels, 1 % with the median's band) are asserted for every
case on the CPU.  Forward: render, alphas, normals, distort, median at the project's 1e-4 max-norm on the kept pixels, last_ids exactly.

Cases: surfel_ref.PAIR_CASES (the covering is asserted in tests/test_surfel_cpu.py), each under dense, one-image and sparse cotangents.
Scenes: 'clamp', 'outside' at 400 Gaussians with the edge-on surfels taken out (see make_scene), and the stack scenes, whose lists of
256 / 257 / 600 entries sit on and across the batch edges of both kernels (properties asserted in tests/test_surfel_cpu.py).

What B is: wider than the plain sum_p |grad[v, p]|.  Per tile every per-Gaussian input is broadcast to a leaf [L, P, ...] and autograd
returns the gradient pair by pair; B sums, over the pixels, the SIZES of the terms that the restatement's own graph adds within one pair
and that may cancel there: the images (one backward each), the two routes of dL/dalpha, the two products of each component of
hv x dL/dz and dL/dz x hu, and px dL/dhu + py dL/dhv in the row M2 (the derivation of each factor is in composite_pairs' docstring).
With the plain sum the float32 restatement itself reaches ratios of 10^3 to 5 * 10^5 under the sparse cotangents on 'clamp' and
'outside', whatever the scene: one pair is a whole element there, and among a few thousand pairs one cancels to a thousandth.  B is
typically 2 to 20 times the plain sum (median element; 1 % of the elements more than 100 to 1000 times), so kappa * 2^-24 * B is a bound
on every element but NOT the project's 1e-4 of the plain sum.  Against the plain sum the test asserts what can hold: the MEDIAN element of
every gradient (those with at least 64 reached elements) within util.SURFEL_PLAIN_MEDIAN_KAPPA = 32, i.e. 1.9e-6 of sum_p |grad|.
The 'one' cotangent drives alpha, normals and distort in turn over the cases (surfel_ref.pair_one_image; distort alone at both tile sizes).

Worst ratio |got - want| / (2^-24 B) on an MI355X per instantiation and gradient, over all cases and cotangents (kappa = 512):
    <C, DIST>     v_M     v_means2d   v_opacity   v_normal   v_colors   v_densify
    <3, false>   15.23      11.80       13.28      26.57      26.11       14.03
    <1, false>  179.89      22.75       18.07      33.14      32.41      180.36
    <1, true>    17.30      34.32       21.47      25.45      20.02       17.38
    <4, false>   18.24      32.86       21.51      41.57      40.71       17.93
    <4, true>    25.45      78.61       34.34      34.26      41.94       25.57
and the worst median of |got - want| / (2^-24 sum_p |grad|) (bar 32; the float32 restatement on the CPU: 6.95):
    <3, false>    7.18       1.69        5.64       6.21       6.40
    <1, false>   13.27       1.91        9.50       4.71       7.72
    <1, true>    16.87       3.19       13.29       7.58       4.00
    <4, false>   11.62       2.08       12.40       3.50       6.08
    <4, true>    18.80       7.41       19.51       3.88       4.70
Run with -s for the figures of every gradient of every case.

Whether the tests bite.  Each one-line change below was built into a scratch library (never committed, every address in bounds) and
this module and tests/test_gpu_surfels.py were run against it on an MI355X; "old" are the seven tests that module had before (the three
RGB+ED cases of test_forward_and_backward, one surfel, the empty view, the branches, the trainer), "modes" its 23 added cases.  The
first failing element of the first failing case here is quoted; the unchanged library passes all 31 + 30.
 (a) GsBfly::owned_index with the stage bits of lane & 1 and lane & 2 swapped -- FAILS all 31 cases (first clamp C=3 t16 dense,
     v_M[2, 4] got 35.33 want 1.381, ratio 12 360 113) and the 23 modes.  Old: 4 fail (the three cases, the trainer).
 (b) the backward's cnt as min(nthreads, hi - start): the first entry of every list is never walked -- FAILS all 31 (first clamp C=3
     t16 dense, v_M[6, 2] got 0 want 0.552, ratio 763 158) and the 23 modes.  Old: 3 fail (outside, clamp, one surfel; 'inside' passes).
 (c) `val[15 + C - 1] +=` written as `=` under DIST: the depth channel loses its render gradient -- FAILS the 13 cases with DIST
     (first clamp C=4 t8 dense, v_colors[1, 3] got -1.054 want 0.223, ratio 1 690 618) and the 12 modes with distloss.  Old: 3 fail.
 (d) the background loops running to C in place of C - depth_channel -- not built: the change cannot be observed.  Both loops also
     stop at k < 3 and the background has three entries, so C = 4 reads the same three; with C = 1 the Python entry passes no
     background (colours are None in the depth-only modes), and C = 3 has no depth channel.  Only a caller of the C ABI that hands a
     background to a depth-only launch would see it.
 (e) `lane < 16` as `lane < 8`: half of the values of every record are never committed -- FAILS all 31 (first clamp C=3 t16 dense,
     v_M[4, 3] got 0 want -1.146, ratio 1 417 153) and the 23 modes.  Old: 5 fail.
 (f) `hi - j <= my_last` as `<`: every pixel loses its last entry -- FAILS all 31 (first clamp C=3 t16 dense, v_M[4, 2] got 0.360 want
     -1.466, ratio 1 190 536) and the 23 modes.  Old: 4 fail.
 (g) the commit to global memory skipping per-tile sums of magnitude up to 1e-6 (`a != 0.0f` as `fabsf(a) > 1e-6f`): small
     contributions dropped, large ones untouched -- FAILS 28 cases: every case of 'outside' and of the stack scenes, one of 'clamp' (first
     clamp C=1 t8 sparse, v_M[8, 2] got -4.52911e-03 want -4.52821e-03, ratio 539).  Old: all 7 pass, and so do the 23 modes: the
     max-norm criterion cannot see it.
"""
import functools

import pytest
import torch

from tests import surfel_ref as R
from tests import util
from tests.util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
KAPPA = util.SURFEL_BUDGET_KAPPA
WORST, WORST_PLAIN = {}, {}               # (C, DIST) -> {gradient: worst ratio}, printed by every test (run with -s)


def _S():
    import geosplatting_amd.surfels as S
    return S


@functools.lru_cache(maxsize=None)
def _reference(name, C, distloss, tile, with_bg):
    """GPU projection, binning and compositor forward of a case, and the float64 restatement with its gradients under the three
    cotangents, on the GPU's own per-Gaussian tensors and lists"""
    S = _S()
    cuda = torch.device("cuda:0")
    sc = R.make_scene(name, **R.PAIR_SCENE_ARGS.get(name, {}))
    W, H = sc["W"], sc["H"]
    d = lambda k: sc[k].to(cuda).contiguous()
    colors = d("sh") if C >= 3 else None
    st = S._project_bin(d("means"), d("quats"), d("scales"), d("opacities"), colors, d("viewmat"), d("K"), W, H, tile, sc["near"], 1e10, 0.0,
                        sc["sh_degree"] if C >= 3 else None, C != 3)
    assert st["C"] == C and st["V"] > 0
    bg = sc["background"].to(cuda) if (with_bg and C >= 3) else None
    fwd = S._raster_fwd(st, bg, W, H, tile, C != 3, distloss)
    torch.cuda.synchronize()
    inp = dict(M=st["ray_transforms"], means2d=st["means2d"], opacities=st["opacities"], colors=st["colors"], normals=st["normals"],
               flatten_ids=st["flatten_ids"], offsets=st["isect_offsets"], W=W, H=H, background=sc["background"])
    case = (name, C, distloss, tile, with_bg)
    ref, cots = R.pair_reference(inp, C, distloss, tile, with_bg, seed=R.PAIR_CASES.index(case), one=R.pair_one_image(case))
    return sc, st, bg, fwd, ref, cots


@pytest.mark.parametrize("name,C,distloss,tile,with_bg", R.PAIR_CASES,
                         ids=[f"{c[0]}-C{c[1]}-{'dist' if c[2] else 'nodist'}-t{c[3]}-{'bg' if c[4] else 'nobg'}" for c in R.PAIR_CASES])
def test_compositor_within_budget(cuda, name, C, distloss, tile, with_bg):
    S = _S()
    sc, st, bg, fwd, ref, cots = _reference(name, C, distloss, tile, with_bg)
    render, alphas, normals, distort, median, last_ids, final_T, final_D = fwd
    W, H, V = sc["W"], sc["H"], st["V"]
    depth_channel = C != 3
    keep = ref["keep"]
    assert (~keep).double().mean().item() <= 0.01

    # ---- forward, on the kept pixels
    masked = lambda a, k=keep: (a.detach().cpu().double() * (k if a.dim() == 2 else k[..., None])).numpy()
    images = [("render", render), ("alpha", alphas), ("normals", normals)] + ([("distort", distort)] if distloss else [])
    for key, got in images:
        err = rel_err(masked(got), masked(ref[key]))
        assert err <= TOL, (key, err)
    if depth_channel:
        keep_med = keep & ~ref["median_bad"]
        assert (~keep_med).double().mean().item() <= 0.01
        assert rel_err(masked(median, keep_med), masked(ref["median"], keep_med)) <= TOL
    else:
        assert float(median.abs().max()) == 0.0
    got_last = last_ids.cpu().long()
    assert torch.equal(got_last[keep], ref["last_ids"][keep]), int((got_last != ref["last_ids"])[keep].sum())

    # ---- backward, every element
    depths = st["depths"].cpu().double()
    worst, worst_plain = WORST.setdefault((C, distloss), {}), WORST_PLAIN.setdefault((C, distloss), {})
    stride = S.L.lib().gs_surfel_grad_stride()
    for kind, cot, (want, B, B_plain) in zip(R.PAIR_COTANGENTS, cots, ref["grads"]):
        keep32 = keep.float()
        v = [None if c is None else (c * (keep32 if c.dim() == 2 else keep32[..., None])).to(cuda).contiguous() for c in cot]
        v_packed, v_densify = S._raster_bwd(st, bg, W, H, tile, depth_channel, distloss, last_ids, final_T, final_D, *v)
        torch.cuda.synchronize()
        vp, vd = v_packed.cpu().numpy(), v_densify.cpu().numpy()
        assert vp.shape == (V, stride) and not vp[:, 15 + C:].any()                  # the pad columns stay 0
        assert float(want.abs().max()) > 0
        unreached = (B == 0).all(1).numpy()
        assert not vp[unreached].any() and not vd[unreached].any()                  # rows no kept pixel reaches
        label = f"{name} C={C} dist={int(distloss)} t{tile} {kind}"
        for nm, a, b in R.packed_groups(C):
            r = util.assert_within_budget(f"{label} {nm}", vp[:, a:b], want[:, a:b].numpy(), B[:, a:b].numpy(), kappa=KAPPA)
            worst[nm] = max(worst.get(nm, 0.0), r)
        # gradient_2dgs: the depth times the two centre terms of the ray transform
        r = util.assert_within_budget(f"{label} v_densify", vd, (depths[:, None] * want[:, [2, 5]]).numpy(),
                                      (depths.abs()[:, None] * B[:, [2, 5]]).numpy(), kappa=KAPPA)
        worst["v_densify"] = max(worst.get("v_densify", 0.0), r)
        # ... and against the plain absolute sum, which B widens: the median element of every gradient
        err = (torch.from_numpy(vp[:, :15 + C]).double() - want).abs()
        medians = R.plain_ratio_medians(err, B_plain, C)
        print(f"  {label} median |got-want|/(eps sum|grad|): " + "  ".join(f"{k} {x:.2f}" for k, x in medians.items()))
        assert max(medians.values()) <= util.SURFEL_PLAIN_MEDIAN_KAPPA, (label, medians)
        for k, x in medians.items():
            worst_plain[k] = max(worst_plain.get(k, 0.0), x)
    print(f"  worst so far <{C}, {str(distloss).lower()}>: " + "  ".join(f"{k} {x:.2f}" for k, x in worst.items()))
    print(f"  worst median so far <{C}, {str(distloss).lower()}>: " + "  ".join(f"{k} {x:.2f}" for k, x in worst_plain.items()))
