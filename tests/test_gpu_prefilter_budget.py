"""GPU: the split-sum prefilter (csrc/gs_splitsum.hip, csrc/gs_splitsum_tiles.hip) against float64, TEXEL BY TEXEL, within the
error budget of the float64 restatement (oracle/gs_oracle_splitsum.c, second half; derivations there and in oracle/__init__.py):
|got - want| <= kappa * 2^-24 * budget for every element, on maps with a 1e4 'sun', exact zeros and sparse / spiked cotangents
(tests/util.py).  The max-norm tests of tests/test_gpu_shading.py see the sun only; tests/test_prefilter_budget_cpu.py shows a wrong
dark texel that they accept and this criterion refuses.

The pair set is the float32 one (the suite pins the boxes bit for bit); pairs whose float64 cosine lies within 4 * 2^-24 of the
cutoff enter through the budget, so both decisions are admissible.  Texels with an empty lobe are 0 / 0 = NaN in the reference and
in the kernels: same texels on both sides, left out; the backward tests use configurations without them.

Whole pyramids: the forward is cut loose per stage (the reference is fed the GPU's own float32 mips), the backward propagates the
budgets through the mip links (util.prefilter_pyramid_backward_reference).

The 32 x 32-texel tile geometry (4, 16), which tile_geometry gives at R >= 512 only, is reached at R = 128 by patching it.

Worst ratio |got - want| / (2^-24 budget) per kernel and configuration, (a) the float32 oracle on the CPU, (b) the kernels on an
MI355X (run with -s to print them); kappa = the smallest power of two >= 4 x the larger, util.PREFILTER_SPEC_KAPPA / _LIN_KAPPA:
                                              (a) oracle32, CPU      (b) MI355X
    direct  (16, 1.0)  fwd / bwd                 1.22 / 0.19            0.17 / 0.22
    direct  (16, 0.5)                            0.51 / 0.38            0.33 / 0.38
    direct  (32, 0.29)                           0.52 / 0.63            0.51 / 0.63
    direct  (64, 0.08)                           1.04 / 0.43            1.04 / 0.43
    direct  (64, 0.395)                          0.56 / 0.44            0.54 / 0.42
    direct  (48, 0.2)  fwd only (570 NaN)        0.70                   0.70
    direct  (24, 0.5)                            0.62 / 0.41            0.48 / 0.44
    direct  bwd accumulating (32, 0.29), (64, 0.395)   --               0.73, 0.96
    tiled (1,1) x8  (16, 1.0)                    as direct              0.22 / 0.23
    tiled (1,1) x8  (32, 0.29)                                          0.51 / 0.63
    tiled (1,1) x8  (32, 0.5)                    0.91 / 0.33            0.37 / 0.35
    tiled (1,2) x8  (64, 0.08)                                          1.04 / 0.43
    tiled (1,2) x8  (64, 0.395)                                         0.55 / 0.43
    tiled (1,2) x1  (64, 0.395), symmetry off                           0.54 / 0.43
    tiled (1,2) x1  (96, 0.2)                    not run (R > 64)       0.52 / 0.71
    tiled (2,4) x8  (128, 0.08)                  not run                0.88 / 0.65
    tiled (2,4) x8  (128, 0.29)                  not run                0.77 / 0.70
    tiled (4,16) x8 (128, 0.08), LDS 22 / 25 KB  not run                0.88 / 0.65      (the table fits: the case is kept)
    gs_diffuse_cubemap_fwd / _bwd / _bwd acc.    0.72 / 0.14            0.16 / 0.23 / 0.82
    gs_cubemap_mip_fwd 64, 32                    0.73, 0.65             0.73, 0.65       (the oracle's bits)
    gs_cubemap_mip_chain_fwd 64, 32              --                     0.73, 0.65
    gs_cubemap_mip_bwd 16, 8 / accumulating      0.08, 0.06             0.08, 0.06 / 0.22, 0.54
    as_splitsum 64:  mips, base, levels          0.73, 0.52, 1.04 1.87 2.77      0.73, 0.18, 1.04 0.38 0.51
                     gradient (dense, sparse, one level)   0.45 0.26 --          0.45 0.26 0.02
    as_splitsum 128: mips, base, levels          (2.83 at the 16^2 level)        0.80, 0.12, 0.88 0.52 0.40 0.57
                     gradient                    0.34 0.65 0.07                  0.34 0.65 0.07
    specular: (a) 2.83 (the roughness-1.0 level of a pyramid: a sequential float32 sum over 1 500 sources; 2.77 in the 64^2
    pyramid the CPU suite runs), (b) 1.04 -> kappa 16;
    diffuse / mip: (a) 0.73, (b) 0.82 -> kappa 4.  Texels that own a pair in doubt: at most 2.4 % (128, 0.08); cap 5 %.
No kernel failed its budget; these ratios are the record that the prefilter holds per texel under HDR content.
"""
import numpy as np
import pytest
import torch

from tests import util
from tests.util import (PREFILTER_COTANGENTS, PREFILTER_DOUBT_CAP, PREFILTER_LIN_KAPPA, PREFILTER_SCENES, PREFILTER_SPEC_KAPPA,
                        assert_prefilter_budget, assert_within_budget, prefilter_cotangent, prefilter_scene)

pytestmark = pytest.mark.gpu

# direct kernels (gs_specular_cubemap_fwd / _bwd): R >= 64 makes the backward use its own box plus the margin of 2; 48 and 24 are no
# powers of two, 24 is not eligible for tiles; (48, 0.2) has 570 empty lobes: forward only
DIRECT = ((16, 1.0), (16, 0.5), (32, 0.29), (64, 0.08), (64, 0.395), (48, 0.2), (24, 0.5))
# tiled tables: (R, roughness, (bw, nb) expected, n_mirrors expected, GEOSPLAT_PREFILTER_SYMMETRY, patched geometry or None)
TILED = ((16, 1.0, (1, 1), 8, "1", None), (32, 0.29, (1, 1), 8, "1", None), (32, 0.5, (1, 1), 8, "1", None),
         (64, 0.08, (1, 2), 8, "1", None), (64, 0.395, (1, 2), 8, "1", None), (128, 0.08, (2, 4), 8, "1", None),
         (128, 0.29, (2, 4), 8, "1", None), (96, 0.2, (1, 2), 1, "1", None), (64, 0.395, (1, 2), 1, "0", None),
         (128, 0.08, (4, 16), 8, "1", (4, 16)))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _check_level(cuda, R, roughness, cached, tag):
    """forward over every scene and backward over every cotangent of one level through gs.specular_cubemap"""
    import geosplatting_amd as gs
    ref = util.prefilter_reference(R, roughness)
    assert ref["fwd_doubt"].mean() <= PREFILTER_DOUBT_CAP
    for k in PREFILTER_SCENES:
        with torch.no_grad():
            y = gs.specular_cubemap(_dev(prefilter_scene(k, R), cuda), roughness, cached=cached)
        assert_prefilter_budget(f"{tag} R={R} r={roughness} fwd {k}", y.cpu().numpy(), *ref["fwd"][k], kappa=PREFILTER_SPEC_KAPPA,
                                nan_expected=ref["has_nan"])
    if ref["has_nan"]:
        assert (R, roughness) == (48, 0.2)
        return
    assert ref["bwd_doubt"].mean() <= PREFILTER_DOUBT_CAP
    x = _dev(prefilter_scene("flat", R), cuda).requires_grad_(True)
    for k in PREFILTER_COTANGENTS:
        y = gs.specular_cubemap(x, roughness, cached=cached)
        g, = torch.autograd.grad(y, x, _dev(prefilter_cotangent(k, R), cuda))
        assert_within_budget(f"{tag} R={R} r={roughness} bwd {k}", g.cpu().numpy(), *ref["bwd"][k], kappa=PREFILTER_SPEC_KAPPA)


@pytest.mark.parametrize("R,roughness", DIRECT)
def test_direct_kernels_within_budget(cuda, R, roughness):
    _check_level(cuda, R, roughness, False, "direct")


@pytest.mark.parametrize("R,roughness,geometry,mirrors,symmetry,patch", TILED)
def test_tiled_tables_within_budget(cuda, monkeypatch, R, roughness, geometry, mirrors, symmetry, patch):
    from geosplatting_amd import splitsum as ss
    private = symmetry != "1" or patch is not None             # tables that no other test may find in the cache
    if private:
        monkeypatch.setenv("GEOSPLAT_PREFILTER_SYMMETRY", symmetry)
        if patch is not None:
            monkeypatch.setattr(ss, "tile_geometry", lambda res: patch)
        ss._tiles_cache.clear()
    try:
        e = ss.specular_tiles(R, roughness, 0.99, cuda)
        assert e is not None and (e["bw"], e["nb"]) == geometry and e["n_mirrors"] == mirrors, (e["bw"], e["nb"], e["n_mirrors"])
        print(f"\n  R={R} r={roughness}: geometry {geometry}, mirrors {mirrors}, LDS {e['fwd']['lds_bytes']} / {e['bwd']['lds_bytes']} B")
        assert max(e["fwd"]["lds_bytes"], e["bwd"]["lds_bytes"]) <= 160 * 1024
        _check_level(cuda, R, roughness, True, f"tiled{geometry}x{mirrors}")
    finally:
        if private:
            ss._tiles_cache.clear()


def _accumulated(val, bud, dst0):
    """reference of a kernel's accumulate form on top of dst0: the sum, and one more rounding of it"""
    return dst0.astype(np.float64) + val, bud + np.abs(dst0) + np.abs(val)


@pytest.mark.parametrize("R,roughness", [(32, 0.29), (64, 0.395)])
def test_direct_backward_accumulates_within_budget(cuda, R, roughness):
    """gs_specular_cubemap_bwd with accumulate = 1 on top of a non-zero destination, below and at the R >= 64 candidate rule"""
    from geosplatting_amd import _lib as L
    from geosplatting_amd import splitsum as ss
    ref = util.prefilter_reference(R, roughness)
    ct, bounds = ss.specular_bounds(R, roughness, 0.99, cuda)
    wsum = ss._weight_sums(R, roughness, 0.99, cuda).unsqueeze(-1)
    dst0 = prefilter_cotangent("dense", R, seed=3)
    for k in PREFILTER_COTANGENTS:
        v = (_dev(prefilter_cotangent(k, R), cuda) / wsum).contiguous()
        g = _dev(dst0, cuda)
        L.check(L.lib().gs_specular_cubemap_bwd(R, L.ptr(bounds), L.ptr(ss.dir_table(R, cuda)), L.ptr(v), L.f32(roughness), L.f32(ct),
                                                L.ptr(g), 1, L.stream()), "gs_specular_cubemap_bwd")
        want, b = _accumulated(*ref["bwd"][k], dst0)
        assert_within_budget(f"direct R={R} r={roughness} bwd {k} accumulate=1", g.cpu().numpy(), want, b, kappa=PREFILTER_SPEC_KAPPA)


def test_diffuse_kernels_within_budget(cuda):
    import oracle
    from geosplatting_amd import _lib as L
    R = 16
    for k in PREFILTER_SCENES:
        c = prefilter_scene(k, R)
        out = torch.empty(6, R, R, 3, device=cuda)
        L.check(L.lib().gs_diffuse_cubemap_fwd(R, L.ptr(_dev(c, cuda)), L.ptr(out), L.stream()), "gs_diffuse_cubemap_fwd")
        assert_within_budget(f"diffuse fwd {k}", out.cpu().numpy(), *oracle.diffuse_budget(c), kappa=PREFILTER_LIN_KAPPA)
    dst0 = prefilter_cotangent("dense", R, seed=3)
    for k in PREFILTER_COTANGENTS:
        v = prefilter_cotangent(k, R)
        val, bud = oracle.diffuse_budget(v, backward=True)
        for acc in (0, 1):
            g = _dev(dst0, cuda)
            L.check(L.lib().gs_diffuse_cubemap_bwd(R, L.ptr(_dev(v, cuda)), L.ptr(g), acc, L.stream()), "gs_diffuse_cubemap_bwd")
            want, b = _accumulated(val, bud, dst0) if acc else (val, bud)
            assert_within_budget(f"diffuse bwd {k} accumulate={acc}", g.cpu().numpy(), want, b, kappa=PREFILTER_LIN_KAPPA)


def test_mip_kernels_within_budget(cuda):
    """gs_cubemap_mip_fwd and gs_cubemap_mip_chain_fwd, each level of 64 -> 32 -> 16 on the level the GPU itself produced;
    gs_cubemap_mip_bwd at coarse R = 16 and 8, plain and accumulating"""
    import oracle
    from geosplatting_amd import _lib as L
    from geosplatting_amd import splitsum as ss
    for k in PREFILTER_SCENES:
        c = _dev(prefilter_scene(k, 64), cuda)
        chain = ss.mip_chain(c)
        assert [m.shape[1] for m in chain] == [64, 32, 16]
        single = [c]
        for _ in range(2):
            single.append(ss._CubeMapMip.apply(single[-1]))
        for name, maps in (("chain", chain), ("single", single)):
            for a, b in zip(maps[:-1], maps[1:]):
                assert_within_budget(f"mip {name} {a.shape[1]} {k}", b.cpu().numpy(), *oracle.cubemap_mip_fwd_budget(a.cpu().numpy()),
                                     kappa=PREFILTER_LIN_KAPPA)
    for R in (16, 8):
        dst0 = prefilter_cotangent("dense", 2 * R, seed=4)
        for k in PREFILTER_COTANGENTS:
            v = prefilter_cotangent(k, R)
            val, bud = oracle.cubemap_mip_bwd_budget(v)
            for acc in (0, 1):
                g = _dev(dst0, cuda)
                L.check(L.lib().gs_cubemap_mip_bwd(R, L.ptr(_dev(v, cuda)), L.ptr(g), acc, L.stream()), "gs_cubemap_mip_bwd")
                want, b = _accumulated(val, bud, dst0) if acc else (val, bud)
                assert_within_budget(f"mip bwd {R} {k} accumulate={acc}", g.cpu().numpy(), want, b, kappa=PREFILTER_LIN_KAPPA)


def _pyramid_cotangents(kind, sizes):
    """(v_base, [v_level]) of a pyramid; 'level1': dense on level 1 alone, everything else zero"""
    base_kind = "dense" if kind == "level1" else kind
    vb = prefilter_cotangent(base_kind, 16, seed=5)
    vl = [prefilter_cotangent(base_kind, R, seed=6 + i) for i, R in enumerate(sizes)]
    if kind == "level1":
        vb = np.zeros_like(vb)
        vl = [v if i == 1 else np.zeros_like(v) for i, v in enumerate(vl)]
    return vb, vl


@pytest.mark.parametrize("R", [64, 128])
def test_as_splitsum_within_budget(cuda, R):
    """as_splitsum at 64^2 (levels at roughness 0.08 / 0.5 / 1.0) and 128^2 (0.08 / 0.29 / 0.5 / 1.0): base and every level for
    'flat' and 'sun', no NaN anywhere; the cubemap gradient for dense and sparse cotangents and for a cotangent on one level only"""
    import geosplatting_amd as gs
    from geosplatting_amd import splitsum as ss
    sizes = [R >> i for i in range(3 if R == 64 else 4)]
    for k in ("flat", "sun"):
        x = _dev(prefilter_scene(k, R), cuda)
        with torch.no_grad():
            env = gs.as_splitsum(x)
        mips = [m.cpu().numpy() for m in ss.mip_chain(x)]
        assert [l.shape[1] for l in env.levels] == sizes == [m.shape[1] for m in mips]
        mip_refs, base_ref, level_refs = util.prefilter_pyramid_forward_reference(mips)
        for i, (want, bud) in enumerate(mip_refs):
            assert_within_budget(f"{R} {k} mip {i + 1}", mips[i + 1], want, bud, kappa=PREFILTER_LIN_KAPPA)
        assert_within_budget(f"{R} {k} base", env.base.cpu().numpy(), *base_ref, kappa=PREFILTER_LIN_KAPPA)
        for i, (want, bud) in enumerate(level_refs):
            assert_prefilter_budget(f"{R} {k} level {i}", env.levels[i].cpu().numpy(), want, bud, kappa=PREFILTER_SPEC_KAPPA)
    x = _dev(prefilter_scene("flat", R), cuda).requires_grad_(True)
    for kind in ("dense", "sparse", "level1"):
        vb, vl = _pyramid_cotangents(kind, sizes)
        env = gs.as_splitsum(x)
        if kind == "level1":
            g, = torch.autograd.grad(env.levels[1], x, _dev(vl[1], cuda))
        else:
            g, = torch.autograd.grad([env.base, *env.levels], x, [_dev(v, cuda) for v in (vb, *vl)])
        want, bud = util.prefilter_pyramid_backward_reference(vb, vl)
        assert_within_budget(f"{R} pyramid bwd {kind}", g.cpu().numpy(), want, bud, kappa=PREFILTER_SPEC_KAPPA)


def test_as_splitsum_cotangent_forms_give_the_same_bits(cuda):
    """a non-contiguous cotangent gives the bits of its contiguous copy, an absent cotangent those of explicit zeros"""
    import geosplatting_amd as gs
    R, sizes = 64, [64, 32, 16]
    x = _dev(prefilter_scene("sun", R), cuda).requires_grad_(True)
    vb, vl = _pyramid_cotangents("dense", sizes)
    cots = [_dev(v, cuda) for v in (vb, *vl)]
    strided = []
    for c in cots:
        wide = torch.zeros(*c.shape[:3], 6, device=cuda)
        wide[..., ::2] = c
        strided.append(wide[..., ::2])
        assert not strided[-1].is_contiguous() and torch.equal(strided[-1], c)

    def grad(outs_of, grads):
        env = gs.as_splitsum(x)
        return torch.autograd.grad(outs_of(env), x, grads)[0]

    every = lambda env: [env.base, *env.levels]
    want = grad(every, cots)
    assert torch.equal(grad(every, strided), want)
    zeros = [torch.zeros_like(c) if i != 2 else c for i, c in enumerate(cots)]
    assert torch.equal(grad(lambda env: [env.levels[1]], [cots[2]]), grad(every, zeros))
    from geosplatting_amd import splitsum as ss
    assert torch.equal(ss.as_splitsum_backward(cots[0], cots[1:]), want)        # the explicit backward the step engine calls
