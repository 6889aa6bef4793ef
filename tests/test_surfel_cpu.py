"""No-GPU checks of the 2D Gaussian splatting path: known answers for the float64 restatement (tests/surfel_ref.py), the exclusion caps
of the GPU tests' scenes on the restatement alone, the properties the stack scenes are built for, the per-pair restatement against
dense autograd and against itself in float32 (the measurement behind tests.util.SURFEL_BUDGET_KAPPA), and the public surface."""
import functools
import math

import pytest
import torch

from tests import surfel_ref as R
from tests.util import EPS32, SURFEL_BUDGET_KAPPA, SURFEL_PLAIN_MEDIAN_KAPPA

F, W, H = 40.0, 16, 16


def _cam():
    K = torch.tensor([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]], dtype=torch.float64)
    return torch.eye(4, dtype=torch.float64), K


def _surfels(zs, s=0.1, o=0.8, quat=(1.0, 0.0, 0.0, 0.0)):
    n = len(zs)
    means = torch.tensor([[0.0, 0.0, z] for z in zs], dtype=torch.float64)
    quats = torch.tensor([quat] * n, dtype=torch.float64)
    scales = torch.full((n, 3), s, dtype=torch.float64)
    return means, quats, scales, torch.full((n,), o, dtype=torch.float64), torch.full((n, 3), 0.5, dtype=torch.float64)


def _render(zs, **kw):
    vm, K = _cam()
    means, quats, scales, opac, cols = _surfels(zs, **kw)
    return R.rasterization_2dgs(means, quats, scales, opac, cols, vm, K, W, H, render_mode="RGB+D", distloss=True)


@pytest.mark.parametrize("s,z", [(0.1, 2.0), (0.004, 1.0)])          # the ray branch everywhere / the low-pass branch everywhere
def test_fronto_parallel_alpha_closed_form(s, z):
    out = _render([z], s=s)
    radius = int(out["radii"][0])
    assert radius == math.ceil(3 * max(s * F / z, 1e-2))
    for y in range(H):
        for x in range(W):
            d2 = (x + 0.5 - W / 2) ** 2 + (y + 0.5 - H / 2) ** 2
            a = R.fronto_parallel_alpha(d2, s, F, z, 0.8)
            want = a if a >= 1 / 255 else 0.0
            assert abs(float(out["alpha"][y, x]) - want) < 1e-12
    assert (out["ray_frac"] == 1.0) if s == 0.1 else (out["lowpass_frac"] == 1.0)


def test_one_surfel_has_no_distortion_two_have_the_pair_term():
    one = _render([2.0])
    assert float(one["distort"].abs().max()) == 0.0
    two = _render([2.0, 3.0])
    y, x = H // 2, W // 2
    d2 = 0.5
    a1, a2 = R.fronto_parallel_alpha(d2, 0.1, F, 2.0, 0.8), R.fronto_parallel_alpha(d2, 0.1, F, 3.0, 0.8)
    vis1, vis2 = a1, a2 * (1 - a1)
    assert abs(float(two["distort"][y, x]) - 2 * vis1 * vis2 * (3.0 - 2.0)) < 1e-12
    assert abs(float(two["median"][y, x]) - (3.0 if 1 - a1 > 0.5 else 2.0)) < 1e-12
    assert abs(float(two["render"][y, x, 3]) - (vis1 * 2.0 + vis2 * 3.0)) < 1e-12


def test_normal_faces_the_camera():
    towards = _render([2.0], quat=(0.0, 1.0, 0.0, 0.0))          # half a turn about x: the surfel's axis is (0, 0, -1)
    away = _render([2.0])                                        # its axis is (0, 0, 1), pointing away: flipped
    for out in (towards, away):
        assert torch.allclose(out["normals_cam"][0], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64), atol=1e-12)
    y, x = H // 2, W // 2
    assert float(away["normals"][y, x, 2]) < 0 and abs(float(away["normals"][y, x, 2]) + float(away["alpha"][y, x])) < 1e-12


def test_depth_to_normal_of_a_plane():
    vm, K = _cam()
    n = R.depth_to_normal(torch.full((H, W, 1), 2.0, dtype=torch.float64), vm, K)
    assert torch.allclose(n[1:-1, 1:-1], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand(H - 2, W - 2, 3), atol=1e-12)
    assert float(n[0].abs().max()) == 0.0 and float(n[:, -1].abs().max()) == 0.0
    import geosplatting_amd as gs
    got = gs.depth_to_normal(torch.full((H, W, 1), 2.0) + 0.01 * torch.arange(W)[None, :, None], vm.float(), K.float())
    want = R.depth_to_normal(torch.full((H, W, 1), 2.0, dtype=torch.float64) + 0.01 * torch.arange(W)[None, :, None], vm, K)
    assert torch.allclose(got.double(), want, atol=1e-5)


@pytest.mark.parametrize("name", ["inside", "outside", "clamp"])
def test_gpu_scene_exclusions_within_caps(name):
    """the seeds of tests/test_gpu_surfels.py: the restatement alone leaves out at most 1 % of the pixels and 0.5 % of the Gaussians"""
    sc = R.make_scene(name)
    with torch.no_grad():
        out = R.rasterization_2dgs(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["opacities"].double(),
                                   sc["sh"].double(), sc["viewmat"].double(), sc["K"].double(), sc["W"], sc["H"], sh_degree=sc["sh_degree"],
                                   background=sc["background"].double(), render_mode="RGB+ED", distloss=True, near=sc["near"])
    assert out["pix_bad"].double().mean().item() <= 0.01
    assert out["gauss_bad"].double().mean().item() <= 0.005
    assert out["n_clamped"] > 0 and out["n_skipped"] > 0
    if name == "inside":
        M2 = out["ray_transforms"][:, 2]
        d = M2[:, 0] ** 2 + M2[:, 1] ** 2 - M2[:, 2] ** 2
        assert 0 < out["ids"].numel() < 0.6 * sc["means"].shape[0] and (d > 0).any() and (d < 0).any()
    elif name == "outside":
        assert out["ray_frac"] >= 0.05 and out["lowpass_frac"] >= 0.05
    else:                                                        # the clamp active on several contributions of either branch
        assert out["n_clamped_ray"] >= 5 and out["n_clamped_lowpass"] >= 4


@pytest.mark.parametrize("case", R.CALL_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_call_level_exclusions_within_caps(case):
    """the added cases of tests/test_gpu_surfels.py (every mode and tile size): at most 1 % of the pixels left out, 1 % for the median,
    0.5 % of the Gaussians"""
    name, mode, distloss, tile, with_bg = case
    sc = R.make_scene(name, **R.CALL_SCENE_ARGS.get(name, {}))
    with torch.no_grad():
        out = R.rasterization_2dgs(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["opacities"].double(),
                                   sc["sh"].double(), sc["viewmat"].double(), sc["K"].double(), sc["W"], sc["H"], sh_degree=sc["sh_degree"],
                                   background=sc["background"].double() if with_bg else None, render_mode=mode, distloss=distloss,
                                   near=sc["near"], tile_size=tile)
    assert out["pix_bad"].double().mean().item() <= 0.01 and out["gauss_bad"].double().mean().item() <= 0.005
    if mode != "RGB":
        assert (out["pix_bad"] | out["median_bad"]).double().mean().item() <= 0.01
    assert out["n_active"] > 0 and out["n_skipped"] > 0 and out["lowpass_frac"] > 0 and out["ray_frac"] > 0


# ------------------------------------------------------------------------------------------------ the per-pair restatement
def test_pairs_equal_dense_autograd():
    """composite_pairs against composite() under autograd on 'clamp' (both branches, the clamp, a background, distloss): the same images,
    and want = the dense gradient; B >= |want|, and 0 exactly where no pair reaches"""
    C, tile = 4, 16
    inp = R.pair_scene_inputs("clamp", C, tile)
    out, cots = R.pair_reference(inp, C, True, tile, True, kinds=("dense",))
    want, B, B_plain = out["grads"][0]
    d = lambda k: inp[k].double().requires_grad_(True)
    leaves = [d(k) for k in ("M", "means2d", "opacities", "normals", "colors")]
    sc = R.make_scene("clamp")
    pr = R.project(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["viewmat"].double(), sc["K"].double(), 32, 32,
                   tile_size=tile)
    co = R.composite(leaves[0], leaves[1], leaves[2], leaves[4], leaves[3], True, pr["rect"][pr["valid"]], 32, 32, tile, True,
                     inp["background"].double(), order_key=inp["depths"].double())
    keep = out["keep"].double()
    for k in ("render", "alpha", "normals", "distort", "median"):
        assert torch.allclose(out[k], co[k].detach(), rtol=0, atol=1e-13), k
    assert torch.equal(out["pix_bad"], co["pix_bad"]) and out["n_active"] == co["n_active"] and out["n_clamped"] == co["n_clamped"]
    v_render, v_alpha, v_normals, v_distort = (c.double() for c in cots[0])
    loss = (co["render"] * v_render * keep[..., None]).sum() + (co["alpha"] * v_alpha * keep).sum() \
        + (co["normals"] * v_normals * keep[..., None]).sum() + (co["distort"] * v_distort * keep).sum()
    loss.backward()
    dense = torch.cat((leaves[0].grad.reshape(-1, 9), leaves[1].grad, leaves[2].grad[:, None], leaves[3].grad, leaves[4].grad), dim=-1)
    assert float(dense.abs().max()) > 0
    assert float((want - dense).abs().max()) <= 1e-12 * float(dense.abs().max())
    assert bool((B >= B_plain * (1 - 1e-12)).all()) and bool((B_plain >= want.abs() * (1 - 1e-12)).all())
    assert not want[-1].any() and not B[-1].any()                  # the surfel that stays below 1/255 everywhere


def _stack_tiles(name, tile):
    """per tile of a stack scene: (list length, last_ids of its kept pixels relative to the list's start), and the restatement"""
    inp = R.pair_scene_inputs(name, 4, tile)
    out, _ = R.pair_reference(inp, 4, True, tile, False, kinds=())
    W, H = inp["W"], inp["H"]
    tw = (W + tile - 1) // tile
    tiles = []
    for t, (start, n) in enumerate(zip(inp["offsets"].tolist(), out["list_len"].tolist())):
        ty, tx = divmod(t, tw)
        sl = (slice(ty * tile, min((ty + 1) * tile, H)), slice(tx * tile, min((tx + 1) * tile, W)))
        last = out["last_ids"][sl][out["keep"][sl]]
        tiles.append((n, torch.where(last >= 0, last - start, last)))
    return tiles, out, inp


@pytest.mark.parametrize("tile", [16, 8])
@pytest.mark.parametrize("name", list(R.STACK_SCENES))
def test_stack_scene_properties(name, tile):
    """what the stack scenes are built to drive, on the restatement: ragged tiles, the list length of every tile, the number of batches
    of nthreads = tile^2 records, the walk reaching the end of the list, and for 'stack_stop' a tile whose every pixel stops within the
    first batch of 256, tiles whose pixels stop at different entries, and a walk of all batches elsewhere"""
    L, stop = R.STACK_SCENES[name]
    tiles, out, inp = _stack_tiles(name, tile)
    W, H = inp["W"], inp["H"]
    assert (W, H) == (37, 27) and W % tile == 5 and H % tile == (11 if tile == 16 else 3)
    assert len(tiles) == (6 if tile == 16 else 20)
    nthreads = tile * tile
    batches = {(256, 16): 1, (257, 16): 2, (600, 16): 3, (256, 8): 4, (257, 8): 5, (600, 8): 10}[(L, tile)]
    assert out["n_clamped"] == 0 and out["ray_frac"] > 0.99
    assert out["pix_bad"].double().mean().item() <= 0.01 and (out["pix_bad"] | out["median_bad"]).double().mean().item() <= 0.01
    if not stop:
        for n, last in tiles:
            assert n == L and -(-n // nthreads) == batches
            assert bool((last == L - 1).all())                     # T stays above 1e-4: the walk starts at the last entry
        assert out["n_skipped"] == 0 and out["n_active"] == L * W * H
        assert float(out["alpha"].max()) < 1 - 1e-4
        return
    assert all(596 <= n <= 600 and -(-n // nthreads) == batches for n, _ in tiles) and max(n for n, _ in tiles) == 600
    distinct = [len(torch.unique(last)) for _, last in tiles]
    assert max(distinct) >= 8, distinct                            # pixels of one tile stop at different entries
    walked = [-(-(int(last.max()) + 1) // nthreads) for _, last in tiles]
    assert max(walked) == batches, walked                          # somewhere the backward walks every batch
    if tile == 16:
        n0, last0 = tiles[0]
        assert n0 >= 596 and int(last0.max()) < 255 and int(last0.min()) >= 0, (n0, int(last0.max()))     # all stopped in batch 0 of 3
        assert min(walked) == 1 and len(set(walked)) > 1
    else:
        assert min(walked) <= 2                                    # tile (0, 0) of 8: stopped within the first two batches of 64


@functools.lru_cache(maxsize=None)
def _pair_runs(case):
    name, C, distloss, tile, with_bg = case
    inp = R.pair_scene_inputs(name, C, tile)
    which = dict(seed=R.PAIR_CASES.index(case), one=R.pair_one_image(case))
    o64, cots = R.pair_reference(inp, C, distloss, tile, with_bg, **which)
    o32, _ = R.pair_reference(inp, C, distloss, tile, with_bg, dtype=torch.float32, keep=o64["keep"], **which)
    return inp, o64, o32, cots


def _pair_cots(case):
    return _pair_runs(case)[3]


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_pair_restatement_float32_within_half_kappa(case):
    """The measurement behind SURFEL_BUDGET_KAPPA and the caps of tests/test_gpu_surfel_budget.py, case by case: the restatement alone
    leaves out at most 1 % of the pixels (1 % with the median's band); in float32, on the pixels kept, it makes the decisions of the
    float64 run (last_ids) and every element of every gradient is within kappa / 2 of it, in units of 2^-24 B; an element with B = 0
    is 0.  Worst ratio over all cases: 41.6 (the figures are beside the constant)."""
    name, C, distloss, tile, with_bg = case
    inp, o64, o32, _ = _pair_runs(case)
    assert SURFEL_BUDGET_KAPPA * EPS32 <= 1e-4
    assert o64["pix_bad"].double().mean().item() <= 0.01
    if C != 3:
        assert (o64["pix_bad"] | o64["median_bad"]).double().mean().item() <= 0.01
    keep = o64["keep"]
    assert torch.equal(o32["last_ids"][keep], o64["last_ids"][keep])
    if name == "clamp":
        assert o64["n_clamped_ray"] >= 5 and o64["n_clamped_lowpass"] >= 4
    elif name == "outside":
        assert o64["lowpass_frac"] >= 0.01 and o64["ray_frac"] >= 0.5 and o64["n_skipped"] > 0 and int(o64["list_len"].max()) > 64
    worst, worst_median = 0.0, 0.0
    for kind, (w64, B64, P64), (w32, _, _) in zip(R.PAIR_COTANGENTS, o64["grads"], o32["grads"]):
        assert float(w64.abs().max()) > 0 and bool(torch.isfinite(B64).all())
        assert bool((B64 >= P64 * (1 - 1e-12)).all()) and bool((P64 >= w64.abs() * (1 - 1e-12)).all()) and bool(((B64 == 0) == (P64 == 0)).all())
        err = (w32.double() - w64).abs()
        assert not err[B64 == 0].any(), (case, kind)
        ratio = float((err[B64 > 0] / (EPS32 * B64[B64 > 0])).max())
        worst = max(worst, ratio)
        assert ratio <= SURFEL_BUDGET_KAPPA / 2, (case, kind, ratio)
        medians = R.plain_ratio_medians(err, P64, C)
        worst_median = max(worst_median, max(medians.values()))
        assert max(medians.values()) <= SURFEL_PLAIN_MEDIAN_KAPPA / 2, (case, kind, medians)
    one = R.pair_one_image(case)
    zero = [k for k, c in zip(("render", "alpha", "normals", "distort"), _pair_cots(case)[1]) if c is not None and not c.any()]
    assert sorted(zero + [one]) == sorted(["render", "alpha", "normals"] + (["distort"] if distloss else []))
    print(f"  {case}: worst float32 ratio {worst:.1f}, worst median against the plain sum {worst_median:.2f}")


def test_pair_cases_cover_every_instantiation():
    """the covering table: every launchable (C, DIST) at both tile sizes; every stack scene at both tile sizes and both DIST values;
    the colour modes with and without a background"""
    cases = set(R.PAIR_CASES)
    for C, dist in ((3, False), (1, False), (1, True), (4, False), (4, True)):
        for tile in (8, 16):
            assert any(c[1:4] == (C, dist, tile) for c in cases), (C, dist, tile)
    for name in R.STACK_SCENES:
        for tile in (8, 16):
            assert any(c[0] == name and c[3] == tile for c in cases)
        for dist in (False, True):
            assert any(c[0] == name and c[2] == dist for c in cases)
    for C in (3, 4):
        for bg in (False, True):
            assert any(c[1] == C and c[4] == bg for c in cases)
    images = {(R.pair_one_image(c), c[2], c[3]) for c in R.PAIR_CASES}              # the 'one' cotangent: every image, at both tile sizes
    for tile in (8, 16):
        assert ("distort", True, tile) in images
        for one in ("alpha", "normals"):
            assert any((one, dist, tile) in images for dist in (False, True)), (one, tile)
    assert {i[0] for i in images if i[1]} == {"alpha", "normals", "distort"} and {i[0] for i in images if not i[1]} == {"alpha", "normals"}
    assert not any(c[1] == 3 and c[2] for c in cases) and {c[0] for c in cases} == {"clamp", "outside"} | set(R.STACK_SCENES)


def test_public_surface():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    assert issubclass(gs.SurfelModel, gs.GSplatModel) and issubclass(gs.SurfelTrainer, gs.GSplatTrainer)
    z = torch.zeros(1, 3)
    args = (z, torch.ones(1, 4), z + 1, torch.ones(1), z, torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.rasterization_2dgs(*args)
    g = gs.GaussianSet.random(4, sh_degree=0, random_scale=1.0, generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError):
        gs.GSplatModel(gaussians=g, rasterize_mode="2dgs").render_rgb(None)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.SurfelModel(gaussians=g).render_rgb(gs.orbit_cameras(1, 3.0, 0.0, 16, 16, focal=20.0)[0])
    t = gs.SurfelTrainer()
    assert (t.normal_weight, t.distort_weight, t.normal_start, t.distort_start) == (5e-2, 1e-2, 7000, 3000)
