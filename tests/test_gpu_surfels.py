"""2D Gaussian splatting on the GPU against the float64 restatement (tests/surfel_ref.py): projection, binning, compositor, the backward
of both, the model and the trainer.  Tolerance: the project's 1e-4 max-norm relative (tests.util.rel_err).  Pixels and Gaussians whose
decision margins in the restatement lie inside its band are left out; the caps (1 % of pixels, 0.5 % of Gaussians) are asserted.
Scenes (tests/surfel_ref.py): two random ones, and a hand-placed one on which the 0.999 clamp is active on either branch of min(w3, w2)."""
import functools

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from tests import surfel_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _reference(name, render_mode="RGB+ED", distloss=True, tile_size=16, with_background=True, small=False):
    """small: the scene at the size of the added cases (R.CALL_SCENE_ARGS)"""
    return R.scene_reference(name, render_mode, distloss, tile_size, with_background, **(R.CALL_SCENE_ARGS.get(name, {}) if small else {}))


def _gpu_call(sc, dev, requires_grad=True, **kw):
    leaves = {k: sc[k].to(dev).requires_grad_(requires_grad) for k in ("means", "quats", "scales", "opacities", "sh")}
    args = dict(viewmats=sc["viewmat"].to(dev)[None], Ks=sc["K"].to(dev)[None], width=sc["W"], height=sc["H"], sh_degree=sc["sh_degree"],
                backgrounds=sc["background"].to(dev)[None], render_mode="RGB+ED", distloss=True, near_plane=sc["near"], tile_size=16)
    args.update(kw)
    out = gs.rasterization_2dgs(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves["sh"], **args)
    return leaves, out


def _masked(a, keep):
    a = a.detach().cpu().double()
    return (a * (keep if a.dim() == 2 else keep[..., None])).numpy()


def _tile_count_bounds(ref, ids_got, means2d_got, radii_got, tile, tw, th):
    """Per tile, the least and the most intersections the restatement allows.  A Gaussian whose cull, radius and tile edges are all
    decided counts once on every tile of the restatement's rectangle.  An undecided one is taken as the kernel projected it, if it did:
    once for certain on the tiles of its square shrunk by a pixel, once at most on those of the square grown by a pixel."""
    undecided = ref["gauss_bad"] | ref["edge_bad"]
    lo = torch.zeros(th, tw, dtype=torch.long)
    for g, (x0, y0, x1, y1) in zip(ref["ids"].tolist(), ref["rect"].tolist()):
        if not undecided[g]:
            lo[y0:y1, x0:x1] += 1
    hi = lo.clone()
    for row in torch.nonzero(undecided[ids_got]).reshape(-1).tolist():
        mx, my, r = means2d_got[row, 0].double(), means2d_got[row, 1].double(), radii_got[row].double()
        x0, y0, x1, y1 = (int(v) for v in R.tile_rect(mx, my, (r - 1).clamp_min(0), tile, tw, th))
        lo[y0:y1, x0:x1] += 1
        x0, y0, x1, y1 = (int(v) for v in R.tile_rect(mx, my, r + 1, tile, tw, th))
        hi[y0:y1, x0:x1] += 1
    return lo, hi


@pytest.mark.parametrize("name", ["inside", "outside", "clamp"])
def test_forward_and_backward(cuda, name):
    _check_call(cuda, _reference(name), "RGB+ED", True, 16, True)


@pytest.mark.parametrize("name,render_mode,distloss,tile,with_bg", R.CALL_CASES,
                         ids=[f"{c[0]}-{c[1]}-{'dist' if c[2] else 'nodist'}-t{c[3]}-{'bg' if c[4] else 'nobg'}" for c in R.CALL_CASES])
def test_forward_and_backward_modes(cuda, name, render_mode, distloss, tile, with_bg):
    """every render mode, with and without distloss, at tile sizes 8 and 16, with and without a background: the ED division and the
    depth-only column routing of the projection backward are on the path of the leaf gradients ('outside' at 400 Gaussians)"""
    _check_call(cuda, _reference(name, render_mode, distloss, tile, with_bg, small=True), render_mode, distloss, tile, with_bg)


def _check_call(cuda, reference, render_mode, distloss, tile, with_bg):
    sc, ref, cot, keep, grads, densify = reference
    N, H, W = sc["means"].shape[0], sc["H"], sc["W"]
    depth_mode, expected = render_mode != "RGB", render_mode in ("ED", "RGB+ED")
    assert (1 - keep).mean().item() <= 0.01 and ref["gauss_bad"].double().mean().item() <= 0.005
    leaves, (render, alpha, normals, nfd, distort, median, meta) = _gpu_call(
        sc, cuda, render_mode=render_mode, distloss=distloss, tile_size=tile, backgrounds=sc["background"].to(cuda)[None] if with_bg else None)
    assert render.shape == (1, H, W, R.MODE_CHANNELS[render_mode]) and (distort is None) == (not distloss) and (nfd is None) == (not expected)
    meta["gradient_2dgs"].retain_grad()

    # ---- projection and binning
    good = ~ref["gauss_bad"]
    ids_ref, ids_got = ref["ids"], meta["gaussian_ids"].cpu()
    sel = lambda ids: ids[good[ids]]
    assert torch.equal(sel(ids_got), sel(ids_ref))
    pos_ref = {int(g): i for i, g in enumerate(ids_ref.tolist())}
    rows_got = [i for i, g in enumerate(ids_got.tolist()) if good[g] and g in pos_ref]
    rows_ref = [pos_ref[int(ids_got[i])] for i in rows_got]
    assert len(rows_got) >= ids_ref.numel() - int(ref["gauss_bad"].sum())
    assert torch.equal(meta["radii"].cpu()[rows_got].long(), ref["radii"][rows_ref])
    for key, want in (("means2d", ref["means2d"]), ("depths", ref["depths"]), ("normals", ref["normals_cam"])):
        err = rel_err(meta[key].detach().cpu()[rows_got], want.detach()[rows_ref])
        assert err <= TOL, (key, err)
    # (the ray transforms of surfels that nearly contain the camera have entries of any size: compared row by row)
    rt_got, rt_ref = meta["ray_transforms"].cpu()[rows_got].double(), ref["ray_transforms"].detach()[rows_ref]
    rt_err = ((rt_got - rt_ref).abs().amax((1, 2)) / rt_ref.abs().amax((1, 2))).max().item()
    assert rt_err <= TOL, rt_err
    # tile offsets and the length of the list: every tile's count, exact wherever no undecided Gaussian reaches
    tw, th = meta["tile_width"], meta["tile_height"]
    assert (tw, th) == ((W + tile - 1) // tile, (H + tile - 1) // tile) and meta["isect_offsets"].shape == (1, th, tw)
    n_isects = meta["flatten_ids"].numel()
    offsets = meta["isect_offsets"].cpu().reshape(-1).long()
    counts_got = (torch.cat((offsets[1:], torch.tensor([n_isects]))) - offsets).reshape(th, tw)
    lo, hi = _tile_count_bounds(ref, ids_got, meta["means2d"].detach().cpu(), meta["radii"].cpu(), tile, tw, th)
    assert int(offsets[0]) == 0 and bool((counts_got >= lo).all()) and bool((counts_got <= hi).all()), (counts_got, lo, hi)
    assert int(lo.sum()) <= n_isects <= int(hi.sum())
    assert n_isects == int(meta["tiles_per_gauss"].sum())

    # ---- images
    images = (("render", render[0]), ("alpha", alpha[0, ..., 0]), ("normals", normals[0]))
    if distloss:
        images += (("distort", distort[0, ..., 0]),)
    for key, got in images:
        err = rel_err(_masked(got, keep), _masked(ref[key], keep))
        assert err <= TOL, (key, err)
    if depth_mode:
        keep_med = keep * (~ref["median_bad"]).double()
        assert (1 - keep_med).mean().item() <= 0.01
        assert rel_err(_masked(median[0, ..., 0], keep_med), _masked(ref["median"], keep_med)) <= TOL
    else:
        assert float(median.abs().max()) == 0.0
    if expected:
        assert nfd.shape == (1, H, W, 3) and float(nfd[0, 0].detach().abs().max()) == 0.0
        nfd_want = R.depth_to_normal(render[0, ..., -1:].detach().cpu().double(), sc["viewmat"].double(), sc["K"].double())
        assert rel_err(nfd[0].detach().cpu(), nfd_want) <= TOL

    # ---- gradients under the cotangent-weighted loss
    dev_keep = keep.to(cuda).float()
    loss = sum((got * cot[key].to(cuda).float() * (dev_keep if got.dim() == 2 else dev_keep[..., None])).sum() for key, got in images)
    loss.backward()
    got_grad = lambda key: torch.zeros_like(leaves[key]) if leaves[key].grad is None else leaves[key].grad
    errs = {key: rel_err(got_grad(key).cpu(), grads[key]) for key in ("means", "quats", "scales", "opacities", "sh")}
    # (the depth-only modes ignore the colours: no gradient reaches them on either side)
    assert (float(grads["sh"].abs().max()) == 0 and float(got_grad("sh").abs().max()) == 0) == (render_mode in ("D", "ED"))
    # the densification signal, row by row of the Gaussians both sides project (an undecided one touches left-out pixels only)
    errs["gradient_2dgs"] = rel_err(meta["gradient_2dgs"].grad.cpu()[rows_got], densify[rows_ref])
    assert float(densify[rows_ref].abs().max()) > 0
    assert all(e <= TOL for e in errs.values()), errs
    assert float(leaves["scales"].grad[:, 2].abs().max()) == 0.0
    invisible = torch.ones(N, dtype=torch.bool)
    invisible[ids_got] = False
    if invisible.any():
        assert float(leaves["means"].grad.cpu()[invisible].abs().max()) == 0.0
    assert float(meta["gradient_2dgs"].detach().abs().max()) == 0.0


def test_branches_clamp_and_skip_all_occur():
    """in the view from outside each branch of min(w3, w2) takes at least 5 % of the contributions (the view from inside is there for
    the culls: its surfels are large on screen); the clamp and the 1/255 skip occur in every scene, and the hand-placed scene has
    the clamp active on several contributions of either branch"""
    refs = [_reference(name)[1] for name in ("inside", "outside", "clamp")]
    assert refs[1]["lowpass_frac"] >= 0.05 and refs[1]["ray_frac"] >= 0.05, (refs[1]["lowpass_frac"], refs[1]["ray_frac"])
    assert all(r["n_clamped"] > 0 and r["n_skipped"] > 0 and r["lowpass_frac"] > 0 for r in refs)
    assert refs[2]["n_clamped_ray"] >= 5 and refs[2]["n_clamped_lowpass"] >= 4, (refs[2]["n_clamped_ray"], refs[2]["n_clamped_lowpass"])


def test_one_surfel_one_tile(cuda):
    f, W, H = 40.0, 16, 16
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    args = (torch.tensor([[0.0, 0.0, 2.0]]), torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.full((1, 3), 0.11), torch.tensor([0.8]),
            torch.tensor([[0.2, 0.5, 0.9]]))
    leaves = [a.to(cuda).requires_grad_(True) for a in args]
    render, alpha, normals, nfd, distort, median, meta = gs.rasterization_2dgs(*leaves, torch.eye(4, device=cuda)[None], K.to(cuda)[None], W, H,
                                                                               render_mode="RGB+D", distloss=True)
    ref = R.rasterization_2dgs(*[a.double() for a in args], torch.eye(4, dtype=torch.float64), K.double(), W, H, render_mode="RGB+D",
                               distloss=True)
    assert meta["gaussian_ids"].tolist() == [0] and meta["radii"].tolist() == ref["radii"].tolist() and nfd is None
    assert rel_err(alpha[0, ..., 0].detach().cpu(), ref["alpha"]) <= TOL and rel_err(render[0].detach().cpu(), ref["render"]) <= TOL
    assert float(distort.detach().abs().max()) == 0.0 and rel_err(median[0, ..., 0].cpu(), ref["median"]) <= TOL
    assert torch.allclose(normals[0, H // 2, W // 2].cpu(), torch.tensor([0.0, 0.0, -1.0]) * alpha[0, H // 2, W // 2].cpu(), atol=1e-6)
    (render.sum() + alpha.sum()).backward()
    assert all(torch.isfinite(l.grad).all() for l in leaves) and float(leaves[3].grad.abs().max()) > 0


def test_empty_view_and_errors(cuda):
    n = 8
    means = torch.zeros(n, 3, device=cuda)
    means[:, 2] = -5.0                                                     # all behind the camera
    leaves = [means.requires_grad_(True), torch.ones(n, 4, device=cuda), torch.full((n, 3), 0.1, device=cuda), torch.full((n,), 0.5, device=cuda),
              torch.rand(n, 3, device=cuda)]
    cam = (torch.eye(4, device=cuda)[None], torch.tensor([[[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]]], device=cuda), 32, 24)
    render, alpha, normals, nfd, distort, median, meta = gs.rasterization_2dgs(*leaves, *cam, render_mode="RGB+ED", distloss=True,
                                                                               backgrounds=torch.tensor([[0.1, 0.2, 0.3]], device=cuda))
    assert meta["gaussian_ids"].numel() == 0 and meta["gradient_2dgs"].shape == (0, 2) and meta["ray_transforms"].shape == (0, 3, 3)
    assert float(alpha.abs().max()) == 0.0 and float(distort.abs().max()) == 0.0 and float(median.abs().max()) == 0.0
    assert torch.allclose(render[0, ..., :3].cpu(), torch.tensor([0.1, 0.2, 0.3]).expand(24, 32, 3))
    (render.sum() + normals.sum()).backward()
    assert float(leaves[0].grad.abs().max()) == 0.0
    with pytest.raises(ValueError):
        gs.rasterization_2dgs(*leaves, *cam, render_mode="RGB", distloss=True)
    with pytest.raises(ValueError):
        gs.rasterization_2dgs(*leaves, *cam, render_mode="XYZ")
    with pytest.raises(ValueError):
        gs.rasterization_2dgs(*leaves, cam[0].repeat(2, 1, 1), cam[1].repeat(2, 1, 1), 32, 24)
    for flag in ("sparse_grad", "absgrad"):
        with pytest.raises(NotImplementedError):
            gs.rasterization_2dgs(*leaves, *cam, **{flag: True})
    with pytest.raises(ValueError):                                        # the 3DGS entry point still refuses the mode
        gs.rasterization_3dgs(*leaves, *cam, rasterize_mode="2dgs")
    r_d, _, _, nfd_d, dist_d, _, _ = gs.rasterization_2dgs(*leaves, *cam, render_mode="D")
    assert r_d.shape == (1, 24, 32, 1) and nfd_d is None and dist_d is None


def test_model_and_trainer(cuda):
    """thirty steps on an 8-view synthetic target with both regularisers on from the first step; one densify and one cull happen"""
    gen = torch.Generator().manual_seed(7)
    W = H = 64
    cams = gs.orbit_cameras(8, radius=3.0, pitch_degree=20.0, width=W, height=H, focal=70.0)
    target = gs.SurfelModel(gaussians=gs.GaussianSet.random(400, sh_degree=1, random_scale=0.7, device=cuda, generator=gen),
                            background_color="black", device=cuda).eval()
    with torch.no_grad():
        target.gaussians.opacities += 3.0
        target.gaussians.colors.copy_(torch.rand(400, 3, generator=gen))
        gts = [target.render_rgba(c.to(cuda)) for c in cams]
        depth = target.render_depth(cams[0].to(cuda))
    assert depth.shape == (H, W, 2) and float(depth[..., 1].max()) > 0.5 and target.update_info is None
    model = gs.SurfelModel(gaussians=gs.GaussianSet.random(600, sh_degree=1, random_scale=0.7, device=cuda, requires_grad=True, generator=gen),
                           background_color="black", prepare_densification=True, device=cuda)
    # (sh_degree_interval: degree 1 is active from step 5, so the SH rest has gradients and Adam moments before the refinements)
    trainer = gs.SurfelTrainer(warmup_length=2, refine_every=10, reset_alpha_every=30, stop_split_at=25, normal_start=0, distort_start=0,
                               sh_degree_interval=5, densify_grad_thresh=1e-5, cull_alpha_thresh=0.05,
                               generator=torch.Generator(device=cuda).manual_seed(1))
    trainer.setup(model, dataset_size=8)
    # dataset_size + refine_every < step % (reset_alpha_every * refine_every): the densify gate of step 20, the cull gate of step 30
    losses = []
    for step in range(1, 31):
        loss, metrics = trainer.train_step(model, cams[step % 8].to(cuda), gts[step % 8], curr_step=step)
        if step == 1:
            assert "normal" in metrics and "distort" in metrics
            assert float(model.update_info.xys.grad.abs().max()) > 0
        losses.append(float(loss))
    kinds = [k for _, k in trainer.refined]
    assert "densify" in kinds and "cull" in kinds, trainer.refined
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    g = model.gaussians
    n = len(g)
    for name, p in g.parameters().items():
        assert p.shape[0] == n and torch.isfinite(p).all(), name
        st = trainer.optimizers[name].state[p]
        assert {"exp_avg", "exp_avg_sq"} <= set(st), (name, sorted(st))
        for moment in ("exp_avg", "exp_avg_sq"):
            assert st[moment].shape == p.shape and torch.isfinite(st[moment]).all(), (name, moment)
