"""Adaptive density control on the device (csrc/gs_densify.hip, geosplatting_amd/gsplat3d.py) against the reference's own results
(tests/golden/ref_densify.npz), the plain-torch restatement (tests/densify_ref.py) and float64 error budgets.

Budgets (eps = 2^-23), from the arithmetic and not from what the kernels give:
  child mean_i   16 eps (|mean_i| + sum_j |R_ij| |exp(s_j) z_j|): the forward bound of a normalised-quaternion rotation (about 6
                 roundings), an `exp` of at most 2 ulp, two products, a three-term sum and one add;
  child scale    4 eps (1 + |s'|): an `exp` and a `log` of at most 2 ulp each around one exact-ish product.
Everything else (classes, totals, indices, copied rows, moments) is compared bit for bit.
"""
import math

import numpy as np
import pytest
import torch

from tests import densify_ref as ref
from tests.test_densify_cpu import EPS, check_against_golden, golden_kwargs, load_golden

pytestmark = pytest.mark.gpu
FIELDS = ref.FIELDS


def _set(P, dev, requires_grad=False):
    import geosplatting_amd as gs
    return gs.GaussianSet(**{k: torch.as_tensor(P[k]) for k in FIELDS}).to(dev).requires_grad_(requires_grad)


def _adam_with_state(param, exp_avg, exp_avg_sq, steps=1.0):
    opt = torch.optim.Adam([param], lr=1e-3, eps=1e-15)
    opt.state[param] = {"step": torch.tensor(steps), "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
    return opt


# ------------------------------------------------------------------------------------------------ the reference's golden
def test_golden_densify_and_cull(cuda):
    G = load_golden()
    g = _set(G, cuda, requires_grad=True)
    g.xys_grad_norm, g.vis_counts = torch.tensor(G["xys_grad_norm"], device=cuda), torch.tensor(G["vis_counts"], device=cuda)
    g.last_width, g.last_height = float(G["last_width"]), float(G["last_height"])
    sq = torch.rand(g.means.shape, device=cuda)
    opt = _adam_with_state(g.means, torch.tensor(G["exp_avg_before"], device=cuda), sq.clone())
    indices = g.densify_and_cull(randn=torch.tensor(G["randn"], device=cuda), optimizers={"means": opt}, **golden_kwargs(G))
    assert list(g.last_totals) == [int(v) for v in G["totals"]]
    assert indices.dtype == torch.int64 and g.requires_grad and g.xys_grad_norm is None
    check_against_golden(G, {k: getattr(g, k).detach().cpu().numpy() for k in FIELDS}, indices.cpu().numpy())
    # the Adam state followed in the same launch: kept rows bit for bit, every new row exactly 0, re-keyed to the new parameter
    assert opt.param_groups[0]["params"][0] is g.means and list(opt.state.keys()) == [g.means]
    st = opt.state[g.means]
    assert float(st["step"]) == 1.0
    assert np.array_equal(st["exp_avg"].cpu().numpy(), G["exp_avg_after"])
    kept = indices >= 0
    assert torch.equal(st["exp_avg_sq"][kept], sq[indices[kept]]) and not bool(st["exp_avg_sq"][~kept].any())
    assert not bool(st["exp_avg"][~kept].any())


def test_golden_cull(cuda):
    G = load_golden()
    g = _set(G, cuda)
    kept = g.cull(cull_alpha_thresh=float(G["cull_alpha_thresh"]), cull_scale_thresh=float(G["cull_scale_thresh"]))
    assert np.array_equal(kept.cpu().numpy(), G["cull_indices"])
    assert g.last_totals == (len(G["cull_indices"]), 0, 0, len(G["cull_indices"]))
    for name in FIELDS:
        assert np.array_equal(getattr(g, name).cpu().numpy(), G["cull_" + name]), name
    # without a scale threshold only the opacity culls
    g2 = _set(G, cuda)
    kept2 = g2.cull(cull_alpha_thresh=float(G["cull_alpha_thresh"]), cull_scale_thresh=None)
    want = (torch.tensor(G["opacities"]).sigmoid()[:, 0] >= float(G["cull_alpha_thresh"])).nonzero()[:, 0]
    assert torch.equal(kept2.cpu(), want)


# ------------------------------------------------------------------------------------------------ statistics
def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_densify_stats_from_a_rendered_view(cuda):
    """gs_densify_stats on the means2d gradient of rasterization_3dgs views.  Counts are exact; a norm is within 2 ulp of
    torch's `grad.norm(dim=-1)`; the second view is added onto the first (the sum of two fp32 addends that each differ by at most
    2 ulp can round one ulp apart, which is all the second comparison allows on top)."""
    import geosplatting_amd.synthetic as syn
    from geosplatting_amd.cameras import orbit_cameras
    from geosplatting_amd.gsplat3d import densify_stats
    from geosplatting_amd.shading import render_rgb
    n = 3000
    sp = syn.random_splats(n, seed=11)
    gen = torch.Generator().manual_seed(12)
    P = dict(means=sp.means, scales=sp.scales, quats=sp.quats, opacities=sp.opacities + 2.0, colors=sp.colors,
             shs=torch.randn(n, 15, 3, generator=gen) * 0.1)
    P = {k: v.clone().to(cuda).requires_grad_(True) for k, v in P.items()}
    cams = orbit_cameras(8, 3.0, 20.0, 96, 96, focal=110.0)
    xys, vis = torch.zeros(n, device=cuda), torch.ones(n, device=cuda)
    xys_ref, vis_ref = xys.clone(), vis.clone()
    target = torch.rand(96, 96, 3, generator=gen).to(cuda)
    first = None
    for view in (1, 5):
        rgb, info = render_rgb(P["means"], P["scales"], P["quats"], P["opacities"], P["colors"], cams[view], torch.zeros(3, device=cuda),
                               shs=P["shs"], sh_degree=3, rasterize_mode="classic", means2d_grad=True, return_meta=True)
        info["means2d"].retain_grad()
        (rgb - target).abs().mean().backward()
        grad, ids = info["means2d"].grad, info["gaussian_ids"]
        assert ids.numel() > n // 4 and ids.unique().numel() == ids.numel()
        before = xys.clone()
        densify_stats(ids, grad, xys, vis)
        ref.update_grad_norm(xys_ref, vis_ref, ids, grad)
        assert torch.equal(vis, vis_ref)
        norm = grad.norm(dim=-1).double().cpu().numpy()
        want = (before[ids] + grad.norm(dim=-1)).double().cpu().numpy()
        got = xys[ids].double().cpu().numpy()
        slack = 2 * _ulp(norm) + (0 if first is None else 1) * _ulp(want)
        assert (np.abs(got - want) <= slack).all(), float(np.abs(got - want).max())
        untouched = torch.ones(n, dtype=torch.bool, device=cuda)
        untouched[ids] = False
        assert torch.equal(xys[untouched], before[untouched])
        first = ids
    assert float(vis.max()) == 3.0 and float(xys.sum()) > 0
    # ids outside [0, N) are skipped
    x2, v2 = torch.zeros(4, device=cuda), torch.ones(4, device=cuda)
    densify_stats(torch.tensor([2, -1, 4, 0], device=cuda), torch.tensor([[3.0, 4.0]] * 4, device=cuda), x2, v2)
    assert x2.tolist() == [5.0, 0.0, 5.0, 0.0] and v2.tolist() == [2.0, 1.0, 2.0, 1.0]


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_against_densify_ref(cuda):
    n = 2_000_000
    P, xys, vis = ref.seeded_inputs(n, cuda, seed=31)
    frac = ref.mask_near_thresholds(P, xys, vis, 400.0, ref.SEEDED_KW)
    assert frac <= 1e-3, frac                                        # the seed keeps the mask below 0.1 % of the rows
    g = _set(P, cuda)
    g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height = xys.clone(), vis.clone(), 800, 600
    gen = torch.Generator(device=cuda).manual_seed(32)
    moments = {k: (torch.randn(P[k].shape, device=cuda, generator=gen), torch.rand(P[k].shape, device=cuda, generator=gen)) for k in FIELDS}
    opts = {k: _adam_with_state(getattr(g, k), moments[k][0].clone(), moments[k][1].clone(), steps=7.0) for k in FIELDS}
    sel, spl, dup, cul, _ = ref.classify(P, xys, vis, 400.0, ref.SEEDED_KW["densify_grad_thresh"], ref.SEEDED_KW["densify_size_thresh"],
                                         ref.SEEDED_KW["cull_alpha_thresh"], ref.SEEDED_KW["cull_scale_thresh"])
    n_sel, n_split, n_dup = int(sel.sum()), int(spl.sum()), int(dup.sum())
    assert min(n_sel, n_split, n_dup, int(cul.sum())) >= 0.10 * n and int((cul & (spl | dup)).sum()) >= 0.01 * n
    randn = torch.randn(2, n_split, 3, device=cuda, generator=gen)
    want, want_idx, _ = ref.densify_and_cull(P, xys, vis, 800, 600, randn=randn, **ref.SEEDED_KW)
    indices = g.densify_and_cull(randn=randn, optimizers=opts, **ref.SEEDED_KW)
    # invariants
    S = ref.SEEDED_KW["num_splits"]
    assert g.last_totals == (n_sel, n_split, n_dup, n_sel + S * n_split + n_dup) and len(g) == g.last_totals[3] == indices.numel()
    kept = indices[indices >= 0]
    assert kept.numel() == n_sel and bool((indices[:n_sel] >= 0).all()) and bool((indices[n_sel:] == -1).all())
    assert bool((kept[1:] > kept[:-1]).all())
    assert torch.equal(indices, want_idx)
    lo, hi = n_sel, n_sel + S * n_split
    for name in ("quats", "colors", "shs", "opacities"):
        assert torch.equal(getattr(g, name), want[name]), name
    for name in ("means", "scales"):
        assert torch.equal(getattr(g, name)[:lo], want[name][:lo]) and torch.equal(getattr(g, name)[hi:], want[name][hi:]), name
    # children against float64
    src = {k: P[k][spl].double() for k in ("means", "scales", "quats")}
    q = src["quats"] / src["quats"].norm(dim=-1, keepdim=True)
    R = ref.unit_quat_rotation(q)[None]                                                                    # [1, n, 3, 3]
    off = (src["scales"].exp()[None] * randn.double())[..., None, :]                              # [S, n, 1, 3]
    child = ((R * off).sum(-1) + src["means"][None]).reshape(-1, 3)
    tol = (16 * EPS * (src["means"].abs()[None] + (R.abs() * off.abs()).sum(-1))).reshape(-1, 3)
    cs = (src["scales"].exp() / 1.6).log()[None].expand(S, -1, -1).reshape(-1, 3)
    cs_tol = 4 * EPS * (1 + cs.abs())
    for got in (g, None):                                                                        # the kernels, then densify_ref itself
        m = (g.means if got is g else want["means"])[lo:hi].double()
        s = (g.scales if got is g else want["scales"])[lo:hi].double()
        print("full size, %s: worst child mean / budget %.3f, worst child scale / budget %.3f" % (
            "kernels" if got is g else "densify_ref", float(((m - child).abs() / tol).max()), float(((s - cs).abs() / cs_tol).max())))
        assert bool(((m - child).abs() <= tol).all()), float(((m - child).abs() / tol).max())
        assert bool(((s - cs).abs() <= cs_tol).all()), float(((s - cs).abs() / cs_tol).max())
    for name in FIELDS:
        st = opts[name].state[getattr(g, name)]
        assert float(st["step"]) == 7.0
        for item, m in zip(("exp_avg", "exp_avg_sq"), moments[name]):
            assert torch.equal(st[item], ref.mutate_moment(m, want_idx)), (name, item)


def test_degree_zero_set_refines(cuda):
    """SH degree 0 (shs [N, 0, 3]): densify_and_cull and cull move the five non-empty fields and keep the empty one empty"""
    n = 5000
    P, xys, vis = ref.seeded_inputs(n, cuda, seed=61)
    P["shs"] = torch.empty(n, 0, 3, device=cuda)
    g = _set(P, cuda, requires_grad=True)
    assert g.sh_degree == 0
    opts = {k: _adam_with_state(getattr(g, k), torch.ones_like(P[k]), torch.ones_like(P[k])) for k in FIELDS if k != "shs"}
    g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height = xys.clone(), vis.clone(), 800, 600
    gen = torch.Generator(device=cuda).manual_seed(62)
    n_split = int(ref.classify(P, xys, vis, 400.0, ref.SEEDED_KW["densify_grad_thresh"], ref.SEEDED_KW["densify_size_thresh"],
                               ref.SEEDED_KW["cull_alpha_thresh"], ref.SEEDED_KW["cull_scale_thresh"])[1].sum())
    randn = torch.randn(2, n_split, 3, device=cuda, generator=gen)
    want, want_idx, _ = ref.densify_and_cull(P, xys, vis, 800, 600, randn=randn, **ref.SEEDED_KW)
    indices = g.densify_and_cull(randn=randn, optimizers=opts, **ref.SEEDED_KW)
    assert g.last_totals[1] == n_split                                   # (no row of this seed sits within rounding of a threshold)
    assert torch.equal(indices, want_idx) and g.shs.shape == (indices.numel(), 0, 3) and g.shs.requires_grad
    for name in ("quats", "colors", "opacities"):
        assert torch.equal(getattr(g, name), want[name]), name
    # children carry their float64 budgets in the golden and full-size tests; here only that they were computed: |values| < 8, and
    # 16 eps * 8 on either side is below 4e-5
    assert torch.allclose(g.means, want["means"], rtol=0, atol=4e-5) and torch.allclose(g.scales, want["scales"], rtol=0, atol=4e-5)
    for k, opt in opts.items():
        assert opt.state[getattr(g, k)]["exp_avg"].shape == getattr(g, k).shape
    Q = {k: getattr(g, k).detach().clone() for k in FIELDS}
    want2, kept2 = ref.cull(Q, cull_alpha_thresh=0.3, cull_scale_thresh=None)
    kept = g.cull(cull_alpha_thresh=0.3, cull_scale_thresh=None, optimizers=opts)
    assert torch.equal(kept, kept2) and g.shs.shape == (kept.numel(), 0, 3)
    for name in FIELDS:
        assert torch.equal(getattr(g, name), want2[name]), name


# ------------------------------------------------------------------------------------------------ the optimiser
def test_adam_follows_a_refinement(cuda):
    import geosplatting_amd as gs
    n = 3000
    P, xys, vis = ref.seeded_inputs(n, cuda, seed=41)
    g = _set(P, cuda, requires_grad=True)
    opts = {k: torch.optim.Adam([getattr(g, k)], lr=1e-3, eps=1e-15) for k in FIELDS}
    gen = torch.Generator(device=cuda).manual_seed(42)

    def steps(count):
        for _ in range(count):
            for k in FIELDS:
                getattr(g, k).grad = torch.randn(getattr(g, k).shape, device=cuda, generator=gen)
                opts[k].step()
    steps(3)
    g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height = xys, vis, 800, 600
    before = {k: opts[k].state[getattr(g, k)]["exp_avg"].clone() for k in FIELDS}
    indices = g.densify_and_cull(optimizers=opts, generator=gen, **ref.SEEDED_KW)
    assert len(g) == indices.numel() != n
    kept = indices >= 0
    for k in FIELDS:
        p = getattr(g, k)
        assert opts[k].param_groups[0]["params"] == [p] and list(opts[k].state.keys()) == [p] and p.requires_grad and p.grad is None
        st = opts[k].state[p]
        assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"][kept], before[k][indices[kept]]) and not bool(st["exp_avg"][~kept].any())
    steps(2)
    assert all(float(opts[k].state[getattr(g, k)]["step"]) == 5.0 and bool(torch.isfinite(getattr(g, k)).all()) for k in FIELDS)
    # the plain form of mutate_adam (indices) equals the moved moments of the fused one
    P2 = {k: v.clone() for k, v in P.items()}
    m = torch.randn(n, 3, device=cuda, generator=gen)
    old = P2["means"].requires_grad_(True)
    o2 = torch.optim.Adam([old], lr=1e-3)
    o2.state[old] = {"step": torch.tensor(2.0), "exp_avg": m.clone(), "exp_avg_sq": m.abs()}
    idx = torch.tensor([5, 0, -1, 7, -1], device=cuda)
    new = torch.zeros(5, 3, device=cuda, requires_grad=True)
    gs.mutate_adam(o2, [new], indices=idx)
    assert list(o2.state.keys()) == [new] and torch.equal(o2.state[new]["exp_avg"], ref.mutate_moment(m, idx)) and float(o2.state[new]["step"]) == 2.0
    # reset_opacities clamps and clears only the opacity group
    g.reset_opacities(reset_value=0.2)
    assert float(g.opacities.detach().max()) <= math.log(0.2 / 0.8) + 1e-6
    gs.mutate_adam(opts["opacities"], [g.opacities], clear=True)
    for k in FIELDS:
        st = opts[k].state[getattr(g, k)]
        assert bool(st["exp_avg"].any()) == (k != "opacities") and bool(st["exp_avg_sq"].any()) == (k != "opacities")
        assert float(st["step"]) == 5.0
    # the statistics are gone after a refinement: a second one raises like the reference's assert
    g.clear_extras_()
    with pytest.raises(AssertionError):
        g.densify_and_cull(optimizers=opts, **ref.SEEDED_KW)


# ------------------------------------------------------------------------------------------------ the trainer
TRAINER_FIELDS = dict(warmup_length=40, refine_every=20, reset_alpha_every=5, sh_degree_interval=50, stop_split_at=260)
NUM_STEPS, NUM_VIEWS = 300, 8


def _hidden_views(cuda):
    import geosplatting_amd as gs
    from geosplatting_amd.cameras import orbit_cameras
    gen = torch.Generator().manual_seed(51)
    n = 400
    hidden = gs.GaussianSet(means=(torch.rand(n, 3, generator=gen) - 0.5) * 1.2, scales=torch.log(0.03 + 0.07 * torch.rand(n, 3, generator=gen)),
                            quats=torch.randn(n, 4, generator=gen), opacities=torch.full((n, 1), 2.0), colors=torch.rand(n, 3, generator=gen),
                            shs=torch.randn(n, 15, 3, generator=gen) * 0.05).to(cuda)
    cams = orbit_cameras(NUM_VIEWS, 3.0, 20.0, 64, 64, focal=80.0)
    model = gs.GSplatModel(gaussians=hidden, training=False)
    gts = []
    with torch.no_grad():
        for cam in cams:
            rgba = model.render_rgba(cam)
            gts.append(torch.cat((rgba[..., :3] / rgba[..., 3:].clamp(min=1e-6), rgba[..., 3:]), dim=-1).clamp(0, 1))
    return cams, gts


def _train(cuda, cams, gts, num_steps, use_ref):
    import geosplatting_amd as gs
    host = torch.Generator().manual_seed(52)
    model = gs.GSplatModel(num_random=1500, random_scale=0.8, sh_degree=3, prepare_densification=True, device=cuda, generator=host)
    trainer = gs.GSplatTrainer(generator=torch.Generator(device=cuda).manual_seed(53), **TRAINER_FIELDS)
    trainer.setup(model, dataset_size=NUM_VIEWS)
    if use_ref:
        def densify(model, scale_thresh):                               # the same event through tests/densify_ref.py
            g = model.gaussians
            P = {k: getattr(g, k).detach() for k in FIELDS}
            half = 0.5 * max(g.last_width, g.last_height)
            n_split = int(ref.classify(P, g.xys_grad_norm, g.vis_counts, half, trainer.densify_grad_thresh, trainer.densify_size_thresh,
                                       trainer.cull_alpha_thresh, scale_thresh)[1].sum())
            randn = torch.randn((trainer.num_splits, n_split, 3), device=cuda, generator=trainer.generator)
            new, idx, _ = ref.densify_and_cull(P, g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height, randn=randn,
                                               densify_grad_thresh=trainer.densify_grad_thresh, densify_size_thresh=trainer.densify_size_thresh,
                                               num_splits=trainer.num_splits, cull_alpha_thresh=trainer.cull_alpha_thresh,
                                               cull_scale_thresh=scale_thresh)
            for k in FIELDS:
                setattr(g, k, new[k].contiguous().requires_grad_(True))
                ref.mutate_adam(trainer.optimizers[k], [getattr(g, k)], indices=idx)
            g.clear_extras_()
            return idx
        trainer._densify = densify
    log = []
    for step in range(1, num_steps + 1):
        n_before = len(model.gaussians)
        loss, metrics = trainer.train_step(model, cams[(step - 1) % NUM_VIEWS], gts[(step - 1) % NUM_VIEWS], curr_step=step)
        assert metrics["#gaussians"] == n_before
        log.append(dict(step=step, loss=float(loss), psnr=float(metrics["psnr"]), n_before=n_before, n_after=len(model.gaussians),
                        totals=model.gaussians.last_totals))
    return trainer, model, log


def test_trainer_schedule_and_convergence(cuda):
    cams, gts = _hidden_views(cuda)
    trainer, model, log = _train(cuda, cams, gts, NUM_STEPS, use_ref=False)
    # the schedule of rfstudio/trainer/gsplat_trainer.py:178-225 evaluated here, in plain Python, from the scaled-down fields
    F, want = TRAINER_FIELDS, []
    interval = F["reset_alpha_every"] * F["refine_every"]
    for s in range(1, NUM_STEPS + 1):
        if not (s > F["warmup_length"] and s % F["refine_every"] == 0):
            continue
        if s < F["stop_split_at"] and s % interval > NUM_VIEWS + F["refine_every"]:
            want.append((s, "densify"))
        if s >= F["stop_split_at"]:
            want.append((s, "cull"))
        if s < F["stop_split_at"] and s % interval == F["refine_every"]:
            want.append((s, "reset"))
    assert trainer.refined == want
    densify_steps = [s for s, k in want if k == "densify"]
    cull_steps = [s for s, k in want if k == "cull"]
    assert len(densify_steps) >= 2 and len(cull_steps) >= 1 and sum(k == "reset" for _, k in want) >= 1
    print("refined:", want)
    print("#gaussians:", [(e["step"], e["n_before"], e["n_after"]) for e in log if e["n_before"] != e["n_after"]])
    print("psnr first / last:", log[0]["psnr"], log[-1]["psnr"])
    changed = [e["step"] for e in log if e["n_before"] != e["n_after"]]
    # #gaussians moves at the refinement steps and nowhere else; a refinement whose plan keeps every row and adds none (its totals
    # say so) is the only one that may leave the count as it was
    for e in log:
        if e["step"] in densify_steps or e["step"] in cull_steps:
            assert e["n_after"] == e["totals"][3]
            assert (e["n_before"] != e["n_after"]) == (e["totals"][3] != e["n_before"])
        else:
            assert e["n_before"] == e["n_after"], e
    assert set(changed) <= set(densify_steps) | set(cull_steps) and set(densify_steps) <= set(changed)
    assert all(math.isfinite(e["loss"]) for e in log)
    assert log[-1]["psnr"] > log[0]["psnr"], (log[0]["psnr"], log[-1]["psnr"])
    for k in FIELDS:
        assert bool(torch.isfinite(getattr(model.gaussians, k)).all())


def test_trainer_first_event_matches_densify_ref(cuda):
    """the run on the HIP ops and the run on tests/densify_ref.py (same seeds, same normal samples): equal N and equal indices up to and
    including the first densify event"""
    cams, gts = _hidden_views(cuda)
    first = 60
    a_tr, a_model, a_log = _train(cuda, cams, gts, first, use_ref=False)
    b_tr, b_model, b_log = _train(cuda, cams, gts, first, use_ref=True)
    assert a_tr.refined == b_tr.refined == [(first, "densify")]
    assert [e["n_after"] for e in a_log] == [e["n_after"] for e in b_log]
    assert torch.equal(a_tr.last_indices, b_tr.last_indices)
    assert len(a_model.gaussians) == len(b_model.gaussians) == a_tr.last_indices.numel()
