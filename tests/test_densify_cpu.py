"""No-GPU checks of the adaptive density control: the plain-torch restatement (tests/densify_ref.py) reproduces what the reference
wrote into tests/golden/ref_densify.npz, the three C entry points validate their arguments before any device work, the Python ops
refuse CPU tensors, and the PLY export reads back."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import densify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23
FIELDS = ref.FIELDS


def load_golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_densify.npz"))
    return {k: z[k] for k in z.files}


def child_bounds(G):
    """float64 evaluation of the children of the golden's split rows and the per-element error budgets of the issue:
    means 16 eps (|mean_i| + sum_j |R_ij| |exp(s_j) z_j|), scales 4 eps (1 + |s'|)."""
    n_sel, n_split, _, _ = (int(v) for v in G["totals"])
    S = int(G["num_splits"])
    # split rows in index order, from the inputs (float64 decisions agree with fp32: the golden keeps 1e-4 off every threshold)
    scale_max = np.exp(G["scales"].astype(np.float64)).max(-1)
    avg = 0.5 * max(float(G["last_width"]), float(G["last_height"])) * (G["xys_grad_norm"].astype(np.float64) / G["vis_counts"])
    split_rows = np.nonzero((avg > float(G["densify_grad_thresh"])) & (scale_max > float(G["densify_size_thresh"])))[0]
    assert split_rows.shape[0] == n_split
    q = G["quats"].astype(np.float64)[split_rows]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    R = ref.unit_quat_rotation(torch.from_numpy(q)).numpy()[None]                                              # float64, [1, n, 3, 3]
    off = np.exp(G["scales"].astype(np.float64)[split_rows])[None] * G["randn"].astype(np.float64)          # [S, n, 3]
    mean = G["means"].astype(np.float64)[split_rows][None]
    child_means = (R * off[..., None, :]).sum(-1) + mean
    means_tol = 16 * EPS * (np.abs(mean) + (np.abs(R) * np.abs(off[..., None, :])).sum(-1))
    child_scales = np.broadcast_to(np.log(np.exp(G["scales"].astype(np.float64)[split_rows]) / 1.6)[None], (S, n_split, 3))
    scales_tol = 4 * EPS * (1 + np.abs(child_scales))
    return (split_rows, child_means.reshape(-1, 3), means_tol.reshape(-1, 3), child_scales.reshape(-1, 3), scales_tol.reshape(-1, 3))


def check_against_golden(G, new, indices, prefix="out_"):
    """indices and every copied row bit for bit, the children within the budgets"""
    n_sel, n_split, n_dup, n_out = (int(v) for v in G["totals"])
    S = int(G["num_splits"])
    assert np.array_equal(indices, G["indices"])
    for name in ("quats", "colors", "shs", "opacities"):
        assert np.array_equal(new[name], G[prefix + name]), name
    lo, hi = n_sel, n_sel + S * n_split
    for name in ("means", "scales"):
        assert new[name].shape == G[prefix + name].shape
        assert np.array_equal(new[name][:lo], G[prefix + name][:lo]) and np.array_equal(new[name][hi:], G[prefix + name][hi:]), name
    _, cm, cm_tol, cs, cs_tol = child_bounds(G)
    for got in (new, {k[len(prefix):]: v for k, v in G.items() if k.startswith(prefix)}):     # the reference's own fp32 meets the budgets too
        assert (np.abs(got["means"][lo:hi].astype(np.float64) - cm) <= cm_tol).all()
        assert (np.abs(got["scales"][lo:hi].astype(np.float64) - cs) <= cs_tol).all()


def golden_params(G, device="cpu"):
    return {name: torch.tensor(G[name], device=device) for name in FIELDS}


def golden_kwargs(G):
    return dict(densify_grad_thresh=float(G["densify_grad_thresh"]), densify_size_thresh=float(G["densify_size_thresh"]),
                num_splits=int(G["num_splits"]), cull_alpha_thresh=float(G["cull_alpha_thresh"]),
                cull_scale_thresh=float(G["cull_scale_thresh"]))


def test_golden_conditions():
    """what the generator promised: mixed classes, culled-and-densified rows, every decision 1e-4 off its threshold"""
    G = load_golden()
    P = golden_params(G)
    kw = golden_kwargs(G)
    half = 0.5 * max(float(G["last_width"]), float(G["last_height"]))
    sel, spl, dup, cul, (avg, smax, alpha) = ref.classify(P, torch.tensor(G["xys_grad_norm"]), torch.tensor(G["vis_counts"]), half,
                                                          kw["densify_grad_thresh"], kw["densify_size_thresh"], kw["cull_alpha_thresh"],
                                                          kw["cull_scale_thresh"])
    n = P["means"].shape[0]
    assert 3500 <= n <= 4500 and P["shs"].shape[1:] == (15, 3)
    for m in (sel, spl, dup, cul):
        assert int(m.sum()) >= 0.10 * n
    assert int((cul & (spl | dup)).sum()) >= 0.01 * n
    for q, t in ((avg, kw["densify_grad_thresh"]), (smax, kw["densify_size_thresh"]), (smax, kw["cull_scale_thresh"]),
                 (alpha, kw["cull_alpha_thresh"])):
        assert bool(((q - t).abs() > 1e-4 * t).all())
    assert [int(sel.sum()), int(spl.sum()), int(dup.sum())] == [int(v) for v in G["totals"][:3]]


def test_densify_ref_reproduces_the_golden():
    G = load_golden()
    new, indices, _ = ref.densify_and_cull(golden_params(G), torch.tensor(G["xys_grad_norm"]), torch.tensor(G["vis_counts"]),
                                           float(G["last_width"]), float(G["last_height"]), randn=torch.tensor(G["randn"]),
                                           **golden_kwargs(G))
    check_against_golden(G, {k: v.numpy() for k, v in new.items()}, indices.numpy())
    culled, kept = ref.cull(golden_params(G), cull_alpha_thresh=float(G["cull_alpha_thresh"]), cull_scale_thresh=float(G["cull_scale_thresh"]))
    assert np.array_equal(kept.numpy(), G["cull_indices"])
    for name in FIELDS:
        assert np.array_equal(culled[name].numpy(), G["cull_" + name]), name
    assert np.array_equal(ref.mutate_moment(torch.tensor(G["exp_avg_before"]), indices).numpy(), G["exp_avg_after"])
    assert (G["exp_avg_after"][G["indices"] < 0] == 0).all() and np.abs(G["exp_avg_after"]).sum() > 0


def test_argument_validation_without_gpu():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    i64, f = C.c_int64, C.c_float
    assert lib.gs_densify_ws_bytes(i64(0), 2) == 0 and lib.gs_densify_ws_bytes(i64(1 << 28), 2) == 0
    assert lib.gs_densify_ws_bytes(i64(1000), 9) == 0
    assert lib.gs_densify_ws_bytes(i64(1 << 21), 2) >= (1 << 21) * (1 + 8) + 3 * 4 * (1 << 13)
    assert lib.gs_densify_ws_bytes(i64(1000), 3) > lib.gs_densify_ws_bytes(i64(1000), 2)
    # stats
    rc = lib.gs_densify_stats(-1, None, None, i64(10), None, None, None)
    assert rc == -1 and b"V must be" in lib.gs_last_error()
    rc = lib.gs_densify_stats(5, None, None, i64(10), None, None, None)
    assert rc == -1 and b"null pointer" in lib.gs_last_error()
    assert lib.gs_densify_stats(0, None, None, i64(10), None, None, None) == 0
    # plan
    th = (f(400.0), f(2e-4), f(0.01), f(0.1), f(0.5))
    rc = lib.gs_densify_plan(i64(0), None, None, None, None, *th, 2, 0, None, C.c_size_t(0), None, None)
    assert rc == -1 and b"N must be" in lib.gs_last_error()
    rc = lib.gs_densify_plan(i64(100), None, None, None, None, *th, 2, 7, None, C.c_size_t(0), None, None)
    assert rc == -1 and b"mode" in lib.gs_last_error()
    rc = lib.gs_densify_plan(i64(100), None, None, None, None, *th, 0, 0, None, C.c_size_t(0), None, None)
    assert rc == -1 and b"num_splits" in lib.gs_last_error()
    rc = lib.gs_densify_plan(i64(100), None, None, None, None, *th, 2, 0, None, C.c_size_t(1 << 20), None, None)
    assert rc == -1 and b"workspace" in lib.gs_last_error()
    # fill
    rc = lib.gs_densify_fill(i64(100), 2, None, C.c_size_t(0), i64(60), i64(50), i64(0), None, 0, None, None, None, None, None)
    assert rc == -1 and b"totals out of range" in lib.gs_last_error()
    rc = lib.gs_densify_fill(i64(100), 2, None, C.c_size_t(0), i64(50), i64(10), i64(5), None, 33, None, None, None, None, None)
    assert rc == -1 and b"n_tensors" in lib.gs_last_error()
    rc = lib.gs_densify_fill(i64(100), 2, None, C.c_size_t(0), i64(50), i64(10), i64(5), None, 2, None, None, None, None, None)
    assert rc == -1 and b"null table" in lib.gs_last_error()
    rc = lib.gs_densify_fill(i64(100), 2, None, C.c_size_t(0), i64(50), i64(10), i64(5), None, 0, None, None, None, None, None)
    assert rc == -1 and b"workspace" in lib.gs_last_error()


def test_gaussian_set_refuses_cpu_tensors():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    from geosplatting_amd.gsplat3d import densify_stats
    g = gs.GaussianSet.random(64, sh_degree=3, random_scale=1.0, generator=torch.Generator().manual_seed(0))
    assert len(g) == 64 and g.sh_degree == 3 and g.shs.shape == (64, 15, 3) and g.opacities.shape == (64, 1)
    assert torch.allclose(g.opacities.sigmoid(), torch.full((64, 1), 0.1)) and bool((g.colors == 0.5).all())
    assert bool((g.scales[:, 0] == g.scales[:, 1]).all()) and bool(torch.isfinite(g.scales).all())
    g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height = torch.zeros(64), torch.ones(64), 64, 64
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        g.densify_and_cull(densify_grad_thresh=2e-4, densify_size_thresh=0.01, num_splits=2, cull_alpha_thresh=0.1, cull_scale_thresh=None)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        g.cull(cull_alpha_thresh=0.1, cull_scale_thresh=0.5)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        g.reset_opacities(reset_value=0.2)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        densify_stats(torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2), g.xys_grad_norm, g.vis_counts)
    g.clear_extras_()
    assert g.xys_grad_norm is None and g.vis_counts is None and g.last_width is None
    assert sorted(g.state_dict()) == ["colors", "means", "opacities", "quats", "scales", "shs"]
    model = gs.GSplatModel(gaussians=g, rasterize_mode="2dgs")
    with pytest.raises(NotImplementedError):
        model.render_rgb(None)


def test_knn_matches_brute_force():
    from geosplatting_amd.gsplat3d import knn_mean_distance
    p = torch.rand(300, 3, generator=torch.Generator().manual_seed(3))
    d = torch.cdist(p.double(), p.double())
    d.fill_diagonal_(float("inf"))
    want = d.sort(dim=-1).values[:, :3].mean(-1).float()
    assert torch.allclose(knn_mean_distance(p, 3, chunk=64), want, rtol=1e-6, atol=0)


def test_refine_schedule_defaults():
    """the gates GSplatTrainer.after_update runs on, at the reference's default fields, against the reference's conditions written
    out here (rfstudio/trainer/gsplat_trainer.py:178-225): densify from 600, none in the window after an opacity reset, post cull
    from 15000, cull_scale_thresh only after step 3000"""
    from geosplatting_amd.gsplat3d import refine_schedule
    kw = dict(warmup_length=500, refine_every=100, reset_alpha_every=30, stop_split_at=15000, dataset_size=100)
    for step in range(1, 16001):
        got = refine_schedule(step, **kw)
        on = step > 500 and step % 100 == 0
        assert got["refine"] == on
        assert got["densify"] == (on and step < 15000 and step % 3000 > 200)
        assert got["cull"] == (on and step >= 15000)
        assert got["reset"] == (on and step < 15000 and step % 3000 == 100)
        assert got["scale_cull"] == (step > 3000)
    assert not refine_schedule(500, **kw)["refine"] and refine_schedule(600, **kw)["densify"]
    assert refine_schedule(3100, **kw)["reset"] and not refine_schedule(3200, **kw)["densify"] and refine_schedule(3300, **kw)["densify"]
    assert not refine_schedule(15000, continue_cull_post_densification=False, **kw)["cull"]


def test_ply_export_reads_back(tmp_path):
    import geosplatting_amd as gs
    gen = torch.Generator().manual_seed(5)
    n = 37
    g = gs.GaussianSet(means=torch.randn(n, 3, generator=gen), scales=torch.randn(n, 3, generator=gen), quats=torch.randn(n, 4, generator=gen),
                       opacities=torch.randn(n, 1, generator=gen), colors=torch.rand(n, 3, generator=gen), shs=torch.zeros(n, 15, 3))
    path = tmp_path / "g.ply"
    g.export_point_cloud(path)
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == f"element vertex {n}"
    props = [l.split() for l in lines[3:] if l]
    assert all(p[0] == "property" and p[1] == "float" for p in props)
    assert [p[2] for p in props] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1",
                                     "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    data = np.frombuffer(body, dtype="<f4").reshape(n, 17)
    assert np.array_equal(data[:, 0:3], g.means.numpy()) and not data[:, 3:6].any()
    assert np.array_equal(data[:, 6:9], ((g.colors - 0.5) / 0.28209479177387814).numpy())
    assert np.array_equal(data[:, 9:10], g.opacities.numpy()) and np.array_equal(data[:, 10:13], g.scales.numpy())
    assert np.array_equal(data[:, 13:17], (g.quats / g.quats.norm(dim=-1, keepdim=True)).numpy())
