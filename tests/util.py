"""Shared helpers for the parity tests (scene builders, tolerances)."""
import math

import numpy as np
import torch

import geosplatting_amd.synthetic as syn
from oracle import mesh_ref
from geosplatting_amd.cameras import orbit_cameras


def rel_err(a, b):
    """max |a-b| / max |b|  (the '1e-4 relative fp32' of BASELINE.json is read as max-norm relative)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def elem_frac(a, b, rtol=1e-4, atol_rel=1e-6):
    """element-wise figure: fraction of elements with |a-b| > rtol*|b| + atol_rel*max|b|"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) > rtol * np.abs(b) + atol_rel * np.abs(b).max()).mean())


def activated(splats):
    """numpy (means, quats, scales_exp, opacities_sigmoid) like GSplatter.render_rgba does (rfstudio/model/gsplat.py:336-339)"""
    return (splats.means.numpy(), splats.quats.numpy(), splats.scales.exp().numpy(),
            torch.sigmoid(splats.opacities).squeeze(-1).numpy())


def sphere_case(level, res, view=1, seed=1, cubemap_res=64):
    # Gaussians from the CPU restatement (oracle/mesh_ref.py): the same scene with and without a GPU; the product's own
    # HIP-built scene is compared with it in tests/test_gpu_mesh.py::test_sphere_scene_hip_equals_restatement
    sc = syn.sphere_scene(level, seed=seed, cubemap_res=cubemap_res, mesh_to_splats_fn=mesh_ref.scene_builder)
    focal = 0.5 * res / math.tan(0.5 * 0.6911112)
    cam = orbit_cameras(8, 4.0 * (2.0 / 3.0), 30.0, res, res, focal=focal)[view]
    return sc, cam


def random_case(n, res, view=0, seed=1):
    sp = syn.random_splats(n, seed=seed)
    cam = orbit_cameras(4, 3.0, 30.0, res, res, hfov_degree=40.0)[view]
    return sp, cam


N_VIEWS, RES, LEVEL = 4, 160, 3      # the small engine scene of the parallel / ordering tests


def small_engine_scene():
    """(scene, cameras, upstream cotangents on the host) of the small engine tests: level-3 sphere from the CPU restatement
    (bit-identical Gaussians in every process), four 160 x 160 Blender-style views."""
    sc = syn.sphere_scene(LEVEL, seed=2, cubemap_res=64, mesh_to_splats_fn=mesh_ref.scene_builder)
    cams = syn.blender_cameras(N_VIEWS, RES, RES)
    ups = [torch.rand(RES, RES, 4, generator=torch.Generator().manual_seed(50 + i)) * 2 - 1 for i in range(N_VIEWS)]
    return sc, cams, ups


def same_step(ref, got):
    """Two runs of the same engine step, each (grads, images): images bit for bit (same kernels on the same inputs), gradients to
    5e-5 of their largest magnitude (the order of the float atomics)."""
    for a, b in zip(ref[1], got[1]):
        assert torch.equal(a, b)
    for k, w in ref[0].items():
        scale = w.abs().max().item() + 1e-30
        assert (got[0][k] - w).abs().max().item() / scale < 5e-5, k


def compare_grads(got, want, tol=2e-5):
    """Gradients of the fused paths against the op-by-op autograd decomposition (GEOSPLAT_SPLAT=ops): max-norm relative error
    below `tol`, 1e-4 for quats / scales / exposure."""
    for k, w in want.items():
        a = got[k]
        assert (a is None) == (w is None), k
        if w is None:
            continue
        scale = float(w.abs().max())
        if k == "quats" and want.get("scales") is not None:      # isotropic / flat splats: the rotation gradient is pure cancellation noise --
            scale = max(scale, float(want["scales"].abs().max()))   # measured against the natural size of a covariance-perturbation gradient
        err = float((a - w).abs().max()) / (scale + 1e-30)
        print(f"  {k:10s} {err:.2e}")
        assert err < (1e-4 if k in ("quats", "scales", "exposure") else tol), (k, err)
