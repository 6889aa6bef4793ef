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


# ----------------------------------------------------------------------------- compositor backward against the oracle's error budget
EPS32 = 2.0 ** -24
BUDGET_KAPPA = 16.0          # one constant for every kernel and scene: 4.8 x the worst ratio seen (tests/test_gpu_raster_budget.py)


def assert_within_budget(name, got, want, budget, kappa=BUDGET_KAPPA):
    """|got - want| <= kappa * 2^-24 * budget for EVERY element (budget from oracle.raster_bwd_budget, in units of 2^-24); an element
    whose budget is 0 was touched by no pair and must be exactly `want`.  Prints the worst ratio |got - want| / (2^-24 budget) and
    returns it."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64); budget = np.asarray(budget, dtype=np.float64)
    assert got.shape == want.shape == budget.shape, (name, got.shape, want.shape, budget.shape)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(budget > 0, err / (EPS32 * budget), np.where(err > 0, np.inf, 0.0))
    if ratio.size == 0:
        return 0.0
    worst = int(np.argmax(ratio))
    r = float(ratio.flat[worst])
    print(f"  {name:28s} worst |got-want|/(eps budget) {r:9.3f}   (kappa {kappa:g})")
    assert np.isfinite(r) and r <= kappa, (
        f"{name}: element {np.unravel_index(worst, got.shape)} got {got.flat[worst]:.9g} want {want.flat[worst]:.9g} "
        f"budget {budget.flat[worst]:.4g} eps: ratio {r:.3f} > kappa {kappa:g}")
    return r


def _screen_scene(name, W, H, u, v, sigma_px, z, opac, seed, background=None, focal=100.0):
    """Gaussians placed in screen space: identity view (camera looks along +z), pinhole K with `focal`; isotropic 3D scale
    sigma_px * z / focal so the projected standard deviation is about sigma_px pixels (before the 0.3 px^2 blur)."""
    u, v, z = (np.asarray(a, np.float64) for a in (u, v, z))
    cx, cy = W / 2.0, H / 2.0
    means = np.stack([(u - cx) * z / focal, (v - cy) * z / focal, z], 1).astype(np.float32)
    s = (np.asarray(sigma_px, np.float64) * z / focal).astype(np.float32)
    N = means.shape[0]
    rng = np.random.RandomState(seed + 1000)
    quats = rng.randn(N, 4).astype(np.float32)                       # (isotropic: the rotation does not matter, the projection normalises)
    return dict(name=name, W=W, H=H, means=means, quats=quats, scales=np.repeat(s[:, None], 3, 1),
                opacities=np.asarray(opac, np.float32), viewmat=np.eye(4, dtype=np.float32),
                K=np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1]], np.float32), seed=seed,
                background=None if background is None else np.asarray(background, np.float32))


def scene_colors(scene, D):
    """deterministic packed-input colours [N, D] of a budget scene, signed around 0.5 so that no channel is trivially positive"""
    return np.random.RandomState(scene["seed"] * 7 + D).uniform(-0.25, 1.25, (scene["means"].shape[0], D)).astype(np.float32)


def deep_stack_scene(seed=0, W=96, H=96, n=5000):
    """thousands of large low-opacity Gaussians over one region: lists longer than 4096, walks of hundreds of records back from
    T_final ~ 1e-4, dense batches whose pairs overflow the pair buffers"""
    r = np.random.RandomState(seed)
    return _screen_scene("deep_stack", W, H, r.uniform(0.3 * W, 0.7 * W, n), r.uniform(0.3 * H, 0.7 * H, n), r.uniform(6.0, 20.0, n),
                         r.uniform(2.0, 6.0, n), r.uniform(0.02, 0.06, n), seed)


def veil_scene(seed=0, W=96, H=96, n=1500, n_veil=14):
    """an opaque veil (packed opacity above the 0.999 clamp at the centres) in front of a deep stack: termination at many depths
    inside one quadrant, ill-conditioned 1 / (1 - alpha)"""
    r = np.random.RandomState(seed + 11)
    u = np.concatenate([np.floor(r.uniform(0.1 * W, 0.9 * W, n_veil)) + 0.5, r.uniform(0.2 * W, 0.8 * W, n)])
    v = np.concatenate([np.floor(r.uniform(0.1 * H, 0.9 * H, n_veil)) + 0.5, r.uniform(0.2 * H, 0.8 * H, n)])
    sig = np.concatenate([r.uniform(25.0, 40.0, n_veil), r.uniform(6.0, 20.0, n)])
    z = np.concatenate([r.uniform(1.5, 2.0, n_veil), r.uniform(2.0, 6.0, n)])
    op = np.concatenate([np.ones(n_veil), r.uniform(0.02, 0.06, n)])
    return _screen_scene("veil", W, H, u, v, sig, z, op, seed + 11)


def speckle_scene(seed=0, W=64, H=64, spots=20, per_spot=40):
    """sparse speckle: clusters of ~1 px Gaussians (walk trips with a handful of busy pixels) plus one large Gaussian sharing
    some of their tiles"""
    r = np.random.RandomState(seed + 23)
    cu = np.floor(r.uniform(4, W - 4, spots)) + 0.5; cv = np.floor(r.uniform(4, H - 4, spots)) + 0.5
    n = spots * per_spot
    u = np.concatenate([np.repeat(cu, per_spot) + r.uniform(-0.3, 0.3, n), [0.25 * W]])
    v = np.concatenate([np.repeat(cv, per_spot) + r.uniform(-0.3, 0.3, n), [0.25 * H]])
    sig = np.concatenate([r.uniform(0.3, 0.5, n), [12.0]])
    z = np.concatenate([r.uniform(2.0, 6.0, n), [4.0]])
    op = np.concatenate([r.uniform(0.1, 0.3, n), [0.5]])
    return _screen_scene("speckle", W, H, u, v, sig, z, op, seed + 23)


def ragged_scene(seed=0, W=97, H=61, n_heavy=2600, n_light=60):
    """97 x 61 (edge quadrants on both axes), one heavy corner beside empty tiles, a background colour"""
    r = np.random.RandomState(seed + 37)
    u = np.concatenate([r.uniform(10, 38, n_heavy), r.uniform(50, 75, n_light)])
    v = np.concatenate([r.uniform(10, 38, n_heavy), r.uniform(36, 60, n_light)])
    sig = np.concatenate([r.uniform(2.0, 8.0, n_heavy), r.uniform(1.0, 3.0, n_light)])
    z = r.uniform(2.0, 6.0, n_heavy + n_light)
    op = np.concatenate([r.uniform(0.05, 0.5, n_heavy), r.uniform(0.3, 0.9, n_light)])
    return _screen_scene("ragged", W, H, u, v, sig, z, op, seed + 37, background=[0.3, -0.2, 0.7])


BUDGET_SCENES = dict(deep_stack=deep_stack_scene, veil=veil_scene, speckle=speckle_scene, ragged=ragged_scene)


def budget_cotangents(kind, H, W, D, seed):
    """upstream cotangents (v_render [H,W,D], v_alpha [H,W]) of the budget tests: 'dense' random signed, 'alpha' (v_render = 0), or
    'sparse' (non-zero on 32 scattered pixels only: a pair credited to the wrong pixel or Gaussian cannot average out)"""
    r = np.random.RandomState(seed)
    vr = r.uniform(-1, 1, (H, W, D)).astype(np.float32); va = r.uniform(-1, 1, (H, W)).astype(np.float32)
    if kind == "alpha":
        vr[:] = 0.0
    elif kind == "sparse":
        keep = np.zeros(H * W, bool); keep[r.choice(H * W, 32, replace=False)] = True
        keep = keep.reshape(H, W)
        vr[~keep] = 0.0; va[~keep] = 0.0
    else:
        assert kind == "dense", kind
    return vr, va


def raster_pair_stats(W, H, means2d, conics, opacities, offsets, flatten_ids, last_ids, tile_size=16):
    """What the compositor backward sees of a view, recomputed from the forward's data (fp32 numpy, threshold-exact up to the
    exponential's last bit): tile list lengths, live pairs (alpha >= 1/255, index <= the pixel's last_ids) per 64 consecutive
    records that hit a quadrant (one wave's 8 x 8 pixels), the fewest pixels such a batch touches (among batches in which some pixel
    has three or more live pairs), distinct last_ids in one quadrant, and live pairs at the 0.999 clamp."""
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    off = np.asarray(offsets).reshape(-1).astype(np.int64)
    ends = np.append(off[1:], len(flatten_ids))
    lens = ends - off
    st = dict(max_list=int(lens.max()), min_list=int(lens.min()), max_live_per64=0, min_busy_pixels=None,
              max_distinct_last=0, clamped_live=0)
    for t in range(tw * th):
        if lens[t] == 0:
            continue
        ty, tx = divmod(t, tw)
        g = flatten_ids[off[t]:ends[t]]
        idx = np.arange(off[t], ends[t])
        ys, xs = np.meshgrid(np.arange(ty * tile_size, (ty + 1) * tile_size), np.arange(tx * tile_size, (tx + 1) * tile_size), indexing="ij")
        inside = (ys < H) & (xs < W)
        py = (ys.astype(np.float32) + np.float32(0.5)).reshape(-1, 1); px = (xs.astype(np.float32) + np.float32(0.5)).reshape(-1, 1)
        dx = means2d[g, 0][None] - px; dy = means2d[g, 1][None] - py
        ca, cb, cc = conics[g, 0][None], conics[g, 1][None], conics[g, 2][None]
        sig = np.float32(0.5) * ca * dx * dx + np.float32(0.5) * cc * dy * dy + cb * dx * dy
        ov = opacities[g][None] * np.exp(-sig)
        alpha = np.minimum(np.float32(0.999), ov)
        last = np.where(inside, last_ids[np.minimum(ys, H - 1), np.minimum(xs, W - 1)], -1).reshape(-1, 1)
        live = (sig >= 0) & (alpha >= np.float32(1.0 / 255.0)) & (idx[None] <= last) & inside.reshape(-1, 1)
        st["clamped_live"] += int((live & (alpha == np.float32(0.999))).sum())
        live = live.reshape(tile_size, tile_size, -1)
        for qy in range(2):
            for qx in range(2):
                q = live[qy * 8:(qy + 1) * 8, qx * 8:(qx + 1) * 8].reshape(64, -1)           # [pixel, record]
                qin = inside[qy * 8:(qy + 1) * 8, qx * 8:(qx + 1) * 8].reshape(64)
                if qin.any():
                    lq = last.reshape(tile_size, tile_size)[qy * 8:(qy + 1) * 8, qx * 8:(qx + 1) * 8].reshape(64)[qin]
                    st["max_distinct_last"] = max(st["max_distinct_last"], len(np.unique(lq)))
                hit = q.any(0)
                qh = q[:, hit]
                for b0 in range(0, qh.shape[1], 64):
                    blk = qh[:, b0:b0 + 64]
                    st["max_live_per64"] = max(st["max_live_per64"], int(blk.sum()))
                    per_pix = blk.sum(1)
                    if per_pix.max() >= 3:
                        busy = int((per_pix > 0).sum())
                        st["min_busy_pixels"] = busy if st["min_busy_pixels"] is None else min(st["min_busy_pixels"], busy)
    return st
