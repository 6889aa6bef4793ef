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
# The projection backward (tests/test_gpu_project_budget.py) has a constant of its own, set from two measurements: (a) the fp32 oracle
# against float64 autograd on the CPU (tests/test_oracle_cpu.py, bar kappa / 2): worst ratio 1.00; (b) the kernels on an MI355X: worst
# ratio 0.54.  Kappa is the smallest power of two that is at least 4 x (b).  The budget there is a rigorous running-error bound, so a
# correct implementation stays near or below 1 whatever the compiler does; the compositor's budget is not of that kind (its worst
# ratio is 3.31), and sharing its 16 would leave 30 x headroom here.
PROJ_BUDGET_KAPPA = 4.0
# The surfel projection and the SH colours (tests/test_gpu_surfel_project_budget.py, reference and budgets in
# tests/surfel_project_ref.py), by the same rule -- the smallest power of two that is at least 4 x the larger of (a) the float32
# restatement against float64 on the CPU (tests/test_surfel_project_cpu.py, bar kappa / 2) and (b) the kernels on an MI355X:
# SURFEL_PROJ_KAPPA (projection forward and backward): (a) 0.70 (ray_transforms / depths; gradients 0.55), (b) 0.85 (ray_transforms of
# the 131 372-row compaction scene; gradients 0.64).  SH_KAPPA (SH colours and coefficient gradients): (a) 0.996, (b) 0.996 -- a
# degree-0 colour is two roundings and a rounded literal against a bound of exactly those.  The scene builders of
# tests/surfel_project_ref.py redraw every Gaussian with a decision margin below 2 * max(kappa) bounds.
SURFEL_PROJ_KAPPA = 4.0
SH_KAPPA = 4.0


# The surfel compositor backward (tests/test_gpu_surfel_budget.py) is measured against the per-pair restatement of tests/surfel_ref.py
# (composite_pairs).  Its budget B is NOT the plain absolute sum over the pixels: it also sums the sizes of the terms that meet within
# one pair (the derivation is in composite_pairs' docstring), and is typically 2 to 20 times the plain sum, far more for single elements.
# So kappa * 2^-24 * B is a per-element bound, but not the project's 1e-4 of sum_p |grad|.  Two constants, both by the rule above:
# SURFEL_BUDGET_KAPPA, every element against B: (a) the restatement in float32 against itself in float64 on the CPU, every case of
# surfel_ref.PAIR_CASES under its three cotangents (tests/test_surfel_cpu.py, bar kappa / 2): worst ratio 110.7 ('outside', C = 1,
# tile 16, sparse; 'clamp' 25, the stack scenes 21); kappa is the smallest power of two that is at least 4 x (a).
# SURFEL_PLAIN_MEDIAN_KAPPA, the MEDIAN element of each gradient against the plain sum (surfel_ref.plain_ratio_medians): (a) worst
# median 6.95; the constant is the smallest power of two that is at least 4 x (a), and 32 * 2^-24 = 1.9e-6.
# The "float32" run of (a) is not float32 throughout: hu = p M2 - M0, hv and hu x hv are formed in float64 and rounded once, forward and
# backward, where the kernels use explicit FMAs and a compensated difference of products in the forward but plain fp32 cross products in
# the backward; (a) is lower than an all-float32 run would give (without it, 245 on 'outside' dense and 440 on 'clamp').
# (b) the kernels on an MI355X: the tables in the docstring of tests/test_gpu_surfel_budget.py.
SURFEL_BUDGET_KAPPA = 512.0
SURFEL_PLAIN_MEDIAN_KAPPA = 32.0


def assert_within_budget(name, got, want, budget, kappa=BUDGET_KAPPA):
    """|got - want| <= kappa * 2^-24 * budget for EVERY element (budget from oracle.raster_bwd_budget / oracle.project_bwd_budget, in
    units of 2^-24); an element whose budget is 0 was touched by no pair (is culled, or has only zero cotangents) and must be exactly
    `want`; a budget that is not finite checks nothing and is refused.  Prints the worst ratio |got - want| / (2^-24 budget) and
    returns it."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64); budget = np.asarray(budget, dtype=np.float64)
    assert got.shape == want.shape == budget.shape, (name, got.shape, want.shape, budget.shape)
    assert np.isfinite(budget).all() and np.isfinite(got).all() and np.isfinite(want).all(), name
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


# ----------------------------------------------------------------------------- projection backward against the oracle's error budget
PROJ_NEAR = 0.01                         # near plane of every projection-budget scene
PROJ_REGIMES = ("plain", "near", "clamp_x", "clamp_y", "clamp_xy", "tiny", "aniso", "iso", "qnorm", "flat")


def proj_camera(yaw, pitch, roll, pos, W, H, fx, fy, cx, cy):
    """a rotated and translated pinhole camera (OpenCV axes): dict(viewmat [4,4] f32 world->camera, K [3,3] f32, W, H)"""
    cy_, sy = math.cos(yaw), math.sin(yaw); cp, sp = math.cos(pitch), math.sin(pitch); cr, sr = math.cos(roll), math.sin(roll)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]]); Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    R = (Ry @ Rx @ Rz).T                                               # world -> camera
    vm = np.eye(4); vm[:3, :3] = R; vm[:3, 3] = -R @ np.asarray(pos, np.float64)
    return dict(viewmat=vm.astype(np.float32), K=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), W=W, H=H)


def proj_limits(view):
    """(lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg) of the tan-fov clamp of a view, float64"""
    K, W, H = view["K"].astype(np.float64), view["W"], view["H"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return (W - cx) / fx + 0.15 * W / fx, cx / fx + 0.15 * W / fx, (H - cy) / fy + 0.15 * H / fy, cy / fy + 0.15 * H / fy


def proj_cam_coords(scene, view):
    """camera-space means [N,3] of a scene in a view (float64 arithmetic on the fp32 inputs)"""
    vm = view["viewmat"].astype(np.float64)
    return scene["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]


def proj_margins_ok(scene, view, rel=1e-3):
    """per Gaussian: every decision of the projection has a margin -- z is `rel` away from the near plane and, in front of it,
    x/z and y/z are `rel` away from both clamp limits -- so that fp32 and float64, or a division and a hardware reciprocal, decide
    alike"""
    mc = proj_cam_coords(scene, view)
    z = mc[:, 2]
    ok = np.abs(z / PROJ_NEAR - 1.0) >= rel
    front = z > PROJ_NEAR
    zs = np.where(front, z, 1.0)
    lxp, lxn, lyp, lyn = proj_limits(view)
    for r, (lp, ln) in ((mc[:, 0] / zs, (lxp, lxn)), (mc[:, 1] / zs, (lyp, lyn))):
        ok &= ~front | ((np.abs(r - lp) >= rel * lp) & (np.abs(r + ln) >= rel * ln))
    return ok


def _rand_quats(r, n):
    q = r.randn(n, 4)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _proj_regime(r, name, n, view, smin):
    """n Gaussians of one regime in the CAMERA space of `view`: (mean_c [n,3], quats [n,4], scales [n,3]); projected sizes are
    chosen in pixels (sigma_px) and turned into scales by z / focal"""
    K, W, H = view["K"].astype(np.float64), view["W"], view["H"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    f = math.sqrt(fx * fy)
    lxp, lxn, lyp, lyn = proj_limits(view)
    z = r.uniform(2.0, 6.0, n)
    xr = (r.uniform(0.05 * W, 0.95 * W, n) - cx) / fx            # x / z, on screen
    yr = (r.uniform(0.05 * H, 0.95 * H, n) - cy) / fy
    quats = _rand_quats(r, n)
    sig = r.uniform(max(smin, 1.2), 8.0, n)                       # pixels
    ratio = r.uniform(0.6, 1.6, (n, 3))                           # mild anisotropy
    if name == "plain":
        sig = r.uniform(smin, 8.0, n)
    elif name == "near":
        z = PROJ_NEAR * np.exp(r.uniform(math.log(1.02), math.log(9.5), n))
        sig = r.uniform(1.5, 6.0, n)
    elif name in ("clamp_x", "clamp_y", "clamp_xy"):
        k = r.uniform(1.02, 1.35, (n, 2)); side = r.rand(n, 2) < 0.5
        ox = np.where(side[:, 0], lxp * k[:, 0], -lxn * k[:, 0]); oy = np.where(side[:, 1], lyp * k[:, 1], -lyn * k[:, 1])
        dx = np.where(side[:, 0], fx * ox + cx - W, -(fx * ox + cx)); dy = np.where(side[:, 1], fy * oy + cy - H, -(fy * oy + cy))
        if name == "clamp_x":
            xr, d = ox, dx
        elif name == "clamp_y":
            yr, d = oy, dy
        else:
            xr, yr, d = ox, oy, np.maximum(dx, dy)
        sig = d / 1.5 + 12.0                                       # large radii: the centre is off screen, the Gaussian is not
        ratio = r.uniform(0.8, 1.25, (n, 3))
    elif name == "tiny":
        sig = np.exp(r.uniform(math.log(0.004), math.log(0.085), n))  # comp ~ sig^2 / 0.3: 5e-5 ... 0.04
        ratio = r.uniform(0.8, 1.25, (n, 3))
    elif name == "aniso":
        sig = r.uniform(5.0, 40.0, n)
        ratio = np.stack([np.ones(n), 10.0 ** r.uniform(-4.0, 0.0, n), 10.0 ** r.uniform(-4.0, 0.0, n)], 1)
        ratio = np.take_along_axis(ratio, np.argsort(r.rand(n, 3), axis=1), 1)
    elif name == "iso":
        ratio = np.ones((n, 3))
    elif name == "qnorm":
        quats = quats * np.exp(r.uniform(math.log(1e-3), math.log(1e3), n))[:, None]
        quats[0] *= 1e-3 / np.linalg.norm(quats[0]); quats[1] *= 1e3 / np.linalg.norm(quats[1])
    elif name == "flat":
        ratio[:, 2] = 1.0
    else:
        raise KeyError(name)
    scales = (sig * z / f)[:, None] * ratio
    if name == "flat":
        scales[:, 2] = math.exp(-10.0)
    return np.stack([xr * z, yr * z, z], 1), quats, scales


def _proj_culled(r, n, view, radius_clip):
    """n Gaussians no view of the forward keeps: behind the camera, between the camera and the near plane, off screen, and (with a
    radius clip) too small"""
    W, H = view["W"], view["H"]
    K = view["K"].astype(np.float64)
    lxp, lxn, lyp, lyn = proj_limits(view)
    mc, quats, scales = _proj_regime(r, "plain", n, view, 1.2)
    kind = np.arange(n) % (4 if radius_clip > 0 else 3)
    mc[kind == 0] *= -1.0                                                           # behind the camera
    m = kind == 1                                                                   # in front of it, before the near plane
    zn = PROJ_NEAR * r.uniform(0.1, 0.99, m.sum())
    mc[m] *= (zn / mc[m, 2])[:, None]; scales[m] *= (zn / (mc[m, 2] + 4.0))[:, None]
    m = kind == 2                                                                   # beyond the clamp limit, small: off screen
    mc[m, 0] = lxp * r.uniform(1.05, 1.3, m.sum()) * mc[m, 2]
    scales[m] = (r.uniform(1.2, 2.0, m.sum()) * mc[m, 2] / math.sqrt(K[0, 0] * K[1, 1]))[:, None] * np.ones(3)
    m = kind == 3                                                                   # radius 2 (the blur alone): below a radius clip of 3
    scales[m] = (r.uniform(0.01, 0.1, m.sum()) * mc[m, 2] / math.sqrt(K[0, 0] * K[1, 1]))[:, None] * np.ones(3)
    return mc, quats, scales, kind


def proj_budget_scene(name, views, n_per=260, n_culled=400, radius_clip=0.0, seed=0):
    """A projection-budget scene: n_per Gaussians of every regime of PROJ_REGIMES placed in the camera space of views[0] and mapped
    back through that camera, culled Gaussians interleaved (one random order).  With several views, Gaussians that sit within the
    decision margin of ANY view are replaced at construction (the builder draws again), so no Gaussian of the scene is ever excluded
    from a check.  dict(means, quats, scales, opacities, views, radius_clip, regime [N] (index into PROJ_REGIMES, -1 = built to be
    culled), seed); the regimes and margins are asserted by proj_scene_forward."""
    r = np.random.RandomState(1000 + seed)
    v0 = views[0]
    vm = v0["viewmat"].astype(np.float64)
    smin = 0.4 if radius_clip == 0.0 else 1.2
    parts = [(i, n_per) for i in range(len(PROJ_REGIMES))] + [(-1, n_culled)]
    means, quats, scales, regime = [], [], [], []
    for reg, n in parts:
        have = 0
        for attempt in range(20):
            if reg >= 0:
                mc, q, s = _proj_regime(r, PROJ_REGIMES[reg], n, v0, smin)
            else:
                mc, q, s, _ = _proj_culled(r, n, v0, radius_clip)
            m = ((mc - vm[:3, 3]) @ vm[:3, :3]).astype(np.float32)
            trial = dict(means=m)
            ok = np.ones(n, bool)
            for vw in views:
                ok &= proj_margins_ok(trial, vw, rel=2e-3)
            take = np.nonzero(ok)[0][:n - have]
            means.append(m[take]); quats.append(q[take]); scales.append(s[take]); regime.append(np.full(len(take), reg))
            have += len(take)
            if have == n:
                break
        assert have == n, (name, reg, have)
    means, quats, scales, regime = (np.concatenate(a) for a in (means, quats, scales, regime))
    order = r.permutation(len(regime))
    sc = dict(name=name, means=means[order].astype(np.float32), quats=quats[order].astype(np.float32),
              scales=scales[order].astype(np.float32), regime=regime[order], views=views, radius_clip=float(radius_clip), seed=seed)
    sc["opacities"] = r.uniform(0.05, 1.0, len(order)).astype(np.float32)
    return sc


def proj_scene_forward(sc, view_index=0, check_regimes=True):
    """oracle.project_fwd of a projection-budget scene in one of its views, with the decision margins asserted for EVERY Gaussian
    and (view 0, which the scene was placed in) every regime of the scene asserted on the forward's outputs, so that a later change
    cannot silently stop covering it.  Returns the oracle's dict."""
    import oracle
    vw = sc["views"][view_index]
    W, H, clip = vw["W"], vw["H"], sc["radius_clip"]
    assert W % 16 and H % 16 and W != H
    K = vw["K"]
    assert K[0, 0] != K[1, 1] and abs(K[0, 2] - W / 2) > 1 and abs(K[1, 2] - H / 2) > 1
    assert proj_margins_ok(sc, vw).all()
    m = oracle.project_fwd(sc["means"], sc["quats"], sc["scales"], vw["viewmat"], K, W, H, near=PROJ_NEAR, radius_clip=clip)
    gid = m["gaussian_ids"]
    vis = np.zeros(len(sc["regime"]), bool); vis[gid] = True
    if clip > 0:                                                   # every radius at least 1 away from the clip
        m0 = oracle.project_fwd(sc["means"], sc["quats"], sc["scales"], vw["viewmat"], K, W, H, near=PROJ_NEAR, radius_clip=0.0)
        assert (np.abs(m0["radii"] - clip) >= 1).all()
        assert len(m0["gaussian_ids"]) > len(gid)                  # ... and the clip culls some
    reg = sc["regime"]
    assert not vis[reg < 0].any() or view_index > 0                # built to be culled
    culled_between = (~vis[:-1] & vis[1:]).sum()
    assert culled_between > 50 or view_index > 0                   # culled rows interleaved with visible ones
    mc = proj_cam_coords(sc, vw)
    xr, yr, z = mc[:, 0] / mc[:, 2], mc[:, 1] / mc[:, 2], mc[:, 2]
    lxp, lxn, lyp, lyn = proj_limits(vw)
    in_x = (xr <= lxp) & (xr >= -lxn); in_y = (yr <= lyp) & (yr >= -lyn)
    comp = np.full(len(reg), np.nan); comp[gid] = m["compensations"]
    if view_index > 0:
        # another camera on a scene placed for view 0: what it must still drive, counted on ITS visible Gaussians -- each clamp route,
        # the near plane, comp -> 0 -- so that a later change of a camera cannot silently empty these
        routes = [(in_x & in_y), (~in_x & in_y), (in_x & ~in_y), (~in_x & ~in_y)]
        counts = [int((r & vis).sum()) for r in routes] + [int((vis & (z < 10 * PROJ_NEAR)).sum()), int((comp < 0.05).sum())]
        assert min(counts) >= 30, (sc["name"], view_index, counts)
    if not (check_regimes and view_index == 0):
        return m
    con = np.full((len(reg), 3), np.nan); con[gid] = m["conics"]
    sel = lambda nm: reg == PROJ_REGIMES.index(nm)
    tiny_culled = clip > 0                                          # (radius 2: the tiny regime is what a radius clip removes)
    for nm in PROJ_REGIMES:
        assert vis[sel(nm)].all() or (nm == "tiny" and tiny_culled), (sc["name"], nm, int((~vis[sel(nm)]).sum()))
    s = sel("plain"); assert (in_x & in_y)[s].all() and (comp[s] > 0.2).all() and (comp[s] < 0.999).all()
    s = sel("near"); assert ((z[s] > PROJ_NEAR) & (z[s] < 10 * PROJ_NEAR)).all()
    s = sel("clamp_x"); assert (~in_x & in_y)[s].all() and (xr[s] > lxp).sum() > 20 and (xr[s] < -lxn).sum() > 20
    s = sel("clamp_y"); assert (in_x & ~in_y)[s].all() and (yr[s] > lyp).sum() > 20 and (yr[s] < -lyn).sum() > 20
    s = sel("clamp_xy"); assert (~in_x & ~in_y)[s].all()
    for a in (xr[s] > lxp, xr[s] < -lxn):
        for b in (yr[s] > lyp, yr[s] < -lyn):
            assert (a & b).sum() > 10
    if not tiny_culled:
        s = sel("tiny"); assert (comp[s] < 0.05).all() and (comp[s] < 1e-3).sum() > 10 and (comp[s] > 0).all()
    s = sel("aniso")
    sr = sc["scales"][s].min(1) / sc["scales"][s].max(1)
    assert sr.min() < 2e-4 and (con[s, 1] ** 2 > 0.99 * con[s, 0] * con[s, 2]).sum() > 5
    s = sel("iso"); assert (sc["scales"][s] == sc["scales"][s][:, :1]).all()
    s = sel("qnorm"); qn = np.linalg.norm(sc["quats"][s].astype(np.float64), axis=1)
    assert qn.min() < 1.1e-3 and qn.max() > 0.9e3
    s = sel("flat"); assert (sc["scales"][s, 2] == np.float32(math.exp(-10.0))).all()
    return m


def _proj_views_single(which):
    if which == "yaw":        # 200 x 120, yawed by 0.4 rad
        return [proj_camera(0.4, 0.0, 0.0, (0.5, -0.2, -1.0), 200, 120, 150.0, 170.0, 90.0, 70.0)]
    return [proj_camera(-0.7, 0.35, 0.2, (-1.5, 0.8, 0.3), 187, 333, 260.0, 230.0, 101.0, 150.0)]


def _proj_views_multi():
    """eight different cameras around one scene: small changes of pose (so that the regimes of view 0 survive in part) and of
    intrinsics and image size"""
    r = np.random.RandomState(77)
    views = [proj_camera(0.4, 0.0, 0.0, (0.5, -0.2, -1.0), 200, 120, 150.0, 170.0, 90.0, 70.0)]
    for i in range(7):
        W, H = (200 + 7 * i, 120 + 5 * i)
        views.append(proj_camera(0.4 + r.uniform(-0.25, 0.25), r.uniform(-0.2, 0.2), r.uniform(-0.3, 0.3),
                                 (0.5 + r.uniform(-0.02, 0.02), -0.2 + r.uniform(-0.02, 0.02), -1.0 + r.uniform(-0.03, 0.03)), W, H,
                                 150.0 + 6 * i, 170.0 - 3 * i, 90.0 + 3 * i, 70.0 + 1.5 * i))
    return views


PROJ_BUDGET_SCENES = dict(
    yaw=lambda: proj_budget_scene("yaw", _proj_views_single("yaw"), seed=0),
    tilt_clip=lambda: proj_budget_scene("tilt_clip", _proj_views_single("tilt"), radius_clip=3.0, seed=1),
    orbit8=lambda: proj_budget_scene("orbit8", _proj_views_multi(), n_per=200, n_culled=300, seed=2))

PROJ_COTANGENTS = ("dense", "geometry", "opacity", "depth")


def proj_budget_cotangents(kind, V, seed):
    """packed cotangents of the projection budget tests: (v_means2d [V,2], v_conics [V,3], v_opacities [V], v_depths [V] or None);
    'dense' random signed, 'geometry' (v_opacities = 0), 'opacity' (only the compensation path is live), 'depth' (dense, with
    v_depths); in every kind each seventh row is all zeros (a Gaussian that reached no pixel: its gradients must be exactly 0)"""
    r = np.random.RandomState(seed)
    vm = r.uniform(-1, 1, (V, 2)).astype(np.float32); vc = r.uniform(-1, 1, (V, 3)).astype(np.float32)
    vo = r.uniform(-1, 1, V).astype(np.float32); vd = r.uniform(-1, 1, V).astype(np.float32)
    if kind == "geometry":
        vo[:] = 0.0
    elif kind == "opacity":
        vm[:] = 0.0; vc[:] = 0.0
    else:
        assert kind in ("dense", "depth"), kind
    for a in (vm, vc, vo, vd):
        a[3::7] = 0.0
    return vm, vc, vo, (vd if kind == "depth" else None)


# ----------------------------------------------------------------------------- shading backward against the oracle's error budget
# tests/test_gpu_shade_budget.py.  The constant follows the rule written beside PROJ_BUDGET_KAPPA: the smallest power of two that is
# at least 4 x the worst ratio the kernels show on an MI355X; the CPU test (oracle against float64 autograd) has the bar kappa / 2.
# Measured: (a) the fp32 oracle against float64 autograd on the CPU: worst ratio 0.28 (v_normals; v_means 0.09, v_kd 0.20, v_ks 0.20,
# texels 0.25); (b) the kernels on an MI355X: gs_shade_bwd / gs_tail_bwd per-Gaussian gradients 0.00 (the oracle's bits), their texel
# sums 0.97 (over a pre-filled pattern, with the test's own n |p| term; 0.04 over zeros); the lean pair path of gs_tail_bwd_multi
# 0.41 (v_kd), texels 0.04.
SHADE_BUDGET_KAPPA = 4.0

_CUBE_FACES = ((2, 1, 0, -1.0, -1.0), (2, 1, 0, 1.0, -1.0), (0, 2, 1, 1.0, 1.0), (0, 2, 1, 1.0, -1.0), (0, 1, 2, 1.0, -1.0), (0, 1, 2, -1.0, -1.0))


def cube_face_point(s, x, y):
    """direction [n,3] of the face coordinates (x, y) of face s (face_point of oracle/gs_oracle_shade.c), float64, not normalised"""
    one = np.ones_like(x)
    return np.stack([(one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one)][s], -1)


def cube_face_coords(d):
    """(face, xn, yn) of directions [n,3] in float64 (select_face / cube_footprint of the oracle); face -1 for a zero direction"""
    d = np.asarray(d, np.float64)
    ax, ay, az = np.abs(d).T
    f = np.where(az > np.maximum(ax, ay), 4, np.where(ay > ax, 2, 0))
    c = np.where(f == 4, d[:, 2], np.where(f == 2, d[:, 1], d[:, 0]))
    f = f + (c < 0)
    xn = np.zeros(len(d)); yn = np.zeros(len(d))
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, (a, b, cc, sx, sy) in enumerate(_CUBE_FACES):
            m = f == s
            xn[m] = sx * d[m, a] / np.abs(d[m, cc]); yn[m] = sy * d[m, b] / np.abs(d[m, cc])
    return np.where(np.abs(d).max(1) > 0, f, -1), xn, yn


SHADE_DIR_REGIMES = tuple(f"face{s}" for s in range(6)) + tuple(f"edge{s}{e}" for s in range(6) for e in range(4)) + \
    tuple(f"corner{s}{k}" for s in range(6) for k in range(4)) + ("axis",)
# Gaussians placed exactly ON a decision boundary, where the arithmetic is exact in fp32 and in float64 alike (roughness = ks[0] with
# min_roughness = 0, compared with constants both sides hold as the same fp32 values): regime -> the margin slots that may be 0
SHADE_ON_BOUNDARY = dict(r_eq_min=("rough", "lam"), r_eq_max=("rough", "lam"), r_eq_one=("rough", "lam"))


def _shade_env(levels_res, base_res, seed):
    """signed texels with magnitudes spread over three decades"""
    r = np.random.RandomState(4000 + seed)
    tex = lambda R: (r.randn(6, R, R, 3) * 10.0 ** r.uniform(-2.0, 1.0, (6, R, R, 1))).astype(np.float32)
    return tex(base_res), [tex(R) for R in levels_res]


def shade_budget_scene(name, mode, levels_res=(64, 32, 16), base_res=16, min_roughness=0.0, max_metallic=1.0, env_min_r=0.08,
                       env_max_r=0.5, random_lut=False, n_per=34, n_pile=300, seed=0, geometry=None):
    """A shading-budget scene for one mode: per-Gaussian inputs (no rasterisation) built regime by regime, `regime` [N] naming the
    regime each Gaussian was built for.  The lookup direction (the normal in 'diffuse', the reflection vector otherwise) drives
    the cube regimes of SHADE_DIR_REGIMES; the others are 'zero_normal' (diffuse), the FG-LUT clamps 'ndv_hi' / 'rough_hi', the view
    regimes 'backface' / 'grazing' / 'tiny_d' (0 < d < 1e-6, exact: the camera straight above along z) / 'at_camera' / 'len' (1e-3
    .. 1e3), the mip regimes 'r_lt_min' / 'r_eq_min' (integer level, f == 0) / 'seg_lo' / 'r_eq_max' / 'seg_hi' / 'r_eq_one', the
    materials 'metal0' / 'metal1' / 'kd_dark', 'plain', and the pile-ups 'pile_a' / 'pile_b' (hundreds of footprints on the same few
    texels).  Candidates whose selections sit within their error bound of a boundary are dropped at construction (the builder draws
    half as many again), those of SHADE_ON_BOUNDARY excepted.  geometry = (means, [cam_pos, ...]): keep the given means (the regimes
    that place the mean are left out; the direction regimes are built for the first camera, the margins hold for every camera) --
    the tail kernels' scenes, whose Gaussians come from a projection scene.  shade_scene_check
    asserts the regimes and the margins."""
    import oracle
    r = np.random.RandomState(3000 + seed)
    base, levels = _shade_env(levels_res, base_res, seed)
    f32 = lambda x: float(np.float32(x))
    opts = dict(min_roughness=f32(min_roughness), max_metallic=f32(max_metallic), env_min_roughness=f32(env_min_r),
                env_max_roughness=f32(env_max_r))
    if random_lut:
        lut = r.uniform(0.0, 1.0, (256, 256, 2)).astype(np.float32)
    else:
        import geosplatting_amd as gs
        lut = gs.get_fg_lut(torch.device("cpu"))[0].numpy()
    Rmax = max(levels_res) if mode != "diffuse" else base_res
    cam = np.array([0.3, -0.2, 2.5], np.float32).astype(np.float64) if geometry is None else np.asarray(geometry[1][0], np.float64)
    regs = list(SHADE_DIR_REGIMES) + ["ndv_hi", "rough_hi", "backface", "grazing", "r_lt_min", "seg_lo", "seg_hi", "metal0", "metal1",
                                      "kd_dark", "plain"]
    if min_roughness == 0.0:                                       # roughness = ks[0] exactly: it can sit ON a boundary
        regs += ["r_eq_min", "r_eq_max", "r_eq_one"]
    if mode == "diffuse":
        regs.append("zero_normal")
    if geometry is None:
        regs += ["tiny_d", "at_camera", "len"]
    elif mode != "diffuse":
        regs.remove("axis")                                        # (an exactly axis-aligned reflection needs the view along the axis)
    counts = [(g, n_per) for g in regs] + [("pile_a", n_pile), ("pile_b", n_pile)]
    pile_dirs = dict(pile_a=np.array([0.31, 0.22, 1.0]), pile_b=np.array([-1.0, 0.4, -0.15]))
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)

    def draw(g, n, given_means):
        s = r.randint(0, 6, n); xn = r.uniform(-0.8, 0.8, n); yn = r.uniform(-0.8, 0.8, n)
        near = lambda k: r.uniform(1.0 - 0.9 / Rmax, 1.0 - 0.02 / Rmax, k)
        if g.startswith("face"):
            s[:] = int(g[4])
        elif g.startswith("edge"):
            s[:] = int(g[4]); e = int(g[5])
            if e < 2:
                xn = near(n) * (1 if e == 1 else -1)
            else:
                yn = near(n) * (1 if e == 3 else -1)
        elif g.startswith("corner"):
            s[:] = int(g[6]); k = int(g[7])
            xn = near(n) * (1 if k & 1 else -1); yn = near(n) * (1 if k & 2 else -1)
        elif g == "axis":
            xn[:] = 0.0; yn[:] = 0.0; s = np.arange(n) % 6
        D = np.zeros((n, 3))
        for f in range(6):
            m = s == f
            D[m] = cube_face_point(f, xn[m], yn[m])
        if g != "axis":
            D = unit(D)
        if g in pile_dirs:
            D = unit(pile_dirs[g] + 0.004 * r.randn(n, 3))
        if given_means is None:
            w = unit(r.randn(n, 3))
            w = np.where((w * D).sum(-1, keepdims=True) < -0.4, -w, w)
            ln = r.uniform(1.5, 4.0, n)
            if g == "len":
                ln = 10.0 ** r.permutation(np.linspace(-3.0, 3.0, n))
            if g == "axis":
                w = D.copy()                                                   # the view along the normal: the reflection is the axis itself
            if g == "tiny_d":
                w = np.tile([0.0, 0.0, 1.0], (n, 1)); ln = r.randint(1, 5, n).astype(np.float64)
            means = (cam - w * ln[:, None]).astype(np.float32)
            if g == "at_camera":
                means = np.tile(cam.astype(np.float32), (n, 1))
            if g == "axis":                                                    # exact: one coordinate differs from the camera's
                means = np.tile(cam.astype(np.float32), (n, 1)).astype(np.float64)
                means = (means - D * r.randint(1, 4, n)[:, None]).astype(np.float32)
        else:
            means = given_means
        v = cam - means.astype(np.float64)
        ln = np.linalg.norm(v, axis=-1, keepdims=True)
        wo = np.where(ln < 1e-6, [0.0, 0.0, 1.0], v / np.maximum(ln, 1e-6))
        if given_means is not None:                                            # keep the reflection away from -wo: mirror the target
            D = np.where((wo * D).sum(-1, keepdims=True) < -0.4, -D, D) if not (g.startswith(("face", "edge", "corner", "pile")) or g == "axis") else D
        normals = D.copy() if mode == "diffuse" else unit(D + wo)
        if g == "axis" and mode != "diffuse":
            normals = D.copy()
        perp = unit(np.cross(wo, unit(r.randn(n, 3))))
        if g == "backface":
            normals = unit(-wo * r.uniform(0.1, 1.0, (n, 1)) + perp)
        elif g == "grazing":
            normals = unit(perp + wo * r.uniform(1e-5, 1e-3, (n, 1)))
        elif g == "ndv_hi":
            normals = unit(wo + perp * r.uniform(0.0, 0.03, (n, 1)))
        elif g == "tiny_d":
            phi = r.uniform(0, 2 * np.pi, n)
            normals = np.stack([np.cos(phi), np.sin(phi), r.uniform(1e-7, 9e-7, n)], -1)
        elif g == "zero_normal":
            normals = np.zeros((n, 3))
        ks = np.stack([r.uniform(0.1, 0.95, n), r.uniform(0.05, 0.95, n)], -1)
        if g in SHADE_DIR_REGIMES or g in pile_dirs:                 # roughness stratified: every direction regime reaches every level
            ks[:, 0] = r.permutation(np.linspace(0.1, 0.95, n))
        kd = r.uniform(0.1, 0.9, (n, 3))
        ksr = lambda rough: (np.float32(rough) - np.float32(min_roughness)) / (np.float32(1.0) - np.float32(min_roughness))
        if g == "rough_hi":
            ks[:, 0] = r.uniform(0.9985, 1.0, n)
        elif g == "r_lt_min":
            ks[:, 0] = r.uniform(0.0, ksr(env_min_r) * 0.9, n)
        elif g == "r_eq_min":
            ks[:, 0] = ksr(env_min_r)
        elif g == "seg_lo":
            ks[:, 0] = r.uniform(ksr(env_min_r) * 1.05 + 0.01, ksr(env_max_r) * 0.98, n)
        elif g == "r_eq_max":
            ks[:, 0] = ksr(env_max_r)
        elif g == "seg_hi":
            ks[:, 0] = r.uniform(ksr(env_max_r) * 1.02, 0.99, n)
        elif g == "r_eq_one":
            ks[:, 0] = 1.0
        elif g == "metal0":
            ks[:, 1] = 0.0
        elif g == "metal1":
            ks[:, 1] = 1.0
        elif g == "kd_dark":
            kd = r.uniform(0.0, 0.04, (n, 3))
        return means, normals.astype(np.float32), kd.astype(np.float32), ks.astype(np.float32)

    cams = [cam] if geometry is None else [np.asarray(c, np.float64) for c in geometry[1]]
    if geometry is not None:                                       # rows beyond the regimes' blocks: plain
        rest = len(geometry[0]) - sum(n for _, n in counts)
        assert rest >= 0, (name, rest)
        counts += [("plain", rest)] if rest else []

    def margins_ok(g, means, normals, kd, ks):
        ok = np.ones(len(means), bool)
        cot = np.ones((len(means), 3), np.float32)
        for c in cams:
            mg = oracle.shade_bwd_budget(means, normals, kd, ks, c.astype(np.float32), lut, base, levels, cot, mode=mode,
                                         return_margins=True, **opts)[2]
            ok &= _shade_margins_ok(mg, [g] * len(means))
        return ok

    parts = []
    at = 0
    for g, n in counts:
        if geometry is None:
            k = n + n // 2
            means, normals, kd, ks = draw(g, k, None)
            take = np.nonzero(margins_ok(g, means, normals, kd, ks))[0][:n]
            assert len(take) == n, (name, mode, g, len(take))
            means, normals, kd, ks = means[take], normals[take], kd[take], ks[take]
        else:                                                      # every row keeps its mean: rows that fail are drawn again
            gm = np.asarray(geometry[0], np.float32)[at:at + n]
            means, normals, kd, ks = draw(g, n, gm)
            for attempt in range(12):
                bad = ~margins_ok(g, means, normals, kd, ks)
                if not bad.any():
                    break
                _, n2, kd2, ks2 = draw(g, n, gm)
                normals[bad], kd[bad], ks[bad] = n2[bad], kd2[bad], ks2[bad]
            assert not bad.any(), (name, mode, g, int(bad.sum()))
        parts.append((means, normals, kd, ks, [g] * n))
        at += n
    cat = lambda i: np.concatenate([p[i] for p in parts])
    regime = np.array(sum((p[4] for p in parts), []))
    order = r.permutation(len(regime)) if geometry is None else np.arange(len(regime))
    return dict(name=name, mode=mode, means=cat(0)[order], normals=cat(1)[order], kd=cat(2)[order], ks=cat(3)[order],
                cam_pos=cam.astype(np.float32), regime=regime[order], lut=lut, base=base, levels=levels, opts=opts, seed=seed)


def _shade_margins_ok(margins, regime):
    """per Gaussian: every selection margin exceeds its forward error bound (a quantity that is exact and not on a boundary has bound
    0 or a margin far above it), the slots SHADE_ON_BOUNDARY lists for the Gaussian's regime excepted"""
    import oracle
    ok = np.ones(len(regime), bool)
    for j, slot in enumerate(oracle.SHADE_MARGINS):
        good = margins[:, j, 0] > 2.0 * margins[:, j, 1]
        exempt = np.array([slot in SHADE_ON_BOUNDARY.get(g, ()) for g in regime])
        ok &= good | exempt
    return ok


def shade_scene_check(sc):
    """Asserts on the oracle's forward of a shading-budget scene that every selection margin exceeds (twice) its error bound -- so
    that fp32, float64 and a kernel with a one-ulp reciprocal select alike -- and that every regime the scene names really occurs
    in at least 30 Gaussians.  Returns the margins."""
    import oracle
    N = len(sc["regime"])
    cot = np.ones((N, 3), np.float32)
    _, _, mg = oracle.shade_bwd_budget(sc["means"], sc["normals"], sc["kd"], sc["ks"], sc["cam_pos"], sc["lut"], sc["base"], sc["levels"],
                                       cot, mode=sc["mode"], return_margins=True, **sc["opts"])
    bad = ~_shade_margins_ok(mg, sc["regime"])
    assert not bad.any(), (sc["name"], sc["mode"], sorted(set(sc["regime"][bad])))
    for g, slots in SHADE_ON_BOUNDARY.items():                        # ... and those really sit ON the boundary
        m = sc["regime"] == g
        if m.any() and sc["mode"] != "diffuse":
            assert (mg[m, 4, 0] == 0).all(), g
    # ---- the regimes, recomputed in float64 from the fp32 inputs
    o = sc["opts"]
    cam = sc["cam_pos"].astype(np.float64)
    v = cam - sc["means"].astype(np.float64)
    ln = np.linalg.norm(v, axis=-1)
    wo = np.where(ln[:, None] < 1e-6, [0.0, 0.0, 1.0], v / np.maximum(ln, 1e-6)[:, None])
    nrm = sc["normals"].astype(np.float64)
    d = (nrm * wo).sum(-1)
    D = nrm if sc["mode"] == "diffuse" else 2.0 * d[:, None] * nrm - wo
    face, xn, yn = cube_face_coords(D)
    rough = sc["ks"][:, 0].astype(np.float64) * (1.0 - o["min_roughness"]) + o["min_roughness"]
    metal = sc["ks"][:, 1].astype(np.float64) * o["max_metallic"]
    res = [sc["base"].shape[1]] if sc["mode"] == "diffuse" else [l.shape[1] for l in sc["levels"]]
    L = len(sc["levels"])
    over = lambda c, R: ((c + 1) * 0.5 * R - 0.5 < 0) | ((c + 1) * 0.5 * R - 0.5 > R - 1)
    ox = np.all([over(xn, R) for R in res], 0); oy = np.all([over(yn, R) for R in res], 0)          # at EVERY level in use
    ix = ~np.any([over(xn, R) for R in res], 0); iy = ~np.any([over(yn, R) for R in res], 0)
    pred = {}
    for s in range(6):
        pred[f"face{s}"] = (face == s) & ix & iy
        for e in range(4):
            side = (xn < 0, xn > 0, yn < 0, yn > 0)[e]
            pred[f"edge{s}{e}"] = (face == s) & side & ((ox & iy) if e < 2 else (oy & ix))
        for k in range(4):
            pred[f"corner{s}{k}"] = (face == s) & ox & oy & ((xn > 0) == bool(k & 1)) & ((yn > 0) == bool(k & 2))
    pred["axis"] = (np.abs(D) > 0).sum(1) == 1
    pred["zero_normal"] = face < 0
    pred["ndv_hi"] = d > 1.0 - 1.0 / 512.0
    pred["rough_hi"] = rough > 1.0 - 1.0 / 512.0
    pred["backface"] = d < 0
    pred["grazing"] = (d > 1e-6) & (d < 1e-3)
    pred["tiny_d"] = (d > 0) & (d < 1e-6)
    pred["at_camera"] = ln == 0
    pred["len"] = np.ones(N, bool)
    emin, emax = o["env_min_roughness"], o["env_max_roughness"]
    pred["r_lt_min"] = rough < emin
    pred["r_eq_min"] = rough == emin
    pred["seg_lo"] = (rough > emin) & (rough < emax)
    pred["r_eq_max"] = rough == emax
    pred["seg_hi"] = (rough > emax) & (rough < 1.0)
    pred["r_eq_one"] = rough == 1.0
    pred["metal0"] = metal == 0
    pred["metal1"] = metal == o["max_metallic"]
    pred["kd_dark"] = (sc["kd"] < 0.04).all(1)
    pred["plain"] = (sc["kd"] > 0.04).all(1)
    pred["pile_a"] = pred["pile_b"] = np.ones(N, bool)
    names = sorted(set(sc["regime"]))
    for g in names:
        m = sc["regime"] == g
        assert m.sum() >= 30 and pred[g][m].all(), (sc["name"], sc["mode"], g, int(m.sum()), int((~pred[g][m]).sum()))
    if "len" in names:
        m = sc["regime"] == "len"
        assert ln[m].min() < 1e-2 and ln[m].max() > 1e2
    for g in ("pile_a", "pile_b"):                                    # hundreds of footprints on a handful of texels of every level
        m = sc["regime"] == g
        for R in res:
            tx = np.floor((xn[m] + 1) * 0.5 * R - 0.5); ty = np.floor((yn[m] + 1) * 0.5 * R - 0.5)
            assert len(set(zip(face[m], tx, ty))) <= 9 and m.sum() >= 100, (g, R)
    if sc["mode"] != "diffuse":                                       # every direction regime is fetched at EVERY level (as l0 or l1)
        lam = np.array([oracle.mip_from_roughness(x, emin, emax, L) for x in (sc["ks"][:, 0] * np.float32(1.0 - o["min_roughness"])
                                                                             + np.float32(o["min_roughness"]))])
        l0 = np.minimum(np.floor(np.clip(lam, 0, L - 1)), L - 1).astype(int)
        l1 = np.where(l0 >= L - 1, -1, l0 + 1)
        for g in names:
            if g in SHADE_DIR_REGIMES or g.startswith("pile"):
                m = sc["regime"] == g
                per_level = [int(((l0[m] == l) | (l1[m] == l)).sum()) for l in range(L)]
                assert min(per_level) >= 3, (sc["name"], g, per_level)
    if sc["mode"] != "diffuse" and L > 2:                             # both mip segments, and an integer level with f == 0
        lam5 = mg[:, 5, 0]
        assert (lam5[sc["regime"] == "r_eq_min"] == 0).all()
    return mg


SHADE_BUDGET_SCENES = dict(
    # (64, 32, 16) + base 16: two levels in LDS, one through HBM atomics; min_roughness = 0 so that roughness < env min occurs
    env3=dict(modes=("pbr", "specular", "diffuse"), kw=dict(levels_res=(64, 32, 16), base_res=16, seed=0)),
    # four levels, a caller-supplied random FG table, max_metallic < 1, min_roughness > 0
    env4=dict(modes=("pbr",), kw=dict(levels_res=(128, 64, 32, 16), base_res=16, min_roughness=0.03125, max_metallic=0.875,
                                      random_lut=True, seed=1)),
    # diffuse with a 64^2 base: the base outside LDS
    base64=dict(modes=("diffuse",), kw=dict(levels_res=(32, 16), base_res=64, seed=2)),
    # a single level (L = 1): always the last level
    single16=dict(modes=("specular",), kw=dict(levels_res=(16,), base_res=16, seed=3)))

SHADE_COTANGENTS = ("dense", "channel", "decades")


def shade_budget_cotangents(kind, N, seed):
    """colour cotangents [N,3] of the shading budget tests: 'dense' random signed, 'channel' (one channel per row live), 'decades'
    (row amplitudes spread over six decades); in every kind each seventh row is all zeros (a Gaussian that reached no pixel: its
    gradients must be exactly 0 and it must touch no texel)"""
    r = np.random.RandomState(seed)
    v = r.uniform(-1, 1, (N, 3)).astype(np.float32)
    if kind == "channel":
        keep = r.randint(0, 3, N)
        v = r.uniform(-1, 1, (N, 3)).astype(np.float32) * (np.arange(3)[None] == keep[:, None])
    elif kind == "decades":
        v = (v * 10.0 ** r.uniform(-3.0, 3.0, (N, 1))).astype(np.float32)
    else:
        assert kind == "dense", kind
    v = v.astype(np.float32)
    v[3::7] = 0.0
    return v


# ----------------------------------------------------------------------------- hash-grid field against the oracle's error budget
# (tests/test_gpu_field_budget.py, tests/test_oracle_cpu.py).  Kappa: the smallest power of two that is at least 4 x the worst ratio
# seen on an MI355X over every case of test_gpu_field_budget.py (0.999, a sum on top of a pre-filled pattern; 0.84 over zeros: the table
# in its docstring); the CPU bar is kappa / 2 (worst 0.98 there).
FIELD_BUDGET_KAPPA = 4.0
FIELD_REGIMES = ("uniform", "mesh_order", "lattice", "plus_one", "minus_one", "outside", "pile", "dead")
FIELD_COTANGENTS = ("dense", "one_level", "decades", "level_off")
FIELD_TGS = (1.0, 16.0, -3.0)
# (num_levels, log2 of the rows per level) -> what the shape drives in csrc/gs_hashgrid.hip
FIELD_BUDGET_SCENES = dict(
    L16_T10=(16, 10),        # slab rows == T, parts = 16
    L2_T14=(2, 14),          # one slab per level, parts = 64
    L16_T15=(16, 15),        # fixed-point minimum (4 slabs per level); float slabs with parts = 8
    L4_T19=(4, 19),          # fixed-point maximum (64 slabs per level: bit 63 of the binning mask)
    L16_T18=(16, 18),        # float slabs with parts == 1; the GaussianField shape
    L3_T20=(3, 20),          # fixed point refused (ws_bytes == 0); float slabs with parts == 1
    L1_T12=(1, 12),          # a single level
    L32_T12=(32, 12))        # GS_HG_MAX_LEVELS
FIELD_SCENE_N = 4367         # odd: divisible by no `parts`; past PU * blockDim = 4096 of the slab loops
FIELD_N_BOUNDARIES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, FIELD_SCENE_N)


def field_budget_scene(name, n=None, dyadic=False, seed=0):
    """Points for the hash-grid budget tests, the regimes interleaved and labelled per point (sc['regime']): uniform points; runs
    of 64, 100 and 300 consecutive points inside ONE cell of level 0, then of level min(4, L - 1) ('mesh_order', what the wave
    pre-aggregation of the atomic kernel was written for); points with x01 * s_l an exact integer on one, two or three axes
    ('lattice': ceil == floor, o = 0, two corners of a lane on one row); x = +1 / -1 exactly; |x| up to 1.5 ('outside': negative
    cells); 500 copies of one point ('pile'); points whose cotangent row is all zero ('dead').  n: only the first n points.
    dyadic: every coordinate rounded to a multiple of 2^-10, where x01 * s is exact in float32 for integer s <= 4096 and float64
    autograd through field_ref.encode computes the same function."""
    from oracle import field_ref
    L, log2_T = FIELD_BUDGET_SCENES[name]
    r = np.random.RandomState(seed + 1000 * L + log2_T)
    s = field_ref.level_scalings(L, 16, 4096).numpy().astype(np.float32)
    assert (s == np.floor(s)).all() and s.max() <= 4096
    lm = min(4, L - 1)
    uni = lambda m: r.uniform(-1, 1, (m, 3))

    def run(m, l):
        cell = r.randint(0, int(s[l]), 3)
        return ((cell + r.uniform(0.05, 0.95, (m, 3))) / float(s[l])) * 2 - 1

    def lattice(m):
        p = uni(m)
        lv = r.randint(0, L, m); lv[:90] = 0
        axes = 1 + np.arange(m) % 3                                   # how many axes sit on the lattice
        for i in range(m):
            ax = r.permutation(3)[:axes[i]]
            k = r.randint(0, int(s[lv[i]]) + 1, 3)
            cand = (2.0 * k / float(s[lv[i]]) - 1.0).astype(np.float32)
            sc_ = (cand * np.float32(0.5) + np.float32(0.5)) * s[lv[i]]
            bad = sc_ != np.floor(sc_)                                # not exact in float32 at this level: take level 0 (s = 16)
            cand = np.where(bad, (2.0 * (k % 17) / 16.0 - 1.0).astype(np.float32), cand)
            p[i, ax] = cand[ax]
        return p

    def ends(m, v):
        p = uni(m)
        for i in range(m):
            p[i, r.permutation(3)[:3 if i < 4 else 1 + i % 3]] = v
        return p

    def outside(m):
        p = r.uniform(-1.5, 1.5, (m, 3))
        near = np.abs(p).max(1) <= 1.01
        p[near, 0] = -1.25 - 0.25 * r.uniform(0, 1, int(near.sum()))
        return p

    n_uni = FIELD_SCENE_N - 2168
    u = [n_uni // 4 + (i < n_uni % 4) for i in range(4)]
    pile = np.tile(r.uniform(-0.9, 0.9, (1, 3)), (500, 1))
    blocks = [("uniform", uni(u[0])), ("mesh_order", run(64, 0)), ("uniform", uni(u[1])), ("mesh_order", run(100, 0)),
              ("lattice", lattice(300)), ("mesh_order", run(300, 0)), ("plus_one", ends(20, 1.0)), ("uniform", uni(u[2])),
              ("mesh_order", run(64, lm)), ("outside", outside(200)), ("mesh_order", run(100, lm)), ("minus_one", ends(20, -1.0)),
              ("pile", pile), ("mesh_order", run(300, lm)), ("dead", uni(200)), ("uniform", uni(u[3]))]
    x = np.concatenate([b for _, b in blocks]).astype(np.float32)
    regime = np.concatenate([[nm] * len(b) for nm, b in blocks])
    runs, at = [], 0
    mesh_levels = iter([0, 0, 0, lm, lm, lm])
    for nm, b in blocks:
        if nm == "mesh_order":
            runs.append((at, len(b), next(mesh_levels)))
        at += len(b)
    assert x.shape[0] == FIELD_SCENE_N
    if dyadic:
        x = (np.round(x.astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
    if n is not None:
        x, regime = x[:n], regime[:n]
        runs = [q for q in runs if q[0] + q[1] <= n]
    return dict(name=name, L=L, log2_T=log2_T, x=np.ascontiguousarray(x), regime=regime, scalings=s, runs=runs, table_seed=seed + 7,
                dyadic=dyadic, full=n is None)


def field_scene_table(sc):
    """the scene's hash table [L * T, 2], uniform in (-1, 1)"""
    return np.random.RandomState(sc["table_seed"]).uniform(-1, 1, (sc["L"] << sc["log2_T"], 2)).astype(np.float32)


def field_budget_cotangents(kind, sc, seed):
    """feature cotangents [N, 2L]: 'dense'; 'one_level' (point n live on level n % L only: every level's share of v_x under its own
    budget, and the zero-gradient skip of the slab kernels); 'decades' (columns scaled by logspace(-6, 0)); 'level_off' (levels 0 and
    L - 1 all zero: the gmax == 0 return of the fixed-point kernel).  'dead' points are zero rows, the pile pushes +3 everywhere (the
    row sums the fixed-point overflow bound exists for)."""
    r = np.random.RandomState(seed)
    N, L = sc["x"].shape[0], sc["L"]
    v = r.standard_normal((N, L, 2))
    v[sc["regime"] == "pile"] = 3.0
    if kind == "one_level":
        v *= (np.arange(N)[:, None] % L == np.arange(L)[None, :])[..., None]
    elif kind == "decades":
        v *= np.logspace(-6, 0, 2 * L).reshape(1, L, 2)
    elif kind == "level_off":
        v[:, 0] = 0.0; v[:, L - 1] = 0.0
    else:
        assert kind == "dense", kind
    v[sc["regime"] == "dead"] = 0.0
    return np.ascontiguousarray(v.reshape(N, 2 * L).astype(np.float32))


def field_scene_check(sc):
    """asserts that a full scene holds what it is built for: every regime populated and doing what its name says, and -- counted
    over the corners with a non-zero weight -- a table row that collects at least 64 contributions, one that collects exactly one,
    a row fed by two corners of the same point, and a touched row in the first and in the last slab of some level for both slab
    sizes (16384 rows or T for the float kernel, 8192 for the fixed-point kernel where it accepts T).  Returns the counts."""
    from oracle import field_ref
    assert sc["full"]
    x, reg, s, L, log2_T = sc["x"], sc["regime"], sc["scalings"], sc["L"], sc["log2_T"]
    T = 1 << log2_T
    for nm in FIELD_REGIMES:
        assert (reg == nm).any(), nm
    rows, o = field_ref.hash_cells(x, s, log2_T)
    scaled = (x * np.float32(0.5) + np.float32(0.5))[:, None, :] * s[None, :, None]
    fl, ce = np.floor(scaled), np.ceil(scaled)
    assert sorted(q[1] for q in sc["runs"]) == [64, 64, 100, 100, 300, 300]
    for at, m, l in sc["runs"]:
        if sc["dyadic"] and s[l] > 64:                                # the 2^-10 grid is too coarse to keep a run inside such a cell
            continue
        assert (reg[at:at + m] == "mesh_order").all() and (fl[at:at + m, l] == fl[at, l]).all(), (at, m, l)
    on = (fl == ce)[reg == "lattice"].sum(2).max(1)                    # axes on the lattice, at the best level
    assert all((on == k).any() or (on > k).any() for k in (1, 2)) and (on == 3).any(), np.bincount(on)
    assert (on[:90] >= 1).all() and (sc["dyadic"] or (on >= 1).all())      # (rounding to 2^-10 keeps the level-0 lattice only)
    for nm, v in (("plus_one", 1.0), ("minus_one", -1.0)):
        q = x[reg == nm]
        assert ((q == v).any(1)).all() and ((q == v).all(1)).any(), nm
    q = x[reg == "outside"]
    assert (np.abs(q).max(1) > 1).all() and np.abs(q).max() <= 1.5 and (fl[reg == "outside"] < 0).any()
    assert (x[reg == "pile"] == x[reg == "pile"][0]).all() and (reg == "pile").sum() == 500
    assert not sc["dyadic"] or (x * 1024 == np.round(x * 1024)).all()
    # contributions per row: corners with a non-zero weight, dead points left out
    w = [np.where(b, o[..., k:k + 1], 1 - o[..., k:k + 1]) for k, b in enumerate(field_ref._corner_bits())]
    live = (w[0] * w[1] * w[2] != 0) & (reg != "dead")[:, None, None]
    grow = rows + (np.arange(L, dtype=np.int64) << log2_T)[None, :, None]
    n = np.bincount(grow[live], minlength=L * T)
    srt = np.sort(rows, axis=2)
    same_lane = int((srt[..., 1:] == srt[..., :-1]).any(2).sum())
    assert n.max() >= 64 and (n == 1).any() and same_lane > 0, (n.max(), same_lane)
    sizes = [min(16384, T)] + ([8192] if 8192 * 4 <= T <= 8192 * 64 else [])
    per_level = n.reshape(L, T)
    for rows_per_slab in sizes:
        assert (per_level[:, :rows_per_slab] > 0).any() and (per_level[:, T - rows_per_slab:] > 0).any(), rows_per_slab
    return dict(n_max=int(n.max()), singles=int((n == 1).sum()), same_lane=same_lane, touched=int((n > 0).sum()))


# ----------------------------------------------------------------------------- FlexiCubes extraction against the oracle's error budget
# tests/test_gpu_flexicubes_budget.py (the kernels on an MI355X) and tests/test_flexicubes_budget_cpu.py (the float32 restatement, bar
# kappa / 2).  Kappa by the rule of FIELD_BUDGET_KAPPA: the smallest power of two that is at least 4 x the worst ratio the unchanged
# library shows on the MI355X; the table is in the GPU module's docstring.  Worst figures: 0.983 (entropy backward, accumulate = 1 over a
# pattern: one addition meeting its own rounding bound), 0.503 elsewhere in the extraction, 0.546 in the hand-off (MESH_BUDGET_KAPPA).
FC_BUDGET_KAPPA = 4.0
FC_SCAN_BLOCK = 1024                      # FC_BLOCK of csrc/gs_flexicubes.hip: cubes / edge slots per scan block
FC_COTANGENTS = ("dense", "centres", "ldev", "decades", "no_ldev")
FC_WEIGHT_MASKS = tuple((a, b, g) for a in (True, False) for b in (True, False) for g in (True, False))


def _fc_grid(res):
    from oracle import flexicubes_ref
    return flexicubes_ref.grid(res)[0].numpy().astype(np.float32)


def _fc_finish(res, sdf, r, deform="tanh", weights="normal"):
    gv = _fc_grid(res)
    Vg, C = gv.shape[0], res[0] * res[1] * res[2]
    lim = np.float32(0.5 / max(res))
    if deform == "tanh":
        verts = gv + np.float32(0.8) * lim * np.tanh(r.standard_normal((Vg, 3))).astype(np.float32)
    else:                                                                 # "limit": every coordinate at +-0.5 / R exactly
        verts = gv + lim * np.where(r.uniform(size=(Vg, 3)) < 0.5, -1, 1).astype(np.float32)
    w = r.standard_normal((C, 21)).astype(np.float32)
    if weights == "saturated":                                            # tanh -> +-1 (beta down to 0.01), expf(-gamma) overflows
        sel = r.uniform(size=(C, 21)) < 0.3
        big = np.where(r.uniform(size=(C, 21)) < 0.5, -1.0, 1.0) * np.concatenate((np.full(20, 8.0), [100.0]))[None]
        w = np.where(sel, big, 0.0).astype(np.float32)
    sdf = np.ascontiguousarray(sdf, dtype=np.float32).reshape(Vg)
    assert np.isfinite(sdf).all() and np.abs(sdf).max() > 0
    return dict(res=tuple(res), vertices=np.ascontiguousarray(verts, dtype=np.float32), sdf=sdf, alpha=np.ascontiguousarray(w[:, :8]),
                beta=np.ascontiguousarray(w[:, 8:20]), gamma=np.ascontiguousarray(w[:, 20:]))


def _fc_blob_signs(res, r):
    gv = _fc_grid(res)
    return (gv * np.array([1.0, 1.2, 0.9], np.float32)).astype(np.float64).__pow__(2).sum(-1) ** 0.5 - 0.55 + 0.08 * r.standard_normal(gv.shape[0])


def fc_scene_atlas():
    """16 x 16 x 8: cube (2i, 2j, 2k) planted with raw case i + 8j + 64k (planted cubes share no corner), the unplanted last layer of
    vertices outside; magnitudes uniform in [0.1, 1]"""
    res = (16, 16, 8)
    r = np.random.RandomState(11)
    s1, s2 = 17, 17 * 17
    sign = np.ones(s2 * 9)
    for i in range(8):
        for j in range(8):
            for k in range(4):
                case = i + 8 * j + 64 * k
                for c in range(8):
                    if case >> c & 1:
                        sign[(2 * i + (c & 1)) + s1 * (2 * j + (c >> 1 & 1)) + s2 * (2 * k + (c >> 2 & 1))] = -1.0
    return _fc_finish(res, sign * r.uniform(0.1, 1.0, sign.shape), r)


def fc_scene_random(res, seed):
    r = np.random.RandomState(seed)
    return _fc_finish(res, r.uniform(-0.5, 0.5, (res[0] + 1) * (res[1] + 1) * (res[2] + 1)), r)


def fc_scene_one_cube():
    r = np.random.RandomState(5)
    return _fc_finish((1, 1, 1), np.array([-0.3, 0.2, 0.5, -0.7, 0.4, 0.6, 0.1, 0.9]), r)


def fc_scene_one_quad():
    """2 x 2 x 2: every vertex outside but (0, 1, 1), so the only interior crossing edge is (0,1,1)-(1,1,1): one quad, four triangles,
    small enough to check by hand"""
    r = np.random.RandomState(3)
    sdf = r.uniform(0.1, 1.0, 27)
    sdf[0 + 3 * 1 + 9 * 1] *= -1
    return _fc_finish((2, 2, 2), sdf, r)


def fc_scene_zeros():
    """a blob with 40 grid vertices next to the surface set to +0.0 or -0.0 (both count as outside: `sdf < 0` occupancy, `sdf > 0`
    flip, interpolation weight exactly 0 or 1)"""
    res = (12, 11, 10)
    r = np.random.RandomState(2)
    sdf = _fc_blob_signs(res, r)
    near = np.nonzero(np.abs(sdf) < 0.06)[0]
    pick = r.choice(near, 40, replace=False)
    sdf[pick[:20]] = 0.0
    sdf[pick[20:]] = -0.0
    sc = _fc_finish(res, sdf, r)
    assert np.signbit(sc["sdf"][pick[20:]]).all() and not np.signbit(sc["sdf"][pick[:20]]).any()
    return sc


def fc_scene_decades():
    """blob signs, |sdf| log-uniform over 1e-6 .. 1 (crossings at the ends of their edges: slivers), vertices deformed to the limit"""
    res = (11, 12, 9)
    r = np.random.RandomState(4)
    sign = np.where(_fc_blob_signs(res, r) < 0, -1.0, 1.0)
    return _fc_finish(res, sign * 10.0 ** r.uniform(-6, 0, sign.shape), r, deform="limit")


def fc_scene_saturated():
    r = np.random.RandomState(6)
    res = (10, 12, 11)
    return _fc_finish(res, _fc_blob_signs(res, r), r, weights="saturated")


FC_BUDGET_SCENES = dict(
    atlas=fc_scene_atlas,
    rand_a0=lambda: fc_scene_random((12, 11, 10), 0), rand_a1=lambda: fc_scene_random((12, 11, 10), 1),
    rand_a2=lambda: fc_scene_random((12, 11, 10), 2), rand_a3=lambda: fc_scene_random((12, 11, 10), 3),
    rand_b0=lambda: fc_scene_random((13, 9, 17), 0),
    one_cube=fc_scene_one_cube, one_quad=fc_scene_one_quad, thin=lambda: fc_scene_random((1, 7, 9), 0),
    zeros=fc_scene_zeros, decades=fc_scene_decades, saturated=fc_scene_saturated)


def fc_budget_cases():
    """(scene, (alpha, beta, gamma present), sdf_eps, weight_scale, cotangent kind): all eight weight combinations on one scene, every
    other scene with all three weights and with none; sdf_eps over {None, 0, 0.05}, weight_scale over {0.99, 0.5} and the five
    cotangents rotate"""
    cases = [("rand_a0", m, None, 0.99, "dense") for m in FC_WEIGHT_MASKS]
    eps, wsc = (None, 0.0, 0.05), (0.99, 0.5)
    for j, name in enumerate(FC_BUDGET_SCENES):
        for t, m in enumerate((FC_WEIGHT_MASKS[0], FC_WEIGHT_MASKS[-1])):
            i = 2 * j + t
            cases.append((name, m, eps[i % 3], wsc[(j + t) % 2], FC_COTANGENTS[i % 5]))     # weight_scale alternates where weights exist
    assert len(set(cases)) == len(cases)
    return cases


def fc_case_id(case):
    name, m, eps, ws, kind = case
    return f"{name}-{''.join(c for c, on in zip('abg', m) if on) or 'plain'}-eps{eps}-ws{ws}-{kind}"


def fc_budget_cotangents(kind, Q, nq, K, seed):
    """(v_out_vertices [Q + nq, 3], v_L_dev [K] or None)"""
    r = np.random.RandomState(seed)
    v = r.standard_normal((Q + nq, 3)); l = r.standard_normal(K)
    if kind == "centres":
        v[:Q] = 0; l[:] = 0
    elif kind == "ldev":
        v[:] = 0
    elif kind == "decades":
        v *= 10.0 ** r.uniform(-6, 0, (Q + nq, 1)); l *= 10.0 ** r.uniform(-6, 0, K)
    else:
        assert kind in ("dense", "no_ldev")
    return v.astype(np.float32), (None if kind == "no_ldev" else l.astype(np.float32))


# the hand-off of extracted meshes to vertex_normals / mesh_to_splats (csrc/gs_mesh.hip), same modules: kappa by the same rule
MESH_BUDGET_KAPPA = 4.0
FC_HANDOFF_SCENES = ("atlas", "decades")


def mesh_degenerate():
    """(vertices [V, 3] float32, faces [F, 3] int64, healthy face mask): a jittered octahedron (healthy, vertices 0-5) and, sharing
    no vertex with it, a face with two coincident vertices (6, 7, 8: 7 and 8 at one position), a collinear face (9, 10, 11), a vertex
    (12) whose two incident face normals cancel exactly, and an isolated vertex (17)"""
    r = np.random.RandomState(8)
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.3 + 0.02 * r.standard_normal((6, 3))
    of = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    rest = np.array([[2, 0, 0], [2.5, 0.25, 0.125], [2.5, 0.25, 0.125],                         # 6, 7, 8: coincident pair
                     [3, 0, 0], [3.25, 0.25, 0.5], [3.5, 0.5, 1.0],                              # 9, 10, 11: collinear
                     [4, 0, 0], [5, 0, 0], [4, 1, 0], [4, -1, 0], [3, 0, 0.0],                   # 12: normals (0,0,1) and (0,0,-1) cancel
                     [9, 9, 9]], np.float64)                                                      # 17: isolated
    verts = np.concatenate((octa, rest)).astype(np.float32)
    faces = np.array(of + [[6, 7, 8], [9, 10, 11], [12, 13, 14], [12, 15, 16]], np.int64)
    return verts, faces, np.arange(faces.shape[0]) < 8


# ----------------------------------------------------------------------------- split-sum prefilter against the float64 error budget
# tests/test_prefilter_budget_cpu.py, tests/test_gpu_prefilter_budget.py.  Two constants by the rule written beside PROJ_BUDGET_KAPPA:
# the smallest power of two that is at least 4 x the larger of (a) the float32 oracle against the float64 restatement on the CPU
# (bar kappa / 2) and (b) the kernels on an MI355X.  The measurements are in the docstring of tests/test_gpu_prefilter_budget.py.
PREFILTER_SPEC_KAPPA = 16.0        # specular operator, forward and backward, direct and tiled: (a) 2.83, (b) 1.04
PREFILTER_LIN_KAPPA = 4.0          # diffuse map and mip links: (a) 0.73, (b) 0.82
PREFILTER_DOUBT_CAP = 0.05         # share of texels that may own a pair whose float64 cosine lies within 4 * 2^-24 of the cutoff
PREFILTER_SCENES = ("flat", "sun", "dark")
PREFILTER_COTANGENTS = ("dense", "sparse", "spiked")


def _cube_dirs(R):
    """float64 unit directions [6,R,R,3] of the texel centres"""
    g = 2.0 * ((np.arange(R) + 0.5) / R) - 1.0
    gy, gx = np.meshgrid(g, g, indexing="ij")
    d = np.stack([cube_face_point(s, gx, gy) for s in range(6)])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def prefilter_sun_texels(R):
    """the five texels of the 'sun' scene as (face, y, x): a 2x2 block across the edge of faces 0 and 4 (columns x = 0 and x = R - 1
    are neighbours there) in rows 1 and 2, next to the cube corner (1, 1, 1); and one lone texel inside face 3, last column of one
    tile and first row of the next for every tile size up to R / 2"""
    return [(0, 1, 0), (0, 2, 0), (4, 1, R - 1), (4, 2, R - 1), (3, R // 2, R // 2 - 1)]


def prefilter_scene(kind, R, seed=0):
    """A [6,R,R,3] float32 environment map: 'flat' (rand + 0.05: every texel of one size), 'sun' (flat with prefilter_sun_texels
    scaled by 1e4: the largest element says nothing about a dark texel), 'dark' (flat with face 5 and the octant x < 0, y < 0,
    z > 0 exactly 0: outputs whose whole lobe is zero must be exactly 0).  Random content: no reflection of the cube maps a scene
    onto itself.  Each scene asserts its own property."""
    c = (np.random.RandomState(900 + seed).rand(6, R, R, 3) + 0.05).astype(np.float32)
    if kind == "sun":
        for s, y, x in prefilter_sun_texels(R):
            c[s, y, x] *= np.float32(1e4)
        assert c.max() / np.median(c) >= 1e4 and (c > 100).any(-1).sum() == 5
    elif kind == "dark":
        d = _cube_dirs(R)
        octant = (d[..., 0] < 0) & (d[..., 1] < 0) & (d[..., 2] > 0)
        c[octant] = 0.0; c[5] = 0.0
        zero = (c == 0).all(-1)
        assert zero[5].all() and zero[octant].all() and 0.25 < zero.mean() < 0.35 and (c[~zero] >= 0.05).all()
    else:
        assert kind == "flat", kind
        assert c.max() / c.min() < 25
    for flip in (lambda a: a[:, :, ::-1], lambda a: a[:, ::-1], lambda a: a.transpose(0, 2, 1, 3)):
        assert not np.array_equal(flip(c), c)
    return c


def prefilter_sparse_texels(R):
    """the non-zero texels of the 'sparse' cotangent: three face corners, both sides of a tile boundary in x and in y, both sides of
    the seam of faces 0 and 4, one interior texel"""
    h = R // 2
    return [(0, 0, 0), (1, R - 1, R - 1), (2, 0, R - 1), (4, 5, h - 1), (4, 5, h), (5, h - 1, 3), (5, h, 3), (0, 3, 0), (4, 3, R - 1),
            (3, 2, R - 3)]


def prefilter_cotangent(kind, R, seed=0):
    """A [6,R,R,3] float32 cotangent: 'dense' (rand - 0.5), 'sparse' (dense on prefilter_sparse_texels only: most gradients then
    have budget 0 and must be exactly 0), 'spiked' (dense with three texels scaled by 1e4)"""
    v = (np.random.RandomState(950 + seed).rand(6, R, R, 3) - 0.5).astype(np.float32)
    if kind == "sparse":
        keep = np.zeros((6, R, R), bool)
        for s, y, x in prefilter_sparse_texels(R):
            keep[s, y, x] = True
        v[~keep] = 0.0
        assert (v != 0).any(-1).sum() == 10
    elif kind == "spiked":
        for s, y, x in ((1, 2, R - 2), (2, R // 2, R // 2), (5, R - 1, 0)):
            v[s, y, x] *= np.float32(1e4)
        assert np.abs(v).max() / np.median(np.abs(v)) >= 1e4
    else:
        assert kind == "dense", kind
    return v


def assert_prefilter_budget(name, got, want, budget, kappa, nan_expected=False):
    """assert_within_budget for a prefiltered level: texels the reference leaves NaN (an empty lobe: 0 / 0) must be NaN in `got`
    too and are then left out; none may appear unless the configuration is known to have them.  Returns the worst ratio."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64); budget = np.asarray(budget, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (name, int(np.isnan(got).sum()), int(nan.sum()))
    assert nan_expected or not nan.any(), (name, int(nan.sum()))
    keep = ~nan
    return assert_within_budget(name, got[keep], want[keep], budget[keep], kappa)


_prefilter_refs = {}
_prefilter_boxes = {}


def prefilter_bounds(R, roughness):
    """(cutoff cosine, the oracle's float32 lobe boxes [6,R,R,24]) of a level, computed once"""
    import oracle
    key = (int(R), float(roughness))
    if key not in _prefilter_boxes:
        ct = oracle.ndf_cutoff(roughness)
        _prefilter_boxes[key] = (ct, oracle.specular_bounds(R, ct))
    return _prefilter_boxes[key]


def prefilter_reference(R, roughness):
    """The float64 reference of one specular level, computed once per (R, roughness) and shared (never modified) by the CPU and
    GPU budget tests: dict(ct, bounds, fwd={scene: (val, budget)}, fwd_doubt, bwd={cotangent: (g, budget)}, bwd_doubt,
    has_nan).  The backward is left out where a lobe is empty (0 / 0 in the reference and in the kernels)."""
    import oracle
    key = (int(R), float(roughness))
    if key not in _prefilter_refs:
        ct, bounds = prefilter_bounds(R, roughness)
        maps = np.concatenate([prefilter_scene(k, R) for k in PREFILTER_SCENES], -1)
        val, bud, doubt = oracle.specular_fwd_budget(maps, bounds, roughness, ct)
        ref = dict(ct=ct, bounds=bounds, fwd_doubt=doubt, has_nan=bool(np.isnan(val).any()),
                   fwd={k: (val[..., 3 * j:3 * j + 3], bud[..., 3 * j:3 * j + 3]) for j, k in enumerate(PREFILTER_SCENES)})
        if not ref["has_nan"]:
            cots = np.concatenate([prefilter_cotangent(k, R) for k in PREFILTER_COTANGENTS], -1)
            g, gb, gd = oracle.specular_bwd_budget(bounds, cots, roughness, ct)
            ref["bwd"] = {k: (g[..., 3 * j:3 * j + 3], gb[..., 3 * j:3 * j + 3]) for j, k in enumerate(PREFILTER_COTANGENTS)}
            ref["bwd_doubt"] = gd
        _prefilter_refs[key] = ref
    return _prefilter_refs[key]


def prefilter_pyramid_roughness(n_levels, min_roughness=0.08, max_roughness=0.5):
    return [(i / (n_levels - 2)) * (max_roughness - min_roughness) + min_roughness for i in range(n_levels - 1)] + [1.0]


def prefilter_pyramid_forward_reference(mips):
    """float64 reference of a pyramid's forward, CUT LOOSE per stage: `mips` are the float32 maps the implementation under test
    itself produced ([map, mip 1, ...]); every stage is judged on the inputs it really read, so no error is carried from one
    stage to the next.  Returns (mip_refs [(val, budget) for mips[1:]], base (val, budget), levels [(val, budget)])."""
    import oracle
    roughs = prefilter_pyramid_roughness(len(mips))
    mip_refs = [oracle.cubemap_mip_fwd_budget(m) for m in mips[:-1]]
    base = oracle.diffuse_budget(mips[-1])
    levels = []
    for m, r in zip(mips, roughs):
        ct, bounds = prefilter_bounds(m.shape[1], r)
        levels.append(oracle.specular_fwd_budget(m, bounds, r, ct)[:2])
    return mip_refs, base, levels


def prefilter_pyramid_backward_reference(v_base, v_levels):
    """float64 reference of a pyramid's backward, with the budgets PROPAGATED (the implementation does not expose the gradients
    of the mips): the last level's gradient is specular + diffuse, every other one specular + the mip link of the level below,
    whose budget is carried through the link's non-negative weights; each accumulation adds one rounding of the sum.
    Returns (g, budget) of the map."""
    import oracle
    roughs = prefilter_pyramid_roughness(len(v_levels))
    parts = []
    for v, r in zip(v_levels, roughs):
        ct, bounds = prefilter_bounds(v.shape[1], r)
        parts.append(oracle.specular_bwd_budget(bounds, v, r, ct)[:2])
    d, db = oracle.diffuse_budget(v_base, backward=True)
    g = parts[-1][0] + d
    b = parts[-1][1] + db + np.abs(g)
    for i in range(len(v_levels) - 1, 0, -1):
        m, mb = oracle.cubemap_mip_bwd_budget(g, b)
        g = parts[i - 1][0] + m
        b = parts[i - 1][1] + mb + np.abs(g)
    return g, b
