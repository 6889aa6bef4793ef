"""CPU suite (no GPU): pins the oracle and the host-side glue.

1. golden vectors generated from the importable reference Python (scripts/make_golden.py -> tests/golden/*.npz):
   camera matrices, safe_normalize / rot2quat, tone mapping, atlas packing, mip chain, MGAdapter, and the S1
   arithmetic + roughness->mip map of the real ``RenderableAttrs.splat``;
2. known-answer micro scenes for the rasterizer semantics;
3. the oracle's hand-derived backward passes vs float64 autograd of an independent torch restatement;
4. structural properties (stable sort, offsets, adjointness of the linear prefilter).
"""
import math
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import torch_ref as tr
import geosplatting_amd.synthetic as syn
from oracle import mesh_ref
from geosplatting_amd import cameras as cam_mod
from geosplatting_amd import splitsum as ss
from tests import util
from tests.util import activated, rel_err, sphere_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gold(name):
    return np.load(os.path.join(GOLD, name))


# ----------------------------------------------------------------------------- 1. reference golden vectors
def test_golden_cameras():
    g = gold("ref_cameras.npz")
    c2w = torch.tensor(g["orbit_c2w"])
    assert np.allclose(cam_mod.view_matrix(c2w).numpy(), g["orbit_view"], atol=1e-6)
    ours = cam_mod.orbit_cameras(4, 3.0, 30.0, 256, 256, hfov_degree=40.0)
    for i, c in enumerate(ours):
        assert np.allclose(c.intrinsic_matrix.numpy(), g["orbit_K"][i], rtol=1e-6)
        # same orbit circle (start azimuth is a free choice of the sampler): radius, elevation, look-at and up agree
        pos = c.c2w[:, 3].numpy()
        assert abs(np.linalg.norm(pos) - 3.0) < 1e-5 and abs(pos[1] - 3.0 * math.sin(math.radians(30))) < 1e-5
        assert np.allclose(np.linalg.norm(g["orbit_c2w"][i][:, 3]), 3.0, atol=1e-5)
    eye = torch.tensor(g["lookat_eye"])
    c2w2 = cam_mod.lookat_c2w(eye, torch.zeros(2, 3), torch.tensor([[0.0, 1.0, 0.0]]).repeat(2, 1))
    assert np.allclose(c2w2.numpy(), g["lookat_c2w"], atol=1e-6)
    assert np.allclose(cam_mod.view_matrix(c2w2).numpy(), g["lookat_view"], atol=1e-6)


def test_view_matrix_and_intrinsics_keep_their_bits():
    """view_matrix negates the y / z columns instead of multiplying by a host-built [1, -1, -1] (a pageable host-to-device copy,
    i.e. a host synchronisation, for a device pose), intrinsic_matrix fills its entries one by one: the same bits as the products."""
    g = torch.Generator().manual_seed(3)
    c2w = torch.randn(5, 3, 4, generator=g)
    R, T = c2w[..., :3, :3], c2w[..., :3, 3:4]
    R_inv = (R * torch.tensor([1.0, -1.0, -1.0])).transpose(-1, -2)
    want = torch.zeros(5, 4, 4)
    want[..., 3, 3] = 1.0
    want[..., :3, :3] = R_inv
    want[..., :3, 3:4] = R_inv @ -T
    assert torch.equal(cam_mod.view_matrix(c2w), want)
    assert torch.equal(cam_mod.view_matrix(c2w[2]), want[2])
    fx, fy, cx, cy = 1111.1111, 1111.2, 400.0, 399.7
    assert torch.equal(cam_mod.intrinsic_matrix(fx, fy, cx, cy), torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]))


def test_golden_math():
    g = gold("ref_math.npz")
    assert np.allclose(mesh_ref.safe_normalize(torch.tensor(g["v"])).numpy(), g["safe_normalize"], atol=1e-7)
    assert np.allclose(mesh_ref.rot2quat(torch.tensor(g["rots"])).numpy(), g["rot2quat"], atol=1e-6)


def test_golden_tonemap():
    g = gold("ref_tonemap.npz")
    for mode in ("naive", "aces"):
        assert rel_err(oracle.tonemap_fwd(g["rgba"], float(g["exposure"]), mode), g[mode]) < 2e-6
        t = tr.tonemap_naive if mode == "naive" else tr.tonemap_aces
        assert rel_err(t(torch.tensor(g["rgba"]), torch.tensor(float(g["exposure"]))).numpy(), g[mode]) < 2e-6


def test_golden_ndf_cutoff():
    """The lobe cut-off cosines of the split-sum prefilter: the reference's own `__ndfBounds`
    (rfstudio/graphics/_mesh/_splitsum/_wrap.py:120-135, run unchanged by scripts/make_golden_ndf.py with `_get_plugin` stubbed)
    against the oracle's and the product's restatement -- float64 NumPy on all three sides, so the values must be EQUAL."""
    g = gold("ref_ndf_cutoff.npz")
    assert len(g["res"]) >= 12
    for rough, cutoff, want in zip(g["roughness"], g["cutoff"], g["costheta"]):
        assert oracle.ndf_cutoff(float(rough), float(cutoff)) == float(want), (rough, cutoff)
        assert ss.ndf_cutoff(float(rough), float(cutoff)) == float(want), (rough, cutoff)
    # the six levels of a 512^2 environment are the first six rows
    assert list(g["res"][:6]) == [512, 256, 128, 64, 32, 16]
    assert np.allclose(g["roughness"][:6], oracle.splitsum_roughness(6), rtol=0, atol=0)


def test_canonical_exp_accuracy():
    """gso_exp_neg (the spelled-out exp(-sigma) shared with the HIP compositor, gs_oracle.c) against the float64 exponential on
    EVERY float of [0, 16].  gsplat evaluates `__expf(-sigma)` = ex2.approx(-sigma * log2 e), documented at 2 + floor(|1.16 x|) ulp:
    the argument product is rounded once there as here, so the error grows with sigma in both -- measured 4.3e-7 on the live
    range (a pair with alpha < 1/255, i.e. sigma > ln 255 = 5.54, is skipped) and 9.3e-7 at sigma = 16; the bar is 1e-4."""
    live, _ = oracle.exp_neg_check(0.0, 5.55)
    assert live < 5e-7, live
    full, cs = oracle.exp_neg_check(0.0, 16.0)
    assert full < 1e-6, full
    assert oracle.exp_neg_check(1.0, 2.0)[1] == oracle.exp_neg_check(1.0, 2.0)[1]      # the checksum is deterministic (threads, order)
    assert oracle.exp_neg_check(0.0, 0.0) == (0.0, 0x3f800000)     # exp(-0) == 1 exactly; checksum of one item = its bits


def test_golden_vertex_sampling_and_schedule():
    """'vertex' sampling of the stage-1 loop and the trainer's schedule against the reference's own code (scripts/make_golden_vertex.py:
    GaussianField.get_patches / get_gaussians_from_vertex, get_rotation_from_relative_vectors, GeoSplatTrainer.before_update)."""
    from types import SimpleNamespace
    from geosplatting_amd import field as F
    from geosplatting_amd.stage1 import GeoSplatSchedule
    g = gold("ref_vertex.npz")
    v, f = torch.tensor(g["vertices"]), torch.tensor(g["faces"])
    n, a = F.vertex_patches(v, f)
    assert np.allclose(n.numpy(), g["patch_normals"], atol=1e-6) and np.allclose(a.numpy(), g["patch_areas"], rtol=1e-5, atol=1e-9)
    R = F.rotation_between(torch.tensor([0.0, 0.0, 1.0]), torch.tensor(g["rel_b"]))
    assert np.allclose(R.numpy(), g["rel_rot"], atol=2e-6)
    # a vector opposite to `a` takes the perturbed restart (the formula's `+ eps` makes that result approximate in the reference
    # too: the image of a is within ~0.2 of b, finite, and the regular row is untouched)
    opp = F.rotation_between(torch.tensor([0.0, 0.0, 1.0]), torch.tensor([[0.0, 0.0, -1.0], [0.6, 0.0, 0.8]]), generator=torch.Generator().manual_seed(1))
    img = (opp @ torch.tensor([0.0, 0.0, 1.0])).numpy()
    assert np.isfinite(opp.numpy()).all() and img[0, 2] < -0.8 and np.allclose(img[1], [0.6, 0.0, 0.8], atol=1e-5)
    # the whole sampling with the golden's stand-in encoders (the hash encoders themselves are pinned by ref_hashgrid.npz)
    Wkd, Wks, Wz = (torch.tensor(g[k]) for k in ("Wkd", "Wks", "Wz"))
    fld = SimpleNamespace(kd_enc=lambda x: torch.sigmoid(x @ Wkd), ks_enc=lambda x: x @ Wks, z_enc=lambda x: x @ Wz)
    sp, attrs = F.GaussianField.get_gaussians_from_vertex(fld, v, f, scale=float(g["scale"]), initial_guess=torch.tensor(g["guess"]))
    for name, got in (("means", sp.means), ("scales", sp.scales), ("quats", sp.quats), ("opacities", sp.opacities), ("kd", attrs.kd),
                      ("ks", attrs.ks), ("normals", attrs.normals)):
        assert np.allclose(got.numpy(), g[name], atol=2e-6, rtol=1e-5), name
    # schedule
    sch = GeoSplatSchedule()
    d = g["sched_defaults"]
    assert [sch.vertex_sample_warmup, sch.light_reg_begin, sch.light_reg_end, sch.light_reg_decay, sch.sdf_reg_begin, sch.sdf_reg_end,
            sch.sdf_reg_decay, sch.kd_grad_reg_begin, sch.kd_grad_reg_end, sch.kd_grad_reg_decay, sch.ks_grad_reg_begin, sch.ks_grad_reg_end,
            sch.ks_grad_reg_decay, sch.kd_regualr_perturb_std, sch.ks_regualr_perturb_std] == list(d)
    model = SimpleNamespace(sample_method="face", light_weight=0.0, sdf_weight=0.0, kd_grad_weight=0.0, kd_regualr_perturb_std=0.0,
                            ks_grad_weight=0.0, ks_regualr_perturb_std=0.0, normal_grad_weight=0.0)
    keys = [str(k) for k in g["sched_keys"]]
    for step, row in zip(g["sched_steps"], g["sched_values"]):
        sch.before_update(model, int(step))
        got = [1.0 if model.sample_method == "vertex" else 0.0] + [float(getattr(model, k)) for k in keys[1:]]
        assert np.allclose(got, row, rtol=1e-12, atol=0), (int(step), got, list(row))
    cm = SimpleNamespace(cubemap=torch.tensor([[-1.0, 0.005, 0.5]]))
    cm.cubemap.grad = torch.ones(1, 3)
    sch.scale_light_gradient(cm); sch.after_update(cm, 10)
    assert torch.equal(cm.cubemap.grad, torch.full((1, 3), 64.0)) and torch.equal(cm.cubemap, torch.tensor([[0.01, 0.01, 0.5]]))


def test_tonemap_none_scales_alpha_too():
    """tone_type='none' is `render_rgba * exposure` (rfstudio/model/geosplat.py:123-124): alpha is scaled with the colours and
    the exposure gradient carries the alpha term"""
    g = gold("ref_tonemap.npz")
    e = float(g["exposure"])
    out = oracle.tonemap_fwd(g["rgba"], e, "none")
    assert np.array_equal(out, (g["rgba"] * np.float32(e)).astype(np.float32))
    v = np.random.default_rng(0).standard_normal(g["rgba"].shape).astype(np.float32)
    v_rgba, v_e = oracle.tonemap_bwd(g["rgba"], e, v, "none")
    assert np.allclose(v_rgba, v * np.float32(e)) and abs(v_e - float((v.astype(np.float64) * g["rgba"]).sum())) < 1e-4 * abs(v_e) + 1e-5


def test_golden_atlas_and_mip():
    g = gold("ref_atlas.npz")
    levels = [torch.tensor(g[k]) for k in ("l0", "l1", "l2")]
    assert np.array_equal(ss.merge_mipmaps(levels).numpy(), g["atlas"])
    for a, k in zip(ss.split_mipmaps(torch.tensor(g["atlas"]), 3), ("s0", "s1", "s2")):
        assert np.array_equal(a.numpy(), g[k])
    assert rel_err(oracle.cubemap_mip_fwd(g["cube"]), g["cube_mip"]) < 1e-7


def test_golden_mgadapter():
    g = gold("ref_mgadapter.npz")
    v, f = torch.tensor(g["vertices"]), torch.tensor(g["faces"])
    vn = mesh_ref.vertex_normals(v, f)
    assert np.allclose(vn.numpy(), g["vnormals"], atol=1e-6)
    splats, normals = mesh_ref.mesh_to_splats_set(v, f, vn)
    assert splats.num == 6 * f.shape[0]
    assert np.allclose(splats.means.numpy(), g["means"], atol=1e-6)
    assert np.allclose(splats.scales.numpy(), g["scales"], atol=1e-5)
    assert np.allclose(splats.opacities.numpy(), g["opacities"], atol=1e-6)
    assert np.allclose(normals.numpy(), g["colors"], atol=1e-6)
    q_ref = g["quats"]; q = splats.quats.numpy()
    sign = np.sign((q * q_ref).sum(-1, keepdims=True))          # q and -q are the same rotation
    assert np.allclose(q * sign, q_ref, atol=1e-5)
    assert np.allclose(splats.scales[:, 2].numpy(), -10.0)


def test_golden_splat_arithmetic_and_mip_map():
    """colors captured from the REAL RenderableAttrs.splat (texture fetches served by this oracle) == oracle.shade_fwd"""
    g = gold("ref_splat_arith.npz")
    lut = np.fromfile(os.path.join(os.path.dirname(GOLD), "..", "geosplatting_amd", "assets", "fg_lut_256.bin"),
                      dtype=np.float32).reshape(256, 256, 2)
    levels = [g[f"level{i}"] for i in range(6)]
    for mode in ("pbr", "diffuse", "specular"):
        col = oracle.shade_fwd(g["means"], g["normals"], g["kd"], g["ks"], g["cam_pos"], lut, g["base"], levels, mode=mode)
        assert rel_err(col, g["colors_" + mode]) < 5e-6, mode
    rough = g["ks"][:, 0] * np.float32(0.9) + np.float32(0.1)
    mine = np.array([oracle.mip_from_roughness(r) for r in rough], np.float32)
    assert np.abs(mine - g["mip_level_bias"]).max() < 2e-6
    assert mine.min() >= 0.0 and mine.max() <= 5.0


# ----------------------------------------------------------------------------- S5 known answers (cubemap.cu by formula)
def _np_cube_dirs(R):
    """cube_to_dir (rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:32-46) for every texel, float64: [6,R,R,3]"""
    f = 2.0 * ((np.arange(R) + 0.5) / R) - 1.0
    fy, fx = np.meshgrid(f, f, indexing="ij")
    one = np.ones_like(fx)
    faces = [(one, -fy, -fx), (-one, -fy, fx), (fx, one, fy), (fx, -one, -fy), (fx, -fy, one), (-fx, -fy, -one)]
    d = np.stack([np.stack(t, -1) for t in faces], 0)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _np_pixel_area(R):
    """pixel_area (cubemap.cu:17-30) incl. its |x - H| convention, float64: [R,R] indexed [y,x]"""
    H = R // 2
    a = np.abs(np.arange(R) - H)
    d = np.arctan((a + 1) / H) - np.arctan(a / H)
    return d[:, None] * d[None, :]


def test_s5_known_answers_from_the_published_formulae():
    """The prefilter oracle against closed-form cases written straight from cubemap.cu:110-139,174-179,246-298 in float64 numpy:
    a constant environment (normalised specular == the constant at every roughness; diffuse == c * sum_L clamp(N.L) dA / 3.141592)
    and a single hot texel at roughness 1.0, where D_GGX(alpha^2 = 1) = 1/pi so that every weight is (N.L) dA / (4 pi) inside
    the lobe -- evaluated WITHOUT the per-face bounding boxes, which also shows that the boxes drop no lobe texel."""
    R = 16
    dirs = _np_cube_dirs(R).reshape(-1, 3); area = np.tile(_np_pixel_area(R)[None], (6, 1, 1)).reshape(-1)
    c = np.array([0.3, 1.7, 0.9], np.float32)
    const = np.broadcast_to(c, (6, R, R, 3)).copy()
    for rough in (0.08, 0.29, 1.0):
        ct = oracle.ndf_cutoff(rough)
        raw = oracle.specular_cubemap_fwd(const, oracle.specular_bounds(R, ct), rough, ct)
        hit = raw[..., 3] > 0
        # SpecularBoundsKernel culls 16x16 tiles with the bounding box of their NORMALISED corner directions (cubemap.cu:209-217),
        # which under-estimates the interior of a tile: with one tile per face (R = 16) a narrow lobe is culled altogether and
        # the texel gets weight 0 -- reference behaviour, restated as is (it cannot happen for the wide lobe of roughness 1)
        assert hit.all() if rough == 1.0 else hit.any()
        assert np.abs(raw[hit][:, :3] / raw[hit][:, 3:] - c).max() < 3e-6 * c.max()
    cosm = np.clip(dirs @ dirs.T, 0.0, 0.999)                                   # [out texel, in texel]
    irr = (cosm * area[None, :]).sum(1) / 3.141592
    got = oracle.diffuse_cubemap_fwd(const).reshape(-1, 3)
    assert np.abs(got - irr[:, None] * c[None, :]).max() < 2e-5 * c.max()
    assert abs(irr.mean() - 1.0) < 0.15          # ~ pi / pi (the atan-product texel area of cubemap.cu:17-30 over-counts by 8 % at R = 16)
    # single hot texel, roughness 1.0
    hot = (4 * R + 5) * R + 11
    cube = np.zeros((6 * R * R, 3), np.float32); cube[hot, 0] = 1.0
    rough = 1.0; ct = oracle.ndf_cutoff(rough)
    raw = oracle.specular_cubemap_fwd(cube.reshape(6, R, R, 3), oracle.specular_bounds(R, ct), rough, ct).reshape(-1, 4)
    dots = dirs @ dirs.T                                                        # [out o, in L]
    inside = dots.astype(np.float32) >= np.float32(ct)
    w = np.maximum(dots, 0.0) * (1.0 / np.pi) * area[None, :] / 4.0 * inside
    # membership is decided in fp32 by the oracle: leave texels within 1e-6 of the cutoff out of the comparison
    edge = (np.abs(dots - ct) < 1e-6).any(1)
    assert np.abs(raw[~edge, 3] - w.sum(1)[~edge]).max() < 2e-5 * w.sum(1).max()
    assert np.abs(raw[~edge, 0] - w[~edge, hot]).max() < 2e-5 * w[:, hot].max()
    assert np.abs(raw[:, 1:3]).max() == 0.0


def test_fg_lut_against_reference_subsample():
    g = gold("ref_fg_lut_sub16.npz")
    lut = np.fromfile(os.path.join(os.path.dirname(GOLD), "..", "geosplatting_amd", "assets", "fg_lut_256.bin"),
                      dtype=np.float32).reshape(256, 256, 2)
    sub = lut[np.ix_(g["rows"], g["cols"])]
    # Round 4: the packaged table is a converged float64 quadrature (scripts/gen_fg_lut.py; last refinement step <= 2.7e-5).  What is
    # left against the reference asset is the ASSET's own distance from the integral -- scripts/fg_lut_study.py
    # (profiles/r04_fg_lut_study.txt): asset vs a 4.2 M-point rule max 2.4e-4 with a smooth +1.2e-4 offset at high roughness,
    # packaged vs asset max 4.0e-4 / mean 1.1e-4 over the full table.  (Round 3's 16 384-sample table was 3e-3 off.)
    assert np.abs(sub - g["values"]).max() < 5e-4
    assert np.abs(sub - g["values"]).mean() < 1.5e-4


# ----------------------------------------------------------------------------- 2. known-answer micro scenes
def _one_gaussian(W=16, H=16, opac=0.8, s=0.5):
    means = np.array([[0.0, 0.0, 4.0]], np.float32)
    quats = np.array([[1.0, 0, 0, 0]], np.float32)
    scales = np.full((1, 3), s, np.float32)
    vm = np.eye(4, dtype=np.float32)
    K = np.array([[20.0, 0, 8.5], [0, 20.0, 8.5], [0, 0, 1]], np.float32)    # projects onto pixel centre (8.5, 8.5)
    return means, quats, scales, np.array([opac], np.float32), vm, K


def test_known_answer_single_gaussian():
    means, quats, scales, opac, vm, K = _one_gaussian()
    col = np.array([[0.2, 0.5, 0.9]], np.float32)
    m = oracle.rasterization(means, quats, scales, opac, col, vm, K, 16, 16)
    # cov2d = (f s / z)^2 I = 6.25 I ; blurred 6.55 I ; compensation = 6.25/6.55 ; radius = ceil(3 sqrt(6.55))
    comp = 6.25 / 6.55
    assert abs(m["compensations"][0] - comp) < 1e-6
    assert m["radii"][0] == math.ceil(3 * math.sqrt(6.55 + 0.1))           # lambda = b + sqrt(max(0.01, 0)) = 6.55 + 0.1
    assert np.allclose(m["means2d"][0], [8.5, 8.5]) and abs(m["depths"][0] - 4.0) < 1e-7
    assert np.allclose(m["conics"][0], [1 / 6.55, 0, 1 / 6.55], atol=1e-7)
    a_center = min(0.999, 0.8 * comp)
    assert abs(m["alphas"][8, 8] - a_center) < 1e-6
    assert np.allclose(m["render"][8, 8], col[0] * a_center, atol=1e-6)
    # one pixel to the right: sigma = 0.5/6.55
    a1 = 0.8 * comp * math.exp(-0.5 / 6.55)
    assert abs(m["alphas"][8, 9] - a1) < 1e-6
    assert m["tiles_per_gauss"][0] == 1 and len(m["flatten_ids"]) == 1 and m["isect_offsets"].reshape(-1)[0] == 0


def test_known_answer_two_overlapping_and_termination():
    # two coincident opaque Gaussians at different depths: front composited first; a third never reached when T<=1e-4
    means = np.array([[0, 0, 5.0], [0, 0, 4.0], [0, 0, 6.0]], np.float32)
    quats = np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (3, 1))
    scales = np.full((3, 3), 2.0, np.float32)
    opac = np.array([0.9995, 0.9995, 0.9995], np.float32)
    col = np.eye(3, dtype=np.float32)
    vm = np.eye(4, dtype=np.float32); K = np.array([[20.0, 0, 8.5], [0, 20.0, 8.5], [0, 0, 1]], np.float32)
    m = oracle.rasterization(means, quats, scales, opac, col, vm, K, 16, 16)
    order = m["flatten_ids"]                                   # sorted by depth: gaussian 1 (z=4), 0 (z=5), 2 (z=6)
    assert list(m["gaussian_ids"][order]) == [1, 0, 2]
    a = 0.9995 * (100.0 / 100.3)                                # opacity * compensation, cov2d = (20*2/4)^2 = 100
    c = m["render"][8, 8]
    # second (z=5): alpha2 = 0.9995*64/64.3 -> next_T = (1-a)(1-alpha2) = 1.8e-5 <= 1e-4 -> terminated WITHOUT compositing
    assert (1 - a) * (1 - 0.9995 * 64.0 / 64.3) <= 1e-4
    assert np.allclose(c, [0.0, a, 0.0], atol=2e-6)
    assert abs(m["alphas"][8, 8] - a) < 2e-6
    assert m["last_ids"][8, 8] == 0


def test_empty_scene_and_all_culled():
    vm = np.eye(4, dtype=np.float32); K = np.array([[20.0, 0, 8], [0, 20.0, 8], [0, 0, 1]], np.float32)
    z = np.zeros((0, 3), np.float32)
    m = oracle.rasterization(z, np.zeros((0, 4), np.float32), z, np.zeros(0, np.float32), z, vm, K, 16, 16)
    assert m["render"].max() == 0 and len(m["flatten_ids"]) == 0
    means = np.array([[0, 0, -1.0], [100.0, 0, 1.0], [0, 0, 0.001]], np.float32)      # behind, off-screen, inside near plane
    q = np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (3, 1))
    m = oracle.rasterization(means, q, np.full((3, 3), 0.01, np.float32), np.full(3, 0.5, np.float32),
                             np.ones((3, 3), np.float32), vm, K, 16, 16)
    assert len(m["gaussian_ids"]) == 0 and m["alphas"].max() == 0


def test_sort_is_stable_and_offsets():
    rng = np.random.RandomState(0)
    keys = (rng.randint(0, 7, 5000).astype(np.int64) << 32) | rng.randint(0, 4, 5000).astype(np.int64)
    vals = np.arange(5000, dtype=np.int32)
    k, v = oracle.sort_pairs(keys, vals)
    idx = np.argsort(keys, kind="stable")
    assert np.array_equal(k, keys[idx]) and np.array_equal(v, vals[idx])
    off = oracle.isect_offsets(k, 10)
    tiles = k >> 32
    for t in range(10):
        assert off[t] == np.searchsorted(tiles, t, side="left")


# ----------------------------------------------------------------------------- 3. backward vs float64 autograd
def test_oracle_backward_vs_float64_autograd():
    sc, cam = sphere_case(2, 64)
    means, quats, scales, opac = activated(sc.splats)
    opac = (opac * 0.5).astype(np.float32)          # keeps 1/(1-alpha) well conditioned so that fp32 noise stays ~1e-5
    N = means.shape[0]
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(0)).numpy()
    vm, K = cam.view_matrix.numpy(), cam.intrinsic_matrix.numpy()
    W = H = 64
    m = oracle.rasterization(means, quats, scales, opac, colors, vm, K, W, H)
    dt = torch.float64
    T = lambda a: torch.tensor(a, dtype=dt, requires_grad=True)
    tm, tq, ts, to, tc = T(means), T(quats), T(scales), T(opac), T(colors)
    m2d, z, con, comp = tr.project(tm, tq, ts, torch.tensor(vm, dtype=dt), torch.tensor(K, dtype=dt), W, H)
    gid = torch.tensor(m["gaussian_ids"]).long()
    assert np.abs(m2d[gid].detach().numpy() - m["means2d"]).max() < 1e-4
    assert rel_err(con[gid].detach().numpy(), m["conics"]) < 1e-5
    render, alpha = tr.rasterize(m2d[gid], con[gid], to[gid] * comp[gid], tc[gid], W, H, 16,
                                 torch.tensor(m["isect_offsets"]), torch.tensor(m["flatten_ids"]))
    amb = torch.tensor(m["ambiguous"])
    assert np.abs(render.detach().numpy() - m["render"])[~m["ambiguous"]].max() < 2e-5
    g = torch.Generator().manual_seed(1)
    vr = torch.rand(H, W, 3, generator=g, dtype=dt) * 2 - 1; va = torch.rand(H, W, generator=g, dtype=dt) * 2 - 1
    vr[amb] = 0; va[amb] = 0
    ((render * vr).sum() + (alpha * va).sum()).backward()
    gr = oracle.rasterization_bwd(means, quats, scales, opac, colors, vm, K, W, H, m, vr.float().numpy(), va.float().numpy())
    assert rel_err(gr["v_means"], tm.grad.numpy()) < 1e-4
    assert rel_err(gr["v_opacities"], to.grad.numpy()) < 1e-4
    assert rel_err(gr["v_colors"], tc.grad.numpy()) < 1e-4
    # flat disks (3rd scale e^-10): quats / scales are ill-conditioned -> fp32 noise floor ~1e-4
    assert rel_err(gr["v_quats"], tq.grad.numpy()) < 5e-4
    assert rel_err(gr["v_scales"], ts.grad.numpy()) < 5e-4


# the ill-conditioned regimes at CPU size: opacity 1 at the 0.999 clamp in front of a deep stack, walks of hundreds of low-alpha records
# back from T_final ~ 1e-4, ~1 px speckle, a ragged image with a background
_BUDGET_CPU_SCENES = dict(deep_stack=lambda: util.deep_stack_scene(W=48, H=48, n=2500),
                          veil=lambda: util.veil_scene(W=48, H=48, n=1200, n_veil=8),
                          speckle=lambda: util.speckle_scene(),
                          ragged=lambda: util.ragged_scene(W=61, H=45, n_heavy=1500, n_light=40))


@pytest.mark.parametrize("kind", ["dense", "alpha", "sparse"])
@pytest.mark.parametrize("scene", list(_BUDGET_CPU_SCENES))
def test_raster_bwd_budget_vs_float64_autograd(scene, kind):
    """The error budget of oracle.raster_bwd_budget is honest: the oracle's fp32 compositor gradients lie within
    (kappa / 2) * 2^-24 * budget of float64 autograd through oracle/torch_ref.py's restatement, element by element -- with the
    stored-state term, since the float64 side has no fp32 alphas (without it the deep walks are off by up to ~2000 eps * budget:
    1 - alphas rounded to fp32 at T_final = 1e-4 is 5000 ulp of T_final).  Pixels whose fp32 / float64 forwards take different
    decisions (oracle `ambiguous`, or T_final off by more than 1e-3) get zero cotangents."""
    sc = _BUDGET_CPU_SCENES[scene]()
    W, H, D, bg = sc["W"], sc["H"], 3, sc["background"]
    m = oracle.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], util.scene_colors(sc, D), sc["viewmat"], sc["K"],
                             W, H, background=bg)
    st = util.raster_pair_stats(W, H, m["means2d"], m["conics"], m["opacities"], m["isect_offsets"], m["flatten_ids"], m["last_ids"])
    if scene == "veil":
        assert st["clamped_live"] > 0 and st["max_distinct_last"] >= 8, st
    if scene in ("deep_stack", "veil", "ragged"):
        assert float((1.0 - m["alphas"]).min()) < 1.1e-4 and st["max_list"] > 1000, st      # walks back from T_final ~ 1e-4
    dt = torch.float64
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    m2d, con, op, col = leaf(m["means2d"]), leaf(m["conics"]), leaf(m["opacities"]), leaf(m["colors"])
    render, alpha = tr.rasterize(m2d, con, op, col, W, H, 16, torch.tensor(m["isect_offsets"]), torch.tensor(m["flatten_ids"]))
    if bg is not None:
        render = render + (1 - alpha)[..., None] * torch.tensor(bg, dtype=dt)
    t32 = 1.0 - m["alphas"].astype(np.float64)
    unstable = m["ambiguous"] | (np.abs((1.0 - alpha.detach().numpy()) - t32) > 1e-3 * t32)
    assert unstable.mean() < 0.02
    vr, va = util.budget_cotangents(kind, H, W, D, seed=5)
    vr[unstable] = 0.0; va[unstable] = 0.0
    ((render * torch.tensor(vr, dtype=dt)).sum() + (alpha * torch.tensor(va, dtype=dt)).sum()).backward()
    got, bud = oracle.raster_bwd_budget(W, H, 16, m["means2d"], m["conics"], m["opacities"], m["colors"], m["isect_offsets"],
                                        m["flatten_ids"], m["alphas"], m["last_ids"], vr, va, background=bg, stored_state=True)
    plain = oracle.raster_bwd(W, H, 16, m["means2d"], m["conics"], m["opacities"], m["colors"], m["isect_offsets"].reshape(-1),
                              m["flatten_ids"], m["alphas"], m["last_ids"], vr, va, background=bg)
    print(f"\n  {scene} / {kind}")
    for name, g, p, want, b in zip(("v_means2d", "v_conics", "v_colors", "v_opacities"), got, plain, (m2d, con, col, op), bud):
        assert np.array_equal(g, p), name                   # the budget walk computes exactly gso_raster_bwd's gradients
        assert float(np.abs(want.grad.numpy()).max()) > 0 or kind == "alpha" and name == "v_colors"
        util.assert_within_budget(name, g, want.grad.numpy(), b, util.BUDGET_KAPPA / 2)


def _proj_float64_grads(sc, vw, gid, vm2, vc, vo, vd, classic):
    """float64 autograd through oracle/torch_ref.project of sum(cotangent * packed output) over the visible Gaussians `gid`"""
    dt = torch.float64
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tm, tq, ts, to = leaf(sc["means"]), leaf(sc["quats"]), leaf(sc["scales"]), leaf(sc["opacities"])
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dt)
    m2d, dep, con, comp = tr.project(tm, tq, ts, T(vw["viewmat"]), T(vw["K"]), float(vw["W"]), float(vw["H"]),
                                     eps2d=float(np.float32(0.3)))
    g = torch.tensor(gid).long()
    op_packed = to[g] if classic else to[g] * comp[g]
    loss = (m2d[g] * T(vm2)).sum() + (con[g] * T(vc)).sum() + (op_packed * T(vo)).sum()
    if vd is not None:
        loss = loss + (dep[g] * T(vd)).sum()
    loss.backward()
    return tm.grad.numpy(), tq.grad.numpy(), ts.grad.numpy(), to.grad.numpy()


@pytest.mark.parametrize("kind", list(util.PROJ_COTANGENTS) + ["classic"])
@pytest.mark.parametrize("scene", list(util.PROJ_BUDGET_SCENES))
def test_project_bwd_budget_vs_float64_autograd(scene, kind):
    """The error budget of oracle.project_bwd_budget is honest: the oracle's fp32 projection gradients lie within
    (kappa / 2) * 2^-24 * budget of float64 autograd through oracle/torch_ref.project, element by element, for EVERY Gaussian of
    every view of the scene (the scenes' decision margins make fp32 and float64 take the same clamp route) -- with the stored-state
    term, since the float64 side has no fp32 conics / compensations.  The gradients are gso_project_bwd's bit for bit, culled
    Gaussians and all-zero cotangent rows give exact zeros with budget 0.  ('classic': dense cotangents, rasterize_mode='classic'.)
    Worst ratios |fp32 - float64| / (2^-24 budget) seen (util.PROJ_BUDGET_KAPPA / 2 = 2): v_means 0.88, v_quats 0.08, v_scales 0.98,
    v_opacities 1.00 (v_opacities = v_op * comp: all of its error is the stored compensation's, which the budget charges as measured)."""
    sc = util.PROJ_BUDGET_SCENES[scene]()
    classic = kind == "classic"
    print(f"\n  {scene} / {kind}")
    for vi, vw in enumerate(sc["views"]):
        m = util.proj_scene_forward(sc, vi)
        gid, V = m["gaussian_ids"], len(m["gaussian_ids"])
        assert V > 1000
        vm2, vc, vo, vd = util.proj_budget_cotangents("dense" if classic else kind, V, seed=11 + vi)
        got, bud = oracle.project_bwd_budget(sc["means"], sc["quats"], sc["scales"], sc["opacities"], vw["viewmat"], vw["K"], vw["W"],
                                             vw["H"], gid, m["conics"], m["compensations"], vm2, vc, vo, v_depths=vd, classic=classic,
                                             stored_state=True)
        plain = oracle.project_bwd(sc["means"], sc["quats"], sc["scales"], sc["opacities"], vw["viewmat"], vw["K"], vw["W"], vw["H"],
                                   gid, m["conics"], m["compensations"], vm2, vc, vo, np.zeros((V, 3), np.float32), v_depths=vd,
                                   classic=classic)
        want = _proj_float64_grads(sc, vw, gid, vm2, vc, vo, vd, classic)
        culled = np.ones(len(sc["regime"]), bool); culled[gid] = False
        dead = culled.copy(); dead[gid[3::7]] = True                # culled, or every cotangent zero
        for name, g, p, w, b in zip(("v_means", "v_quats", "v_scales", "v_opacities"), got, plain, want, bud):
            assert g.view(np.int32).tobytes() == p.view(np.int32).tobytes(), name       # exactly gso_project_bwd's gradients
            assert not g[dead].any() and not b[dead].any() and not w[dead].any(), name
            if classic and name == "v_opacities":
                assert np.array_equal(g[gid], vo)
            assert np.isfinite(b).all(), name                      # no element of any Gaussian without a bound
            assert float(np.abs(w).max()) > 0 or (kind == "geometry" and name == "v_opacities")
            util.assert_within_budget(f"view {vi} {name}", g, w, b, util.PROJ_BUDGET_KAPPA / 2)


@pytest.mark.parametrize("mode", ["pbr", "diffuse", "specular"])
def test_oracle_shading_vs_float64_autograd(mode):
    sc, cam = sphere_case(1, 32)
    lut = np.fromfile(os.path.join(os.path.dirname(GOLD), "..", "geosplatting_amd", "assets", "fg_lut_256.bin"),
                      dtype=np.float32).reshape(256, 256, 2)
    g = torch.Generator().manual_seed(3)
    levels = [torch.rand(6, r, r, 3, generator=g).numpy() for r in (64, 32, 16)]
    base = torch.rand(6, 16, 16, 3, generator=g).numpy()
    means, normals, kd, ks = sc.splats.means.numpy(), sc.normals.numpy(), sc.kd.numpy(), sc.ks.numpy()
    cam_pos = np.array([1.0, 1.5, 2.0], np.float32)
    col = oracle.shade_fwd(means, normals, kd, ks, cam_pos, lut, base, levels, mode=mode)
    dt = torch.float64
    T = lambda a: torch.tensor(a, dtype=dt, requires_grad=True)
    tm, tn, tkd, tks, tb = T(means), T(normals), T(kd), T(ks), T(base)
    tl = [T(l) for l in levels]
    col2 = tr.shade(tm, tn, tkd, tks, torch.tensor(cam_pos, dtype=dt), torch.tensor(lut, dtype=dt), tb, tl, mode=mode)
    assert np.abs(col2.detach().numpy() - col).max() < 1e-5
    vc = torch.rand(means.shape[0], 3, generator=g, dtype=dt) * 2 - 1
    (col2 * vc).sum().backward()
    gb = oracle.shade_bwd(means, normals, kd, ks, cam_pos, lut, base, levels, vc.float().numpy(), mode=mode)
    z = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()
    for name, t in (("v_means", tm), ("v_normals", tn), ("v_kd", tkd), ("v_ks", tks), ("v_base", tb)):
        if np.abs(z(t)).max() == 0:
            assert np.abs(gb[name]).max() == 0
        else:
            assert rel_err(gb[name], z(t)) < 5e-5, name
    for a, b in zip(gb["v_levels"], tl):
        if np.abs(z(b)).max() > 0:
            assert rel_err(a, z(b)) < 5e-5


def test_cube_lookup_seams_vs_torch():
    g = torch.Generator().manual_seed(5)
    tex = torch.rand(6, 16, 16, 3, generator=g)
    d = torch.randn(5000, 3, generator=g)
    d[:1000] = torch.sign(d[:1000]) * (1 + 0.03 * torch.randn(1000, 3, generator=g))     # near cube corners / edges
    out, dd = oracle.cube_linear(tex.numpy(), d.numpy())
    td = d.double().requires_grad_(True)
    o2 = tr.cube_linear(tex.double(), td)
    assert np.abs(o2.detach().numpy() - out).max() < 1e-5
    o2[:, 1].sum().backward()
    assert np.abs(td.grad.numpy() - dd[:, 1, :]).max() / np.abs(dd).max() < 1e-4
    # continuity across a face edge
    a, _ = oracle.cube_linear(tex.numpy(), np.array([[1.0, 0.3, 0.9999999]], np.float32))
    b, _ = oracle.cube_linear(tex.numpy(), np.array([[0.9999999, 0.3, 1.0]], np.float32))
    assert np.abs(a - b).max() < 1e-4


# ----------------------------------------------------------------------------- 4. prefilter structure
def test_prefilter_linear_maps_are_adjoint():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(6, 16, 16, 3, generator=g).numpy(); v = (torch.rand(6, 16, 16, 3, generator=g) - 0.5).numpy()
    lhs = (oracle.diffuse_cubemap_fwd(x) * v).sum(dtype=np.float64)
    rhs = (x * oracle.diffuse_cubemap_bwd(v)).sum(dtype=np.float64)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)
    # (the reference only ever filters the 16^2 level with roughness 1.0; its blunt per-16x16-tile interval test
    #  is not conservative when one tile spans a whole face, so narrower lobes are exercised at 32^2 below)
    ct = oracle.ndf_cutoff(1.0)
    b = oracle.specular_bounds(16, ct)
    raw = oracle.specular_cubemap_fwd(x, b, 1.0, ct)
    lhs = (raw[..., :3] * v).sum(dtype=np.float64)
    rhs = (x * oracle.specular_cubemap_bwd(b, v, 1.0, ct)).sum(dtype=np.float64)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)
    # wsum does not depend on the texels; a constant cubemap is reproduced exactly
    const = np.full((6, 16, 16, 3), 0.7, np.float32)
    r2 = oracle.specular_cubemap_fwd(const, b, 1.0, ct)
    assert np.allclose(r2[..., :3] / r2[..., 3:], 0.7, atol=1e-5)
    assert np.allclose(r2[..., 3], raw[..., 3])
    x32 = torch.rand(6, 32, 32, 3, generator=g).numpy(); v32 = (torch.rand(6, 32, 32, 3, generator=g) - 0.5).numpy()
    ct = oracle.ndf_cutoff(0.3)
    b = oracle.specular_bounds(32, ct)
    raw = oracle.specular_cubemap_fwd(x32, b, 0.3, ct)
    assert (raw[..., 3] > 0).all()
    lhs = (raw[..., :3] * v32).sum(dtype=np.float64)
    rhs = (x32 * oracle.specular_cubemap_bwd(b, v32, 0.3, ct)).sum(dtype=np.float64)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)


def test_as_splitsum_shapes_and_energy():
    cube = syn.make_cubemap(64, seed=2).numpy()
    base, levels, saved = oracle.as_splitsum(cube)
    assert base.shape == (6, 16, 16, 3) and [l.shape[1] for l in levels] == [64, 32, 16]
    assert all(np.isfinite(l).all() for l in levels) and np.isfinite(base).all()
    # prefiltering is an average: stays within the range of the input
    assert levels[0].min() >= cube.min() - 1e-4 and levels[0].max() <= cube.max() + 1e-4


# ----------------------------------------------------------------------------- loss side (section 8f rank 2)
def test_golden_loss_glue():
    """oracle/loss_ref.view_loss == the reference's own SSIML1Loss / PSNRLoss / image-space conversions composed as
    geosplat_trainer.py:171-195 (tests/golden/ref_loss.npz, scripts/make_golden_loss.py)"""
    from oracle import loss_ref
    g = gold("ref_loss.npz")
    t = lambda k: torch.tensor(g[k])
    assert np.allclose(loss_ref.rgb2srgb(t("rgb")).numpy(), g["rgb2srgb"][..., :3], atol=1e-7)
    assert np.allclose(loss_ref.srgb2rgb(t("gt_rgba")[..., :3]).numpy(), g["srgb2rgb"][..., :3], atol=1e-7)
    out = loss_ref.view_loss(t("rgb"), t("alpha"), t("gt_rgba"), t("train_bg"), metric_bg=t("bg_color"))
    assert abs(float(out["loss"]) - float(g["loss"])) < 1e-6
    assert abs(float(out["ssim_loss"]) * 0.2 + float(out["l1"]) * 0.8 - float(g["ssim_l1"])) < 1e-6
    assert abs(float(out["psnr"]) - float(g["psnr"])) < 1e-4


def test_ssim_restatement_vs_scipy():
    """independent formulation of the torchmetrics SSIM: scipy separable filters with reflect borders + crop"""
    from scipy.ndimage import correlate1d
    from oracle import loss_ref
    rng = np.random.default_rng(3)
    a = rng.random((1, 3, 37, 45)); b = np.clip(a + 0.2 * rng.standard_normal(a.shape), 0, 1)
    w = loss_ref.gaussian_window(11, 1.5, torch.float64).numpy()
    blur = lambda z: correlate1d(correlate1d(z, w, axis=-1, mode="mirror"), w, axis=-2, mode="mirror")
    mu_a, mu_b = blur(a), blur(b)
    va = np.maximum(blur(a * a) - mu_a ** 2, 0); vb = np.maximum(blur(b * b) - mu_b ** 2, 0); cab = blur(a * b) - mu_a * mu_b
    s = ((2 * mu_a * mu_b + 1e-4) * (2 * cab + 9e-4)) / ((mu_a ** 2 + mu_b ** 2 + 1e-4) * (va + vb + 9e-4))
    expect = s[..., 5:-5, 5:-5].mean()
    got = float(loss_ref.ssim_torchmetrics(torch.tensor(a), torch.tensor(b))[0])
    assert abs(got - expect) < 1e-12
    assert abs(float(loss_ref.ssim_torchmetrics(torch.tensor(a), torch.tensor(a))[0]) - 1.0) < 1e-12


# ----------------------------------------------------------------------------- hash-grid field (section 8f rank 3)
def _hashgrid_golden():
    g = gold("ref_hashgrid.npz")
    tb = torch.Generator().manual_seed(0)
    torch.manual_seed(int(g["b_table_seed"]))
    b_table = torch.rand(16 * 2 ** int(g["b_log2"]), 2) * 2 - 1        # the generator script draws it the same way
    return g, b_table


def test_golden_hashgrid_restatement():
    """oracle/field_ref == outputs of the reference's own HashEncoding (torch backend) + MLP code"""
    from oracle import field_ref
    g, b_table = _hashgrid_golden()
    assert np.array_equal(field_ref.level_scalings(16, 16, 4096).numpy(), g["a_scalings"])
    for tag, table in (("a", torch.tensor(g["a_table"])), ("b", b_table)):
        x = torch.tensor(g[f"{tag}_x"]).requires_grad_(True)
        t = table.clone().requires_grad_(True)
        f = field_ref.encode(x, t, torch.tensor(g[f"{tag}_scalings"]), int(g[f"{tag}_log2"]))
        assert np.allclose(f.detach().numpy(), g[f"{tag}_feats"], atol=1e-6), tag
        (f * torch.tensor(g[f"{tag}_g"])).sum().backward()
        assert np.allclose(x.grad.numpy(), g[f"{tag}_v_x"], rtol=1e-4, atol=1e-4 * np.abs(g[f"{tag}_v_x"]).max()), tag
        rows = torch.tensor(g[f"{tag}_touched"])
        assert np.allclose(t.grad[rows].numpy(), g[f"{tag}_v_table_touched"], atol=1e-5), tag
        mask = torch.ones(t.shape[0], dtype=torch.bool); mask[rows] = False
        assert t.grad[mask].abs().max().item() == 0.0
    # full call: grad-scaling trick + MLP
    x = torch.tensor(g["a_x"][:256]).requires_grad_(True)
    t = torch.tensor(g["a_table"]).requires_grad_(True)
    y = field_ref.hash_encoding(x, t, torch.tensor(g["a_scalings"]), int(g["a_log2"]),
                                [torch.tensor(g["c_w0"]), torch.tensor(g["c_w1"]), torch.tensor(g["c_w2"])], "sigmoid", 16.0)
    assert np.allclose(y.detach().numpy(), g["c_y"], atol=1e-6)
    (y * torch.tensor(g["c_gy"])).sum().backward()
    assert np.allclose(x.grad.numpy(), g["c_v_x"], rtol=1e-4, atol=1e-4 * np.abs(g["c_v_x"]).max())
    assert np.allclose(t.grad[torch.tensor(g["c_touched"])].numpy(), g["c_v_table_touched"], atol=1e-5)


@pytest.mark.parametrize("tag", ["rand4", "rand6", "rand567", "blob10", "blob_plain"])
def test_golden_flexicubes_restatement(tag):
    """oracle/flexicubes_ref.py (tables derived by rule, index formulation of its own) against the reference's own
    dual_marching_cubes / compute_entropy outputs and autograd gradients (scripts/make_golden_flexicubes.py)."""
    from oracle import flexicubes_ref as O
    g = np.load(os.path.join(GOLD, "ref_flexicubes.npz"))
    res = tuple(int(r) for r in g[f"{tag}.res"])
    ins = {k: torch.from_numpy(g[f"{tag}.in.{k}"]).requires_grad_(True)
           for k in ("vertices", "sdf", "alpha", "beta", "gamma") if f"{tag}.in.{k}" in g}
    v, f, L = O.extract(ins["vertices"], ins["sdf"], res, ins.get("alpha"), ins.get("beta"), ins.get("gamma"))
    ent = O.entropy(ins["sdf"], res)
    assert torch.equal(f, torch.from_numpy(g[f"{tag}.out.faces"]))                      # index work: bit-exact
    assert torch.equal(v.detach(), torch.from_numpy(g[f"{tag}.out.vertices"]))
    assert torch.equal(L.detach(), torch.from_numpy(g[f"{tag}.out.L_dev"]))
    np.testing.assert_allclose(ent.item(), g[f"{tag}.out.entropy"], rtol=1e-6)
    ((v * torch.from_numpy(g[f"{tag}.cot.vertices"])).sum() + (L * torch.from_numpy(g[f"{tag}.cot.L_dev"])).sum()
     + 0.7 * ent).backward()
    for k, t in ins.items():
        ref = g[f"{tag}.grad.{k}"]
        np.testing.assert_allclose(t.grad.numpy(), ref, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(ref).max()))


def test_flexicubes_tables_cover_all_cases():
    from oracle import flexicubes_ref as O
    dmc, nvd, chk = O.tables()
    for c in range(256):
        crossing = sorted(i for i, (a, b) in enumerate(O.CUBE_EDGES) if (c >> a & 1) != (c >> b & 1))
        assert sorted(e for p in dmc[c] for e in p) == crossing          # every crossing edge in exactly one patch
        assert all(3 <= len(p) <= 7 for p in dmc[c]) and len(dmc[c]) <= 4
    assert int(chk[:, 0].sum()) == 36 and all(chk[c, 4] == 255 - c for c in range(256) if chk[c, 0])


# ----------------------------------------------------------------------------- shading backward: the error budget
_SHADE_CASES = [(nm, mode) for nm, spec in util.SHADE_BUDGET_SCENES.items() for mode in spec["modes"]]
_shade_scene_cache = {}


def _shade_scene(name, mode):
    if (name, mode) not in _shade_scene_cache:
        sc = util.shade_budget_scene(name, mode, **util.SHADE_BUDGET_SCENES[name]["kw"])
        util.shade_scene_check(sc)                                   # every regime present, every selection margin above its bound
        t = lambda a: torch.tensor(a, dtype=torch.float64)
        _shade_scene_cache[(name, mode)] = sc, dict(means=t(sc["means"]), normals=t(sc["normals"]), kd=t(sc["kd"]), ks=t(sc["ks"]),
                                                    base=t(sc["base"]), levels=[t(l) for l in sc["levels"]])
    return _shade_scene_cache[(name, mode)]


@pytest.mark.parametrize("kind", util.SHADE_COTANGENTS)
@pytest.mark.parametrize("scene,mode", _SHADE_CASES)
def test_shade_bwd_budget_vs_float64_autograd(scene, mode, kind):
    """oracle.shade_bwd_budget on every shading-budget scene (tests/util.py SHADE_BUDGET_SCENES; shade_scene_check asserts the regimes
    and the selection margins): the fp32 gradients equal gso_shade_bwd's bit for bit, every budget is finite, rows with an all-zero
    cotangent and texels no footprint touches are exact zeros with budget 0, and every element of v_means / v_normals / v_kd / v_ks /
    v_base / v_levels[l] lies within (kappa / 2) * 2^-24 * budget of float64 autograd through oracle/torch_ref.shade.

    torch_ref.cube_linear took another route than the C code for a direction without a major axis (a zero normal in 'diffuse'): it
    sampled the centre of face +x where cube_footprint declares the footprint invalid (colour 0, no gradients); it now does the same.

    Worst ratios |fp32 - float64| / (2^-24 budget) seen (util.SHADE_BUDGET_KAPPA / 2 = 2):
    v_means 0.09, v_normals 0.28, v_kd 0.20, v_ks 0.20, v_base 0.25, v_levels[0..3] 0.13 / 0.15 / 0.13 / 0.10."""
    sc, t64 = _shade_scene(scene, mode)
    N = len(sc["regime"])
    cot = util.shade_budget_cotangents(kind, N, seed=7)
    args = (sc["means"], sc["normals"], sc["kd"], sc["ks"], sc["cam_pos"], sc["lut"], sc["base"], sc["levels"], cot)
    g, b = oracle.shade_bwd_budget(*args, mode=mode, **sc["opts"])
    g0 = oracle.shade_bwd(*args, mode=mode, **sc["opts"])
    flat = lambda x: [x["v_means"], x["v_normals"], x["v_kd"], x["v_ks"], x["v_base"]] + list(x["v_levels"])
    names = ["v_means", "v_normals", "v_kd", "v_ks", "v_base"] + [f"v_levels[{l}]" for l in range(len(sc["levels"]))]
    # ---- float64 autograd
    leaves = [t64[k].clone().requires_grad_(True) for k in ("means", "normals", "kd", "ks", "base")]
    lv = [l.clone().requires_grad_(True) for l in t64["levels"]]
    o = sc["opts"]
    col = tr.shade(leaves[0], leaves[1], leaves[2], leaves[3], torch.tensor(sc["cam_pos"], dtype=torch.float64),
                   torch.tensor(sc["lut"], dtype=torch.float64), leaves[4], lv, min_roughness=o["min_roughness"],
                   max_metallic=o["max_metallic"], mode=mode, env_min_r=o["env_min_roughness"], env_max_r=o["env_max_roughness"])
    (col * torch.tensor(cot, dtype=torch.float64)).sum().backward()
    want = [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in leaves + lv]
    dead = ~cot.any(1)
    assert dead.sum() >= N // 7
    for nm, a, a0, bb, w in zip(names, flat(g), flat(g0), flat(b), want):
        assert a.view(np.int32).tobytes() == a0.view(np.int32).tobytes(), nm          # the same bits as gso_shade_bwd
        assert np.isfinite(bb).all(), nm
        if a.shape[0] == N and a.ndim == 2:
            assert not a[dead].any() and not bb[dead].any(), nm
        else:
            assert not a[bb == 0].any() and (w[bb == 0] == 0).all(), nm               # untouched texels
            assert (bb == 0).any() or a.shape[1] <= 32, nm
        r = util.assert_within_budget(f"{scene}/{mode}/{kind} {nm}", a, w, bb, util.SHADE_BUDGET_KAPPA / 2)
        print(f"    {nm:12s} {r:6.3f}")


# ----------------------------------------------------------------------------- hash-grid field: the error budget
@pytest.mark.parametrize("scene", list(util.FIELD_BUDGET_SCENES))
def test_field_budget_scenes_hold_their_regimes(scene):
    """every scene of tests/test_gpu_field_budget.py, as drawn and rounded to the dyadic grid: all regimes populated, the mesh-order
    runs inside one cell, lattice points on 1 / 2 / 3 axes, negative cells, and rows with >= 64 contributions, with exactly one,
    with two corners of one point, in the first and in the last slab (util.field_scene_check)"""
    for dyadic in (False, True):
        st = util.field_scene_check(util.field_budget_scene(scene, dyadic=dyadic))
        print(f"  {scene} dyadic={dyadic}: {st}")


@pytest.mark.parametrize("scene", list(util.FIELD_BUDGET_SCENES))
def test_field_budget_vs_float64_autograd(scene):
    """oracle/field_ref.py's float32 restatements of the features, v_x and v_table (float order and fixed point) lie within
    (kappa / 2) * 2^-24 * budget of float64 autograd through field_ref.encode, element by element, under every cotangent kind and
    every table-gradient scale -- on the scene rounded to multiples of 2^-10, where x01 * s is exact in float32 and both sides
    compute the same function (elsewhere the float32 cell arithmetic makes float64 a different function).  Rows no corner reaches
    are exactly 0 in autograd; elements with no non-zero contribution have budget 0 and are exactly 0 on both sides.

    Worst ratios seen (util.FIELD_BUDGET_KAPPA / 2 = 2): features 0.41, v_x 0.26, v_table float 0.67, v_table fixed 0.98."""
    from oracle import field_ref
    sc = util.field_budget_scene(scene, dyadic=True)
    util.field_scene_check(sc)
    L, log2_T = sc["L"], sc["log2_T"]
    table = util.field_scene_table(sc)
    s64 = torch.tensor(sc["scalings"], dtype=torch.float64)
    f32, f64, fb = field_ref.encode_fwd(sc["x"], table, sc["scalings"], log2_T)
    worst = dict(features=0.0, v_x=0.0, v_table_float=0.0, v_table_fixed=0.0)
    bar = util.FIELD_BUDGET_KAPPA / 2
    for ki, kind in enumerate(util.FIELD_COTANGENTS):
        tgs = util.FIELD_TGS[(ki + L) % 3]
        cot = util.field_budget_cotangents(kind, sc, seed=11)
        x = torch.tensor(sc["x"], dtype=torch.float64, requires_grad=True)
        t = torch.tensor(table, dtype=torch.float64, requires_grad=True)
        f = field_ref.encode(x, t, s64, log2_T)
        (f * torch.tensor(cot, dtype=torch.float64)).sum().backward()
        if ki == 0:
            assert np.array_equal(f64, f.detach().numpy())             # the oracle's float64 forward IS autograd's function here
            worst["features"] = util.assert_within_budget(f"{scene} features", f32, f.detach().numpy(), fb, bar)
        vt = t.grad.numpy() * tgs
        for mode in ("float", "fixed"):
            b = field_ref.encode_bwd_budget(sc["x"], table, sc["scalings"], log2_T, cot, tgs, mode)
            mask = np.ones(vt.shape[0], bool); mask[b["rows"]] = False
            assert not vt[mask].any()
            assert np.isfinite(b["v_table_budget"]).all() and not b["v_table_f32"][b["n"] == 0].any()
            assert np.abs(b["v_table"] - vt[b["rows"]]).max() <= 1e-12 * np.abs(vt).max()       # two float64 sums of the same addends
            r = util.assert_within_budget(f"{scene}/{kind} v_table {mode}", b["v_table_f32"], vt[b["rows"]], b["v_table_budget"], bar)
            worst[f"v_table_{mode}"] = max(worst[f"v_table_{mode}"], r)
        dead = sc["regime"] == "dead"
        assert not b["v_x_f32"][dead].any() and not b["v_x_budget"][dead].any()
        worst["v_x"] = max(worst["v_x"], util.assert_within_budget(f"{scene}/{kind} v_x", b["v_x_f32"], x.grad.numpy(), b["v_x_budget"], bar))
    print("  worst " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("O,I", [(1, 1), (32, 32), (3, 32), (32, 7), (17, 5)])
def test_wgrad_budget_vs_float64(O, I):
    """field_ref.wgrad_f32 (a float32 sum in gs_mlp_wgrad's plan order: per wave, the four-wave fold, the strided reduce) within
    (kappa / 2) budgets of the float64 product, every element, columns of dY and X over six decades.  Worst ratio seen: 0.08."""
    from oracle import field_ref
    worst = 0.0
    for N in (1, 2, 15, 16, 17, 511, 512, 513, 4097, 70001):
        r = np.random.RandomState(N + O)
        dY = (r.standard_normal((N, O)) * np.logspace(-6, 0, O)).astype(np.float32)
        X = (r.standard_normal((N, I)) * np.logspace(0, -6, I)).astype(np.float32)
        nb = field_ref.wgrad_plan_blocks(N)
        for scale in (1.0, -0.25):
            want, bud = field_ref.wgrad_budget(dY, X, scale, nb)
            got = field_ref.wgrad_f32(dY, X, scale, nb)
            worst = max(worst, util.assert_within_budget(f"wgrad {O}x{I} N={N} scale={scale}", got, want, bud, util.FIELD_BUDGET_KAPPA / 2))
    print(f"  worst {worst:.3f}")
