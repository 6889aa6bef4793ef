"""GPU: the workspace contract of the entry points that take caller-allocated scratch, under poisoned scratch (tests/ws_poison.py).

Every family runs its small shape through the public wrapper three times -- scratch filled with 0x00 ("zero", what a fresh allocation
reads as), with the bytes a LARGER call of the same family left behind ("recycle": the large shape runs under 0xFF first), and with 0xFF
("ones": NaN in a float, -1 in an int) -- and asserts
  * both 4 KB guards of every workspace intact in every mode (an overrun farther than one guard, 4096 bytes, is NOT seen by this method);
  * the EXACT outputs bit-identical between the three modes;
  * the FLOAT-ATOMIC outputs (sums of fp32 atomics, whose bits differ from run to run) pass, in each of the three runs, the op's own check
    against its float64 reference, called from the op's own test module with that module's tolerance, and hold nothing non-finite.
Nothing here restates a reference or introduces a tolerance.  With -s every family prints its workspace requests and, per mode, the worst
ratio (error / bound of the op's own check) of its float-atomic outputs; the ratios are information, not thresholds.

Which output is in which class
  rasterization   exact: every meta tensor (ids, radii, tiles, isect ids, flatten ids, offsets, last_ids, means2d, depths, conics,
                  opacities, colours), render, alpha -- forward, no atomics.  float-atomic: the five leaf gradients (the compositor's
                  packed gradients are fp32 atomics over tiles); checked by test_gpu_gsplat_modes._compare_grads (GRAD_TOL).  Capacity
                  path: render / alphas / last_ids / flatten ids / offsets exact and equal to the exact path's; v_packed float-atomic,
                  columns against oracle.raster_bwd with GRAD_TOL as test_gpu_gsplat_modes.test_means2d_grad does.
  surfels         exact: ids, radii, tiles, flatten ids, offsets, projected rows, the four images, median.  float-atomic: leaf gradients
                  and the densification signal (test_gpu_surfels._check_call, TOL).
  front / splat   exact: the tone-mapped images of both views, in both passes (exact counts, then capacity with 24-bit keys).
                  float-atomic: every leaf gradient incl. the cubemap (tests.util.compare_grads against the op-by-op decomposition).
  shade_bwd       exact: colours, v_means, v_normals, v_kd, v_ks (one thread per Gaussian, the oracle's bits).  float-atomic: the texel
                  gradients (test_gpu_shade_budget._check_texels, TEXEL_ORDER_BAR).
  specular bounds exact: the bounds (integers in floats).
  losses          exact: all of out[0:6], v_rgb, v_alpha, the smooth loss and v_img (partials summed in a fixed order;
                  test_gpu_loss_budget.test_two_calls_same_bits requires it).
  field           exact: features, v_x, the fixed-point table gradient (integer sums), dW of gs_mlp_wgrad (fixed order; header).
                  float-atomic: the float-slab table gradient (LDS float atomics; the bound of test_gpu_field lines 79-80: 1e-4 of the
                  largest element against oracle.field_ref).
  FlexiCubes      exact: faces, out_vertices, L_dev (test_topology_bit_for_bit requires two forwards to agree), the entropy.
                  float-atomic: g_vertices, g_sdf, g_alpha, g_beta, g_gamma, the entropy's g_sdf (budgets of
                  test_flexicubes_budget_cpu.case_budget / flexicubes_ref.entropy_budget, FC_BUDGET_KAPPA).
  TSDF / Poisson  exact: counts, vertices, faces; the splatted grid (64-bit integer atomics: test_gpu_poisson.test_reproducibility).
  mesh rasterizer exact: rast (64-bit atomic min of (depth, face): order independent), with and without near_clip.
  BVH, NN grid    exact: the node buffer, closest-hit (t, face, bary) and occlusion; (dist, index) of the 1- and 3-nearest.
  densify         exact: totals, indices, every output row (the normals are an input).

The segment audit (csrc, `take<` / `tail<` / `pad(` sites and the hand-carved layouts), read BEFORE the first poisoned run.  Every launch
is on the call's stream `s`.  segment: first writer -> first reader.
  gs_project_fwd_vis(_ex)  ScanWs ctrl[4], desc[4 chunks]: gs_zero_async of the whole workspace -> project_fwd*_kernel (ticket, look-back)
  gs_front_fwd             ScanWs ctrl, desc: front_setup_kernel zeroes every word -> front_fwd_kernel
  gs_isect_sort            SortWs table: radix_hist_kernel writes [digit < nbins][block], radix_rowscan_kernel the row totals ->
                           radix_scatter_kernel reads the same entries; keys / vals: scatter of pass p -> hist of pass p + 1; pad: never
  gs_isect_bin(_cap/_tiles_cap)  RadixWs table: as above; da / db: scatter -> next pass; rect: tile_rect_kernel (v < V) ->
                           emit_chained_kernel (rows the depth order names, < V); state: bin_setup_kernel zeroes n_state_words ->
                           emit_chained_kernel; ia: emit_chained_kernel (positions < min(I, cap)) -> radix_hist_kernel (i < I);
                           ib: scatter -> hist; tile_ids: absent; pad: never
  gs_isect_bin_front       tile first (hand-carved): cursor[tiles] zeroed and class_count[2], lists written by tile_offsets_scan_kernel
                           -> bin_scatter_kernel (cursor), seg_sort*_kernel (count, list[b < count]); items: bin_scatter_kernel ->
                           seg_sort*_kernel over [offsets[t], offsets[t + 1]) (after an overflow the unwritten tail is read and CLAMPED to
                           a valid row, by design).  Radix path: RadixWs as above with tile_ids: FinalTiles store -> bin_offsets_tiles_kernel
  gs_raster_prepare*       RasterWs rec0..2: build_stream_packed_kernel (i < I) -> compositor (i < offsets end); order:
                           tile_order_kernel -> compositor; vis: pack_visible_kernel (only without vis_records) -> build_stream;
                           bo.bcount[64]: ZEROED by tile_order_kernel (prepare), incremented by raster_fwd_window_kernel of
                           gs_raster_composite_tone_log, read by raster_bwd_log_kernel; bo.blist: the log forward (k < tiles) -> the
                           log backward, only when the counts sum to the tile count.  CROSS-CALL CONTRACT (stated in
                           include/geosplat_hip.h above gs_raster_log_ws_bytes): a composite needs a prepared workspace, and the bucket
                           lists are used only when exactly one log forward ran since the prepare; else the forward's own tile order.
                           test_prepare_between_composites shows the consequence on valid input.
  gs_raster_composite_tone_log  CullLogWs mask, idx: forward, entries < log_n of the quadrant -> backward, entries < count;
                           count[4 tiles]: forward, every tile -> backward
  gs_surfel_project_fwd    tiles[N], block_v, block_i: surfel_count_kernel -> surfel_scan_kernel, surfel_write_kernel
  gs_shade_bwd             priv copies (hand-carved): gs_zero_async of all of them -> shade_bwd_kernel<true> atomics -> priv_reduce_kernel
  gs_specular_bounds_fast  tile_box, group_box (hand-carved): bounds_tile_aabb_kernel, every entry -> specular_bounds_fast_kernel
  gs_photo_loss            maps[9 W H]: loss_stats_kernel, every pixel -> loss_grad_kernel (pixels inside the image only);
                           partials[4 blocks]: loss_stats_kernel -> loss_finalize_kernel
  gs_smooth_loss           partials: smooth_loss_kernel, every block -> smooth_finalize_kernel
  gs_hashgrid_bwd          v_lm (hand-carved): hashgrid_transpose_kernel -> hashgrid_bwd_slab_kernel
  gs_hashgrid_bwd_fixed    HgFixedWs v_lm: hashgrid_transpose_kernel -> hashgrid_level_max_kernel; q_counts, gmax: ONE gs_zero_async
                           from q_counts up to queues -> hashgrid_level_max_kernel (atomicMax into gmax), hashgrid_bin_kernel (q_counts);
                           queues: hashgrid_bin_kernel -> hashgrid_bwd_slabfx_kernel (entries < q_counts)
  gs_mlp_wgrad             partial[blocks][1024]: mlp_wgrad_kernel, wave 0 writes all 1024 -> mlp_wgrad_reduce_kernel
  gs_flexicubes_count      FcWs blk_cube, blk_slot: fc_*_count_kernel -> fc_scan_blocks_kernel (in place; totals into hdr[0..7],
                           hdr[8..10]) -> fc_*_assign_kernel; case8: every cube; vd_base, k_base: cubes with a dual vertex (the readers
                           load them for every cube with case != 0 but use them only under nvd > 0); quad_id: every slot;
                           partial: fc_entropy_kernel -> fc_entropy_finalize_kernel.  CONTRACT (header, "Step 1..3"): fwd / bwd /
                           entropy read what gs_flexicubes_count left for the same sdf; the wrapper keeps the block in the autograd node.
  gs_tsdf_extract_count    TsLayout info, eflag, vbase: every voxel; blocks[4 nb]: tsdf_cubes_kernel rows 1..3, tsdf_edges_kernel row 0
                           -> tsdf_scan_kernel -> tsdf_vbase_kernel.  CONTRACT (header): gs_tsdf_extract_fill reads the count's `ws`.
  gs_grid_splat            gmax + accumulators (hand-carved): gs_zero_async of the whole workspace -> ps_max_kernel, splat, convert
  gs_meshraster_fwd / gs_meshclip_fwd  MrLayout keys, n_big[0] (and n_big[1] with clip): mr_fill_kernel -> mr_small_kernel; big / cross:
                           appended by mr_small_kernel -> mr_big_kernel / mr_cross_kernel (entries < the counters).  CONTRACT (header):
                           gs_mesh*_resolve reads the keys the fwd of the same call pair left.
  gs_bvh_build             BvhWs bounds[6], count[F]: bvh_init_kernel -> bvh_bounds_kernel (atomics), bvh_fit_kernel (arrival counters);
                           keys, vals: bvh_morton_kernel; skeys, svals, sort: gs_isect_sort (above); parent, right, last, rsplit:
                           bvh_karras_kernel (parent[0] = -1; every other node and every gap g < F - 1 exactly once) -> bvh_fit_kernel
  gs_nn_build              NnWs keys, vals: nn_keys_kernel; skeys, svals, sort: gs_isect_sort -> nn_gather_kernel, nn_cellstart_kernel
  gs_densify_plan          DnLayout flags: densify_classify_kernel, every row; blocks[3 nb]: classify -> densify_scan_kernel (in place).
                           gs_densify_fill: rowmap: densify_map_kernel (rows < N_out) -> the row kernels.  CONTRACT (header): fill reads
                           the plan in `ws`.
No segment is read before its call (or, for the count -> fill pairs, its stated predecessor) wrote it.  The count -> fill contracts are
what every test of those ops already exercises; the one arrangement that spans unrelated launches (bcount) has its own test below.

Evidence that the method sees what it is meant to see (done once against a scratch build of the library, never committed): with the
gs_zero_async of gs_hashgrid_bwd_fixed shortened to end in front of `gmax` -- a float maximum that scales the fixed point, never an
index or a loop count -- test_field passes its "zero" run and fails at the first poisoned one: "exact output `fixed_table` differs
between zero and recycle scratch (524295)" of 1 048 576 elements, the stale maximum being a NaN pattern that the kernel propagates
into every slab it touches.  The unchanged library passes all three modes.

Seen on an MI355X (requests of the small shape in bytes; worst ratio of the op's own check under zero / recycle / ones; "-": the
family has no float-atomic output, or its check returns no figure):
  rasterization, exact counts   [272, 281088, 806400]                        0.018 / 0.018 / 0.036
  rasterization, capacity       [272, 359168, 1018880]                       0.004 / 0.005 / 0.006
  surfels                       [2064, 44288] twice (run + the module's call) -
  front / splat                 per view [144, 59904, 353792, 485888], 16 in two views x two passes    0.025 / 0.025 / 0.025
  shade_bwd, private copies     [2359296]                                    0.007 / 0.007 / 0.007
  gs_specular_bounds_fast       [288]                                        -
  photo + smooth loss           [70788, 288]                                 -
  hash grid + gs_mlp_wgrad      [384512, 128000, 8192]                       0.001 / 0.001 / 0.001
  FlexiCubes                    [34048, 34048]                               0.366 / 0.366 / 0.366
  TSDF extraction               [7648]                                       -
  grid splat + mesh_from_indicator  [4112, 28928]                            -
  mesh rasterizer               [16032], near_clip [16352]                   -
  BVH                           [23808]                                      -
  NN grid                       [41216]                                      -
  densify                       [36352]                                      -
No guard was touched, no exact output changed a bit and no segment was found that is read before it is written: no kernel was changed.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.ws_poison import poisoned

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ the three runs
def _bits(t):
    """a host copy whose equality is equality of bits (NaN payloads and -0 included)"""
    t = t.detach().contiguous().cpu()
    if t.is_floating_point():
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _flatten(out, prefix=""):
    """{name: tensor} of a nested dict / list / tuple of tensors, numbers and None"""
    flat = {}
    if isinstance(out, dict):
        for k, v in out.items():
            flat.update(_flatten(v, f"{prefix}{k}."))
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flat.update(_flatten(v, f"{prefix}{i}."))
    elif isinstance(out, torch.Tensor):
        flat[prefix[:-1]] = out
    elif isinstance(out, np.ndarray):
        flat[prefix[:-1]] = torch.from_numpy(np.ascontiguousarray(out))
    elif out is not None:
        flat[prefix[:-1]] = torch.tensor(out)
    return flat


def _three_runs(family, small, large, check=None):
    """small() -> (exact, atomic) under zero, recycle (behind large() under ones) and ones; check(atomic, mode) -> worst ratio or None"""
    outs, runs = {}, {}
    with poisoned("zero") as runs["zero"]:
        outs["zero"] = small()
    with poisoned("ones") as big:
        large()
    with poisoned("recycle") as runs["recycle"]:
        outs["recycle"] = small()
    with poisoned("ones") as runs["ones"]:
        outs["ones"] = small()
    sizes = runs["zero"].sizes
    assert len(sizes) > 0, f"{family}: no workspace went through _lib.workspace"
    assert runs["recycle"].sizes == sizes and runs["ones"].sizes == sizes, f"{family}: the request sizes depend on the scratch"
    assert sum(big.sizes) > sum(sizes), f"{family}: the large variant asked for no more scratch than the small one"
    base = _flatten(outs["zero"][0])
    assert base, family
    for mode in ("recycle", "ones"):
        got = _flatten(outs[mode][0])
        assert got.keys() == base.keys(), (family, mode)
        for k, want in base.items():
            a, b = _bits(got[k]), _bits(want)
            assert a.shape == b.shape and torch.equal(a, b), \
                f"{family}: exact output `{k}` differs between zero and {mode} scratch ({int((a != b).sum()) if a.shape == b.shape else 'shape'})"
    ratios = {}
    finite0 = {k: bool(torch.isfinite(v).all()) for k, v in _flatten(outs["zero"][1]).items() if v.is_floating_point()}
    for mode in ("zero", "recycle", "ones"):
        for k, v in _flatten(outs[mode][1]).items():
            if v.is_floating_point() and finite0.get(k, False):
                assert bool(torch.isfinite(v).all()), f"{family}: `{k}` holds a non-finite value under {mode} scratch"
        if check is not None:
            ratios[mode] = check(outs[mode][1], mode)
    shown = "  ".join(f"{m} {'-' if r is None else format(r, '.3f')}" for m, r in ratios.items()) or \
        ("no float-atomic output" if not _flatten(outs["zero"][1]) else "checked inside each run (that check returns no figure)")
    print(f"\n  {family}: {len(sizes)} workspace requests {sizes} (large variant {big.sizes}); worst ratio of the op's own check: {shown}")
    return outs


# ------------------------------------------------------------------------------------------------------------ rasterization()
def test_rasterization(cuda):
    """project, isect_bin, raster through rasterization() with backward (SH degree 0: D = 3), then the capacity protocol on the same view"""
    import oracle
    from geosplatting_amd import _lib as L
    from tests import test_gpu_gsplat_modes as M
    from tests.test_gpu_raster_budget import _R
    R = _R()                                                                        # the module geosplatting_amd.rasterization
    from tests.util import rel_err
    means, quats, scales, opac, cam = M._scene()                                    # 4 000 splats, camera inside, 100 x 75
    coeffs = M._coeffs(means.shape[0], 1, seed=103)
    vr, va = M._upstream(cam, 3, 3)
    big = M._scene(n=8000, seed=4, inside=False)                                   # 128 x 128: another tile grid
    big_coeffs = M._coeffs(8000, 1, seed=104)
    keys = ("gaussian_ids", "radii", "tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets", "last_ids", "means2d", "depths",
            "conics", "opacities", "colors", "compensations")

    def run(sc, co, cot):
        m_, q_, s_, o_, cam_ = sc
        ts, (render, alpha, meta) = M._call(cuda, m_, q_, s_, o_, co, cam_, sh_degree=0)
        (render[0] * cot[0].to(cuda)).sum().add((alpha[0, ..., 0] * cot[1].to(cuda)).sum()).backward()
        torch.cuda.synchronize()
        exact = dict(render=render, alpha=alpha, **{k: meta[k] for k in keys if k in meta})
        return exact, dict(grads=[t.grad for t in ts]), (ts, meta, alpha)

    want = {}

    def small():
        exact, atomic, (ts, meta, alpha) = run((means, quats, scales, opac, cam), coeffs, (vr, va))
        if not want:                                                                # the meta tensors are exact outputs: one reference serves the three runs
            m = dict(meta, _alpha=alpha[0, ..., 0].detach().cpu().numpy(), _colors_np=meta["colors"].cpu().numpy())
            want["g"], _ = M._expected_sh_grads(means, quats, scales, opac, coeffs, cam, m, 0, vr.numpy(), va.numpy(), False)
        return exact, dict(atomic, _ts=list(ts))

    def check(atomic, mode):
        M._compare_grads(atomic["_ts"], want["g"], scales)                         # the module's own check, GRAD_TOL
        names = ("v_means", "v_quats", "v_scales", "v_opacities", "v_colors")
        return max(float(np.abs(t.grad.cpu().numpy() - want["g"][n]).max() / (np.abs(want["g"][n]).max() + 1e-30))
                   for n, t in zip(names, atomic["_ts"]) if n != "v_quats") / M.GRAD_TOL

    outs = _three_runs("rasterization (exact counts)", small,
                       lambda: run(big, big_coeffs, M._upstream(big[4], 3, 4)), check)

    # ---- capacity protocol: the same view with the counts left on the device
    exact0 = outs["zero"][0]
    I = int(exact0["flatten_ids"].numel()); V = int(exact0["gaussian_ids"].numel())
    lib = L.lib()
    t = lambda a: torch.tensor(a, device=cuda)
    colors = exact0["colors"].detach()                                              # [V,3] in packed order -> per-Gaussian rows
    col_n = torch.zeros(means.shape[0], 3, device=cuda); col_n[exact0["gaussian_ids"].long()] = colors
    W, H = cam.width, cam.height
    tvr, tva = vr.to(cuda).contiguous(), va.to(cuda).contiguous()

    def cap(sc, cols, i_cap, cot):
        m_, q_, s_, o_, cam_ = sc
        pr = R._project_stage(t(m_), t(q_), t(s_), t(o_), cols, cam_.view_matrix.to(cuda), cam_.intrinsic_matrix.to(cuda), cam_.width,
                              cam_.height, 16, 0.3, 0.01, 1e10, 0.0)
        status = torch.zeros(3, dtype=torch.int64, device=cuda)
        state, Vc, Ic, D, whs = R._bin_stage_cap(pr, i_cap, status, want_ids=False)
        state = R._prepare_stage_cap(state, Vc, Ic, D, whs)
        render, alphas, st = R._composite_stage_cap(state, Vc, Ic, D, whs, None)
        vp = torch.empty(Vc, lib.gs_raster_grad_stride(D), device=cuda)
        rws = st["raster_ws"]
        L.check(lib.gs_raster_bwd_cap(cam_.width, cam_.height, 16, D, Vc, L.ptr(st["colors"]), None, L.i64(Ic), L.ptr(st["counts"]),
                                      L.ptr(st["isect_offsets"]), L.ptr(alphas), L.ptr(st["last_ids"]), L.ptr(cot[0]), L.ptr(cot[1]),
                                      L.ptr(vp), L.ptr(rws), C.c_size_t(rws.numel()), L.stream()), "gs_raster_bwd_cap")
        torch.cuda.synchronize()
        assert int(status[0]) == 0
        n_v, n_i = (int(x) for x in st["counts"].tolist())
        exact = dict(render=render, alphas=alphas, last_ids=st["last_ids"], flatten_ids=st["flatten_ids"][:n_i],
                     offsets=st["isect_offsets"], counts=st["counts"])
        return exact, dict(v_packed=vp[:n_v])

    gb = torch.Generator().manual_seed(9)
    big_cols = torch.rand(8000, 3, generator=gb).to(cuda)
    bvr, bva = M._upstream(big[4], 3, 4)
    m = {k: exact0[k].detach().cpu().numpy() for k in ("means2d", "conics", "opacities", "isect_offsets", "flatten_ids", "last_ids")}
    v_m2d, v_con, v_col, v_op = oracle.raster_bwd(W, H, 16, m["means2d"], m["conics"], m["opacities"], colors.cpu().numpy(),
                                                  m["isect_offsets"].reshape(-1), m["flatten_ids"], exact0["alpha"][0, ..., 0].detach().cpu().numpy(),
                                                  m["last_ids"][0], vr.numpy(), va.numpy())

    def check_cap(atomic, mode):
        vp = atomic["v_packed"].cpu().numpy()
        errs = [rel_err(vp[:, 0:2], v_m2d), rel_err(vp[:, 2:5], v_con), rel_err(vp[:, 5], v_op), rel_err(vp[:, 6:9], v_col)]
        assert max(errs) < M.GRAD_TOL, (mode, errs)                                  # as test_gpu_gsplat_modes.test_means2d_grad
        return max(errs) / M.GRAD_TOL

    outs_cap = _three_runs("rasterization (capacity)", lambda: cap((means, quats, scales, opac, cam), col_n, I + 777, (tvr, tva)),
                           lambda: cap(big, big_cols, 400000, (bvr.to(cuda).contiguous(), bva.to(cuda).contiguous())), check_cap)
    c0 = outs_cap["zero"][0]
    assert c0["counts"].tolist() == [V, I]
    assert torch.equal(c0["flatten_ids"], exact0["flatten_ids"]) and torch.equal(c0["offsets"].reshape(-1), exact0["isect_offsets"].reshape(-1))
    assert torch.equal(_bits(c0["render"]), _bits(exact0["render"][0].detach())) and torch.equal(c0["last_ids"], exact0["last_ids"][0])


# ------------------------------------------------------------------------------------------------------------ surfels
def test_surfels(cuda):
    """surfel_project, isect_bin and the ray-splat compositor with backward: the 400-surfel 'outside' scene of tests/surfel_ref.py"""
    from tests import surfel_ref as R
    from tests import test_gpu_surfels as S
    case = ("RGB+ED", True, 16, True)
    reference = S._reference("outside", *case, small=True)
    sc = reference[0]
    big = R.make_scene("inside")                                                    # 1 500 surfels at 100 x 75: another tile grid

    def run(scn, backward=True):
        leaves, (render, alpha, normals, nfd, distort, median, meta) = S._gpu_call(scn, cuda, render_mode="RGB+ED", distloss=True, tile_size=16)
        if backward:
            (render.sum() + alpha.sum() + normals.sum() + distort.sum()).backward()
        torch.cuda.synchronize()
        ints = {"meta_" + k: meta[k] for k in ("gaussian_ids", "radii", "tiles_per_gauss", "flatten_ids", "isect_offsets", "means2d", "depths", "normals",
                                     "ray_transforms") if k in meta}
        return dict(render=render, alpha=alpha, normals=normals, distort=distort, median=median, **ints), dict(grads=[v.grad for v in leaves.values()])

    def check(atomic, mode):
        S._check_call(cuda, reference, *case)                                       # the module's own check (its own GPU call, under this mode's scratch)
        return None

    def small():
        exact, atomic = run(sc)
        check(atomic, None)
        return exact, atomic

    _three_runs("surfels", small, lambda: run(big))


# ------------------------------------------------------------------------------------------------------------ front / splat
def test_front_splat_two_views(cuda, monkeypatch):
    """front, isect_bin_front (tile first), raster, raster_log through RenderableAttrs.splat over two views, forward and backward: pass 0
    with exact counts, pass 1 under the capacity protocol with 24-bit keys"""
    import geosplatting_amd as gs
    from tests import test_gpu_callshape as CS
    from tests.util import compare_grads, sphere_case
    sc, _ = sphere_case(2, 96, cubemap_res=64)
    cams = CS._cams(96, 2)
    g = torch.Generator().manual_seed(2)
    ups = [(torch.rand(96, 96, 4, generator=g) * 2 - 1).to(cuda) for _ in cams]
    sc_big, _ = sphere_case(3, 144, cubemap_res=64)
    cams_big = CS._cams(144, 2)
    ups_big = [(torch.rand(144, 144, 4, generator=g) * 2 - 1).to(cuda) for _ in cams_big]
    monkeypatch.setenv("GEOSPLAT_SPLAT", "ops")
    ref_i, ref_g = CS._run(sc, cams, ups, cuda)                                     # the op-by-op decomposition, default allocator: the reference
    monkeypatch.setenv("GEOSPLAT_SPLAT", "fused")

    def run(s, c, u):
        gs.viewbatch.reset()
        passes = [CS._run(s, c, u, cuda) for _ in range(2)]
        return dict(images=[p[0] for p in passes]), dict(grads=[p[1] for p in passes])

    def check(atomic, mode):
        for gr in atomic["grads"]:
            compare_grads(gr, ref_g)                                                # tests/util.py, its own tolerances
        worst = 0.0
        for gr in atomic["grads"]:
            for k, w in ref_g.items():
                if w is not None and k not in ("quats", "scales", "exposure"):
                    worst = max(worst, float((gr[k] - w).abs().max()) / (float(w.abs().max()) + 1e-30) / 2e-5)
        return worst

    outs = _three_runs("front / splat", lambda: run(sc, cams, ups), lambda: run(sc_big, cams_big, ups_big), check)
    for imgs in outs["zero"][0]["images"]:
        for a, b in zip(imgs, ref_i):
            assert torch.equal(a, b)
    gs.viewbatch.reset()


def test_prepare_between_composites(cuda):
    """The stated cross-call contract of the compositor workspace (include/geosplat_hip.h, above gs_raster_log_ws_bytes) on valid input:
    the backward's bucket lists are cleared by gs_raster_prepare*, not by the forward that files the tiles.  ONE log forward behind a
    prepare: the counts sum to the tile count and the lists are used.  A second forward WITHOUT a prepare counts past it and the backward
    falls back to the forward's tile order; a prepare in between restores the lists.  All three give the image bit for bit and the
    gradient records to the order of the float atomics (the bound of test_gpu_front.test_cull_log_backward_equals_plain_backward)."""
    from geosplatting_amd import _lib as L
    from geosplatting_amd import front as F
    from tests import test_gpu_front as TF
    from tests.util import rel_err
    lib = L.lib()
    x = TF._inputs(cuda, level=2, res=96)
    W = H = 96
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    fr, _ = TF._front(x, TF._env(cuda), cuda)
    V, I = int(fr.host_counts[0]), int(fr.host_counts[1])
    g = torch.Generator().manual_seed(3)
    v_img = (torch.rand(H, W, 4, generator=g) * 2 - 1).to(cuda)
    exposure = torch.tensor([1.3], device=cuda)
    a256 = lambda n: (n + 255) & ~255

    def bcount(rws):                                                                # RasterWs: rec0..2 [I] float4, order [tiles], then bcount [64]
        at = 3 * a256(16 * max(I, 1)) + a256(4 * tiles)
        return rws[at:at + 256].cpu().numpy().view(np.int32)

    def prepare(state):
        rws = state["raster_ws"]
        L.check(lib.gs_raster_prepare_vis(W, H, 16, 3, V, L.ptr(fr.vis), L.i64(I), L.ptr(state["isect_offsets"]), L.ptr(state["flatten_ids"]),
                                          L.ptr(rws), C.c_size_t(rws.numel()), L.stream()), "gs_raster_prepare_vis")

    def sequence(steps):
        state, V_, I_ = F.bin_stage(fr, None, None)                                 # binning + prepare on a fresh workspace
        assert (V_, I_) == (V, I)
        out = None
        for step in steps:
            if step == "prepare":
                prepare(state)
            else:
                log = F.log_ws(I, W, H, cuda)
                out = F.composite_fwd(state, V, I, W, H, 1, exposure, log)
        state["v_packed"] = torch.zeros(V, lib.gs_raster_grad_stride(3), device=cuda)
        g_exp = torch.zeros(1, device=cuda)
        img, render, alphas, last = out
        F.composite_bwd(state, V, I, W, H, 1, exposure, render, alphas, last, log, v_img, g_exp)
        torch.cuda.synchronize()
        return img, last, state["v_packed"], bcount(state["raster_ws"])

    one = sequence(["fwd"])
    two = sequence(["fwd", "fwd"])
    between = sequence(["fwd", "prepare", "fwd"])
    assert int(one[3].sum()) == tiles and int(between[3].sum()) == tiles and int(two[3].sum()) == 2 * tiles
    assert float(one[2].abs().max()) > 0
    for other in (two, between):
        assert torch.equal(other[0], one[0]) and torch.equal(other[1], one[1])
        assert rel_err(other[2].cpu().numpy(), one[2].cpu().numpy()) < 2e-6


# ------------------------------------------------------------------------------------------------------------ shading backward
def test_shade_bwd_private_copies(cuda, monkeypatch):
    """gs_shade_bwd with the XCD-private texel copies (GEOSPLAT_SHADE_PRIV=1) through gs.shade: the env3 / pbr scene of
    tests/test_gpu_shade_budget.py (a 64^2 level outside LDS), whose Gaussians keep their margins from every decision"""
    import geosplatting_amd as gs
    from tests import test_gpu_shade_budget as SB
    from tests import util
    monkeypatch.setenv("GEOSPLAT_SHADE_PRIV", "1")
    sc = SB._scene("env3", "pbr")
    cot, (want, bud, pool) = SB._want("env3", "pbr", "dense", 3)
    big = SB._scene("env4", "pbr")                                                  # four levels up to 128^2: more private floats
    o = sc["opts"]

    def run(s, c):
        t = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda)
        leaves = [t(s[k]).requires_grad_(True) for k in ("means", "normals", "kd", "ks")]
        base = t(s["base"]).requires_grad_(True); levels = [t(l).requires_grad_(True) for l in s["levels"]]
        so = s["opts"]
        env = gs.TextureSplitSum(base, levels, so["env_min_roughness"], so["env_max_roughness"])
        col = gs.shade(*leaves, t(s["cam_pos"]), env, min_roughness=so["min_roughness"], max_metallic=so["max_metallic"], mode="pbr",
                       fg_lut=t(s["lut"]).reshape(1, 256, 256, 2).contiguous())
        col.backward(t(c))
        torch.cuda.synchronize()
        return dict(colors=col, rows=[l.grad for l in leaves]), dict(texels=[l.grad for l in levels] + [base.grad])

    def check(atomic, mode):
        SB._check_texels(f"shade_priv_poison env3/pbr/dense/{mode}", atomic["texels"], SB._texels(want), SB._texels(bud), bar=SB.TEXEL_ORDER_BAR)
        return SB.WORST.get(("shade_priv_poison", "texels"))

    outs = _three_runs("shade_bwd (private copies)", lambda: run(sc, cot),
                       lambda: run(big, util.shade_budget_cotangents("dense", len(big["regime"]), 3)), check)
    SB._check_rows("shade_priv_poison env3/pbr/dense", outs["zero"][0]["rows"], want, bud, dead=~cot.any(1))


# ------------------------------------------------------------------------------------------------------------ prefilter bounds
def test_specular_bounds(cuda):
    from geosplatting_amd import splitsum as SS

    def run(res):
        SS._bounds_cache.clear()
        ct, b = SS.specular_bounds(res, 0.29, 0.99, cuda)
        torch.cuda.synchronize()
        SS._bounds_cache.clear()
        return dict(bounds=b, ct=ct), {}

    outs = _three_runs("gs_specular_bounds_fast", lambda: run(16), lambda: run(40))
    b = outs["zero"][0]["bounds"]
    assert bool((b[..., 0::4] <= b[..., 1::4]).any()) and float(b.max()) <= 15.0 and float(b.min()) >= 0.0


# ------------------------------------------------------------------------------------------------------------ losses
def test_losses(cuda):
    """gs_photo_loss and gs_smooth_loss at 37 x 53 (three blocks by four, partial last ones)"""
    from geosplatting_amd.loss import SMOOTH_EDGE, SMOOTH_TV, smooth_loss_and_grad
    from tests import loss_budget as lb
    from tests import test_gpu_loss_budget as LB
    inputs, bud = lb.tier_a_case(37, 53, True, 5.0)
    g = torch.Generator().manual_seed(7)
    big_inputs = (torch.rand(70, 90, 3, generator=g), torch.rand(70, 90, 1, generator=g), torch.rand(70, 90, 4, generator=g),
                  torch.rand(70, 90, 3, generator=g))
    assert [tuple(a.shape[2:]) for a in inputs] == [tuple(a.shape[2:]) for a in big_inputs]
    img, gt = torch.rand(37, 53, 9, generator=g).to(cuda), torch.rand(37, 53, 3, generator=g).to(cuda)
    img_b, gt_b = torch.rand(70, 90, 9, generator=g).to(cuda), torch.rand(70, 90, 3, generator=g).to(cuda)

    def run(inp, im, gtt):
        out, v_rgb, v_alpha = LB._run(cuda, inp, True, 5.0)
        s_out, v_img = smooth_loss_and_grad(im, gtt, (SMOOTH_EDGE, SMOOTH_TV, SMOOTH_EDGE), (0.2, 0.1, 0.3))
        torch.cuda.synchronize()
        return dict(out=out[:6], v_rgb=v_rgb, v_alpha=v_alpha, smooth=s_out, v_img=v_img), {}

    outs = _three_runs("gs_photo_loss + gs_smooth_loss", lambda: run(inputs, img, gt), lambda: run(big_inputs, img_b, gt_b))
    e = outs["ones"][0]
    assert lb.fraction(e["v_rgb"], bud["d_rgb"], bud["bound_rgb"]) <= 1.0 and lb.fraction(e["v_alpha"], bud["d_alpha"], bud["bound_alpha"]) <= 1.0
    LB._assert_values(LB._values(e["out"]), bud["values"], "poisoned 37x53")


# ------------------------------------------------------------------------------------------------------------ field
def test_field(cuda, monkeypatch):
    """hash grid backward in both modes that take a workspace (fixed point, float slabs) and gs_mlp_wgrad: N = 1 000, sixteen levels
    16..2048 of 2^15 rows as tests/test_gpu_field.py"""
    from geosplatting_amd.field import hash_encode, level_scalings, linear
    from oracle import field_ref
    log2_T = 15
    sc = level_scalings(16, 16, 2048)

    def data(N, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.rand(N, 3, generator=g) * 1.2 - 0.6
        table = (torch.rand(16 * 2 ** log2_T, 2, generator=g) * 2 - 1) * 1e-2
        gy = torch.randn(N, 32, generator=g) * torch.logspace(-6, 0, 32)
        w = torch.randn(32, 32, generator=g)
        return x, table, gy, w

    x, table, gy, w = data(1000, 5)
    big = data(2300, 6)
    t64 = table.double().requires_grad_(True); x64 = x.clone().requires_grad_(True)
    field_ref.encode(x64, t64, sc, log2_T).backward(gy.double())
    ref_t, ref_x = t64.grad * 16.0, x64.grad

    def run(d):
        x_, table_, gy_, w_ = (a.to(cuda) for a in d)
        res = {}
        for mode in ("2", "1"):
            monkeypatch.setenv("GEOSPLAT_HASHGRID_SLABS", mode)
            t = table_.clone().requires_grad_(True); xx = x_.clone().requires_grad_(True)
            f = hash_encode(xx, t, sc, log2_T, grad_scaling=16.0)
            f.backward(gy_)
            res[mode] = (f.detach(), t.grad, xx.grad)
        wc = w_.clone().requires_grad_(True)
        feats = res["2"][0]
        (linear(feats, wc) * gy_).sum().backward()
        torch.cuda.synchronize()
        exact = dict(features=res["2"][0], fixed_table=res["2"][1], v_x=res["2"][2], v_x_float=res["1"][2], dW=wc.grad)
        return exact, dict(float_table=res["1"][1])

    def check(atomic, mode):
        err = float((atomic["float_table"].cpu().double() - ref_t).abs().max()) / (1e-4 * float(ref_t.abs().max()))
        assert err < 1.0, (mode, err)                                               # tests/test_gpu_field.py:80
        return err

    outs = _three_runs("hash grid backward + gs_mlp_wgrad", lambda: run((x, table, gy, w)), lambda: run(big), check)
    e = outs["zero"][0]
    assert float((e["fixed_table"].cpu().double() - ref_t).abs().max()) / float(ref_t.abs().max()) < 1e-6      # test_hashgrid_fixed_point_table_gradient
    assert float((e["v_x"].cpu().double() - ref_x.double()).abs().max()) < 1e-4 * float(ref_x.abs().max())
    assert torch.equal(e["v_x"], e["v_x_float"])


# ------------------------------------------------------------------------------------------------------------ FlexiCubes
def test_flexicubes(cuda):
    """count -> fwd -> bwd and the entropy pair through geosplatting_amd.flexicubes on rand_a0 (12 x 11 x 10: two scan blocks of cubes,
    five of edge slots, the last ones partial), all three weights, dense cotangents"""
    from geosplatting_amd.flexicubes import _Entropy, _Extract
    from oracle import flexicubes_ref as O
    from tests import util
    from tests.test_flexicubes_budget_cpu import case_budget, scene
    case = util.fc_budget_cases()[0]
    assert case[0] == "rand_a0" and all(case[1]) and case[4] == "dense"
    name, _, eps, wsc, _ = case
    sc = scene(name)
    w, cv_h, cl_h, b = case_budget(case)
    eb = O.entropy_budget(sc["sdf"], sc["res"], v_out=0.7)
    big = scene("rand_b0")
    t = lambda a: None if a is None else torch.tensor(a, device=cuda)

    def run(s, wts, cv, cl):
        ins = [t(s["vertices"]).requires_grad_(True), t(s["sdf"]).requires_grad_(True)] + [t(wts[k]).requires_grad_(True) for k in ("alpha", "beta", "gamma")]
        out_v, faces, Ld = _Extract.apply(*ins, tuple(s["res"]), float(wsc), eps)
        if cv is None:
            (out_v.sum() + Ld.sum()).backward()
        else:
            torch.autograd.backward([out_v, Ld], [t(cv), t(cl)])
        sdf2 = t(s["sdf"]).requires_grad_(True)
        ent = _Entropy.apply(sdf2, tuple(s["res"]))
        ent.backward(torch.tensor(0.7, device=cuda))
        torch.cuda.synchronize()
        return dict(out_vertices=out_v, faces=faces, L_dev=Ld, entropy=ent), dict(grads=[i.grad for i in ins], ent_g=sdf2.grad)

    def check(atomic, mode):
        worst = 0.0
        for k, g in zip(("g_vertices", "g_sdf", "g_alpha", "g_beta", "g_gamma"), atomic["grads"]):
            got = g.cpu().numpy().reshape(b[k].shape)
            assert not np.ascontiguousarray(got).view(np.int32)[b[k + "_n"] == 0].any(), (mode, k)
            worst = max(worst, util.assert_within_budget(f"poisoned {mode} {k}", got, b[k], b[k + "_budget"], util.FC_BUDGET_KAPPA))
        worst = max(worst, util.assert_within_budget(f"poisoned {mode} entropy g_sdf", atomic["ent_g"].cpu().numpy().reshape(eb["g_sdf"].shape),
                                                     eb["g_sdf"], eb["g_sdf_budget"], util.FC_BUDGET_KAPPA))
        return worst

    outs = _three_runs("FlexiCubes", lambda: run(sc, w, cv_h, cl_h),
                       lambda: run(big, dict(alpha=big["alpha"], beta=big["beta"], gamma=big["gamma"]), None, None), check)
    e = outs["ones"][0]
    assert np.array_equal(e["faces"].cpu().numpy(), b["faces"])
    util.assert_within_budget("poisoned out_vertices", e["out_vertices"].detach().cpu().numpy(), b["out_vertices"], b["out_vertices_budget"], util.FC_BUDGET_KAPPA)
    util.assert_within_budget("poisoned L_dev", e["L_dev"].detach().cpu().numpy(), b["L_dev"], b["L_dev_budget"], util.FC_BUDGET_KAPPA)
    util.assert_within_budget("poisoned entropy", e["entropy"].detach().cpu().numpy().reshape(1), [eb["entropy"]], [eb["entropy_budget"]], util.FC_BUDGET_KAPPA)


# ------------------------------------------------------------------------------------------------------------ TSDF, Poisson
def _random_volume(cuda, res, seed):
    import geosplatting_amd as gs
    rng = np.random.default_rng(seed)
    n = res[0] * res[1] * res[2]
    tv = (rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.05, 1.0, size=n)).astype(np.float32)
    tv[rng.random(n) < 0.05] = 0.0
    w = np.where(rng.random(n) < 0.3, 0.0, rng.integers(1, 9, size=n)).astype(np.float32)
    vol = gs.TSDFVolume(res, bounds=((-0.3, 0.1, 1.0), (0.9, 1.1, 1.9)), device=cuda)
    vol.volume.copy_(torch.from_numpy(np.stack((tv, w), -1).reshape(res[2], res[1], res[0], 2)))
    return vol


def test_tsdf_extraction(cuda):
    """gs_tsdf_extract_count / _fill through TSDFVolume.extract_mesh: 12 x 10 x 9 (five blocks of voxels, the last partial)"""
    from tests import test_gpu_fusion as TF
    vol, big = _random_volume(cuda, (12, 10, 9), 11), _random_volume(cuda, (15, 13, 11), 12)

    def run(v):
        verts, faces = v.extract_mesh()
        torch.cuda.synchronize()
        return dict(vertices=verts, faces=faces, counts=list(v.last_counts)), {}

    outs = _three_runs("TSDF extraction", lambda: run(vol), lambda: run(big))
    assert outs["zero"][0]["faces"].shape[0] > 50
    with poisoned("ones"):
        TF._check_extraction(vol, "random 12x10x9 on 0xFF scratch")                # the module's own check against tests/tsdf_ref.py


def test_grid_splat(cuda):
    """gs_grid_splat through splat_to_grid: the smallest full case of tests/test_gpu_poisson.py (N = 1 000 + the awkward rows, C = 1,
    8 x 8 x 8), and through mesh_from_indicator, which reaches the TSDF extraction from poisson.py"""
    import geosplatting_amd as gs
    from tests import test_gpu_poisson as TP
    c, big = TP._case(1000, 1, (8, 8, 8)), TP._case(1000, 3, (8, 12, 10))
    phi = TP._sphere_phi((16, 16, 16)).to(cuda)
    ax = [(torch.arange(r) + 0.5) / r - 0.5 for r in (24, 20, 28)]
    phi_big = (0.3 - torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).norm(dim=-1)).to(cuda)      # a sphere on another grid

    def run(cs, res, ph):
        out = gs.splat_to_grid(cs["p"].to(cuda), cs["v"].to(cuda), res)
        v, f, n = gs.mesh_from_indicator(ph)
        torch.cuda.synchronize()
        return dict(grid=out, mesh_v=v, mesh_f=f, mesh_n=n), {}

    outs = _three_runs("grid splat + mesh_from_indicator", lambda: run(c, (8, 8, 8), phi), lambda: run(big, (8, 12, 10), phi_big))
    assert TP._ratio(outs["ones"][0]["grid"], c["splat"], c["splat_bud"]) <= 1.0


# ------------------------------------------------------------------------------------------------------------ mesh rasterizer
@pytest.mark.parametrize("near_clip", [False, True], ids=["plain", "near_clip"])
def test_mesh_rasterizer(cuda, near_clip):
    """gs_meshraster_* / gs_meshclip_* through rasterize_mesh: icosphere(1) around the camera's near plane at 37 x 53 (faces in front,
    crossing and behind), against tests/meshraster_ref.py where no face crosses"""
    import geosplatting_amd as gs
    from geosplatting_amd.synthetic import icosphere
    from tests import meshraster_ref as ref

    def mesh(level, radius, z):
        v, f = icosphere(level, radius)
        return (v + torch.tensor([0.05, -0.03, z])).to(cuda), f.to(cuda)

    v, f = mesh(1, 0.5, 0.45 if near_clip else 1.6)                                 # near_clip: the sphere straddles z = near
    vb, fb = mesh(2, 0.5, 1.6)
    intr = (40.0, 42.0, 26.5, 18.5, 37, 53)
    intr_big = (60.0, 60.0, 40.0, 30.0, 61, 83)

    def run(vv, ff, it):
        rast = gs.rasterize_mesh(vv, ff, it, cull="none", near=0.1, near_clip=near_clip)
        torch.cuda.synchronize()
        return dict(rast=rast), {}

    outs = _three_runs(f"mesh rasterizer (near_clip={near_clip})", lambda: run(v, f, intr), lambda: run(vb, fb, intr_big))
    rast = outs["ones"][0]["rast"]
    covered = int((rast[..., 3] > 0).sum())
    assert covered > 100
    if not near_clip:
        res = ref.rasterize(v.cpu().numpy(), f.cpu().numpy(), intr, cull="none", near=0.1)
        solid = ~res["fragile"]
        assert np.array_equal((rast[..., 3].long() - 1).cpu().numpy()[solid], res["face"][solid])


# ------------------------------------------------------------------------------------------------------------ BVH, NN grid
def test_bvh(cuda):
    """gs_bvh_build (with the radix passes of gs_isect_sort inside), then closest-hit and occlusion: icosphere(2), 320 faces"""
    import geosplatting_amd as gs
    from geosplatting_amd.synthetic import icosphere
    g = torch.Generator().manual_seed(4)
    o = (torch.randn(700, 3, generator=g) * 0.1).to(cuda)
    d = torch.nn.functional.normalize(torch.randn(700, 3, generator=g), dim=-1).to(cuda)

    def run(level):
        v, f = icosphere(level, 0.5)
        bvh = gs.MeshBVH(v.to(cuda), f.to(cuda))
        t, face, bary = bvh.closest_hit(o, d)
        occ = bvh.occluded(o, d)
        tb, fb, bb = bvh.closest_hit(o, d, brute_force=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(t), _bits(tb)) and torch.equal(face, fb) and torch.equal(_bits(bary), _bits(bb))      # as test_gpu_raytrace
        return dict(nodes=bvh.nodes, t=t, face=face, bary=bary, occ=occ), {}

    outs = _three_runs("BVH build + closest hit", lambda: run(2), lambda: run(3))
    assert int((outs["ones"][0]["face"] >= 0).sum()) > 600                           # the rays start inside the closed sphere


def test_nn_grid(cuda):
    """gs_nn_build, then the 1- and 3-nearest queries: M = 1 000 points (four blocks, the last partial), against tests/chamfer_ref.py"""
    import geosplatting_amd as gs
    from tests import chamfer_ref as ref
    from tests import test_gpu_nn as TN
    p, q = ref.cloud(1000, 31), ref.cloud(777, 32)
    pb = ref.cloud(2500, 33)

    def run(points):
        grid = gs.PointGrid(torch.from_numpy(np.ascontiguousarray(points)).to(cuda))
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(cuda)
        d1, i1 = grid.nearest(qd)
        d3, i3 = grid.k_nearest(qd, 3)
        torch.cuda.synchronize()
        return dict(d1=d1, i1=i1, d3=d3, i3=i3), {}                                  # (the grid buffer is sized for the most cells: its tail is never written)

    outs = _three_runs("NN grid build + query", lambda: run(p), lambda: run(pb))
    e = outs["ones"][0]
    d_ref, i_ref = ref.nearest_f32(q, p)
    TN._same(e["d1"], e["i1"], d_ref, i_ref, "poisoned nearest")


# ------------------------------------------------------------------------------------------------------------ densify
def test_densify(cuda):
    """gs_densify_plan / gs_densify_fill through GaussianSet.densify_and_cull: the golden of tests/test_gpu_densify.py (num_splits = 2)"""
    from tests import test_gpu_densify as TD
    from tests.test_densify_cpu import check_against_golden, golden_kwargs, load_golden
    G = load_golden()
    assert int(G["num_splits"]) == 2
    kw = golden_kwargs(G)

    def run(reps):
        P = {k: np.concatenate([G[k]] * reps) for k in TD.FIELDS}
        g = TD._set(P, cuda)
        g.xys_grad_norm = torch.tensor(np.concatenate([G["xys_grad_norm"]] * reps), device=cuda)
        g.vis_counts = torch.tensor(np.concatenate([G["vis_counts"]] * reps), device=cuda)
        g.last_width, g.last_height = float(G["last_width"]), float(G["last_height"])
        randn = torch.tensor(G["randn"], device=cuda)
        randn = randn if reps == 1 else torch.cat([randn] * reps, dim=1)
        idx = g.densify_and_cull(randn=randn, **kw)
        torch.cuda.synchronize()
        return dict(indices=idx, totals=list(g.last_totals), **{k: getattr(g, k).detach() for k in TD.FIELDS}), {}

    outs = _three_runs("densify", lambda: run(1), lambda: run(2))
    e = outs["ones"][0]
    assert e["totals"] == [int(v) for v in G["totals"]]
    check_against_golden(G, {k: e[k].cpu().numpy() for k in TD.FIELDS}, e["indices"].cpu().numpy())
