"""GPU: the FlexiCubes extraction (csrc/gs_flexicubes.hip) against oracle/flexicubes_ref.py, ELEMENT BY ELEMENT.

Topology bit for bit (the eight counts, the faces and -- read back from the workspace -- the resolved case of every cube, the dual-vertex
and L_dev row base of every surface cube and the quad id of every edge slot); every value and every gradient within the oracle's
budget, |got - want| <= kappa * 2^-24 * budget (oracle.flexicubes_ref.extract_budget / entropy_budget; validated against the float32
restatement in tests/test_flexicubes_budget_cpu.py); an element no contribution reaches is bitwise +0, or keeps the pre-filled
pattern's bits under accumulate = 1.  The entry points are called through the C ABI, so the branches the Python wrapper never takes
are reached: each of alpha / beta / gamma NULL on its own, v_L_dev = NULL, an all-zero v_out_vertices, sdf_eps = 0, weight_scale = 0.5,
accumulate = 1 of the entropy backward, a short workspace and mismatched gradient buffers.  Scenes and cases: tests/util.py
(FC_BUDGET_SCENES, fc_budget_cases).

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X over all cases of the unchanged library, with the float32 restatement's
figure on the CPU (tests/test_flexicubes_budget_cpu.py, bar kappa / 2) beside it; kappa = util.FC_BUDGET_KAPPA = util.MESH_BUDGET_KAPPA
= 4, the smallest power of two that is at least 4 x the worst figure:
    entry point                  tensor          MI355X    CPU float32
    gs_flexicubes_fwd            out_vertices     0.347      0.347
    gs_flexicubes_fwd            L_dev            0.087      0.093
    gs_flexicubes_bwd            g_vertices       0.503      0.503
    gs_flexicubes_bwd            g_sdf            0.128      0.301
    gs_flexicubes_bwd            g_alpha          0.254      0.531
    gs_flexicubes_bwd            g_beta           0.186      0.168
    gs_flexicubes_bwd            g_gamma          0.036      0.056
    gs_flexicubes_entropy_fwd    entropy          0.128      0.208
    gs_flexicubes_entropy_bwd    g_sdf acc0       0.418      0.421
    gs_flexicubes_entropy_bwd    g_sdf acc1       0.983        -
    gs_vertex_normals_fwd        vnormals         0.239      0.235
    gs_vertex_normals_bwd        g_vertices       0.073      0.063
    gs_mgadapter_fwd             means / scales / quats / normals    0.546 / 0.382 / 0.195 / 0.352      0.556 / 0.233 / 0.210 / 0.450
    gs_mgadapter_bwd             g_vertices / g_vnormals             0.020 / 0.037                      0.021 / 0.032
The 0.983 alone sets kappa, and it is legitimate: under accumulate = 1 an element with one contribution c on top of a pattern value p
is charged |p| + |c| for one addition whose rounding is at most 2^-24 |p + c|; the bound is attained when p and c have the same sign
and cannot be exceeded by correct code.  Everything else stays near or below half a budget.  The mgadapter gradients' 0.02 says that
their budget is loose: each face's contribution is charged 77 roundings of sum |g d| for the 78-term dot product the kernel sums in
sequence.  No quaternion came out with the opposite sign on either hand-off mesh.  No kernel bug showed.

Budgets (units of 2^-24, first order, float64 intermediates).  Forward: running bounds of the interpolation weight, the weighted sum and
its division, the distances, their mean and |d - mean| by its operands.  Backward: every contribution a slot collects through atomics
(g_vertices, g_sdf, g_gamma, the dual-vertex scratch) carries its own bound, and the slot is charged (n - 1) * sum of the sizes of the
terms on top; ue - vd (beta), v02 - ctr / v13 - ctr (gamma), d_j - mean and its sign (L_dev), 1 - tanh^2 and 1 - sigmoid are charged by
their operands, and so are sum_c g_c (xb_c - xa_c) and d w / d A = 1 / D - A / D^2, which float32 autograd of the restatement evaluates
as differences.  Nothing is left out of a comparison (0 elements excluded in every case): where the reference is not differentiable
(|d_j - mean|, or the distance d_j, inside its own rounding bound) the jump 2 |v_L| is charged to the elements it reaches; their count
is printed (at most 12 of 1 716 g_sdf elements, `zeros`).  The hand-off: csrc/gs_mesh.hip's operations evaluated on (value, bound)
pairs and on the kernels' dual numbers over such pairs (oracle/mesh_ref.py); a cross product is charged by the sizes of its products,
a vertex by its valence.

Whether the tests bite.  Each one-line change below (arithmetic only, every address in bounds) was built into a scratch library, never
committed, and this module and tests/test_gpu_flexicubes.py / tests/test_gpu_mesh.py ("old") were run against it once on an MI355X;
the first failing element of the first failing new case is quoted.  The unchanged scratch library passes new and old.
 (a) dwz not scaled by 1 - sdf_eps -- FAILS the 6 cases with sdf_eps = 0.05 and a cotangent on L_dev (first rand_a0-abg-eps0.05-ws0.5-
     ldev, g_sdf[121] got 2.5233 want 2.2906, ratio 6 263).  Old: 1 fails (vs_float64 with eps 0.05).
 (b) gd[j] taking +v_L for df < 0 -- FAILS all 23 cases with a cotangent on L_dev (first rand_a0-abg-dense, g_vertices[1092, 2] got
     -0.198 want -0.061, ratio 217 240).  Old: 8 fail (every golden and vs_float64 case).
 (c) gd[j] -= ssum / cnt dropped -- FAILS the same 23 (g_vertices[119, 1] got 1.224 want 0.071, ratio 351 557).  Old: 8 fail.
 (d) gv -= zg dropped -- FAILS the same 23 (g_vertices[119, 2] got -0.205 want -0.581, ratio 105 661).  Old: 8 fail.
 (e) dg[0] using q.gm[0] -- FAILS all 13 cases with gamma (first rand_a0-abg-dense, g_gamma[1228] got 0.0664 want 0.0206, ratio
     120 199).  Old: 6 fail (the goldens with weights, vs_float64 with weights).
 (f) weight_scale dropped from the gamma derivative -- FAILS the same 13 (g_gamma[422] got -0.06830 want -0.06762, ratio 819: the 1 %
     of weight_scale = 0.99).  Old: 6 fail.
 (g) the forward L_dev pass interpolating with the alpha-weighted values -- FAILS all 16 cases with alpha (first rand_a0-abg-dense,
     L_dev[11] got 0.814 want 0.105, ratio 233 534).  Old: 6 fail.
 (h) the flip test sf >= 0 in fc_slot -- FAILS test_topology_bit_for_bit[zeros] (counts: 128 flipped quads for 107) and both `zeros`
     cases (faces).  Old: all 10 pass -- no old case has a grid vertex with sdf == 0.
 (i) fc_case complementing whenever the neighbour exists -- FAILS 9 topology cases (atlas: Q 2 984 for 2 824) and 26 extract cases (all
     but one_cube, one_quad and decades, which have no ambiguous cube with a neighbour).  Old: 6 fail.
 (j) accumulate ignored in the entropy backward -- FAILS all 12 test_entropy_within_budget cases (untouched elements lose the
     pattern's bits).  Old: all 10 pass -- accumulate is always 0 there.
 (k) the n (n.g) projection dropped in vnormal_bwd_vertex_kernel -- FAILS the 3 hand-off tests (first atlas, vertex-normal
     g_vertices[151, 0] got 86.53 want 10.61, ratio 290 451).  Old: 1 fails (test_vertex_normals_golden_and_gradient).
 (l) the second ring constant of mgadapter_face off by 1 % -- FAILS the 3 hand-off tests (first atlas, means[52063, 1] got 0.001757 want
     0.000463, ratio 60 048).  Old: 6 fail.
So the old max-norm tests do notice (a)-(g), (i), (k) and (l) -- a wrong term of the size of the gradient moves the largest elements
too -- and the expectation that they would not is not borne out; what only this module sees are (h) and (j), the zero-budget
elements, and every error below 1e-4 of a tensor's largest element.

Run with -s to print the ratio of every check.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import flexicubes_ref as O
from tests import util
from tests.test_flexicubes_budget_cpu import case_budget, check_jump_cap, scene, scene_topology

pytestmark = pytest.mark.gpu

KAPPA = util.FC_BUDGET_KAPPA
CASES = util.fc_budget_cases()
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module's tests: the worst ratio per entry point and tensor over whatever ran (shown with -s)"""
    yield
    print()
    for key in sorted(WORST):
        print(f"    {key[0]:28s} {key[1]:14s} {WORST[key]:7.3f}")


def _record(entry, nm, r):
    WORST[(entry, nm)] = max(WORST.get((entry, nm), 0.0), r)


def _al256(n):
    return (n + 255) & ~255


def _ws_views(ws, res):
    """the workspace arrays gs_flexicubes_count leaves behind (layout of fc_ws: a 64-int header, then case8 [C] bytes, vd_base [C],
    k_base [C], quad_id [3 Vg] ints, each 256-byte aligned)"""
    R0, R1, R2 = res
    Cn, Vg = R0 * R1 * R2, (R0 + 1) * (R1 + 1) * (R2 + 1)
    h = ws.cpu().numpy()
    o = 256
    case8 = h[o:o + Cn].copy(); o += _al256(Cn)
    vd_base = h[o:o + 4 * Cn].view(np.int32).copy(); o += _al256(4 * Cn)
    k_base = h[o:o + 4 * Cn].view(np.int32).copy(); o += _al256(4 * Cn)
    quad_id = h[o:o + 12 * Vg].view(np.int32).copy()
    return case8, vd_base, k_base, quad_id


def _count(cuda, sc):
    from geosplatting_amd import _lib as L
    lib = L.lib()
    R0, R1, R2 = sc["res"]
    nbytes = int(lib.gs_flexicubes_ws_bytes(R0, R1, R2))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=cuda)
    counts = torch.full((8,), -7, dtype=torch.int64, device=cuda)
    sdf = torch.tensor(sc["sdf"], device=cuda)
    L.check(lib.gs_flexicubes_count(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes), L.ptr(counts), L.stream()), "gs_flexicubes_count")
    torch.cuda.synchronize()
    return sdf, ws, nbytes, counts.cpu().tolist()


def _dev(cuda, a):
    return None if a is None else torch.tensor(a, device=cuda)


def _fwd(cuda, sc, w, eps, wsc, sdf, ws, nbytes, Q, nq, K):
    from geosplatting_amd import _lib as L
    R0, R1, R2 = sc["res"]
    x = _dev(cuda, sc["vertices"])
    a, b, g = (_dev(cuda, w[k]) for k in ("alpha", "beta", "gamma"))
    out_v = torch.full((Q + nq, 3), 123.0, device=cuda); faces = torch.full((4 * nq, 3), -5, dtype=torch.int64, device=cuda)
    Ld = torch.full((K,), 123.0, device=cuda)
    rc = L.lib().gs_flexicubes_fwd(R0, R1, R2, L.ptr(x), L.ptr(sdf), L.ptr(a), L.ptr(b), L.ptr(g), L.f32(wsc), L.f32(-1.0 if eps is None else eps),
                                   L.ptr(ws), C.c_size_t(nbytes), L.i64(Q), L.i64(nq), L.i64(K), L.ptr(out_v), L.ptr(faces), L.ptr(Ld), L.stream())
    torch.cuda.synchronize()
    return rc, (x, a, b, g), out_v, faces, Ld


def _bwd(cuda, sc, eps, wsc, sdf, ws, nbytes, Q, nq, K, ins, out_v, cv, cl, grads=None):
    from geosplatting_amd import _lib as L
    R0, R1, R2 = sc["res"]
    x, a, b, g = ins
    if grads is None:
        grads = [torch.full_like(x, 123.0), torch.full_like(sdf, 123.0)] + [None if t is None else torch.full_like(t, 123.0) for t in (a, b, g)]
    scratch = torch.full((Q, 3), 123.0, device=cuda)
    rc = L.lib().gs_flexicubes_bwd(R0, R1, R2, L.ptr(x), L.ptr(sdf), L.ptr(a), L.ptr(b), L.ptr(g), L.f32(wsc), L.f32(-1.0 if eps is None else eps),
                                   L.ptr(ws), C.c_size_t(nbytes), L.i64(Q), L.i64(nq), L.i64(K), L.ptr(out_v), L.ptr(cv), L.ptr(cl), L.ptr(scratch),
                                   *[L.ptr(t) for t in grads], L.stream())
    torch.cuda.synchronize()
    return rc, grads


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", list(util.FC_BUDGET_SCENES))
def test_topology_bit_for_bit(cuda, name):
    """the scans where they happen: counts, resolved cases, dual-vertex / L_dev row bases and quad ids from the workspace, then the faces;
    two forward calls give the same bits"""
    sc, aux = scene(name), scene_topology(name)
    sdf, ws, nbytes, counts = _count(cuda, sc)
    N, Q, nq, K = len(aux["surf_cubes"]), aux["Q"], aux["num_quads"], aux["K"]
    assert counts == [N, Q, K, aux["E"], nq, aux["num_flipped"], 0, 0]
    case8, vd_base, k_base, quad_id = _ws_views(ws, sc["res"])
    assert np.array_equal(case8, aux["case8"])
    sid = aux["surf_cubes"]
    assert np.array_equal(vd_base[sid], aux["vd_base"]) and np.array_equal(k_base[sid], aux["k_base"])
    assert np.array_equal(quad_id, aux["quad_id"])
    w = dict(alpha=sc["alpha"], beta=sc["beta"], gamma=sc["gamma"])
    d = lambda t: torch.from_numpy(t.astype(np.float64))
    faces_ref = O.extract(d(sc["vertices"]), d(sc["sdf"]), sc["res"])[1].numpy()
    runs = []
    for _ in range(2):
        rc, _, out_v, faces, Ld = _fwd(cuda, sc, w, None, 0.99, sdf, ws, nbytes, Q, nq, K)
        assert rc == 0
        runs.append((out_v.cpu().numpy(), faces.cpu().numpy(), Ld.cpu().numpy()))
    assert runs[0][1].shape == (4 * nq, 3) and np.array_equal(runs[0][1], faces_ref)
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))
    assert np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("case", CASES, ids=util.fc_case_id)
def test_extract_within_budget(cuda, case):
    """gs_flexicubes_fwd / gs_flexicubes_bwd over 123-filled outputs: every element of out_vertices, L_dev, g_vertices, g_sdf, g_alpha,
    g_beta, g_gamma within its budget, the elements no contribution reaches bitwise +0"""
    name, _, eps, wsc, kind = case
    sc = scene(name)
    w, cv_h, cl_h, b = case_budget(case)
    lab = util.fc_case_id(case)
    check_jump_cap(lab, b)
    aux = b["aux"]
    Q, nq, K = aux["Q"], aux["num_quads"], b["L_dev"].shape[0]
    sdf, ws, nbytes, counts = _count(cuda, sc)
    assert counts[1:3] == [Q, K] and counts[4] == nq
    rc, ins, out_v, faces, Ld = _fwd(cuda, sc, w, eps, wsc, sdf, ws, nbytes, Q, nq, K)
    assert rc == 0
    assert np.array_equal(faces.cpu().numpy(), b["faces"])
    _record("gs_flexicubes_fwd", "out_vertices", util.assert_within_budget(f"{lab} out_vertices", out_v.cpu().numpy(), b["out_vertices"],
                                                                           b["out_vertices_budget"], KAPPA))
    _record("gs_flexicubes_fwd", "L_dev", util.assert_within_budget(f"{lab} L_dev", Ld.cpu().numpy(), b["L_dev"], b["L_dev_budget"], KAPPA))
    rc, grads = _bwd(cuda, sc, eps, wsc, sdf, ws, nbytes, Q, nq, K, ins, out_v, _dev(cuda, cv_h), _dev(cuda, cl_h))
    assert rc == 0
    for k, t in zip(("g_vertices", "g_sdf", "g_alpha", "g_beta", "g_gamma"), grads):
        assert (t is None) == (k not in b), k
        if t is None:
            continue
        got = t.cpu().numpy().reshape(b[k].shape)
        assert not _bits(got)[b[k + "_n"] == 0].any(), f"{lab} {k}: an element without a contribution is not +0"
        _record("gs_flexicubes_bwd", k, util.assert_within_budget(f"{lab} {k}", got, b[k], b[k + "_budget"], KAPPA))


@pytest.mark.parametrize("name", list(util.FC_BUDGET_SCENES))
def test_entropy_within_budget(cuda, name):
    """gs_flexicubes_entropy_fwd, and gs_flexicubes_entropy_bwd with accumulate = 0 and accumulate = 1 over the same random pattern:
    accumulate = 0 overwrites it (untouched elements +0), accumulate = 1 adds to it (untouched elements keep the pattern's bits; an
    element collecting n contributions is charged n |p| + sum |c| more: every addition may round a sum that holds p)"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc = scene(name)
    R0, R1, R2 = sc["res"]
    b = O.entropy_budget(sc["sdf"], sc["res"], v_out=0.7)
    sdf, ws, nbytes, counts = _count(cuda, sc)
    assert counts[3] == b["E"]
    outs = []
    for _ in range(2):
        out = torch.full((1,), 123.0, device=cuda)
        L.check(lib.gs_flexicubes_entropy_fwd(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes), L.ptr(out), L.stream()), "entropy_fwd")
        outs.append(out.cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    _record("gs_flexicubes_entropy_fwd", "entropy", util.assert_within_budget(f"{name} entropy", outs[0], [b["entropy"]], [b["entropy_budget"]], KAPPA))
    pat = np.random.RandomState(9).uniform(-2, 2, sc["sdf"].shape).astype(np.float32)
    v = torch.tensor([0.7], device=cuda)
    n0 = b["g_sdf_n"] == 0
    for acc in (0, 1):
        g = torch.tensor(pat, device=cuda)
        L.check(lib.gs_flexicubes_entropy_bwd(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes), L.ptr(v), L.ptr(g), acc, L.stream()), "entropy_bwd")
        torch.cuda.synchronize()
        got = g.cpu().numpy()
        if acc == 0:
            assert not _bits(got)[n0].any()
            want, bud = b["g_sdf"], b["g_sdf_budget"]
        else:
            assert np.array_equal(_bits(got)[n0], _bits(pat)[n0])
            want = b["g_sdf"] + pat
            bud = np.where(n0, 0.0, b["g_sdf_budget"] + b["g_sdf_n"] * np.abs(pat) + b["g_sdf_abs"])
        _record("gs_flexicubes_entropy_bwd", f"g_sdf acc{acc}", util.assert_within_budget(f"{name} entropy g_sdf acc{acc}", got, want, bud, KAPPA))


def test_refusals_leave_outputs_alone(cuda):
    """a workspace one byte short and gradient buffers that do not match the given weights: an error code, and nothing written"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    sc, aux = scene("thin"), scene_topology("thin")
    R0, R1, R2 = sc["res"]
    Q, nq, K = aux["Q"], aux["num_quads"], aux["K"]
    sdf, ws, nbytes, _ = _count(cuda, sc)
    w = dict(alpha=sc["alpha"], beta=sc["beta"], gamma=sc["gamma"])
    counts = torch.full((8,), -7, dtype=torch.int64, device=cuda)
    assert lib.gs_flexicubes_count(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes - 1), L.ptr(counts), L.stream()) != 0
    assert counts.cpu().tolist() == [-7] * 8
    rc, ins, out_v, faces, Ld = _fwd(cuda, sc, w, None, 0.99, sdf, ws, nbytes - 1, Q, nq, K)
    assert rc != 0 and bool((out_v == 123.0).all()) and bool((faces == -5).all()) and bool((Ld == 123.0).all())
    rc, ins, out_v, faces, Ld = _fwd(cuda, sc, w, None, 0.99, sdf, ws, nbytes, Q, nq, K)
    assert rc == 0
    cv, cl = (_dev(cuda, t) for t in util.fc_budget_cotangents("dense", Q, nq, K, seed=1))
    untouched = lambda gs: all(t is None or bool((t == 123.0).all()) for t in gs)
    rc, grads = _bwd(cuda, sc, None, 0.99, sdf, ws, nbytes - 1, Q, nq, K, ins, out_v, cv, cl)
    assert rc != 0 and untouched(grads)
    for drop in (2, 3, 4):                                               # alpha / beta / gamma given, its gradient buffer NULL
        grads = [torch.full_like(ins[0], 123.0), torch.full_like(sdf, 123.0)] + [torch.full_like(t, 123.0) for t in ins[1:]]
        grads[drop] = None
        rc, grads = _bwd(cuda, sc, None, 0.99, sdf, ws, nbytes, Q, nq, K, ins, out_v, cv, cl, grads=grads)
        assert rc != 0 and untouched(grads)
    grads = [torch.full_like(ins[0], 123.0), torch.full_like(sdf, 123.0)] + [torch.full_like(t, 123.0) for t in ins[1:]]
    rc, grads = _bwd(cuda, sc, None, 0.99, sdf, ws, nbytes, Q, nq, K, (ins[0], None, ins[2], ins[3]), out_v, cv, cl, grads=grads)
    assert rc != 0 and untouched(grads)                                  # a gradient buffer for an absent alpha
    out = torch.full((1,), 123.0, device=cuda)
    assert lib.gs_flexicubes_entropy_fwd(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes - 1), L.ptr(out), L.stream()) != 0
    g = torch.full_like(sdf, 123.0)
    assert lib.gs_flexicubes_entropy_bwd(R0, R1, R2, L.ptr(sdf), L.ptr(ws), C.c_size_t(nbytes - 1), L.ptr(out), L.ptr(g), 0, L.stream()) != 0
    torch.cuda.synchronize()
    assert float(out) == 123.0 and bool((g == 123.0).all())


# ---- the hand-off of extracted meshes: vertex_normals, then mesh_to_splats (csrc/gs_mesh.hip), each stage on identical float32 inputs
MESH_KAPPA = util.MESH_BUDGET_KAPPA


def _handoff_gpu(cuda, v, f, cot, a):
    """vertex_normals -> mesh_to_splats on the GPU with each stage cut loose from the other: returns the normals, the splat outputs, the
    gradients of mesh_to_splats to its two inputs for `cot`, and the gradient of vertex_normals for the cotangent `a`"""
    from geosplatting_amd.mesh import mesh_to_splats, vertex_normals
    fc = torch.tensor(f, device=cuda)
    vc = torch.tensor(v, device=cuda).requires_grad_(True)
    vn = vertex_normals(vc, fc)
    vn.backward(torch.tensor(a, device=cuda))
    g_vn_stage = vc.grad.cpu().numpy()
    vc2 = torch.tensor(v, device=cuda).requires_grad_(True)
    nc = vn.detach().clone().requires_grad_(True)
    sp, nrm = mesh_to_splats(vc2, fc, nc)
    return vn.detach().cpu().numpy(), (vc2, nc, sp, nrm), g_vn_stage


def _splat_backward(cuda, handles, cot, sign):
    vc2, nc, sp, nrm = handles
    t = [torch.tensor(c, device=cuda) for c in cot]
    ((sp.means * t[0]).sum() + (sp.scales * t[1]).sum() + (sp.quats * torch.tensor(sign, device=cuda) * t[2]).sum() + (nrm * t[3]).sum()).backward()
    return vc2.grad.cpu().numpy(), nc.grad.cpu().numpy()


@pytest.mark.parametrize("name", util.FC_HANDOFF_SCENES)
def test_handoff_within_budget(cuda, name):
    """the mesh the oracle extracts from the scene (four triangles fanned round every quad centre, neighbour valence 3 .. 14, slivers,
    vertices on no face): vertex normals and their gradient, then the six Gaussians of every face and the gradients to the vertices
    and to the normals, every element within budget; quaternions modulo sign"""
    from tests.test_flexicubes_budget_cpu import handoff_cotangents, handoff_mesh, handoff_normals_budget
    from oracle import mesh_ref
    v, f = handoff_mesh(name)
    cot, a = handoff_cotangents(name, f.shape[0], v.shape[0])
    b = handoff_normals_budget(name)
    vn, handles, g_stage = _handoff_gpu(cuda, v, f, cot, a)
    iso = b["isolated"]
    assert np.array_equal(vn[iso], np.tile(np.float32([0, 0, 1]), (int(iso.sum()), 1)))
    _record("gs_vertex_normals_fwd", "vnormals", util.assert_within_budget(f"{name} vnormals", vn, b["vnormals"], b["vnormals_budget"], MESH_KAPPA))
    assert not _bits(g_stage)[b["g_vertices_n"] == 0].any()
    _record("gs_vertex_normals_bwd", "g_vertices", util.assert_within_budget(f"{name} vnormals g_vertices", g_stage, b["g_vertices"],
                                                                             b["g_vertices_budget"], MESH_KAPPA))
    sp, nrm = handles[2], handles[3]
    q = sp.quats.detach().cpu().numpy()
    plain = mesh_ref.mesh_to_splats_budget(v, f, vn)
    sign = np.sign((q.astype(np.float64) * plain["quats"]).sum(-1, keepdims=True)).astype(np.float32)
    assert np.abs(sign).min() == 1
    print(f"  {name}: {int((sign < 0).sum())} of {sign.size} quaternions come out with the opposite sign")
    mb = mesh_ref.mesh_to_splats_budget(v, f, vn, cot, quat_sign=sign)
    for k, got in (("means", sp.means), ("scales", sp.scales), ("quats", sp.quats), ("normals", nrm)):
        _record("gs_mgadapter_fwd", k, util.assert_within_budget(f"{name} {k}", got.detach().cpu().numpy(), mb[k], mb[k + "_budget"], MESH_KAPPA))
    gv, gn = _splat_backward(cuda, handles, cot, sign)
    for k, got in (("g_vertices", gv), ("g_vnormals", gn)):
        assert not _bits(got)[mb[k + "_n"] == 0].any()
        _record("gs_mgadapter_bwd", k, util.assert_within_budget(f"{name} splats {k}", got, mb[k], mb[k + "_budget"], MESH_KAPPA))


def test_handoff_degenerate_mesh(cuda):
    """a face with two coincident vertices, a collinear face, a vertex whose face normals cancel, an isolated vertex, next to a healthy
    octahedron that shares no vertex with them: forward outputs within budget of the restatement everywhere (the clamps and the
    (0, 0, 1) constants are taken the same way), gradients finite everywhere and, on the octahedron, within budget"""
    from oracle import mesh_ref
    v, f, healthy = util.mesh_degenerate()
    F, V = f.shape[0], v.shape[0]
    r = np.random.RandomState(12)
    cot = [r.standard_normal((6 * F, w)).astype(np.float32) for w in (3, 3, 4, 3)]
    a = r.standard_normal((V, 3)).astype(np.float32)
    vn, handles, g_stage = _handoff_gpu(cuda, v, f, cot, a)
    hv = np.zeros(V, bool); hv[np.unique(f[healthy])] = True
    b = mesh_ref.vertex_normals_budget(v, f[healthy], a)
    want_rest = np.tile(np.float32([0, 0, 1]), (V, 1))                    # zero raw normal or no face: the fixing constant
    want_rest[[15, 16]] = [0, 0, -1]                                      # 13-16 carry their one face's normal, exactly +-(0, 0, 1)
    assert np.array_equal(vn[~hv], want_rest[~hv])
    util.assert_within_budget("degenerate vnormals", vn[hv], b["vnormals"][hv], b["vnormals_budget"][hv], MESH_KAPPA)
    # vertex 12's own normal is the constant and passes no gradient on, but its position still moves the normals of 13-16
    assert np.isfinite(g_stage).all() and not g_stage[17].any() and g_stage[12].any()
    util.assert_within_budget("degenerate vnormals g_vertices", g_stage[hv], b["g_vertices"][hv], b["g_vertices_budget"][hv], MESH_KAPPA)
    sp, nrm = handles[2], handles[3]
    fwd = mesh_ref.mesh_to_splats_budget(v, f, vn)                        # forward, all faces
    q = sp.quats.detach().cpu().numpy()
    sign = np.sign((q.astype(np.float64) * fwd["quats"]).sum(-1, keepdims=True)).astype(np.float32)
    sign[sign == 0] = 1
    for k, got in (("means", sp.means), ("scales", sp.scales), ("normals", nrm)):
        util.assert_within_budget(f"degenerate {k}", got.detach().cpu().numpy(), fwd[k], fwd[k + "_budget"], MESH_KAPPA)
    util.assert_within_budget("degenerate quats", q * sign, fwd["quats"], fwd["quats_budget"], MESH_KAPPA)
    # a clamp at 1e-10 makes the bound of a degenerate face's outputs meaningless: those are held against the float32 restatement,
    # which takes every clamp and constant the same way on these exactly degenerate inputs
    m32, s32, q32, _, n32 = mesh_ref.mesh_to_splats(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(vn))
    for k, got, want, tol in (("means", sp.means, m32, 2e-6), ("scales", sp.scales, s32, 2e-5), ("quats", sp.quats, q32, 2e-6), ("normals", nrm, n32, 2e-6)):
        err = float((got.detach().cpu() - want).abs().max())
        print(f"  degenerate {k}: max |kernel - float32 restatement| {err:.2e}")
        assert err <= tol, (k, err)
    gv, gn = _splat_backward(cuda, handles, cot, sign)
    assert np.isfinite(gv).all() and np.isfinite(gn).all() and not gv[17].any() and not gn[17].any()
    rows = np.concatenate([part * F + np.nonzero(healthy)[0] for part in range(6)])
    rows_h = np.concatenate([part * int(healthy.sum()) + np.arange(int(healthy.sum())) for part in range(6)])
    assert np.array_equal(np.nonzero(healthy)[0], np.arange(int(healthy.sum())))
    mb = mesh_ref.mesh_to_splats_budget(v, f[healthy], vn, [c[rows] for c in cot], quat_sign=sign[rows])
    assert rows_h.size == rows.size
    for k, got in (("g_vertices", gv), ("g_vnormals", gn)):
        util.assert_within_budget(f"degenerate splats {k}", got[hv], mb[k][hv], mb[k + "_budget"][hv], MESH_KAPPA)
