"""CPU: the FlexiCubes error budgets of oracle/flexicubes_ref.py (extract_budget, entropy_budget) and the scene set of tests/util.py
(FC_BUDGET_SCENES) that tests/test_gpu_flexicubes_budget.py runs the kernels on.

  * the same restatement (`extract`, `entropy`) evaluated in float32 torch with float32 autograd stays within FC_BUDGET_KAPPA / 2
    budgets of the float64 reference, element by element, on every case the GPU module runs; an element with budget 0 is exactly 0;
  * the budget's hand-derived chain rule equals float64 autograd (asserted inside extract_budget);
  * the scene set covers what the kernels branch on: all 254 surface cases raw and resolved, patch counts 1 .. 4, each of the 36
    ambiguous cases complemented and kept (with its neighbour inside the grid), every neighbour direction leaving the grid, more than
    one scan block with a partial last block, grids without any quad, exact zeros of both signs at the ends of crossing edges,
    interpolation weights at 0 and 1, saturated weights;
  * no element is left out of any comparison.  Where the reference is not differentiable (an L_dev term whose d_j - mean, or whose
    distance d_j, lies inside its own rounding bound) the jump is charged to the budget of the elements it reaches, which are still
    compared; their count is printed and is at most 1 in 100 of every tensor in every case.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import flexicubes_ref as O
from oracle import mesh_ref
from tests import util

KAPPA = util.FC_BUDGET_KAPPA
MESH_KAPPA = util.MESH_BUDGET_KAPPA
CASES = util.fc_budget_cases()
GRADS = ("g_vertices", "g_sdf", "g_alpha", "g_beta", "g_gamma")
WORST = {}


@functools.lru_cache(maxsize=None)
def scene(name):
    return util.FC_BUDGET_SCENES[name]()


@functools.lru_cache(maxsize=4)
def case_budget(case):
    name, (ha, hb, hg), eps, ws, kind = case
    sc = scene(name)
    w = dict(alpha=sc["alpha"] if ha else None, beta=sc["beta"] if hb else None, gamma=sc["gamma"] if hg else None)
    aux = scene_topology(name)
    cv, cl = util.fc_budget_cotangents(kind, aux["Q"], aux["num_quads"], aux["K"], seed=len(name) + 7)
    return w, cv, cl, O.extract_budget(sc["vertices"], sc["sdf"], sc["res"], **w, weight_scale=ws, sdf_eps=eps, v_vertices=cv, v_L_dev=cl)


@functools.lru_cache(maxsize=None)
def scene_topology(name):
    sc = scene(name)
    d = lambda a: torch.from_numpy(a.astype(np.float64))
    _, _, L, aux = O.extract(d(sc["vertices"]), d(sc["sdf"]), sc["res"], return_aux=True)
    return dict(aux, K=int(L.shape[0]))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for k in sorted(WORST):
        print(f"    float32 restatement  {k:14s} {WORST[k]:7.3f}")


def _rec(k, r):
    WORST[k] = max(WORST.get(k, 0.0), r)


def check_jump_cap(label, b):
    """the elements whose budget holds a charged discontinuity (criterion from the float64 side alone): counted, at most 1 in 100"""
    for k, m in b["jump"].items():
        n = int(np.count_nonzero(m & (b[k + "_budget"] > 0)))
        if n:
            print(f"  {label} {k}: {n} of {m.size} elements carry a charged discontinuity")
        assert n * 100 <= m.size, (label, k, n, m.size)


@pytest.mark.parametrize("case", CASES, ids=util.fc_case_id)
def test_float32_restatement_within_half_kappa(case):
    name, _, eps, ws, kind = case
    sc = scene(name)
    w, cv, cl, b = case_budget(case)
    check_jump_cap(util.fc_case_id(case), b)
    t = lambda a: None if a is None else torch.from_numpy(a).requires_grad_(True)
    ins = dict(vertices=t(sc["vertices"]), sdf=t(sc["sdf"]), alpha=t(w["alpha"]), beta=t(w["beta"]), gamma=t(w["gamma"]))
    ws32, eps32 = float(np.float32(ws)), None if eps is None else float(np.float32(eps))
    v, f, L = O.extract(ins["vertices"], ins["sdf"], sc["res"], ins["alpha"], ins["beta"], ins["gamma"], weight_scale=ws32, sdf_eps=eps32)
    assert v.dtype == torch.float32 and np.array_equal(f.numpy(), b["faces"])
    loss = (v * torch.from_numpy(cv)).sum() + (0 if cl is None else (L * torch.from_numpy(cl)).sum())
    loss.backward()
    lab = util.fc_case_id(case)
    _rec("out_vertices", util.assert_within_budget(f"{lab} out_vertices", v.detach().numpy(), b["out_vertices"], b["out_vertices_budget"], KAPPA / 2))
    _rec("L_dev", util.assert_within_budget(f"{lab} L_dev", L.detach().numpy(), b["L_dev"], b["L_dev_budget"], KAPPA / 2))
    for k in GRADS:
        if k not in b:
            continue
        got = ins[k[2:]].grad
        got = np.zeros(b[k].shape, np.float32) if got is None else got.numpy().reshape(b[k].shape)
        assert not got[b[k + "_n"] == 0].any(), (lab, k)
        _rec(k, util.assert_within_budget(f"{lab} {k}", got, b[k], b[k + "_budget"], KAPPA / 2))


@pytest.mark.parametrize("name", list(util.FC_BUDGET_SCENES))
def test_entropy_float32_within_half_kappa(name):
    sc = scene(name)
    b = O.entropy_budget(sc["sdf"], sc["res"], v_out=0.7)
    s = torch.from_numpy(sc["sdf"]).requires_grad_(True)
    e = O.entropy(s, sc["res"])
    (e * float(np.float32(0.7))).backward()
    _rec("entropy", util.assert_within_budget(f"{name} entropy", [e.item()], [b["entropy"]], [b["entropy_budget"]], KAPPA / 2))
    assert not s.grad.numpy()[b["g_sdf_n"] == 0].any()
    _rec("entropy g_sdf", util.assert_within_budget(f"{name} entropy g_sdf", s.grad.numpy(), b["g_sdf"], b["g_sdf_budget"], KAPPA / 2))


def test_scene_set_coverage():
    raw, resolved, nvd = set(), set(), set()
    comp, kept, outside = set(), set(), set()
    for name in util.FC_BUDGET_SCENES:
        aux = scene_topology(name)
        raw |= set(aux["raw"][aux["surf_cubes"]].tolist()); resolved |= set(aux["case"].tolist()); nvd |= set(aux["num_vd"].tolist())
        a = aux["ambiguous"]
        comp |= set(a["raw"][a["complemented"]].tolist())
        kept |= set(a["raw"][a["inside"] & ~a["complemented"]].tolist())
        outside |= {tuple(d) for d in a["axis_dir"][~a["inside"]].tolist()}
    amb = {c for c in range(256) if O.check_entry(c) is not None}
    assert len(amb) == 36
    assert raw == set(range(1, 255)) and resolved == set(range(1, 255)) and nvd == {1, 2, 3, 4}
    assert comp == amb and kept == amb, (len(comp), len(kept))
    assert len(outside) == 6
    at = scene_topology("atlas")
    assert (len(at["surf_cubes"]), at["Q"], at["num_quads"], at["K"]) == (2036, 2824, 2716, 11728)
    assert len(set(at["raw"][at["surf_cubes"]].tolist())) == 254 and len(set(at["case"].tolist())) == 254
    # more than one scan block, the last one partial, for the cubes and for the edge slots
    for name in ("atlas", "rand_a0", "rand_b0"):
        r = scene(name)["res"]
        C, slots = r[0] * r[1] * r[2], 3 * (r[0] + 1) * (r[1] + 1) * (r[2] + 1)
        assert C > util.FC_SCAN_BLOCK and slots > util.FC_SCAN_BLOCK and slots % util.FC_SCAN_BLOCK
        assert C % util.FC_SCAN_BLOCK or name == "atlas"                  # atlas: two full blocks of cubes
    assert scene_topology("one_cube")["num_quads"] == 0 and scene_topology("one_quad")["num_quads"] == 1
    th = scene_topology("thin")
    assert th["num_quads"] > 0 and set((np.nonzero(th["quad_id"] >= 0)[0] % 3).tolist()) == {1}
    # exact zeros: both signs of zero at ends of crossing edges, as first and as second vertex, and on an interior edge (the pinned
    # reversed quad: flip is `sdf > 0`, so a zero first vertex counts as not flipped)
    z, sz = scene_topology("zeros"), scene("zeros")["sdf"]
    fz, sec = sz[z["cross_first"]], sz[z["cross_second"]]
    for arr in (fz, sec):
        assert ((arr == 0) & ~np.signbit(arr)).any() and ((arr == 0) & np.signbit(arr)).any()
    slot_first = np.nonzero(z["quad_id"] >= 0)[0] // 3
    assert (sz[slot_first] == 0).any()
    # decades: interpolation weights within 1e-4 of 0 and of 1
    dsc, dz = scene("decades"), scene_topology("decades")
    sa, sb = dsc["sdf"][dz["cross_first"]].astype(np.float64), dsc["sdf"][dz["cross_second"]].astype(np.float64)
    wgt = sa / (sa - sb)
    assert (wgt < 1e-4).any() and (wgt > 1 - 1e-4).any()
    sat = scene("saturated")
    assert (np.abs(sat["beta"]) == 8).any() and (sat["gamma"] == 100).any() and (sat["gamma"] == -100).any()
    assert float(np.tanh(np.float32(8.0))) < 1.0 and not np.isfinite(np.exp(np.float32(100.0)))


def test_one_quad_by_hand():
    """2 x 2 x 2 with one inside vertex on the boundary: the only interior crossing edge is (0,1,1)-(1,1,1); its four cubes each own
    one dual vertex; the first vertex of the edge is inside (sdf < 0), so the quad is not flipped and winds (2, 3, 1, 0)"""
    aux = scene_topology("one_quad")
    assert aux["Q"] == 4 and aux["num_quads"] == 1 and aux["num_flipped"] == 0
    assert sorted(aux["surf_cubes"].tolist()) == [0, 2, 4, 6]
    assert aux["quad_vd"].tolist() == [[2, 3, 1, 0]]
    sc = scene("one_quad")
    b = O.extract_budget(sc["vertices"], sc["sdf"], sc["res"], v_vertices=np.ones((5, 3), np.float32))
    assert b["faces"].tolist() == [[2, 3, 4], [3, 1, 4], [1, 0, 4], [0, 2, 4]]
    assert np.allclose(b["out_vertices"][4], b["out_vertices"][:4].mean(0))


# ---- the hand-off: the meshes the oracle extracts from the scenes, through vertex_normals and mesh_to_splats
@functools.lru_cache(maxsize=None)
def handoff_mesh(name):
    """(vertices float32 [V, 3], faces int64 [F, 3]) the float64 oracle extracts from the scene with all three weights"""
    sc = scene(name)
    d = lambda a: torch.from_numpy(a.astype(np.float64))
    v, f, _ = O.extract(d(sc["vertices"]), d(sc["sdf"]), sc["res"], d(sc["alpha"]), d(sc["beta"]), d(sc["gamma"]))
    return np.ascontiguousarray(v.numpy().astype(np.float32)), f.numpy()


def handoff_cotangents(name, F, V):
    r = np.random.RandomState(len(name))
    return [r.standard_normal((6 * F, w)).astype(np.float32) for w in (3, 3, 4, 3)], r.standard_normal((V, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def handoff_normals_budget(name):
    v, f = handoff_mesh(name)
    return mesh_ref.vertex_normals_budget(v, f, handoff_cotangents(name, f.shape[0], v.shape[0])[1])


def neighbour_valence(faces, V):
    e = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    e = np.unique(np.sort(e, 1), axis=0)
    return np.bincount(e.reshape(-1), minlength=V)


@pytest.mark.parametrize("name", util.FC_HANDOFF_SCENES)
def test_handoff_float32_restatement_within_half_kappa(name):
    v, f = handoff_mesh(name)
    cot, a = handoff_cotangents(name, f.shape[0], v.shape[0])
    b = handoff_normals_budget(name)
    live = ~b["isolated"]
    vt, ft = torch.from_numpy(v).requires_grad_(True), torch.from_numpy(f)
    n32 = mesh_ref.vertex_normals(vt, ft)
    (n32[torch.from_numpy(live)] * torch.from_numpy(a)[torch.from_numpy(live)]).sum().backward()
    _rec("vnormals", util.assert_within_budget(f"{name} vnormals", n32.detach().numpy()[live], b["vnormals"][live], b["vnormals_budget"][live], MESH_KAPPA / 2))
    assert not vt.grad.numpy()[b["g_vertices_n"] == 0].any()
    _rec("vnormals g_vertices", util.assert_within_budget(f"{name} vnormals g_vertices", vt.grad.numpy(), b["g_vertices"], b["g_vertices_budget"], MESH_KAPPA / 2))
    vn = b["vnormals"].astype(np.float32)
    mb = mesh_ref.mesh_to_splats_budget(v, f, vn, cot)
    vt, nt = torch.from_numpy(v).requires_grad_(True), torch.from_numpy(vn).requires_grad_(True)
    m, s, q, _, nn = mesh_ref.mesh_to_splats(vt, ft, nt, masked_sqrt=True)
    sg = torch.sign((q.detach().double() * torch.from_numpy(mb["quats"])).sum(-1, keepdim=True)).float()
    tc = [torch.from_numpy(c) for c in cot]
    ((m * tc[0]).sum() + (s * tc[1]).sum() + (q * sg * tc[2]).sum() + (nn * tc[3]).sum()).backward()
    for k, got in (("means", m), ("scales", s), ("quats", q * sg), ("normals", nn)):
        _rec("splats " + k, util.assert_within_budget(f"{name} {k}", got.detach().numpy(), mb[k], mb[k + "_budget"], MESH_KAPPA / 2))
    for k, t in (("g_vertices", vt), ("g_vnormals", nt)):
        assert not t.grad.numpy()[mb[k + "_n"] == 0].any()
        _rec("splats " + k, util.assert_within_budget(f"{name} splats {k}", t.grad.numpy(), mb[k], mb[k + "_budget"], MESH_KAPPA / 2))


def test_handoff_coverage():
    """over the hand-off meshes: every rot2quat candidate is selected somewhere, the neighbour valence covers 3 .. 10, there are
    vertices on no face, and slivers (a face normal 100 times smaller than |e1| |e2|: its components are differences of products that cancel)"""
    cands, val, sliver = set(), set(), False
    for name in util.FC_HANDOFF_SCENES:
        v, f = handoff_mesh(name)
        b = handoff_normals_budget(name)
        mb = mesh_ref.mesh_to_splats_budget(v, f, b["vnormals"].astype(np.float32))
        cands |= set(mb["candidates"].tolist())
        val |= set(neighbour_valence(f, v.shape[0]).tolist())
        p = v.astype(np.float64)[f]
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        fn = np.cross(e1, e2)
        sliver |= bool((np.linalg.norm(fn, axis=-1) < 1e-2 * np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1)).any())
        assert np.linalg.norm(fn, axis=-1).min() > 1.05e-6                 # no face within rounding of safe_normalize's 1e-6 switch
    assert cands == {0, 1, 2, 3} and val >= set(range(3, 11)) and 0 in val and sliver
    v, f, healthy = util.mesh_degenerate()
    p = v.astype(np.float64)[f]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.abs(fn[8:10]).max() == 0) and np.array_equal(fn[10], -fn[11]) and fn[10].any()
    assert np.array_equal(v[7], v[8]) and not (f == 17).any() and not np.isin(f[~healthy], f[healthy]).any()
