"""The mesh-prior regularisers on the GPU (csrc/gs_meshreg.hip through geosplatting_amd/meshreg.py) against the float64 restatement
of tests/meshreg_ref.py: per-item terms, the three means and the per-vertex gradients of each mean within the budgets stated there,
on the smallest shapes that reach each code path (more than one workgroup with a partial last one, an open boundary, a non-manifold
edge, an unused vertex, lists above 64 and above 128 entries that a wave walks, P = 0, F = 0)."""
import pytest
import torch

from tests import meshreg_ref as R

pytestmark = pytest.mark.gpu

TINY = 1e-30


def _run(name, target=0.0, vertices=None):
    """-> (values, terms, grads of each mean, ref) of a case on the GPU"""
    import geosplatting_amd as gs
    v32, f, topo = R.case(name)
    v32 = v32 if vertices is None else vertices
    dev = torch.device("cuda:0")
    t = gs.MeshRegTopology(f.to(dev), v32.shape[0])
    v = v32.to(dev).requires_grad_(True)
    lap, edge, nc, tl, te, tp = gs.mesh_regularizers(v, t, target, return_terms=True)
    grads = []
    for val in (lap, edge, nc):
        g, = torch.autograd.grad(val, v, retain_graph=True)
        grads.append(g.cpu().double())
    return ([x.detach().cpu().double() for x in (lap, edge, nc)], [x.detach().cpu().double() for x in (tl, te, tp)], grads,
            R.evaluate(v32, topo, target))


def _check(values, terms, grads, ref, what):
    for k, key in enumerate(("lap", "edge", "nc")):
        assert values[k].ndim == 0 and terms[k].shape == ref[key + "_terms"].shape, (what, key)
        err, bud = (terms[k] - ref[key + "_terms"]).abs(), ref[key + "_terms_budget"]
        ratio = float((err / (bud + TINY)).max()) if err.numel() else 0.0
        print(f"{what} {key}: terms worst error / budget {ratio:.3g}", end="; ")
        assert bool((err <= bud).all()), (what, key, "terms", ratio)
        err, bud = float((values[k] - ref[key]).abs()), float(ref[key + "_budget"])
        print(f"value {float(values[k]):.6g} error {err:.3g} budget {bud:.3g}", end="; ")
        assert err <= bud, (what, key, "value")
        err, bud = (grads[k] - ref["grad_" + key]).abs(), ref["grad_" + key + "_budget"]
        ratio = float((err / (bud + TINY)).max()) if err.numel() else 0.0
        print(f"gradient worst error / budget {ratio:.3g}")
        assert bool(torch.isfinite(grads[k]).all()) and bool((err <= bud).all()), (what, key, "gradient", ratio)


@pytest.mark.parametrize("name", R.CASES)
def test_terms_values_and_gradients_within_budget(name):
    values, terms, grads, ref = _run(name)
    _check(values, terms, grads, ref, name)
    if name == "one_triangle":
        assert terms[2].numel() == 0 and float(values[2]) == 0.0 and not bool(grads[2].any())
    if name == "no_faces":
        assert all(float(x) == 0.0 for x in values) and not any(bool(g.any()) for g in grads)
    if name == "unused_vertex":
        assert float(terms[0][-1]) == 0.0 and not any(bool(g[-1].any()) for g in grads)


@pytest.mark.parametrize("name", ["icosphere2", "fan200", "three_faces"])
def test_target_length(name):
    values, terms, grads, ref = _run(name, target=0.07)
    _check(values, terms, grads, ref, name + " target 0.07")
    assert float(values[1]) != float(_run(name)[0][1])


def test_zero_area_face_is_finite():
    """two coincident vertices: a zero-length edge, zero-area faces, zero normals under the clamp.  Finite values and gradients, and the
    zero subgradient where a norm's argument is zero (the restatement agrees with float64 autograd on this, tests/test_meshreg_cpu.py)"""
    v32, f, topo = R.case("icosphere2")
    v32 = v32.clone()
    e = topo["edges"][17]
    v32[e[1]] = v32[e[0]]
    values, terms, grads, ref = _run("icosphere2", vertices=v32)
    assert all(bool(torch.isfinite(x).all()) for x in values + terms + grads)
    _check(values, terms, grads, ref, "coincident vertices")


def test_single_term_forms_and_weighted_gradient():
    import geosplatting_amd as gs
    from geosplatting_amd import meshreg
    v32, f, topo = R.case("icosphere2")
    dev = torch.device("cuda:0")
    t = gs.MeshRegTopology(f.to(dev), v32.shape[0])
    v = v32.to(dev).requires_grad_(True)
    lap, edge, nc = gs.mesh_regularizers(v, t, 0.05)
    assert lap.dtype == torch.float32 and lap.ndim == 0
    assert torch.equal(meshreg.laplacian_smooth_loss(v, t), lap) and torch.equal(meshreg.mesh_edge_loss(v, t, 0.05), edge)
    assert torch.equal(meshreg.mesh_normal_consistency(v, t), nc)
    # one backward of a weighted sum: the three gradients added with their weights
    w = (1e-3, 0.1, 3e-4)
    (w[0] * lap + w[1] * edge + w[2] * nc).backward()
    ref = R.evaluate(v32, topo, 0.05)
    want = sum(wk * ref["grad_" + k] for wk, k in zip(w, ("lap", "edge", "nc")))
    bud = sum(wk * ref["grad_" + k + "_budget"] for wk, k in zip(w, ("lap", "edge", "nc")))
    assert bool(((v.grad.cpu().double() - want).abs() <= bud * (1 + 1e-3)).all())
    with pytest.raises(ValueError):
        gs.mesh_regularizers(v[:-1], t)
    with pytest.raises(ValueError):
        gs.mesh_regularizers(v.double(), t)


@pytest.mark.parametrize("name", ["icosphere3", "fan200"])
def test_two_runs_give_equal_bits(name):
    import geosplatting_amd as gs
    v32, f, _ = R.case(name)
    dev = torch.device("cuda:0")
    t = gs.MeshRegTopology(f.to(dev), v32.shape[0])
    runs = []
    for _ in range(2):
        v = v32.to(dev).requires_grad_(True)
        out = gs.mesh_regularizers(v, t, 0.01, return_terms=True)
        (out[0] * 0.3 + out[1] * 1.7 + out[2] * 0.9).backward()
        runs.append([x.detach().clone() for x in out] + [v.grad.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_value_errors():
    import geosplatting_amd as gs
    dev = torch.device("cuda:0")
    with pytest.raises(ValueError, match="repeats"):
        gs.MeshRegTopology(torch.tensor([[0, 1, 2], [2, 4, 2]], device=dev), 5)
    with pytest.raises(ValueError, match="outside"):
        gs.MeshRegTopology(torch.tensor([[0, 1, 5]], device=dev), 5)


def test_adam_on_the_regularisers_lowers_each_term():
    """50 Adam steps on the three regularisers alone, on a jittered sphere: every term ends below where it began"""
    import geosplatting_amd as gs
    v32, f, _ = R.case("icosphere2")
    dev = torch.device("cuda:0")
    t = gs.MeshRegTopology(f.to(dev), v32.shape[0])
    v = v32.to(dev).requires_grad_(True)
    opt = torch.optim.Adam([v], lr=2e-3)
    first = last = None
    for _ in range(50):
        opt.zero_grad()
        lap, edge, nc = gs.mesh_regularizers(v, t)
        last = (float(lap), float(edge), float(nc))
        first = first or last
        (lap + edge + nc).backward()
        opt.step()
    print("first", first, "last", last)
    assert all(b < a for a, b in zip(first, last))
