"""No-GPU checks of the float64 restatement of the mesh-prior regularisers (tests/meshreg_ref.py) -- the yardstick of
tests/test_gpu_meshreg.py -- against float64 autograd of the literal formulas (a sparse `L @ v`, `torch.cosine_similarity`, `norm`), and
of the topology `MeshRegTopology` builds (torch ops: they run on the CPU too) against the restatement's own."""
import numpy as np
import pytest
import torch

from geosplatting_amd.meshreg import MeshRegTopology
from geosplatting_amd.synthetic import icosphere
from tests import meshreg_ref as R


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("target", [0.0, 0.07])
def test_restatement_matches_autograd_of_the_literal_formulas(name, target):
    v32, f, topo = R.case(name)
    ref = R.evaluate(v32, topo, target)
    v = v32.double().requires_grad_(True)
    values = R.literal(v, f, topo, target)
    for key, val in zip(("lap", "edge", "nc"), values):
        assert abs(float(val) - float(ref[key])) <= 1e-12 * (1 + abs(float(val))), key
        grad, = torch.autograd.grad(val, v, allow_unused=True, retain_graph=True)
        grad = torch.zeros_like(v) if grad is None else grad
        scale = float(grad.abs().max()) + 1e-30
        assert float((grad - ref["grad_" + key]).abs().max()) <= 1e-10 * scale, key
        assert bool((ref["grad_" + key + "_budget"] >= 0).all()) and bool((ref[key + "_terms_budget"] >= 0).all())
        # a budget is a sum of absolute values of terms that add up to the element: never below the element itself
        assert bool((ref["grad_" + key + "_budget"] * (1 + 1e-9) >= R.KAPPA * ref["grad_" + key].abs()).all()), key


def test_zero_length_vectors_give_the_zero_subgradient():
    """two coincident vertices (a zero-area face and a zero-length edge) and a vertex at the mean of its neighbours: finite, and equal
    to autograd's, whose norm backward returns 0 at 0"""
    v32 = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 1.0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [1, 0, 4], [2, 1, 4]])
    topo = R.topology(f.numpy(), 5)
    ref = R.evaluate(v32, topo)
    v = v32.double().requires_grad_(True)
    for key, val in zip(("lap", "edge", "nc"), R.literal(v, f, topo)):
        grad, = torch.autograd.grad(val, v, retain_graph=True)
        assert bool(torch.isfinite(ref["grad_" + key]).all()) and bool(torch.isfinite(grad).all())
        assert float((grad - ref["grad_" + key]).abs().max()) <= 1e-10 * (float(grad.abs().max()) + 1e-30), key


def test_topology_counts_on_known_meshes():
    v, f = icosphere(2)
    for topo in (R.topology(f.numpy(), v.shape[0]), None):
        t = MeshRegTopology(f, v.shape[0])
        deg = t.degree.numpy() if topo is None else topo["degree"]
        E, P = (t.num_edges, t.num_pairs) if topo is None else (len(topo["edges"]), len(topo["pairs"]))
        assert v.shape[0] == 162 and E == 480 and P == 480
        assert int((deg == 5).sum()) == 12 and int((deg == 6).sum()) == 150
    # a closed manifold: V - E + F = 2
    assert 162 - 480 + f.shape[0] == 2


@pytest.mark.parametrize("name", R.CASES)
def test_topology_matches_the_restatement(name):
    v, f, topo = R.case(name)
    V = v.shape[0]
    t = MeshRegTopology(f, V)
    assert t.edges.dtype == torch.int32 and t.pairs.dtype == torch.int32
    assert np.array_equal(t.edges.numpy(), topo["edges"]) and np.array_equal(t.pairs.numpy(), topo["pairs"])
    assert np.array_equal(t.degree.numpy(), topo["degree"])
    assert bool((t.edges[:, 0] < t.edges[:, 1]).all())
    key = t.edges[:, 0].long() * V + t.edges[:, 1].long()
    assert bool((key[1:] > key[:-1]).all())
    off, nbr = t.nbr_off.tolist(), t.nbr.tolist()
    assert [nbr[off[i]:off[i + 1]] for i in range(V)] == topo["nbrs"]
    # every (pair, role) code sits in the list of the vertex it names, ascending
    poff, pr = t.pr_off.tolist(), t.pr.tolist()
    flat = t.pairs.reshape(-1).tolist()
    assert len(pr) == 4 * t.num_pairs and sorted(pr) == list(range(4 * t.num_pairs))
    for i in range(V):
        codes = pr[poff[i]:poff[i + 1]]
        assert codes == sorted(codes) and all(flat[c] == i for c in codes)
    n_codes = np.diff(np.array(poff))
    assert t.long_verts.tolist() == [i for i in range(V) if topo["degree"][i] > 64 or n_codes[i] > 64]


def test_special_topologies():
    _, f, topo = R.case("three_faces")
    t = MeshRegTopology(f, 5)
    assert t.pairs.tolist() == [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4]] and t.num_edges == 7
    _, f, _ = R.case("grid")
    t = MeshRegTopology(f, 63)
    assert t.num_pairs == t.num_edges - 2 * (8 + 6)                   # the boundary edges have no pair
    _, f, _ = R.case("unused_vertex")
    assert MeshRegTopology(f, 43).degree[-1] == 0
    _, f, _ = R.case("fan200")
    t = MeshRegTopology(f, 202)
    assert t.long_verts.tolist() == [0] and int(t.degree[0]) == 201 and int(t.pr_off[1] - t.pr_off[0]) == 199
    t = MeshRegTopology(torch.zeros(0, 3, dtype=torch.long), 5)
    assert (t.num_edges, t.num_pairs, t.num_long) == (0, 0, 0) and t.nbr_off.tolist() == [0] * 6


def test_topology_refuses_bad_faces():
    with pytest.raises(ValueError, match="repeats"):
        MeshRegTopology(torch.tensor([[0, 1, 2], [3, 3, 4]]), 5)
    with pytest.raises(ValueError, match="outside"):
        MeshRegTopology(torch.tensor([[0, 1, 5]]), 5)
    with pytest.raises(ValueError, match="outside"):
        MeshRegTopology(torch.tensor([[0, 1, -1]]), 5)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        MeshRegTopology(torch.tensor([[0, 1, 2, 3]]), 5)


def test_lap_is_zero_inside_a_flat_regular_grid():
    """every interior vertex of the regular grid triangulation has its 6 neighbours placed symmetrically: deg v - sum = 0 exactly"""
    v, f = R.grid_mesh(7, 6)
    topo = R.topology(f.numpy(), v.shape[0])
    ref = R.evaluate(v, topo)
    lap = ref["lap_terms"].reshape(6, 7)
    assert bool((lap[1:-1, 1:-1] == 0).all()) and bool((lap[0] > 0).all()) and bool((lap[:, 0] > 0).all())
    assert bool((ref["nc_terms"].abs() <= 1e-15).all())              # coplanar faces with consistent winding: cos = 1
    assert bool(torch.allclose(ref["edge_terms"].sqrt().sort().values.unique(), torch.tensor([1.0, 2 ** 0.5], dtype=torch.float64)))


def test_ops_refuse_cpu_tensors():
    from geosplatting_amd import meshreg
    from geosplatting_amd._lib import GeoSplatHipError
    v, f, _ = R.case("icosphere2")
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        meshreg.mesh_regularizers(v, MeshRegTopology(f, v.shape[0]))
