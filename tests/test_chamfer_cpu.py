"""The numpy restatement of the nearest-neighbour search (tests/chamfer_ref.py) against float64 and scipy, the surface sampler and
the metric formulae of geosplatting_amd/geometry.py on CPU tensors.  No GPU.

  * fp32 against float64: |d32 - d64| <= 6 u d64 for every query, u = 2^-24.  Three differences (relative error u each), three
    squares of them (2 u from the difference, u from the product: 3 u on each square), the sum of the first two (u more), the sum with
    the third (u more): 5 u on every distance to first order, 6 u with the second-order terms, and the minimum of distances that are
    each within 6 u of their float64 values is within 6 u of the float64 minimum.  The largest seen on these inputs is printed.
  * float64 against scipy.spatial.cKDTree: 1e-12 relative on the squared distance.
"""
import numpy as np
import pytest
import torch

from geosplatting_amd import geometry
from geosplatting_amd.synthetic import icosphere
from tests import chamfer_ref as ref

U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def clouds():
    q, p = ref.cloud(3000, 1), ref.cloud(4097, 2)
    d32, i32 = ref.nearest_f32(q, p)
    d64, i64 = ref.nearest_f64(q, p)
    return q, p, d32, i32, d64, i64


def test_fp32_restatement_against_float64(clouds):
    q, p, d32, i32, d64, i64 = clouds
    err = np.abs(d32.astype(np.float64) - d64)
    worst = (err[d64 > 0] / d64[d64 > 0]).max() / U24
    print(f"worst |d32 - d64| / d64 = {worst:.2f} u; {int((i32 != i64).sum())} of {q.shape[0]} queries pick another index")
    assert (err <= 6 * U24 * d64).all()


def test_ties_are_in_the_inputs(clouds):
    q, p, d32, i32, _, _ = clouds
    d = ((q[:, None, :].astype(np.float32) - p[None, :, :]) ** 2)
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    tied = ((d == d32[:, None]).sum(1) > 1).sum()
    print(f"{int(tied)} of {q.shape[0]} queries have more than one point at the smallest distance")
    assert tied >= 50
    assert (i32 == np.argmax(d == d32[:, None], axis=1)).all()          # the lowest index among them


def test_float64_restatement_against_ckdtree(clouds):
    from scipy.spatial import cKDTree
    q, p, _, _, d64, _ = clouds
    dist, _ = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=1)
    err = np.abs(dist ** 2 - d64)
    print(f"worst relative difference {(err[d64 > 0] / d64[d64 > 0]).max():.3g}; {int((d64 == 0).sum())} zero distances")
    assert (err <= 1e-12 * d64).all()                                       # every query; a zero distance must be zero there too


def test_restatement_rules_on_small_sets():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0], [1, 0, 0]], np.float32)
    q = np.array([[0.9, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [0.5, 0, 0]], np.float32)
    d, i = ref.nearest_f32(q, p)
    assert i.tolist() == [2, -1, -1, 0] and d[1] == np.inf and d[2] == np.inf
    dk, ik = ref.k_nearest_f32(q, p, 4)
    assert ik[0].tolist() == [2, 4, 0, -1] and dk[0, 3] == np.inf and ik[1].tolist() == [-1] * 4
    d, i = ref.nearest_f32(q, p[[1, 3]])
    assert (i == -1).all() and np.isinf(d).all()


# ---- sample_mesh_surface -------------------------------------------------------------------------------------------------------
def _barycentrics(pos, v, f, face_of):
    tri = v[f[face_of]].double()
    e0, e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pos.double() - tri[:, 0]
    d00, d01, d11 = (e0 * e0).sum(-1), (e0 * e1).sum(-1), (e1 * e1).sum(-1)
    d20, d21 = (e2 * e0).sum(-1), (e2 * e1).sum(-1)
    den = d00 * d11 - d01 * d01
    b1, b2 = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    n = torch.cross(e0, e1, dim=-1)
    off = (e2 * n).sum(-1) / n.norm(dim=-1)
    return torch.stack([1 - b1 - b2, b1, b2], -1), off


@pytest.mark.parametrize("in_face", ["random", "r2"])
def test_uniform_counts_and_samples_in_their_triangles(in_face):
    v, f = icosphere(2)
    v = v * torch.tensor([1.0, 0.6, 1.7])                                   # unequal areas
    S = 5003
    g = torch.Generator().manual_seed(3)
    pos, nrm = geometry.sample_mesh_surface(v, f, S, samples_per_face="uniform", samples_in_face=in_face, generator=g)
    assert pos.shape == (S, 3) and nrm.shape == (S, 3)
    c = v[f]
    area = torch.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], dim=-1).norm(dim=-1)
    floor_counts = (area / area.sum() * S).floor().long()
    # the first sum(floor) samples are laid out face by face; the remainder follows: recover every sample's face from the positions
    first = int(floor_counts.sum())
    face_of = torch.arange(f.shape[0]).repeat_interleave(floor_counts)
    bary, off = _barycentrics(pos[:first], v, f, face_of)
    assert (bary >= -1e-6).all() and ((bary.sum(-1) - 1).abs() <= 1e-6).all() and (off.abs() <= 1e-6).all()
    assert torch.allclose(nrm.norm(dim=-1), torch.ones(S), atol=1e-6)
    # the remainder: every sample lies in SOME triangle, and the counts sum to S with every face at its floor or above
    rest = pos[first:]
    best = torch.full((rest.shape[0],), -1, dtype=torch.long)
    for face in range(f.shape[0]):
        b, o = _barycentrics(rest, v, f, torch.full((rest.shape[0],), face))
        inside = (b >= -1e-6).all(-1) & (o.abs() <= 1e-6)
        best = torch.where((best < 0) & inside, torch.full_like(best, face), best)
    assert (best >= 0).all()
    counts = floor_counts + torch.bincount(best, minlength=f.shape[0])
    assert int(counts.sum()) == S and (counts >= floor_counts).all()


def test_r2_is_deterministic_and_random_follows_the_generator():
    v, f = icosphere(1)
    kw = dict(samples_per_face="uniform", probs_per_face="uniform")
    g = lambda s: torch.Generator().manual_seed(s)
    S = f.shape[0] * 7                                                      # fp32 p S is the integer 7: no remainder, no draw at all
    a = geometry.sample_mesh_surface(v, f, S, samples_in_face="r2", generator=g(1), **kw)[0]
    b = geometry.sample_mesh_surface(v, f, S, samples_in_face="r2", generator=g(2), **kw)[0]
    assert torch.equal(a, b)
    a = geometry.sample_mesh_surface(v, f, 1000, generator=g(5))[0]
    b = geometry.sample_mesh_surface(v, f, 1000, generator=g(5))[0]
    c = geometry.sample_mesh_surface(v, f, 1000, generator=g(6))[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    state = torch.get_rng_state()
    geometry.sample_mesh_surface(v, f, 1000, generator=g(5))
    assert torch.equal(state, torch.get_rng_state())                        # the global generator is left alone


def test_uniform_nonzero_raises_where_the_reference_does():
    v, f = icosphere(1)
    F = f.shape[0]
    # the reference raises when some floor(p S) is 0 and names ceil(1 / min p) as the count that is needed: 80 faces, p = 1 / 80
    with pytest.raises(RuntimeError, match=f"num_samples = {F - 1} .* at least {F} samples"):
        geometry.sample_mesh_surface(v, f, F - 1, samples_per_face="uniform+nonzero", probs_per_face="uniform")
    pos, _ = geometry.sample_mesh_surface(v, f, 4 * F, samples_per_face="uniform+nonzero", probs_per_face="uniform")
    assert pos.shape == (4 * F, 3)
    with pytest.raises(ValueError):
        geometry.sample_mesh_surface(v, f, 10, samples_per_face="random", probs_per_face="uniform")
    with pytest.raises(ValueError):
        geometry.sample_mesh_surface(v, f, 10, samples_per_face="stratified")
    with pytest.raises(ValueError):
        geometry.sample_mesh_surface(v, f, 10, samples_in_face="halton")


def test_gradient_to_vertices_equals_the_weights():
    v, f = icosphere(1)
    v = v.clone().requires_grad_(True)
    S = f.shape[0] * 3
    kw = dict(samples_per_face="uniform", probs_per_face="uniform", samples_in_face="r2")
    pos, _ = geometry.sample_mesh_surface(v, f, S, **kw)
    cot = torch.randn(S, 3, generator=torch.Generator().manual_seed(0))
    (pos * cot).sum().backward()
    # the weights, from the positions of a detached call: every face holds 3 consecutive samples
    with torch.no_grad():
        face_of = torch.arange(f.shape[0]).repeat_interleave(3)
        bary, off = _barycentrics(pos.detach(), v.detach(), f, face_of)
        assert off.abs().max() <= 1e-6 and (bary >= -1e-6).all()
        want = torch.zeros_like(v, dtype=torch.float64)
        for corner in range(3):
            want.index_add_(0, f[face_of, corner], bary[:, corner, None] * cot.double())
    assert torch.allclose(v.grad.double(), want, atol=1e-5)


# ---- metric formulae -----------------------------------------------------------------------------------------------------------
def test_fscore_formulae_on_hand_made_distances():
    dab = torch.tensor([0.0, 0.0005, 0.001, 0.002])                        # 2 of 4 strictly below 0.001
    dba = torch.tensor([0.0009, 0.5])                                       # 1 of 2
    ch, fs = geometry.fscore_from_distances(dab, dba, 0.001)
    assert float(ch) == pytest.approx(0.0035 / 4 + 0.5009 / 2, rel=1e-6)
    assert float(fs) == pytest.approx(2 * 0.5 * 0.5 / 1.0, rel=1e-6)
    ch_ref, fs_ref = ref.fscore(dab.numpy(), dba.numpy(), 0.001)
    assert float(ch) == pytest.approx(ch_ref, rel=1e-6) and float(fs) == pytest.approx(fs_ref, rel=1e-6)
    # nothing below the threshold: 0 / clamp(0, 1e-10) = 0, not NaN
    ch, fs = geometry.fscore_from_distances(dab + 1, dba + 1, 0.001)
    assert float(fs) == 0.0 and np.isfinite(float(ch))
    # everything below: 1
    _, fs = geometry.fscore_from_distances(dab, dba, 10.0)
    assert float(fs) == 1.0


def test_cpu_tensors_and_empty_sets_are_refused():
    from geosplatting_amd._lib import GeoSplatHipError
    with pytest.raises(ValueError, match="empty"):
        geometry.PointGrid(torch.zeros(0, 3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        geometry.PointGrid(torch.zeros(4, 3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        geometry.chamfer_distance(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        geometry.k_nearest(torch.zeros(4, 3), 2)
