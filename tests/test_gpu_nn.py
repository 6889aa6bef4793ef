"""The nearest-neighbour search, the Chamfer pair and the geometry metrics on the GPU (csrc/gs_nn.hip, geosplatting_amd/geometry.py)
against the numpy restatement of tests/chamfer_ref.py.

Every comparison of a search result is BIT FOR BIT in d and EQUAL in idx for every query, for the grid form and for the brute-force
form (which therefore equal each other): include/geosplat_hip.h fixes the fp32 operation order of the distance, the tie rule and the
non-finite rule, so there is nothing to tolerate.  The backward is compared per element with the any-order bound derived in the
docstring of chamfer_ref.  The Chamfer value is the sum of two means that geometry.py accumulates in float64 and rounds to float32
once: against the float64 means of the restatement's (bit-equal) distances it may differ by that rounding, 2^-24 relative, plus the
float64 reduction's own n 2^-53 -- asserted within 2 * 2^-24, so that ONE wrong distance among 20 000 of this size shows.  The
F-score is a ratio of exact counts: four fp32 roundings.

Measured on an MI355X: no search result differs in any case; the backward's largest error is 0.79 of its bound on grad_xyz1 and 0.69
on grad_xyz2; the scales of knn='device' differ from the host path's by at most 1.2e-7 relative."""
import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd.gsplat3d import GaussianSet, knn_mean_distance
from geosplatting_amd.synthetic import icosphere
from tests import chamfer_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U24 = 2.0 ** -24


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


def _same(d, i, d_ref, i_ref, what):
    i = i.cpu().numpy()
    bad = np.nonzero((_bits(d) != _bits(d_ref)) | (i != i_ref))
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {i.size} differ, first at {tuple(b[0] for b in bad)}"


def _check(q, p, what, k=None):
    """grid and brute force against the restatement, for every query"""
    grid = gs.PointGrid(_t(p))
    if k is None:
        d_ref, i_ref = ref.nearest_f32(q, p)
    else:
        d_ref, i_ref = ref.k_nearest_f32(q, p, k)
    for brute in (False, True):
        d, i = grid.nearest(_t(q), brute_force=brute) if k is None else grid.k_nearest(_t(q), k, brute_force=brute)
        assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == d_ref.shape
        _same(d, i, d_ref, i_ref, f"{what}, {'brute force' if brute else 'grid'}")
    return d_ref, i_ref


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(1, 1), (513, 7), (3000, 4097), (4097, 3000), (100, 3), (67, 130)])
def test_shapes(N, M):
    # (a quarter of both sets sits on a 1/4 lattice: ties and duplicates; 3 and 7 points are below one cell's worth, 4 M < 4)
    _check(ref.cloud(N, 10 + N), ref.cloud(M, 20 + M), f"{N} x {M}")


def test_ties_are_many():
    q, p = ref.cloud(3000, 3010), ref.cloud(4097, 4117)
    d_ref, _ = ref.nearest_f32(q, p)
    assert (d_ref == 0).sum() > 20                                  # queries that coincide with set points, several of them duplicated


def test_power_of_two_lattice_puts_points_on_cell_faces():
    rng = np.random.default_rng(5)
    p = (np.round(rng.uniform(-1, 1, (4096, 3)) * 8) / 8).astype(np.float32)
    p[:8] = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)      # the box is exactly [-1, 1]^3
    q = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    q[:1000] = (np.round(q[:1000] * 16) / 16).astype(np.float32)    # on the lattice and half way between its points
    _check(q, p, "power-of-two lattice")


# ---- degenerate boxes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["identical", "plane", "line", "crowded"])
def test_degenerate_boxes(kind):
    rng = np.random.default_rng(7)
    p = rng.uniform(-1, 1, (3001, 3)).astype(np.float32)
    if kind == "identical":
        p[:] = np.float32([0.3, -0.2, 0.7])
    elif kind == "plane":
        p[:, 2] = np.float32(0.25)
    elif kind == "line":
        p[:, 1:] = np.float32([0.5, -0.125])
    else:
        p[:2700] = np.float32([0.4, 0.4, -0.6]) + rng.uniform(-1e-3, 1e-3, (2700, 3)).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, (777, 3)).astype(np.float32)
    q[:100] = p[:100]
    q[100:200] = p[100:200] + rng.uniform(-1e-3, 1e-3, (100, 3)).astype(np.float32)
    _check(q, p, kind)


# ---- far queries ---------------------------------------------------------------------------------------------------------------
def test_far_queries():
    p = ref.cloud(3000, 31)
    rng = np.random.default_rng(8)
    ext = p.max(0) - p.min(0)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1]], np.float32)
    q = (dirs[np.arange(64) % 7] * 10 * ext + rng.uniform(-1, 1, (64, 3))).astype(np.float32)
    q[-1] = np.float32([1e30, -1e30, 1e30])                          # however far
    q[-2] = np.float32([3e38, 3e38, -3e38])                          # every d overflows: (+inf, lowest index)
    d_ref, i_ref = _check(q, p, "far queries")
    assert i_ref[-2] == 0 and np.isinf(d_ref[-2])


# ---- non-finite rows -----------------------------------------------------------------------------------------------------------
def test_non_finite_rows():
    p, q = ref.cloud(1500, 41), ref.cloud(700, 42)
    for arr, step in ((p, 7), (q, 5)):
        arr[0::step * 3, 0] = np.nan
        arr[1::step * 3, 1] = np.inf
        arr[2::step * 3, 2] = -np.inf
    q[3] = p[0]
    d_ref, i_ref = _check(q, p, "non-finite rows")
    bad_q, bad_p = ~np.isfinite(q).all(-1), ~np.isfinite(p).all(-1)
    assert bad_q.sum() > 100 and bad_p.sum() > 200
    assert (i_ref[bad_q] == -1).all() and np.isinf(d_ref[bad_q]).all() and not bad_p[i_ref[~bad_q]].any()
    d_ref, i_ref = _check(q, p[bad_p], "a set without a finite point")
    assert (i_ref == -1).all()
    _check(q, p, "non-finite rows, k = 3", k=3)


# ---- k nearest -----------------------------------------------------------------------------------------------------------------
def _dup_cloud():
    p = ref.cloud(2000, 51)
    p[1000:1200] = p[:200]                                           # exact duplicates besides the lattice ones
    p[1200:1250] = p[:50]
    return p


@pytest.mark.parametrize("k", [1, 3, 8])
def test_k_nearest(k):
    p = _dup_cloud()
    _check(p, p, f"k = {k} in the set itself", k=k)
    _check(ref.cloud(501, 52), p, f"k = {k}", k=k)


def test_k_nearest_padding_and_range():
    p, q = ref.cloud(5, 53), ref.cloud(70, 54)
    d_ref, i_ref = _check(q, p, "M < k", k=8)
    assert (i_ref[:, 5:] == -1).all() and np.isinf(d_ref[:, 5:]).all() and (i_ref[:, :5] >= 0).all()
    grid = gs.PointGrid(_t(p))
    for k in (0, 9):
        with pytest.raises(ValueError):
            grid.k_nearest(_t(q), k)
    with pytest.raises(ValueError, match="empty"):
        gs.PointGrid(torch.zeros(0, 3, device=DEV))
    d, i = grid.nearest(torch.zeros(0, 3, device=DEV))
    assert d.shape == (0,) and i.shape == (0,)


def test_k_nearest_returns_distances():
    p = _dup_cloud()
    d_ref, i_ref = ref.k_nearest_f32(p, p, 4)
    d, i = gs.k_nearest(_t(p), 3)
    _same(d, i, np.sqrt(d_ref[:, 1:]), i_ref[:, 1:], "k_nearest(points, 3)")
    q = ref.cloud(300, 55)
    d_ref, i_ref = ref.k_nearest_f32(q, p, 2)
    d, i = gs.k_nearest_in(_t(q), _t(p), 2)
    _same(d, i, np.sqrt(d_ref), i_ref, "k_nearest_in(points, queries, 2)")


# ---- rebuild -------------------------------------------------------------------------------------------------------------------
def test_rebuild_equals_a_fresh_grid():
    p0, q = ref.cloud(3000, 61), ref.cloud(1000, 62)
    p1 = (p0 * np.float32(3.0) + np.float32([5.0, -2.0, 0.5])).astype(np.float32)[::-1].copy()
    grid = gs.PointGrid(_t(p0))
    buffers = (grid.grid.data_ptr(), grid._ws.data_ptr())
    grid.rebuild(_t(p1))
    assert (grid.grid.data_ptr(), grid._ws.data_ptr()) == buffers
    fresh = gs.PointGrid(_t(p1))
    qt = _t(q * np.float32(3.0) + np.float32([5.0, -2.0, 0.5]))
    d, i = grid.nearest(qt)
    d2, i2 = fresh.nearest(qt)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(i, i2)
    d_ref, i_ref = ref.nearest_f32(qt.cpu().numpy(), p1)
    _same(d, i, d_ref, i_ref, "rebuilt grid")
    with pytest.raises(ValueError):
        grid.rebuild(_t(p1[:-1]))


# ---- chamfer_distance ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chamfer_case():
    a, b = ref.cloud(1201, 71), ref.cloud(997, 72)
    a[5] = np.nan                                                    # paired with -1 in dist1, never chosen in dist2
    b[:40] = a[100:140]                                              # many rows of a share a neighbour
    b[7, 1] = np.inf
    a[200:260] = a[100]                                              # ... and sixty of them are one point: sixty atomics on one row
    d1, i1 = ref.nearest_f32(a, b)
    d2, i2 = ref.nearest_f32(b, a)
    rng = np.random.default_rng(73)
    g1, g2 = rng.standard_normal(a.shape[0]).astype(np.float32), rng.standard_normal(b.shape[0]).astype(np.float32)
    return a, b, d1, i1, d2, i2, g1, g2


@pytest.mark.parametrize("batched", [False, True])
def test_chamfer_distance_forward_and_backward(chamfer_case, batched):
    a, b, d1, i1, d2, i2, g1, g2 = chamfer_case
    ta, tb = _t(a).requires_grad_(True), _t(b).requires_grad_(True)
    xa, xb = (ta[None], tb[None]) if batched else (ta, tb)
    dist1, dist2, idx1, idx2 = gs.chamfer_distance(xa, xb, return_indices=True)
    assert dist1.shape == ((1, a.shape[0]) if batched else (a.shape[0],)) and dist1.requires_grad and not idx1.requires_grad
    _same(dist1.reshape(-1), idx1.reshape(-1), d1, i1, "dist1")
    _same(dist2.reshape(-1), idx2.reshape(-1), d2, i2, "dist2")
    assert i1[5] == -1 and i2[7] == -1 and (i2 != 5).all() and (i1 != 7).all()
    torch.autograd.backward([dist1, dist2], [_t(g1).reshape(dist1.shape), _t(g2).reshape(dist2.shape)])
    ga, ba, gb, bb = ref.chamfer_bwd_budget(np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0),
                                            np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0), i1, i2, g1, g2)
    for name, got, want, bound in (("grad_xyz1", ta.grad, ga, ba), ("grad_xyz2", tb.grad, gb, bb)):
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        used = (err[bound > 0] / bound[bound > 0]).max()
        print(f"{name}: largest error {used:.3f} of its bound")
        assert (err <= bound).all(), f"{name}: {(err > bound).sum()} elements over their bound, worst {used:.3f}"
    assert (ta.grad[5] == 0).all() and (tb.grad[7] == 0).all()      # rows paired with -1


def test_chamfer_distance_refuses_bad_shapes():
    a = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError):
        gs.chamfer_distance(a, a[None])
    with pytest.raises(ValueError):
        gs.chamfer_distance(a[None], torch.zeros(2, 4, 3, device=DEV))
    with pytest.raises(ValueError, match="empty"):
        gs.chamfer_distance(a, a[:0])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_translated_copy_of_a_point_set():
    rng = np.random.default_rng(81)
    cells = rng.choice(129 ** 3, 4000, replace=False)                # distinct points of the 2^-6 lattice in [-1, 1]^3
    p = (np.stack([cells // (129 * 129), (cells // 129) % 129, cells % 129], -1) / 64.0 - 1.0).astype(np.float32)
    t = np.float32([2.0 ** -9, -2.0 ** -10, 2.0 ** -11])            # |t| < 2^-7 = half the spacing; p + t is exact in fp32
    moved = p + t
    assert np.array_equal(moved.astype(np.float64), p.astype(np.float64) + t.astype(np.float64))
    tt = np.float32(np.float32(t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    d_ab, d_ba, i_ab, i_ba = gs.chamfer_distance(_t(p), _t(moved), return_indices=True)
    assert (_bits(d_ab) == _bits(tt)).all() and (_bits(d_ba) == _bits(tt)).all()
    assert torch.equal(i_ab.cpu(), torch.arange(4000, dtype=torch.int32)) and torch.equal(i_ba, i_ab)
    ch, fs = gs.chamfer_fscore(_t(p), _t(moved), threshold=float(tt) * 1.5)
    assert float(fs) == 1.0 and float(ch) == pytest.approx(2 * float(tt), rel=2 * U24)
    for thr in (float(tt), float(tt) * 0.5):                         # strictly below the threshold counts
        assert float(gs.chamfer_fscore(_t(p), _t(moved), threshold=thr)[1]) == 0.0
    assert float(gs.chamfer(_t(p), _t(moved))) == float(ch)


def test_chamfer_fscore_on_meshes():
    v, f = icosphere(3)
    v, f = v.to(DEV), f.to(DEV)
    S, thr = 20000, 2e-4

    def metric(seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        ch, fs = gs.chamfer_fscore((v, f), (v * 1.01, f), threshold=thr, target_num_points=S, generator=g)
        return float(ch), float(fs)

    got = metric(7)
    g = torch.Generator(device=DEV).manual_seed(7)                   # the same samples: a first, then b, from one generator
    pa = gs.sample_mesh_surface(v, f, S, samples_per_face="uniform", generator=g)[0]
    pb = gs.sample_mesh_surface(v * 1.01, f, S, samples_per_face="uniform", generator=g)[0]
    assert pa.shape == (S, 3)
    d_ab, _ = ref.nearest_f32(pa.cpu().numpy(), pb.cpu().numpy())
    d_ba, _ = ref.nearest_f32(pb.cpu().numpy(), pa.cpu().numpy())
    ch_ref, fs_ref = ref.fscore(d_ab, d_ba, np.float32(thr))
    print(f"chamfer {got[0]:.9g} (float64 mean of the restatement {ch_ref:.9g}), fscore {got[1]:.9g} ({fs_ref:.9g})")
    assert 0.05 < fs_ref < 0.95                                      # the threshold cuts through the distances
    assert abs(got[0] - ch_ref) <= 2 * U24 * ch_ref and abs(got[1] - fs_ref) <= 4 * U24 * fs_ref
    assert metric(7) == got and metric(8) != got
    # the default sample count: max(10 F, 100 000)
    ch, fs = gs.chamfer_fscore((v, f), (v * 1.01, f), generator=torch.Generator(device=DEV).manual_seed(1))
    assert float(fs) > 0.99 and 1e-4 < float(ch) < 6e-4


def test_chamfer_distance_is_a_mesh_loss():
    """gradients reach the vertices through the samples"""
    v, f = icosphere(2)
    v, f = v.to(DEV).requires_grad_(True), f.to(DEV)
    target = ref.cloud(3000, 91)
    target = _t(target / np.linalg.norm(target, axis=-1, keepdims=True).astype(np.float32) * np.float32(1.1))
    g = torch.Generator(device=DEV).manual_seed(2)
    pos, _ = gs.sample_mesh_surface(v, f, 5000, samples_per_face="uniform", generator=g)
    d1, d2 = gs.chamfer_distance(pos, target)
    (d1.mean() + d2.mean()).backward()
    assert torch.isfinite(v.grad).all() and (v.grad * v.detach()).sum() < 0        # growing the sphere lowers the loss


# ---- GaussianSet.from_points ---------------------------------------------------------------------------------------------------
def test_from_points_knn():
    gen = torch.Generator().manual_seed(3)
    pts, col = torch.rand(5000, 3, generator=gen) * 2 - 1, torch.rand(5000, 3, generator=gen)
    parent = knn_mean_distance(pts, 3)[:, None].log().repeat(1, 3)   # what the constructor computed before it had the option
    host = GaussianSet.from_points(pts, col, sh_degree=0, device=DEV, generator=torch.Generator().manual_seed(4))
    assert torch.equal(host.scales.cpu(), parent)
    dev = GaussianSet.from_points(pts, col, sh_degree=0, device=DEV, generator=torch.Generator().manual_seed(4), knn="device")
    rel = ((dev.scales - host.scales).abs() / host.scales.abs()).max()
    print(f"knn='device' against 'host': largest relative difference of the scales {float(rel):.3g}")
    assert float(rel) <= 1e-5
    assert torch.equal(dev.quats, host.quats) and torch.equal(dev.means, host.means)
    with pytest.raises(ValueError):
        GaussianSet.from_points(pts, col, sh_degree=0, device=DEV, knn="gpu")
