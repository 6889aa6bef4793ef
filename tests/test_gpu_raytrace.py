"""Ray queries on the GPU (csrc/gs_bvh.hip, geosplatting_amd/raytrace.py) against the node-buffer contract, against their own
brute-force form, and against the float64 restatement of tests/raytrace_ref.py.

Three kinds of condition, none of them a measured tolerance:
  * structure: the device-built node buffer is walked on the host against the layout include/geosplat_hip.h fixes;
  * BVH == brute force BIT FOR BIT on every ray, fragile ones included: the two forms share one triangle routine, the box test is
    conservative (it never culls a box that holds a triangle the routine would accept) and the closest hit is a minimum over
    (t, face), which does not depend on the order of traversal;
  * against float64 on the rays the reference does not mark fragile (raytrace_ref: within rounding of an edge, of an end of the
    interval, or of a second face): the occluded flag and the face are EQUAL, and
        |t - t_ref| <= eps_t,   |b_i - b_ref_i| <= eps_b  (i = 1, 2),   |b_0 - b_ref_0| <= 2 eps_b + 2 u   (b_0 = 1 - b_1 - b_2 in fp32)
    with eps_b = 4 (20 L M + 6 L^2) u / |det| + 4 u and eps_t = 3 eps_b (max z - min z) + 8 u max |z| of the winning pair, u = 2^-24,
    as derived from the kernel's arithmetic in the docstring of raytrace_ref.  The fragile share is asserted <= 1 % here too.
  * watertightness: rays aimed at every vertex, edge midpoint and edge third point of a closed mesh from inside never leak, with
    no fragile exclusion.

Measured on an MI355X: the largest error is 0.53 of the budget in t (the flat grid; 0.05 - 0.35 on the other meshes) and 0.04 of it in
the barycentrics; the fragile share is 0.46 % on the flat grid and at most 0.06 % elsewhere; no BVH result differs from brute force,
and no fragile shadow ray differed from float64 either."""
import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from tests import raytrace_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FRAGILE_CAP = 0.01
U24 = 2.0 ** -24
NODE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("left", "<i4"), ("skip", "<i4")])

_cache = {}


def _bvh(name):
    """one MeshBVH per mesh and process (int32 faces for every other mesh: both dtypes are accepted)"""
    if name not in _cache:
        v, f = ref.mesh(name)
        ft = torch.from_numpy(f).to(DEV)
        if ref.MESH_NAMES.index(name) % 2:
            ft = ft.to(torch.int32)
        _cache[name] = gs.MeshBVH(torch.from_numpy(v).to(DEV), ft)
    return _cache[name]


def _nodes(bvh):
    return np.frombuffer(bvh.nodes.cpu().numpy().tobytes(), dtype=NODE)


def _query(bvh, batch, brute):
    o, d = torch.from_numpy(batch["origins"]).to(DEV), torch.from_numpy(batch["dirs"]).to(DEV)
    kw = dict(tmin=batch["tmin"], tmax=batch["tmax"], brute_force=brute)
    occ = bvh.occluded(o, d, **kw)
    t, face, bary = bvh.closest_hit(o, d, **kw)
    return occ, t, face, bary


def _results(name, brute):
    key = (name, brute)
    if key not in _cache:
        _cache[key] = [_query(_bvh(name), b, brute) for b in ref.ray_batches(name)]
    return _cache[key]


def _leaf_box(v, f, V):
    tri = v[np.clip(f, 0, V - 1)]
    if (f < 0).any() or (f >= V).any() or not np.isfinite(tri).all():
        return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    return tri.min(0), tri.max(0)


@pytest.mark.parametrize("name", ref.MESH_NAMES)
def test_node_buffer_structure(name):
    v, f = ref.mesh(name)
    V, F = v.shape[0], f.shape[0]
    bvh = _bvh(name)
    assert bvh.nodes.numel() == 32 * (2 * F - 1)
    n = _nodes(bvh)
    assert n.shape[0] == 2 * F - 1
    left, skip = n["left"].astype(np.int64), n["skip"].astype(np.int64)
    is_leaf = np.arange(2 * F - 1) >= F - 1
    # the depth-first walk over left / skip links visits every node once and ends
    order, node = [], 0
    while node >= 0 and len(order) <= 2 * F:
        assert 0 <= node < 2 * F - 1
        order.append(node)
        node = skip[node] if is_leaf[node] else left[node]
    assert sorted(order) == list(range(2 * F - 1))
    # every face is in exactly one leaf
    assert sorted(left[is_leaf].tolist()) == list(range(F))
    assert skip[0] == -1
    for i in range(F - 1):                                                            # internal nodes
        L = left[i]
        assert 0 < L < 2 * F - 1
        R = skip[L]
        assert 0 < R < 2 * F - 1 and R != L and skip[R] == skip[i]
        # a box is the union of its children's (min / max are exact) -- so it contains them and, by induction, its triangles
        assert np.array_equal(n["lo"][i], np.minimum(n["lo"][L], n["lo"][R])) and np.array_equal(n["hi"][i], np.maximum(n["hi"][L], n["hi"][R]))
    los, his = zip(*[_leaf_box(v, f[k], V) for k in range(F)])
    los, his = np.stack(los), np.stack(his)
    leaf_faces = left[is_leaf]
    assert np.array_equal(n["lo"][is_leaf], los[leaf_faces]) and np.array_equal(n["hi"][is_leaf], his[leaf_faces])
    # the root box is the bounds of the finite faces: the NaN vertex is in no box, the sliver and the zero-area face are
    assert np.array_equal(n["lo"][0], los.min(0)) and np.array_equal(n["hi"][0], his.max(0))
    assert np.isfinite(n["lo"][0]).all() and np.isfinite(n["hi"][0]).all()
    # two builds give the same bytes
    again = gs.MeshBVH(bvh.vertices.clone(), bvh.faces.clone())
    assert torch.equal(again.nodes, bvh.nodes)


@pytest.mark.parametrize("name", ["tri1", "tri2", "ico2", "bad"])
def test_rebuild_equals_a_fresh_build(name):
    v, f = ref.mesh(name)
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    bvh = gs.MeshBVH(vt, ft)
    before = bvh.nodes.clone()
    moved = (vt * torch.tensor([1.1, 0.9, 1.3], device=DEV) + torch.tensor([0.05, -0.02, 0.4], device=DEV)).contiguous()
    assert bvh.rebuild(moved) is bvh
    fresh = gs.MeshBVH(moved, ft)
    assert torch.equal(bvh.nodes, fresh.nodes) and not torch.equal(bvh.nodes, before)
    o = torch.tensor([[0.0, 0.0, 3.0]], device=DEV)
    d = (moved[ft[0]].mean(0) - o[0])[None].contiguous()                              # at the centroid of face 0, where it is now
    assert bool(bvh.occluded(o, d)[0, 0]) and bool(bvh.occluded(o, d, brute_force=True)[0, 0])
    with pytest.raises(ValueError, match="rebuild needs vertices of shape"):
        bvh.rebuild(moved[:-1])


@pytest.mark.parametrize("name", ref.MESH_NAMES)
def test_bvh_equals_brute_force_bit_for_bit(name):
    for batch, a, b in zip(ref.ray_batches(name), _results(name, False), _results(name, True)):
        P = batch["origins"].shape[0]
        S = ref.expand(batch["origins"], batch["dirs"])[2]
        assert a[0].shape == (P, S) and a[0].dtype == torch.bool and a[1].dtype == torch.float32 and a[2].dtype == torch.int64
        assert a[3].shape == (P, S, 3)
        assert torch.equal(a[0], b[0]), batch["label"]
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), batch["label"]
        assert torch.equal(a[2], b[2]), batch["label"]
        assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)), batch["label"]
        # occluded and closest agree with each other: the same triangles are accepted
        assert torch.equal(a[0], a[2] >= 0) and torch.equal(a[0], torch.isfinite(a[1]))


@pytest.mark.parametrize("name", ref.MESH_NAMES)
def test_against_float64_on_non_fragile_rays(name):
    n_fragile = n_rays = 0
    worst_t = worst_b = 0.0
    for batch, got, want in zip(ref.ray_batches(name), _results(name, False), ref.expected(name)):
        occ, t, face, bary = (x.cpu().numpy().reshape((-1,) + tuple(x.shape[2:])) for x in got)
        keep_any, keep = ~want["fragile_any"], ~want["fragile"]
        n_fragile += int(want["fragile"].sum())
        n_rays += keep.size
        assert np.array_equal(occ[keep_any], want["occluded"][keep_any]), batch["label"]
        assert np.array_equal(face[keep], want["face"][keep]), batch["label"]
        hit = keep & (want["face"] >= 0)
        assert np.isinf(t[keep & ~hit]).all() and not bary[keep & ~hit].any()
        err_t = np.abs(t[hit].astype(np.float64) - want["t"][hit])
        err_b = np.abs(bary[hit].astype(np.float64) - want["bary"][hit])
        bb = want["b_budget"][hit]
        budget_b = np.stack([2 * bb + 2 * U24, bb, bb], -1)
        if hit.any():
            worst_t = max(worst_t, float((err_t / want["t_budget"][hit]).max()))
            worst_b = max(worst_b, float((err_b / budget_b).max()))
        assert (err_t <= want["t_budget"][hit]).all(), batch["label"]
        assert (err_b <= budget_b).all(), batch["label"]
        # the invalid rays of the last batch miss
        if batch["label"] == "single":
            assert not occ[[3, 7, 11]].any() and (face[[3, 7, 11]] == -1).all()
    print(f"{name}: fragile {100 * n_fragile / n_rays:.3f} % of {n_rays} rays, max err / budget: t {worst_t:.3f}, bary {worst_b:.3f}")
    assert n_fragile <= FRAGILE_CAP * n_rays


def test_special_faces_are_never_hit():
    """the zero-area face and the NaN-vertex face of 'bad' are never reported, by either form; the sliver across the scene is"""
    v, f = ref.mesh("bad")
    zero, nan, sliver = 40, 61, f.shape[0] - 1
    assert f[zero][1] == f[zero][2] and np.isnan(v[f[nan][0]]).any()
    faces = torch.cat([r[2].reshape(-1) for brute in (False, True) for r in _results("bad", brute)])
    assert not bool(((faces == zero) | (faces == nan)).any())
    bvh = _bvh("bad")
    s0, s1, s2 = v[f[sliver]].astype(np.float64)
    p = s0 + (5.0 / 6.0) * (0.5 * (s1 + s2) - s0)                                      # inside the sliver, outside the sphere (x = 2)
    o = torch.tensor([[p[0], p[1], p[2] + 0.5]], device=DEV, dtype=torch.float32)
    t, face, _ = bvh.closest_hit(o, torch.tensor([[0.0, 0.0, -1.0]], device=DEV))
    assert int(face[0, 0]) == sliver and abs(float(t[0, 0]) - 0.5) < 1e-5
    # rays aimed at the corners of the zero-area face from outside still hit its neighbours, never it
    o2 = torch.from_numpy(v[f[zero]] * 3.0).to(DEV).contiguous()
    t2, face2, _ = bvh.closest_hit(o2, -o2)
    assert bool((face2 >= 0).all()) and not bool((face2 == zero).any())


def test_duplicate_faces_tie_to_the_lowest_index():
    for brute in (False, True):
        for r in _results("dup64", brute):
            assert bool(((r[2] == 0) | (r[2] == -1)).all())
    assert any(bool((r[2] == 0).any()) for r in _results("dup64", False))


def test_watertight_closed_mesh():
    """Every ray from inside the closed bumpy icosphere(2) towards a vertex, an edge midpoint or an edge third point (targets and
    directions rounded to fp32, so the rays pass within rounding of the edges, on either side) is occluded and has a closest hit:
    no leaks, no fragile exclusion."""
    v, f = ref.mesh("ico2")
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    assert e.shape[0] == 480
    a, b = v[e[:, 0]], v[e[:, 1]]
    third = np.float32(1.0) / np.float32(3.0)
    targets = np.concatenate([v, (a + b) * np.float32(0.5), a + (b - a) * third, b + (a - b) * third]).astype(np.float32)
    origins = np.array([[0.0, 0.0, 0.0], [0.2, -0.1, 0.15], [-0.3, 0.25, -0.2]], np.float32)
    dirs = (targets[None] - origins[:, None]).astype(np.float32)
    assert dirs.shape == (3, 162 + 3 * 480, 3)
    bvh = _bvh("ico2")
    o, d = torch.from_numpy(origins).to(DEV), torch.from_numpy(dirs).to(DEV)
    for brute in (False, True):
        occ = bvh.occluded(o, d, brute_force=brute)
        t, face, bary = bvh.closest_hit(o, d, brute_force=brute)
        assert int((~occ).sum()) == 0 and int((face < 0).sum()) == 0
        assert bool(torch.isfinite(t).all()) and bool((t > 0.5).all()) and bool((t < 1.5).all())    # the target is at t = 1


def test_shared_directions_equal_expanded_directions():
    bvh = _bvh("ico3")
    b = ref.ray_batches("ico3")[3]
    assert b["label"] == "inside" and b["dirs"].ndim == 2
    o, d = torch.from_numpy(b["origins"]).to(DEV), torch.from_numpy(b["dirs"]).to(DEV)
    full = d[None].expand(o.shape[0], -1, -1).contiguous()
    for brute in (False, True):
        assert torch.equal(bvh.occluded(o, d, brute_force=brute), bvh.occluded(o, full, brute_force=brute))
        for x, y in zip(bvh.closest_hit(o, d, brute_force=brute), bvh.closest_hit(o, full, brute_force=brute)):
            assert torch.equal(x, y)
    with pytest.raises(ValueError, match=r"dirs must be.*\(15, 64, 3\)"):
        bvh.occluded(o, full[:15])
    with pytest.raises(gs._lib.GeoSplatHipError, match="GPU only"):
        bvh.occluded(o.cpu(), d.cpu())


def test_shadow_visibility_of_mgadapter_gaussians():
    """The reference's shadow_test as splat_mc calls it: origins = position + normal * offset, offset 1e-5 and 1e-3, 8 fixed
    directions, from the MGAdapter Gaussians of the bumpy icosphere(2) made by the existing mesh ops."""
    v, f = ref.mesh("ico2")
    vt, ft = torch.from_numpy(v).to(DEV).requires_grad_(True), torch.from_numpy(f).to(DEV)
    splats, normals = gs.mesh_to_splats(vt, ft, gs.vertex_normals(vt, ft))
    pos, nrm = splats.means[::ref.SHADOW_STRIDE], normals[::ref.SHADOW_STRIDE]
    assert pos.requires_grad and pos.shape[0] == 640
    bvh = _bvh("ico2")
    dirs = torch.from_numpy(ref.SHADOW_DIRS).to(DEV)
    for offset in (1e-5, 1e-3):
        vis = gs.shadow_visibility(bvh, pos, nrm, dirs, offset=offset)
        assert vis.shape == (640, 8) and vis.dtype == torch.float32 and not vis.requires_grad
        want = ref.shadow_expected(pos.detach().cpu().numpy(), nrm.detach().cpu().numpy(), offset)
        keep = ~want["fragile_any"]
        got = vis.cpu().numpy().reshape(-1)
        print(f"shadow offset {offset}: fragile {100 * (~keep).mean():.3f} %, lit {got.mean():.3f}, mismatches among fragile "
              f"{int((got[~keep] != 1.0 - want['occluded'][~keep]).sum())}")
        assert (~keep).mean() <= FRAGILE_CAP
        assert set(np.unique(got)) <= {0.0, 1.0}
        assert np.array_equal(got[keep], 1.0 - want["occluded"][keep])
        half = gs.shadow_visibility(bvh, pos, nrm, dirs, offset=offset, shadow_scale=0.5)
        assert torch.equal(half, vis * 0.5 + 0.5) and not half.requires_grad
        assert torch.equal(vis, 1.0 - bvh.occluded((pos + nrm * offset).detach(), dirs, tmax=1e16, brute_force=True).float())


def test_empty_and_bad_input_on_the_device():
    with pytest.raises(ValueError, match="empty mesh"):
        gs.MeshBVH(torch.zeros(3, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    with pytest.raises(gs._lib.GeoSplatHipError, match=r"float64.*\(3, 3\)"):
        gs.MeshBVH(torch.zeros(3, 3, device=DEV, dtype=torch.float64), torch.tensor([[0, 1, 2]], device=DEV))
    bvh = _bvh("tri1")
    occ = bvh.occluded(torch.zeros(0, 3, device=DEV), torch.zeros(4, 3, device=DEV))     # no rays: fine
    assert occ.shape == (0, 4)
