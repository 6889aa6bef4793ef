"""Mesh decimation and the component filter on the GPU (csrc/gs_simplify.hip through geosplatting_amd/meshsimplify.py) against the
float64 restatement tests/simplify_ref.py, on the smallest meshes that reach each branch (tests/test_simplify_cpu.py states what the
rule does to them on the CPU).

Per edge: `edges`, `valid` and the low word of `key` are exact;  |cost - ref| <= 1e-10 |h|^T |Q| |h| + one fp32 ulp of the reference
cost (six orders above the float64 rounding of the ~40 operations, three below fp32 epsilon: an fp32 metric fails);  `position` within
2 fp32 ulps per coordinate.  Edges the restatement marks as near a branch threshold are skipped, at most 2 % of them (0 measured)."""
import functools

import numpy as np
import pytest
import torch

from tests import simplify_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _gpu(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)


def _simplify(v, f, target, **kw):
    import geosplatting_amd as gs
    v2, f2, vmap, info = gs.simplify_mesh(*_gpu(v, f), target, return_info=True, **kw)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int64 and vmap.dtype == torch.int64 and vmap.shape == (len(v),)
    return v2.cpu().numpy(), f2.cpu().numpy(), vmap.cpu().numpy(), info


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return {"bumpy": R.bumpy_sphere, "cube6": lambda: R.cube(6), "torus6x3": lambda: R.torus(6, 3), "icosphere3": lambda: R.icosphere(3),
            "torus24x12": lambda: R.torus(24, 12), "square8": lambda: R.square(8), "torus4x3": lambda: R.torus(4, 3),
            "tetrahedron": R.tetrahedron}[name]()


@functools.lru_cache(maxsize=None)
def _reference_costs(name):
    v, f = _mesh(name)
    return R.edge_costs(v, f, R.initial_quadrics(v, f))


# ------------------------------------------------------------------------------------------------ 1. per edge
@pytest.mark.parametrize("name", ["bumpy", "cube6", "torus6x3"])
def test_per_edge_against_the_restatement(name):
    import geosplatting_amd as gs
    v, f = _mesh(name)
    ref = _reference_costs(name)
    edges, cost, position, valid, key = (x.cpu().numpy() for x in gs.edge_collapse_costs(*_gpu(v, f)))
    E = len(ref["edges"])
    assert edges.dtype == np.int32 and np.array_equal(edges, ref["edges"])
    assert cost.dtype == np.float32 and position.dtype == np.float32 and valid.dtype == np.bool_ and key.dtype == np.int64
    assert np.array_equal(key & 0xFFFFFFFF, (np.arange(E, dtype=np.int64) * R.HASH) & 0xFFFFFFFF)
    assert np.array_equal(key >> 32, cost.view(np.uint32).astype(np.int64))
    full = name == "bumpy"                         # elsewhere the fallback ties are exact zeros: the branch is not comparable
    keep = ~ref["near"] if full else np.ones(E, dtype=bool)
    print(f"{name}: {E} edges, {int(ref['valid'].sum())} valid, {int((~keep).sum())} skipped as near a threshold")
    assert (~keep).sum() <= 0.02 * E
    assert np.array_equal(valid[keep], ref["valid"][keep])
    err = np.abs(cost.astype(np.float64) - ref["cost"].astype(np.float64))
    bound = 1e-10 * ref["budget"] + np.spacing(ref["cost"]).astype(np.float64)
    print(f"  cost: worst error / bound {float((err / bound)[keep].max()):.3g}, largest cost {float(ref['cost'].max()):.3g}")
    assert bool((err <= bound)[keep].all())
    if full:
        perr = np.abs(position.astype(np.float64) - ref["position"].astype(np.float64))
        ulps = perr / np.spacing(np.abs(ref["position"])).astype(np.float64)
        print(f"  position: worst error {float(ulps[keep].max()):.3g} fp32 ulps")
        assert bool((ulps[keep] <= 2.0).all())
    if name == "torus6x3":
        # exactly the 18 link failures: with the normal test switched off nothing else refuses an edge of this closed mesh
        loose = gs.edge_collapse_costs(*_gpu(v, f), min_normal_dot=-1.0)[3].cpu().numpy()
        assert int(ref["link_fail"].sum()) == 18 and np.array_equal(~loose, ref["link_fail"]) and not valid[ref["link_fail"]].any()


# ------------------------------------------------------------------------------------------------ 2. one round
def test_one_round_is_independent():
    import geosplatting_amd as gs
    v, f = _mesh("icosphere3")
    edges, cost, position, valid, key = (x.cpu().numpy() for x in gs.edge_collapse_costs(*_gpu(v, f)))
    v2, f2, vmap, info = _simplify(v, f, 1, max_rounds=1)
    assert info["rounds"] == 1 and not info["stalled"] and len(info["per_round"]) == 1
    n_edges, n_valid, n_win, n_applied = info["per_round"][0]
    assert (n_edges, n_valid) == (len(edges), int(valid.sum())) and n_win == n_applied > 0      # the budget takes every winner
    groups = {}
    for old, new in enumerate(vmap):
        groups.setdefault(int(new), []).append(old)
    assert -1 not in groups and all(len(g) <= 2 for g in groups.values())
    pairs = sorted(tuple(g) for g in groups.values() if len(g) == 2)
    assert len(pairs) == n_applied and len(f2) == len(f) - 2 * n_applied
    index = {tuple(int(x) for x in e): i for i, e in enumerate(edges)}
    nbr = [set() for _ in range(len(v))]
    for a, b in edges:
        nbr[a].add(int(b))
        nbr[b].add(int(a))
    region = [{int(a), int(b)} | nbr[a] | nbr[b] for a, b in edges]
    applied = []
    for p in pairs:
        assert p in index and valid[index[p]], p                                                 # a valid input edge
        applied.append(index[p])
    for i in applied:
        u, w = (int(x) for x in edges[i])
        assert all(not ({int(x) for x in edges[j]} & region[i]) for j in applied if j != i)     # no endpoint in another's region
        rivals = [j for j in np.nonzero(valid)[0] if u in region[j] and w in region[j]]
        assert i in rivals and all(key[i] <= key[j] for j in rivals)                             # the smallest key that claims both
        assert np.array_equal(v2[vmap[u]].view(np.uint32), position[i].view(np.uint32))          # moved bit for bit
    print(f"one round: {n_edges} edges, {n_valid} valid, {n_win} winners")


# ------------------------------------------------------------------------------------------------ 3. topology and placement
def _check_topology(name, target):
    v, f = _mesh(name)
    v2, f2, vmap, info = _simplify(v, f, target)
    print(f"{name} -> {target}: {len(f2)} faces, {len(v2)} vertices, {info['rounds']} rounds, stalled {info['stalled']}")
    assert info["stalled"] or len(f2) in (target - 1, target)
    assert R.euler(f2) == R.euler(f) and R.directed_edges_once(f2)
    assert R.is_closed_manifold(f2) == R.is_closed_manifold(f)
    assert R.no_repeats_no_unused(v2, f2) and R.map_is_consistent(f, vmap, f2)
    assert info["rounds"] == len(info["per_round"]) and bool(np.isfinite(v2).all())
    return v2, f2, info


def test_sphere():
    v2, f2, _ = _check_topology("icosphere3", 320)
    radii = np.linalg.norm(v2.astype(np.float64), axis=1)
    centroid = np.linalg.norm(v2.astype(np.float64)[f2].mean(1), axis=1).min()
    v0, f0 = R.icosphere(2)
    regular = np.linalg.norm(v0.astype(np.float64)[f0].mean(1), axis=1).min()
    print(f"  radii [{radii.min():.4f}, {radii.max():.4f}], inward deviation {(1 - centroid) / (1 - regular):.3f} x icosphere(2)'s")
    assert 1.0 <= radii.min() and radii.max() <= 1.02                 # midpoint placement lands inside the sphere
    assert 1 - centroid <= 1.5 * (1 - regular)
    assert R.signed_volume(v2, f2) > 0


def test_torus():
    _check_topology("torus24x12", 144)


@pytest.mark.parametrize("target", [48, 12])
def test_cube(target):
    v2, f2, _ = _check_topology("cube6", target)
    assert abs(R.signed_volume(v2, f2) - 1.0) <= 1e-6
    assert float(np.abs(np.abs(v2.astype(np.float64) - 0.5).max(axis=1) - 0.5).max()) <= 1e-6
    if target == 12:
        assert len(v2) == 8


def test_flat_square():
    v2, f2, _ = _check_topology("square8", 8)
    assert abs(R.area(v2, f2) - 1.0) <= 1e-6 and bool((v2[:, 2] == 0).all())
    on_border = ((v2[:, :2] == 0) | (v2[:, :2] == 1)).any(axis=1)
    boundary = np.unique([e for e, k in R.edge_faces_count(f2).items() if k == 1])
    assert bool(on_border[boundary].all())
    assert {(float(x), float(y)) for x, y, _ in v2 if x in (0, 1) and y in (0, 1)} == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}


def test_stalls():
    v2, f2, info = _check_topology("torus4x3", 12)
    assert info["stalled"] and info["per_round"][-1][2:] == (0, 0) and len(f2) > 12
    v, f = _mesh("tetrahedron")
    v2, f2, info = _check_topology("tetrahedron", 2)
    assert info["stalled"] and info["rounds"] == 1 and np.array_equal(v2, v) and np.array_equal(f2, f)


# ------------------------------------------------------------------------------------------------ 4. bits repeat
def test_bits_repeat():
    import geosplatting_amd as gs
    v, f = _gpu(*_mesh("bumpy"))
    a, b = gs.simplify_mesh(v, f, 100), gs.simplify_mesh(v, f, 100)
    assert a[1].shape[0] in (99, 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c = gs.simplify_mesh(v, f.flip(0).contiguous(), 100)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
    assert np.array_equal(R.canonical_faces(a[1].cpu().numpy()), R.canonical_faces(c[1].cpu().numpy()))


# ------------------------------------------------------------------------------------------------ 5. components
def _floaters():
    """two icosphere(1) at x = -2 / +2, a tetrahedron floater and two unused vertices; vertex indices permuted, faces shuffled"""
    rng = np.random.default_rng(3)
    sv, sf = R.icosphere(1)
    tv, tf = R.tetrahedron()
    n = len(sv)
    v = np.concatenate((sv + np.float32([-2, 0, 0]), sv + np.float32([2, 0, 0]), 0.1 * tv + np.float32([-0.5, 3, 0]), np.float32([[0, -3, 0], [0, 0, 5]])))
    f = np.concatenate((sf, sf + n, tf + 2 * n))
    perm = rng.permutation(len(v))                                       # old index -> new index
    v2 = np.empty_like(v)
    v2[perm] = v
    f2 = perm[f][rng.permutation(len(f))]
    part = np.concatenate((np.zeros(n, int), np.ones(n, int), np.full(4, 2), np.full(2, -1)))
    part2 = np.empty_like(part)
    part2[perm] = part
    return v2, f2, part2


def test_components():
    import geosplatting_amd as gs
    v, f, part = _floaters()
    want = R.union_find_labels(f, len(v))
    assert sorted(np.unique(want).tolist())[0] == -1 and len(np.unique(want)) == 4 and int((want == -1).sum()) == 2
    vd, fd = _gpu(v, f)
    vl, fl, info = gs.mesh_components(fd, len(v))
    assert vl.dtype == torch.int32 and fl.dtype == torch.int32
    assert np.array_equal(vl.cpu().numpy(), want) and np.array_equal(fl.cpu().numpy(), want[f[:, 0]])
    print(f"components: {info['iterations']} iterations on {len(f)} faces")
    tetra = part == 2
    for kw in (dict(largest=2), dict(min_faces=5)):
        v2, f2, vmap = (x.cpu().numpy() for x in gs.keep_components(vd, fd, **kw))
        kept = (part == 0) | (part == 1)
        assert np.array_equal(vmap >= 0, kept) and not (vmap[tetra] >= 0).any()
        assert np.array_equal(vmap[kept], np.arange(kept.sum())) and np.array_equal(v2, v[kept])       # ascending old index
        assert len(f2) == 160 and R.map_is_consistent(f[kept[f[:, 0]]], vmap, f2) and R.no_repeats_no_unused(v2, f2)
    v2, f2, vmap = (x.cpu().numpy() for x in gs.keep_components(vd, fd, bounds=((-4, -4, -4), (0, 4, 4))))
    assert np.array_equal(vmap >= 0, (part == 0) | tetra) and len(f2) == 84        # x <= 0: the sphere at -2 and the floater
    v2, f2, vmap = (x.cpu().numpy() for x in gs.keep_components(vd, fd, bounds=((-4, -4, -4), (0, 4, 4)), largest=1))
    assert np.array_equal(vmap >= 0, part == 0) and len(f2) == 80
    # ties go to the smaller label: the two spheres have 80 faces each
    v2, f2, vmap = (x.cpu().numpy() for x in gs.keep_components(vd, fd, largest=1))
    first = 0 if want[part == 0][0] < want[part == 1][0] else 1
    assert np.array_equal(vmap >= 0, part == first) and len(f2) == 80


def test_components_long_chain():
    """a 4096-triangle strip with permuted indices: labels have to travel the whole chain"""
    import geosplatting_amd as gs
    v, f = R.strip(4096)
    perm = np.random.default_rng(4).permutation(len(v))
    vl, fl, info = gs.mesh_components(torch.from_numpy(perm[f]).to(DEV), len(v))
    print(f"strip of 4096 triangles: {info['iterations']} iterations")
    assert bool((vl == 0).all()) and bool((fl == 0).all()) and info["iterations"] >= 1


# ------------------------------------------------------------------------------------------------ 6. errors and the hook
def test_errors():
    import geosplatting_amd as gs
    v, f = _gpu(*_mesh("tetrahedron"))
    for bad in (lambda: gs.simplify_mesh(v, f, 0), lambda: gs.simplify_mesh(v.double(), f, 2), lambda: gs.simplify_mesh(v[:, :2], f, 2),
                lambda: gs.simplify_mesh(v, f.float(), 2), lambda: gs.simplify_mesh(v, f[:, :2], 2), lambda: gs.simplify_mesh(v, f + 1, 2),
                lambda: gs.simplify_mesh(v, f - 1, 2), lambda: gs.simplify_mesh(v * float("nan"), f, 2),
                lambda: gs.simplify_mesh(v * float("inf"), f, 2), lambda: gs.edge_collapse_costs(v, f + 1),
                lambda: gs.mesh_components(f, 3), lambda: gs.mesh_components(f.float(), 4), lambda: gs.keep_components(v, f + 1, largest=1),
                lambda: gs.keep_components(v, f, largest=0)):
        with pytest.raises(ValueError):
            bad()
    # a face that repeats an index is dropped on entry; duplicate faces are legal and never collapse
    rep = torch.cat((f, torch.tensor([[0, 0, 1]], device=DEV)))
    assert torch.equal(gs.edge_collapse_costs(v, rep)[0], gs.edge_collapse_costs(v, f)[0])
    dup = torch.cat((f, f[:1]))
    edges, _, _, valid, _ = gs.edge_collapse_costs(v, dup)
    assert edges.shape[0] == 6 and not bool(valid.any())
    v2, f2, _, info = gs.simplify_mesh(v, dup, 2, return_info=True)
    assert info["stalled"] and f2.shape[0] == 5
    e = gs.simplify_mesh(v, f[:0], 1)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and bool((e[2] == -1).all())


def test_extract_mesh_hook():
    import geosplatting_amd as gs
    from geosplatting_amd import synthetic as syn
    v, f = syn.icosphere(3, radius=0.5)
    v, f = v.to(DEV), f.to(DEV)
    sp, _ = gs.mesh_to_splats(v, f, gs.vertex_normals(v, f))
    n = sp.means.shape[0]
    g = gs.GaussianSet(means=sp.means, scales=sp.scales, quats=sp.quats, opacities=sp.opacities.reshape(n, 1),
                       colors=torch.full((n, 3), 0.5, device=DEV), shs=torch.zeros(n, 3, 3, device=DEV))
    model = gs.GSplatModel(gaussians=g, background_color="black")
    kw = dict(resolution=32, num_views=8, radius=3.0, image_size=96, bounds=((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8)))
    plain = model.extract_mesh(generator=torch.Generator().manual_seed(5), **kw)
    again = model.extract_mesh(generator=torch.Generator().manual_seed(5), target_faces=None, min_component_faces=None, **kw)
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1]) and plain[1].shape[0] > 400
    # (eight small views leave this shell with holes, Euler characteristic -39: decimation keeps them and stalls near 230 faces)
    v2, f2 = model.extract_mesh(generator=torch.Generator().manual_seed(5), target_faces=1000, min_component_faces=20, **kw)
    print(f"extract_mesh: {plain[1].shape[0]} faces, {f2.shape[0]} with target_faces=1000")
    assert 0 < f2.shape[0] <= 1000 and f2.dtype == torch.int64 and int(f2.max()) == v2.shape[0] - 1
    assert bool(torch.isfinite(v2).all())
    only = model.extract_mesh(generator=torch.Generator().manual_seed(5), min_component_faces=20, **kw)
    assert 5000 < only[1].shape[0] < plain[1].shape[0]                  # the floaters go, the shell stays
