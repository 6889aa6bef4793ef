"""Float64 CPU restatement of the mesh-prior regularisers (csrc/gs_meshreg.hip, geosplatting_amd/meshreg.py) with per-element error
budgets, shared by tests/test_meshreg_cpu.py, tests/test_gpu_meshreg.py and tests/test_gpu_stage2.py.  Everything here runs on the CPU.

`topology(faces, V)` builds the index arrays on its own (a dictionary over the sides, in Python): edges (lo, hi) ascending by
lo V + hi, pairs (v0, v1, a, b) for every two faces f < g of an edge ascending in (edge, f, g), the neighbour sets.  `evaluate` returns
the per-item terms, the three means and the ANALYTIC gradients of each mean, all in float64, and the budgets.

Budgets follow the project's contract (KAPPA = 1e-4 as in tests/loss_budget.py): an element's bound is KAPPA times the float64 sum of
the absolute values of the terms added to form it.  The terms, per element:

  lap_i        d_i = deg_i v_i - sum_j v_j per component c:  A_ic = deg_i |v_ic| + sum_j |v_jc|;  the term is |d_i|, whose error is at most
               the length of the error of d_i:  bound = KAPPA |A_i|_2
  edge_e       (len - t)^2 = len^2 - 2 len t + t^2 with len^2 = sum_c (v_lo,c - v_hi,c)^2:
               bound = KAPPA (sum_c (|v_lo,c| + |v_hi,c|)^2 + 2 len |t| + t^2)
  nc_p         1 - cos:  bound = KAPPA (1 + |cos|)
  mean         (1/N) sum of the terms:  bound = KAPPA (1/N) sum |term| + (1/N) sum of the terms' bounds
  d lap / d v_kc    (1/V) (deg_k u_kc - sum_{j in N(k)} u_jc), u = d / |d|:  KAPPA (1/V) (deg_k |u_kc| + sum_j |u_jc|)
  d edge / d v_kc   (1/E) sum_{j in N(k)} [2 (v_kc - v_jc) - 2 t (v_kc - v_jc) / len_kj]:
                    KAPPA (1/E) sum_j (2 |v_kc| + 2 |v_jc| + 2 |t| (|v_kc| + |v_jc|) / len_kj)
  d nc / d v_kc     (1/P) sum over the (pair, role) appearances of k.  With G0 = d nc / d n0 = -(mh - cos nh0) / |n0| (mh = -n1 / |n1|,
                    nh0 = n0 / |n0|: the two cancelling parts mh / |n0| and cos nh0 / |n0|), G1 likewise, e = v1 - v0, pa = a - v0, pb = b - v0:
                      role v1: pa x G0 + pb x G1,  role a: G0 x e,  role b: G1 x e,  role v0: minus the sum of the three;
                    every component of a cross product is a difference of two products.  The absolute sum replaces every product by
                    the product of absolute values, with |G0|_c := (|mh_c| + |cos nh0_c|) / max(|n0|, 1e-8), and e, pa, pb by the sums
                    of the absolute coordinates they are differences of:  KAPPA (1/P) times that sum.
"""
import functools

import numpy as np
import torch

KAPPA = 1e-4
EPS = 1e-8


def topology(faces, V):
    """faces [F,3] (any integer array-like) -> dict of int64 numpy arrays: edges [E,2], pairs [P,4], degree [V], and `nbrs`, a list of
    sorted neighbour lists"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sides = {}
    for f, (i, j, k) in enumerate(faces.tolist()):
        for (p, q, o) in ((i, j, k), (j, k, i), (k, i, j)):
            sides.setdefault((min(p, q), max(p, q)), []).append((f, o))
    keys = sorted(sides)
    edges = np.array(keys, dtype=np.int64).reshape(-1, 2)
    pairs = []
    for (lo, hi) in keys:
        inc = sorted(sides[(lo, hi)])
        for x in range(len(inc)):
            for y in range(x + 1, len(inc)):
                pairs.append((lo, hi, inc[x][1], inc[y][1]))
    nbrs = [set() for _ in range(V)]
    for lo, hi in keys:
        nbrs[lo].add(hi); nbrs[hi].add(lo)
    nbrs = [sorted(s) for s in nbrs]
    return {"edges": edges, "pairs": np.array(pairs, dtype=np.int64).reshape(-1, 4), "nbrs": nbrs,
            "degree": np.array([len(s) for s in nbrs], dtype=np.int64)}


def _cross(a, b):
    return torch.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), 1)


def _cross_abs(a, b):
    """the absolute sum of the products of a cross product's components, for non-negative a and b"""
    return torch.stack((a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]), 1)


def _unit(d):
    n = d.norm(dim=1, keepdim=True)
    return torch.where(n > 0, d / n.clamp_min(1e-300), torch.zeros_like(d)), n[:, 0]


def evaluate(vertices, topo, target_length=0.0):
    """vertices [V,3] (any float tensor) -> dict of float64 CPU tensors:
    lap_terms [V], edge_terms [E], nc_terms [P], lap / edge / nc (0-d), grad_lap / grad_edge / grad_nc [V,3] (of the MEANS), and the
    budgets under the same names with the suffix _budget"""
    v = vertices.detach().double().cpu()
    V, t = v.shape[0], float(target_length)
    edges, pairs = torch.from_numpy(topo["edges"]), torch.from_numpy(topo["pairs"])
    E, P = edges.shape[0], pairs.shape[0]
    deg = torch.from_numpy(topo["degree"]).double()
    # adjacency as both directions of every edge
    src, dst = torch.cat((edges[:, 0], edges[:, 1])), torch.cat((edges[:, 1], edges[:, 0]))
    out = {}

    def scatter(values):                                                      # sum over the neighbours j of k of values[(k, j)]
        return torch.zeros(V, 3, dtype=torch.float64).index_add_(0, src, values)

    # Laplacian
    d = deg[:, None] * v - scatter(v[dst])
    u, dn = _unit(d)
    out["lap_terms"] = dn
    out["lap_terms_budget"] = KAPPA * (deg[:, None] * v.abs() + scatter(v[dst].abs())).norm(dim=1)
    out["grad_lap"] = (deg[:, None] * u - scatter(u[dst])) / max(V, 1)
    out["grad_lap_budget"] = KAPPA * (deg[:, None] * u.abs() + scatter(u[dst].abs())) / max(V, 1)
    # edges
    dv = v[edges[:, 0]] - v[edges[:, 1]]
    ln = dv.norm(dim=1)
    out["edge_terms"] = (ln - t) ** 2
    out["edge_terms_budget"] = KAPPA * (((v[edges[:, 0]].abs() + v[edges[:, 1]].abs()) ** 2).sum(1) + 2 * ln * abs(t) + t * t)
    dkj = v[src] - v[dst]
    lkj = dkj.norm(dim=1, keepdim=True)
    safe = lkj.clamp_min(1e-300)
    g = torch.where(lkj > 0, 2 * dkj - 2 * t * dkj / safe, torch.zeros_like(dkj))
    ga = torch.where(lkj > 0, (2 + 2 * abs(t) / safe) * (v[src].abs() + v[dst].abs()), torch.zeros_like(dkj))
    out["grad_edge"] = scatter(g) / max(E, 1)
    out["grad_edge_budget"] = KAPPA * scatter(ga) / max(E, 1)
    # normal consistency
    v0, v1, a, b = (v[pairs[:, k]] for k in range(4))
    e, pa, pb = v1 - v0, a - v0, b - v0
    ea, paa, pba = v1.abs() + v0.abs(), a.abs() + v0.abs(), b.abs() + v0.abs()
    n0, n1 = _cross(e, pa), _cross(e, pb)
    m1 = -n1
    l0, l1 = n0.norm(dim=1, keepdim=True), n1.norm(dim=1, keepdim=True)
    c0, c1 = l0.clamp_min(EPS), l1.clamp_min(EPS)
    s = (n0 * m1).sum(1, keepdim=True)
    cos = s / (c0 * c1)
    out["nc_terms"] = (1 - cos)[:, 0]
    out["nc_terms_budget"] = KAPPA * (1 + cos.abs())[:, 0]
    # d (1 - cos) / d n0 = -(m1 / (c0 c1) - cos n0 / (c0 l0)) where l0 >= eps (the clamp passes the gradient), else -m1 / (c0 c1)
    on0, on1 = (l0 >= EPS).double(), (l1 >= EPS).double()
    G0 = -(m1 / (c0 * c1) - on0 * cos * n0 / (c0 * l0.clamp_min(1e-300)))
    H1 = -(n0 / (c0 * c1) - on1 * cos * m1 / (c1 * l1.clamp_min(1e-300)))     # with respect to m1
    G1 = -H1
    G0a = m1.abs() / (c0 * c1) + on0 * (cos * n0).abs() / (c0 * l0.clamp_min(1e-300))
    G1a = n0.abs() / (c0 * c1) + on1 * (cos * m1).abs() / (c1 * l1.clamp_min(1e-300))
    ge, gpa, gpb = _cross(pa, G0) + _cross(pb, G1), _cross(G0, e), _cross(G1, e)
    gea, gpaa, gpba = _cross_abs(paa, G0a) + _cross_abs(pba, G1a), _cross_abs(G0a, ea), _cross_abs(G1a, ea)
    grad, gabs = torch.zeros(V, 3, dtype=torch.float64), torch.zeros(V, 3, dtype=torch.float64)
    for k, (gv, gva) in enumerate(((-(ge + gpa + gpb), gea + gpaa + gpba), (ge, gea), (gpa, gpaa), (gpb, gpba))):
        grad.index_add_(0, pairs[:, k], gv)
        gabs.index_add_(0, pairs[:, k], gva)
    out["grad_nc"] = grad / max(P, 1)
    out["grad_nc_budget"] = KAPPA * gabs / max(P, 1)
    for name, n in (("lap", V), ("edge", E), ("nc", P)):
        terms, bud = out[name + "_terms"], out[name + "_terms_budget"]
        out[name] = terms.sum() / n if n > 0 else torch.zeros((), dtype=torch.float64)
        out[name + "_budget"] = (KAPPA * terms.abs().sum() + bud.sum()) / n if n > 0 else torch.zeros((), dtype=torch.float64)
    return out


def literal(vertices, faces, topo, target_length=0.0):
    """The three values by the literal formulas in float64 with autograd: a sparse uniform Laplacian `L @ v` (L = D - A over the unique
    undirected edges) and `norm`, the edge lengths, `torch.cosine_similarity` of the two normals of every pair.  -> (lap, edge, nc)"""
    v = vertices
    V = v.shape[0]
    edges, pairs = torch.from_numpy(topo["edges"]), torch.from_numpy(topo["pairs"])
    zero = (v.sum() * 0)
    if edges.shape[0] > 0:
        i = torch.cat((edges, edges.flip(1), torch.arange(V)[:, None].expand(V, 2)), 0).t()
        w = torch.cat((-torch.ones(2 * edges.shape[0], dtype=v.dtype), torch.from_numpy(topo["degree"]).to(v.dtype)))
        L = torch.sparse_coo_tensor(i, w, (V, V)).coalesce()
        lap = torch.sparse.mm(L, v).norm(dim=1).mean()
        edge = ((v[edges[:, 0]] - v[edges[:, 1]]).norm(dim=1) - target_length).square().mean()
    else:
        lap, edge = zero, zero
    if pairs.shape[0] > 0:
        v0, v1, a, b = (v[pairs[:, k]] for k in range(4))
        n0, n1 = torch.cross(v1 - v0, a - v0, dim=1), torch.cross(v1 - v0, b - v0, dim=1)
        nc = (1 - torch.cosine_similarity(n0, -n1, dim=1)).mean()
    else:
        nc = zero
    return lap, edge, nc


def grid_mesh(nx, ny):
    """a flat regular nx x ny vertex grid in the z = 0 plane, two triangles a cell -> (vertices [nx ny, 3] float64, faces int64)"""
    ys, xs = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
    v = torch.stack((xs.reshape(-1).double(), ys.reshape(-1).double(), torch.zeros(nx * ny, dtype=torch.float64)), 1)
    i = (ys[:-1, :-1] * nx + xs[:-1, :-1]).reshape(-1)
    f = torch.cat((torch.stack((i, i + 1, i + nx), 1), torch.stack((i + 1, i + nx + 1, i + nx), 1)), 0)
    return v, f


def fan_mesh(n):
    """n triangles around vertex 0, open: vertices 1..n+1 on a circle, the centre lifted -> (vertices [n+2,3] float64, faces int64)"""
    ang = torch.arange(n + 1, dtype=torch.float64) * (2 * np.pi * 0.9 / n)
    rim = torch.stack((ang.cos(), ang.sin(), torch.zeros_like(ang)), 1)
    v = torch.cat((torch.tensor([[0.0, 0.0, 0.4]], dtype=torch.float64), rim), 0)
    k = torch.arange(n)
    return v, torch.stack((torch.zeros(n, dtype=torch.long), k + 1, k + 2), 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared cases: -> (vertices float32 [V,3], faces int64 [F,3], topology dict).  Jitter from a fixed seed."""
    from geosplatting_amd.synthetic import icosphere
    g = torch.Generator().manual_seed(1234)
    jit = lambda v, s: (v.double() + s * (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1)).float()
    if name == "icosphere2":
        v, f = icosphere(2)
        v = jit(v, 0.03)
    elif name == "icosphere3":
        v, f = icosphere(3)
        v = jit(v, 0.01)
    elif name == "grid":                                    # open patch: the boundary edges have no pair
        v, f = grid_mesh(9, 7)
        v = jit(v * 0.25, 0.05)
    elif name == "three_faces":                             # three faces on the edge (0, 1): 3 pairs
        v = torch.tensor([[0, 0, 0], [1, 0, 0], [0.4, 1, 0.1], [0.5, -0.9, 0.3], [0.6, 0.2, 1.1]], dtype=torch.float32)
        f = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    elif name == "unused_vertex":
        v, f = icosphere(1)
        v = torch.cat((jit(v, 0.03), torch.tensor([[3.0, 3.0, 3.0]])), 0)
    elif name == "fan200":                                  # the centre has 201 neighbours and 199 (pair, role) codes: above 64 and above 128
        v, f = fan_mesh(200)
        v = jit(v, 0.004)
    elif name == "one_triangle":
        v, f = torch.tensor([[0, 0, 0], [1, 0, 0.2], [0.3, 1, 0]], dtype=torch.float32), torch.tensor([[0, 1, 2]])
    elif name == "no_faces":
        v, f = jit(torch.zeros(5, 3), 1.0), torch.zeros(0, 3, dtype=torch.long)
    else:
        raise KeyError(name)
    f = f.long()
    return v.contiguous(), f, topology(f.numpy(), v.shape[0])


CASES = ("icosphere2", "icosphere3", "grid", "three_faces", "unused_vertex", "fan200", "one_triangle", "no_faces")
