"""The mesh-prior regularisers of the reference's `GeoSplatterPrior` (rfstudio/model/geosplat_prior.py: a uniform-Laplacian term,
pytorch3d's `mesh_edge_loss` and `mesh_normal_consistency`) on a topology that is built ONCE per face array (csrc/gs_meshreg.hip).

The reference rebuilds the Laplacian (a `unique` over 2 * 3F index pairs) and a pytorch3d `Meshes` (another sort / unique for
`edges_packed`) in every step although the faces never change.  Here `MeshRegTopology` does that work at construction, with torch ops
on the device; a step is one forward launch over the V + E + P items plus a one-workgroup sum, and one backward launch over the
vertices.  Neither uses atomics: the same inputs give the same bits.  include/geosplat_hip.h states the formulas."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib

__all__ = ["MeshRegTopology", "mesh_regularizers", "laplacian_smooth_loss", "mesh_edge_loss", "mesh_normal_consistency"]

LONG_LIST = 64                     # MR_LONG of csrc/gs_meshreg.hip: a vertex with a longer list is walked by a wave
MAX_ITEMS = 1 << 30


class MeshRegTopology:
    """Index arrays of the three regularisers for `faces` [F,3] over `num_vertices` vertices (see the module docstring).

    edges [E,2] int32   the unique undirected sides (lo, hi), lo < hi, ascending by lo * V + hi
    degree [V] int32    distinct neighbours of a vertex; 0 for a vertex no face uses
    pairs [P,4] int32   (v0, v1, a, b): for every edge with k >= 2 faces every unordered pair f < g of them, ascending in (edge, f, g);
                        (v0, v1) the edge, a / b the vertices of f / g opposite to it.  k faces give k (k - 1) / 2 pairs.
    nbr_off [V+1], nbr [2E] / pr_off [V+1], pr [4P]: the inverted lists of the backward (neighbours; codes 4 * pair + role), ascending
    long_verts [NL]     vertices with more than LONG_LIST entries in either list

    Built with torch ops on the device of `faces` (a one-time cost; the counts are read back here, nothing is per step).
    Raises ValueError for a face with a repeated vertex index and for an index outside [0, num_vertices)."""

    def __init__(self, faces: Tensor, num_vertices: int):
        if not isinstance(faces, Tensor) or faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"faces must be an int32 / int64 tensor [F,3], got "
                             f"{(faces.dtype, tuple(faces.shape)) if isinstance(faces, Tensor) else type(faces).__name__}")
        V = int(num_vertices)
        if V < 0 or V >= MAX_ITEMS:
            raise ValueError(f"num_vertices must be in [0, 2^30), got {num_vertices}")
        dev, F = faces.device, faces.shape[0]
        f = faces.long()
        if F > 0:
            if int(f.min()) < 0 or int(f.max()) >= V:
                raise ValueError(f"faces index outside [0, {V}): min {int(f.min())}, max {int(f.max())}")
            if bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any()):
                raise ValueError("a face repeats a vertex index")
        # the 3F sides, face-major (so that a stable sort by edge leaves the faces of an edge ascending), and their opposite vertices
        a, b, opp = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
        lo, hi = torch.minimum(a, b), torch.maximum(a, b)
        key, order = torch.sort(lo * V + hi, stable=True)
        opp = opp[order]
        ukey, count = torch.unique_consecutive(key, return_counts=True)
        E = ukey.shape[0]
        e_lo, e_hi = ukey // max(V, 1), ukey % max(V, 1)
        self.edges = torch.stack((e_lo, e_hi), dim=1).to(torch.int32).contiguous()
        # pairs: the side at rank r of an edge with k sides is the first member of k - 1 - r pairs, with the sides after it
        start = torch.cumsum(count, 0) - count
        edge_of = torch.repeat_interleave(torch.arange(E, device=dev), count)
        rank = torch.arange(3 * F, device=dev) - start[edge_of]
        n_first = count[edge_of] - 1 - rank
        first = torch.repeat_interleave(torch.arange(3 * F, device=dev), n_first)
        P = first.shape[0]
        if V + E + P > MAX_ITEMS or 4 * P > MAX_ITEMS:
            raise ValueError(f"mesh too large: V + E + P = {V + E + P} and 4 P must not exceed 2^30")
        pstart = torch.cumsum(n_first, 0) - n_first
        second = first + 1 + (torch.arange(P, device=dev) - pstart[first])
        pe = edge_of[first]
        self.pairs = torch.stack((e_lo[pe], e_hi[pe], opp[first], opp[second]), dim=1).to(torch.int32).contiguous()
        # neighbour lists: both directions of every edge, by (vertex, neighbour)
        src, dst = torch.cat((e_lo, e_hi)), torch.cat((e_hi, e_lo))
        nkey, _ = torch.sort(src * V + dst)
        self.nbr = (nkey % max(V, 1)).to(torch.int32).contiguous()
        degree = torch.bincount(src, minlength=V)[:V] if V > 0 else torch.zeros(0, dtype=torch.long, device=dev)
        self.degree = degree.to(torch.int32)
        self.nbr_off = self._offsets(degree, dev)
        # (pair, role) lists: codes 4 * pair + role by vertex, ascending
        pv = self.pairs.reshape(-1).long()
        _, code = torch.sort(pv, stable=True)
        self.pr = code.to(torch.int32).contiguous()
        n_codes = torch.bincount(pv, minlength=V)[:V] if V > 0 else torch.zeros(0, dtype=torch.long, device=dev)
        self.pr_off = self._offsets(n_codes, dev)
        self.long_verts = torch.nonzero((degree > LONG_LIST) | (n_codes > LONG_LIST)).reshape(-1).to(torch.int32).contiguous()
        self.num_vertices, self.num_edges, self.num_pairs, self.num_long = V, E, P, int(self.long_verts.shape[0])
        self.partial_rows = int(_lib.lib().gs_meshreg_partial_rows(V, E, P, self.num_long))
        self.device = dev

    @staticmethod
    def _offsets(counts: Tensor, dev) -> Tensor:
        return torch.cat((torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(counts, 0))).to(torch.int32).contiguous()


class _MeshReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, topo, target_length):
        t, L = topo, _lib
        V, E, P = t.num_vertices, t.num_edges, t.num_pairs
        dev = vertices.device
        need = ctx.needs_input_grad[0]
        terms = torch.empty(V + E + P, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(t.partial_rows, 3, dtype=torch.float64, device=dev)
        lap_dir = torch.empty(V, 3, dtype=torch.float32, device=dev) if need else None
        pair_grad = torch.empty(P, 4, 3, dtype=torch.float32, device=dev) if need else None
        L.check(L.lib().gs_meshreg_fwd(V, E, P, t.num_long, L.ptr(vertices), L.ptr(t.edges), L.ptr(t.pairs), L.ptr(t.nbr_off), L.ptr(t.nbr),
                                       L.ptr(t.pr_off), L.ptr(t.long_verts), target_length, L.ptr(terms), L.ptr(lap_dir), L.ptr(pair_grad),
                                       L.ptr(partials), L.ptr(out), L.stream()), "gs_meshreg_fwd")
        ctx.topo, ctx.target_length = t, target_length
        if need:
            ctx.save_for_backward(vertices, lap_dir, pair_grad)
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    def backward(ctx, out_grad, _terms_grad):
        vertices, lap_dir, pair_grad = ctx.saved_tensors
        t, L = ctx.topo, _lib
        grad = torch.empty_like(vertices)
        out_grad = out_grad.contiguous().float()
        L.check(L.lib().gs_meshreg_bwd(t.num_vertices, t.num_edges, t.num_pairs, t.num_long, L.ptr(vertices), L.ptr(t.nbr_off), L.ptr(t.nbr),
                                       L.ptr(t.pr_off), L.ptr(t.pr), L.ptr(t.long_verts), ctx.target_length, L.ptr(lap_dir), L.ptr(pair_grad),
                                       L.ptr(out_grad), L.ptr(grad), L.stream()), "gs_meshreg_bwd")
        return grad, None, None


def mesh_regularizers(vertices: Tensor, topo: MeshRegTopology, target_length: float = 0.0, *, return_terms: bool = False):
    """-> (lap, edge, nc): three 0-d float32 tensors, differentiable in `vertices` [V,3] (analytic gradients, csrc/gs_meshreg.hip).

      lap  = (1/V) sum_i |deg_i v_i - sum_{j in N(i)} v_j|          (V counts unused vertices; their term is 0)
      edge = (1/E) sum_e (|v_lo - v_hi| - target_length)^2
      nc   = (1/P) sum_p [1 - (n0 . -n1) / (max(|n0|, 1e-8) max(|n1|, 1e-8))],   n0 = (v1 - v0) x (a - v0), n1 = (v1 - v0) x (b - v0)

    A term without elements is 0 with a zero gradient; a zero-length vector under a norm contributes the zero subgradient.
    return_terms=True (a test and debugging keyword) also returns the per-vertex [V], per-edge [E] and per-pair [P] terms."""
    if not isinstance(topo, MeshRegTopology):
        raise ValueError("topo must be a MeshRegTopology")
    if not isinstance(vertices, Tensor) or vertices.dtype != torch.float32 or tuple(vertices.shape) != (topo.num_vertices, 3):
        raise ValueError(f"vertices must be a float32 tensor [{topo.num_vertices},3], got "
                         f"{(vertices.dtype, tuple(vertices.shape)) if isinstance(vertices, Tensor) else type(vertices).__name__}")
    _lib.require_cuda(vertices)
    if vertices.device != topo.device:
        raise ValueError(f"vertices on {vertices.device}, the topology on {topo.device}")
    out, terms = _MeshReg.apply(vertices.contiguous(), topo, float(target_length))
    values = (out[0], out[1], out[2])
    if not return_terms:
        return values
    V, E = topo.num_vertices, topo.num_edges
    return values + (terms[:V], terms[V:V + E], terms[V + E:])


def laplacian_smooth_loss(vertices: Tensor, topo: MeshRegTopology) -> Tensor:
    return mesh_regularizers(vertices, topo)[0]


def mesh_edge_loss(vertices: Tensor, topo: MeshRegTopology, target_length: float = 0.0) -> Tensor:
    return mesh_regularizers(vertices, topo, target_length)[1]


def mesh_normal_consistency(vertices: Tensor, topo: MeshRegTopology) -> Tensor:
    return mesh_regularizers(vertices, topo)[2]
