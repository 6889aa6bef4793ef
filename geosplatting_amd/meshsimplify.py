"""Mesh decimation and the component filter: the "cropping and simplifying" the reference's README leaves to outside tools before its
prior flow (`PriorModel(vertices, faces)` places six Gaussians on every face), on the device (csrc/gs_simplify.hip).

  mesh_components / keep_components   connected components by min-label hooking with pointer jumping; keep the largest, those above a
                                      face count, and / or what lies inside a box
  simplify_mesh / edge_collapse_costs Garland-Heckbert quadric error metrics run as rounds of independent edge collapses

A round rebuilds the index arrays of the current faces with torch sorts (unique edges ascending by lo V + hi as in MeshRegTopology,
faces per edge, sorted neighbour lists, vertex -> face lists, boundary flags); one kernel prices and validates every edge in float64;
every valid edge claims its closed neighbourhood with a 64-bit atomic minimum of (cost bits, hashed index) and wins where it holds
both endpoints, so the winners of a round are independent, do not depend on the launch order and are applied together.  Quadrics are
carried (Q_u += Q_v), never recomputed.  include/geosplat_hip.h states the rule, tests/simplify_ref.py restates it in float64 numpy.
The host reads a few counters per round: this is a one-off preprocessing call like MeshRegTopology.  Same inputs, same bits.

Left out: no attribute / uv transfer, no gradient (a topology operation), no hole filling."""
from __future__ import annotations

import time
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib

__all__ = ["mesh_components", "keep_components", "simplify_mesh", "edge_collapse_costs"]

MAX_ITEMS = 1 << 30


def _check_faces(faces, num_vertices: int) -> Tensor:
    if not isinstance(faces, Tensor) or faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be an int32 / int64 tensor [F,3], got "
                         f"{(faces.dtype, tuple(faces.shape)) if isinstance(faces, Tensor) else type(faces).__name__}")
    V = int(num_vertices)
    if V < 0 or V > MAX_ITEMS or 3 * faces.shape[0] > MAX_ITEMS:
        raise ValueError(f"num_vertices in [0, 2^30] and at most 2^30 edges, got V = {num_vertices}, F = {faces.shape[0]}")
    _lib.require_cuda(faces)
    f = faces.long()
    if f.shape[0] > 0 and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError(f"faces index outside [0, {V}): min {int(f.min())}, max {int(f.max())}")
    return f


def _check_vertices(vertices) -> Tensor:
    if not isinstance(vertices, Tensor) or vertices.ndim != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"vertices must be a float32 tensor [V,3], got "
                         f"{(vertices.dtype, tuple(vertices.shape)) if isinstance(vertices, Tensor) else type(vertices).__name__}")
    _lib.require_cuda(vertices)
    if not bool(torch.isfinite(vertices).all()):
        raise ValueError("vertices must be finite")
    return vertices.detach().contiguous()


def _offsets(counts: Tensor) -> Tensor:
    return torch.cat((torch.zeros(1, dtype=torch.long, device=counts.device), torch.cumsum(counts, 0))).to(torch.int32).contiguous()


def _unique_edges(f: Tensor, V: int):
    """the 3F sides of `f` [F,3] int64 sorted by lo V + hi -> (sorted keys' unique values, inverse, counts, the sort order)"""
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    key, order = torch.sort(torch.minimum(a, b) * V + torch.maximum(a, b), stable=True)
    ukey, inverse, count = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    return ukey, inverse, count, order


class _Topology:
    """The index arrays of one round (include/geosplat_hip.h lists them), built with torch sorts on the device of `f`."""

    def __init__(self, f: Tensor, V: int):
        dev, F = f.device, f.shape[0]
        ukey, inverse, count, order = _unique_edges(f, V)
        E = ukey.shape[0]
        if E > MAX_ITEMS:
            raise ValueError(f"more than 2^30 edges ({E})")
        e_lo, e_hi = ukey // max(V, 1), ukey % max(V, 1)
        self.edges = torch.stack((e_lo, e_hi), dim=1).to(torch.int32).contiguous()
        self.edge_faces = count.to(torch.int32)
        # the vertices opposite to an edge in its first two faces (a stable sort keeps the faces of an edge ascending)
        opp = f[:, [2, 0, 1]].reshape(-1)[order]
        start = torch.cumsum(count, 0) - count
        edge_opp = torch.full((E, 2), -1, dtype=torch.long, device=dev)
        if E > 0:
            edge_opp[:, 0] = opp[start]
            two = count >= 2
            edge_opp[two, 1] = opp[start[two] + 1]
        self.edge_opp = edge_opp.to(torch.int32).contiguous()
        one_face = count == 1
        side_boundary = torch.empty(3 * F, dtype=torch.uint8, device=dev)
        side_boundary[order] = one_face[inverse].to(torch.uint8)
        self.side_boundary = side_boundary
        boundary = torch.zeros(V, dtype=torch.uint8, device=dev)
        boundary[e_lo[one_face]] = 1
        boundary[e_hi[one_face]] = 1
        self.boundary = boundary
        # neighbour lists: both directions of every edge, by (vertex, neighbour)
        src, dst = torch.cat((e_lo, e_hi)), torch.cat((e_hi, e_lo))
        nkey, _ = torch.sort(src * V + dst)
        self.nbr = (nkey % max(V, 1)).to(torch.int32).contiguous()
        self.nbr_off = _offsets(torch.bincount(src, minlength=V)[:V] if V > 0 else torch.zeros(0, dtype=torch.long, device=dev))
        # vertex -> face lists, the faces of a vertex ascending
        corner = f.reshape(-1)
        _, corder = torch.sort(corner, stable=True)
        self.vf = (corder // 3).to(torch.int32).contiguous()
        self.vf_off = _offsets(torch.bincount(corner, minlength=V)[:V] if V > 0 else torch.zeros(0, dtype=torch.long, device=dev))
        self.faces = f.to(torch.int32).contiguous()
        self.V, self.E, self.F = V, E, F


def _quadrics(vertices: Tensor, t: _Topology, boundary_weight: float) -> Tensor:
    Q = torch.empty(t.V, 10, dtype=torch.float64, device=vertices.device)
    L = _lib
    L.check(L.lib().gs_simplify_quadrics(t.V, t.F, L.ptr(vertices), L.ptr(t.faces), L.ptr(t.vf_off), L.ptr(t.vf), L.ptr(t.side_boundary),
                                         float(boundary_weight), L.ptr(Q), L.stream()), "gs_simplify_quadrics")
    return Q


def _edge_costs(vertices: Tensor, Q: Tensor, t: _Topology, min_normal_dot: float):
    dev, E, L = vertices.device, t.E, _lib
    position = torch.empty(E, 3, dtype=torch.float32, device=dev)
    cost = torch.empty(E, dtype=torch.float32, device=dev)
    valid = torch.empty(E, dtype=torch.uint8, device=dev)
    key = torch.empty(E, dtype=torch.int64, device=dev)
    L.check(L.lib().gs_simplify_edge_costs(t.V, E, L.ptr(vertices), L.ptr(Q), L.ptr(t.faces), L.ptr(t.edges), L.ptr(t.edge_faces), L.ptr(t.edge_opp),
                                           L.ptr(t.nbr_off), L.ptr(t.nbr), L.ptr(t.vf_off), L.ptr(t.vf), L.ptr(t.boundary), float(min_normal_dot),
                                           L.ptr(position), L.ptr(cost), L.ptr(valid), L.ptr(key), L.stream()), "gs_simplify_edge_costs")
    return position, cost, valid, key


def _check_options(boundary_weight: float, min_normal_dot: float) -> None:
    if not (0.0 <= float(boundary_weight) < float("inf")):
        raise ValueError(f"boundary_weight must be finite and >= 0, got {boundary_weight}")
    if not (-1.0 <= float(min_normal_dot) < 1.0):
        raise ValueError(f"min_normal_dot must be in [-1, 1), got {min_normal_dot}")


def _drop_repeats(f: Tensor) -> Tensor:
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]


@torch.no_grad()
def edge_collapse_costs(vertices: Tensor, faces: Tensor, *, boundary_weight: float = 1000.0, min_normal_dot: float = 0.2):
    """Round 0's per-edge kernel of simplify_mesh -> (edges [E,2] int32, cost [E] fp32, position [E,3] fp32, valid [E] bool,
    key [E] int64): the unique edges ascending by lo V + hi, the quadric cost of collapsing each and where the merged vertex would
    go, whether the collapse is allowed, and the selection key (cost bits << 32 | hashed edge index)."""
    v = _check_vertices(vertices)
    f = _drop_repeats(_check_faces(faces, v.shape[0]))
    if f.device != v.device:
        raise ValueError(f"vertices on {v.device}, faces on {f.device}")
    _check_options(boundary_weight, min_normal_dot)
    t = _Topology(f, v.shape[0])
    position, cost, valid, key = _edge_costs(v, _quadrics(v, t, boundary_weight), t, min_normal_dot)
    return t.edges, cost, position, valid.bool(), key


@torch.no_grad()
def simplify_mesh(vertices: Tensor, faces: Tensor, target_faces: int, *, boundary_weight: float = 1000.0, min_normal_dot: float = 0.2,
                  max_rounds: int = 4096, return_info: bool = False, _timing: Optional[list] = None):
    """Decimate to `target_faces` -> (vertices' [V',3] fp32, faces' [F',3] int64, vertex_map [V_in] int64), plus info with
    return_info=True.  No gradient.

    Rounds of independent quadric edge collapses (the module docstring; include/geosplat_hip.h states the per-edge rule).  In a round
    the winners are applied in ascending key order while the faces they remove stay within F - target_faces (the single cheapest if
    that takes none), so it ends at target_faces or target_faces - 1; it also ends when a round has no winner (info['stalled'], the
    mesh returned as it is) or after max_rounds.  Unused vertices are dropped at the end; vertex_map follows every input vertex
    through the merges to its output index, -1 if that vertex is unused.  A face that repeats an index is dropped on entry; duplicate
    faces and edges with three or more faces are legal and never collapse.
    info: rounds, stalled, per_round = [(edges, valid, winners, applied), ...].  (_timing: a list that scripts/simplify_bench.py
    passes to get (topology ms, kernel ms, apply ms) per round, each part closed by a device wait.)"""
    v = _check_vertices(vertices)
    V = v.shape[0]
    f = _drop_repeats(_check_faces(faces, V))
    if f.device != v.device:
        raise ValueError(f"vertices on {v.device}, faces on {f.device}")
    if int(target_faces) < 1:
        raise ValueError(f"target_faces must be at least 1, got {target_faces}")
    _check_options(boundary_weight, min_normal_dot)
    target, max_rounds = int(target_faces), int(max_rounds)
    dev, L = v.device, _lib
    v = v.clone()
    rep = torch.arange(V, device=dev)
    info = {"rounds": 0, "stalled": False, "per_round": []}
    Q = None
    claim = torch.empty(V, dtype=torch.int64, device=dev)

    def lap(marks):
        if _timing is not None:
            torch.cuda.synchronize(dev)
            marks.append(time.perf_counter())

    while f.shape[0] > target and info["rounds"] < max_rounds:            # at most max_rounds trips
        marks = []
        lap(marks)
        t = _Topology(f, V)
        lap(marks)
        if Q is None:
            Q = _quadrics(v, t, boundary_weight)
        position, _, valid, key = _edge_costs(v, Q, t, min_normal_dot)
        winner = torch.empty(t.E, dtype=torch.uint8, device=dev)
        L.check(L.lib().gs_simplify_select(V, t.E, L.ptr(t.edges), L.ptr(valid), L.ptr(key), L.ptr(t.nbr_off), L.ptr(t.nbr), L.ptr(claim),
                                           L.ptr(winner), L.stream()), "gs_simplify_select")
        info["rounds"] += 1
        lap(marks)
        win = torch.nonzero(winner).reshape(-1)
        n_valid = int(valid.sum())
        if win.shape[0] == 0:
            info["stalled"] = True
            info["per_round"].append((t.E, n_valid, 0, 0))
            break
        # keys of non-negative costs are below 2^63: their order as int64 is their order as unsigned integers
        _, order = torch.sort(key[win])
        win = win[order]
        removed = torch.cumsum(t.edge_faces[win].long(), 0)
        n_apply = max(int((removed <= f.shape[0] - target).sum()), 1)
        selected = win[:n_apply].contiguous()
        remap = torch.arange(V, device=dev)
        L.check(L.lib().gs_simplify_apply(V, t.E, n_apply, L.ptr(selected), L.ptr(t.edges), L.ptr(position), L.ptr(v), L.ptr(Q), L.ptr(remap),
                                          L.stream()), "gs_simplify_apply")
        rep = remap[rep]
        f = _drop_repeats(remap[f])
        info["per_round"].append((t.E, n_valid, int(win.shape[0]), n_apply))
        lap(marks)
        if _timing is not None:
            _timing.append(tuple(1e3 * (b - a) for a, b in zip(marks, marks[1:])))
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[f.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    vertex_map = torch.where(used[rep], new[rep], torch.full_like(rep, -1))
    out = (v[used].contiguous(), new[f].contiguous(), vertex_map)
    return out + (info,) if return_info else out


@torch.no_grad()
def mesh_components(faces: Tensor, num_vertices: int):
    """-> (vertex_label [V] int32, face_label [F] int32, info): two vertices are in one component when a chain of faces that share a
    vertex index connects them; the label is the smallest vertex index of the component, -1 for a vertex no face uses.
    Min-label hooking over the unique edges with pointer jumping (gs_components_step), repeated until the device flag says nothing
    changed; info['iterations'] counts the passes (the last one changes nothing)."""
    f = _check_faces(faces, num_vertices)
    V, dev, L = int(num_vertices), f.device, _lib
    ukey, _, _, _ = _unique_edges(f, V)
    E = ukey.shape[0]
    if E > MAX_ITEMS:
        raise ValueError(f"more than 2^30 edges ({E})")
    edges = torch.stack((ukey // max(V, 1), ukey % max(V, 1)), dim=1).to(torch.int32).contiguous()
    parent = torch.arange(V, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    iterations = 0
    while True:                                                             # every pass but the last lowers a parent: at most V + 1
        if iterations > V:
            raise RuntimeError(f"mesh_components did not settle in {V} + 1 passes")
        L.check(L.lib().gs_components_step(V, E, L.ptr(edges), L.ptr(parent), L.ptr(changed), L.stream()), "gs_components_step")
        iterations += 1
        if int(changed.item()) == 0:
            break
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[f.reshape(-1)] = True
    vertex_label = torch.where(used, parent, torch.full_like(parent, -1))
    face_label = vertex_label[f[:, 0]] if f.shape[0] > 0 else torch.zeros(0, dtype=torch.int32, device=dev)
    return vertex_label, face_label.contiguous(), {"iterations": iterations, "edges": E}


@torch.no_grad()
def keep_components(vertices: Tensor, faces: Tensor, *, largest: Optional[int] = None, min_faces: Optional[int] = None,
                    bounds=None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (vertices', faces' int64, vertex_map [V_in] int64: the new index or -1).  First drops the faces with a vertex outside
    bounds = ((x0, y0, z0), (x1, y1, z1)) (the cropping), then keeps the `largest` components by face count (ties go to the smaller
    label) and / or those with at least `min_faces` faces; the vertices are compacted in ascending old index."""
    v = _check_vertices(vertices)
    V = v.shape[0]
    f = _check_faces(faces, V)
    if f.device != v.device:
        raise ValueError(f"vertices on {v.device}, faces on {f.device}")
    if largest is not None and int(largest) < 1:
        raise ValueError(f"largest must be at least 1, got {largest}")
    if min_faces is not None and int(min_faces) < 0:
        raise ValueError(f"min_faces must not be negative, got {min_faces}")
    dev = v.device
    if bounds is not None:
        lo, hi = (torch.tensor([float(c) for c in b], dtype=torch.float32, device=dev) for b in bounds)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("bounds must be ((x0, y0, z0), (x1, y1, z1))")
        inside = ((v >= lo) & (v <= hi)).all(dim=1)
        f = f[inside[f].all(dim=1)]
    if (largest is not None or min_faces is not None) and f.shape[0] > 0:
        _, face_label, _ = mesh_components(f, V)
        count = torch.bincount(face_label.long(), minlength=V)              # faces per label
        keep = count > 0
        if min_faces is not None:
            keep &= count >= int(min_faces)
        if largest is not None:
            order = torch.sort(count, descending=True, stable=True).indices[:int(largest)]      # ties: the smaller label first
            top = torch.zeros(V, dtype=torch.bool, device=dev)
            top[order] = True
            keep &= top
        f = f[keep[face_label.long()]]
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[f.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    vertex_map = torch.where(used, new, torch.full_like(new, -1))
    return v[used].contiguous(), new[f].contiguous(), vertex_map
