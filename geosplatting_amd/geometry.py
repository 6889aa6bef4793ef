"""Geometry metrics between meshes and point sets (csrc/gs_nn.hip): the number the reference reports for an extracted mesh.

  PointGrid / k_nearest / k_nearest_in   == Points.k_nearest / k_nearest_in (rfstudio/graphics/_points.py:38-67), on the device
  chamfer_distance                       == ChamferDistance (rfstudio/loss/_chamfer): squared distances both ways, differentiable
  sample_mesh_surface                    == TriangleMesh.uniformly_sample (rfstudio/graphics/_mesh/_triangle_mesh.py:768-859)
  chamfer / chamfer_fscore               == ChamferDistanceMetric / ChamferDistanceFscoreMetric (rfstudio/loss/geometric_loss.py)

The search is exact: include/geosplat_hip.h fixes the fp32 distance to the bit, the tie rule (lowest index among equal distances) and
what happens to non-finite rows, and the grid search returns what the brute-force form returns.  There is no ``Points`` class here:
point sets are plain ``[N,3]`` tensors and meshes are ``(vertices, faces)`` pairs."""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib

__all__ = ["PointGrid", "k_nearest", "k_nearest_in", "chamfer_distance", "sample_mesh_surface", "chamfer", "chamfer_fscore",
           "fscore_from_distances"]

MAX_K = 8
MeshOrPoints = Union[Tensor, Tuple[Tensor, Tensor]]


def _points32(points: Tensor, what: str = "points") -> Tensor:
    if points.ndim != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise _lib.GeoSplatHipError(f"{what} must be float32 [N,3], got {points.dtype} {tuple(points.shape)}")
    return points.detach().contiguous()


class PointGrid:
    """``PointGrid(points)`` builds a uniform grid over the finite rows of ``points`` [M,3]; it keeps a reference to the tensor it
    was built from (the brute-force form reads the points through it).  ``grid`` is the opaque buffer of include/geosplat_hip.h."""

    def __init__(self, points: Tensor):
        if points.ndim == 2 and points.shape[0] == 0:
            raise ValueError(f"empty point set: points has shape {tuple(points.shape)}")
        _lib.require_cuda(points)
        self.points = _points32(points)
        lib = _lib.lib()
        M = self.points.shape[0]
        nbytes, ws_bytes = lib.gs_nn_grid_bytes(M), lib.gs_nn_ws_bytes(M)
        if nbytes == 0 or ws_bytes == 0:
            raise _lib.GeoSplatHipError(f"at most 2^30 points, got {M}")
        dev = self.points.device
        self.grid = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._ws = _lib.workspace(ws_bytes, dev)
        self._build()

    @property
    def num_points(self) -> int:
        return self.points.shape[0]

    def _build(self) -> None:
        p = self.points
        _lib.check(_lib.lib().gs_nn_build(p.shape[0], _lib.ptr(p), _lib.ptr(self.grid), self.grid.numel(), _lib.ptr(self._ws),
                                          self._ws.numel(), _lib.stream()), "gs_nn_build")

    def rebuild(self, points: Tensor) -> "PointGrid":
        """As many points, moved: a full rebuild into the same buffers."""
        _lib.require_cuda(points)
        p = _points32(points)
        if p.shape != self.points.shape or p.device != self.points.device:
            raise ValueError(f"rebuild needs points of shape {tuple(self.points.shape)} on {self.points.device}, "
                             f"got {tuple(p.shape)} on {p.device}")
        self.points = p
        self._build()
        return self

    def k_nearest(self, queries: Tensor, k: int, brute_force: bool = False) -> Tuple[Tensor, Tensor]:
        """(d [N,k] fp32, idx [N,k] int32): the k smallest (squared distance, index) pairs of every query in ascending order, padded
        with (+inf, -1); 1 <= k <= 8.  ``brute_force`` meets every point with the same device routine and gives the same bits."""
        _lib.require_cuda(queries)
        q = _points32(queries, "queries")
        if q.device != self.points.device:
            raise ValueError(f"queries on {q.device}, points on {self.points.device}")
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        N, k = q.shape[0], int(k)
        d = torch.empty(N, k, dtype=torch.float32, device=q.device)
        idx = torch.empty(N, k, dtype=torch.int32, device=q.device)
        p = self.points
        _lib.check(_lib.lib().gs_nn_query(p.shape[0], _lib.ptr(p), None if brute_force else _lib.ptr(self.grid), N, _lib.ptr(q), k,
                                          _lib.ptr(d), _lib.ptr(idx), _lib.stream()), "gs_nn_query")
        return d, idx

    def nearest(self, queries: Tensor, brute_force: bool = False) -> Tuple[Tensor, Tensor]:
        """(d [N] fp32, idx [N] int32): squared distance to, and index of, the nearest point; (+inf, -1) for a non-finite query or a
        set without a finite point."""
        d, idx = self.k_nearest(queries, 1, brute_force)
        return d[:, 0], idx[:, 0]


def k_nearest_in(points: Tensor, queries: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """Points.k_nearest_in(queries, k=k) of the reference: for every row of ``points`` its k nearest rows of ``queries`` (the set
    that is searched), as (distances [N,k] fp32, indices [N,k] int32).  DISTANCES, not squares: the square root is taken here."""
    d, idx = PointGrid(queries).k_nearest(points, k)
    return d.sqrt(), idx


def k_nearest(points: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """Points.k_nearest(k=k) of the reference: k + 1 neighbours of every point in the set itself, the first column dropped (the
    point itself, or a duplicate of it with a lower index); 1 <= k <= 7.  DISTANCES, not squares: the square root is taken here."""
    if not 1 <= int(k) <= MAX_K - 1:
        raise ValueError(f"k must be in [1, {MAX_K - 1}], got {k}")
    d, idx = PointGrid(points).k_nearest(points, int(k) + 1)
    return d[:, 1:].sqrt(), idx[:, 1:].contiguous()


# ---- Chamfer distance ------------------------------------------------------------------------------------------------------------
class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1: Tensor, xyz2: Tensor):
        a, b = _points32(xyz1, "xyz1"), _points32(xyz2, "xyz2")
        dist1, idx1 = PointGrid(b).nearest(a)
        dist2, idx2 = PointGrid(a).nearest(b)
        ctx.save_for_backward(a, b, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, grad1, grad2, _g3, _g4):
        a, b, idx1, idx2 = ctx.saved_tensors
        g1 = torch.zeros_like(idx1, dtype=torch.float32) if grad1 is None else grad1.float().contiguous()
        g2 = torch.zeros_like(idx2, dtype=torch.float32) if grad2 is None else grad2.float().contiguous()
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        _lib.check(_lib.lib().gs_chamfer_bwd(a.shape[0], b.shape[0], _lib.ptr(a), _lib.ptr(b), _lib.ptr(idx1), _lib.ptr(idx2),
                                             _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(ga), _lib.ptr(gb), _lib.stream()), "gs_chamfer_bwd")
        return ga, gb


def chamfer_distance(xyz1: Tensor, xyz2: Tensor, return_indices: bool = False):
    """ChamferDistance()(xyz1, xyz2) of the reference: (dist1, dist2), the SQUARED distance of every row of xyz1 to its nearest row
    of xyz2 and the other way round, for [N,3] and [M,3] or [B,N,3] and [B,M,3].  Differentiable in both inputs at the indices of
    the forward.  ``return_indices`` adds (idx1, idx2), int32, -1 where there is no neighbour (such rows get no gradient)."""
    _lib.require_cuda(xyz1, xyz2)
    if xyz1.ndim != xyz2.ndim or xyz1.ndim not in (2, 3) or xyz1.shape[-1] != 3 or xyz2.shape[-1] != 3 or \
            (xyz1.ndim == 3 and xyz1.shape[0] != xyz2.shape[0]):
        raise ValueError(f"xyz1 and xyz2 must be [N,3] and [M,3] or [B,N,3] and [B,M,3], got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}")
    if xyz1.shape[-2] == 0 or xyz2.shape[-2] == 0:
        raise ValueError(f"empty point set: {tuple(xyz1.shape)} and {tuple(xyz2.shape)}")
    if xyz1.ndim == 2:
        out = _Chamfer.apply(xyz1, xyz2)
    else:
        rows = [_Chamfer.apply(xyz1[b], xyz2[b]) for b in range(xyz1.shape[0])]
        out = tuple(torch.stack([r[i] for r in rows]) for i in range(4))
    return out if return_indices else out[:2]


# ---- surface sampling ------------------------------------------------------------------------------------------------------------
_PLASTIC = 1.3247179572447460259609088            # the plastic number: the R2 sequence steps by 1 / g and 1 / g^2


def _draw(weights: Tensor, n: int, generator: Optional[torch.Generator]) -> Tensor:
    """n indices drawn with replacement in proportion to ``weights`` (a categorical distribution over the faces)"""
    return torch.multinomial(weights / weights.sum(), n, replacement=True, generator=generator)


def _faces_of_samples(share: Tensor, total: int, mode: str, generator: Optional[torch.Generator]) -> Tensor:
    """face index of every sample, [total], for per-face probabilities ``share`` [F]"""
    if mode == "random":
        return _draw(share, total, generator)
    if mode not in ("uniform", "uniform+nonzero"):
        raise ValueError("samples_per_face must be 'random', 'uniform' or 'uniform+nonzero'")
    expected = share * total
    whole = expected.floor().long()                                              # every face gets the whole part of its expectation
    if mode == "uniform+nonzero" and bool((whole == 0).any()):
        needed = int((1 / share.min()).ceil().long().item())
        raise RuntimeError(f"samples_per_face='uniform+nonzero': with num_samples = {total} some face gets no sample; "
                           f"at least {needed} samples are needed")
    leftover = total - int(whole.sum().item())
    face_of = torch.arange(share.shape[0], device=share.device).repeat_interleave(whole)
    if leftover > 0:                                                             # ... and the rest is drawn over the fractional parts
        face_of = torch.cat((face_of, _draw(expected - whole, leftover, generator)))
    return face_of


def _barycentric_weights(total: int, mode: str, device, generator: Optional[torch.Generator]) -> Tensor:
    """[total, 3] weights of the three corners, non-negative, summing to one"""
    if mode == "random":
        s = torch.rand(total, device=device, generator=generator)
        t = torch.rand(total, device=device, generator=generator).sqrt()         # the square-root warp: uniform in area
        return torch.stack((t * (1 - s), s * t, 1 - t), dim=-1)
    if mode == "r2":
        n = torch.arange(total, device=device)
        s, t = (n / _PLASTIC).frac(), (n / (_PLASTIC * _PLASTIC)).frac()          # fp32, as in the reference
        outside = s + t > 1                                                      # fold the far half of the unit square back
        s, t = torch.where(outside, 1 - s, s), torch.where(outside, 1 - t, t)
        return torch.stack((s, t, 1 - s - t), dim=-1)
    raise ValueError("samples_in_face must be 'random' or 'r2'")


def sample_mesh_surface(vertices: Tensor, faces: Tensor, num_samples: int, *, samples_per_face: str = "random",
                        samples_in_face: str = "random", probs_per_face: str = "area",
                        generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """TriangleMesh.uniformly_sample of the reference as torch ops: (positions [S,3], unit normals [S,3]).

    samples_per_face: 'random' draws every sample's face from the face probabilities; 'uniform' gives face f floor(p_f S) samples
    and draws the remaining ones from the fractional parts; 'uniform+nonzero' is 'uniform' and raises RuntimeError when some face
    would get floor(p_f S) = 0.  probs_per_face: 'area', or 'uniform' (1 / F + 1e-12, only with the two uniform modes).
    samples_in_face: 'random' (u, sqrt(v) warp) or 'r2' (the fp32 R2 sequence, deterministic).  The positions are differentiable in
    ``vertices`` through the barycentric weights; the face choice and the normals are not.  Every random draw comes from
    ``generator`` (a generator of the vertices' device), unlike the reference, which uses the global one."""
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"vertices [V,3] and faces [F,3] expected, got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    num_faces, total = faces.shape[0], int(num_samples)
    corners = vertices[faces.long()]                                            # [F,3,3]
    fixed = corners.detach()
    normal = torch.cross(fixed[:, 1] - fixed[:, 0], fixed[:, 2] - fixed[:, 0], dim=-1)
    twice_area = normal.norm(dim=-1)
    if probs_per_face == "area":
        share = twice_area / twice_area.sum(-1, keepdim=True)
    elif probs_per_face == "uniform" and samples_per_face in ("uniform", "uniform+nonzero"):
        share = torch.full_like(twice_area, 1.0 / num_faces + 1e-12)
    else:
        raise ValueError("probs_per_face must be 'area', or 'uniform' together with samples_per_face 'uniform' / 'uniform+nonzero'")
    face_of = _faces_of_samples(share, total, samples_per_face, generator)
    weights = _barycentric_weights(total, samples_in_face, vertices.device, generator).to(vertices.dtype)
    positions = (corners[face_of] * weights[:, :, None]).sum(-2)
    unit = (normal / twice_area[:, None])[face_of]  # the reference blends three copies of the face normal with the weights: the same direction
    return positions, unit / unit.norm(dim=-1, keepdim=True)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def _as_points(x: MeshOrPoints, target_num_points: Optional[int], generator: Optional[torch.Generator]) -> Tensor:
    if isinstance(x, Tensor):
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"a point set must be [N,3], got {tuple(x.shape)}")
        return x
    if isinstance(x, (tuple, list)) and len(x) == 2:
        vertices, faces = x
        n = max(faces.shape[0] * 10, 100000) if target_num_points is None else int(target_num_points)
        return sample_mesh_surface(vertices, faces, n, samples_per_face="uniform", generator=generator)[0]
    raise TypeError(f"a (vertices, faces) pair or a point tensor expected, got {type(x).__name__}")


def fscore_from_distances(dist_ab: Tensor, dist_ba: Tensor, threshold: float = 0.001) -> Tuple[Tensor, Tensor]:
    """(chamfer, fscore) from the two SQUARED distance vectors: chamfer = mean(dist_ab) + mean(dist_ba); precision p = mean(dist <
    threshold) each way, fscore = 2 p_ab p_ba / clamp(p_ab + p_ba, 1e-10).  The two means of the distances are accumulated in float64."""
    p_ab = (dist_ab < threshold).float().mean()
    p_ba = (dist_ba < threshold).float().mean()
    fscore = 2 * p_ab * p_ba / (p_ab + p_ba).clamp(min=1e-10)
    return _chamfer_of(dist_ab, dist_ba), fscore


def _chamfer_of(dist_ab: Tensor, dist_ba: Tensor) -> Tensor:
    """mean(dist_ab) + mean(dist_ba), accumulated in float64 and rounded to float32 ONCE: the value does not depend on the order in
    which a reduction adds a million terms (the reference's float32 means do)."""
    return (dist_ab.double().mean() + dist_ba.double().mean()).to(dist_ab.dtype)


def chamfer_fscore(a: MeshOrPoints, b: MeshOrPoints, *, threshold: float = 0.001, target_num_points: Optional[int] = None,
                   generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """ChamferDistanceFscoreMetric(threshold, target_num_points)(a, b) of the reference: (chamfer, fscore), two scalars.  ``a`` and
    ``b`` are each a (vertices, faces) pair -- sampled with samples_per_face='uniform' to max(10 F, 100 000) points, or to
    target_num_points -- or an [N,3] point tensor.  The threshold applies to the SQUARED distance, as there."""
    pa, pb = _as_points(a, target_num_points, generator), _as_points(b, target_num_points, generator)
    dist_ab, dist_ba = chamfer_distance(pa.float(), pb.float())
    return fscore_from_distances(dist_ab, dist_ba, threshold)


def chamfer(a: MeshOrPoints, b: MeshOrPoints, *, target_num_points: Optional[int] = None,
            generator: Optional[torch.Generator] = None) -> Tensor:
    """ChamferDistanceMetric(target_num_points)(a, b) of the reference: mean(dist_ab) + mean(dist_ba) over squared distances."""
    pa, pb = _as_points(a, target_num_points, generator), _as_points(b, target_num_points, generator)
    dist_ab, dist_ba = chamfer_distance(pa.float(), pb.float())
    return _chamfer_of(dist_ab, dist_ba)
