"""Ray queries against a triangle mesh (csrc/gs_bvh.hip): what the reference's OptiX stages get from ``optix_build_bvh`` and from
the shadow test inside ``optix_env_shade``.  An LBVH built on the device, an any-hit query (`occluded`), a closest-hit query, and
the brute-force form of both, which defines the semantics (include/geosplat_hip.h).  No autograd anywhere in this module: the
reference ignores the gradient of the shadow boundary on purpose (envsampling/kernel.cu:97-99), and gradients of `closest_hit` are
out of scope."""
from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from .meshrender import _faces32

__all__ = ["MeshBVH", "ray_layout", "shadow_visibility"]


def _vertices32(vertices: Tensor) -> Tensor:
    if vertices.ndim != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise _lib.GeoSplatHipError(f"vertices must be float32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}")
    return vertices.detach().contiguous()


def ray_layout(origins: Tensor, dirs: Tensor) -> Tuple[int, int, int]:
    """(P, S, dirs_per_point) of a ray batch: origins [P,3]; dirs [P,S,3], or [S,3] shared by all points (never expanded), or [P,3]
    -- one direction per origin, S = 1 (a 2-D `dirs` with as many rows as `origins` is read this way).  ValueError otherwise."""
    if origins.ndim != 2 or origins.shape[1] != 3 or origins.dtype != torch.float32:
        raise ValueError(f"origins must be float32 [P,3], got {origins.dtype} {tuple(origins.shape)}")
    P = origins.shape[0]
    if dirs.dtype == torch.float32 and dirs.shape[-1:] == (3,):
        if dirs.ndim == 3 and dirs.shape[0] == P:
            return P, dirs.shape[1], 1
        if dirs.ndim == 2 and dirs.shape[0] == P:
            return P, 1, 1
        if dirs.ndim == 2:
            return P, dirs.shape[0], 0
    raise ValueError(f"dirs must be float32 [P,S,3], [S,3] or [P,3] for origins {tuple(origins.shape)}, "
                     f"got {dirs.dtype} {tuple(dirs.shape)}")


class MeshBVH:
    """``MeshBVH(vertices, faces)`` builds the hierarchy; it keeps references to the tensors it was built from (the queries read
    the triangles through them, so do not write into them between a build and a query).  ``nodes`` is the node buffer whose layout
    include/geosplat_hip.h fixes."""

    def __init__(self, vertices: Tensor, faces: Tensor):
        if faces.ndim == 2 and faces.shape[0] == 0:
            raise ValueError(f"empty mesh: faces has shape {tuple(faces.shape)}")
        _lib.require_cuda(vertices, faces)
        self.faces = _faces32(faces.detach())
        self.vertices = _vertices32(vertices)
        if self.vertices.shape[0] == 0:
            raise ValueError(f"empty mesh: vertices has shape {tuple(vertices.shape)}")
        lib = _lib.lib()
        F = self.faces.shape[0]
        nbytes, ws_bytes = lib.gs_bvh_bytes(F), lib.gs_bvh_ws_bytes(F)
        if nbytes == 0 or ws_bytes == 0:
            raise _lib.GeoSplatHipError(f"at most 2^30 faces, got {F}")
        dev = self.vertices.device
        self.nodes = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._ws = _lib.workspace(ws_bytes, dev)
        self._build()

    @property
    def num_faces(self) -> int:
        return self.faces.shape[0]

    def _build(self) -> None:
        v, f = self.vertices, self.faces
        _lib.check(_lib.lib().gs_bvh_build(v.shape[0], f.shape[0], _lib.ptr(v), _lib.ptr(f), _lib.ptr(self.nodes), self.nodes.numel(),
                                           _lib.ptr(self._ws), self._ws.numel(), _lib.stream()), "gs_bvh_build")

    def rebuild(self, vertices: Tensor) -> "MeshBVH":
        """Same faces, moved vertices: a full rebuild into the same buffers (the reference's rebuild=1)."""
        _lib.require_cuda(vertices)
        v = _vertices32(vertices)
        if v.shape != self.vertices.shape or v.device != self.vertices.device:
            raise ValueError(f"rebuild needs vertices of shape {tuple(self.vertices.shape)} on {self.vertices.device}, "
                             f"got {tuple(v.shape)} on {v.device}")
        self.vertices = v
        self._build()
        return self

    # ---- queries ------------------------------------------------------------------------------------------------------------
    def _rays(self, origins: Tensor, dirs: Tensor):
        _lib.require_cuda(origins, dirs)
        P, S, per_point = ray_layout(origins, dirs)
        if origins.device != self.vertices.device or dirs.device != self.vertices.device:
            raise ValueError(f"rays on {origins.device} / {dirs.device}, mesh on {self.vertices.device}")
        return origins.detach().contiguous(), dirs.detach().contiguous(), P, S, per_point

    def _head(self, o: Tensor, d: Tensor, P: int, S: int, per_point: int, tmin: float, tmax: float, brute_force: bool):
        v, f = self.vertices, self.faces
        return (v.shape[0], f.shape[0], _lib.ptr(v), _lib.ptr(f), None if brute_force else _lib.ptr(self.nodes), P, S, _lib.ptr(o),
                _lib.ptr(d), per_point, float(tmin), float(tmax))

    def occluded(self, origins: Tensor, dirs: Tensor, *, tmin: float = 0.0, tmax: float = math.inf, brute_force: bool = False) -> Tensor:
        """bool [P,S]: does the ray origins[p] + t dirs[p,s] hit any face for tmin < t < tmax (both strict, both sides)?
        ``brute_force`` tests every face for every ray with the same device routine (the tests and the benchmark use it)."""
        o, d, P, S, per_point = self._rays(origins, dirs)
        out = torch.empty(P, S, dtype=torch.uint8, device=o.device)
        _lib.check(_lib.lib().gs_ray_occluded(*self._head(o, d, P, S, per_point, tmin, tmax, brute_force), _lib.ptr(out), _lib.stream()),
                   "gs_ray_occluded")
        return out.view(torch.bool)

    def closest_hit(self, origins: Tensor, dirs: Tensor, *, tmin: float = 0.0, tmax: float = math.inf,
                    brute_force: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """(t [P,S] fp32, +inf on a miss; face [P,S] int64, -1 on a miss; bary [P,S,3], weights of the face's three vertices, 0 on a
        miss).  The smallest fp32 t wins, the lower face index among equal t."""
        o, d, P, S, per_point = self._rays(origins, dirs)
        t = torch.empty(P, S, dtype=torch.float32, device=o.device)
        face = torch.empty(P, S, dtype=torch.int32, device=o.device)
        b12 = torch.empty(P, S, 2, dtype=torch.float32, device=o.device)
        _lib.check(_lib.lib().gs_ray_closest(*self._head(o, d, P, S, per_point, tmin, tmax, brute_force), _lib.ptr(t), _lib.ptr(face),
                                             _lib.ptr(b12), _lib.stream()), "gs_ray_closest")
        b0 = torch.where(face >= 0, 1.0 - b12[..., 0] - b12[..., 1], torch.zeros_like(t))
        return t, face.to(torch.int64), torch.cat([b0[..., None], b12], -1)


def shadow_visibility(bvh: MeshBVH, positions: Tensor, normals: Tensor, dirs: Tensor, *, offset: float = 1e-5,
                      shadow_scale: float = 1.0) -> Tensor:
    """The reference's shadow test as ``splat_mc`` calls it (rfstudio/model/geosplat.py:171, 308): an any-hit ray from
    ``positions + normals.detach() * offset`` towards every direction, tmin = 0, tmax = 1e16, no face culling; returns
    ``V * shadow_scale + (1 - shadow_scale)`` with V = 1 where nothing is hit, fp32 [P,S].

    There is NO gradient: the output never requires grad.  Visibility is piecewise constant in the positions and the vertices, and
    the reference leaves the gradient of the shadow boundary out on purpose (envsampling/kernel.cu:97-99, 420)."""
    _lib.require_cuda(positions, normals, dirs)
    if positions.shape != normals.shape or positions.ndim != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions and normals must both be [P,3], got {tuple(positions.shape)} and {tuple(normals.shape)}")
    with torch.no_grad():
        origins = positions.detach() + normals.detach() * offset
        occ = bvh.occluded(origins, dirs, tmin=0.0, tmax=1e16)
        vis = (~occ).to(torch.float32)
        return vis * shadow_scale + (1.0 - shadow_scale)
