"""Ambient occlusion for the mesh shaders (csrc/gs_ao.hip): the per-face visibility behind ``PBRShader(occlusion_type='ao')`` of the
reference (rfstudio/graphics/shaders.py:92-94).  include/geosplat_hip.h states it sample by sample; tests/ao_ref.py restates it in
float64.  (The screen-space map of ``occlusion_type='ssao'`` / ``SSAOShader`` is not provided: INTEGRATION.md section 1d.)

  ambient_occlusion(bvh, positions, normals, targets=None, *, offset, brute_force, lanes, return_samples) -> [P]
      cosine-weighted visibility of points towards a shared set of target points: one shadow segment per (point, target) on a
      `MeshBVH`.  ``targets=None``: the eyes of ``sphere_cameras(128, 3.0, ..., up=(0, 0, 1))`` under a fixed seed.
  face_ambient_occlusion(vertices, faces, bvh=None, targets=None, ...) -> [F]
      the same at the face centroids with the unit face normals: the role of ``TriangleMesh.compute_ambient_occlusion``
      (rfstudio/graphics/_mesh/_triangle_mesh.py:616-678), whose 128 cameras are the targets.  Against it: rays instead of 128
      depth-peeled views of 1024^2 (no pixel quantisation), its depth tolerance of 0.02 becomes ``offset`` along the normal, and
      back-facing targets are left out where the reference counts them as occluded with weight 1e-4.

Nothing here has a gradient: the reference's ``compute_ambient_occlusion`` is ``no_grad`` and the map is piecewise constant in the
geometry.  Every op raises GeoSplatHipError on CPU tensors; there is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib
from .cameras import sphere_cameras
from .raytrace import MeshBVH

__all__ = ["ambient_occlusion", "face_ambient_occlusion", "default_ao_targets", "AO_MAX_TARGETS"]

AO_MAX_TARGETS = 4096
AO_TARGET_SEED = 0

_target_cache: Dict[str, Tensor] = {}


def default_ao_targets(device) -> Tensor:
    """[128,3]: the eyes of ``sphere_cameras(128, 3.0, 1024, 1024, up=(0, 0, 1))`` with the generator seeded by AO_TARGET_SEED (the
    reference draws its 128 cameras afresh on every call); one tensor per device."""
    key = str(torch.device(device))
    if key not in _target_cache:
        cams = sphere_cameras(128, 3.0, 1024, 1024, up=(0.0, 0.0, 1.0), generator=torch.Generator().manual_seed(AO_TARGET_SEED))
        _target_cache[key] = torch.stack([c.c2w[:, 3] for c in cams]).float().contiguous().to(device)
    return _target_cache[key]


def _rows3(name: str, t: Tensor) -> Tensor:
    if not isinstance(t, Tensor) or t.ndim != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 [N,3], got "
                         f"{(t.dtype, tuple(t.shape)) if isinstance(t, Tensor) else type(t).__name__}")
    return t.detach().contiguous()


def ambient_occlusion(bvh: MeshBVH, positions: Tensor, normals: Tensor, targets: Optional[Tensor] = None, *, offset: float = 1e-3,
                      brute_force: bool = False, lanes: Optional[int] = None, return_samples: bool = False):
    """-> vis [P] float32 in [0, 1]: sum of max(c, 1e-4) over the unoccluded front-facing targets by the sum over all front-facing
    ones, c the cosine between the normal and the direction to the target from ``positions + normals * offset`` (module docstring;
    include/geosplat_hip.h).  ``targets`` [S,3] with 1 <= S <= 4096.  ``lanes`` (None, 1, 16 or 64) lanes share a point: the order of
    the sums only.  ``brute_force`` tests every face (the same bits).  ``return_samples=True`` -> (vis, hit bool [P,S], w [P,S])."""
    if not isinstance(bvh, MeshBVH):
        raise TypeError(f"bvh must be a MeshBVH, got {type(bvh).__name__}")
    pos, nrm = _rows3("positions", positions), _rows3("normals", normals)
    if pos.shape != nrm.shape:
        raise ValueError(f"positions and normals must share [P,3], got {tuple(pos.shape)} and {tuple(nrm.shape)}")
    if targets is not None:
        tg = _rows3("targets", targets)
        if not 1 <= tg.shape[0] <= AO_MAX_TARGETS:
            raise ValueError(f"targets must hold 1..{AO_MAX_TARGETS} points, got {tg.shape[0]}")
    if lanes not in (None, 1, 16, 64):
        raise ValueError(f"lanes must be None, 1, 16 or 64, got {lanes!r}")
    _lib.require_cuda(pos, nrm, targets)
    tg = default_ao_targets(pos.device) if targets is None else tg
    dev = bvh.vertices.device
    if pos.device != dev or nrm.device != dev or tg.device != dev:
        raise ValueError(f"points on {pos.device}, targets on {tg.device}, mesh on {dev}")
    P, S = pos.shape[0], tg.shape[0]
    vis = torch.empty(P, dtype=torch.float32, device=dev)
    hit = torch.zeros(P, S, dtype=torch.uint8, device=dev) if return_samples else None
    w = torch.zeros(P, S, dtype=torch.float32, device=dev) if return_samples else None
    v, f = bvh.vertices, bvh.faces
    _lib.check(_lib.lib().gs_ray_ao(v.shape[0], f.shape[0], _lib.ptr(v), _lib.ptr(f), None if brute_force else _lib.ptr(bvh.nodes), P,
                                    _lib.ptr(pos), _lib.ptr(nrm), S, _lib.ptr(tg), float(offset), int(lanes or 0), _lib.ptr(vis),
                                    _lib.ptr(hit), _lib.ptr(w), _lib.stream()), "gs_ray_ao")
    return (vis, hit.view(torch.bool), w) if return_samples else vis


def face_ambient_occlusion(vertices: Tensor, faces: Tensor, bvh: Optional[MeshBVH] = None, targets: Optional[Tensor] = None, *,
                           offset: float = 1e-3, brute_force: bool = False, lanes: Optional[int] = None) -> Tensor:
    """-> [F]: `ambient_occlusion` at the face centroids with the unit face normals ((0, 0, 1) for a face without area) -- what
    ``TriangleMesh.compute_ambient_occlusion`` is for.  ``bvh``: a `MeshBVH` of this mesh, built here when None."""
    _lib.require_cuda(vertices, faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"vertices must be [V,3] and faces [F,3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    with torch.no_grad():
        v = vertices.detach().float().contiguous()
        if bvh is None:
            bvh = MeshBVH(v, faces)
        elif bvh.num_faces != faces.shape[0]:
            raise ValueError(f"bvh was built for {bvh.num_faces} faces, the mesh has {faces.shape[0]}")
        fl = faces.to(torch.int64)
        a, b, c = v[fl[:, 0]], v[fl[:, 1]], v[fl[:, 2]]
        from .meshrender import _unit_or_z
        normals = _unit_or_z(torch.cross(b - a, c - a, dim=-1))
        centroids = (a + b + c) / 3.0
        return ambient_occlusion(bvh, centroids.contiguous(), normals.contiguous(), targets, offset=offset, brute_force=brute_force,
                                 lanes=lanes)
