"""Differentiable Poisson surface reconstruction from oriented points (Shape-as-Points): `TriangleMesh.from_diff_poisson_reconstruction`
(rfstudio/graphics/_mesh/_triangle_mesh.py:301-319) and the `_mesh/_dpsr` package behind it.  Oriented points become a periodic
indicator grid by a spectral Poisson solve, the zero level set becomes a mesh, and a gradient runs from the mesh vertices back to
the points.  The one mesh constructor that needs no cameras and no renders.

  splat_to_grid(points01, values, resolution)        point_rasterize: periodic trilinear scatter -> [C,R0,R1,R2]   (gs_grid_splat)
  sample_grid(grid, points01)                        grid_interp: the adjoint gather -> [N,C]                      (gs_grid_sample_fwd)
  poisson_indicator(points01, normals, resolution, smoothness, shift=True, scale=True)
                                                     DPSR.forward for one batch -> phi [R0,R1,R2]
  mesh_from_indicator(phi, lo=-1.25, hi=1.25)        PSR2Mesh: marching cubes at level 0 -> (vertices, faces, vertex_normals)
  diff_poisson_surface_recon(points, normals, *, smoothness, resolution)
  mesh_from_oriented_points(points, normals, resolution=512, smoothness=0.02)
  remesh_poisson(vertices, faces, resolution=256, smoothness=0.02)
                                                     the reference's Mesh2Mesh task: closes a TSDF mesh before PriorModel

What runs where: the splat, the sample, their gradients, the Fourier-space step (filter, -i omega, regularised Laplacian, DC),
the hand-off to marching cubes and the vertex normals are csrc/gs_poisson.hip; the triangulation is gs_tsdf_extract_*.  The FFTs
are torch.fft (hipFFT); the shift / scale step (one mean, one |phi[0,0,0]|, two elementwise ops) and the affine maps between the
unit cube and the world are torch ops.  Points live in the unit cube, node i at i / R per axis, the grid is periodic; a finite
point outside [0, 1) wraps where the reference raises for p = 1.0.  Sign: with outward normals phi < 0 inside, the convention of
gs_tsdf_extract_*, so faces come out facing outward.  Not here: batches above 1, the 2-D solve, the exact per-edge vertex gradient
(the backward of mesh_from_indicator is the Shape-as-Points rule g_phi = splat(v, -(g_v . n))), oriented points from a splat model.
No CPU path.
"""
from __future__ import annotations

from typing import Sequence, Tuple, Union

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib

Resolution = Union[int, Sequence[int]]


def _res3(resolution: Resolution) -> Tuple[int, int, int]:
    res = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    if len(res) != 3 or min(res) < 4 or res[0] * res[1] * res[2] >= 2 ** 31:
        raise ValueError(f"resolution {res} out of range (three sides >= 4, fewer than 2^31 nodes)")
    return res


def _rows(points: Tensor, values: Tensor, what: str) -> Tuple[Tensor, Tensor]:
    _lib.require_cuda(points, values)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(points.shape)}")
    if values.dim() != 2 or values.shape[0] != points.shape[0] or not 1 <= values.shape[1] <= 4:
        raise ValueError(f"{what} must be [N,C] with C in 1..4, got {tuple(values.shape)}")
    return points.detach().float().contiguous(), values.detach().float().contiguous()


def _splat(points: Tensor, values: Tensor, res: Tuple[int, int, int]) -> Tensor:
    lib = _lib.lib()
    N, C = values.shape
    ws_bytes = lib.gs_grid_splat_ws_bytes(C, res[0], res[1], res[2])
    if ws_bytes == 0:
        raise _lib.GeoSplatHipError("resolution or channel count out of range")
    ws = _lib.workspace(ws_bytes, points.device)
    grid = torch.empty(C, *res, device=points.device)
    _lib.check(lib.gs_grid_splat(N, C, res[0], res[1], res[2], _lib.ptr(points), _lib.ptr(values), _lib.ptr(grid), _lib.ptr(ws), ws_bytes,
                                 _lib.stream()), "gs_grid_splat")
    return grid


def _sample(grid: Tensor, points: Tensor) -> Tensor:
    C, R0, R1, R2 = grid.shape
    out = torch.empty(points.shape[0], C, device=points.device)
    _lib.check(_lib.lib().gs_grid_sample_fwd(points.shape[0], C, R0, R1, R2, _lib.ptr(grid), _lib.ptr(points), _lib.ptr(out),
                                             _lib.stream()), "gs_grid_sample_fwd")
    return out


def _sample_dp(grid: Tensor, points: Tensor, cot: Tensor) -> Tensor:
    C, R0, R1, R2 = grid.shape
    g = torch.empty(points.shape[0], 3, device=points.device)
    _lib.check(_lib.lib().gs_grid_sample_bwd(points.shape[0], C, R0, R1, R2, _lib.ptr(grid), _lib.ptr(points), _lib.ptr(cot), _lib.ptr(g),
                                             _lib.stream()), "gs_grid_sample_bwd")
    return g


class _SplatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points: Tensor, values: Tensor, res: Tuple[int, int, int]) -> Tensor:
        p, v = _rows(points, values, "values")
        ctx.save_for_backward(p, v)
        return _splat(p, v, res)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_grid: Tensor):
        p, v = ctx.saved_tensors
        g = g_grid.float().contiguous()
        g_points = _sample_dp(g, p, v) if ctx.needs_input_grad[0] else None
        g_values = _sample(g, p) if ctx.needs_input_grad[1] else None
        return g_points, g_values, None


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid: Tensor, points: Tensor) -> Tensor:
        g = grid.detach().float().contiguous()
        ctx.save_for_backward(g, points)
        return _sample(g, points)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out: Tensor):
        grid, p = ctx.saved_tensors
        cot = g_out.float().contiguous()
        g_grid = _splat(p, cot, tuple(grid.shape[1:])) if ctx.needs_input_grad[0] else None
        g_points = _sample_dp(grid, p, cot) if ctx.needs_input_grad[1] else None
        return g_grid, g_points


def splat_to_grid(points01: Tensor, values: Tensor, resolution: Resolution) -> Tensor:
    """Periodic trilinear scatter of `values` [N,C], C in 1..4, at `points01` [N,3] (unit cube) -> grid [C,R0,R1,R2].  Bitwise
    reproducible from run to run.  Gradients to both inputs.  Rows with a non-finite coordinate or |p| >= 1024 add nothing."""
    return _SplatFn.apply(points01, values, _res3(resolution))


def sample_grid(grid: Tensor, points01: Tensor) -> Tensor:
    """Periodic trilinear lookup of `grid` [C,R0,R1,R2] at `points01` [N,3] -> [N,C]: the adjoint of splat_to_grid.  Gradients to
    both inputs (to the grid: a splat of the cotangent)."""
    _lib.require_cuda(grid, points01)
    if grid.dim() != 4 or not 1 <= grid.shape[0] <= 4:
        raise ValueError(f"grid must be [C,R0,R1,R2] with C in 1..4, got {tuple(grid.shape)}")
    _res3(grid.shape[1:])
    if points01.dim() != 2 or points01.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(points01.shape)}")
    return _SampleFn.apply(grid, points01.float().contiguous())


class _SpectralFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S: Tensor, res: Tuple[int, int, int], sigma: float) -> Tensor:
        ctx.res, ctx.sigma = res, sigma
        S = torch.view_as_real(S.detach().contiguous())
        Phi = torch.empty(res[0], res[1], res[2] // 2 + 1, 2, device=S.device)
        _lib.check(_lib.lib().gs_poisson_spectral_fwd(res[0], res[1], res[2], sigma, _lib.ptr(S), _lib.ptr(Phi), _lib.stream()),
                   "gs_poisson_spectral_fwd")
        return torch.view_as_complex(Phi)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_Phi: Tensor):
        res = ctx.res
        g = torch.view_as_real(g_Phi.contiguous())
        g_S = torch.empty(3, res[0], res[1], res[2] // 2 + 1, 2, device=g.device)
        _lib.check(_lib.lib().gs_poisson_spectral_bwd(res[0], res[1], res[2], ctx.sigma, _lib.ptr(g), _lib.ptr(g_S), _lib.stream()),
                   "gs_poisson_spectral_bwd")
        return torch.view_as_complex(g_S), None, None


def poisson_spectral(S: Tensor, resolution: Resolution, smoothness: float) -> Tensor:
    """The Fourier-space step alone: S [3,R0,R1,R2/2+1] complex64 -> Phi [R0,R1,R2/2+1] complex64 (include/geosplat_hip.h)."""
    res = _res3(resolution)
    _lib.require_cuda(S)
    if S.dtype != torch.complex64 or tuple(S.shape) != (3, res[0], res[1], res[2] // 2 + 1):
        raise ValueError(f"S must be complex64 [3,{res[0]},{res[1]},{res[2] // 2 + 1}], got {S.dtype} {tuple(S.shape)}")
    return _SpectralFn.apply(S, res, float(smoothness))


def poisson_indicator(points01: Tensor, normals: Tensor, resolution: Resolution, smoothness: float, shift: bool = True,
                      scale: bool = True) -> Tensor:
    """`DPSR(res, sig, scale, shift).forward` for one batch: points [N,3] in the unit cube and their normals [N,3] -> the indicator
    phi [R0,R1,R2], differentiable in both.  With outward normals and shift + scale, phi[0,0,0] = +0.5 and phi < 0 inside."""
    res = _res3(resolution)
    _lib.require_cuda(points01, normals)
    if normals.dim() != 2 or normals.shape != points01.shape or normals.shape[1] != 3:
        raise ValueError(f"points and normals must both be [N,3], got {tuple(points01.shape)} and {tuple(normals.shape)}")
    raster = splat_to_grid(points01, normals, res)
    S = torch.fft.rfftn(raster, dim=(1, 2, 3))
    Phi = _SpectralFn.apply(S, res, float(smoothness))
    phi = torch.fft.irfftn(Phi, s=res, dim=(0, 1, 2))
    if shift or scale:
        if shift:
            phi = phi - sample_grid(phi[None], points01).mean()
        if scale:
            phi = -phi / phi[0, 0, 0].abs() * 0.5
    return phi


class _MeshFn(torch.autograd.Function):
    """-> (vertices in the unit cube [V,3], faces [F,3] int64, vertex normals [V,3]); backward: the Shape-as-Points rule."""

    @staticmethod
    def forward(ctx, phi: Tensor):
        lib = _lib.lib()
        R0, R1, R2 = phi.shape
        dev = phi.device
        p = phi.detach().float().contiguous()
        volume = torch.empty(R0, R1, R2, 2, device=dev)
        _lib.check(lib.gs_grid_pack_volume(R0, R1, R2, _lib.ptr(p), _lib.ptr(volume), _lib.stream()), "gs_grid_pack_volume")
        # the extractor's fastest axis is its first: it sees (R2, R1, R0) and returns coordinates as (axis 2, axis 1, axis 0)
        ws_bytes = lib.gs_tsdf_extract_ws_bytes(R2, R1, R0)
        if ws_bytes == 0:
            raise _lib.GeoSplatHipError("resolution out of range")
        ws = _lib.workspace(ws_bytes, dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.check(lib.gs_tsdf_extract_count(R2, R1, R0, _lib.ptr(volume), _lib.ptr(ws), ws_bytes, _lib.ptr(counts), _lib.stream()),
                   "gs_tsdf_extract_count")
        V, F = counts.tolist()[:2]                                             # the one read-back
        nodes = torch.empty(V, 3, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int64, device=dev)
        normals = torch.empty(V, 3, device=dev)
        if V > 0 or F > 0:
            # origin -0.5 and voxel size 1: a voxel centre is its node index, so vertices come back in node units
            _lib.check(lib.gs_tsdf_extract_fill(R2, R1, R0, -0.5, -0.5, -0.5, 1.0, _lib.ptr(volume), _lib.ptr(ws), ws_bytes, V, F,
                                                _lib.ptr(nodes), _lib.ptr(faces), _lib.stream()), "gs_tsdf_extract_fill")
            nodes = nodes.flip(-1).contiguous()                                # (axis 0, axis 1, axis 2): a reflection ...
            faces = faces[:, [0, 2, 1]].contiguous()                           # ... so the winding flips with it
            _lib.check(lib.gs_grid_vertex_normals(R0, R1, R2, _lib.ptr(p), V, _lib.ptr(nodes), _lib.ptr(normals), _lib.stream()),
                       "gs_grid_vertex_normals")
        verts01 = nodes / torch.tensor([R0, R1, R2], dtype=torch.float32, device=dev)
        ctx.save_for_backward(verts01, normals)
        ctx.res = (R0, R1, R2)
        ctx.mark_non_differentiable(faces, normals)
        return verts01, faces, normals

    @staticmethod
    @once_differentiable
    def backward(ctx, g_verts: Tensor, _g_faces, _g_normals):
        verts01, normals = ctx.saved_tensors
        if verts01.shape[0] == 0:
            return torch.zeros(ctx.res, device=verts01.device)
        cot = -(g_verts.float() * normals).sum(-1, keepdim=True).contiguous()
        return _splat(verts01, cot, ctx.res)[0]


def mesh_from_indicator(phi: Tensor, lo: float = -1.25, hi: float = 1.25) -> Tuple[Tensor, Tensor, Tensor]:
    """Marching cubes at level 0 over the (R0-1)(R1-1)(R2-1) cubes of `phi` (no wrap) -> (vertices [V,3], faces [F,3] int64,
    vertex_normals [V,3]); node i of an axis lands on lo + (hi - lo) i / R.  Inside iff phi < 0; faces and normals point toward
    positive phi.  Normals carry no gradient; the gradient of the vertices to phi is g_phi = splat(v, -(g_v . n)).  One read-back of
    the counts; a phi without a sign change gives empty tensors."""
    _lib.require_cuda(phi)
    if phi.dim() != 3:
        raise ValueError(f"phi must be [R0,R1,R2], got {tuple(phi.shape)}")
    _res3(phi.shape)
    verts01, faces, normals = _MeshFn.apply(phi)
    return verts01 * (float(hi) - float(lo)) + float(lo), faces, normals


def diff_poisson_surface_recon(points: Tensor, normals: Tensor, *, smoothness: float, resolution: int) -> Tuple[Tensor, Tensor, Tensor]:
    """The reference's call: world points in [-1.25, 1.25]^3 (mapped by 0.4 x + 0.5 and clamped to the unit cube) and normals ->
    (vertices, faces, vertex_normals), vertices mapped back by 2.5 v - 1.25."""
    _lib.require_cuda(points, normals)
    phi = poisson_indicator((points * 0.4 + 0.5).clamp(0, 1), normals, resolution, smoothness)
    return mesh_from_indicator(phi, -1.25, 1.25)


def mesh_from_oriented_points(points: Tensor, normals: Tensor, resolution: int = 512, smoothness: float = 0.02) -> Tuple[Tensor, Tensor, Tensor]:
    """`TriangleMesh.from_diff_poisson_reconstruction` -> (vertices, faces, vertex_normals)."""
    return diff_poisson_surface_recon(points, normals, smoothness=smoothness, resolution=resolution)


def remesh_poisson(vertices: Tensor, faces: Tensor, resolution: int = 256, smoothness: float = 0.02) -> Tuple[Tensor, Tensor, Tensor]:
    """Re-solve a mesh through its face centres and unit face normals (the reference's Mesh2Mesh task, tests/graphics/test_dpsr.py):
    a closed, smooth surface from a mesh with holes and floaters.  The way to close a TSDF mesh (`extract_mesh()`) before
    `PriorModel(vertices, faces)`.  The mesh must fit [-1.25, 1.25]^3; zero-area faces are dropped."""
    _lib.require_cuda(vertices, faces)
    tri = vertices.float()[faces.long()]                                       # [F,3,3]
    n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    length = n.norm(dim=-1, keepdim=True)
    keep = length[:, 0] > 0
    return mesh_from_oriented_points(tri.mean(1)[keep], (n / length.clamp_min(1e-30))[keep], resolution, smoothness)
