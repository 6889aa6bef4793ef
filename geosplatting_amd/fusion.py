"""TSDF depth fusion and marching-cubes mesh extraction on the GPU: `TriangleMesh.from_depth_fusion`
(rfstudio/graphics/_mesh/_triangle_mesh.py:321-388) and the `MeshExport` task (tests/model/test_gsplat.py:169-202) without Open3D.

  TSDFVolume(resolution= | voxel_size=, bounds, sdf_trunc)   a dense volume; .integrate(depth_alpha, cameras), .extract_mesh()
  mesh_from_depth_fusion(depths, cameras, ...)               from_depth_fusion's signature plus the bounds a dense volume needs
  save_obj(path, vertices, faces)                            export(only_geometry=True): `v` / `f` lines

Integration and extraction are csrc/gs_tsdf.hip (gs_tsdf_integrate; gs_tsdf_extract_count -> one 32-byte read-back ->
gs_tsdf_extract_fill).  The reference's volume is hashed (Open3D ScalableTSDFVolume) and allocates blocks near observed depth; this
one is dense over `bounds` -- the two differ only in voxels no surface crosses.  A depth texel is looked up with this project's pixel
convention (pixel j covers [j, j + 1), centre j + 0.5), the one render_depth rasterizes with.  No CPU path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .cameras import Camera

MAX_VIEWS = 16
Bounds = Tuple[Sequence[float], Sequence[float]]
DEFAULT_BOUNDS: Bounds = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def camera_matrices(cameras: Sequence[Camera], device) -> Tuple[Tensor, Tensor]:
    """(viewmats [B,4,4], Ks [B,3,3]) on `device`, the matrices integrate hands to the kernel: every pose of a call in one batched
    inverse and the intrinsics in one upload -- a handful of launches, not a dozen per view.  cameras.view_matrix written with
    elementwise products (no BLAS call), so a camera's matrix does not depend on which others share its batch."""
    c2w = torch.stack([c.c2w.to(device, torch.float32) for c in cameras])                  # [B,3,4], OpenGL
    R = torch.cat((c2w[:, :, :1], -c2w[:, :, 1:3]), dim=-1)                                # y and z negated: OpenCV
    Rt = R.transpose(1, 2)
    T = c2w[:, :, 3]
    t = -(Rt[:, :, 0] * T[:, None, 0] + Rt[:, :, 1] * T[:, None, 1] + Rt[:, :, 2] * T[:, None, 2])
    vms = torch.zeros(len(cameras), 4, 4, device=c2w.device)
    vms[:, 3, 3].fill_(1.0)
    vms[:, :3, :3] = Rt
    vms[:, :3, 3] = t
    Ks = torch.tensor([[[c.fx, 0.0, c.cx], [0.0, c.fy, c.cy], [0.0, 0.0, 1.0]] for c in cameras], dtype=torch.float32).to(device)
    return vms, Ks


class TSDFVolume:
    """Dense truncated signed distance volume.  Give `resolution` (an int: voxels along the longest side of `bounds`, or three
    ints) or `voxel_size`; voxel n = i0 + R0 (i1 + R1 i2) has its centre at bounds[0] + (i + 0.5) voxel_size."""

    def __init__(self, resolution: Union[None, int, Sequence[int]] = None, *, voxel_size: Optional[float] = None,
                 bounds: Bounds = DEFAULT_BOUNDS, sdf_trunc: Optional[float] = None, device=None):
        lo, hi = (tuple(float(x) for x in b) for b in bounds)
        extent = tuple(h - l for l, h in zip(lo, hi))
        if len(lo) != 3 or len(hi) != 3 or min(extent) <= 0:
            raise ValueError("bounds must be ((x0, y0, z0), (x1, y1, z1)) with x1 > x0, ...")
        if (resolution is None) == (voxel_size is None):
            raise ValueError("give exactly one of resolution and voxel_size")
        if resolution is not None and not isinstance(resolution, int):
            res = tuple(int(r) for r in resolution)
            voxel_size = max(e / r for e, r in zip(extent, res))
        else:
            if resolution is not None:
                voxel_size = max(extent) / int(resolution)
            res = tuple(max(1, int(round(e / voxel_size))) for e in extent)
        if len(res) != 3 or min(res) < 1 or res[0] * res[1] * res[2] >= 2 ** 31:
            raise ValueError(f"resolution {res} out of range (fewer than 2^31 voxels)")
        self.resolution: Tuple[int, int, int] = res
        self.voxel_size = float(voxel_size)
        self.origin = lo
        self.sdf_trunc = 5.0 * self.voxel_size if sdf_trunc is None else float(sdf_trunc)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GeoSplatHipError("geosplatting_amd ops run on the GPU only (TSDFVolume on %s); there is no CPU path" % self.device)
        R0, R1, R2 = res
        self.volume = torch.zeros(R2, R1, R0, 2, device=self.device)           # interleaved (tsdf, weight), i0 fastest

    @property
    def tsdf(self) -> Tensor:
        """[R2, R1, R0] view onto the volume"""
        return self.volume[..., 0]

    @property
    def weight(self) -> Tensor:
        return self.volume[..., 1]

    def integrate(self, depth_alpha: Union[Tensor, Sequence[Tensor]], cameras: Sequence[Camera], *, alpha_trunc: float = 0.5,
                  depth_trunc: float = 4.0) -> "TSDFVolume":
        """Fuse `depth_alpha` ([B,H,W,2] or a list of [H,W,2]: what render_depth returns) seen from `cameras`, in order.  Any B:
        launches of at most 16 views.  No pose data is read back on the host."""
        maps = [depth_alpha] if isinstance(depth_alpha, Tensor) and depth_alpha.dim() == 3 else list(depth_alpha)
        cameras = [cameras] if isinstance(cameras, Camera) else list(cameras)
        if len(maps) != len(cameras):
            raise ValueError("Number of cameras must match the number of depth images.")
        lib = _lib.lib()
        if not maps:
            return self
        vms, Ks = camera_matrices(cameras, self.device)
        keep: List[Tensor] = [vms, Ks]
        views = []
        for k, (da, cam) in enumerate(zip(maps, cameras)):
            _lib.require_cuda(da)
            if da.dim() != 3 or da.shape[2] != 2 or da.shape[0] != cam.height or da.shape[1] != cam.width:
                raise ValueError(f"depth_alpha must be [H,W,2] of its camera, got {tuple(da.shape)}")
            da = da.detach().to(self.device, torch.float32).contiguous()
            keep.append(da)
            views.append(_lib.GsTsdfView(da.data_ptr(), vms[k].data_ptr(), Ks[k].data_ptr(), int(cam.width), int(cam.height)))
        R0, R1, R2 = self.resolution
        for lo in range(0, len(views), MAX_VIEWS):
            chunk = views[lo:lo + MAX_VIEWS]
            arr = (_lib.GsTsdfView * len(chunk))(*chunk)
            _lib.check(lib.gs_tsdf_integrate(R0, R1, R2, *self.origin, self.voxel_size, self.sdf_trunc, float(alpha_trunc),
                                             float(depth_trunc), len(chunk), arr, _lib.ptr(self.volume), _lib.stream()),
                       "gs_tsdf_integrate")
        del keep                                                               # (same stream: the allocator reuses them in order)
        return self

    def extract_mesh(self) -> Tuple[Tensor, Tensor]:
        """-> (vertices [V,3] float32, faces [F,3] int64); one 32-byte read-back of the counts.  `last_counts` keeps
        (vertices, triangles, valid cubes, surface cubes)."""
        lib = _lib.lib()
        R0, R1, R2 = self.resolution
        ws_bytes = lib.gs_tsdf_extract_ws_bytes(R0, R1, R2)
        if ws_bytes == 0:
            raise _lib.GeoSplatHipError("resolution out of range")
        ws = _lib.workspace(ws_bytes, self.device)
        counts = torch.empty(4, dtype=torch.int64, device=self.device)
        _lib.check(lib.gs_tsdf_extract_count(R0, R1, R2, _lib.ptr(self.volume), _lib.ptr(ws), ws_bytes, _lib.ptr(counts),
                                             _lib.stream()), "gs_tsdf_extract_count")
        V, F, n_valid, n_surface = counts.tolist()
        self.last_counts = (V, F, n_valid, n_surface)
        vertices = torch.empty(V, 3, device=self.device)
        faces = torch.empty(F, 3, dtype=torch.int64, device=self.device)
        _lib.check(lib.gs_tsdf_extract_fill(R0, R1, R2, *self.origin, self.voxel_size, _lib.ptr(self.volume), _lib.ptr(ws), ws_bytes,
                                            V, F, _lib.ptr(vertices), _lib.ptr(faces), _lib.stream()), "gs_tsdf_extract_fill")
        return vertices, faces


def mesh_from_depth_fusion(depths: Union[Tensor, Sequence[Tensor]], cameras: Sequence[Camera], *, voxel_size: float = 0.01,
                           sdf_trunc: float = 0.05, depth_scale: float = 1.0, depth_trunc: float = 4.0, alpha_trunc: float = 0.5,
                           bounds: Bounds = DEFAULT_BOUNDS, device=None) -> Tuple[Tensor, Tensor]:
    """`TriangleMesh.from_depth_fusion` -> (vertices, faces).  `depths` are (depth, alpha) images; depth is divided by depth_scale."""
    maps = [depths] if isinstance(depths, Tensor) and depths.dim() == 3 else list(depths)
    if len(maps) == 0:
        raise ValueError("no depth images")
    if depth_scale != 1.0:
        maps = [torch.cat((m[..., :1] / depth_scale, m[..., 1:]), dim=-1) for m in maps]
    vol = TSDFVolume(voxel_size=voxel_size, bounds=bounds, sdf_trunc=sdf_trunc, device=maps[0].device if device is None else device)
    vol.integrate(maps, cameras, alpha_trunc=alpha_trunc, depth_trunc=depth_trunc)
    return vol.extract_mesh()


def save_obj(path, vertices: Tensor, faces: Tensor) -> None:
    """Geometry only: one `v x y z` line per vertex, one 1-based `f a b c` line per face."""
    v = vertices.detach().cpu().double().tolist()
    f = (faces.detach().cpu().long() + 1).tolist()
    with open(path, "w") as out:
        out.writelines("v %.9g %.9g %.9g\n" % tuple(r) for r in v)
        out.writelines("f %d %d %d\n" % tuple(r) for r in f)


def load_obj(path) -> Tuple[Tensor, Tensor]:
    """What save_obj wrote -> (vertices [V,3] float32, faces [F,3] int64, 0-based), on the host."""
    v, f = [], []
    with open(path) as src:
        for line in src:
            tok = line.split()
            if tok and tok[0] == "v":
                v.append([float(x) for x in tok[1:4]])
            elif tok and tok[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in tok[1:4]])
    return torch.tensor(v, dtype=torch.float32).reshape(-1, 3), torch.tensor(f, dtype=torch.int64).reshape(-1, 3)
