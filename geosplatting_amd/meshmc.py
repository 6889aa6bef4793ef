"""The Monte-Carlo mesh shader: ``TriangleMesh.render(cameras, shader=MCShader(envmap=...))`` of the reference
(rfstudio/graphics/shaders.py:282-359), the default of its ``PrettyShader`` -- the physically based look at an extracted mesh, with
shadows.  A composition of the package's autograd functions, no kernel of its own:

  G-buffer     rasterize_mesh + interpolate: world positions, the normal map of `normal_type`, per-face-vertex uvs
  materials    kd, ks = Texture2D.sample(uv)
  light        env_shade(bvh, mask = coverage, ro = pos + n 1e-3, pos, n, camera position, kd, ks, envmap, BSDF='pbr',
               n_samples_x = num_samples_per_ray, rnd_seed, shadow_scale) -> diff, spec [H,W,3] and the shadowed share resi [H,W,2]
  filter       bilateral_denoiser(., n, depth, sigma = max(2 shadow_scale, 1e-4)) with depth = (pos - cam_pos) . (-c2w[:, 2])
  'pbr'        denoise(diff) kd (1 - ks[2]) + denoise(spec)       (one 6-channel filter call: the filter is per channel)
  'diffuse'    denoise(diff) kd
  'vis'        1 - denoise(resi[0] + resi[1], expanded to 3 channels)

Gradients reach the kd / ks textures, the light and -- through positions and normals -- the vertices, because the pieces have them;
never the sample directions or the visibility.  Against the reference: 'vis' has 3 channels with `denoise=False` too (the reference
returns its 2-channel residual there); a map that carries a frame transform is refused (bake it), where the reference moves the scene
into the map's frame; pixels without coverage are 0.  Not provided: PrettyShader(occlusion_type='mc')'s daylight map (a dataset file),
ShadowShader, PathTraceShader."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .cameras import Camera
from .denoise import bilateral_denoiser
from .envshade import LatLngEnvMap, env_shade, require_baked
from .meshrender import _faces32, _unit_or_z, interpolate, rasterize_mesh, to_camera_space
from .meshshade import _as_texture
from .raytrace import MeshBVH

__all__ = ["render_mesh_mc"]

_RENDER_TYPES = ("pbr", "diffuse", "vis")


def render_mesh_mc(vertices: Tensor, faces: Tensor, camera: Camera, *, kd, ks, uvs: Optional[Tensor], envmap: LatLngEnvMap,
                   bvh: Optional[MeshBVH] = None, num_samples_per_ray: int = 8, shadow_scale: float = 1.0, denoise: bool = True,
                   render_type: str = "pbr", normal_type: str = "vertex", vertex_normals: Optional[Tensor] = None,
                   rnd_seed: Optional[int] = None, cull: str = "back", near: float = 1e-2, near_clip: bool = False) -> Tensor:
    """MCShader -> colour [H,W,3], 0 where empty (module docstring).  `kd`, `ks`: Texture2D; `uvs` [F,3,2] or None with 1x1 textures;
    `envmap` a LatLngEnvMap without a transform; `bvh`: a MeshBVH of this mesh (built here when None); `rnd_seed=None` draws a fresh
    seed in forward and again in backward, as `env_shade` documents."""
    if render_type not in _RENDER_TYPES:
        raise ValueError(f"render_type must be one of {_RENDER_TYPES}, got {render_type!r}")
    if normal_type not in ("vertex", "flat"):
        raise ValueError("normal_type must be 'vertex' or 'flat'")
    if not isinstance(envmap, LatLngEnvMap):
        raise TypeError(f"envmap must be a LatLngEnvMap, got {type(envmap).__name__}")
    require_baked(envmap, "render_mesh_mc")
    kd, ks = _as_texture(kd, "kd"), _as_texture(ks, "ks")
    if uvs is None and not (kd.data.shape[:2] == (1, 1) and ks.data.shape[:2] == (1, 1)):
        raise ValueError("uvs=None is allowed only with 1x1 textures")
    _lib.require_cuda(vertices, faces, kd.data, ks.data, envmap.data, uvs)
    f32 = _faces32(faces)
    if uvs is not None and tuple(uvs.shape) != (f32.shape[0], 3, 2):
        raise _lib.GeoSplatHipError("uvs must be [F,3,2]")
    v = vertices.float()
    if bvh is None:
        bvh = MeshBVH(v.detach().contiguous(), f32)
    vc = to_camera_space(v, camera)
    rast = rasterize_mesh(vc, f32, camera, cull=cull, near=near, near_clip=near_clip)
    H, W = rast.shape[:2]
    position = interpolate(v.contiguous(), rast, f32)
    if normal_type == "vertex":
        if vertex_normals is None:
            from .mesh import vertex_normals as compute_vertex_normals
            vertex_normals = compute_vertex_normals(v, faces.to(torch.int64))
        normal = _unit_or_z(interpolate(vertex_normals, rast, f32))
    else:
        fl = faces.to(torch.int64)
        fn = _unit_or_z(torch.cross(v[fl[:, 1]] - v[fl[:, 0]], v[fl[:, 2]] - v[fl[:, 0]], dim=-1))
        normal = fn[(rast[..., 3].long() - 1).clamp_min(0)]
    uv = interpolate(uvs.float(), rast, f32) if uvs is not None else torch.zeros(H, W, 2, device=rast.device)
    kd_map, ks_map = kd.sample(uv), ks.sample(uv)
    c2w = camera.c2w.to(rast.device, torch.float32)
    cam_pos = c2w[:, 3].contiguous()
    depth = ((position - cam_pos) * (-c2w[:, 2])).sum(-1, keepdim=True)
    mask = (rast[..., 3] > 0).float()
    flat = lambda t: t.reshape(H * W, t.shape[-1])
    diff, spec, resi = env_shade(bvh, mask.reshape(-1), flat(position + normal * 1e-3), flat(position), flat(normal), cam_pos, flat(kd_map),
                                 flat(ks_map), envmap, BSDF="pbr", n_samples_x=int(num_samples_per_ray), rnd_seed=rnd_seed,
                                 shadow_scale=float(shadow_scale))
    diff, spec, resi = diff.view(H, W, 3), spec.view(H, W, 3), resi.view(H, W, 2)
    sigma = max(2.0 * float(shadow_scale), 1e-4)
    nrm_c, depth_c = normal.detach().contiguous(), depth.detach().contiguous()
    if render_type == "pbr":
        if denoise:
            diff, spec = bilateral_denoiser(torch.cat((diff, spec), -1), nrm_c, depth_c, sigma).split(3, -1)
        return diff * kd_map * (1.0 - ks_map[..., 2:3]) + spec
    if render_type == "diffuse":
        if denoise:
            diff = bilateral_denoiser(diff.contiguous(), nrm_c, depth_c, sigma)
        return diff * kd_map
    shadow = resi.sum(-1, keepdim=True).expand(H, W, 3).contiguous()
    if denoise:
        shadow = bilateral_denoiser(shadow, nrm_c, depth_c, sigma)
    return 1.0 - shadow
