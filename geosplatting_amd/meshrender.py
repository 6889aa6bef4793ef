"""A differentiable triangle-mesh rasterizer for the meshes this package extracts (FlexiCubes, TSDF + marching cubes): depth, normal,
silhouette and face-index maps from a camera.  What the reference gets from `TriangleMesh.render(cameras, shader=...)` and
`TriangleMesh.visible_faces` (rfstudio/graphics/_mesh/_triangle_mesh.py:496-555, rfstudio/graphics/shaders.py:107-132) through
nvdiffrast's `rasterize`, `interpolate` and `antialias`.  nvdiffrast is not restated line by line: the semantics below are this
project's, the kernels are csrc/gs_meshraster.hip and csrc/gs_meshaa.hip.

  rasterize_mesh(verts_cam, faces, camera_or_intrinsics, *, cull='none', near=1e-2, near_clip=False) -> rast [H,W,4]
  interpolate(attr, rast, faces)                                                    -> [H,W,C]
  mesh_edge_topology(faces)                                                         -> EdgeTopology
  antialias(color, rast, verts_cam, faces, camera_or_intrinsics, *, topology, cull, near, near_clip) -> [H,W,C]
  render_mesh(vertices, faces, camera, *, outputs, normal_type, cull, vertex_normals, near_clip, antialias,
              kd, ks, uvs, envmap, occlusion, min_visibility, bend_back_normal,
              ao, bvh, visibility)                                                  -> dict of maps ('color': meshshade.py;
                                                                                       'ao': occlusion.py)
  visible_faces(vertices, faces, camera, *, near_clip)                              -> sorted unique face ids
`render_mesh` with occlusion='ao' is the reference's PBRShader(occlusion_type='ao') (rfstudio/graphics/shaders.py:92-94) and its
output 'ao' is ShadingContext.ao; occlusion='screen' shades with a map the caller passes (the reference's 'ssao' map is not provided);
the Monte-Carlo shader is meshmc.py.
  silhouette_loss(alpha, target_mask)                                               -> scalar

Semantics of `rasterize_mesh`
  Inputs    verts_cam [V,3] fp32 in camera space, OpenCV convention, +z forward (what Camera.view_matrix produces); faces [F,3]
            (int32 for the kernels; int64 is converted); fx, fy, cx, cy, H, W from a Camera or a tuple (fx, fy, cx, cy, H, W).
            xs = fx X / Z + cx, ys = fy Y / Z + cy.  Pixel j covers [j, j + 1) and has its centre at j + 0.5 (the convention of
            render_depth and of the TSDF integration); row 0 is the top of the image.
  Coverage  exact and watertight.  (xs, ys) are snapped to 1/256 px, X = rint(256 xs); the three edge functions are evaluated in
            64-bit integers at (256 px + 128, 256 py + 128) and oriented by the sign of the snapped area.  A pixel is inside when
            all three are > 0; one that lies exactly on an edge belongs to the triangle only if that edge is a top or a left edge
            (top-left fill rule), so a pixel on an edge shared by two triangles is covered exactly once.
  Dropped   a triangle is dropped WHOLE when its snapped area is zero, when any snapped coordinate lies outside +-2^22 (+-16384 px)
            and, by default, when any vertex has Z <= near.  An object-centred camera never reaches the near plane; a camera that
            stands inside the mesh (scene-scale models, the reference's truck and courthouse configurations) does: `near_clip`.
  near_clip (opt-in; False gives the bits above) a vertex is inside iff Z > near (a NaN fails).  Three inside: a non-crossing face,
            the code and the bits above.  None inside, or a non-finite coordinate: dropped.  Otherwise a CROSSING face, clipped
            (Sutherland-Hodgman, at most 8 vertices) in camera space against Z > near and then against four guard planes
            |xs| <= G, |ys| <= G with G = 16000 px, in homogeneous form, e.g. (G - cx) Z - fx X >= 0: nothing is divided by a
            small Z, and every snapped coordinate of the result passes the +-2^22 test.  A new vertex is always computed from the
            inside endpoint A towards the outside endpoint B, t = dA / (dA - dB), C = fma(t, B - A, A) per coordinate in fp32:
            two faces that share the edge get the same bits for the cut, hence the same snapped vertex, hence a watertight seam.
            The polygon is fan-triangulated (v0, vk, vk+1) into at most 6 sub-triangles of the face's winding; each is projected,
            snapped, set up and walked like any triangle (top-left rule, `cull` on the sign of its snapped area, dropped on zero
            snapped area), so a pixel on an edge shared by two sub-triangles, two crossing faces, or a crossing and a
            non-crossing face is covered exactly once.  The values at a covered pixel are those of the FACE, in its three
            original vertices (which may lie behind the eye): the ray d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1) meets
            the face's plane at depth * d = sum_i b_i P_i.  Solved relative to P0 in fp32, every operation rounded once:
            e1 = P1 - P0, e2 = P2 - P0, h = d x e2, a = e1 . h, g = P0 x e1, b1 = -(P0 . h) / a, b2 = -(d . g) / a,
            depth = -(e2 . g) / a, b0 = (1 - b1) - b2 (the function w_i = d . (P_{i+1} x P_{i+2}), b_i = w_i / sum w,
            depth = det[P0 P1 P2] / sum w).  The fragment key and the resolve evaluate the same function, per face.  rast[..., 3]
            is the original face id + 1, so `interpolate`, shade_pixels and face-attribute lookups need no change.  Backward: with
            the face ids and the clip fixed, the gradient goes through that solve to all three original vertices, the ones behind
            the plane included.  Not clipped: the far plane (there is none), and images wider than the guard band.
  Culling   cull='none' rasterizes both windings.  cull='back' keeps the faces the reference keeps (_triangle_mesh.py:539),
            (camera_pos - centroid) . ((v1 - v0) x (v2 - v0)) > 0.  In camera space the eye is the origin and the normal is
            orthogonal to the triangle's edges, so the test is -det[v0; v1; v2] > 0, and det[v0; v1; v2] = Z0 Z1 Z2 / (fx fy) times the
            signed screen area (xs1 - xs0)(ys2 - ys0) - (ys1 - ys0)(xs2 - xs0).  Every kept Z is positive: a face is kept iff that
            area is NEGATIVE (decided on the snapped area, the one coverage uses).
  Values    at a covered pixel, from the UNSNAPPED fp32 positions taken relative to the pixel centre (the rounding error then
            scales with the triangle, not with the image): e_i = q_{i+1} x q_{i+2}, lambda_i = e_i / sum e (not clamped),
            perspective-correct b_i = (lambda_i / Z_i) / sum_j lambda_j / Z_j, depth = 1 / sum_j lambda_j / Z_j.
  Depth     among the triangles covering a pixel the smallest fp32 depth wins, the lower face index on equal depth; the result
            does not depend on launch order (one 64-bit atomic min per fragment).
  Output    rast [H,W,4] fp32 = (b0, b1, depth, face_id + 1), all zero where empty: nvdiffrast's layout with the view depth in
            place of z / w.  At most 2^24 faces.
  Backward  d rast[..., :3] -> d verts_cam with the face ids held fixed, through lambda, the perspective correction and the depth.
            The face-id channel and coverage carry no gradient here: silhouette gradients come from `antialias`.

Semantics of `antialias` (the reference's `dr.antialias(rgba, rast, projected, indices)`, on by default in its mesh shaders)
  Topology  mesh_edge_topology(faces): for every half-edge (f, i) -- edge i of face f runs between its vertices i + 1 and i + 2,
            opposite vertex i -- the other faces on the same undirected edge, any number of them (extracted meshes need not be
            manifold).  It depends on `faces` alone: build it once and pass it for every view and step.
  Pairs     pixels p and q = p + (1, 0) or p + (0, 1), both in the image, whose face-id channels differ.
  Foregr.   the pixel of the pair with a face and the smaller rast[..., 2]; an empty pixel loses, the lower face id wins equal
            depths.  a = that pixel, b = the other, T = the face at a.
  Exit edge with T's snapped integer edge functions and top-left biases, exactly as coverage uses them: edge i separates the pair
            when E_i(a) + bias_i >= 0 and E_i(b) + bias_i < 0.  The exit edge is the separating edge with the smallest
            E_i(a) / (E_i(a) - E_i(b)), compared exactly (128-bit cross products), ties to the lower i.  No separating edge (T covers
            b too and is occluded there): the pair blends nothing.
  Silhou.   the pair blends only if no other face on the exit edge has its opposite vertex strictly on the far side of the edge's
            line from T's opposite vertex (sign of the snapped 64-bit cross product).  A face the rasterizer would drop or cull does
            not count: `cull` and `near` must be the values `rast` was made with.  Boundary edges and creases whose faces fold onto
            the same side are silhouettes.
  Weight    q1, q2 = the UNSNAPPED fp32 positions of the exit edge's endpoints relative to a's pixel centre, s = +-1 from a to b.
            Horizontal pair: x* = (q1x q2y - q1y q2x) / (q2y - q1y), where the edge's line meets the row (vertical: x and y
            exchanged).  d = clamp(s x*, 0, 1).  d > 0.5: out[b] += (d - 0.5) (color[a] - color[b]); d < 0.5:
            out[a] += (0.5 - d) (color[b] - color[a]).  out = color + the sum over a pixel's (at most four) pairs.
  Backward  d color: the transpose of the blend.  d verts_cam: through d, with every discrete decision and the snap held fixed (the
            unsnapped positions of the exit edge's two vertices, xs = fx X / Z + cx); zero where d is clamped.  No gradient to rast.
  near_clip must be the value `rast` was made with.  A crossing face with at least one surviving sub-triangle counts as a neighbour
            in the silhouette test; its side of the exit edge's line is decided on the snapped position of the vertex that follows
            the edge's second endpoint (the face's vertex i + 2 for its half-edge i) in its clipped polygon -- every vertex of
            that polygon off the edge lies on the same side in exact arithmetic.  (It does not count when the guard band removed
            that endpoint.)  A pair whose FOREGROUND face is a crossing face blends nothing, with no gradient: its weight would
            need the derivative of the clip point.

Differences from nvdiffrast: near clipping is opt-in (`near_clip`) and leaves out the antialias weight on crossing foreground
faces, images wider than the guard band and the far plane; view depth in the third channel, y-down pixel rows; in `antialias`, the pairs, the
foreground, the exit edge and the silhouette test are decided on the snapped integer positions (and depth ties on the face id) while
the weight comes from the unsnapped ones, and a silhouette is tested against every face on the edge, not against one neighbour.
Every op raises GeoSplatHipError on CPU tensors; there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .cameras import Camera

Intrinsics = Union[Camera, Tuple[float, float, float, float, int, int]]
_CULL = {"none": 0, "back": 1}


def _intrinsics(cam: Intrinsics) -> Tuple[float, float, float, float, int, int]:
    if isinstance(cam, Camera):
        return float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), int(cam.height), int(cam.width)
    fx, fy, cx, cy, H, W = cam
    return float(fx), float(fy), float(cx), float(cy), int(H), int(W)


def _faces32(faces: Tensor) -> Tensor:
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise _lib.GeoSplatHipError("faces must be int32 or int64 [F,3]")
    return faces.to(torch.int32).contiguous()


def _mesh_head(v: Tensor, f: Tensor, intr, near: float):
    fx, fy, cx, cy, H, W = intr
    return (v.shape[0], f.shape[0], _lib.ptr(v), _lib.ptr(f), fx, fy, cx, cy, H, W, float(near))


def _entry(name: str, near_clip: bool):
    """gs_meshraster_<name> / gs_meshaa_<name>, or their near_clip twins gs_meshclip_<name> / gs_meshclip_aa_<name>"""
    stem, _, step = name.partition("_")
    twin = {"meshraster": "gs_meshclip_", "meshaa": "gs_meshclip_aa_"}[stem] + step
    return getattr(_lib.lib(), twin if near_clip else "gs_" + name), (twin if near_clip else "gs_" + name)


def rasterize_raw(verts_cam: Tensor, faces32: Tensor, intr, *, cull: str = "none", near: float = 1e-2,
                  stats: Optional[Tensor] = None, near_clip: bool = False) -> Tensor:
    """The two forward launches without autograd: gs_meshraster_fwd, gs_meshraster_resolve -> rast (gs_meshclip_* with `near_clip`).
    `stats` (int64[4] on the device, added to): fragments and atomics of the thread-per-triangle pass, then of the wave-per-triangle
    pass (which counts the crossing faces of `near_clip` too)."""
    if cull not in _CULL:
        raise ValueError("cull must be 'none' or 'back'")
    H, W = intr[4], intr[5]
    ws_bytes = _entry("meshraster_ws_bytes", near_clip)[0](faces32.shape[0], H, W)
    if ws_bytes == 0:
        raise _lib.GeoSplatHipError("mesh or image size out of range (at most 2^24 faces, H W < 2^31)")
    ws = _lib.workspace(ws_bytes, verts_cam.device)
    rast = torch.empty(H, W, 4, device=verts_cam.device)
    head = _mesh_head(verts_cam, faces32, intr, near)
    fwd, fwd_name = _entry("meshraster_fwd", near_clip)
    resolve, resolve_name = _entry("meshraster_resolve", near_clip)
    _lib.check(fwd(*head, _CULL[cull], _lib.ptr(ws), ws_bytes, _lib.ptr(stats), _lib.stream()), fwd_name)
    _lib.check(resolve(*head, _lib.ptr(ws), ws_bytes, _lib.ptr(rast), _lib.stream()), resolve_name)
    return rast


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_cam: Tensor, faces32: Tensor, intr, cull: str, near: float, near_clip: bool):
        v = verts_cam.detach().contiguous().float()
        rast = rasterize_raw(v, faces32, intr, cull=cull, near=near, near_clip=near_clip)
        ctx.save_for_backward(v, faces32, rast)
        ctx.intr, ctx.near, ctx.near_clip = intr, near, near_clip
        return rast

    @staticmethod
    def backward(ctx, d_rast: Tensor):
        v, f, rast = ctx.saved_tensors
        d_vc = torch.empty_like(v)
        bwd, name = _entry("meshraster_bwd", ctx.near_clip)
        _lib.check(bwd(*_mesh_head(v, f, ctx.intr, ctx.near), _lib.ptr(rast), _lib.ptr(d_rast.contiguous().float()), _lib.ptr(d_vc),
                       _lib.stream()), name)
        return d_vc, None, None, None, None, None


def rasterize_mesh(verts_cam: Tensor, faces: Tensor, camera_or_intrinsics: Intrinsics, *, cull: str = "none",
                   near: float = 1e-2, near_clip: bool = False) -> Tensor:
    """-> rast [H,W,4] = (b0, b1, view depth, face_id + 1), zeros where empty; differentiable in `verts_cam` (module docstring).
    `near_clip`: faces that cross the near plane are clipped instead of dropped."""
    _lib.require_cuda(verts_cam, faces)
    if verts_cam.ndim != 2 or verts_cam.shape[1] != 3:
        raise _lib.GeoSplatHipError("verts_cam must be [V,3]")
    if cull not in _CULL:
        raise ValueError("cull must be 'none' or 'back'")
    return _Rasterize.apply(verts_cam, _faces32(faces), _intrinsics(camera_or_intrinsics), cull, float(near), bool(near_clip))


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr: Tensor, rast: Tensor, faces32: Tensor):
        a = attr.detach().contiguous().float()
        r = rast.detach().contiguous().float()
        per_face_vertex = int(a.ndim == 3)
        C, F = a.shape[-1], faces32.shape[0]
        V = 0 if per_face_vertex else a.shape[0]
        P = r.numel() // 4
        out = torch.empty(*r.shape[:-1], C, device=a.device)
        _lib.check(_lib.lib().gs_mesh_interp_fwd(P, C, F, V, per_face_vertex, _lib.ptr(r), _lib.ptr(faces32), _lib.ptr(a), _lib.ptr(out),
                                                 _lib.stream()), "gs_mesh_interp_fwd")
        ctx.save_for_backward(a, r, faces32)
        ctx.dims = (P, C, F, V, per_face_vertex)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        a, r, f = ctx.saved_tensors
        d_attr = torch.empty_like(a)
        d_rast = torch.empty_like(r) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().gs_mesh_interp_bwd(*ctx.dims, _lib.ptr(r), _lib.ptr(f), _lib.ptr(a), _lib.ptr(d_out.contiguous().float()),
                                                 _lib.ptr(d_attr), _lib.ptr(d_rast), _lib.stream()), "gs_mesh_interp_bwd")
        return d_attr, d_rast, None


def interpolate(attr: Tensor, rast: Tensor, faces: Tensor) -> Tensor:
    """out[p] = sum_i b_i attr_i at the face rast names, b2 = 1 - b0 - b1; zeros where empty.  `attr` [V,C]: per-vertex attributes
    through the face's vertex indices (nvdiffrast's interpolate); [F,3,C]: per-face-vertex attributes (the reference's
    facial_vertex_attribute_map).  Differentiable in `attr` and in rast[..., :2]."""
    _lib.require_cuda(attr, rast, faces)
    f = _faces32(faces)
    if rast.ndim < 2 or rast.shape[-1] != 4:
        raise _lib.GeoSplatHipError("rast must be [...,4]")
    if not (attr.ndim == 2 or (attr.ndim == 3 and attr.shape[1] == 3 and attr.shape[0] == f.shape[0])) or attr.shape[-1] < 1:
        raise _lib.GeoSplatHipError("attr must be [V,C] or [F,3,C]")
    return _Interpolate.apply(attr, rast, f)


class EdgeTopology:
    """The half-edge neighbourhoods of a face array, on the device (module docstring; layout in csrc/gs_meshaa.hip).  Valid for as
    long as `faces` is unchanged, for any vertex positions and any camera."""

    def __init__(self, buffer: Tensor, n_faces: int):
        self.buffer, self.n_faces = buffer, int(n_faces)

    def neighbours(self):
        """Host copy, for inspection: for every half-edge 3 f + i the sorted list of (other face, index of its opposite vertex)."""
        F = self.n_faces
        slots = 16
        while slots < 6 * F:
            slots *= 2
        words = self.buffer.cpu()[8 * slots:8 * slots + 4 * (slots + 6 * F)].view(torch.int32).tolist()
        head, slot, nxt = words[:slots], words[slots:slots + 3 * F], words[slots + 3 * F:]
        out = []
        for h in range(3 * F):
            group, k = [], head[slot[h]] if slot[h] >= 0 else -1
            while k >= 0 and len(group) <= 3 * F:
                if k // 3 != h // 3:
                    group.append((k // 3, k % 3))
                k = nxt[k]
            out.append(sorted(group))
        return out


def mesh_edge_topology(faces: Tensor) -> EdgeTopology:
    """faces [F,3] -> the EdgeTopology `antialias` needs; built on the device, reusable while `faces` is unchanged."""
    _lib.require_cuda(faces)
    f = _faces32(faces)
    lib = _lib.lib()
    F = f.shape[0]
    n = lib.gs_mesh_topology_bytes(F)
    if n == 0:
        raise _lib.GeoSplatHipError("at most 2^24 faces")
    buf = torch.empty(n, dtype=torch.uint8, device=f.device)
    _lib.check(lib.gs_mesh_topology_build(F, _lib.ptr(f), _lib.ptr(buf), n, _lib.stream()), "gs_mesh_topology_build")
    return EdgeTopology(buf, F)


def _aa_head(v: Tensor, f: Tensor, intr, near: float, cull: str, topo: EdgeTopology, C: int, rast: Tensor, color: Tensor):
    return (*_mesh_head(v, f, intr, near), _CULL[cull], _lib.ptr(topo.buffer), topo.buffer.numel(), C, _lib.ptr(rast), _lib.ptr(color))


def antialias_raw(color: Tensor, rast: Tensor, verts_cam: Tensor, faces32: Tensor, intr, topo: EdgeTopology, *, cull: str = "none",
                  near: float = 1e-2, debug: bool = False, near_clip: bool = False):
    """gs_meshaa_fwd without autograd on contiguous fp32 tensors -> out, or (out, decisions int32 [H,W,2]) with `debug`: per pixel p
    the pairs (p, p + (1,0)) and (p, p + (0,1)); 0 = nothing blended, else 1 + exit edge + 4 (0 zero weight, 1 p receives, 2 the
    other pixel receives) + 16 (the foreground is the other pixel)."""
    H, W = intr[4], intr[5]
    C = color.shape[-1]
    out = torch.empty_like(color)
    dbg = torch.empty(H, W, 2, dtype=torch.int32, device=color.device) if debug else None
    fwd, name = _entry("meshaa_fwd", near_clip)
    _lib.check(fwd(*_aa_head(verts_cam, faces32, intr, near, cull, topo, C, rast, color), _lib.ptr(out), _lib.ptr(dbg), _lib.stream()),
               name)
    return (out, dbg) if debug else out


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color: Tensor, verts_cam: Tensor, rast: Tensor, faces32: Tensor, topo: EdgeTopology, intr, cull: str, near: float,
                near_clip: bool):
        c = color.detach().contiguous().float()
        v = verts_cam.detach().contiguous().float()
        r = rast.detach().contiguous().float()
        out = antialias_raw(c, r, v, faces32, intr, topo, cull=cull, near=near, near_clip=near_clip)
        ctx.save_for_backward(c, v, r, faces32)
        ctx.topo, ctx.intr, ctx.cull, ctx.near, ctx.near_clip = topo, intr, cull, near, near_clip
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        c, v, r, f = ctx.saved_tensors
        g = d_out.contiguous().float()
        d_color = torch.empty_like(c)
        d_vc = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        bwd, name = _entry("meshaa_bwd", ctx.near_clip)
        _lib.check(bwd(*_aa_head(v, f, ctx.intr, ctx.near, ctx.cull, ctx.topo, c.shape[-1], r, c), _lib.ptr(g), _lib.ptr(d_color),
                       _lib.ptr(d_vc), _lib.stream()), name)
        return d_color, d_vc, None, None, None, None, None, None, None


def antialias(color: Tensor, rast: Tensor, verts_cam: Tensor, faces: Tensor, camera_or_intrinsics: Intrinsics, *,
              topology: Optional[EdgeTopology] = None, cull: str = "none", near: float = 1e-2, near_clip: bool = False) -> Tensor:
    """color [H,W,C] -> [H,W,C] with the silhouette pixels blended across the outline (module docstring); differentiable in `color` and
    in `verts_cam`, not in `rast`.  `cull`, `near` and `near_clip` must be the values `rast` was made with; `topology`
    (mesh_edge_topology(faces)) is built here when none is passed."""
    _lib.require_cuda(color, rast, verts_cam, faces)
    if cull not in _CULL:
        raise ValueError("cull must be 'none' or 'back'")
    intr = _intrinsics(camera_or_intrinsics)
    f = _faces32(faces)
    if verts_cam.ndim != 2 or verts_cam.shape[1] != 3:
        raise _lib.GeoSplatHipError("verts_cam must be [V,3]")
    if rast.shape != (intr[4], intr[5], 4):
        raise _lib.GeoSplatHipError("rast must be [H,W,4]")
    if color.ndim != 3 or color.shape[:2] != rast.shape[:2] or color.shape[2] < 1:
        raise _lib.GeoSplatHipError("color must be [H,W,C] with C >= 1")
    if topology is None:
        topology = mesh_edge_topology(f)
    elif topology.n_faces != f.shape[0] or topology.buffer.device != color.device:
        raise _lib.GeoSplatHipError("topology was built for another face array or device")
    return _Antialias.apply(color, verts_cam, rast, f, topology, intr, cull, float(near), bool(near_clip))


_antialias = antialias


def silhouette_loss(alpha: Tensor, target_mask: Tensor) -> Tensor:
    """Mean squared error between an antialiased `alpha` map and a target mask of the same number of elements: the mask term a mesh
    gets once its outline has a gradient (render_mesh(..., antialias=True))."""
    return ((alpha - target_mask.to(alpha.dtype).reshape(alpha.shape)) ** 2).mean()


def _unit_or_z(v: Tensor) -> Tensor:
    """rfstudio.graphics.math.safe_normalize: unit vectors, (0, 0, 1) where the length is below 1e-6"""
    n = v.norm(dim=-1, keepdim=True)
    z = torch.zeros(3, device=v.device, dtype=v.dtype)
    z[2].fill_(1.0)
    return torch.where(n < 1e-6, z, v / n.clamp_min(1e-6))


def to_camera_space(vertices: Tensor, camera: Camera) -> Tensor:
    """world -> camera (OpenCV) through Camera.view_matrix, written elementwise; plain torch, differentiable"""
    M = camera.view_matrix.to(vertices.device, torch.float32)
    R, t = M[:3, :3], M[:3, 3]
    v = vertices.float()
    return v[:, 0:1] * R[:, 0] + v[:, 1:2] * R[:, 1] + v[:, 2:3] * R[:, 2] + t


def render_mesh(vertices: Tensor, faces: Tensor, camera: Camera, *, outputs: Sequence[str] = ("depth", "normal", "alpha", "face"),
                normal_type: str = "vertex", cull: str = "back", vertex_normals: Optional[Tensor] = None,
                near: float = 1e-2, near_clip: bool = False, antialias: bool = False, topology: Optional[EdgeTopology] = None,
                kd=None, ks=None, uvs: Optional[Tensor] = None, envmap=None, occlusion: str = "texture",
                min_visibility: float = 0.0, bend_back_normal: bool = False, ao: Optional[Tensor] = None, bvh=None,
                visibility: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """World-space mesh seen from `camera` -> {'rast' [H,W,4] and the requested maps}:
      depth  [H,W,1]  interpolated view depth (DepthShader), 0 where empty
      normal [H,W,3]  world-space normals (NormalShader): 'vertex' safe_normalize of the interpolated `vertex_normals` (default: the
                      area-weighted gs.vertex_normals), 'flat' the unit face normal of the winning face
      alpha  [H,W,1]  rast[..., 3:] > 0 as float
      face   [H,W,1]  int64 face index, -1 where empty (ShadingContext.face_indices)
      color  [H,W,3]  PBRShader: meshshade.shade_pixels on the interpolated world positions, the normal map of `normal_type` and the
                      interpolated `uvs` [F,3,2] (per face-vertex), with the Texture2D `kd`, `ks` under the TextureSplitSum `envmap`;
                      `occlusion`, `min_visibility`, `bend_back_normal` as there.  `uvs=None` is allowed only with 1x1 textures and means
                      zeros (PrettyShader).  0 where empty.  Differentiable in the textures, the environment and `vertices`.
                      occlusion='ao' shades with the map 'ao' below, occlusion='screen' with the map `visibility` [H,W] (required
                      there, refused otherwise).
      ao     [H,W,1]  ShadingContext.ao: the per-face ambient occlusion `ao` [F] (default: occlusion.face_ambient_occlusion of the mesh,
                      on `bvh` when one is passed) looked up through the face ids, face 0 where empty as face_attribute_map does; no
                      gradient, not antialiased
    depth and normal are differentiable in `vertices` (and `vertex_normals`); coverage is not, unless `antialias` is set: then the
    requested maps among depth, normal, color and alpha go through `antialias` together as one image (the way the reference
    antialiases its rgba), normal is normalised again, and alpha lies strictly between 0 and 1 along the outline with a gradient to
    the vertices of the outline's faces.  face and rast are never changed.  `topology`: mesh_edge_topology(faces), to reuse it.
    `near_clip`: faces that cross the near plane are clipped instead of dropped (module docstring), for cameras inside the mesh."""
    _lib.require_cuda(vertices, faces)
    unknown = set(outputs) - {"depth", "normal", "alpha", "face", "color", "ao"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    if normal_type not in ("vertex", "flat"):
        raise ValueError("normal_type must be 'vertex' or 'flat'")
    want_color = "color" in outputs
    if want_color:
        from .meshshade import _as_texture, check_occlusion
        if kd is None or ks is None or envmap is None:
            raise ValueError("outputs 'color' needs kd, ks and envmap")
        check_occlusion(occlusion)
        kd, ks = _as_texture(kd, "kd"), _as_texture(ks, "ks")
        if uvs is None and not (kd.data.shape[:2] == (1, 1) and ks.data.shape[:2] == (1, 1)):
            raise ValueError("uvs=None is allowed only with 1x1 textures")
    f32 = _faces32(faces)
    want_ao = "ao" in outputs or (want_color and occlusion == "ao")
    if (visibility is not None) != (want_color and occlusion == "screen"):
        raise ValueError("visibility [H,W] is the map of outputs 'color' with occlusion='screen': required there, refused otherwise")
    _lib.require_cuda(ao)
    if ao is not None and (not isinstance(ao, Tensor) or tuple(ao.shape) != (f32.shape[0],)):
        raise ValueError(f"ao must be a tensor [F] = [{f32.shape[0]}], got {tuple(ao.shape) if isinstance(ao, Tensor) else type(ao).__name__}")
    if want_color and uvs is not None and tuple(uvs.shape) != (f32.shape[0], 3, 2):
        raise _lib.GeoSplatHipError("uvs must be [F,3,2]")
    vc = to_camera_space(vertices, camera)
    rast = rasterize_mesh(vc, f32, camera, cull=cull, near=near, near_clip=near_clip)
    out: Dict[str, Tensor] = {"rast": rast}
    if "depth" in outputs:
        out["depth"] = interpolate(vc[:, 2:3].contiguous(), rast, f32)
    if "normal" in outputs or want_color:
        if normal_type == "vertex":
            if vertex_normals is None:
                from .mesh import vertex_normals as compute_vertex_normals
                vertex_normals = compute_vertex_normals(vertices.float(), faces.to(torch.int64))
            normal_map = _unit_or_z(interpolate(vertex_normals, rast, f32))
        else:
            fl = faces.to(torch.int64)
            v = vertices.float()
            fn = _unit_or_z(torch.cross(v[fl[:, 1]] - v[fl[:, 0]], v[fl[:, 2]] - v[fl[:, 0]], dim=-1))
            normal_map = fn[(rast[..., 3].long() - 1).clamp_min(0)]            # (face_attribute_map: face 0 where empty)
        if "normal" in outputs:
            out["normal"] = normal_map
    ao_map = None
    if want_ao:
        from .occlusion import face_ambient_occlusion
        per_face = ao.detach().float() if ao is not None else face_ambient_occlusion(vertices, f32, bvh)
        ao_map = per_face[(rast[..., 3].long() - 1).clamp_min(0)]                     # (face_attribute_map: face 0 where empty)
        if "ao" in outputs:
            out["ao"] = ao_map[..., None]
    if want_color:
        from .meshshade import shade_pixels
        position = interpolate(vertices.float().contiguous(), rast, f32)
        uv = interpolate(uvs.float(), rast, f32) if uvs is not None else torch.zeros(*rast.shape[:2], 2, device=rast.device)
        out["color"] = shade_pixels(position, normal_map, uv, rast, kd, ks, camera.c2w[:, 3].to(rast.device), envmap,
                                    occlusion=occlusion, min_visibility=min_visibility, bend_back_normal=bend_back_normal,
                                    visibility=ao_map if occlusion == "ao" else visibility)
    if "alpha" in outputs:
        out["alpha"] = (rast[..., 3:] > 0).float()
    if "face" in outputs:
        out["face"] = rast[..., 3:].long() - 1
    names = [k for k in ("depth", "normal", "color", "alpha") if k in out]
    if antialias and names:
        widths = [out[k].shape[-1] for k in names]
        blended = _antialias(torch.cat([out[k] for k in names], -1), rast, vc, f32, camera, topology=topology, cull=cull, near=near,
                             near_clip=near_clip)
        for k, part in zip(names, blended.split(widths, -1)):
            out[k] = _unit_or_z(part) if k == "normal" else part
    return out


def visible_faces(vertices: Tensor, faces: Tensor, camera: Camera, *, cull: str = "none", near: float = 1e-2,
                  near_clip: bool = False) -> Tensor:
    """TriangleMesh.visible_faces: the sorted unique ids of the faces that own at least one pixel (no culling, as there); with
    `near_clip` the faces that cross the near plane are among them."""
    _lib.require_cuda(vertices, faces)
    with torch.no_grad():
        rast = rasterize_mesh(to_camera_space(vertices, camera), faces, camera, cull=cull, near=near, near_clip=near_clip)
    ids = rast[..., 3]
    return (ids[ids > 0].long() - 1).unique()
