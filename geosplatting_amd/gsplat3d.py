"""Vanilla-3DGS training on the GPU: the reference's second model, end to end.

  GaussianSet     == rfstudio/graphics/_splats.py  Splats (random / from_points, reset_opacities, densify_and_cull, cull,
                     clear_extras_) + the state_dict / PLY export of rfstudio/model/gsplat.py:59-98
  GSplatModel     == rfstudio/model/gsplat.py      GSplatter (render_rgb / render_rgba / render_depth, background colour,
                     SH-degree cap, update_grad_norm)
  mutate_adam     == rfstudio/optim/optimizer.py:121-191  ModuleOptimizers.mutate_params for torch.optim.Adam
  GSplatTrainer   == rfstudio/trainer/gsplat_trainer.py   (six Adam groups, the step, the refine schedule)

The refinement is the hot path: classification, ranks, the row map and the move of every parameter AND Adam-moment row are
csrc/gs_densify.hip (gs_densify_plan -> one 32-byte read-back -> gs_densify_fill, one gather launch).  The densification
statistics are gs_densify_stats.  No CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .cameras import Camera
from .loss import photo_loss
from .shading import _rasterize_activated

KIND_COPY, KIND_MEANS, KIND_SCALES, KIND_MOMENT = 0, 1, 2, 3
MODE_DENSIFY, MODE_CULL = 0, 1
FIELDS = ("means", "scales", "quats", "colors", "shs", "opacities")
_KIND = {"means": KIND_MEANS, "scales": KIND_SCALES}
_ADAM_ITEMS = ("exp_avg", "exp_avg_sq")
SH_C0 = 0.28209479177387814


def _sh_dim(sh_degree: int) -> int:
    if sh_degree not in (0, 1, 2, 3, 4):
        raise ValueError(sh_degree)
    return (sh_degree + 1) ** 2


def _random_quaternion(size: int, generator: Optional[torch.Generator]) -> Tensor:
    """rfstudio/graphics/math.py:59-72"""
    u = torch.rand(size, generator=generator)
    v = torch.rand(size, generator=generator) * (2 * math.pi)
    w = torch.rand(size, generator=generator) * (2 * math.pi)
    return torch.stack([torch.sqrt(1 - u) * torch.sin(v), torch.sqrt(1 - u) * torch.cos(v),
                        torch.sqrt(u) * torch.sin(w), torch.sqrt(u) * torch.cos(w)], dim=-1)


def knn_mean_distance(points: Tensor, k: int = 3, chunk: int = 2048) -> Tensor:
    """Mean distance to the k nearest other points, [N] (Points.k_nearest(k)[0].mean(-1)): chunked torch.cdist on the host.  Runs once
    at initialisation."""
    p = points.detach().cpu().double()
    n = p.shape[0]
    out = torch.empty(n, dtype=torch.float64)
    for lo in range(0, n, chunk):
        d = torch.cdist(p[lo:lo + chunk], p)
        d[torch.arange(d.shape[0]), torch.arange(lo, lo + d.shape[0])] = float("inf")      # not its own neighbour
        out[lo:lo + chunk] = d.topk(min(k, n - 1), dim=-1, largest=False).values.mean(-1)
    return out.float()


def _moment_rows(optimizers: Optional[Dict[str, torch.optim.Optimizer]], name: str, param: Tensor) -> List[Tuple[dict, str, Tensor]]:
    """(state dict, item, tensor) of every Adam moment that follows `param`"""
    if not optimizers or name not in optimizers:
        return []
    opt = optimizers[name]
    if not isinstance(opt, torch.optim.Adam):
        raise NotImplementedError("only torch.optim.Adam state follows a refinement")
    st = opt.state.get(param)
    if not st:
        return []
    return [(st, item, st[item]) for item in _ADAM_ITEMS if item in st]


class GaussianSet:
    """Trainable Gaussians with log scales, logit opacities [N,1], RGB colours and the SH rest shs [N, (deg+1)^2 - 1, 3]."""

    def __init__(self, means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor, colors: Tensor, shs: Tensor,
                 requires_grad: bool = False):
        n = means.shape[0]
        if means.shape != (n, 3) or scales.shape != (n, 3) or quats.shape != (n, 4) or opacities.shape != (n, 1) or \
                colors.shape != (n, 3) or shs.dim() != 3 or shs.shape[0] != n or shs.shape[2] != 3:
            raise ValueError("GaussianSet expects means[N,3], scales[N,3], quats[N,4], opacities[N,1], colors[N,3], shs[N,K,3]")
        _sh_dim_to_degree(shs.shape[1] + 1)
        self.means, self.scales, self.quats, self.opacities, self.colors, self.shs = (
            t.detach().float().contiguous().requires_grad_(requires_grad) for t in (means, scales, quats, opacities, colors, shs))
        self.xys_grad_norm: Optional[Tensor] = None
        self.vis_counts: Optional[Tensor] = None
        self.last_width: Optional[int] = None
        self.last_height: Optional[int] = None
        self.last_totals: Optional[Tuple[int, int, int, int]] = None      # (n_selected, n_split, n_dup, N') of the last refinement

    # ---------------------------------------------------------------------------------------- construction
    @classmethod
    def random(cls, size: int, *, sh_degree: int, random_scale: float, device=None, requires_grad: bool = False,
               generator: Optional[torch.Generator] = None) -> "GaussianSet":
        """Splats.random (rfstudio/graphics/_splats.py:61-80): uniform points in the cube of half-width random_scale."""
        points = (torch.rand((size, 3), generator=generator) - 0.5) * (2 * random_scale)
        return cls._from_positions(points, torch.ones(size, 3) * 0.5, sh_degree, device, requires_grad, generator)

    @classmethod
    def from_points(cls, positions: Tensor, colors: Tensor, *, sh_degree: int, device=None, requires_grad: bool = False,
                    generator: Optional[torch.Generator] = None, knn: str = "host") -> "GaussianSet":
        """Splats.from_points (rfstudio/graphics/_splats.py:38-58).  ``knn`` chooses where the mean distance to the three nearest
        other points (the initial scale) is computed: 'host' (the default) is `knn_mean_distance`, a chunked float64 torch.cdist,
        O(N^2); 'device' is `geometry.k_nearest` on the GPU (``device``, or the device of ``positions``), an exact grid search in
        fp32.  The two differ in the last fp32 bits of the scales: float64 distances rounded once against fp32 squared distances
        and an fp32 square root."""
        if knn not in ("host", "device"):
            raise ValueError(f"knn must be 'host' or 'device', got {knn!r}")
        dist = None
        if knn == "device":
            from .geometry import k_nearest
            dev = torch.device(device) if device is not None else positions.device
            n = positions.shape[0]
            if n < 2:
                raise ValueError("knn='device' needs at least two points")
            dist = k_nearest(positions.detach().float().to(dev), min(3, n - 1))[0].mean(-1).cpu()
        return cls._from_positions(positions.detach().cpu().float(), colors.detach().cpu().float(), sh_degree, device, requires_grad,
                                   generator, dist)

    @classmethod
    def _from_positions(cls, points, colors, sh_degree, device, requires_grad, generator, dist=None):
        size = points.shape[0]
        if dist is None:
            dist = knn_mean_distance(points, 3)
        gs = cls(means=points.clone(), scales=dist[:, None].log().repeat(1, 3), quats=_random_quaternion(size, generator),
                 opacities=torch.logit(0.1 * torch.ones(size, 1)), colors=colors.clone(),
                 shs=torch.zeros(size, _sh_dim(sh_degree) - 1, 3))
        return gs.to(device).requires_grad_(requires_grad)

    # ---------------------------------------------------------------------------------------- plumbing
    @property
    def shape(self) -> Tuple[int]:
        return (self.means.shape[0],)

    def __len__(self) -> int:
        return self.means.shape[0]

    @property
    def device(self) -> torch.device:
        return self.means.device

    @property
    def sh_dim(self) -> int:
        return self.shs.shape[1]

    @property
    def sh_degree(self) -> int:
        return _sh_dim_to_degree(self.sh_dim + 1)

    @property
    def requires_grad(self) -> bool:
        return self.means.requires_grad

    def requires_grad_(self, flag: bool = True) -> "GaussianSet":
        for name in FIELDS:
            getattr(self, name).requires_grad_(flag)
        return self

    def to(self, device) -> "GaussianSet":
        if device is None:
            return self
        rg = self.requires_grad
        for name in FIELDS:
            setattr(self, name, getattr(self, name).detach().to(device).requires_grad_(rg))
        if self.xys_grad_norm is not None:
            self.xys_grad_norm, self.vis_counts = self.xys_grad_norm.to(device), self.vis_counts.to(device)
        return self

    def parameters(self) -> Dict[str, Tensor]:
        return {name: getattr(self, name) for name in FIELDS}

    def state_dict(self) -> Dict[str, Tensor]:
        """the keys of GSplatter.state_dict (rfstudio/model/gsplat.py:59-67)"""
        return {name: getattr(self, name) for name in ("means", "colors", "shs", "opacities", "scales", "quats")}

    def load_state_dict(self, state_dict: Dict[str, Tensor]) -> None:
        fresh = GaussianSet(**{name: state_dict[name] for name in FIELDS}).to(self.device).requires_grad_(self.requires_grad)
        for name in FIELDS:
            setattr(self, name, getattr(fresh, name))
        self.clear_extras_()

    def clear_extras_(self) -> "GaussianSet":
        self.xys_grad_norm = self.vis_counts = self.last_width = self.last_height = None
        return self

    @torch.no_grad()
    def export_point_cloud(self, path) -> None:
        """Binary little-endian PLY with the property names of GSplatter.export_point_cloud (rfstudio/model/gsplat.py:80-98):
        positions, zero normals, f_dc_*, opacity, scale_*, rot_* (normalised quaternion)."""
        quats = self.quats / self.quats.norm(dim=-1, keepdim=True)
        cols = [self.means, torch.zeros_like(self.means), (self.colors - 0.5) / SH_C0, self.opacities, self.scales, quats]
        data = torch.cat([c.detach().float().cpu() for c in cols], dim=-1).numpy().astype("<f4")
        names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                 "rot_0", "rot_1", "rot_2", "rot_3"]
        header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % data.shape[0]
        header += "".join("property float %s\n" % n for n in names) + "end_header\n"
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(np.ascontiguousarray(data).tobytes())

    # ---------------------------------------------------------------------------------------- refinement
    @torch.no_grad()
    def reset_opacities(self, *, reset_value: float) -> None:
        """Splats.reset_opacities (:82-85)"""
        _lib.require_cuda(self.opacities)
        self.opacities.data.clamp_(max=torch.logit(torch.tensor(reset_value)).item())

    @torch.no_grad()
    def densify_and_cull(self, *, densify_grad_thresh: float, densify_size_thresh: float, num_splits: int, cull_alpha_thresh: float,
                         cull_scale_thresh: Optional[float], randn: Optional[Tensor] = None,
                         generator: Optional[torch.Generator] = None,
                         optimizers: Optional[Dict[str, torch.optim.Optimizer]] = None) -> Tensor:
        """Splats.densify_and_cull (:121-159).  Returns indices i64[N']: the source row of every kept row, -1 for every new one.
        randn [num_splits, n_split, 3] are the normal samples of Splats.split (drawn here from `generator` when None).  With
        `optimizers` (field name -> torch.optim.Adam over that field) the Adam moments move in the same launch and the state is
        re-keyed to the new parameters, i.e. ModuleOptimizers.mutate_params(indices=...) is done."""
        _lib.require_cuda(*self.parameters().values())
        assert self.xys_grad_norm is not None and self.vis_counts is not None
        half_extent = 0.5 * max(float(self.last_width), float(self.last_height))
        return self._refine(MODE_DENSIFY, half_extent, densify_grad_thresh, densify_size_thresh, num_splits, cull_alpha_thresh,
                            cull_scale_thresh, randn, generator, optimizers)

    @torch.no_grad()
    def cull(self, *, cull_alpha_thresh: float, cull_scale_thresh: Optional[float],
             optimizers: Optional[Dict[str, torch.optim.Optimizer]] = None) -> Tensor:
        """Splats.cull (:161-175).  Returns the kept source rows, i64[N'].  The statistics are dropped with the rows (the trainer clears them
        right after either refinement)."""
        _lib.require_cuda(*self.parameters().values())
        return self._refine(MODE_CULL, 0.0, 0.0, 0.0, 0, cull_alpha_thresh, cull_scale_thresh, None, None, optimizers)

    def _refine(self, mode, half_extent, grad_thresh, size_thresh, num_splits, alpha_thresh, scale_thresh, randn, generator, optimizers):
        lib, dev, n = _lib.lib(), self.device, len(self)
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=dev)
        nbytes = lib.gs_densify_ws_bytes(n, int(num_splits))
        if nbytes == 0:
            raise _lib.GeoSplatHipError(f"densify: N={n} / num_splits={num_splits} outside the supported range")
        ws = _lib.workspace(nbytes, dev)
        totals = torch.empty(4, dtype=torch.int64, device=dev)
        src = {name: getattr(self, name).detach().contiguous() for name in FIELDS}
        opac = src["opacities"].view(-1)
        stats = (None, None) if mode == MODE_CULL else (self.xys_grad_norm.float().contiguous(), self.vis_counts.float().contiguous())
        if mode == MODE_DENSIFY and (stats[0].shape != (n,) or stats[1].shape != (n,)):
            raise _lib.GeoSplatHipError("densify: xys_grad_norm / vis_counts must be [N]")
        _lib.check(lib.gs_densify_plan(n, _lib.ptr(src["scales"]), _lib.ptr(opac), _lib.ptr(stats[0]), _lib.ptr(stats[1]),
                                       half_extent, grad_thresh, size_thresh, alpha_thresh,
                                       -1.0 if scale_thresh is None else scale_thresh, int(num_splits), mode, _lib.ptr(ws), nbytes,
                                       _lib.ptr(totals), _lib.stream()), "gs_densify_plan")
        n_sel, n_split, n_dup, n_out = (int(v) for v in totals.tolist())        # the reference's own sync (nonzero / boolean indexing)
        self.last_totals = (n_sel, n_split, n_dup, n_out)
        if mode == MODE_DENSIFY:
            if randn is None:
                randn = torch.randn((num_splits, n_split, 3), device=dev, generator=generator)
            _lib.require_cuda(randn)
            if tuple(randn.shape) != (num_splits, n_split, 3):
                raise _lib.GeoSplatHipError(f"densify: randn must be [{num_splits}, {n_split}, 3], got {tuple(randn.shape)}")
            randn = randn.float().contiguous()
        indices = torch.empty(n_out, dtype=torch.int64, device=dev)
        rows, new, moments = [], {}, []
        for name in FIELDS:
            new[name] = torch.empty((n_out,) + tuple(src[name].shape[1:]), device=dev)
            fpr = src[name][0].numel()
            if fpr == 0:                                                    # SH degree 0: shs is [N, 0, 3], nothing to move
                continue
            rows.append((src[name], new[name], fpr, _KIND.get(name, KIND_COPY)))
            for st, item, m in _moment_rows(optimizers, name, getattr(self, name)):
                m = m.detach().contiguous()
                if m.shape != src[name].shape or m.dtype != torch.float32:
                    raise _lib.GeoSplatHipError(f"densify: Adam {item} of {name} does not match the parameter")
                out = torch.empty_like(new[name])
                rows.append((m, out, fpr, KIND_MOMENT))
                moments.append((name, st, item, out))
        table = (_lib.GsDensifyTensor * len(rows))()
        for k, (s, d, fpr, kind) in enumerate(rows):
            table[k].src, table[k].dst, table[k].floats_per_row, table[k].kind = s.data_ptr(), d.data_ptr(), fpr, kind
        _lib.check(lib.gs_densify_fill(n, int(num_splits), _lib.ptr(ws), nbytes, n_sel, n_split, n_dup, table, len(rows),
                                       _lib.ptr(src["quats"]), _lib.ptr(src["scales"]),
                                       _lib.ptr(randn) if (randn is not None and randn.numel()) else None, _lib.ptr(indices),
                                       _lib.stream()), "gs_densify_fill")
        rg = self.requires_grad
        old = {name: getattr(self, name) for name in FIELDS}
        for name in FIELDS:
            setattr(self, name, new[name].requires_grad_(rg))
        self.clear_extras_()
        if optimizers:
            by_name: Dict[str, Dict[str, Tensor]] = {}
            for name, _st, item, out in moments:
                by_name.setdefault(name, {})[item] = out
            for name, opt in optimizers.items():
                if name in old:
                    mutate_adam(opt, [getattr(self, name)], moments=[by_name.get(name, {})], old_params=[old[name]])
        return indices


def _sh_dim_to_degree(sh_dim: int) -> int:
    deg = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}.get(sh_dim)
    if deg is None:
        raise ValueError(f"shs with {sh_dim - 1} coefficients is no SH degree")
    return deg


# ------------------------------------------------------------------------------------------------ optimiser state
@torch.no_grad()
def mutate_adam(optimizer: torch.optim.Optimizer, new_params: Sequence[Tensor], *, indices: Optional[Tensor] = None, clear: bool = False,
                moments: Optional[Sequence[Dict[str, Tensor]]] = None, old_params: Optional[Sequence[Tensor]] = None) -> None:
    """ModuleOptimizers.mutate_params for one torch.optim.Adam (rfstudio/optim/optimizer.py:155-185): the state of every old
    parameter of param_groups[0] is re-keyed to the new parameter in the same position; `step` and every other entry stay.
      indices  i64[N'] (or [N',1]): exp_avg / exp_avg_sq rows follow `indices`, rows with a negative index start at 0;
      moments  the moved exp_avg / exp_avg_sq per parameter, as GaussianSet.densify_and_cull / cull produced them next to the
               parameters in their gs_densify_fill launch (what the trainer uses; nothing is gathered here);
      clear    zero the moments in place (the opacity reset)."""
    if not isinstance(optimizer, torch.optim.Adam):
        raise NotImplementedError("mutate_adam handles torch.optim.Adam")
    assert clear or indices is not None or moments is not None
    group = optimizer.param_groups[0]
    new_params = list(new_params)
    olds = list(group["params"]) if old_params is None else list(old_params)
    if indices is not None or moments is not None:
        if len(olds) != len(new_params):
            raise ValueError("mutate_adam: one new parameter per old parameter")
        idx = None if indices is None else indices.reshape(indices.shape[0], -1)[:, 0]
        for k, (param, new_param) in enumerate(zip(olds, new_params)):
            if param not in optimizer.state:
                continue
            st = optimizer.state[param]
            for item in _ADAM_ITEMS:
                if item not in st:
                    continue
                if moments is not None:
                    moved = moments[k][item]
                else:
                    moved = st[item][idx]
                    moved[idx < 0] = 0
                if moved.shape != new_param.shape:
                    raise ValueError(f"mutate_adam: {item} {tuple(moved.shape)} does not match the parameter {tuple(new_param.shape)}")
                st[item] = moved
            del optimizer.state[param]
            optimizer.state[new_param] = st
        group["params"] = new_params
    if clear:
        for param in group["params"]:
            st = optimizer.state.get(param, {})
            for item in _ADAM_ITEMS:
                if item in st:
                    st[item].zero_()


# ------------------------------------------------------------------------------------------------ the model
@dataclass
class UpdateInfo:
    xys: Tensor
    indices: Tensor
    last_width: int
    last_height: int


@dataclass
class GSplatModel:
    """GSplatter (rfstudio/model/gsplat.py:20-57) on rasterization_3dgs."""
    num_random: int = 50000
    random_scale: float = 1.0
    sh_degree: int = 3
    block_width: int = 16
    background_color: str = "random"
    prepare_densification: bool = False
    rasterize_mode: str = "classic"
    device: Optional[torch.device] = None
    generator: Optional[torch.Generator] = None          # host generator of the initialisation and the random background
    gaussians: Optional[GaussianSet] = None
    training: bool = True
    update_info: Optional[UpdateInfo] = field(default=None, repr=False)
    max_sh_degree: Optional[int] = None

    def __post_init__(self) -> None:
        if self.gaussians is None:
            self.gaussians = GaussianSet.random(self.num_random, sh_degree=self.sh_degree, random_scale=self.random_scale,
                                                device=self.device, requires_grad=True, generator=self.generator)
        if self.device is None:
            self.device = self.gaussians.device

    def train(self, mode: bool = True) -> "GSplatModel":
        self.training = mode
        return self

    def eval(self) -> "GSplatModel":
        return self.train(False)

    def state_dict(self) -> Dict[str, Tensor]:
        return self.gaussians.state_dict()

    def load_state_dict(self, state_dict: Dict[str, Tensor]) -> None:
        self.gaussians.load_state_dict(state_dict)

    def export_point_cloud(self, path) -> None:
        self.gaussians.export_point_cloud(path)

    def get_background_color(self) -> Tensor:
        """:100-107"""
        if self.background_color == "black":
            return torch.zeros(3)
        if self.background_color == "white":
            return torch.ones(3)
        if self.training:
            return torch.rand(3, generator=self.generator)
        return torch.tensor([0.1490, 0.1647, 0.2157])

    def set_max_sh_degree(self, value: Optional[int] = None) -> None:
        self.max_sh_degree = value

    def _active_sh_degree(self) -> int:
        deg = self.gaussians.sh_degree
        return deg if self.max_sh_degree is None else min(self.max_sh_degree, deg)

    def _rasterize(self, camera: Camera, render_mode: str):
        if self.rasterize_mode == "2dgs":
            raise NotImplementedError("rasterize_mode='2dgs' (rasterization_2dgs) is geosplatting_amd.SurfelModel, not GSplatModel")
        if self.rasterize_mode not in ("antialiased", "classic"):
            raise ValueError(f"Unknown rasterize_mode: {self.rasterize_mode}")
        g = self.gaussians
        _lib.require_cuda(g.means)
        track = self.training and self.prepare_densification and g.requires_grad and torch.is_grad_enabled()
        render, alpha, info = _rasterize_activated(g.means, g.scales, g.quats, g.opacities, g.colors, camera, render_mode,
                                                   self.block_width, shs=g.shs, sh_degree=self._active_sh_degree(),
                                                   rasterize_mode=self.rasterize_mode, means2d_grad=track)
        if track and info["means2d"].requires_grad:
            info["means2d"].retain_grad()
            self.update_info = UpdateInfo(xys=info["means2d"], indices=info["gaussian_ids"], last_width=int(camera.width),
                                          last_height=int(camera.height))
        return render, alpha

    def render_layers(self, camera: Camera) -> Tuple[Tensor, Tensor]:
        """(render [H,W,3] premultiplied, alpha [H,W,1]) of one camera: what render_rgb blends and the loss consumes"""
        render, alpha = self._rasterize(camera, "RGB")
        return render[..., :3].squeeze(0), alpha.squeeze(0)

    def render_rgb(self, camera: Camera, background_color: Optional[Tensor] = None) -> Tensor:
        """:188-282 -> [H,W,3] over the background colour"""
        bg = self.get_background_color() if background_color is None else background_color
        render, alpha = self.render_layers(camera)
        return render + (1 - alpha) * bg.to(render)

    def render_rgba(self, camera: Camera) -> Tensor:
        """:284-358 -> [H,W,4]"""
        return torch.cat(self.render_layers(camera), dim=-1)

    def render_depth(self, camera: Camera) -> Tensor:
        """:112-186 -> [H,W,2] (expected depth, alpha)"""
        render, alpha = self._rasterize(camera, "ED")
        return torch.cat((render, alpha), dim=-1).squeeze(0)

    @torch.no_grad()
    def extract_mesh(self, resolution: int = 512, fusing_alpha_threshold: float = 0.5, num_views: int = 100, radius: float = 3.0,
                     image_size: int = 800, up: Sequence[float] = (0.0, 0.0, 1.0),
                     bounds=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), generator: Optional[torch.Generator] = None,
                     target_faces: Optional[int] = None, min_component_faces: Optional[int] = None) -> Tuple[Tensor, Tensor]:
        """The MeshExport task (tests/model/test_gsplat.py:169-202) -> (vertices [V,3], faces [F,3] int64): depth from `num_views`
        cameras on a sphere of `radius` around the centre of `bounds`, fused into a dense TSDF of `resolution` voxels along the longest
        side (voxel_size = extent / resolution, sdf_trunc = 5 voxel_size: the task's 2 / 512 and 10 / 512), marching cubes.  Renders
        in eval mode, at most 16 views in flight.  min_component_faces drops the connected components with fewer faces (TSDF
        floaters) and target_faces decimates what is left (meshsimplify.keep_components, then simplify_mesh); with both None the
        marching-cubes mesh is returned as it is."""
        from .cameras import sphere_cameras
        from .fusion import MAX_VIEWS, TSDFVolume
        lo, hi = bounds
        center = tuple(0.5 * (float(a) + float(b)) for a, b in zip(lo, hi))
        cams = sphere_cameras(num_views, radius, image_size, image_size, center=center, up=up, generator=generator)
        volume = TSDFVolume(int(resolution), bounds=bounds, device=self.gaussians.device)   # sdf_trunc defaults to 5 voxels
        was_training = self.training
        self.eval()
        try:
            for first in range(0, num_views, MAX_VIEWS):
                batch = [c.to(self.gaussians.device) for c in cams[first:first + MAX_VIEWS]]
                volume.integrate([self.render_depth(c) for c in batch], batch, alpha_trunc=fusing_alpha_threshold)
        finally:
            self.train(was_training)
        vertices, faces = volume.extract_mesh()
        if min_component_faces is not None or target_faces is not None:
            from .meshsimplify import keep_components, simplify_mesh
            if min_component_faces is not None:
                vertices, faces, _ = keep_components(vertices, faces, min_faces=min_component_faces)
            if target_faces is not None:
                vertices, faces, _ = simplify_mesh(vertices, faces, target_faces)
        return vertices, faces

    def render_mesh(self, cameras, vertices: Tensor, faces: Tensor, **kw):
        """A mesh of this model (what extract_mesh returned) seen from `cameras` (a Camera or a sequence): meshrender.render_mesh per
        camera -> a dict of maps ('depth', 'normal', 'alpha', 'face', 'rast'), or a list of them; its depth compares with
        render_depth's.  antialias=True (and topology=mesh_edge_topology(faces), to build it once) blends the outline, meshrender.antialias.
        outputs=(..., 'color') with kd=, ks=, uvs=, envmap=, occlusion=, min_visibility=, bend_back_normal= shades it (meshshade.py)."""
        from .meshrender import render_mesh
        if isinstance(cameras, Camera):
            return render_mesh(vertices, faces, cameras, **kw)
        return [render_mesh(vertices, faces, c, **kw) for c in cameras]

    @torch.no_grad()
    def update_grad_norm(self) -> None:
        """:360-374 on gs_densify_stats"""
        assert self.update_info is not None
        info, g = self.update_info, self.gaussians
        grad = info.xys.grad
        assert grad is not None, "update_grad_norm needs a backward pass through the last render"
        if g.xys_grad_norm is None:
            g.xys_grad_norm = torch.zeros(len(g), device=g.device)
            g.vis_counts = torch.ones(len(g), device=g.device)
            g.last_width, g.last_height = info.last_width, info.last_height
        densify_stats(info.indices, grad, g.xys_grad_norm, g.vis_counts)


def densify_stats(gaussian_ids: Tensor, v_means2d: Tensor, xys_grad_norm: Tensor, vis_counts: Tensor) -> None:
    """xys_grad_norm[ids] += |v_means2d|, vis_counts[ids] += 1 in place (gs_densify_stats); ids unique within a call."""
    _lib.require_cuda(gaussian_ids, v_means2d, xys_grad_norm, vis_counts)
    ids = gaussian_ids.reshape(-1).to(torch.int64).contiguous()
    grad = v_means2d.detach().reshape(-1, 2).float().contiguous()
    if grad.shape[0] != ids.shape[0] or xys_grad_norm.shape != vis_counts.shape or xys_grad_norm.dtype != torch.float32 or \
            vis_counts.dtype != torch.float32:
        raise _lib.GeoSplatHipError("densify_stats expects ids[V], v_means2d[V,2] and fp32 xys_grad_norm[N], vis_counts[N]")
    _lib.check(_lib.lib().gs_densify_stats(int(ids.shape[0]), _lib.ptr(ids), _lib.ptr(grad), xys_grad_norm.numel(),
                                           _lib.ptr(xys_grad_norm), _lib.ptr(vis_counts), _lib.stream()), "gs_densify_stats")


# ------------------------------------------------------------------------------------------------ the trainer
def refine_schedule(curr_step: int, *, warmup_length: int, refine_every: int, reset_alpha_every: int, stop_split_at: int,
                    dataset_size: int, continue_cull_post_densification: bool = True) -> Dict[str, bool]:
    """The gates of GSplatTrainer.after_update at a step (rfstudio/trainer/gsplat_trainer.py:178-225), pure arithmetic:
    `refine` (a refinement step: the statistics are cleared at its end), and inside it `densify`, `cull` (post-densification),
    `reset` (opacity reset) and `scale_cull` (cull_scale_thresh applies; None before)."""
    refine = curr_step > warmup_length and curr_step % refine_every == 0
    reset_interval = reset_alpha_every * refine_every
    splitting = curr_step < stop_split_at
    return {"refine": refine,
            "densify": refine and splitting and curr_step % reset_interval > dataset_size + refine_every,   # every image seen since the reset
            "cull": refine and not splitting and continue_cull_post_densification,
            "reset": refine and splitting and curr_step % reset_interval == refine_every,
            "scale_cull": curr_step > refine_every * reset_alpha_every}


@dataclass
class GSplatTrainer:
    """rfstudio/trainer/gsplat_trainer.py:18-225 for the 3DGS modes."""
    base_lr: float = 1e-3
    base_eps: float = 1e-15
    pos_lr_decay: int = 4500
    warmup_length: int = 500
    refine_every: int = 100
    cull_alpha_thresh: float = 0.1
    cull_scale_thresh: float = 0.5
    continue_cull_post_densification: bool = True
    reset_alpha_every: int = 30
    densify_grad_thresh: float = 0.0002
    densify_size_thresh: float = 0.01
    num_splits: int = 2
    sh_degree_interval: int = 1000
    stop_split_at: int = 15000
    ssim_lambda: float = 0.2
    generator: Optional[torch.Generator] = None          # device generator of the split samples
    # camera-pose refinement (poseopt.CameraPoseDeltas): off by default, and then no code path or bit changes.  pose_lr / pose_reg
    # are the defaults of upstream gsplat's trainer AS REMEMBERED (pose_opt_lr = 1e-5, pose_opt_reg = 1e-6): unpinned.
    pose_opt: bool = False
    pose_lr: float = 1e-5
    pose_reg: float = 1e-6

    def setup(self, model: GSplatModel, dataset_size: int) -> Dict[str, torch.optim.Adam]:
        """:57-118: one Adam per field; the exp scheduler (half-life pos_lr_decay) on the means.  With pose_opt: one correction per
        dataset camera and one more Adam (weight_decay = pose_reg) keyed "poses" -- no Gaussian field, so densification and
        mutate_adam, which go by field name, never touch it."""
        self._dataset_size = int(dataset_size)
        g = model.gaussians
        lrs = {"means": self.base_lr * 0.16, "scales": self.base_lr * 5, "quats": self.base_lr, "colors": self.base_lr * 2.5,
               "opacities": self.base_lr * 50}
        if model.sh_degree > 0:
            lrs["shs"] = self.base_lr * 0.125
        self.optimizers = {name: torch.optim.Adam([getattr(g, name)], lr=lr, eps=self.base_eps) for name, lr in lrs.items()}
        lam = math.log(2) / self.pos_lr_decay
        self.schedulers = {"means": torch.optim.lr_scheduler.LambdaLR(self.optimizers["means"], lr_lambda=lambda s: math.exp(-lam * s))}
        self.refined: List[Tuple[int, str]] = []
        self.last_indices: Optional[Tensor] = None
        self.pose_deltas = None
        if self.pose_opt:
            from .poseopt import CameraPoseDeltas
            self.pose_deltas = CameraPoseDeltas(self._dataset_size, device=g.device)
            self.optimizers["poses"] = torch.optim.Adam(self.pose_deltas.parameters(), lr=self.pose_lr, weight_decay=self.pose_reg)
        return self.optimizers

    def step(self, model: GSplatModel, camera: Camera, gt: Tensor, camera_index: Optional[int] = None) -> Tuple[Tensor, Dict[str, object]]:
        """:120-151.  gt [H,W,4] (blended over this step's background colour, as RGBAImages.blend) or [H,W,3].  With pose_opt and a
        camera_index (the camera's place in the dataset) the render goes through that camera's corrected pose."""
        if self.pose_opt and camera_index is not None:
            camera = self.pose_deltas.camera(camera, camera_index)
        bg = model.get_background_color().to(model.gaussians.device)
        gt = gt.to(model.gaussians.device).clamp(0, 1)
        if gt.shape[-1] == 3:
            gt = torch.cat((gt, torch.ones_like(gt[..., :1])), dim=-1)
        render, alpha = model.render_layers(camera)
        train_bg = bg.expand(render.shape).contiguous()
        loss, _ = photo_loss(render, alpha, gt, train_bg=train_bg, gt_is_srgb=False, ssim_lambda=self.ssim_lambda, use_mask_loss=False)
        with torch.no_grad():
            out = render + (1 - alpha) * bg
            ref = gt[..., :3] * gt[..., 3:] + (1 - gt[..., 3:]) * bg
            psnr = -10 * (out - ref).square().mean().log10()
        return loss, {"ssim": loss.detach(), "psnr": psnr, "#gaussians": len(model.gaussians)}

    def before_update(self, model: GSplatModel, *, curr_step: int) -> None:
        model.set_max_sh_degree(curr_step // self.sh_degree_interval)

    def after_update(self, model: GSplatModel, *, curr_step: int) -> None:
        """:166-225"""
        model.set_max_sh_degree(None)
        if curr_step < self.stop_split_at:
            model.update_grad_norm()
        gate = refine_schedule(curr_step, warmup_length=self.warmup_length, refine_every=self.refine_every,
                               reset_alpha_every=self.reset_alpha_every, stop_split_at=self.stop_split_at,
                               dataset_size=self._dataset_size,
                               continue_cull_post_densification=self.continue_cull_post_densification)
        if not gate["refine"]:
            return
        scale_thresh = self.cull_scale_thresh if gate["scale_cull"] else None
        if gate["densify"]:
            self.last_indices = self._densify(model, scale_thresh)
            self.refined.append((curr_step, "densify"))
        if gate["cull"]:
            self.last_indices = model.gaussians.cull(cull_alpha_thresh=self.cull_alpha_thresh, cull_scale_thresh=scale_thresh,
                                                     optimizers=self.optimizers)
            self.refined.append((curr_step, "cull"))
        if gate["reset"]:
            model.gaussians.reset_opacities(reset_value=self.cull_alpha_thresh * 2.0)
            mutate_adam(self.optimizers["opacities"], [model.gaussians.opacities], clear=True)
            self.refined.append((curr_step, "reset"))
        model.gaussians.clear_extras_()

    def _densify(self, model: GSplatModel, scale_thresh: Optional[float]) -> Tensor:
        return model.gaussians.densify_and_cull(densify_grad_thresh=self.densify_grad_thresh, densify_size_thresh=self.densify_size_thresh,
                                                num_splits=self.num_splits, cull_alpha_thresh=self.cull_alpha_thresh,
                                                cull_scale_thresh=scale_thresh, generator=self.generator, optimizers=self.optimizers)

    def train_step(self, model: GSplatModel, camera: Camera, gt: Tensor, *, curr_step: int,
                   camera_index: Optional[int] = None) -> Tuple[Tensor, Dict[str, object]]:
        """One iteration of the reference's loop (rfstudio/engine/train.py:76-112); curr_step counts from 1."""
        for opt in self.optimizers.values():
            opt.zero_grad()
        model.train(True)
        self.before_update(model, curr_step=curr_step)
        # (a subclass's step keeps the three-argument form: the index is passed only when one was given)
        loss, metrics = self.step(model, camera, gt) if camera_index is None else self.step(model, camera, gt, camera_index)
        loss.backward()
        for opt in self.optimizers.values():
            opt.step()
        for sch in self.schedulers.values():
            sch.step()
        self.after_update(model, curr_step=curr_step)
        return loss.detach(), metrics
