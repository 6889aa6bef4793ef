"""The reference's two stage-2 models and their trainer step: Monte-Carlo shading of a lat-long light with shadow rays on the stage's
own mesh, the per-Gaussian estimates filtered by the bilateral denoiser (`RenderableAttrs.splat_mc_denoised`).

`Stage2Model.from_export(path)` is `GeoSplatterMC` (rfstudio/model/geosplat_mc.py): it continues a `Stage1Model.export_model` file --
FlexiCubes geometry, the cube map resampled to a 256 x 512 lat-long parameter, a field with the occlusion encoder, the residual light on.
`PriorModel(vertices, faces)` is `GeoSplatterPrior` (rfstudio/model/geosplat_prior.py): it starts from a mesh (for instance
`GSplatModel.extract_mesh()` of a trained 3DGS / 2DGS model) and deforms its vertices under the three mesh regularisers of
`meshreg.mesh_regularizers`, on a topology built once.  `_Stage2Base` holds what the two share: `get_gsplat`, `render_report`,
`export_model` (the stage-3 hand-off), `state_dict` and checkpoints in the style of `Stage1Model`.  `Stage2Schedule` is the two
trainers' `setup` / `before_update` / `after_update` (geosplat_mc_trainer.py:21-128, :214-251; geosplat_prior_trainer.py:22-128, :210-242)
and `train_step` their `step`: per-pixel random background, SSIM / L1 in linear space plus the mask term, the mean over the views plus the
regulariser.  Single process.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .cameras import Camera
from .envmap import EnvCubeMap
from .envshade import LatLngEnvMap
from .field import GaussianField, face_offsets
from .flexicubes import FlexiCubes, get_geometry
from .loss import photo_loss
from .meshreg import MeshRegTopology, mesh_regularizers
from .raytrace import MeshBVH
from .stage1 import configure_allocator, smoothing_regularization

_ENCODERS = ("kd_enc", "ks_enc", "z_enc", "occ_enc")


class _Stage2Base:
    """What `Stage2Model` and `PriorModel` share.  A subclass sets `residual`, provides `get_geometry()`, `_bvh(vertices, faces)`,
    `_geometry_parameters()` and `_export_head()`."""
    residual = False

    def _setup(self, dev: torch.device, *, scale: float, min_roughness: float, max_metallic: float, seed: int, log2_hashmap_size: int,
               smooth_type: str = "jitter") -> None:
        if smooth_type not in ("jitter", "grad", "tv"):
            raise ValueError(smooth_type)
        if dev.type == "cuda":
            configure_allocator()
        self.scale, self.min_roughness, self.max_metallic = float(scale), float(min_roughness), float(max_metallic)
        self.field = GaussianField(device=dev, log2_hashmap_size=log2_hashmap_size, seed=seed + 1, occ=True)
        self.initial_guess_bias = torch.zeros(2, device=dev)
        self.exposure_params = torch.zeros(1, device=dev, requires_grad=True)
        self.shadow_scale = 1.0
        self.num_samples_per_ray = 8                             # render_report's n_samples_x (2 n^2 rays per Gaussian)
        # scalar weights of __setup__; the schedule sets them
        self.sdf_weight = 0.0; self.occ_weight = 0.0; self.light_weight = 0.0
        self.kd_grad_weight = 0.0; self.kd_regualr_perturb_std = 0.0
        self.ks_grad_weight = 0.0; self.ks_regualr_perturb_std = 0.0
        self.normal_grad_weight = 0.0
        self.smooth_type = smooth_type
        self.background_color = torch.ones(3, device=dev)
        self.last_num_gaussians = 0
        self._jitter_gen = torch.Generator(device=dev).manual_seed(seed * 7919 + 17)
        self._bg_gen = torch.Generator(device=dev).manual_seed(seed * 1000003 + 29)
        self._dev, self._seed = dev, seed

    # ------------------------------------------------------------------------------------------------- parameters
    def _field_encoders(self) -> Tuple[str, ...]:
        return _ENCODERS

    def named_parameters(self) -> Dict[str, Tensor]:
        out = dict(self._geometry_parameters())
        out["latlng"] = self.latlng
        out["exposure_params"] = self.exposure_params
        for name in self._field_encoders():
            for i, p in enumerate(getattr(self.field, name).parameters()):
                out[f"field.{name}.{i}"] = p
        return out

    def parameters(self) -> List[Tensor]:
        return list(self.named_parameters().values())

    def state_dict(self) -> Dict[str, Tensor]:
        out = {k: v.detach().cpu().clone() for k, v in self.named_parameters().items() if not k.startswith("field.")}
        out["initial_guess_bias"] = self.initial_guess_bias.detach().cpu().clone()
        for name in _ENCODERS:
            for k, v in getattr(self.field, name).state_dict().items():
                out[f"field.{name}.{k}"] = v
        return out

    def load_state_dict(self, sd: Dict[str, Tensor]) -> None:
        with torch.no_grad():
            for k, p in self.named_parameters().items():
                if not k.startswith("field."):
                    p.copy_(sd[k].to(p.device))
            self.initial_guess_bias = sd["initial_guess_bias"].to(self._dev).float()
        for name in _ENCODERS:
            pre = f"field.{name}."
            getattr(self.field, name).load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})

    def save_checkpoint(self, ckpt_dir, step: int) -> str:
        """`<ckpt_dir>/<step:010d>.ckpt` = state_dict, as `Stage1Model.save_checkpoint`"""
        os.makedirs(ckpt_dir, exist_ok=True)
        path = os.path.join(ckpt_dir, f"{step:010d}.ckpt")
        torch.save(self.state_dict(), path)
        return path

    def load_checkpoint(self, ckpt_dir, step: Optional[int] = None) -> Optional[int]:
        """the given step, else the newest `*.ckpt`; None if there is none"""
        if not os.path.isdir(ckpt_dir):
            return None
        if step is None:
            steps = [int(f.rsplit(".", 1)[0]) for f in os.listdir(ckpt_dir) if f.endswith(".ckpt")]
            if not steps:
                return None
            step = max(steps)
        path = os.path.join(ckpt_dir, f"{step:010d}.ckpt")
        if not os.path.exists(path):
            return None
        self.load_state_dict(torch.load(path, map_location="cpu"))
        return step

    # ------------------------------------------------------------------------------------------------- forward pieces
    def get_envmap(self) -> LatLngEnvMap:
        return LatLngEnvMap(self.latlng).compute_pdf_()

    def _gaussians(self, v: Tensor, f: Tensor, kd_std: float, ks_std: float):
        return self.field.get_gaussians_from_face(v, f, kd_std, ks_std, scale=self.scale, initial_guess=self.initial_guess_bias,
                                                  generator=self._jitter_gen)

    def get_gsplat(self):
        """geosplat_mc.py:117-143, geosplat_prior.py:150-187 -> (mesh, splats, attrs, regularisation, offsets)"""
        (v, f), reg = self.get_geometry()
        self.last_num_gaussians = f.shape[0] * 6
        kd_std = self.kd_regualr_perturb_std if self.smooth_type == "jitter" else 0.0
        ks_std = self.ks_regualr_perturb_std if self.smooth_type == "jitter" else 0.0
        splats, attrs, offsets = self._gaussians(v, f, kd_std, ks_std)
        if kd_std > 0 and self.kd_grad_weight > 0:
            reg = reg + self.kd_grad_weight * (attrs.kd_jitter - attrs.kd).abs().mean()
        if ks_std > 0 and self.ks_grad_weight > 0:
            reg = reg + self.ks_grad_weight * (attrs.ks_jitter - attrs.ks).abs().mean()
        if self.occ_weight > 0 and attrs.occ is not None:
            reg = reg + self.occ_weight * attrs.occ.abs().mean()
        return (v, f), splats, attrs, reg, offsets

    def render_report(self, cameras: Sequence[Camera], gt_rgba: Optional[Sequence[Tensor]] = None, batch_size: Optional[int] = None,
                      rnd_seed: Optional[int] = None) -> Tuple[List[Tensor], int, Tensor]:
        """geosplat_mc.py:172-250, geosplat_prior.py:215-293 -> (tone-mapped linear RGBA per camera, #Gaussians, regularisation): one
        `splat_mc_denoised` per view on a hierarchy of this step's mesh; gt_rgba (linear RGBA per camera) is only read by the 'grad' /
        normal smoothing branches; `rnd_seed` goes to the shader (None: a fresh seed per pass)."""
        (v, f), splats, attrs, reg, offsets = self.get_gsplat()
        with torch.no_grad():
            bvh = self._bvh(v.detach(), f)
            mc_positions = (splats.means + offsets).detach()
        envmap = self.get_envmap()
        exposure = self.exposure_params.exp()[0]
        images = []
        for cam in cameras:
            img, view_reg = attrs.splat_mc_denoised(splats, [cam], bvh=bvh, exposure=exposure, positions=mc_positions, envmap=envmap,
                                                    min_roughness=self.min_roughness, max_metallic=self.max_metallic,
                                                    num_samples_per_ray=self.num_samples_per_ray, shadow_scale=self.shadow_scale,
                                                    residual=self.residual, rnd_seed=rnd_seed)
            images.append(img.reshape(cam.height, cam.width, 4))
            reg = reg + view_reg / len(cameras)
        if self.smooth_type != "jitter" or self.normal_grad_weight > 0:
            reg = reg + smoothing_regularization(self, splats, attrs, cameras, gt_rgba, batch_size or len(cameras))
        return images, splats.means.shape[0], reg

    # ------------------------------------------------------------------------------------------------- stage hand-off
    def export_model(self, path) -> None:
        """The file stage 3 starts from: the keys of geosplat_mc.py:148-169 / geosplat_prior.py:192-212"""
        with torch.no_grad():
            (v, f), splats, attrs, _, offsets = self.get_gsplat()
            cpu = lambda t: None if t is None else t.detach().cpu().clone()
            attributes = dict(self._export_head())
            attributes.update({
                "min_roughness": self.min_roughness,
                "max_metallic": self.max_metallic,
                "exposure": cpu(self.exposure_params),
                "latlng": cpu(self.latlng),
                "means": cpu(splats.means), "scales": cpu(splats.scales), "quats": cpu(splats.quats), "opacities": cpu(splats.opacities),
                "normals": cpu(attrs.normals), "kd": cpu(attrs.kd), "ks": cpu(attrs.ks), "occ": cpu(attrs.occ),
                "ks_enc": self.field.ks_enc.state_dict(),
                "occ_enc": self.field.occ_enc.state_dict(),
                "mc_positions": cpu(splats.means + offsets),
                "mc_vertices": cpu(v),
                "mc_indices": f.detach().cpu().to(torch.int32),
                "initial_guess": cpu(self.initial_guess_bias),
            })
        torch.save(attributes, path)


class Stage2Model(_Stage2Base):
    """`GeoSplatterMC`: stage-1 FlexiCubes geometry under the Monte-Carlo shader, with the residual light.  Built by `from_export`."""
    residual = True

    def __init__(self, resolution: int, *, scale: float, min_roughness: float = 0.1, max_metallic: float = 1.0, device="cuda",
                 seed: int = 0, log2_hashmap_size: int = 18, smooth_type: str = "jitter"):
        dev = torch.device(device)
        self._setup(dev, scale=scale, min_roughness=min_roughness, max_metallic=max_metallic, seed=seed,
                    log2_hashmap_size=log2_hashmap_size, smooth_type=smooth_type)
        self.resolution = int(resolution)
        self.grid = FlexiCubes.from_resolution(self.resolution, device=dev, random_sdf=False, scale=self.scale)
        V, Cn = self.grid.vertices.shape[0], self.resolution ** 3
        self.sdf_params = torch.zeros(V, 1, device=dev, requires_grad=True)
        self.deform_params = torch.zeros(V, 3, device=dev, requires_grad=True)
        self.weight_params = torch.zeros(Cn, 21, device=dev, requires_grad=True)
        self.latlng = torch.full((256, 512, 3), 0.5, device=dev, requires_grad=True)

    @classmethod
    def from_export(cls, path, device="cuda", **kwargs) -> "Stage2Model":
        """`GeoSplatterMC.__setup__` (geosplat_mc.py:56-83) on a `Stage1Model.export_model` file: geometry, exposure and the ks encoder
        are loaded, the cube map becomes the lat-long parameter `EnvCubeMap(cubemap).as_latlng(512, 256).data`; the kd, z and occlusion
        encoders start fresh."""
        a = torch.load(path, map_location="cpu")
        log2 = int(round(math.log2(a["ks_enc"]["encoder.params"].shape[0] / 16.0)))
        m = cls(int(a["resolution"]), scale=float(a["geom_scale"]), min_roughness=float(a["min_roughness"]),
                max_metallic=float(a["max_metallic"]), device=device, log2_hashmap_size=log2, **kwargs)
        dev = m._dev
        with torch.no_grad():
            m.exposure_params.copy_(a["exposure"].to(dev))
            m.deform_params.copy_(a["deforms"].to(dev))
            m.weight_params.copy_(a["weights"].to(dev))
            m.sdf_params.copy_(a["sdfs"].to(dev))
            m.initial_guess_bias = a["initial_guess"].to(dev).float()
            latlng = EnvCubeMap(a["cubemap"].to(dev).float().contiguous()).as_latlng(512, 256).data
        m.latlng = latlng.detach().clone().requires_grad_(True)
        m.field.ks_enc.load_state_dict(a["ks_enc"])
        return m

    def _geometry_parameters(self) -> Dict[str, Tensor]:
        return {"sdf_params": self.sdf_params, "deform_params": self.deform_params, "weight_params": self.weight_params}

    def _export_head(self) -> Dict[str, object]:
        return {"geom_scale": self.scale, "resolution": self.resolution}

    def get_geometry(self):
        """geosplat_mc.py:85-103: stage 1's, with `sdf_weight`"""
        return get_geometry(self.grid, self.deform_params, self.sdf_params, self.weight_params, scale=self.scale,
                            resolution=self.resolution, sdf_weight=self.sdf_weight)

    def _bvh(self, vertices: Tensor, faces: Tensor) -> MeshBVH:
        return MeshBVH(vertices.contiguous(), faces)              # the face count changes from step to step: a new hierarchy


class PriorModel(_Stage2Base):
    """`GeoSplatterPrior`: a given mesh whose vertices move by `deform_params` under
    reg = 1e-3 lap + 3e-4 nc + 0.1 edge + 0.1 mean(|deform|^2) (`meshreg.mesh_regularizers`; geosplat_prior.py:123-136).  With
    smooth_type 'jitter' the appearance comes from the field; otherwise from per-Gaussian parameters `kdks_params` [6F,5] and
    `zs_params` [6F,1] (:106-111, :170-178), the field's encoders are not parameters, and `attrs.occ` is None."""
    residual = False

    def __init__(self, vertices: Tensor, faces: Tensor, scale: float = 1.0, min_roughness: float = 0.1, max_metallic: float = 1.0,
                 smooth_type: str = "jitter", *, seed: int = 0, log2_hashmap_size: int = 18):
        from . import _lib
        _lib.require_cuda(vertices, faces)
        dev = vertices.device
        self._setup(dev, scale=scale, min_roughness=min_roughness, max_metallic=max_metallic, seed=seed,
                    log2_hashmap_size=log2_hashmap_size, smooth_type=smooth_type)
        self.vertices = vertices.detach().float().contiguous().clone()
        self.faces = faces.detach().long().contiguous().clone()
        self.topology = MeshRegTopology(self.faces, self.vertices.shape[0])           # once: the faces never change
        self.deform_params = torch.zeros_like(self.vertices, requires_grad=True)
        self.latlng = torch.full((256, 512, 3), 0.5, device=dev, requires_grad=True)
        if smooth_type != "jitter":
            self.kdks_params = torch.zeros(self.faces.shape[0] * 6, 5, device=dev, requires_grad=True)
            self.zs_params = torch.zeros(self.faces.shape[0] * 6, 1, device=dev, requires_grad=True)
        self._hierarchy: Optional[MeshBVH] = None

    def _field_encoders(self) -> Tuple[str, ...]:
        return _ENCODERS if self.smooth_type == "jitter" else ()

    def _geometry_parameters(self) -> Dict[str, Tensor]:
        out = {"deform_params": self.deform_params}
        if self.smooth_type != "jitter":
            out.update(kdks_params=self.kdks_params, zs_params=self.zs_params)
        return out

    def _export_head(self) -> Dict[str, object]:
        return {"geom_scale": self.scale}

    def get_geometry(self):
        v = self.vertices + self.deform_params
        lap, edge, nc = mesh_regularizers(v, self.topology)
        offset = self.deform_params.square().sum(-1).mean()
        return (v, self.faces), lap * 1e-3 + nc * 3e-4 + edge * 0.1 + offset * 0.1

    def _gaussians(self, v: Tensor, f: Tensor, kd_std: float, ks_std: float):
        if self.smooth_type == "jitter":
            return super()._gaussians(v, f, kd_std, ks_std)
        from .mesh import mesh_to_splats, vertex_normals
        from .shading import RenderableAttrs
        from .splats import SplatSet
        splats, shading_normals = mesh_to_splats(v, f, vertex_normals(v, f))
        offsets = face_offsets(v, f) * self.zs_params.sigmoid()
        attrs = RenderableAttrs(kd=self.kdks_params[..., :3].sigmoid(), ks=(self.kdks_params[..., 3:] + self.initial_guess_bias).sigmoid(),
                                normals=shading_normals)
        return SplatSet(splats.means - offsets, splats.scales, splats.quats, splats.opacities, splats.colors), attrs, offsets

    def _bvh(self, vertices: Tensor, faces: Tensor) -> MeshBVH:
        if self._hierarchy is None:
            self._hierarchy = MeshBVH(vertices.contiguous(), faces)
            return self._hierarchy
        return self._hierarchy.rebuild(vertices.contiguous())      # same faces, moved vertices (the reference's rebuild=1)


@dataclass
class Stage2Schedule:
    """`setup` / `before_update` / `after_update` and the learning-rate table of the reference's two stage-2 trainers as plain host
    code.  The defaults are `GeoSplatMCTrainer`'s (geosplat_mc_trainer.py:21-46); `Stage2Schedule.prior()` gives
    `GeoSplatPriorTrainer`'s (geosplat_prior_trainer.py:22-43)."""
    cov3d_lr: float = 3e-3
    geometry_lr: float = 3e-3
    appearance_lr: float = 1e-2
    light_lr: float = 1e-2
    ks_lr_factor: float = 0.2                  # the ks encoder's share of appearance_lr
    geometry_warm_up: Optional[int] = 50
    base_decay: Optional[int] = 800            # half-life of every learning rate, in steps
    base_eps: float = 1e-15
    sdf_reg_begin: float = 0.2
    sdf_reg_end: float = 0.01
    sdf_reg_decay: int = 500
    kd_grad_reg_begin: float = 0.03
    kd_grad_reg_end: float = 0.03
    kd_grad_reg_decay: int = 250
    kd_regualr_perturb_std: float = 0.01
    ks_grad_reg_begin: float = 0.03
    ks_grad_reg_end: float = 0.03
    ks_grad_reg_decay: int = 250
    ks_regualr_perturb_std: float = 0.01
    normal_grad_reg_begin: float = 0.03
    normal_grad_reg_end: float = 0.03
    normal_grad_reg_decay: int = 0
    occ_weight: float = 1e-3
    light_gradient_scale: float = 64.0
    latlng_floor: float = 1e-2

    @classmethod
    def prior(cls, **kw) -> "Stage2Schedule":
        base = dict(cov3d_lr=1e-3, geometry_lr=1e-4, ks_lr_factor=1.0, geometry_warm_up=None, sdf_reg_decay=0, ks_grad_reg_begin=0.01,
                    ks_grad_reg_end=0.01)
        base.update(kw)
        return cls(**base)

    @staticmethod
    def _ramp(begin: float, end: float, t: float) -> float:
        return begin - (begin - end) * min(1.0, t)

    def learning_rates(self, model) -> Dict[str, Tuple[List[Tensor], float, Optional[int]]]:
        """{group: (parameters, learning rate, warm-up steps)}: the `optim_dict` of the trainer that fits the model"""
        groups: Dict[str, Tuple[List[Tensor], float, Optional[int]]] = {}
        geo = self.geometry_warm_up
        for name, key in (("deforms", "deform_params"), ("weights", "weight_params"), ("sdfs", "sdf_params")):
            if hasattr(model, key):
                groups[name] = ([getattr(model, key)], self.geometry_lr, geo)
        groups["exposure"] = ([model.exposure_params], self.light_lr * 0.5, None)
        groups["light"] = ([model.latlng], self.light_lr, None)
        if model.smooth_type == "jitter" or not isinstance(model, PriorModel):
            groups["kd"] = (model.field.kd_enc.parameters(), self.appearance_lr, None)
            groups["occ"] = (model.field.occ_enc.parameters(), self.appearance_lr, None)
            groups["ks"] = (model.field.ks_enc.parameters(), self.appearance_lr * self.ks_lr_factor, None)
            groups["z"] = (model.field.z_enc.parameters(), self.cov3d_lr, None)
        else:
            groups["kdks"] = ([model.kdks_params], self.appearance_lr * 3, None)
            groups["zs"] = ([model.zs_params], self.cov3d_lr, None)
        return groups

    def lr_factor(self, step: int, warm_up: Optional[int]) -> float:
        """the reference's exponential schedule (rfstudio/optim/optimizer.py:23-31): (step / warm_up)^2 during the warm-up, then a
        half-life of `base_decay` steps"""
        if warm_up is not None:
            if step < warm_up:
                return (step / warm_up) ** 2
            if self.base_decay is None:
                return 1.0
        if self.base_decay is None:
            return 1.0
        return math.exp(-math.log(2.0) / self.base_decay * (step - (warm_up or 0)))

    def setup(self, model) -> Dict[str, torch.optim.Adam]:
        """`setup`: `occ_weight`, and one Adam per group of `learning_rates` (the x64 of the light's gradient is `scale_light_gradient`)"""
        model.occ_weight = self.occ_weight
        self._groups = self.learning_rates(model)
        return {name: torch.optim.Adam(params, lr=lr, eps=self.base_eps) for name, (params, lr, _) in self._groups.items()}

    def before_update(self, model, curr_step: int, optimizers: Optional[Dict[str, torch.optim.Adam]] = None) -> None:
        if self.sdf_reg_decay > 0:
            model.sdf_weight = self._ramp(self.sdf_reg_begin, self.sdf_reg_end, curr_step / self.sdf_reg_decay)
        if self.kd_grad_reg_decay > 0:
            model.kd_grad_weight = self._ramp(self.kd_grad_reg_begin, self.kd_grad_reg_end, curr_step / self.kd_grad_reg_decay)
            model.kd_regualr_perturb_std = self.kd_regualr_perturb_std
        if self.ks_grad_reg_decay > 0:
            model.ks_grad_weight = self._ramp(self.ks_grad_reg_begin, self.ks_grad_reg_end, curr_step / self.ks_grad_reg_decay)
            model.ks_regualr_perturb_std = self.ks_regualr_perturb_std
        if self.normal_grad_reg_decay > 0:
            model.normal_grad_weight = self._ramp(self.normal_grad_reg_begin, self.normal_grad_reg_end,
                                                  curr_step / self.normal_grad_reg_decay)
        if optimizers is not None:
            for name, opt in optimizers.items():
                _, lr, warm_up = self._groups[name]
                for group in opt.param_groups:
                    group["lr"] = lr * self.lr_factor(curr_step, warm_up)

    def scale_light_gradient(self, model) -> None:
        """setup's `model.latlng.register_hook(lambda g: g * 64)`, applied to the finished gradient"""
        if model.latlng.grad is not None:
            model.latlng.grad.mul_(self.light_gradient_scale)

    def after_update(self, model, curr_step: int) -> None:
        with torch.no_grad():
            model.latlng.clamp_min_(self.latlng_floor)


def train_step(model: _Stage2Base, cameras: Sequence[Camera], gt_rgba: Sequence[Tensor], *, gt_is_srgb: bool = True,
               use_mask_loss: bool = True, bg_generator: Optional[torch.Generator] = None, train_bg: Optional[Sequence[Tensor]] = None,
               rnd_seed: Optional[int] = None) -> Dict[str, Tensor]:
    """One `GeoSplatMCTrainer.step` / `GeoSplatPriorTrainer.step` + backward over `cameras` (geosplat_mc_trainer.py:134-212): leaves
    d(mean view loss + regularisation) / d(parameter) in every parameter's .grad.  train_bg: fixed per-view backgrounds instead of the
    trainer's torch.rand_like; rnd_seed: a fixed shader seed (tests).  A view that outgrew the intersection capacity repeats the step
    (`viewbatch.retry_on_capacity`).  Returns detached metrics."""
    from .viewbatch import retry_on_capacity
    n = len(cameras)
    gen = model._bg_gen if bg_generator is None else bg_generator

    def attempt():
        for p in model.parameters():
            p.grad = None
        images, num_gaussians, reg = model.render_report(cameras, gt_rgba, batch_size=n, rnd_seed=rnd_seed)
        total, losses = reg, []
        for i, img in enumerate(images):
            bg = train_bg[i] if train_bg is not None else torch.rand(img.shape[0], img.shape[1], 3, device=img.device, generator=gen)
            loss, _ = photo_loss(img[..., :3], img[..., 3:], gt_rgba[i], bg, gt_is_srgb=gt_is_srgb, use_mask_loss=use_mask_loss)
            losses.append(loss.detach())
            total = total + loss / n
        total.backward()
        return num_gaussians, reg, losses
    num_gaussians, reg, losses = retry_on_capacity(attempt)()
    for p in model.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    return {"loss": torch.stack(losses).mean(), "regularization": reg.detach(), "#gaussians": torch.tensor(num_gaussians),
            "exposure": model.exposure_params.detach().exp().mean()}
