"""The reference's stage-3 model, its trainer step and its relighting evaluation: deferred Monte-Carlo shading
(`RenderableAttrs.splat_mc_deferred`) of free per-Gaussian materials on the frozen mesh that stage 2 exported.

`Stage3Model.from_export(path)` is `GeoSplatterDefer` (rfstudio/model/geosplat_defer.py): it continues a `Stage2Model.export_model` /
`PriorModel.export_model` file.  The Gaussians, their normals, the exported kd / occ (now free parameters, no longer a field), the
exposure, the ks encoder and the light (as hue and log-value) are learned; the mesh only casts shadows and gives the surface points,
so its hierarchy is built once.  `Stage3Schedule` is `GeoSplatDeferTrainer.setup / before_update / after_update`
(rfstudio/trainer/geosplat_defer_trainer.py) as plain host code and `train_step` its `step` + backward.  `albedo_scaling` and
`evaluate_relighting` are the `RelightEvaler` task (tests/model/test_geosplat_defer.py:345-493): NVS, relighting and albedo PSNR.

No kernel of its own: every device pass is one of the package's existing ops.  A training view makes two compositor passes (the
14-channel G-buffer and ONE 6-channel pass for both edge-aware terms, where the reference renders kd and the normals separately) and
`material_maps` one 9-channel pass (the reference: three 3-channel renders).  Single process.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .cameras import Camera
from .envmap import EnvCubeMap, load_hdr
from .envshade import LatLngEnvMap, require_baked
from .field import HashEncoding
from .loss import photo_loss
from .raytrace import MeshBVH
from .stage1 import _edge_aware, configure_allocator

_LEARNED = ("means", "scales", "quats", "opacities", "normals", "kd_params", "occ_params", "exposure_params", "latlng_hue",
            "latlng_value")
_BACKGROUNDS = ("random", "black", "white")
_EVAL_BACKGROUND = (0.1490, 0.1647, 0.2157)


# ------------------------------------------------------------------------------------------------------- small pure functions
def light_to_params(latlng: Tensor) -> Tuple[Tensor, Tensor]:
    """geosplat_defer.py:81-82: a radiance map L -> (hue, value) = (L / (L + 1), log(L + 1.00001))"""
    return latlng / (latlng + 1), (latlng + 1.00001).log()


def light_from_params(hue: Tensor, value: Tensor) -> Tensor:
    """geosplat_defer.py:112: hue * exp(value) = L (L + 1.00001) / (L + 1), which is L + L * 1e-5 / (L + 1)"""
    return hue * value.exp()


def linear_to_srgb(x: Tensor) -> Tensor:
    """The piecewise sRGB curve of `rgb2srgb` (rfstudio/graphics/_images.py:165-182; geosplat_defer.py:255-259)"""
    return torch.where(x <= 0.0031308, x * 12.92, torch.clamp(x, min=0.0031308).pow(1.0 / 2.4) * 1.055 - 0.055)


def srgb_to_linear(x: Tensor) -> Tensor:
    """`srgb2rgb` (rfstudio/graphics/_images.py:139-156)"""
    return torch.where(x <= 0.04045, x / 12.92, torch.pow((x.clamp_min(0.04045) + 0.055) / 1.055, 2.4))


def _render_channels(means: Tensor, log_scales: Tensor, quats: Tensor, logit_opacities: Tensor, colors: Tensor, camera: Camera,
                     background_color: Tensor) -> Tuple[Tensor, Tensor]:
    """`GSplatter.render_rgb` for D = 3k channels in one compositor pass -> ([H,W,D] over the background colour repeated k times,
    alpha [H,W,1]).  The one un-shaded render of this module: the regulariser and `material_maps` go through it."""
    from .shading import _rasterize_activated
    if colors.shape[-1] % 3:
        raise ValueError(f"colors must have a multiple of 3 channels, got {colors.shape[-1]}")
    render, alpha, _ = _rasterize_activated(means, log_scales, quats, logit_opacities, colors, camera, "RGB")
    bg = background_color.to(render).repeat(colors.shape[-1] // 3)
    return (render + (1 - alpha) * bg).squeeze(0), alpha.squeeze(0)


# ------------------------------------------------------------------------------------------------------------------ the model
class Stage3Model:
    """`GeoSplatterDefer`.  Built by `from_export`; `training` (default True) only selects the 'random' background.

    Learned (leaf tensors): means, scales, quats, opacities, normals, kd_params [N,3], occ_params [N,6], exposure_params, the `ks_enc`
    hash encoder and the light as latlng_hue = L / (L + 1) and latlng_value = log(L + 1.00001).  Frozen: mesh_v, mesh_i, mesh_pos,
    initial_guess and the scalars scale, min_roughness, max_metallic.  The scalar weights kd_weight, ks_weight, normal_weight are set
    by the schedule.  `generator` feeds the ks jitter and the 'random' background, in that order within a `render_report`."""

    def __init__(self, attributes: Dict[str, object], device="cuda", *, background_color: str = "random", gt_envmap=None, seed: int = 0):
        a = attributes
        if background_color not in _BACKGROUNDS:
            raise ValueError(f"background_color must be one of {_BACKGROUNDS}, got {background_color!r}")
        if "vertices" in a and "indices" in a:
            mesh_v, mesh_i, mesh_pos = a["vertices"], a["indices"], a["means"]              # geosplat_defer.py:62-66
        elif "mc_vertices" in a and "mc_indices" in a and "mc_positions" in a:
            mesh_v, mesh_i, mesh_pos = a["mc_vertices"], a["mc_indices"], a["mc_positions"]   # :67-71, a stage-2 export
        else:
            raise ValueError("the export has no mesh: it needs 'mc_vertices' / 'mc_indices' / 'mc_positions' (Stage2Model / PriorModel"
                             ".export_model) or 'vertices' / 'indices'")
        if a.get("occ") is None:
            raise ValueError("the export's 'occ' is None (a PriorModel with smooth_type != 'jitter' writes such a file): stage 3 needs "
                             "the six occlusion channels per Gaussian, the G-buffer of splat_mc_deferred has 14 channels")
        dev = torch.device(device)
        if dev.type == "cuda":
            configure_allocator()
        self._dev, self._seed = dev, seed
        leaf = lambda t: t.detach().to(dev).float().contiguous().clone().requires_grad_(True)
        frozen = lambda t: t.detach().to(dev).float().contiguous().clone()
        self.means, self.scales, self.quats = leaf(a["means"]), leaf(a["scales"]), leaf(a["quats"])
        self.opacities, self.normals = leaf(a["opacities"]), leaf(a["normals"])
        self.kd_params, self.occ_params = leaf(a["kd"]), leaf(a["occ"])
        self.exposure_params = leaf(a["exposure"])
        hue, value = light_to_params(frozen(a["latlng"]))
        self.latlng_hue, self.latlng_value = hue.requires_grad_(True), value.requires_grad_(True)
        log2 = int(round(math.log2(a["ks_enc"]["encoder.params"].shape[0] / 16.0)))          # as Stage2Model.from_export
        self.ks_enc = HashEncoding([-1, 32, 2], activation="none", max_res=4096, log2_hashmap_size=log2, grad_scaling=16.0,
                                   device=dev, seed=seed + 1)
        self.ks_enc.load_state_dict(a["ks_enc"])
        self.mesh_v, self.mesh_pos = frozen(mesh_v), frozen(mesh_pos)
        self.mesh_i = mesh_i.detach().to(dev).long().contiguous().clone()
        self.initial_guess = frozen(a["initial_guess"])
        self.scale = float(a["geom_scale"])
        self.min_roughness, self.max_metallic = float(a["min_roughness"]), float(a.get("max_metallic", 1))
        self.background_color = background_color
        self.training = True
        self.kd_weight = 0.0; self.ks_weight = 0.0; self.normal_weight = 0.0
        self.shadow_scale = 1.0
        self.num_samples_per_ray = 16                            # splat_mc_deferred's n_samples_x (geosplat_defer.py:222)
        self.albedo_scaling: Optional[Tensor] = None
        self._fixed_envmap: Optional[LatLngEnvMap] = None
        self._hierarchy: Optional[MeshBVH] = None
        self.generator = torch.Generator(device=dev).manual_seed(seed * 7919 + 17)
        self._bg_gen = torch.Generator(device=dev).manual_seed(seed * 1000003 + 29)
        if gt_envmap is not None:                                # a given light from the start: nothing of the materials changes
            self._fixed_envmap = self._resolve_envmap(gt_envmap)

    @classmethod
    def from_export(cls, path, device="cuda", *, background_color: str = "random", gt_envmap=None, seed: int = 0) -> "Stage3Model":
        """`GeoSplatterDefer.__setup__` (geosplat_defer.py:54-93) on a `Stage2Model.export_model` / `PriorModel.export_model` file.
        ValueError for a file whose `occ` is None or that has no mesh."""
        return cls(torch.load(path, map_location="cpu"), device, background_color=background_color, gt_envmap=gt_envmap, seed=seed)

    # ------------------------------------------------------------------------------------------------- parameters
    def named_parameters(self) -> Dict[str, Tensor]:
        out = {name: getattr(self, name) for name in _LEARNED}
        for i, p in enumerate(self.ks_enc.parameters()):
            out[f"ks_enc.{i}"] = p
        return out

    def parameters(self) -> List[Tensor]:
        return list(self.named_parameters().values())

    def state_dict(self) -> Dict[str, Tensor]:
        """The learned tensors and `initial_guess`; the frozen mesh stays with the export the model was built from"""
        out = {name: getattr(self, name).detach().cpu().clone() for name in _LEARNED}
        out["initial_guess"] = self.initial_guess.detach().cpu().clone()
        for k, v in self.ks_enc.state_dict().items():
            out[f"ks_enc.{k}"] = v
        return out

    def load_state_dict(self, sd: Dict[str, Tensor]) -> None:
        with torch.no_grad():
            for name in _LEARNED:
                getattr(self, name).copy_(sd[name].to(self._dev))
            self.initial_guess = sd["initial_guess"].to(self._dev).float()
        self.ks_enc.load_state_dict({k[len("ks_enc."):]: v for k, v in sd.items() if k.startswith("ks_enc.")})

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

    # ------------------------------------------------------------------------------------------------- light and background
    def get_background_color(self) -> Tensor:
        """geosplat_defer.py:95-102, on the model's device: 'random' draws from `generator` while `training`"""
        if self.background_color == "black":
            return torch.zeros(3, device=self._dev)
        if self.background_color == "white":
            return torch.ones(3, device=self._dev)
        if self.background_color != "random":
            raise ValueError(f"background_color must be one of {_BACKGROUNDS}, got {self.background_color!r}")
        if self.training:
            return torch.rand(3, device=self._dev, generator=self.generator)
        return torch.tensor(_EVAL_BACKGROUND, device=self._dev)

    def _resolve_envmap(self, envmap) -> LatLngEnvMap:
        if isinstance(envmap, EnvCubeMap):
            with torch.no_grad():
                envmap = EnvCubeMap(envmap.data.detach().to(self._dev).float().contiguous(), envmap.transform).as_latlng(512, 256)
        elif not isinstance(envmap, LatLngEnvMap):
            envmap = LatLngEnvMap(load_hdr(envmap))
        require_baked(envmap, "Stage3Model")
        return LatLngEnvMap(envmap.data.detach().to(self._dev).float().contiguous()).compute_pdf_()

    @property
    def learned_light(self) -> bool:
        return self._fixed_envmap is None

    def set_relight_envmap(self, envmap, albedo_scaling: Tensor) -> None:
        """geosplat_defer.py:104-108: render under a given light from here on.  `envmap`: a `LatLngEnvMap`, an `EnvCubeMap`
        (resampled with `as_latlng(512, 256)`, :114-119) or the path of a lat-long `.hdr` picture; its sampling tables are built here,
        once.  `albedo_scaling` [3] multiplies kd; with it set, occ becomes mean(occ) * (1, kd) and the exposure 1 (`render_report`)."""
        albedo_scaling = torch.as_tensor(albedo_scaling, dtype=torch.float32)
        if tuple(albedo_scaling.shape) != (3,):
            raise ValueError(f"albedo_scaling must be a 3-vector, got {tuple(albedo_scaling.shape)}")
        self._fixed_envmap = self._resolve_envmap(envmap)
        self.albedo_scaling = albedo_scaling.detach().to(self._dev)

    def clear_relight_envmap(self) -> None:
        """back to the learned light, the unscaled kd, the learned occ and exposure"""
        self._fixed_envmap, self.albedo_scaling = None, None

    def get_envmap(self) -> LatLngEnvMap:
        """geosplat_defer.py:110-120"""
        if self._fixed_envmap is not None:
            return self._fixed_envmap
        return LatLngEnvMap(light_from_params(self.latlng_hue, self.latlng_value)).compute_pdf_()

    # ------------------------------------------------------------------------------------------------- forward pieces
    def bvh(self) -> MeshBVH:
        """The hierarchy of the frozen mesh, built on first use (the mesh never moves in this stage)"""
        if self._hierarchy is None:
            with torch.no_grad():
                self._hierarchy = MeshBVH(self.mesh_v, self.mesh_i)
        return self._hierarchy

    def get_gsplat(self):
        """geosplat_defer.py:122-138 -> SplatSet whose colours are the unit normals"""
        from .meshrender import _unit_or_z as safe_normalize
        from .splats import SplatSet
        return SplatSet(self.means, self.scales, self.quats, self.opacities, safe_normalize(self.normals))

    def ks_at(self, positions: Tensor) -> Tensor:
        """sigmoid(ks_enc(clamp(positions / scale, -1, 1)) + initial_guess) [N,2]: (roughness, metallic) before modulation"""
        return (self.ks_enc((positions / self.scale).clamp(-1, 1)) + self.initial_guess).sigmoid()

    def _materials(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(kd, ks, occ) as `render_report` shades them (geosplat_defer.py:163-175): under a relight map occ is formed from the
        UNSCALED kd, then kd is scaled"""
        kd, occ = self.kd_params, self.occ_params
        ks = self.ks_at(self.means)
        if self.albedo_scaling is not None:
            occ = self.occ_params.mean(-1, keepdim=True) * torch.cat((torch.ones_like(kd), kd), dim=-1)
            kd = kd * self.albedo_scaling
        return kd, ks, occ

    def surface(self, camera: Camera, *, near_clip: bool = False) -> Tuple[Tensor, Tensor]:
        """-> (positions [H,W,3], mask [H,W,1]): the first visible layer of the frozen mesh, `rasterize_mesh` + `interpolate(mesh_v)`,
        mask = 1 where a face covers the pixel -- what `dr.DepthPeeler(...).rasterize_next_layer()` + `dr.interpolate` give at
        geosplat_defer.py:202-209.  No gradient.  By default a face that crosses the near plane is dropped whole and leaves a hole in
        both maps; `near_clip=True` clips it instead, for a camera that stands inside the mesh (the far
        plane and images wider than the guard band are not clipped)."""
        from .meshrender import interpolate, rasterize_mesh, to_camera_space
        with torch.no_grad():
            rast = rasterize_mesh(to_camera_space(self.mesh_v, camera), self.mesh_i, camera, near_clip=near_clip)
            return interpolate(self.mesh_v, rast, self.mesh_i), (rast[..., -1:] > 0).float()

    def render_report(self, cameras: Sequence[Camera], gt_rgba: Optional[Sequence[Tensor]] = None, *, rnd_seed: Optional[int] = None,
                      denoise: bool = False) -> Tuple[List[Tensor], Tensor, int]:
        """geosplat_defer.py:152-242 -> (tone-mapped linear RGBA [H,W,4] per camera, regularisation, #Gaussians).

        Once per call: ks at the means and at means + 0.01 randn (one draw from `generator`); ks_reg = ks_weight mean|ks - ks_jitter|.
        Per camera: `splat_mc_deferred` at `surface(camera)` with num_samples_per_ray, shadow_scale, residual=True, tone 'naive' and
        exposure exp(exposure_params) -- or, under a relight map, exposure 1, kd * albedo_scaling and occ = mean(occ) (1, kd).
        Per camera with a ground truth gt_rgba[i] (linear RGBA) and kd_weight or normal_weight non-zero: ONE 6-channel un-shaded pass
        of (kd, normals * 0.5 + 0.5) over `get_background_color()` (drawn per view) with the opacities as they are -- the reference
        does not write the bent ones back --, and
            view_reg = edge_aware(kd image, gt) * kd_weight + edge_aware(normal image, gt) * normal_weight
        against gt[..., :3] * a + (1 - a).  reg = ks_reg + sum(view_reg) / len(cameras).  `rnd_seed` goes to the shader."""
        from .shading import RenderableAttrs
        splats = self.get_gsplat()
        normals = splats.colors
        envmap = self.get_envmap()
        kd, ks, occ = self._materials()
        jitter = torch.randn(self.means.shape, device=self._dev, generator=self.generator) * 0.01
        ks_reg = (ks - self.ks_at(self.means + jitter)).abs().mean() * self.ks_weight
        relit = self.albedo_scaling is not None
        exposure = torch.ones((), device=self._dev) if relit else self.exposure_params.exp()[0]
        attrs = RenderableAttrs(kd=kd, ks=ks, occ=occ, normals=normals)
        bvh = self.bvh()
        images: List[Tensor] = []
        view_regs = ks_reg.new_zeros(())
        for i, cam in enumerate(cameras):
            positions, mask = self.surface(cam)
            img, view_reg = attrs.splat_mc_deferred(splats, [cam], bvh=bvh, exposure=exposure, positions=positions, mask=mask,
                                                    envmap=envmap, min_roughness=self.min_roughness, max_metallic=self.max_metallic,
                                                    num_samples_per_ray=self.num_samples_per_ray, shadow_scale=self.shadow_scale,
                                                    denoise=denoise, residual=True, tone_type="naive", rnd_seed=rnd_seed)
            images.append(img.reshape(cam.height, cam.width, 4))
            if gt_rgba is not None and gt_rgba[i] is not None and (self.kd_weight != 0 or self.normal_weight != 0):
                gt = gt_rgba[i]
                gt_rgb = gt[..., :3] * gt[..., 3:] + (1 - gt[..., 3:])
                both, _ = _render_channels(splats.means, splats.scales, splats.quats, splats.opacities,
                                           torch.cat((kd, normals * 0.5 + 0.5), dim=-1), cam, self.get_background_color())
                view_reg = view_reg + _edge_aware(both[..., :3], gt_rgb) * self.kd_weight
                view_reg = view_reg + _edge_aware(both[..., 3:], gt_rgb) * self.normal_weight
            view_regs = view_regs + view_reg
        return images, ks_reg + view_regs / len(cameras), self.means.shape[0]

    @torch.no_grad()
    def material_maps(self, camera: Camera) -> Dict[str, Tensor]:
        """What the evaluator and a viewer read from `vis` (geosplat_defer.py:243-264), from ONE 9-channel un-shaded pass with the
        bent opacities (a Gaussian whose normal points along the view direction gets logit -2) over `get_background_color()`:
          kd       [H,W,3]  linear albedo (scaled under a relight map)        kd_srgb  the same through the sRGB curve of :255-259
          ks       [H,W,3]  (0, roughness, metallic), modulated by min_roughness / max_metallic
          direct   [H,W,3]  sigmoid(occ[:, :3] - 3), the diffuse residual light
          alpha    [H,W,1]"""
        lookat = -camera.c2w.to(self._dev)[:, 2]
        bend = (self.normals * lookat).sum(-1, keepdim=True) > 0
        opacities = torch.where(bend, torch.full_like(self.opacities, -2.0), self.opacities)
        kd, ks, occ = self._materials()
        modulated_ks = torch.cat((torch.zeros_like(ks[..., :1]), ks[..., :1] * (1 - self.min_roughness) + self.min_roughness,
                                  ks[..., 1:] * self.max_metallic), dim=-1)
        maps, alpha = _render_channels(self.means, self.scales, self.quats, opacities,
                                       torch.cat((kd, modulated_ks, (occ[..., :3] - 3).sigmoid()), dim=-1), camera,
                                       self.get_background_color())
        return {"kd": maps[..., 0:3], "kd_srgb": linear_to_srgb(maps[..., 0:3]), "ks": maps[..., 3:6], "direct": maps[..., 6:9],
                "alpha": alpha}

    def render_depth(self, cameras: Sequence[Camera]) -> List[Tensor]:
        """geosplat_defer.py:140-150 -> cat(expected depth, alpha) [H,W,2] per camera, from the Gaussians that face it"""
        from .shading import render_depth
        splats = self.get_gsplat()
        out = []
        for cam in cameras:
            visible = ((cam.c2w.to(self._dev)[:, 3] - splats.means) * splats.colors).sum(-1) > 0
            out.append(render_depth(splats.means[visible], splats.scales[visible], splats.quats[visible], splats.opacities[visible], cam))
        return out


# --------------------------------------------------------------------------------------------------------------- the schedule
@dataclass
class Stage3Schedule:
    """`setup` / `before_update` / `after_update` and the learning-rate table of `GeoSplatDeferTrainer`
    (rfstudio/trainer/geosplat_defer_trainer.py:21-126, :196-212) as plain host code."""
    base_lr: float = 1e-3
    light_lr: float = 1e-3
    base_decay: Optional[int] = 500            # half-life, in steps, of the groups that decay
    base_eps: float = 1e-15
    fix_material: bool = False
    kd_reg: float = 0.2
    ks_reg: float = 0.05
    normal_reg: float = 0.0
    light_gradient_scale: float = 64.0

    def learning_rates(self, model: Stage3Model) -> Dict[str, Tuple[List[Tensor], float, bool]]:
        """{group: (parameters, learning rate, decays)}: the trainer's `optim_dict`"""
        b, l = self.base_lr, self.light_lr
        groups = {
            "light_hue": ([model.latlng_hue], l, True),
            "light_value": ([model.latlng_value], l, True),
            "exposure": ([model.exposure_params], l * 0.5, True),
            "means": ([model.means], b * 0.16, True),
            "scales": ([model.scales], b * 5, False),
            "quats": ([model.quats], b, False),
            "normals": ([model.normals], b, True),
            "opacities": ([model.opacities], b * 50, False),
        }
        if not self.fix_material:
            groups["kd"] = ([model.kd_params], b * 5, False)
            groups["ks"] = (model.ks_enc.parameters(), b * 0.5, False)
            groups["occ"] = ([model.occ_params], b * 2.5, False)
        return groups

    def lr_factor(self, step: int, decays: bool) -> float:
        """`Stage2Schedule.lr_factor` without a warm-up: a half-life of `base_decay` steps for the groups that decay"""
        if not decays or self.base_decay is None:
            return 1.0
        return math.exp(-math.log(2.0) / self.base_decay * step)

    def setup(self, model: Stage3Model) -> Dict[str, torch.optim.Adam]:
        """one Adam per group of `learning_rates` (the x64 of the light's gradients is `scale_light_gradient`)"""
        self._groups = self.learning_rates(model)
        return {name: torch.optim.Adam(params, lr=lr, eps=self.base_eps) for name, (params, lr, _) in self._groups.items()}

    def before_update(self, model: Stage3Model, curr_step: int, optimizers: Optional[Dict[str, torch.optim.Adam]] = None) -> None:
        model.kd_weight, model.ks_weight, model.normal_weight = self.kd_reg, self.ks_reg, self.normal_reg
        if optimizers is not None:
            for name, opt in optimizers.items():
                _, lr, decays = self._groups[name]
                for group in opt.param_groups:
                    group["lr"] = lr * self.lr_factor(curr_step, decays)

    def scale_light_gradient(self, model: Stage3Model) -> None:
        """setup's `register_hook(lambda g: g * 64)` on hue and value, applied to the finished gradients"""
        for p in (model.latlng_hue, model.latlng_value):
            if p.grad is not None:
                p.grad.mul_(self.light_gradient_scale)

    def after_update(self, model: Stage3Model, curr_step: int) -> None:
        with torch.no_grad():
            if model.learned_light:
                model.latlng_hue.clamp_(0.01, 0.99)
            model.kd_params.clamp_(0.01, 0.99)


def train_step(model: Stage3Model, cameras: Sequence[Camera], gt_rgba: Sequence[Tensor], *, gt_is_srgb: bool = True,
               use_mask_loss: bool = False, train_bg: Optional[Sequence[Tensor]] = None, bg_generator: Optional[torch.Generator] = None,
               rnd_seed: Optional[int] = None) -> Dict[str, Tensor]:
    """One `GeoSplatDeferTrainer.step` + backward over `cameras` (geosplat_defer_trainer.py:128-194): leaves
    d(mean view loss + regularisation) / d(parameter) in every parameter's .grad.  gt_rgba: the dataset's RGBA per camera, sRGB unless
    gt_is_srgb=False; the regulariser sees it clamped to [0,1] and linear, as the trainer passes it.  train_bg: fixed per-view
    backgrounds instead of the trainer's torch.rand_like; rnd_seed: a fixed shader seed (tests).  A view that outgrew the intersection
    capacity repeats the step (`viewbatch.retry_on_capacity`).  Returns detached metrics.  (A function of its own next to
    `stage2.train_step`: the render_report signatures, the linear ground truth and the mask default differ.)"""
    from .viewbatch import retry_on_capacity
    n = len(cameras)
    gen = model._bg_gen if bg_generator is None else bg_generator
    with torch.no_grad():
        gt_linear = [torch.cat((srgb_to_linear(g[..., :3].clamp(0, 1)) if gt_is_srgb else g[..., :3].clamp(0, 1), g[..., 3:].clamp(0, 1)),
                               dim=-1) for g in gt_rgba]

    def attempt():
        for p in model.parameters():
            p.grad = None
        images, reg, num_gaussians = model.render_report(cameras, gt_linear, rnd_seed=rnd_seed)
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


# ------------------------------------------------------------------------------------------------------------- the evaluation
def albedo_scaling(albedos: Sequence[Tensor], gt_albedos: Sequence[Tensor], mode: str = "least-square") -> Tensor:
    """The per-channel factor between the model's albedo and the dataset's (tests/model/test_geosplat_defer.py:385-404) -> [3].
    albedos: linear [H,W,3] per view; gt_albedos: linear RGBA [H,W,4] per view.
      'least-square'  per view sum(a * gt over black) / sum(a^2), then the mean over the views
      'median'        the median over the pixels of all views whose gt alpha is positive of gt[..., :3] / max(a, 1e-3)"""
    if mode not in ("least-square", "median"):
        raise ValueError(mode)
    if len(albedos) != len(gt_albedos) or not albedos:
        raise ValueError("albedo_scaling needs one ground truth per albedo map, and at least one")
    per_view = []
    for a, gt in zip(albedos, gt_albedos):
        if mode == "least-square":
            over_black = gt[..., :3] * gt[..., 3:]
            per_view.append((a * over_black).reshape(-1, 3).sum(0) / a.reshape(-1, 3).square().sum(0))
        else:
            mask = (gt[..., 3:] > 0).expand_as(a)
            per_view.append((gt[..., :3] / a.clamp_min(1e-3))[mask].view(-1, 3))
    if mode == "least-square":
        return torch.stack(per_view).mean(0)
    return torch.cat(per_view).median(0).values


def psnr(a: Tensor, b: Tensor) -> Tensor:
    """-10 log10(mean squared error)"""
    return -10.0 * torch.log10((a - b).square().mean())


def _ssim(a: Tensor, b: Tensor) -> Tensor:
    """SSIM of two blended [H,W,3] pictures from the loss kernel: with alpha 1 on both sides the kernel's blend leaves them as they
    are, and its `ssim_loss` output is 1 - SSIM"""
    one = torch.ones_like(a[..., :1])
    _, metrics = photo_loss(a.contiguous(), one, torch.cat((b, one), dim=-1), torch.zeros_like(a), gt_is_srgb=False, use_mask_loss=False)
    return 1.0 - metrics["ssim_loss"]


def _blend(rgba: Tensor, bg: Tensor) -> Tensor:
    """`RGBAImages.blend`: alpha * rgb + (1 - alpha) * background"""
    return rgba[..., 3:] * rgba[..., :3] + bg * (1 - rgba[..., 3:])


@torch.no_grad()
def evaluate_relighting(model: Stage3Model, cameras: Sequence[Camera], gt_views: Sequence[Tensor],
                        relights: Sequence[Tuple[object, Sequence[Tensor]]], *, gt_albedos: Optional[Sequence[Tensor]] = None,
                        gt_roughness: Optional[Sequence[Tensor]] = None, scaling: str = "least-square", bg: str = "white",
                        rnd_seed: Optional[int] = None) -> Dict[str, object]:
    """The `RelightEvaler` task (tests/model/test_geosplat_defer.py:345-493) on test `cameras`.

    gt_views: the dataset's sRGB RGBA [H,W,4] per camera; relights: [(envmap, sRGB RGBA per camera)], envmap as `set_relight_envmap`
    takes it; gt_albedos: sRGB RGBA per camera; gt_roughness: RGBA per camera whose first channel is the roughness; bg: 'black',
    'white' or 'default' (the model's own); scaling: the `albedo_scaling` mode.  Order of work, as the reference:
      1. albedo scaling from `material_maps(cam)["kd"]` over black against the linearised gt_albedos (ones(3) without gt_albedos)
      2. NVS under the model's own light; 3. every relight map after `set_relight_envmap(envmap, albedo_scaling)`
      4. with gt_albedos: albedo PSNR of `kd_srgb` (clamped) over black under the first relight map's scaling, and the roughness MSE
    Every picture is compared as the reference does: `rgb2srgb` of the rendered RGB, then alpha * rgb + (1 - alpha) * bg, clamped to
    [0,1], against the ground truth blended the same way.  PSNR is -10 log10(mse) per view, averaged over the views.  SSIM is
    1 - `photo_loss`'s ssim term on the blended pair (the trainer's SSIM kernel, alpha 1 on both sides).  LPIPS is not provided: it
    needs network weights that are no part of this package.  Returns
      {'albedo_scaling' [3], 'nvs_psnr', 'nvs_ssim', 'relight_psnr' [per map], 'relight_ssim' [per map], 'relight_psnr_mean',
       and with gt_albedos 'albedo_psnr', 'albedo_ssim', with gt_roughness 'roughness_mse'} as Python floats (the scaling a CPU tensor).
    The model's light, background and `training` flag are what they were on exit, also after an exception."""
    if bg not in ("black", "white", "default"):
        raise ValueError(bg)
    if len(gt_views) != len(cameras) or any(len(gts) != len(cameras) for _, gts in relights):
        raise ValueError("evaluate_relighting needs one ground truth per camera, in gt_views and for every relight map")
    saved = (model.background_color, model.training, model._fixed_envmap, model.albedo_scaling)
    dev = model._dev
    out: Dict[str, object] = {}
    mean = lambda xs: float(torch.stack(xs).mean())

    def compare(gts):
        color = model.get_background_color()
        psnrs, ssims = [], []
        for cam, gt in zip(cameras, gts):
            img = model.render_report([cam], rnd_seed=rnd_seed)[0][0]
            rgb = _blend(torch.cat((linear_to_srgb(img[..., :3]), img[..., 3:]), dim=-1), color).clamp(0, 1)
            gt_rgb = _blend(gt.to(dev), color).clamp(0, 1)
            psnrs.append(psnr(rgb, gt_rgb))
            ssims.append(_ssim(rgb, gt_rgb))
        return mean(psnrs), mean(ssims)
    try:
        model.training = False
        model.background_color = "black"
        scale = torch.ones(3, device=dev)
        if gt_albedos is not None:
            linear_gt = [torch.cat((srgb_to_linear(g[..., :3]), g[..., 3:]), dim=-1).to(dev) for g in gt_albedos]
            scale = albedo_scaling([model.material_maps(cam)["kd"] for cam in cameras], linear_gt, scaling)
        out["albedo_scaling"] = scale.detach().cpu()
        model.background_color = saved[0] if bg == "default" else bg
        out["nvs_psnr"], out["nvs_ssim"] = compare(gt_views)
        out["relight_psnr"], out["relight_ssim"] = [], []
        for envmap, gts in relights:
            model.set_relight_envmap(envmap, scale)
            p, s = compare(gts)
            out["relight_psnr"].append(p); out["relight_ssim"].append(s)
        if relights:
            out["relight_psnr_mean"] = sum(out["relight_psnr"]) / len(relights)
        if gt_albedos is not None:
            model.background_color = "black"
            if relights:
                model.set_relight_envmap(relights[0][0], scale)
            else:                                                # no map to relight with: only the scaling of the albedo matters
                model.albedo_scaling = scale
            color = model.get_background_color()
            psnrs, ssims, mses = [], [], []
            for i, cam in enumerate(cameras):
                maps = model.material_maps(cam)
                albedo, gt_albedo = maps["kd_srgb"].clamp(0, 1), _blend(gt_albedos[i].to(dev), color)
                psnrs.append(psnr(albedo, gt_albedo))
                ssims.append(_ssim(albedo, gt_albedo))
                if gt_roughness is not None:
                    mses.append((maps["ks"][..., 1:2] - _blend(gt_roughness[i].to(dev), color)[..., 0:1]).square().mean())
            out["albedo_psnr"], out["albedo_ssim"] = mean(psnrs), mean(ssims)
            if gt_roughness is not None:
                out["roughness_mse"] = mean(mses)
    finally:
        model.background_color, model.training, model._fixed_envmap, model.albedo_scaling = saved
    return out
