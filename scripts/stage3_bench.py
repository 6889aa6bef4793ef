#!/usr/bin/env python3
"""Time one stage-3 (`Stage3Model`) training step and the parts of its forward.

    python scripts/stage3_bench.py [--cells 224] [--runs 5] [--warmup 2] [--image 800] [--samples 16] [--out FILE.json]

The frozen mesh is the bumpy height field of scripts/meshreg_bench.py (cells x cells x 2 triangles; 224: 100 352 faces, 602 112
Gaussians), exported by a `PriorModel` under a 256 x 512 light with a sun and loaded with `Stage3Model.from_export`; one image x image
view, num_samples_per_ray `samples`.  Each figure is the median (min, max) in ms of `runs` windows after `warmup`, each between two
device events, each part in a run of its own:
  train_step       one `stage3.train_step` (forward, loss, regularisers, backward) under `Stage3Schedule`'s weights
  surface          `rasterize_mesh` + `interpolate` of the frozen mesh
  gbuffer          the 14-channel compositor pass of `splat_mc_deferred`, forward
  env_shade        the per-pixel Monte-Carlo shader on that G-buffer, forward
  reg_pass         the 6-channel un-shaded pass of the two edge-aware terms, forward
  deferred         `splat_mc_deferred` as a whole, forward; `remainder` = deferred - gbuffer - env_shade is what torch composes around
                   the two kernels (bending, unpacking, clamps, the residual light, tone mapping), `remainder_share` its share of deferred
  material_maps    the 9-channel pass and the sRGB curve
  eval_view        `render_report` of one view without a ground truth, forward only (ks encoder twice, surface, deferred)
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage3_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import stage3
    from geosplatting_amd import synthetic as syn
    from geosplatting_amd.meshrender import _unit_or_z
    from geosplatting_amd.shading import _rasterize_activated
    from meshreg_bench import height_field, timed
    dev = torch.device("cuda:0")
    stat = lambda t: {"ms": t[0], "ms_min_max": [t[1], t[2]]}
    run = lambda fn: stat(timed(fn, a.runs, a.warmup))

    v0, f = height_field(a.cells, dev)
    prior = gs.PriorModel(v0, f, log2_hashmap_size=18)
    g = torch.Generator().manual_seed(0)
    light = torch.rand(256, 512, 3, generator=g) * 0.4 + 0.1
    light[60:66, 120:132] += 400.0                                  # the sun
    with torch.no_grad():
        prior.latlng.copy_(light.to(dev))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "stage2.pth")
        prior.export_model(path)
        model = gs.Stage3Model.from_export(path, device=dev)
    del prior
    model.num_samples_per_ray = a.samples
    sched = gs.Stage3Schedule()
    sched.setup(model)
    sched.before_update(model, 0)
    cam = syn.blender_cameras(1, a.image, a.image)[0]
    r = {"faces": int(f.shape[0]), "gaussians": int(model.means.shape[0]), "image": a.image, "views": 1, "num_samples_per_ray": a.samples,
         "light": list(light.shape[:2])}
    with torch.no_grad():
        gts = [img.clamp(0, 1) for img in model.render_report([cam], rnd_seed=1)[0]]
    r["coverage"] = float((gts[0][..., 3] > 0.5).float().mean())
    r["train_step"] = run(lambda: stage3.train_step(model, [cam], gts, gt_is_srgb=False))
    print("train_step", json.dumps(r["train_step"]), flush=True)

    with torch.no_grad():
        model.training = False
        splats = model.get_gsplat()
        kd, ks, occ = model._materials()
        envmap = model.get_envmap()
        bvh = model.bvh()
        positions, mask = model.surface(cam)
        c2w = cam.c2w.to(dev)
        camera_pos, lookat = c2w[:, 3].contiguous(), -c2w[:, 2]
        bend = (splats.colors * lookat).sum(-1, keepdim=True) > 0
        normals = torch.where(bend, -splats.colors, splats.colors)
        opacities = torch.where(bend, torch.full_like(splats.opacities, -2.0), splats.opacities)
        channels = torch.cat((normals, kd, ks, occ), dim=-1)
        gbuffer = lambda: _rasterize_activated(splats.means, splats.scales, splats.quats, opacities, channels, cam, "RGB")
        render, alpha, _ = gbuffer()
        render = render / alpha.clamp_min(1e-6)
        frag_n = _unit_or_z(render[..., 0:3]).reshape(-1, 3)
        frag_kd = render[..., 3:6].reshape(-1, 3).contiguous()
        rough = render[..., 6:7] * (1 - model.min_roughness) + model.min_roughness
        frag_ks = torch.cat((torch.zeros_like(rough), rough, render[..., 7:8] * model.max_metallic), dim=-1).reshape(-1, 3)
        pos = positions.reshape(-1, 3)
        pdf, rows, cols = envmap.tables()
        shade = lambda: gs.env_shade(bvh, mask.reshape(-1), frag_n * 1e-3 + pos, pos, frag_n, camera_pos, frag_kd, frag_ks, envmap.data,
                                     pdf, rows, cols, BSDF="pbr", n_samples_x=a.samples, shadow_scale=model.shadow_scale)
        attrs = gs.RenderableAttrs(kd=kd, ks=ks, occ=occ, normals=splats.colors)
        exposure = model.exposure_params.exp()[0]
        deferred = lambda: attrs.splat_mc_deferred(splats, [cam], bvh=bvh, exposure=exposure, positions=positions, mask=mask, envmap=envmap,
                                                   min_roughness=model.min_roughness, max_metallic=model.max_metallic,
                                                   num_samples_per_ray=a.samples, shadow_scale=model.shadow_scale, residual=True)
        six = torch.cat((kd, splats.colors * 0.5 + 0.5), dim=-1)
        bg = model.get_background_color()
        for name, fn in (("surface", lambda: model.surface(cam)), ("gbuffer", gbuffer), ("env_shade", shade),
                         ("reg_pass", lambda: stage3._render_channels(splats.means, splats.scales, splats.quats, splats.opacities, six, cam, bg)),
                         ("deferred", deferred), ("material_maps", lambda: model.material_maps(cam)),
                         ("eval_view", lambda: model.render_report([cam]))):
            r[name] = run(fn)
            print(name, json.dumps(r[name]), flush=True)
    rest = r["deferred"]["ms"] - r["gbuffer"]["ms"] - r["env_shade"]["ms"]
    r["remainder"] = {"ms": rest, "of": "medians: deferred - gbuffer - env_shade"}
    r["remainder_share"] = rest / r["deferred"]["ms"]
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
