#!/usr/bin/env python3
"""Time the ambient-occlusion map and the shaders on it (csrc/gs_ao.hip, the visibility modes of csrc/gs_meshshade.hip, meshmc.py) at
the workload's own shape.

    python scripts/mesh_ao_bench.py [--runs 5] [--warmup 2] [--size 800] [--cells 224] [--parts ao,shade,mc] [--out FILE.json]

Mesh: the bumpy height field of scripts/meshreg_bench.py (cells x cells x 2 triangles; 224: 100 352 faces), seen from one size x size
camera (800: the reference's resolution); 128 ambient-occlusion targets.  Each figure is the median (min, max) in ms of `runs` timed
windows between two device events after `warmup`.
  face_ambient_occlusion one launch over F points x 128 targets on a MeshBVH built once, against MeshBVH.occluded on materialised
                         [F,128,3] directions plus the torch reductions of the same weights
  shade_pixels           occlusion 'ao' and 'screen' (a random map) against 'none', forward and forward + backward
  render_mesh_mc         num_samples_per_ray = 8, denoise on: the whole call, and its parts (G-buffer, env_shade, the filter)
No threshold is asserted.  Needs a GPU; there is no CPU path."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def torch_face_ao(bvh, centroids, normals, targets, offset):
    """the same weights from torch ops around MeshBVH.occluded on materialised directions"""
    o = centroids + normals * offset
    d = targets[None, :, :] - o[:, None, :]
    c = (normals[:, None, :] * d).sum(-1) / d.norm(dim=-1)
    hit = bvh.occluded(o, d.contiguous(), tmin=0.0, tmax=1.0)
    w = torch.where(c > 0, c.clamp_min(1e-4), torch.zeros_like(c))
    return (w * (~hit).float()).sum(-1) / w.sum(-1).clamp_min(1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--cells", type=int, default=224)
    ap.add_argument("--parts", default="ao,shade,mc", help="comma-separated subset of ao, shade, mc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_ao_bench needs a GPU")
    import geosplatting_amd as gs
    from denoise_bench import timed
    from meshreg_bench import height_field
    dev = torch.device("cuda:0")
    stat = lambda t: {"ms": t[0], "ms_min_max": t[1:]}
    v, f = height_field(a.cells, dev)
    size = a.size
    focal = 0.5 * size / math.tan(math.radians(20.0))
    eye, target, up = (torch.tensor(t) for t in ((0.9, 1.6, 1.7), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    cam = gs.Camera(gs.lookat_c2w(eye, target, up).to(dev).contiguous(), focal, focal, size / 2.0, size / 2.0, size, size)
    vn = gs.vertex_normals(v, f)
    results = {"size": size, "faces": int(f.shape[0]), "targets": 128, "runs": a.runs,
               "device": torch.cuda.get_device_name(0)}

    maps = gs.render_mesh(v, f, cam, outputs=("normal",), vertex_normals=vn)
    rast, normal = maps["rast"], maps["normal"]
    position = gs.interpolate(v, rast, f)
    results["covered_pixels"] = int((rast[..., 3] > 0).sum())
    parts = set(a.parts.split(","))
    sync = torch.cuda.synchronize            # after every first call of a kind: an error is then reported where it belongs
    bvh = gs.MeshBVH(v, f)
    if "ao" in parts:
        bench_ao(a, gs, timed, stat, results, v, f, bvh, dev)
    if "shade" in parts:
        bench_shade(a, gs, timed, stat, results, position, normal, rast, cam, dev)
    if "mc" in parts:
        bench_mc(a, gs, timed, stat, results, v, f, vn, bvh, position, normal, rast, cam, dev)
    sync()
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


def bench_ao(a, gs, timed, stat, results, v, f, bvh, dev):
    targets = gs.occlusion.default_ao_targets(dev)
    tri = v[f]
    centroids = tri.mean(1).contiguous()
    fn = torch.nn.functional.normalize(torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1), dim=-1).contiguous()
    hip = gs.face_ambient_occlusion(v, f, bvh)
    torch.cuda.synchronize()
    ref = torch_face_ao(bvh, centroids, fn, targets, 1e-3)
    torch.cuda.synchronize()
    results["face_ambient_occlusion"] = {
        "hip": stat(timed(lambda: gs.face_ambient_occlusion(v, f, bvh), a.runs, a.warmup)),
        "hip_kernel_only": stat(timed(lambda: gs.ambient_occlusion(bvh, centroids, fn, targets), a.runs, a.warmup)),
        "occluded_plus_torch": stat(timed(lambda: torch_face_ao(bvh, centroids, fn, targets, 1e-3), a.runs, 1)),
        "bvh_build": stat(timed(lambda: bvh.rebuild(v), a.runs, a.warmup)),
        "max_abs_difference": float((hip - ref).abs().max()), "mean_visibility": float(hip.mean())}
    print("face_ambient_occlusion", json.dumps(results["face_ambient_occlusion"]), flush=True)



def bench_shade(a, gs, timed, stat, results, position, normal, rast, cam, dev):
    size = a.size
    g = torch.Generator().manual_seed(1)
    kd = gs.Texture2D((torch.rand(64, 64, 3, generator=g) * 0.8 + 0.1).to(dev).requires_grad_())
    ks = gs.Texture2D(torch.rand(64, 64, 3, generator=g).to(dev).requires_grad_())
    env = gs.TextureSplitSum((torch.rand(6, 16, 16, 3, generator=g) + 0.2).to(dev).requires_grad_(),
                             [(torch.rand(6, r, r, 3, generator=g) + 0.2).to(dev).requires_grad_() for r in (256, 128, 64, 32, 16)], 0.08, 0.5)
    uv = (position[..., [0, 2]] * 0.6 + 0.5).contiguous()
    cot = torch.randn(size, size, 3, generator=g).to(dev)
    pos_leaf, nrm_leaf = position.detach().clone().requires_grad_(), normal.detach().clone().requires_grad_()
    vis_map = torch.rand(size, size, generator=g).to(dev)
    results["shade_pixels"] = {}
    for mode in ("none", "ao", "screen"):
        kw = dict(occlusion=mode, visibility=None if mode == "none" else vis_map)
        shade = lambda: gs.shade_pixels(pos_leaf, nrm_leaf, uv, rast, kd, ks, cam.c2w[:, 3], env, **kw)

        def both():
            out = shade()
            torch.autograd.grad(out, [pos_leaf, nrm_leaf, kd.data, ks.data, env.base], cot)

        with torch.no_grad():
            fwd = timed(shade, a.runs, a.warmup, 10)
        results["shade_pixels"][mode] = {"forward": stat(fwd), "forward_backward": stat(timed(both, a.runs, a.warmup, 5))}
        print("shade_pixels", mode, json.dumps(results["shade_pixels"][mode]), flush=True)



def bench_mc(a, gs, timed, stat, results, v, f, vn, bvh, position, normal, rast, cam, dev):
    size = a.size
    g = torch.Generator().manual_seed(2)
    light = gs.LatLngEnvMap((torch.rand(256, 512, 3, generator=g) * 0.5 + 0.05).to(dev))
    light.data[40:60, 100:140] = 30.0
    light.compute_pdf_()
    kd1 = gs.Texture2D.from_constants((0.7, 0.6, 0.5), device=dev)
    ks1 = gs.Texture2D.from_constants((0.0, 0.4, 0.1), device=dev)
    call = lambda: gs.render_mesh_mc(v, f, cam, kd=kd1, ks=ks1, uvs=None, envmap=light, bvh=bvh, num_samples_per_ray=8, rnd_seed=3,
                                     vertex_normals=vn)
    with torch.no_grad():
        whole = timed(call, a.runs, a.warmup)
        gbuf = timed(lambda: gs.render_mesh(v, f, cam, outputs=("normal",), vertex_normals=vn), a.runs, a.warmup)
        flat = lambda t: t.reshape(-1, t.shape[-1]).contiguous()
        P = size * size
        mask = (rast[..., 3] > 0).float().reshape(-1)
        kd_map, ks_map = kd1.data.reshape(1, 3).expand(P, 3).contiguous(), ks1.data.reshape(1, 3).expand(P, 3).contiguous()
        ro = flat(position + normal * 1e-3)
        shade = lambda: gs.env_shade(bvh, mask, ro, flat(position), flat(normal), cam.c2w[:, 3].contiguous(), kd_map, ks_map, light,
                                     BSDF="pbr", n_samples_x=8, rnd_seed=3)
        env_t = timed(shade, a.runs, a.warmup)
        six = torch.rand(size, size, 6, generator=g).to(dev)
        depth = ((position - cam.c2w[:, 3]) * (-cam.c2w[:, 2])).sum(-1, keepdim=True).contiguous()
        den = timed(lambda: gs.bilateral_denoiser(six, normal.contiguous(), depth, 2.0), a.runs, a.warmup)
    results["render_mesh_mc"] = {"whole": stat(whole), "g_buffer": stat(gbuf), "env_shade": stat(env_t), "denoise_6_channels": stat(den)}
    print("render_mesh_mc", json.dumps(results["render_mesh_mc"]), flush=True)


if __name__ == "__main__":
    main()
