#!/usr/bin/env python3
"""Time the per-pixel mesh shader (csrc/gs_meshshade.hip through geosplatting_amd.meshshade) at 800 x 800 on a sphere mesh, for 1 x 1 and
1024 x 1024 kd / ks textures, against the composition that was possible before it on the same device.

    python scripts/mesh_shade_bench.py [--size 800] [--textures 1,1024] [--runs 20] [--warmup 3] [--out FILE.json]

The G-buffer (rast, world positions, vertex normals, per-face-vertex spherical uvs) comes from render_mesh's own pieces on
syn.icosphere(5, 0.6), seen by the first syn.blender_cameras view; the environment is as_splitsum of a random 512^2 cube map
(levels 512 .. 16, base 16).  Per texture size, `runs` windows after `warmup`, each window ten back-to-back calls between two device
events (the slow composed backward: one call per window); the median time per call:
  fwd_ms          gs_meshshade_fwd (shade_pixels under no_grad)
  fwd_bwd_ms      shade_pixels + backward of sum(colour * random cotangent), gradients to position, normal, uv, kd, ks, base, levels
                  (includes zeroing the texel-gradient buffers); bwd_ms = fwd_bwd_ms - fwd_ms
  composed_*      the same colour from existing ops: a torch bilinear wrap lookup of kd and ks (index arithmetic + four gathers), then
                  shade(mode='diffuse') + shade(mode='specular') with min_roughness = 0, max_metallic = 1 on the covered pixels, times
                  the visibility, scattered back into the image; forward, and forward + backward to the same leaves
  max_abs_diff    between the two colours (the composition clamps n.v at 1e-6 instead of 1e-4)
texel_adds = fp32 adds of texel gradients per view, from the kernel's structure and not from counters: 12 per shaded pixel for each of
kd, ks and base, 12 per level in use.  Which of them are LDS adds and how many global atomics the flushes issue is decided in
csrc/gs_meshshade.hip (gs_meshshade_bwd's LDS layout) and is not restated here.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


CALLS = 10          # calls per timed window: one call is 0.05 - 0.5 ms, the scale of a launch's own overhead


def timed(fn, runs, warmup, calls=CALLS):
    """median, min and max over `runs` windows of the time per call, each window `calls` back-to-back calls between two events"""
    out = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out), min(out), max(out)


def torch_wrap_lookup(tex, uv):
    """Texture2D.sample in plain torch: [n,2] -> [n,3]"""
    Ht, Wt = tex.shape[:2]
    q = uv * uv.new_tensor([1.0 - 1.0 / Wt, 1.0 - 1.0 / Ht]) + uv.new_tensor([0.5 / Wt, 0.5 / Ht])
    q = q - q.detach().floor()
    x, y = q[:, 0] * Wt - 0.5, q[:, 1] * Ht - 0.5
    ix0, iy0 = x.detach().floor().long(), y.detach().floor().long()
    fx, fy = (x - ix0)[:, None], (y - iy0)[:, None]
    jx0, jx1, jy0, jy1 = ix0 % Wt, (ix0 + 1) % Wt, iy0 % Ht, (iy0 + 1) % Ht
    flat = tex.reshape(-1, 3)
    top = flat[jy0 * Wt + jx0] + fx * (flat[jy0 * Wt + jx1] - flat[jy0 * Wt + jx0])
    bot = flat[jy1 * Wt + jx0] + fx * (flat[jy1 * Wt + jx1] - flat[jy1 * Wt + jx0])
    return top + fy * (bot - top)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--textures", default="1,1024")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_shade_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import synthetic as syn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    cam = syn.blender_cameras(8, a.size, a.size)[0].to(dev)
    v, f = syn.icosphere(5, 0.6)
    v, f = v.to(dev), f.to(dev)
    corner = v[f]
    uvs = torch.stack((torch.atan2(corner[..., 1], corner[..., 0]) / (2 * math.pi) + 0.5,
                       torch.acos((corner[..., 2] / 0.6).clamp(-1, 1)) / math.pi), -1).contiguous()
    with torch.no_grad():
        maps = gs.render_mesh(v, f, cam, outputs=("normal",))
        rast, normal = maps["rast"], maps["normal"].contiguous()
        position, uv = gs.interpolate(v, rast, f), gs.interpolate(uvs, rast, f)
        env = gs.as_splitsum(torch.rand(6, 512, 512, 3, generator=g).to(dev) + 0.2)
    cam_pos = cam.c2w[:, 3].to(dev).contiguous()
    covered = rast[..., 3] > 0
    n_cov = int(covered.sum())
    H = W = a.size
    cot = torch.randn(H, W, 3, generator=g).to(dev)
    res = [int(l.shape[1]) for l in env.levels]
    results = {"image": a.size, "covered_pixels": n_cov, "faces": int(f.shape[0]), "levels": res, "base": int(env.base.shape[1]), "textures": {}}
    leaf = lambda t: t.detach().clone().requires_grad_()
    for T in [int(t) for t in a.textures.split(",")]:
        kd0 = torch.rand(T, T, 3, generator=g).to(dev) * 0.9 + 0.05
        ks0 = torch.rand(T, T, 3, generator=g).to(dev) * torch.tensor([0.5, 1.0, 1.0], device=dev)
        P, N, U = leaf(position), leaf(normal), leaf(uv)
        kd, ks = gs.Texture2D(leaf(kd0)), gs.Texture2D(leaf(ks0))
        e = gs.TextureSplitSum(leaf(env.base), [leaf(l) for l in env.levels], env.min_roughness, env.max_roughness)
        leaves = [P, N, U, kd.data, ks.data, e.base] + list(e.levels)

        def fwd():
            with torch.no_grad():
                return gs.shade_pixels(P, N, U, rast, kd, ks, cam_pos, e)

        def fwd_bwd():
            for t in leaves:
                t.grad = None
            (gs.shade_pixels(P, N, U, rast, kd, ks, cam_pos, e) * cot).sum().backward()

        def composed(grad):
            with torch.set_grad_enabled(grad):
                p, n, q = P[covered], N[covered], U[covered]
                kd_s, ks_s = torch_wrap_lookup(kd.data, q), torch_wrap_lookup(ks.data, q)
                kw = dict(min_roughness=0.0, max_metallic=1.0)
                col = gs.shade(p, n, kd_s, ks_s[:, 1:3].contiguous(), cam_pos, e, mode="diffuse", **kw) + \
                    gs.shade(p, n, kd_s, ks_s[:, 1:3].contiguous(), cam_pos, e, mode="specular", **kw)
                col = col * (1.0 - ks_s[:, 0:1]).clamp_min(0.0)
                out = torch.zeros(H, W, 3, device=dev).masked_scatter(covered[..., None].expand(H, W, 3), col)
                if grad:
                    for t in leaves:
                        t.grad = None
                    (out * cot).sum().backward()
                return out

        diff = float((fwd() - composed(False)).abs().max())
        t_f, t_fb = timed(fwd, a.runs, a.warmup), timed(fwd_bwd, a.runs, a.warmup)
        t_cf, t_cfb = timed(lambda: composed(False), a.runs, a.warmup), timed(lambda: composed(True), 5, 1, calls=1)
        results["textures"][f"{T}x{T}"] = {
            "fwd_ms": t_f[0], "fwd_ms_min_max": t_f[1:], "fwd_bwd_ms": t_fb[0], "fwd_bwd_ms_min_max": t_fb[1:], "bwd_ms": t_fb[0] - t_f[0],
            "composed_fwd_ms": t_cf[0], "composed_fwd_bwd_ms": t_cfb[0], "max_abs_diff": diff,
            "texel_adds": n_cov * (12 * 3 + 24),
        }
        print(f"{T}x{T}", json.dumps(results["textures"][f"{T}x{T}"]), flush=True)
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
