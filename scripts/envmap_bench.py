#!/usr/bin/env python3
"""Time the environment resampling kernels (csrc/gs_envmap.hip) at the shapes the reference uses them at.

    python scripts/envmap_bench.py [--runs 5] [--warmup 2] [--iters 20] [--out FILE.json]

Shapes: a 512^2 cube map to a 256 x 512 and to a 512 x 1024 lat-long map (TextureCubeMap.as_latlng as stage 2 and the relighting loop
call it), a 256 x 512 lat-long map to a 512^2 cube map (TextureLatLng.as_cubemap(resolution=512)), forward and backward for both,
and the background of an 800 x 800 camera from a 512^2 cube map.  Seeded random texels.

Per entry `runs` windows after `warmup`, each window `iters` launches of the C entry point between two device events on buffers
allocated beforehand (the backward adds into one zeroed buffer: what it does under autograd, minus the allocation); the median
window (min, max) divided by `iters`, in microseconds, and the bytes the call has to move at least (each side of the resampling
once; the taps come from the caches) over that time.

Beside each: the composition available without these kernels, timed the same way through its public call (allocation included, as a
user pays it).
  lat-long -> cube   torch ops for the lookup coordinates of every cube texel, then `texture2d(..., 'wrap')`; backward by autograd.
  cube -> lat-long,  no cube lookup was public: torch ops for the directions, then a torch restatement of the lookup by gathers (face
  background         selection, face coordinates, four clamped taps, bilinear weights -- the seam rule left out, which only makes it
                     cheaper); backward by autograd (index_put with accumulation).
Needs a GPU; there is no CPU path."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn, runs, warmup, iters):
    out = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(1e3 * e0.elapsed_time(e1) / iters)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


# ------------------------------------------------------------------------------------------------ the compositions
def latlng_dirs(H, W, dev):
    gy = torch.linspace(1.0 / H, 1.0 - 1.0 / H, H, device=dev) * math.pi
    gx = torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, device=dev) * math.pi
    gy, gx = torch.meshgrid(gy, gx, indexing="ij")
    st = gy.sin()
    return torch.stack((st * gx.sin(), gy.cos(), -st * gx.cos()), -1)


def torch_cube_gather(cube, d):
    """bilinear cube lookup by torch ops, taps clamped to the face (no seam rule): cube [6,R,R,3], d [...,3]"""
    R = cube.shape[1]
    d = d.reshape(-1, 3)
    a = d.abs()
    axis = a.argmax(-1)
    major = d.gather(1, axis[:, None])[:, 0]
    face = 2 * axis + (major < 0).long()
    inv = 1.0 / major.abs()
    ia = torch.tensor([2, 2, 0, 0, 0, 0], device=d.device)[face]
    ib = torch.tensor([1, 1, 2, 2, 1, 1], device=d.device)[face]
    sx = torch.tensor([-1.0, 1.0, 1.0, 1.0, 1.0, -1.0], device=d.device)[face]
    sy = torch.tensor([-1.0, -1.0, 1.0, -1.0, -1.0, -1.0], device=d.device)[face]
    x = sx * d.gather(1, ia[:, None])[:, 0] * inv
    y = sy * d.gather(1, ib[:, None])[:, 0] * inv
    tx, ty = (x + 1) * 0.5 * R - 0.5, (y + 1) * 0.5 * R - 0.5
    ix0, iy0 = tx.floor(), ty.floor()
    fx, fy = (tx - ix0)[:, None], (ty - iy0)[:, None]
    ix0, iy0 = ix0.long(), iy0.long()
    ix1, iy1 = (ix0 + 1).clamp(0, R - 1), (iy0 + 1).clamp(0, R - 1)
    ix0, iy0 = ix0.clamp(0, R - 1), iy0.clamp(0, R - 1)
    top = cube[face, iy0, ix0] * (1 - fx) + cube[face, iy0, ix1] * fx
    bot = cube[face, iy1, ix0] * (1 - fx) + cube[face, iy1, ix1] * fx
    return top * (1 - fy) + bot * fy


def cube_texel_uv(R, dev):
    g = torch.linspace(-1.0 + 1.0 / R, 1.0 - 1.0 / R, R, device=dev)
    y, x = torch.meshgrid(g, g, indexing="ij")
    one = torch.ones_like(x)
    v = torch.stack([torch.stack(t, -1) for t in ((one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one))])
    v = v / v.norm(dim=-1, keepdim=True)
    tu = torch.atan2(v[..., 0], -v[..., 2]) / (2 * math.pi) + 0.5
    tv = torch.acos(v[..., 1].clamp(-1, 1)) / math.pi
    return torch.stack((tu, tv), -1)


def rgb2srgb(c):
    return torch.where(c <= 0.0031308, c * 12.92, c.clamp(min=0.0031308).pow(1.0 / 2.4) * 1.055 - 0.055)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("envmap_bench.py needs a GPU: there is no CPU path and no number without one")
    import geosplatting_amd as gs
    from geosplatting_amd import _lib as L
    dev = torch.device("cuda:0")
    lib = L.lib()
    g = torch.Generator().manual_seed(0)
    R = 512
    cube = torch.rand(6, R, R, 3, generator=g).to(dev)
    T = gs.EnvCubeMap(cube).z_up_to_y_up_().rotateY_(0.7).transform.contiguous()
    t = lambda fn: timed(fn, args.runs, args.warmup, args.iters)
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "iters": args.iters, "entries": {}}

    def entry(name, kernel, composition, moved_bytes):
        kernel, composition = t(kernel), t(composition)
        res["entries"][name] = {"kernel": kernel, "composition": composition, "moved_bytes": moved_bytes,
                                "kernel_gb_per_s": moved_bytes / kernel["median_us"] * 1e-3,
                                "speedup": composition["median_us"] / kernel["median_us"]}
        print(f"{name:34s} kernel {kernel['median_us']:9.1f} us ({kernel['min_us']:.1f} .. {kernel['max_us']:.1f})   composition "
              f"{composition['median_us']:9.1f} us ({composition['min_us']:.1f} .. {composition['max_us']:.1f})   "
              f"{res['entries'][name]['kernel_gb_per_s']:7.1f} GB/s", flush=True)

    for H, W in ((256, 512), (512, 1024)):
        out = torch.empty(H, W, 3, device=dev)
        cot = torch.rand(H, W, 3, generator=g).to(dev)
        d_cube = torch.zeros_like(cube)
        leaf = cube.clone().requires_grad_(True)
        moved = H * W * 12 + cube.numel() * 4                    # the lat-long side once and the cube side once
        entry(f"cube {R} -> latlng {H}x{W} fwd",
              lambda: L.check(lib.gs_env_cube_to_latlng_fwd(R, H, W, L.ptr(cube), L.ptr(T), L.ptr(out), L.stream()), "fwd"),
              lambda: torch_cube_gather(cube, latlng_dirs(H, W, dev) @ T.T), moved)
        entry(f"cube {R} -> latlng {H}x{W} bwd",
              lambda: L.check(lib.gs_env_cube_to_latlng_bwd(R, H, W, L.ptr(T), L.ptr(cot), L.ptr(d_cube), L.stream()), "bwd"),
              lambda: torch.autograd.grad((torch_cube_gather(leaf, latlng_dirs(H, W, dev) @ T.T) * cot.reshape(-1, 3)).sum(), leaf),
              moved)
    H, W = 256, 512
    lat = torch.rand(H, W, 3, generator=g).to(dev)
    out = torch.empty(6, R, R, 3, device=dev)
    cot = torch.rand(6, R, R, 3, generator=g).to(dev)
    d_lat = torch.zeros_like(lat)
    leaf = lat.clone().requires_grad_(True)
    entry(f"latlng {H}x{W} -> cube {R} fwd",
          lambda: L.check(lib.gs_env_latlng_to_cube_fwd(H, W, R, L.ptr(lat), L.ptr(out), L.stream()), "fwd"),
          lambda: gs.texture2d(lat, cube_texel_uv(R, dev), "wrap"), 6 * R * R * 12 + H * W * 12)
    entry(f"latlng {H}x{W} -> cube {R} bwd",
          lambda: L.check(lib.gs_env_latlng_to_cube_bwd(H, W, R, L.ptr(cot), L.ptr(d_lat), L.stream()), "bwd"),
          lambda: torch.autograd.grad((gs.texture2d(leaf, cube_texel_uv(R, dev), "wrap") * cot).sum(), leaf), 6 * R * R * 12 + H * W * 12)
    Hc = Wc = 800
    cam = gs.orbit_cameras(8, 3.0, 20.0, Wc, Hc, focal=0.8 * Wc)[3].to(dev)
    img = torch.empty(Hc, Wc, 3, device=dev)
    c2w = cam.c2w.contiguous()

    def composed_background():
        i, j = torch.meshgrid(torch.arange(Hc, device=dev, dtype=torch.float32), torch.arange(Wc, device=dev, dtype=torch.float32), indexing="ij")
        v = torch.stack(((0.5 - cam.cx + j) / cam.fx, -(0.5 - cam.cy + i) / cam.fy, -torch.ones_like(i)), -1)
        return rgb2srgb(torch_cube_gather(cube, v @ c2w[:, :3].T @ T.T))

    entry(f"background {Hc}x{Wc} from cube {R}",
          lambda: L.check(lib.gs_env_background_fwd(R, Hc, Wc, L.ptr(cube), cam.fx, cam.fy, cam.cx, cam.cy, L.ptr(c2w), L.ptr(T), 1, L.ptr(img),
                                                    L.stream()), "background"),
          composed_background, Hc * Wc * 12 + cube.numel() * 4)
    # the two forms agree where the composition states the same lookup (lat-long -> cube), and nearly so away from the seams
    same = (out - gs.texture2d(lat, cube_texel_uv(R, dev), "wrap")).abs().max().item()
    res["latlng_to_cube_max_abs_difference_to_composition"] = same
    print(f"lat-long -> cube: largest difference between the kernel and the composition {same:.2e}")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
