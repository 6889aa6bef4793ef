#!/usr/bin/env python3
"""Time TSDF depth fusion (csrc/gs_tsdf.hip through geosplatting_amd.fusion) at the MeshExport shape: a 512^3 volume over +-1 and
100 views of 800 x 800 from cameras on a sphere of radius 3, against the same integration written as torch ops on the same device.

    python scripts/tsdf_bench.py [--resolution 512] [--views 100] [--size 800] [--runs 3] [--warmup 1] [--out FILE.json]

The depth maps are analytic: a bumpy sphere r(dir) = 0.6 + 0.05 sin(5 x) sin(5 y) sin(5 z) ray-marched on the device (no renderer
in the timed region).  Device events, a warm-up, the median over --runs:
  integrate  TSDFVolume.integrate of all views (ceil(views / 16) launches) into a zeroed volume
  extract    TSDFVolume.extract_mesh (count, the 32-byte read-back, fill)
  torch      the same update as elementwise torch ops, one view at a time over chunks of 2^24 voxels (what fits beside the volume)
The volume traffic a launch implies is 16 B per voxel (the (tsdf, weight) pair read and written once), whatever the number of
views in it; the torch form moves that per VIEW.  Needs a GPU; there is no CPU path.
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
import geosplatting_amd as gs                                              # noqa: E402
from geosplatting_amd.fusion import camera_matrices                       # noqa: E402

BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def bumpy_depth(cam, dev, steps=48):
    """[H,W,2] (z-depth, alpha) of the bumpy sphere: sphere tracing of f(p) = |p| - r(p / |p|) along the pixel-centre rays"""
    vm, K = cam.view_matrix.to(dev), cam.intrinsic_matrix.to(dev)
    H, W = cam.height, cam.width
    jj, ii = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
    dc = torch.stack(((ii - K[0, 2]) / K[0, 0], (jj - K[1, 2]) / K[1, 1], torch.ones_like(ii)), -1)    # z = 1: the parameter is z
    R, t = vm[:3, :3], vm[:3, 3]
    eye = -(R.T @ t)
    d = dc @ R
    speed = d.norm(dim=-1)
    s = torch.full((H, W), 2.0, device=dev)
    for _ in range(steps):
        p = eye + s[..., None] * d
        r = p.norm(dim=-1)
        q = 5.0 * p / r[..., None]
        f = r - (0.6 + 0.05 * torch.sin(q[..., 0]) * torch.sin(q[..., 1]) * torch.sin(q[..., 2]))
        s = s + 0.7 * f / speed
    hit = (f.abs() < 1e-3) & (s < 4.0)
    return torch.stack((torch.where(hit, s, torch.zeros_like(s)), hit.float()), -1).contiguous()


def torch_integrate(volume, res, origin, vs, sdf_trunc, maps, cams, alpha_trunc=0.5, depth_trunc=4.0, chunk=1 << 24):
    """The update of gs_tsdf_integrate as torch ops, in place on `volume` [N,2]"""
    R0, R1, R2 = res
    N = R0 * R1 * R2
    dev = volume.device
    o = torch.tensor(origin, device=dev)
    mats = list(zip(*camera_matrices(cams, dev)))                          # the matrices integrate hands to the kernel
    for lo in range(0, N, chunk):
        n = torch.arange(lo, min(lo + chunk, N), device=dev)
        idx = torch.stack((n % R0, (n // R0) % R1, n // (R0 * R1)), -1)
        p = o + (idx.float() + 0.5) * vs
        tsdf, w = volume[lo:lo + chunk, 0].clone(), volume[lo:lo + chunk, 1].clone()
        for da, cam, (vm, K) in zip(maps, cams, mats):
            pc = p @ vm[:3, :3].T + vm[:3, 3]
            z = pc[:, 2]
            u = K[0, 0] * pc[:, 0] / z + K[0, 2]
            v = K[1, 1] * pc[:, 1] / z + K[1, 2]
            ok = (z > 0) & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height)
            iu = u.clamp(0, cam.width - 1).nan_to_num(0).long()
            iv = v.clamp(0, cam.height - 1).nan_to_num(0).long()
            tex = da.reshape(-1, 2)[iv * cam.width + iu]
            d = tex[:, 0]
            ok &= (tex[:, 1] > alpha_trunc) & (d > 0) & (d < depth_trunc)
            sdf = d - z
            ok &= sdf > -sdf_trunc
            val = (sdf / sdf_trunc).clamp(max=1.0)
            tsdf = torch.where(ok, (tsdf * w + val) / (w + 1), tsdf)
            w = torch.where(ok, w + 1, w)
        volume[lo:lo + chunk, 0] = tsdf
        volume[lo:lo + chunk, 1] = w


def timed(fn, runs, warmup):
    out = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-runs", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench needs a GPU")
    dev = torch.device("cuda:0")
    cams = [c.to(dev) for c in gs.sphere_cameras(a.views, 3.0, a.size, a.size, generator=torch.Generator().manual_seed(0))]
    maps = [bumpy_depth(c, dev) for c in cams]
    vol = gs.TSDFVolume(a.resolution, bounds=BOUNDS, device=dev)
    N = a.resolution ** 3

    def run_integrate():
        vol.volume.zero_()
        vol.integrate(maps, cams)

    t_int, all_int = timed(run_integrate, a.runs, a.warmup)
    mesh = {}

    def run_extract():
        mesh["v"], mesh["f"] = vol.extract_mesh()

    t_ext, all_ext = timed(run_extract, a.runs, a.warmup)
    hip_volume = vol.volume.reshape(-1, 2).clone()

    flat = vol.volume.reshape(-1, 2)

    def run_torch():
        flat.zero_()
        torch_integrate(flat, vol.resolution, vol.origin, vol.voxel_size, vol.sdf_trunc, maps, cams)

    t_torch, all_torch = timed(run_torch, a.torch_runs, 0 if a.torch_runs == 1 else 1)
    same_w = (flat[:, 1] == hip_volume[:, 1]).float().mean().item()
    max_dt = (flat[:, 0] - hip_volume[:, 0]).abs()[flat[:, 1] == hip_volume[:, 1]].max().item()
    launches = math.ceil(a.views / 16)
    res = {
        "resolution": a.resolution, "views": a.views, "image": a.size, "voxel_view_updates": N * a.views,
        "integrate_ms": t_int, "integrate_ms_all": all_int, "launches": launches,
        "volume_bytes_per_launch": 16 * N, "volume_gbps": 16 * N * launches / (t_int * 1e-3) / 1e9,
        "voxel_views_per_ns": N * a.views / (t_int * 1e6),
        "extract_ms": t_ext, "extract_ms_all": all_ext, "vertices": int(mesh["v"].shape[0]), "faces": int(mesh["f"].shape[0]),
        "counts": list(vol.last_counts),
        "torch_integrate_ms": t_torch, "torch_ms_all": all_torch, "torch_volume_bytes": 16 * N * a.views, "speedup": t_torch / t_int,
        "torch_same_weight_fraction": same_w, "torch_max_tsdf_diff_where_same_weight": max_dt,
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
