#!/usr/bin/env python3
"""Time the ray-mesh queries (csrc/gs_bvh.hip through geosplatting_amd.raytrace): the LBVH build, `occluded` and `closest_hit`.

    python scripts/raytrace_bench.py [--runs 20] [--warmup 3] [--out FILE.json]

Meshes: the stage-1 FlexiCubes sphere at 96^3 (the mesh of scripts/mesh_render_bench.py, about 100 k faces) and syn.icosphere(7)
(327 680 faces).  Rays start at the mesh's own MGAdapter Gaussians, offset by 1e-3 along their shading normals as the shadow test does,
towards seeded uniform directions:
  shared     the [S,3] form, S = 128 directions shared by 4 096 of the points (evenly strided)       524 288 rays
  per_point  the [P,S,3] form, S = 16 directions per point for 65 536 of the points               1 048 576 rays
Per mesh, `runs` windows after `warmup`, each window a few back-to-back calls between two device events; median (min, max) per call:
  build_ms                   MeshBVH.rebuild (every launch of gs_bvh_build, radix passes included)
  occluded / closest_hit     ms per call and rays per second
Two baselines measured in the same run, since nothing here has a predecessor to compare with:
  brute_force   the null-buffer form of both queries on icosphere(4) (5 120 faces), 32 768 rays
  torch_mt      Moeller-Trumbore composed from torch ops over all (ray, face) pairs of icosphere(3) (1 280 faces), 4 096 rays:
                an any-hit reduction, what a user could write without this module
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn, runs, warmup, calls):
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


def flexicubes_sphere(R, dev):
    """the mesh of scripts/mesh_render_bench.py: Stage1Model with a sphere SDF of radius 0.8"""
    import geosplatting_amd as gs
    from geosplatting_amd.stage1 import Stage1Model
    grid = gs.FlexiCubes.from_resolution(R, device=dev, random_sdf=False, scale=1.05)
    model = Stage1Model(R, light_resolution=16, device=dev, sdf_init=grid.vertices.norm(dim=-1) - 0.8)
    with torch.no_grad():
        (v, f), _ = model.get_geometry()
    return v.contiguous(), f.contiguous()


def torch_mt_any(v, f, o, d):
    """any-hit by Moeller-Trumbore over all pairs, both sides, t > 0: [R] bool"""
    t0, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    pv = torch.cross(d[:, None, :].expand(-1, f.shape[0], -1), e2[None].expand(d.shape[0], -1, -1), dim=-1)
    det = (e1[None] * pv).sum(-1)
    inv = 1.0 / det
    tv = o[:, None, :] - t0[None]
    u = (tv * pv).sum(-1) * inv
    qv = torch.cross(tv, e1[None].expand_as(tv), dim=-1)
    w = (d[:, None, :] * qv).sum(-1) * inv
    t = (e2[None] * qv).sum(-1) * inv
    return ((det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)).any(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raytrace_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import synthetic as syn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1).to(dev).contiguous()
    stat = lambda t, rays=None: {"ms": t[0], "ms_min_max": t[1:], **({"rays_per_s": rays / (t[0] * 1e-3)} if rays else {})}
    results = {"meshes": {}}

    def rays_of(v, f, offset=1e-3):
        with torch.no_grad():
            splats, normals = gs.mesh_to_splats(v, f, gs.vertex_normals(v, f))
            return (splats.means + normals * offset).contiguous()

    for name, (v, f) in (("flexicubes_96", flexicubes_sphere(96, dev)), ("icosphere_7", tuple(t.to(dev) for t in syn.icosphere(7, 0.8)))):
        bvh = gs.MeshBVH(v, f)
        origins = rays_of(v, f)
        n = origins.shape[0]
        o_shared = origins[:: max(1, n // 4096)][:4096].contiguous()
        o_pp = origins[:: max(1, n // 65536)][:65536].contiguous()
        d_shared, d_pp = unit(128), unit(o_pp.shape[0], 16)
        r = {"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "gaussians": int(n),
             "build": stat(timed(lambda: bvh.rebuild(v), a.runs, a.warmup, 5))}
        for label, o, d in (("shared", o_shared, d_shared), ("per_point", o_pp, d_pp)):
            rays = o.shape[0] * d.shape[-2]
            occ = bvh.occluded(o, d)
            r[label] = {"rays": rays, "occluded_share": float(occ.float().mean()),
                        "occluded": stat(timed(lambda: bvh.occluded(o, d), a.runs, a.warmup, 3), rays),
                        "closest_hit": stat(timed(lambda: bvh.closest_hit(o, d), a.runs, a.warmup, 3), rays)}
        results["meshes"][name] = r
        print(name, json.dumps(r), flush=True)

    v, f = (t.to(dev) for t in syn.icosphere(4, 0.8))
    bvh = gs.MeshBVH(v, f)
    o = rays_of(v, f)[:2048].contiguous()
    d = unit(2048, 16)
    rays = 2048 * 16
    assert torch.equal(bvh.occluded(o, d), bvh.occluded(o, d, brute_force=True))
    results["brute_force"] = {"faces": int(f.shape[0]), "rays": rays,
                              "occluded": stat(timed(lambda: bvh.occluded(o, d, brute_force=True), a.runs, a.warmup, 1), rays),
                              "closest_hit": stat(timed(lambda: bvh.closest_hit(o, d, brute_force=True), a.runs, a.warmup, 1), rays),
                              "bvh_occluded": stat(timed(lambda: bvh.occluded(o, d), a.runs, a.warmup, 3), rays),
                              "bvh_closest_hit": stat(timed(lambda: bvh.closest_hit(o, d), a.runs, a.warmup, 3), rays)}
    print("brute_force", json.dumps(results["brute_force"]), flush=True)

    v, f = (t.to(dev) for t in syn.icosphere(3, 0.8))
    bvh = gs.MeshBVH(v, f)
    o = rays_of(v, f)[:4096].contiguous()
    d = unit(4096)
    ours, theirs = bvh.occluded(o, d)[:, 0], torch_mt_any(v, f, o, d)
    results["torch_mt"] = {"faces": int(f.shape[0]), "rays": 4096, "disagreements": int((ours != theirs).sum()),
                           "torch_any_hit": stat(timed(lambda: torch_mt_any(v, f, o, d), 5, 1, 1), 4096),
                           "bvh_occluded": stat(timed(lambda: bvh.occluded(o, d), a.runs, a.warmup, 3), 4096)}
    print("torch_mt", json.dumps(results["torch_mt"]), flush=True)
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
