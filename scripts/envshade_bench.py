#!/usr/bin/env python3
"""Time the Monte-Carlo environment shader (csrc/gs_envshade.hip through geosplatting_amd.env_shade) at the stage-2 workload shape.

    python scripts/envshade_bench.py [--runs 10] [--warmup 2] [--points N] [--out FILE.json]

Scene: the stage-1 FlexiCubes sphere at 96^3 (the mesh of scripts/raytrace_bench.py, about 100 k faces) and its MGAdapter Gaussians
(6 per face), shaded from a camera at (0, 0, 3) with the normals bent towards it as splat_mc does; a 256 x 512 lat-long map of seeded
radiance with a sun (a 3 x 3 block x 5 000).  n_samples_x 8 (training) and 16 (evaluation): 128 and 512 shadow rays per Gaussian.
Per n and per arrangement (lanes_per_point 1 = a thread per point, 16, 64), `runs` windows after `warmup`, one call per window between
two device events; median (min, max):
  forward_ms, backward_ms (the backward kernel alone, through autograd), rays per second of each
  backward with merge_rounds 0 (every lane issues its own light_grad atomics) against the default, for the kept arrangement
Baseline, from what the tree offered before this shader: the same 2 n^2 directions per point materialised by torch ops (uniform
hemisphere directions stand in for the samplers: the baseline is not charged for sampling at all), `shadow_visibility` on them,
Lambert and GGX evaluated by torch ops, summed per point -- forward only, on a subset of the points sized to fit memory, scaled.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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
    return statistics.median(out), min(out), max(out)


def sun_map(dev):
    g = torch.Generator().manual_seed(0)
    light = torch.rand(256, 512, 3, generator=g) * 0.5 + 0.05
    light[60:63, 300:303] *= 5000.0
    return light.to(dev).contiguous()


def torch_baseline(gs, bvh, pos, nrm_bent, nrm, view, kd, ks, light, S):
    """directions, visibility and BSDF by ops the parent commit offers; returns (diff, spec) [P,3]"""
    P = pos.shape[0]
    d = torch.nn.functional.normalize(torch.randn(P, S, 3, device=pos.device), dim=-1)
    d = torch.where((d * nrm_bent[:, None]).sum(-1, keepdim=True) < 0, -d, d)
    vis = gs.shadow_visibility(bvh, pos, nrm, d.contiguous(), offset=1e-5)
    u = torch.atan2(d[..., 0], -d[..., 2]) / (2 * math.pi) + 0.5
    v = torch.acos(d[..., 1].clamp(-1, 1)) / math.pi
    H, W = light.shape[:2]
    L = light[(v * H).long().clamp(0, H - 1), (u * W).long().clamp(0, W - 1)]
    n = nrm_bent[:, None]
    wo = torch.nn.functional.normalize(view - pos, dim=-1)[:, None]
    lam = ((n * d).sum(-1) / math.pi).clamp_min(0)
    a2 = (ks[:, 1:2] ** 2).clamp(0.0064, 1.0) ** 2
    h = torch.nn.functional.normalize(wo + d, dim=-1)
    cl = lambda c: c.clamp(1e-4, 1 - 1e-4)
    nv, nl, vh, nh = (wo * n).sum(-1), (d * n).sum(-1), (wo * h).sum(-1), (n * h).sum(-1)
    c = cl(nh)
    D = a2 / (math.pi * ((c * a2 - c) * c + 1) ** 2)
    lam_f = lambda x: 0.5 * (torch.sqrt(1 + a2 * (1 - cl(x) ** 2) / cl(x) ** 2) - 1)
    G = 1 / (1 + lam_f(nv) + lam_f(nl))
    col = ((0.04 * (1 - ks[:, 2:3]) + kd * ks[:, 2:3]) * (1 - ks[:, 0:1]))[:, None]
    s = ((1 - cl(vh)) ** 5)[..., None]
    spec = (col * (1 - s) + s) * (D * G * 0.25 / nv)[..., None] * ((nv > 1e-4) & (nl > 1e-4))[..., None]
    w = (vis * (2 * math.pi / S))[..., None]
    return (lam[..., None] * L * w).sum(1), (spec * L * w).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=0, help="shade only the first N Gaussians (0: all)")
    ap.add_argument("--samples", type=int, nargs="*", default=[8, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("envshade_bench needs a GPU")
    import geosplatting_amd as gs
    from raytrace_bench import flexicubes_sphere
    dev = torch.device("cuda:0")
    v, f = flexicubes_sphere(96, dev)
    bvh = gs.MeshBVH(v, f)
    with torch.no_grad():
        splats, nrm = gs.mesh_to_splats(v, f, gs.vertex_normals(v, f))
    pos = splats.means.detach().contiguous()
    nrm = nrm.detach().contiguous()
    if a.points:
        pos, nrm = pos[:: max(1, pos.shape[0] // a.points)][:a.points].contiguous(), nrm[:: max(1, nrm.shape[0] // a.points)][:a.points].contiguous()
    P = pos.shape[0]
    view = torch.tensor([0.0, 0.0, 3.0], device=dev)
    bent = torch.where((nrm * torch.tensor([0.0, 0.0, -1.0], device=dev)).sum(-1, keepdim=True) > 1e-3, -nrm, nrm).contiguous()
    g = torch.Generator().manual_seed(1)
    kd = torch.rand(P, 3, generator=g).to(dev)
    ks = torch.cat((torch.zeros(P, 1), torch.rand(P, 1, generator=g) * 0.92 + 0.08, torch.rand(P, 1, generator=g)), -1).to(dev)
    light = sun_map(dev)
    env = gs.LatLngEnvMap(light).compute_pdf_()
    pdf, rows, cols = (t.contiguous() for t in env.tables())
    mask = torch.ones(P, device=dev)
    ro = (pos + nrm * 1e-5).contiguous()
    stat = lambda t, rays: {"ms": t[0], "ms_min_max": t[1:], "rays_per_s": rays / (t[0] * 1e-3)}
    results = {"faces": int(f.shape[0]), "points": P, "light": list(light.shape), "runs": a.runs, "device": torch.cuda.get_device_name(0), "n": {}}
    for n in a.samples:
        rays = P * 2 * n * n
        perms = gs.make_perms(n, dev, generator=None)
        r = {"rays": rays, "arrangements": {}}
        for lanes in (1, 16, 64):
            leaves = [t.clone().requires_grad_(True) for t in (pos, bent, kd, ks, light)]

            def fwd(lv=leaves, lanes=lanes, merge=-1):
                return gs.env_shade(bvh, mask, ro, lv[0], lv[1], view, lv[2], lv[3], lv[4], pdf, rows, cols, n_samples_x=n, rnd_seed=11,
                                    perms=perms, lanes_per_point=lanes, merge_rounds=merge)

            with torch.no_grad():
                t_f = timed(fwd, a.runs, a.warmup)
                d0, s0, r0 = fwd()
            entry = {"forward": stat(t_f, rays)}
            gd, gsp = torch.rand_like(d0), torch.rand_like(s0)
            for label, merge in (("backward", -1), ("backward_no_merge", 0)):
                d, s, _ = fwd(merge=merge)
                t_b = timed(lambda: torch.autograd.grad((d, s), leaves, (gd, gsp), retain_graph=True), a.runs, a.warmup)
                entry[label] = stat(t_b, rays)
            r["arrangements"][str(lanes)] = entry
            print(n, lanes, json.dumps(entry), flush=True)
        # baseline on a subset: P_b * S * 3 floats a tensor, a dozen of them alive
        S = 2 * n * n
        Pb = min(P, max(1024, (1 << 27) // (S * 3 * 16)))
        sl = slice(0, Pb)
        with torch.no_grad():
            t_base = timed(lambda: torch_baseline(gs, bvh, pos[sl], bent[sl], nrm[sl], view, kd[sl], ks[sl], light, S), max(3, a.runs // 2), 1)
        r["torch_baseline"] = {"points": Pb, "forward": stat(t_base, Pb * S), "forward_ms_scaled_to_all_points": t_base[0] * P / Pb}
        print(n, "torch_baseline", json.dumps(r["torch_baseline"]), flush=True)
        results["n"][str(n)] = r
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
