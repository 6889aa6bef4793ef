#!/usr/bin/env python3
"""Time the bilateral denoiser (csrc/gs_denoise.hip through geosplatting_amd.bilateral_denoiser) at the stage-3 workload shape.

    python scripts/denoise_bench.py [--runs 5] [--warmup 2] [--calls 20] [--size 800] [--out FILE.json]

Image: size x size (800: the reference's training resolution), sigma = 2 (2 * shadow_scale), so R = 11 and 23 x 23 = 529 taps a pixel;
C = 3 (one of the reference's three calls) and C = 8 (the one call splat_mc_deferred makes); zdz with one channel.  Guides: unit normals
turning smoothly with two creases, a depth ramp with a step -- weights that are neither all one nor all zero.
Per C and per form (tiled: the halo staged in LDS; plain: taps from global memory), `runs` windows after `warmup`, `calls` calls per
window between two device events (a single call is a fraction of a millisecond); median (min, max) of the per-call forward_ms and
backward_ms (the backward kernel alone, through autograd) and the taps per second of each.  The forms' outputs are compared bit for
bit on the way.
Baseline: the same filter composed from torch ops on the same device -- a loop over the 529 offsets of shifted slices of zero-padded
inputs (a zero normal gives the weight 0), the weights under no_grad, the backward by autograd through the products.
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


def timed(fn, runs, warmup, calls=1):
    """per-call milliseconds of `runs` windows of `calls` back-to-back calls each"""
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


def guides(size, dev):
    y, x = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    tilt = 0.4 * torch.sin(x * (6.0 / size)) + torch.where((x > 0.3 * size) & (x < 0.7 * size), 0.9, 0.0)
    roll = 0.3 * torch.cos(y * (5.0 / size))
    nrm = torch.stack((torch.sin(tilt) * torch.cos(roll), torch.sin(roll), torch.cos(tilt) * torch.cos(roll)), -1)
    z = 2.0 + x * (0.5 / size) + y * (0.8 / size) + torch.where(y > 0.5 * size, 0.3, 0.0)
    return nrm[None].contiguous().to(dev), z[None, ..., None].contiguous().to(dev)


def torch_composition(col, nrm, zdz, sigma):
    """out of the header's formulas by shifted slices; differentiable in col"""
    B, H, W, C = col.shape
    R, v = 2 * math.ceil(2.5 * sigma) + 1, sigma * sigma
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, R, R, R, R))
    colp, nrmp, zp = pad(col), pad(nrm), pad(zdz[..., :1])
    z, dz = zdz[..., :1], zdz[..., -1:]
    S, Wsum = torch.zeros_like(col), torch.zeros_like(z)
    for fy in range(-R, R + 1):
        for fx in range(-R, R + 1):
            win = (slice(None), slice(R + fy, R + fy + H), slice(R + fx, R + fx + W))
            with torch.no_grad():
                d2 = float(fx * fx + fy * fy)
                w_n = (nrmp[win] * nrm).sum(-1, keepdim=True).clamp(1e-4, 1.0) ** 128
                w_z = torch.exp(-(zp[win] - z).abs() / (dz * math.sqrt(d2)).clamp_min(1e-4))
                w = math.exp(-d2 / (2.0 * v)) * w_n * w_z
            S = S + w * colp[win]
            Wsum = Wsum + w
    return S / Wsum.clamp_min(1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls of a HIP form per timed window (the torch composition: one)")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench needs a GPU")
    import geosplatting_amd as gs
    dev = torch.device("cuda:0")
    sigma = 2.0
    nrm, zdz = guides(a.size, dev)
    taps = a.size * a.size * (2 * gs.filter_radius(sigma) + 1) ** 2
    stat = lambda t: {"ms": t[0], "ms_min_max": t[1:], "taps_per_s": taps / (t[0] * 1e-3)}
    results = {"size": a.size, "sigma": sigma, "radius": gs.filter_radius(sigma), "taps": taps, "runs": a.runs, "calls": a.calls,
               "device": torch.cuda.get_device_name(0), "C": {}}
    for C in (3, 8):
        g = torch.Generator().manual_seed(C)
        col = torch.rand(1, a.size, a.size, C, generator=g).to(dev)
        grad = torch.randn(1, a.size, a.size, C, generator=g).to(dev)
        r, outs = {}, {}
        for form, tiled in (("tiled", True), ("plain", False)):
            leaf = col.clone().requires_grad_(True)
            with torch.no_grad():
                t_f = timed(lambda: gs.bilateral_denoiser(leaf, nrm, zdz, sigma, tiled=tiled), a.runs, a.warmup, a.calls)
            out = gs.bilateral_denoiser(leaf, nrm, zdz, sigma, tiled=tiled)
            t_b = timed(lambda: torch.autograd.grad(out, leaf, grad, retain_graph=True), a.runs, a.warmup, a.calls)
            outs[form] = (out.detach(), torch.autograd.grad(out, leaf, grad)[0])
            r[form] = {"forward": stat(t_f), "backward": stat(t_b)}
            print(C, form, json.dumps(r[form]), flush=True)
        r["forms_agree_bit_for_bit"] = bool(torch.equal(outs["tiled"][0], outs["plain"][0]) and torch.equal(outs["tiled"][1], outs["plain"][1]))
        leaf = col.clone().requires_grad_(True)
        with torch.no_grad():
            t_f = timed(lambda: torch_composition(leaf, nrm, zdz, sigma), a.runs, 1)
        base = torch_composition(leaf, nrm, zdz, sigma)
        t_b = timed(lambda: torch.autograd.grad(base, leaf, grad, retain_graph=True), a.runs, 1)
        r["torch_composition"] = {"forward": stat(t_f), "backward": stat(t_b),
                                  "max_abs_difference_to_hip": float((base.detach() - outs["plain"][0]).abs().max())}
        print(C, "torch_composition", json.dumps(r["torch_composition"]), flush=True)
        del base
        results["C"][str(C)] = r
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
