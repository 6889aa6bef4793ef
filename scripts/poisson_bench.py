#!/usr/bin/env python3
"""Time differentiable Poisson reconstruction (csrc/gs_poisson.hip through geosplatting_amd.poisson).

    python scripts/poisson_bench.py [--points 1000000] [--res 256 512] [--runs 5] [--warmup 2] [--cells 224] [--out FILE.json]

Input: `points` samples (positions and unit normals, sample_mesh_surface) of the bumpy height field of scripts/meshreg_bench.py
(cells x cells x 2 triangles; 224: 100 352 faces), scaled into the unit cube.  Each figure is the median (min, max) in ms of `runs`
windows after `warmup`, each between two device events:
  splat_fwd / splat_bwd       splat_to_grid of the three normal components; its backward to points and values for a fixed cotangent
  sample_fwd / sample_bwd     sample_grid of a scalar grid at the points; its backward to the grid and the points
  spectral_fwd / spectral_bwd the Fourier-space kernel on S [3,R,R,R/2+1] and its adjoint
  rfftn / irfftn              torch.fft (hipFFT) of the three rasters and of Phi
  extract                     mesh_from_indicator of the solved phi without a gradient (pack, classify, one read-back, fill, normals)
  whole / whole_torch         mesh_from_oriented_points forward + backward of sum(vertices . c) to points and normals, and the same
                              pipeline with the splat, the sample and the Fourier-space step composed from torch ops (index_add_,
                              advanced indexing, elementwise complex arithmetic, autograd); the triangulation is this project's in
                              both, since torch has none
  splat_torch / sample_torch  the torch compositions of the two ops alone, forward and forward + backward
`splat_added_bytes_per_s` is N x 8 corners x 3 channels x 8 bytes (64-bit integer atomics) over the time of splat_fwd, clearing and
conversion passes included, next to the chip-wide float-atomic rate of about 1.3e12 added bytes per second.
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

FLOAT_ATOMIC_BYTES_PER_S = 1.3e12


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
    return {"ms": statistics.median(out), "ms_min_max": [min(out), max(out)]}


def height_field(cells, dev):
    n = cells + 1
    ys, xs = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    x, y = xs.reshape(-1).float() / cells * 1.6 - 0.8, ys.reshape(-1).float() / cells * 1.6 - 0.8
    v = torch.stack((x, 0.15 * torch.sin(7 * x) * torch.cos(5 * y), y), 1).contiguous()
    i = (ys[:-1, :-1] * n + xs[:-1, :-1]).reshape(-1)
    f = torch.cat((torch.stack((i, i + n, i + 1), 1), torch.stack((i + 1, i + n, i + n + 1), 1)), 0)
    return v, f.contiguous()


# ---- the same pipeline from torch ops ---------------------------------------------------------------------------------------------
def _cell(p, res):
    R = torch.tensor(res, device=p.device, dtype=p.dtype)
    s = (p - torch.floor(p)) * R
    lo_f = torch.floor(s.detach())
    f = s - lo_f
    Ri = torch.tensor(res, device=p.device)
    lo = lo_f.long() % Ri
    return lo, (lo + 1) % Ri, f


def _corner(lo, hi, f, res, k):
    b = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
    idx = [hi[:, a] if b[a] else lo[:, a] for a in range(3)]
    w = [f[:, a] if b[a] else 1.0 - f[:, a] for a in range(3)]
    return (idx[0] * res[1] + idx[1]) * res[2] + idx[2], w[0] * w[1] * w[2]


def torch_splat(p, v, res):
    lo, hi, f = _cell(p, res)
    corners = [_corner(lo, hi, f, res, k) for k in range(8)]
    node = torch.cat([c[0] for c in corners])
    contrib = torch.cat([c[1][:, None] * v for c in corners])
    grid = torch.zeros(res[0] * res[1] * res[2], v.shape[1], device=p.device)
    grid.index_add_(0, node, contrib)
    return grid.T.reshape(v.shape[1], *res)


def torch_sample(grid, p):
    res = tuple(grid.shape[1:])
    lo, hi, f = _cell(p, res)
    flat = grid.reshape(grid.shape[0], -1)
    out = 0
    for k in range(8):
        node, w = _corner(lo, hi, f, res, k)
        out = out + flat[:, node].T * w[:, None]
    return out


def torch_coefficients(res, sigma, dev):
    k = torch.stack(torch.meshgrid(torch.fft.fftfreq(res[0], 1.0 / res[0], dtype=torch.float64),
                                   torch.fft.fftfreq(res[1], 1.0 / res[1], dtype=torch.float64),
                                   torch.fft.rfftfreq(res[2], 1.0 / res[2], dtype=torch.float64), indexing="ij"), 0).to(dev)
    kk = (k * k).sum(0)
    a = -(torch.exp(-2.0 * sigma * sigma * kk) * 2.0 * math.pi * k) / (-(2.0 * math.pi) ** 2 * kk + 1e-6)
    a[:, 0, 0, 0] = 0
    return torch.complex(torch.zeros_like(a), a).to(torch.complex64)


def torch_indicator(p, n, res, coeff):
    S = torch.fft.rfftn(torch_splat(p, n, res), dim=(1, 2, 3))
    phi = torch.fft.irfftn((coeff * S).sum(0), s=res, dim=(0, 1, 2))
    phi = phi - torch_sample(phi[None], p).mean()
    return -phi / phi[0, 0, 0].abs() * 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=224)
    ap.add_argument("--smoothness", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("poisson_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import poisson as GP
    dev = torch.device("cuda:0")
    v, f = height_field(a.cells, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pts, nrm = (t.contiguous() for t in gs.sample_mesh_surface(v, f, a.points, generator=gen))
    N = pts.shape[0]
    result = {"points": N, "faces": int(f.shape[0]), "smoothness": a.smoothness, "float_atomic_bytes_per_s": FLOAT_ATOMIC_BYTES_PER_S,
              "sizes": {}}
    T = lambda fn: timed(fn, a.runs, a.warmup)
    for R in a.res:
        res = (R, R, R)
        p01 = (pts * 0.4 + 0.5).clamp(0, 1).contiguous()
        r = {}
        pl, nl = p01.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
        g_grid = torch.randn(3, *res, device=dev, generator=gen)
        raster = gs.splat_to_grid(pl, nl, res)
        r["splat_fwd"] = T(lambda: gs.splat_to_grid(p01, nrm, res))
        r["splat_bwd"] = T(lambda: torch.autograd.grad(raster, (pl, nl), g_grid, retain_graph=True))
        r["splat_added_bytes_per_s"] = N * 8 * 3 * 8 / (r["splat_fwd"]["ms"] * 1e-3)
        r["splat_vs_float_atomic_rate"] = r["splat_added_bytes_per_s"] / FLOAT_ATOMIC_BYTES_PER_S
        scalar = g_grid[:1].clone().requires_grad_(True)
        smp = gs.sample_grid(scalar, pl)
        cot = torch.randn(N, 1, device=dev, generator=gen)
        r["sample_fwd"] = T(lambda: gs.sample_grid(scalar.detach(), p01))
        r["sample_bwd"] = T(lambda: torch.autograd.grad(smp, (scalar, pl), cot, retain_graph=True))
        S = torch.fft.rfftn(raster.detach(), dim=(1, 2, 3)).requires_grad_(True)
        Phi = GP.poisson_spectral(S, res, a.smoothness)
        g_Phi = torch.randn_like(torch.view_as_real(Phi.detach()))
        g_Phi = torch.view_as_complex(g_Phi)
        r["spectral_fwd"] = T(lambda: GP.poisson_spectral(S.detach(), res, a.smoothness))
        r["spectral_bwd"] = T(lambda: torch.autograd.grad(Phi, S, g_Phi, retain_graph=True))
        r["rfftn"] = T(lambda: torch.fft.rfftn(raster.detach(), dim=(1, 2, 3)))
        r["irfftn"] = T(lambda: torch.fft.irfftn(Phi.detach(), s=res, dim=(0, 1, 2)))
        phi = gs.poisson_indicator(p01, nrm, res, a.smoothness)
        r["indicator_fwd"] = T(lambda: gs.poisson_indicator(p01, nrm, res, a.smoothness))
        r["extract"] = T(lambda: gs.mesh_from_indicator(phi))
        mv, mf, _ = gs.mesh_from_indicator(phi)
        r["vertices"], r["triangles"] = int(mv.shape[0]), int(mf.shape[0])
        del raster, S, Phi, g_Phi, smp, g_grid
        c = torch.tensor([0.3, -0.5, 0.8], device=dev)

        def whole():
            pw, nw = pts.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
            vv, _f, _n = gs.mesh_from_oriented_points(pw, nw, R, a.smoothness)
            (vv * c).sum().backward()
            return pw.grad, nw.grad

        coeff = torch_coefficients(res, a.smoothness, dev)

        def whole_torch():
            pw, nw = pts.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
            ph = torch_indicator((pw * 0.4 + 0.5).clamp(0, 1), nw, res, coeff)
            vv, _f, _n = gs.mesh_from_indicator(ph)
            (vv * c).sum().backward()
            return pw.grad, nw.grad

        (ga, gb), (ta, tb) = whole(), whole_torch()
        r["whole_vs_torch_max_rel_diff"] = [float((ga - ta).abs().max() / ta.abs().max()), float((gb - tb).abs().max() / tb.abs().max())]
        r["whole"] = T(whole)
        r["whole_torch"] = T(whole_torch)

        def splat_torch_fb():
            pw, nw = p01.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
            torch_splat(pw, nw, res).sum().backward()

        def sample_torch_fb():
            pw = p01.clone().requires_grad_(True)
            torch_sample(phi[None], pw).sum().backward()

        def splat_ours_fb():
            pw, nw = p01.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
            gs.splat_to_grid(pw, nw, res).sum().backward()

        def sample_ours_fb():
            pw = p01.clone().requires_grad_(True)
            gs.sample_grid(phi[None], pw).sum().backward()

        with torch.no_grad():
            r["splat_torch_fwd"] = T(lambda: torch_splat(p01, nrm, res))
            r["sample_torch_fwd"] = T(lambda: torch_sample(phi[None], p01))
        r["splat_torch_fwd_bwd"] = T(splat_torch_fb)
        r["splat_fwd_bwd"] = T(splat_ours_fb)
        r["sample_torch_fwd_bwd"] = T(sample_torch_fb)
        r["sample_fwd_bwd"] = T(sample_ours_fb)
        r["splat_sample_speedup_vs_torch"] = (r["splat_torch_fwd_bwd"]["ms"] + r["sample_torch_fwd_bwd"]["ms"]) / \
            (r["splat_fwd_bwd"]["ms"] + r["sample_fwd_bwd"]["ms"])
        r["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
        result["sizes"][str(R)] = r
        print(R, json.dumps(r), flush=True)
        del phi, coeff
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
