#!/usr/bin/env python3
"""Time the projection backward with and without the gradient of the view matrix, and the same twelve numbers from plain torch.

    python scripts/viewgrad_bench.py [--level 7] [--res 800] [--runs 5] [--inner 10] [--out FILE.json]

The 1 966 080-Gaussian sphere scene at 800 x 800 (icosphere level 7, as bench.py), one view, random packed cotangents.  Per
configuration (plain colours antialiased; SH degree 3, K = 16, classic):
    gs_project_bwd_ex      the parameter gradients alone
    gs_project_bwd_view    the same plus v_viewmat: project_bwd_view_kernel (wave and workgroup sums in fp64, one row of 12 doubles per
                           256 Gaussians) and project_view_sum_kernel (one workgroup adds the 7 680 rows and rounds once)
    torch                  float32 autograd on the device of the restated forward (means2d, conics, opacity * compensation, depth,
                           SH colours) with the view matrix as the one leaf: the twelve numbers and nothing else
Device events around --inner calls, median of --runs, the three alternating.  The second launch by itself is read from a kernel
trace of this script (rocprofv3 --kernel-trace --stats, a run of its own).  Needs a GPU; there is no CPU path.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import geosplatting_amd as gs                                              # noqa: E402
import geosplatting_amd.synthetic as syn                                   # noqa: E402
from geosplatting_amd import _lib as L                                     # noqa: E402
from geosplatting_amd.engine import params_from_scene                      # noqa: E402

R = importlib.import_module("geosplatting_amd.rasterization")


def torch_view_grad(means, quats, scales, opac, vm0, K, W, H, gids, cot, classic, sh):
    """v_viewmat [4,4] by float32 autograd of the restated forward over the visible Gaussians"""
    vm2, vc, vo, vd, rgb = cot
    g = gids.long()
    m, q, s, o = means[g], quats[g], scales[g], opac[g]
    vm = vm0.clone().requires_grad_(True)
    Rm, t = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    mc = m @ Rm.T + t
    qn = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = qn.unbind(-1)
    Rq = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = Rq * s[:, None, :]
    covc = Rm @ (M @ M.transpose(-1, -2)) @ Rm.T
    X, Y, Z = mc.unbind(-1)
    lim = lambda a, f, n: a / f + 0.3 * 0.5 * n / f
    rz = 1.0 / Z
    tx = Z * torch.minimum(lim(W - cx, fx, W), torch.maximum(-lim(cx, fx, W), X * rz))
    ty = Z * torch.minimum(lim(H - cy, fy, H), torch.maximum(-lim(cy, fy, H), Y * rz))
    zero = torch.zeros_like(Z)
    J = torch.stack([fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz], -1).reshape(-1, 2, 3)
    c2 = J @ covc @ J.transpose(-1, -2)
    det0 = c2[:, 0, 0] * c2[:, 1, 1] - c2[:, 0, 1] * c2[:, 1, 0]
    c00, c11, c01 = c2[:, 0, 0] + 0.3, c2[:, 1, 1] + 0.3, c2[:, 0, 1]
    det = c00 * c11 - c01 * c2[:, 1, 0]
    comp = torch.sqrt(torch.clamp(det0 / det, min=1e-12))
    conics = torch.stack([c11 / det, -c01 / det, c00 / det], -1)
    m2d = torch.stack([fx * X * rz + cx, fy * Y * rz + cy], -1)
    loss = (m2d * vm2).sum() + (conics * vc).sum() + ((o if classic else o * comp) * vo).sum() + (Z * vd).sum()
    if sh is not None:
        from tests import surfel_ref
        loss = loss + (surfel_ref.sh_colors(3, m, -(Rm.T @ t), sh[g]) * rgb).sum()
    loss.backward()
    return vm.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viewgrad_bench needs a GPU")
    dev = torch.device("cuda:0")
    lib = L.lib()
    scene = syn.sphere_scene(a.level, seed=1, cubemap_res=64, device=dev)
    cam = syn.blender_cameras(num=8, width=a.res, height=a.res)[0]
    p = params_from_scene(scene, dev)
    N = p.means.shape[0]
    gen = torch.Generator().manual_seed(3)
    means, quats = p.means.detach().contiguous(), p.quats.detach().contiguous()
    scales, opac = p.scales.detach().exp().contiguous(), torch.sigmoid(p.opacities.detach()).squeeze(-1).contiguous()
    rgb = torch.rand(N, 3, generator=gen).to(dev)
    shs = (torch.randn(N, 16, 3, generator=gen) * 0.1).to(dev)
    vm, K = cam.view_matrix.to(dev).contiguous(), cam.intrinsic_matrix.to(dev).contiguous()
    W = H = a.res
    stride = lib.gs_raster_grad_stride(4)
    results = []
    for name, sh, classic in (("plain colours, antialiased", None, False), ("SH degree 3 (K = 16), classic", shs, True)):
        deg = None if sh is None else 3
        pr = R._project_stage(means, quats, scales, opac, rgb if sh is None else sh, vm, K, W, H, 16, 0.3, 0.01, 1e10, 0.0,
                              sh_degree=deg, classic=classic)
        torch.cuda.synchronize()
        V = int(pr.host_counts[0])
        gids, conics, comps = pr.bufs[0], pr.bufs[4], pr.bufs[5]
        v_packed = (torch.rand(V, stride, generator=gen) * 2 - 1).to(dev)
        v_depths = v_packed[:, 9].contiguous()
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        o = [f(N, 3), f(N, 4), f(N, 3), f(N), f(N, 3), f(N, 16, 3)]
        out16 = f(16)
        ws_bytes = lib.gs_project_bwd_view_ws_bytes(N)
        ws = L.workspace(ws_bytes, dev)
        common = (N, V, 3, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opac), L.ptr(vm), L.ptr(K), W, H, 0.3, L.ptr(gids), L.ptr(conics),
                  L.ptr(comps), L.ptr(v_packed), stride, L.ptr(v_depths), L.ptr(sh), 0 if sh is None else 16, -1 if sh is None else 3,
                  1 if classic else 0, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.ptr(o[4]) if sh is None else None,
                  None if sh is None else L.ptr(o[5]), 0)
        cot = (v_packed[:, 0:2], v_packed[:, 2:5], v_packed[:, 5], v_depths, v_packed[:, 6:9])

        def run_ex():
            L.check(lib.gs_project_bwd_ex(*common, L.stream()), "gs_project_bwd_ex")

        def run_view():
            L.check(lib.gs_project_bwd_view(*common, L.ptr(out16), L.ptr(ws), ws_bytes, L.stream()), "gs_project_bwd_view")

        def run_torch():
            return torch_view_grad(means, quats, scales, opac, vm, K, float(W), float(H), gids[:V], cot, classic, sh)

        def timed(fn, inner):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / inner

        for fn in (run_ex, run_view, run_torch):
            fn(); fn()
        torch.cuda.synchronize()
        t = dict(ex=[], view=[], torch=[])
        for _ in range(a.runs):                                             # alternate the three
            t["ex"].append(timed(run_ex, a.inner))
            t["view"].append(timed(run_view, a.inner))
            t["torch"].append(timed(run_torch, 1))
        med = {k: statistics.median(v) for k, v in t.items()}
        run_view()
        got = out16.reshape(4, 4).clone()
        ref = run_torch()
        rel = float((got - ref).abs().max() / ref.abs().max())
        results.append(dict(config=name, N=N, V=V, ex_ms=med["ex"], view_ms=med["view"], torch_ms=med["torch"],
                            view_over_ex=med["view"] / med["ex"], torch_over_view=med["torch"] / med["view"],
                            ex_ms_all=t["ex"], view_ms_all=t["view"], torch_ms_all=t["torch"], ws_bytes=int(ws_bytes),
                            max_rel_diff_vs_torch_f32=rel))
        print(f"{name:32s} N={N} V={V}: ex {med['ex']:.3f} ms | view {med['view']:.3f} ms ({med['view'] / med['ex']:.3f} x) | "
              f"torch f32 {med['torch']:.2f} ms | v_viewmat vs torch f32: {rel:.2e} of the largest entry")
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), res=a.res, runs=a.runs, inner=a.inner, results=results))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
