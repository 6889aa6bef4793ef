"""rasterization_2dgs ('RGB+ED', distloss on) forward + backward of one view at the bench scene's size (level-7 sphere scene, 2 M surface
Gaussians, 800 x 800, degree-3 SH colours), next to rasterization_3dgs ('RGB+ED') on the same scene as the yardstick, with the split
of the surfel call into its stages (each timed alone between device synchronisations).
usage: python scripts/surfel_bench.py [iters]      prints one JSON line at the end"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import geosplatting_amd as gs, geosplatting_amd.synthetic as syn
from geosplatting_amd import surfels
from geosplatting_amd.engine import params_from_scene

dev = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
scene = syn.sphere_scene(7, seed=1, cubemap_res=64, device=dev)
cam = syn.blender_cameras(num=8, width=800, height=800)[0]
p = params_from_scene(scene, dev)
N = p.means.shape[0]
g = torch.Generator().manual_seed(3)
shs = (torch.randn(N, 16, 3, generator=g) * 0.1).to(dev)
shs[:, 0] = (torch.rand(N, 3, generator=g).to(dev) - 0.5) / 0.28209479177387814
leaves = [p.means.detach().clone(), p.quats.detach().clone(), p.scales.detach().exp(), torch.sigmoid(p.opacities.detach()).squeeze(-1), shs]
for t in leaves:
    t.requires_grad_(True)
vm, K = cam.view_matrix.to(dev)[None], cam.intrinsic_matrix.to(dev)[None]
kw = dict(viewmats=vm, Ks=K, width=800, height=800, sh_degree=3, render_mode="RGB+ED")


def surfel_view():
    r, a, n, pn, d, _m, meta = gs.rasterization_2dgs(*leaves, distloss=True, **kw)
    (r.sum() + a.sum() + n.sum() + d.sum()).backward()
    return meta


def splat_view():
    r, a, meta = gs.rasterization_3dgs(*leaves, **kw)
    (r.sum() + a.sum()).backward()
    return meta


def timed(fn, n):
    for _ in range(2):
        meta = fn()
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
        for t in leaves:
            t.grad = None
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, meta


def stage(fn, n):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, out


ms_2d, meta = timed(surfel_view, iters)
ms_3d, meta3 = timed(splat_view, iters)
res = {"N": N, "V_2dgs": int(meta["radii"].shape[0]), "I_2dgs": int(meta["flatten_ids"].shape[0]), "V_3dgs": int(meta3["radii"].shape[0]),
       "I_3dgs": int(meta3["flatten_ids"].shape[0]), "ms_2dgs_fwd_bwd": ms_2d, "ms_3dgs_fwd_bwd": ms_3d}

# the split: the stages of the surfel call one by one (autograd and the torch glue left out)
with torch.no_grad():
    det = [t.detach() for t in leaves]
    vm2, K2 = vm[0].contiguous(), K[0].contiguous()
    res["ms_project_bin"], st = stage(lambda: surfels._project_bin(*det, vm2, K2, 800, 800, 16, 0.01, 1e10, 0.0, 3, True), iters)
fwd = lambda: surfels._raster_fwd(st, None, 800, 800, 16, True, True)
res["ms_raster_fwd"], (render, alphas, normals, distort, _median, last_ids, final_T, final_D) = stage(fwd, iters)
cots = [torch.ones_like(o) for o in (render, alphas, normals, distort)]
res["ms_raster_bwd"], _ = stage(lambda: surfels._raster_bwd(st, None, 800, 800, 16, True, True, last_ids, final_T, final_D, *cots), iters)
print(f"2dgs {ms_2d:.3f} ms   3dgs {ms_3d:.3f} ms per view forward + backward (N={N})")
print(json.dumps(res))
