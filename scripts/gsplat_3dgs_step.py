"""GSplatter's rasterization call (rfstudio/model/gsplat.py:188-282: SH colours, rasterize_mode='classic', info["means2d"] kept
for densification) forward + backward of one view at the bench size, next to today's path -- the command rocprofv3 traces for
the per-kernel split.   usage: python scripts/gsplat_3dgs_step.py [iters]

Configurations: sh_degree=None antialiased | sh_degree=None classic | sh_degree=3 classic (K = 16) | the same with
means2d_grad=True.  Also prints the SH coefficient traffic of the projection kernels (the floor at 6.3 TB/s)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import geosplatting_amd as gs, geosplatting_amd.synthetic as syn
from geosplatting_amd.engine import params_from_scene
dev = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
scene = syn.sphere_scene(7, seed=1, cubemap_res=64, device=dev)
cam = syn.blender_cameras(num=8, width=800, height=800)[0]
p = params_from_scene(scene, dev)
N = p.means.shape[0]
g = torch.Generator().manual_seed(3)
rgb = torch.rand(N, 3, generator=g).to(dev).requires_grad_(True)
shs = (torch.randn(N, 16, 3, generator=g) * 0.1).to(dev)
shs[:, 0] = (torch.rand(N, 3, generator=g).to(dev) - 0.5) / 0.28209479177387814
shs.requires_grad_(True)
means = p.means.detach().clone().requires_grad_(True)
scales = p.scales.exp(); opac = torch.sigmoid(p.opacities).squeeze(-1)
vm, K = cam.view_matrix.to(dev)[None], cam.intrinsic_matrix.to(dev)[None]
CONFIGS = [("sh None, antialiased", dict(colors=rgb)),
           ("sh None, classic", dict(colors=rgb, rasterize_mode="classic")),
           ("sh 3 (K=16), classic", dict(colors=shs, sh_degree=3, rasterize_mode="classic")),
           ("sh 3 (K=16), classic, means2d_grad", dict(colors=shs, sh_degree=3, rasterize_mode="classic", means2d_grad=True))]


def one(kw):
    fn = gs.rasterization_3dgs if kw.get("rasterize_mode") == "classic" else gs.rasterization
    kw = dict(kw, means2d_grad=kw.get("means2d_grad", False))
    r, a, meta = fn(means, p.quats, scales, opac, viewmats=vm, Ks=K, width=800, height=800, **kw)
    if kw.get("means2d_grad"):
        meta["means2d"].retain_grad()
    (r.sum() + a.sum()).backward()
    means.grad = None; rgb.grad = None; shs.grad = None
    return meta


for name, kw in CONFIGS:
    for _ in range(3):
        meta = one(kw)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        one(kw)
    t1.record()
    torch.cuda.synchronize()
    print(f"{name:38s}: {t0.elapsed_time(t1) / iters:.3f} ms per view fwd+bwd  (N={N}, V={meta['radii'].shape[0]})")
V = meta["radii"].shape[0]
fwd_b, bwd_b = V * 16 * 3 * 4, N * 16 * 3 * 4 + V * 16 * 3 * 4
print(f"SH coefficient traffic: forward {fwd_b / 1e6:.0f} MB (floor {fwd_b / 6.3e12 * 1e3:.3f} ms at 6.3 TB/s), "
      f"backward {bwd_b / 1e6:.0f} MB (floor {bwd_b / 6.3e12 * 1e3:.3f} ms)")
