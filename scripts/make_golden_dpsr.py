#!/usr/bin/env python3
"""Generate tests/golden/ref_dpsr.npz from the reference's OWN differentiable Poisson solver, on the CPU:

    python scripts/make_golden_dpsr.py <path to the reference checkout>

What it pins: point_rasterize and DPSR.forward (rfstudio/graphics/_mesh/_dpsr/ops.py) executed as they are, fp32, on seeded
noisy oriented points on a bumpy sphere -- two cubic grids, a non-cubic one, an odd one and one without shift / scale -- plus the
gradients torch autograd gives the reference for a seeded cotangent.  Arrays only: inputs, raster, phi, cotangent, gradients.  No
mesh (PSR2Mesh needs skimage).  It also prints how far the reference's fp32 results are from tests/poisson_ref.py's float64
restatement: the E_ref tests/test_poisson_cpu.py recomputes and tests/test_gpu_poisson.py scales its bound from.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT", "."))
import poisson_ref as P                                                   # noqa: E402

for name in ["open3d", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils",
             "cv2", "pyexr", "trimesh", "nvdiffrast", "nvdiffrast.torch", "kornia", "kornia.filters", "gsplat",
             "torchmetrics", "torchmetrics.functional", "torchmetrics.functional.image", "ffmpegcv", "nerfacc", "tyro",
             "skimage", "skimage.measure", "rfviser", "viser", "appdirs", "huggingface_hub", "pytorch3d",
             "pytorch3d.loss", "pytorch3d.structures", "rfstudio.graphics._mesh._optix", "rfstudio.graphics._mesh._splitsum",
             "tinycudann", "plotext", "imageio", "lpips", "matplotlib", "matplotlib.pyplot", "viser.transforms",
             "rfviser.transforms", "torchmetrics.image", "torchmetrics.image.lpip", "jaxtyping"]:
    sys.modules.setdefault(name, MagicMock())

from rfstudio.graphics._mesh._dpsr import ops as R                        # noqa: E402

# tag, resolution, N, sigma, shift, scale, seed (r16_plain solves r16's points again: its inputs and raster are r16's, not stored twice)
CASES = [("r16", (16, 16, 16), 500, 0.02, True, True, 0), ("r24", (24, 24, 24), 1500, 0.02, True, True, 1),
         ("r8x12x10", (8, 12, 10), 300, 0.05, True, True, 2), ("r9", (9, 9, 9), 200, 0.05, True, True, 3),
         ("r16_plain", (16, 16, 16), 500, 0.02, False, False, 0)]
out = {}
for tag, res, N, sigma, shift, scale, seed in CASES:
    p, n = P.bumpy_sphere(N, seed)
    pl, nl = p.clone().requires_grad_(True), n.clone().requires_grad_(True)
    raster = R.point_rasterize(pl[None], nl[None], res)[0]
    phi = R.DPSR(res=list(res), sig=sigma, scale=scale, shift=shift)(pl[None], nl[None])[0]
    cot = torch.round(16.0 * torch.randn(res, generator=torch.Generator().manual_seed(100 + seed))) / 16.0      # (compresses)
    (phi * cot).sum().backward()
    out[f"{tag}.res"] = np.array(res)
    out[f"{tag}.sigma"] = np.array(sigma)
    out[f"{tag}.flags"] = np.array([shift, scale])
    if tag != "r16_plain":
        out[f"{tag}.points"] = p.numpy(); out[f"{tag}.normals"] = n.numpy()
        out[f"{tag}.raster"] = raster.detach().numpy()
    out[f"{tag}.phi"] = phi.detach().numpy()
    out[f"{tag}.cot"] = cot.numpy()
    out[f"{tag}.grad.points"] = pl.grad.numpy(); out[f"{tag}.grad.normals"] = nl.grad.numpy()
    p64, n64 = p.double().requires_grad_(True), n.double().requires_grad_(True)
    phi64 = P.indicator(p64, n64, res, sigma, shift, scale)
    (phi64 * cot.double()).sum().backward()
    e_phi = float((phi.detach().double() - phi64.detach()).abs().max())
    e_gp = float((pl.grad.double() - p64.grad).abs().max() / p64.grad.abs().max())
    e_gn = float((nl.grad.double() - n64.grad).abs().max() / n64.grad.abs().max())
    e_r = float((raster.detach().double() - P.splat(p, n, res)).abs().max())
    print(f"{tag}: max|phi| {float(phi.detach().abs().max()):.3f}  E_ref phi {e_phi:.2e}  grad points {e_gp:.2e}  grad normals {e_gn:.2e}"
          f"  raster {e_r:.2e}")
np.savez_compressed(os.path.join(OUT, "ref_dpsr.npz"), **out)
print("wrote", os.path.join(OUT, "ref_dpsr.npz"), os.path.getsize(os.path.join(OUT, "ref_dpsr.npz")), "bytes")
