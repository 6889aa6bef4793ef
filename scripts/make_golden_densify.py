#!/usr/bin/env python3
"""Generate tests/golden/ref_densify.npz from the reference's OWN Splats.densify_and_cull / Splats.cull / mutate_params
(build container only; the reference checkout on PYTHONPATH, run from outside this repository):

    PYTHONPATH=<reference checkout> python <repo>/scripts/make_golden_densify.py

The stub-import recipe of scripts/make_golden_loss.py plus a throw-away `jaxtyping` stub.  Only input / output
vectors are written.  About 4 000 Gaussians of SH degree 3 whose classes are mixed on purpose, and whose decision quantities all keep
1e-4 (relative) away from their thresholds, so that an `exp` that differs in the last bit cannot move a row to another class and
the classification can be compared bit for bit on any machine.  Inputs are drawn on coarse binary grids (they are exact fp32
values either way): the copied rows then compress, and the file stays small.
"""
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")

stub = tempfile.mkdtemp()
os.makedirs(os.path.join(stub, "jaxtyping"))
with open(os.path.join(stub, "jaxtyping", "__init__.py"), "w") as f:
    f.write("class _A:\n    def __class_getitem__(cls, item):\n        return cls\n"
            "Float = Float32 = Float64 = Int = Int32 = Int64 = Bool = Shaped = UInt8 = Num = Integer = _A\n"
            "def __getattr__(name):\n    return _A\n")
sys.path.insert(0, stub)
for name in ["open3d", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils",
             "cv2", "pyexr", "trimesh", "nvdiffrast", "nvdiffrast.torch", "kornia", "kornia.filters", "gsplat",
             "torchmetrics", "torchmetrics.functional", "torchmetrics.functional.image", "ffmpegcv", "nerfacc", "tyro",
             "skimage", "skimage.measure", "rfviser", "viser", "appdirs", "huggingface_hub", "pytorch3d",
             "pytorch3d.loss", "pytorch3d.structures", "rfstudio.graphics._mesh._optix", "rfstudio.graphics._mesh._splitsum",
             "tinycudann", "plotext", "imageio", "lpips", "matplotlib", "matplotlib.pyplot", "viser.transforms",
             "rfviser.transforms", "torchmetrics.image", "torchmetrics.image.lpip"]:
    sys.modules.setdefault(name, MagicMock())

sys.path.insert(0, ROOT)
from tests import densify_ref                                              # noqa: E402
from rfstudio.graphics import Splats                                       # noqa: E402
from rfstudio.optim import ModuleOptimizers, Optimizer                     # noqa: E402

N, S, W, H = 4000, 2, 800, 600
GRAD_T, SIZE_T, ALPHA_T, SCALE_T = 0.0002, 0.01, 0.1, 0.5
SEED_SPLIT = 4242
g = torch.Generator().manual_seed(2025)


def grid(x, bits):
    return torch.round(x * (1 << bits)) / (1 << bits)


def near(x, t):
    return (x - t).abs() <= 1e-4 * abs(t) * 4                             # four times the margin the golden promises


def draw():
    means = grid(torch.rand(N, 3, generator=g) * 2 - 1, 10)
    # scale_max from 0.002 to 0.8, log-uniform: splits (> 0.01), duplicates (<= 0.01) and too-big rows (> 0.5)
    smax = torch.exp(torch.rand(N, generator=g) * (np.log(0.8) - np.log(0.002)) + np.log(0.002))
    scales = grid((smax[:, None] * (0.3 + 0.7 * torch.rand(N, 3, generator=g))).log(), 8)
    scales[torch.arange(N), torch.randint(0, 3, (N,), generator=g)] = grid(smax.log(), 8)
    quats = grid(torch.randn(N, 4, generator=g), 8) * (0.5 + grid(torch.rand(N, 1, generator=g), 4))    # not unit length
    quats[(quats.abs().sum(-1) == 0)] = 1.0
    opacities = grid(torch.randn(N, 1, generator=g) * 1.8 - 1.0, 8)
    colors = grid(torch.rand(N, 3, generator=g), 6)
    shs = torch.randint(-2, 3, (N, 15, 3), generator=g).float() / 4 * (torch.rand(N, 15, 3, generator=g) < 0.25)     # sparse: compresses
    shs[:, 0, 0] = torch.arange(N).float()                                # every row carries its own index: a wrong source row shows
    vis = torch.randint(1, 40, (N,), generator=g).float()
    high = torch.rand(N, generator=g) < 0.55
    avg = torch.where(high, 3e-4 + 2e-3 * torch.rand(N, generator=g), 1e-5 + 1.4e-4 * torch.rand(N, generator=g))
    xys = avg * vis / (0.5 * max(W, H))
    return means, scales, quats, opacities, colors, shs, xys, vis


means, scales, quats, opacities, colors, shs, xys, vis = draw()
half_extent = 0.5 * max(W, H)
for _ in range(50):                                                        # move rows off the thresholds
    scale_max = scales.exp().max(-1).values
    bad = near(scale_max, SIZE_T) | near(scale_max, SCALE_T) | near(opacities.sigmoid()[:, 0], ALPHA_T) | \
        near(half_extent * (xys / vis), GRAD_T)
    if not bad.any():
        break
    scales[bad] += 1.0 / 64
    opacities[bad] += 1.0 / 64
    xys[bad] *= 1.01
else:
    raise SystemExit("could not separate the decision quantities from their thresholds")

scale_max = scales.exp().max(-1).values
avg = half_extent * (xys / vis)
alpha = opacities.sigmoid()[:, 0]
for q, t in ((scale_max, SIZE_T), (scale_max, SCALE_T), (alpha, ALPHA_T), (avg, GRAD_T)):
    assert ((q - t).abs() > 1e-4 * t).all()
high = avg > GRAD_T
splits, dups = high & (scale_max > SIZE_T), high & (scale_max <= SIZE_T)
culls = (alpha < ALPHA_T) | (scale_max > SCALE_T)
kept = ~(culls | splits)
for name, m in (("kept", kept), ("split", splits), ("dup", dups), ("culled", culls)):
    assert m.float().mean() >= 0.10, (name, float(m.float().mean()))
assert (culls & (splits | dups)).float().mean() >= 0.01


def make():
    sp = Splats(means=means.clone(), scales=scales.clone(), quats=quats.clone(), colors=colors.clone(), shs=shs.clone(),
                opacities=opacities.clone()).requires_grad_(True)
    return sp


def fields(sp, prefix):
    return {prefix + k: getattr(sp, k).detach().numpy().copy() for k in ("means", "scales", "quats", "colors", "shs", "opacities")}


# ---- one densify_and_cull with an Adam state that follows it
sp = make()
optimizers = ModuleOptimizers(mixed_precision=False, optim_dict={
    "means": Optimizer(category=torch.optim.Adam, modules=sp.as_module(field_name="means"), lr=1e-3)})
wgt = torch.randn(N, 3, generator=g)
optimizers.backward((sp.means * wgt).sum())
optimizers.step()
adam = optimizers.optimizers["means"]
exp_avg_before = adam.state[adam.param_groups[0]["params"][0]]["exp_avg"].clone()
with torch.no_grad():
    sp.means.copy_(means)                                                  # the step was only there to create the Adam state
means_after_step = sp.means.detach().clone()
sp.annotate_(xys_grad_norm=xys.clone(), vis_counts=vis.clone(), last_width=torch.tensor([float(W)]), last_height=torch.tensor([float(H)]))
torch.manual_seed(SEED_SPLIT)
indices = sp.densify_and_cull(densify_grad_thresh=GRAD_T, densify_size_thresh=SIZE_T, num_splits=S, cull_alpha_thresh=ALPHA_T,
                              cull_scale_thresh=SCALE_T)
optimizers.mutate_params(indices=indices)
exp_avg_after = adam.state[adam.param_groups[0]["params"][0]]["exp_avg"].clone()
assert adam.param_groups[0]["params"][0] is sp.means

n_sel, n_split, n_dup = int(kept.sum()), int(splits.sum()), int(dups.sum())
assert sp.shape[0] == n_sel + S * n_split + n_dup
torch.manual_seed(SEED_SPLIT)
randn = torch.randn(S, n_split, 3)
# the recovered samples reproduce the reference's child means, or nothing is written
child = densify_ref.child_means({"means": means_after_step[splits], "scales": scales[splits], "quats": quats[splits]}, randn)
got = sp.means.detach()[n_sel:n_sel + S * n_split].view(S, n_split, 3)
assert torch.allclose(child, got, rtol=1e-5, atol=1e-6), float((child - got).abs().max())

out = dict(means=means_after_step.numpy(), scales=scales.numpy(), quats=quats.numpy(), colors=colors.numpy(), shs=shs.numpy(),
           opacities=opacities.numpy(), xys_grad_norm=xys.numpy(), vis_counts=vis.numpy(), last_width=np.float32(W),
           last_height=np.float32(H), densify_grad_thresh=np.float64(GRAD_T), densify_size_thresh=np.float64(SIZE_T),
           cull_alpha_thresh=np.float64(ALPHA_T), cull_scale_thresh=np.float64(SCALE_T), num_splits=np.int64(S), randn=randn.numpy(),
           totals=np.array([n_sel, n_split, n_dup, sp.shape[0]], dtype=np.int64), indices=indices.numpy()[:, 0].astype(np.int64),
           exp_avg_before=exp_avg_before.numpy(), exp_avg_after=exp_avg_after.numpy())
out.update(fields(sp, "out_"))

# ---- one cull on the same inputs
sp2 = make()
with torch.no_grad():
    sp2.means.copy_(means_after_step)
kept2 = sp2.cull(cull_alpha_thresh=ALPHA_T, cull_scale_thresh=SCALE_T)
out["cull_indices"] = kept2.numpy()[:, 0].astype(np.int64)
out.update(fields(sp2, "cull_"))

path = os.path.join(OUT, "ref_densify.npz")
np.savez_compressed(path, **out)
print("N", N, "->", sp.shape[0], "kept/split/dup", n_sel, n_split, n_dup, "culled", int(culls.sum()), "culled&(split|dup)",
      int((culls & (splits | dups)).sum()), "cull ->", sp2.shape[0], "bytes", os.path.getsize(path))
