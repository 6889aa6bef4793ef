"""Plain-torch restatement of the reference's adaptive density control, the yardstick of the densify tests and of
scripts/densify_bench.py: Splats.split / densify_and_cull / cull (rfstudio/graphics/_splats.py:87-175), GSplatter.update_grad_norm
(rfstudio/model/gsplat.py:360-374) and the Adam branch of ModuleOptimizers.mutate_params (rfstudio/optim/optimizer.py:155-185).
Runs on whatever device its tensors live on.  `P` is a dict means / scales / quats / colors / shs / opacities ([N,1]).
"""
import math
from typing import Dict, Optional, Tuple

import torch

FIELDS = ("means", "scales", "quats", "colors", "shs", "opacities")


def unit_quat_rotation(quats: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] rotation of the direction of the quaternion (w, x, y, z), any length: I - (2 / q.q) [...] on the raw components,
    row by row (normalising first is the same rotation with more roundings)"""
    w, x, y, z = quats.unbind(-1)
    h = 2 / (quats * quats).sum(-1)
    rows = [[1 - h * (y * y + z * z), h * (x * y - w * z), h * (x * z + w * y)],
            [h * (x * y + w * z), 1 - h * (x * x + z * z), h * (y * z - w * x)],
            [h * (x * z - w * y), h * (y * z + w * x), 1 - h * (x * x + y * y)]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def child_means(P: Dict[str, torch.Tensor], randn: torch.Tensor) -> torch.Tensor:
    """[S, n, 3]: every sample z of randn [S, n, 3] scaled by the Gaussian's extents in its own frame, turned into the world frame
    and added to its centre.  Evaluated in float64 and rounded once: the yardstick is the correctly rounded value (an fp32 rotation
    entry that cancels to ~0 keeps an absolute error no bound relative to the row's terms covers)."""
    local = randn.double() * P["scales"].double().exp()
    world = torch.einsum("nij,snj->sni", unit_quat_rotation(P["quats"].double()), local) + P["means"].double()
    return world.to(P["means"].dtype)


def split(P: Dict[str, torch.Tensor], randn: torch.Tensor, shrink: float = 1.6) -> Dict[str, torch.Tensor]:
    """The S * n children of the n Gaussians of P for the samples randn [S, n, 3], S-major (child s of every parent, then s + 1):
    sampled centres, extents divided by `shrink`, everything else the parent's."""
    S, n = randn.shape[0], randn.shape[1]
    out = {"means": child_means(P, randn).reshape(S * n, 3)}
    for name in FIELDS[1:]:
        parent = (P[name].exp() * (1 / shrink)).log() if name == "scales" else P[name]
        out[name] = parent.repeat(S, *([1] * (parent.dim() - 1)))
    return out


def classify(P, xys_grad_norm, vis_counts, half_extent, densify_grad_thresh, densify_size_thresh, cull_alpha_thresh, cull_scale_thresh):
    """(selected, splits, dups, culls) and the decision quantities (avg_grad_norm, scale_max, alpha)"""
    scale_max = P["scales"].exp().max(dim=-1).values
    avg = half_extent * (xys_grad_norm / vis_counts)
    high, big = avg > densify_grad_thresh, scale_max > densify_size_thresh
    splits, dups = high & big, high & (scale_max <= densify_size_thresh)
    alpha = P["opacities"].sigmoid()[..., 0]
    culls = alpha < cull_alpha_thresh
    if cull_scale_thresh is not None:
        culls = culls | (scale_max > cull_scale_thresh)
    return ~(culls | splits), splits, dups, culls, (avg, scale_max, alpha)


def densify_and_cull(P, xys_grad_norm, vis_counts, last_width, last_height, *, densify_grad_thresh, densify_size_thresh, num_splits,
                     cull_alpha_thresh, cull_scale_thresh, randn=None) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, torch.Tensor]:
    """-> (new P, indices i64[N'] with -1 for every new row, the randn used)"""
    half_extent = 0.5 * max(float(last_width), float(last_height))
    selected, splits, dups, _, _ = classify(P, xys_grad_norm, vis_counts, half_extent, densify_grad_thresh, densify_size_thresh,
                                            cull_alpha_thresh, cull_scale_thresh)
    src = {name: P[name][splits] for name in FIELDS}
    if randn is None:
        randn = torch.randn((num_splits, src["means"].shape[0], 3), device=P["means"].device)
    children = split(src, randn)
    new = {name: torch.cat([P[name][selected], children[name], P[name][dups]], dim=0) for name in FIELDS}
    kept = selected.nonzero()[:, 0]
    indices = torch.cat([kept, -kept.new_ones(new["means"].shape[0] - kept.shape[0])])
    return new, indices, randn


def cull(P, *, cull_alpha_thresh, cull_scale_thresh) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    culls = P["opacities"].sigmoid()[..., 0] < cull_alpha_thresh
    if cull_scale_thresh is not None:
        culls = culls | (P["scales"].exp().max(dim=-1).values > cull_scale_thresh)
    selected = ~culls
    return {name: P[name][selected] for name in FIELDS}, selected.nonzero()[:, 0]


def update_grad_norm(xys_grad_norm, vis_counts, gaussian_ids, v_means2d) -> None:
    vis_counts[gaussian_ids] += 1
    xys_grad_norm[gaussian_ids] += v_means2d.norm(dim=-1)


def mutate_moment(moment: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """one exp_avg / exp_avg_sq through mutate_params(indices=...)"""
    moved = moment[indices.clamp(min=0)]
    moved[indices < 0] = 0
    return moved


def mutate_adam(optimizer: torch.optim.Adam, new_params, indices: Optional[torch.Tensor] = None, clear: bool = False) -> None:
    group = optimizer.param_groups[0]
    if indices is not None:
        for param, new_param in zip(group["params"], new_params):
            if param not in optimizer.state:
                continue
            st = optimizer.state[param]
            for item in ("exp_avg", "exp_avg_sq"):
                if item in st:
                    st[item] = mutate_moment(st[item], indices)
            del optimizer.state[param]
            optimizer.state[new_param] = st
    if clear:
        for param in group["params"]:
            for item in ("exp_avg", "exp_avg_sq"):
                if item in optimizer.state.get(param, {}):
                    optimizer.state[param][item][...] = 0
    group["params"] = list(new_params)


# ---- seeded inputs shared by the full-size test and scripts/densify_bench.py
def seeded_inputs(n, dev, seed):
    """seeded set with the golden's class mix: splits, duplicates, opacity and size culls, culled rows that still densify"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=gen)
    smax = torch.exp(r(n) * (math.log(0.8) - math.log(0.002)) + math.log(0.002))
    scales = (smax[:, None] * (0.3 + 0.7 * r(n, 3))).log()
    scales[torch.arange(n, device=dev), torch.randint(0, 3, (n,), device=dev, generator=gen)] = smax.log()
    P = dict(means=r(n, 3) * 2 - 1, scales=scales, quats=torch.randn(n, 4, device=dev, generator=gen) * (0.5 + r(n, 1)),
             opacities=torch.randn(n, 1, device=dev, generator=gen) * 1.8 - 1.0, colors=r(n, 3),
             shs=torch.randn(n, 15, 3, device=dev, generator=gen) * 0.1)
    vis = torch.randint(1, 40, (n,), device=dev, generator=gen).float()
    avg = torch.where(r(n) < 0.55, 3e-4 + 2e-3 * r(n), 1e-5 + 1.4e-4 * r(n))
    return P, avg * vis / 400.0, vis


SEEDED_KW = dict(densify_grad_thresh=0.0002, densify_size_thresh=0.01, num_splits=2, cull_alpha_thresh=0.1, cull_scale_thresh=0.5)


def mask_near_thresholds(P, xys, vis, half_extent, kw):
    """Both decision paths run on the device here, so a row within 1e-4 (relative) of a threshold may be classified differently by
    the two (`exp` differs in the last bit).  Such rows are taken out of the comparison by turning them into plain culled rows
    (tiny opacity, mid size, no gradient) for BOTH paths.  Returns their fraction."""
    _, _, _, _, (avg, smax, alpha) = classify(P, xys, vis, half_extent, kw["densify_grad_thresh"], kw["densify_size_thresh"],
                                                  kw["cull_alpha_thresh"], kw["cull_scale_thresh"])
    near = torch.zeros_like(avg, dtype=torch.bool)
    for q, t in ((avg, kw["densify_grad_thresh"]), (smax, kw["densify_size_thresh"]), (smax, kw["cull_scale_thresh"]),
                 (alpha, kw["cull_alpha_thresh"])):
        near |= (q - t).abs() <= 1e-4 * t
    P["opacities"][near] = -10.0
    P["scales"][near] = math.log(0.05)
    xys[near] = 0.0
    return float(near.float().mean())
