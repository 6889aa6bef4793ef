#!/usr/bin/env python3
"""Time the fused mesh-prior regularisers (csrc/gs_meshreg.hip through geosplatting_amd.meshreg) and one stage-2 `PriorModel` step.

    python scripts/meshreg_bench.py [--cells 224] [--runs 5] [--warmup 2] [--image 800] [--no-step] [--out FILE.json]

The mesh is a bumpy height field of cells x cells x 2 triangles (224: 100 352 faces).  Each figure is the median (min, max) in ms of
`runs` windows after `warmup`, each between two device events, of forward + backward of
lap * 1e-3 + nc * 3e-4 + edge * 0.1 with respect to the vertices:
  fused          mesh_regularizers on a MeshRegTopology built once (the topology build is timed on its own: topology_build)
  torch_rebuilt  the reference's shape in torch ops on the same device: the uniform Laplacian rebuilt from a `unique` over the 2 * 3F
                 index pairs into a coalesced sparse matrix, and the edges / face pairs rebuilt from a sort + unique of the 3F sides,
                 in every step (rfstudio/model/geosplat_prior.py:32-60, :123-136; pytorch3d's Meshes does the second)
  torch_hoisted  the same arithmetic with all of that built once
The fused result is checked against the same composition in float64 (1e-5 of the loss, 1e-4 of the largest gradient element; the
torch composition's errors are reported next to it).  `prior_step`: one `stage2.train_step` of a `PriorModel` on that mesh, one image x image
view, num_samples_per_ray 8 (hierarchy rebuild, field, Monte-Carlo shading, denoiser, splatting, loss, regularisers, backward).
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


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


def height_field(cells, dev):
    n = cells + 1
    ys, xs = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    x, y = xs.reshape(-1).float() / cells * 1.6 - 0.8, ys.reshape(-1).float() / cells * 1.6 - 0.8
    v = torch.stack((x, 0.15 * torch.sin(7 * x) * torch.cos(5 * y), y), 1).contiguous()
    i = (ys[:-1, :-1] * n + xs[:-1, :-1]).reshape(-1)
    f = torch.cat((torch.stack((i, i + n, i + 1), 1), torch.stack((i + 1, i + n, i + n + 1), 1)), 0)
    return v, f.long().contiguous()


def torch_topology(f, V):
    """what the reference rebuilds per step: the Laplacian (unique over the directed pairs, coalesce) and the edges with the pairs of
    faces on them (sort + unique of the sides; consecutive equal sides are a pair on this manifold mesh)"""
    ii, jj = f[:, [1, 2, 0]].flatten(), f[:, [2, 0, 1]].flatten()
    adj = torch.stack([torch.cat([ii, jj]), torch.cat([jj, ii])], dim=0).unique(dim=1)
    ones = torch.ones(adj.shape[1], device=f.device)
    idx = torch.cat((adj, torch.stack((adj[0], adj[0]), dim=0)), dim=1)
    L = torch.sparse_coo_tensor(idx, torch.cat((-ones, ones)), (V, V)).coalesce()
    a, b, opp = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    key, order = torch.sort(lo * V + hi)
    ukey = torch.unique_consecutive(key)
    edges = torch.stack((ukey // V, ukey % V), 1)
    same = key[1:] == key[:-1]
    first = torch.nonzero(same).reshape(-1)
    pairs = torch.stack((key[first] // V, key[first] % V, opp[order][first], opp[order][first + 1]), 1)
    return L, edges, pairs


def torch_loss(v, topo):
    L, edges, pairs = topo
    lap = L.mm(v).norm(dim=1).mean()
    edge = (v[edges[:, 0]] - v[edges[:, 1]]).norm(dim=1).square().mean()
    v0, v1, a, b = (v[pairs[:, k]] for k in range(4))
    n0, n1 = torch.cross(v1 - v0, a - v0, dim=1), torch.cross(v1 - v0, b - v0, dim=1)
    nc = (1 - torch.cosine_similarity(n0, -n1, dim=1)).mean()
    return lap * 1e-3 + nc * 3e-4 + edge * 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshreg_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import stage2
    from geosplatting_amd import synthetic as syn
    dev = torch.device("cuda:0")
    stat = lambda t: {"ms": t[0], "ms_min_max": [t[1], t[2]]}
    v0, f = height_field(a.cells, dev)
    V = v0.shape[0]
    topo = gs.MeshRegTopology(f, V)
    r = {"faces": int(f.shape[0]), "vertices": V, "edges": topo.num_edges, "pairs": topo.num_pairs}

    def fused():
        v = v0.clone().requires_grad_(True)
        lap, edge, nc = gs.mesh_regularizers(v, topo)
        loss = lap * 1e-3 + nc * 3e-4 + edge * 0.1
        loss.backward()
        return loss.detach(), v.grad

    hoisted_topo = torch_topology(f, V)

    def in_torch(rebuild):
        v = v0.clone().requires_grad_(True)
        with torch.no_grad():
            t = torch_topology(f, V) if rebuild else hoisted_topo
        loss = torch_loss(v, t)
        loss.backward()
        return loss.detach(), v.grad

    # both against the same composition in float64: 1e-4 of the largest gradient element (the nc gradient is a difference of two
    # nearly equal parts on a smooth mesh, so two float32 evaluations differ by more than their last bits)
    v64 = v0.double().requires_grad_(True)
    l64 = torch_loss(v64, (hoisted_topo[0].double(), hoisted_topo[1], hoisted_topo[2]))
    l64.backward()
    r["loss"] = float(l64)
    for name, (l, g) in (("fused", fused()), ("torch_rebuilt", in_torch(True))):
        err_l, err_g = abs(float(l) - float(l64)) / abs(float(l64)), float((g.double() - v64.grad).abs().max() / v64.grad.abs().max())
        r[name + "_error"] = {"loss_rel": err_l, "grad_rel_to_max": err_g}
        assert name != "fused" or (err_l <= 1e-5 and err_g <= 1e-4), (name, err_l, err_g)
    r["topology_build"] = stat(timed(lambda: gs.MeshRegTopology(f, V), a.runs, a.warmup))
    r["fused"] = stat(timed(fused, a.runs, a.warmup))
    r["torch_rebuilt"] = stat(timed(lambda: in_torch(True), a.runs, a.warmup))
    r["torch_hoisted"] = stat(timed(lambda: in_torch(False), a.runs, a.warmup))
    print("regularisers", json.dumps(r), flush=True)

    if not a.no_step:
        cams = syn.blender_cameras(1, a.image, a.image)
        model = gs.PriorModel(v0, f, log2_hashmap_size=18)
        sched = gs.Stage2Schedule.prior()
        sched.setup(model)
        sched.before_update(model, 0)
        with torch.no_grad():
            gts = [img.clamp(0, 1) for img in model.render_report(cams, rnd_seed=1)[0]]
        r["prior_step"] = dict(stat(timed(lambda: stage2.train_step(model, cams, gts, gt_is_srgb=False), a.runs, a.warmup)),
                               image=a.image, gaussians=model.last_num_gaussians, views=1, num_samples_per_ray=model.num_samples_per_ray)
        print("prior_step", json.dumps(r["prior_step"]), flush=True)
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
