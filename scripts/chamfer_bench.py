#!/usr/bin/env python3
"""Time the nearest-neighbour search and the Chamfer / F-score metric (csrc/gs_nn.hip through geosplatting_amd.geometry).

    python scripts/chamfer_bench.py [--points 1000000] [--runs 5] [--warmup 1] [--subset 16384] [--out FILE.json]

The evaluation shape of the reference (tests/loss/test_chamfer_distance.py: 1 000 000 samples per mesh): syn.icosphere(6, 0.8) against
syn.bumpy_sphere(6), both sampled with samples_per_face='uniform'.  `runs` windows after `warmup`, each between two device events;
median (min, max) in ms:
  sample         sample_mesh_surface of one mesh
  build          PointGrid.rebuild (every launch of gs_nn_build, radix passes included)
  query          PointGrid.nearest of all samples of the other mesh, in the sampler's order (face by face) and in a random order
  chamfer_pair   chamfer_distance: two builds and two queries
  chamfer_fscore the whole metric from the two meshes: sampling, the pair, the means
Two yardsticks on the same device, timed on the first `subset` queries against the whole set and scaled to all queries (they are
linear in the number of queries, and at full size one call runs for minutes):
  brute_force    the null-grid form of gs_nn_query (LDS tiles, the same distance routine); its results are asserted equal
  torch_cdist    torch.cdist in chunks of 1 024 queries and a min over each chunk's row
The degrading case: the same `subset` queries moved 10 box extents along x, wholly outside the other set's box, grid against brute force.
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


def cdist_nearest(q, p, chunk=1024):
    d = torch.empty(q.shape[0], device=q.device)
    i = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for lo in range(0, q.shape[0], chunk):
        d[lo:lo + chunk], i[lo:lo + chunk] = torch.cdist(q[lo:lo + chunk], p).min(dim=1)
    return d, i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--subset", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_bench needs a GPU")
    import geosplatting_amd as gs
    from geosplatting_amd import synthetic as syn
    dev = torch.device("cuda:0")
    S, sub = a.points, min(a.subset, a.points)
    stat = lambda t, scale=1.0: {"ms": t[0] * scale, "ms_min_max": [t[1] * scale, t[2] * scale]}
    va, fa = (t.to(dev) for t in syn.icosphere(6, 0.8))
    vb, fb = (t.to(dev) for t in syn.bumpy_sphere(6)[:2])
    gen = torch.Generator(device=dev).manual_seed(0)
    sample = lambda v, f: gs.sample_mesh_surface(v, f, S, samples_per_face="uniform", generator=gen)[0]
    pa, pb = sample(va, fa).contiguous(), sample(vb, fb).contiguous()
    grid = gs.PointGrid(pb)
    shuffled = pa[torch.randperm(S, device=dev, generator=gen)].contiguous()
    r = {"points": S, "faces": [int(fa.shape[0]), int(fb.shape[0])], "subset": sub,
         "sample": stat(timed(lambda: sample(va, fa), a.runs, a.warmup)),
         "build": stat(timed(lambda: grid.rebuild(pb), a.runs, a.warmup)),
         "query": stat(timed(lambda: grid.nearest(pa), a.runs, a.warmup)),
         "query_shuffled": stat(timed(lambda: grid.nearest(shuffled), a.runs, a.warmup)),
         "query_k4": stat(timed(lambda: grid.k_nearest(pa, 4), a.runs, a.warmup)),
         "chamfer_pair": stat(timed(lambda: gs.chamfer_distance(pa, pb), a.runs, a.warmup)),
         "chamfer_fscore": stat(timed(lambda: gs.chamfer_fscore((va, fa), (vb, fb), target_num_points=S, generator=gen), a.runs, a.warmup))}
    ch, fs = gs.chamfer_fscore((va, fa), (vb, fb), target_num_points=S, generator=gen)
    r["chamfer"], r["fscore"] = float(ch), float(fs)
    print("grid", json.dumps(r), flush=True)

    qs = pa[:: max(1, S // sub)][:sub].contiguous()
    scale = S / qs.shape[0]
    d, i = grid.nearest(qs)
    db, ib = grid.nearest(qs, brute_force=True)
    assert torch.equal(d.view(torch.int32), db.view(torch.int32)) and torch.equal(i, ib)
    dc, ic = cdist_nearest(qs, pb)
    r["yardsticks"] = {"queries": int(qs.shape[0]), "scaled_by": scale,
                       "grid_subset": stat(timed(lambda: grid.nearest(qs), a.runs, a.warmup)),
                       "brute_force": stat(timed(lambda: grid.nearest(qs, brute_force=True), a.runs, a.warmup), scale),
                       "torch_cdist": stat(timed(lambda: cdist_nearest(qs, pb), a.runs, a.warmup), scale),
                       "cdist_index_disagreements": int((ic.int() != i).sum()),
                       "cdist_max_abs_diff_of_d": float((dc * dc - d).abs().max())}
    print("yardsticks", json.dumps(r["yardsticks"]), flush=True)

    ext = pb.max(0).values - pb.min(0).values
    far = (qs + torch.tensor([10.0, 0.0, 0.0], device=dev) * ext).contiguous()
    d, i = grid.nearest(far)
    db, ib = grid.nearest(far, brute_force=True)
    assert torch.equal(d.view(torch.int32), db.view(torch.int32)) and torch.equal(i, ib)
    r["far"] = {"queries": int(far.shape[0]),
                "grid": stat(timed(lambda: grid.nearest(far), a.runs, a.warmup)),
                "brute_force": stat(timed(lambda: grid.nearest(far, brute_force=True), a.runs, a.warmup))}
    print("far", json.dumps(r["far"]), flush=True)
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
