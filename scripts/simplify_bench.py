#!/usr/bin/env python3
"""Time mesh decimation and the component labelling (csrc/gs_simplify.hip through geosplatting_amd.meshsimplify), and measure what
the decimated mesh loses.

    python scripts/simplify_bench.py [--res 512] [--target 100352] [--points 1000000] [--runs 5] [--warmup 1] [--out FILE.json]

Input: the Poisson mesh of scripts/poisson_bench.py -- `points` oriented samples of its bumpy height field (224 x 224 x 2 triangles)
solved at `res`^3 (mesh_from_oriented_points) -- decimated to `target` faces, the size every benchmark of the prior flow uses.
  simplify          median (min, max) in ms of `runs` whole simplify_mesh calls after `warmup`, host time between two device waits
                    (the call reads counters back every round, so the host is part of it), with the rounds and the faces it ended at
  per_round         one further run with a device wait after each part of a round: mean ms per round of the topology rebuild (torch
                    sorts), the kernels (edge costs and selection; round 0 also sums the quadrics) and the application (winner sort,
                    apply kernel, face remap and compaction); and their totals
  components        mesh_components alone on the input mesh: median ms and the passes it took
  quality           chamfer_fscore (squared-distance threshold 1e-3 and 1e-5) of the decimated mesh against the input mesh, next to
                    remesh_poisson of the input at the resolution whose face count is nearest to the decimated one
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)


def host_timed(fn, runs, warmup, dev):
    out, last = [], None
    for k in range(warmup + runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize(dev)
        if k >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return {"ms": statistics.median(out), "ms_min_max": [min(out), max(out)]}, last


def quality(mesh, reference, seed):
    import geosplatting_amd as gs
    out = {}
    for name, thr in (("1e-3", 1e-3), ("1e-5", 1e-5)):
        gen = torch.Generator(device=mesh[0].device).manual_seed(seed)
        chamfer, fscore = gs.chamfer_fscore(mesh, reference, threshold=thr, generator=gen)
        out["chamfer"] = float(chamfer)
        out["fscore_" + name] = float(fscore)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--target", type=int, default=100352)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--smoothness", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench needs a GPU")
    import geosplatting_amd as gs
    from poisson_bench import height_field
    dev = torch.device("cuda:0")
    hv, hf = height_field(224, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pts, nrm = (t.contiguous() for t in gs.sample_mesh_surface(hv, hf, a.points, generator=gen))
    with torch.no_grad():
        v, f, _ = gs.mesh_from_oriented_points(pts, nrm, a.res, a.smoothness)
    v, f = v.detach().contiguous(), f.contiguous()
    result = {"resolution": a.res, "input_vertices": int(v.shape[0]), "input_faces": int(f.shape[0]), "target_faces": a.target}
    print(json.dumps(result), flush=True)

    timing, (v2, f2, _, info) = host_timed(lambda: gs.simplify_mesh(v, f, a.target, return_info=True), a.runs, a.warmup, dev)
    result["simplify"] = dict(timing, rounds=info["rounds"], stalled=info["stalled"], faces=int(f2.shape[0]), vertices=int(v2.shape[0]),
                              first_round=info["per_round"][0], last_round=info["per_round"][-1])
    parts = []
    gs.simplify_mesh(v, f, a.target, _timing=parts)
    totals = [sum(p[k] for p in parts) for k in range(3)]
    result["per_round"] = {"rounds": len(parts), "topology_ms": totals[0] / len(parts), "kernels_ms": totals[1] / len(parts),
                           "apply_ms": totals[2] / len(parts), "topology_total_ms": totals[0], "kernels_total_ms": totals[1],
                           "apply_total_ms": totals[2], "first_round_ms": list(parts[0])}
    timing, (_, _, cinfo) = host_timed(lambda: gs.mesh_components(f, v.shape[0]), a.runs, a.warmup, dev)
    result["components"] = dict(timing, iterations=cinfo["iterations"], labels=int(torch.unique(gs.mesh_components(f, v.shape[0])[0]).shape[0]))
    print(json.dumps(result), flush=True)

    # remesh_poisson at the resolution whose face count is nearest: faces grow with the square of the resolution
    guess = a.res * (f2.shape[0] / f.shape[0]) ** 0.5
    best = None
    for R in sorted({max(16, 8 * round(guess / 8) + d) for d in (-24, -16, -8, 0, 8, 16, 24)}):
        with torch.no_grad():
            rv, rf, _ = gs.remesh_poisson(v, f, R, a.smoothness)
        if best is None or abs(rf.shape[0] - f2.shape[0]) < abs(best[2].shape[0] - f2.shape[0]):
            best = (R, rv.detach().contiguous(), rf.contiguous())
    result["quality"] = {"simplify_mesh": dict(quality((v2, f2), (v, f), 1), faces=int(f2.shape[0])),
                         "remesh_poisson": dict(quality(best[1:], (v, f), 1), faces=int(best[2].shape[0]), resolution=best[0])}
    result["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
