#!/usr/bin/env python3
"""Time GaussianSet.densify_and_cull (parameters AND the twelve Adam moment tensors, csrc/gs_densify.hip) against the plain-torch
form of the same refinement (tests/densify_ref.py: masks, nonzero, gathers, cats, then the moments through mutate_params' indexing)
on the same device, in the same process, alternating the two.

    python scripts/densify_bench.py [--n 2000000] [--runs 20] [--warmup 3] [--out FILE.json]

2 M Gaussians of SH degree 3 with the class mix of tests/test_gpu_densify.py::test_full_size_against_densify_ref.  Device events
around each call (both forms end in their own read-back of the counts, which is inside the window), median over --runs.  The
effective bandwidth is (rows read + rows written) x 708 B / time: 59 parameter + 118 moment floats per Gaussian, each source row
counted once and each output row once.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import geosplatting_amd as gs                                              # noqa: E402
from tests import densify_ref as ref                                       # noqa: E402

ROW_BYTES = 708
COPY_TBPS = 6.29                                                           # the project's measured device copy figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_bench needs a GPU")
    dev = torch.device("cuda:0")
    P, xys, vis = ref.seeded_inputs(a.n, dev, seed=31)
    ref.mask_near_thresholds(P, xys, vis, 400.0, ref.SEEDED_KW)
    gen = torch.Generator(device=dev).manual_seed(32)
    moments = {k: (torch.randn(P[k].shape, device=dev, generator=gen), torch.rand(P[k].shape, device=dev, generator=gen)) for k in ref.FIELDS}
    n_split = int(ref.classify(P, xys, vis, 400.0, ref.SEEDED_KW["densify_grad_thresh"], ref.SEEDED_KW["densify_size_thresh"],
                               ref.SEEDED_KW["cull_alpha_thresh"], ref.SEEDED_KW["cull_scale_thresh"])[1].sum())
    randn = torch.randn(ref.SEEDED_KW["num_splits"], n_split, 3, device=dev, generator=gen)

    def run_hip():
        g = gs.GaussianSet(**P)
        g.xys_grad_norm, g.vis_counts, g.last_width, g.last_height = xys, vis, 800, 600
        opts = {}
        for k in ref.FIELDS:
            p = getattr(g, k)
            opts[k] = torch.optim.Adam([p], lr=1e-3)
            opts[k].state[p] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0], "exp_avg_sq": moments[k][1]}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.densify_and_cull(randn=randn, optimizers=opts, **ref.SEEDED_KW)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), g.last_totals

    def run_ref():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        new, idx, _ = ref.densify_and_cull(P, xys, vis, 800, 600, randn=randn, **ref.SEEDED_KW)
        moved = [ref.mutate_moment(m, idx) for k in ref.FIELDS for m in moments[k]]
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (new["means"].shape[0], len(moved))

    for _ in range(a.warmup):
        run_hip(), run_ref()
    t_hip, t_ref = [], []
    for _ in range(a.runs):                                                # alternate the two forms
        ms, totals = run_hip()
        t_hip.append(ms)
        t_ref.append(run_ref()[0])
    m_hip, m_ref = statistics.median(t_hip), statistics.median(t_ref)
    rows = a.n + totals[3]
    tbps = rows * ROW_BYTES / (m_hip * 1e-3) / 1e12
    res = dict(n=a.n, n_out=totals[3], n_selected=totals[0], n_split=totals[1], n_dup=totals[2], runs=a.runs,
               hip_ms_median=m_hip, hip_ms_min=min(t_hip), hip_ms_max=max(t_hip), ref_ms_median=m_ref, ref_ms_min=min(t_ref),
               ref_ms_max=max(t_ref), ref_over_hip=m_ref / m_hip, effective_tbps=tbps, copy_tbps=COPY_TBPS,
               fraction_of_copy=tbps / COPY_TBPS, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if m_hip > m_ref:
        raise SystemExit(f"the HIP path ({m_hip:.3f} ms) is slower than densify_ref ({m_ref:.3f} ms)")


if __name__ == "__main__":
    main()
