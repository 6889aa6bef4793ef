#!/usr/bin/env python3
"""Time the mesh rasterizer and its antialias pass (csrc/gs_meshraster.hip, csrc/gs_meshaa.hip through geosplatting_amd.meshrender) at
800 x 800 on the meshes this project extracts, and count the rasterizer's atomics.

    python scripts/mesh_render_bench.py [--meshes flexicubes96,tsdf512,ico3,ico5,ico7,plane] [--size 800] [--runs 20] [--warmup 3]
                                        [--lib PATH/libgeosplat_hip.so] [--out FILE.json] [--near-clip]

--near-clip adds a section: `rasterize_raw` (forward + resolve) on flexicubes96 with near_clip=False and True in the same process,
median of 5, cull='none', for the object-centred view (no face crosses the near plane) and for an eye 2 mm inside the wall looking
along it, with the number of crossing faces.  `--meshes ""` runs that section alone.

Meshes
  flexicubes96  the stage-1 FlexiCubes mesh at 96^3 (Stage1Model with a sphere SDF of radius 0.8)
  tsdf512       marching cubes of an analytic sphere TSDF (radius 0.6) in a 512^3 volume over +-1, about 1e6 faces of 1-3 px
  icoL          syn.icosphere(L, 0.6): 20 * 4^L faces; ico3 has triangles of about 40 px (the wave-per-triangle path), ico5 about 10 px
                (the thread path's largest boxes), ico7 about 2.5 px
  plane         two triangles that fill the image: the wave path alone
Every mesh is seen by the first syn.blender_cameras view (focal 1111 px, distance 2.67), cull='back'.

Per mesh, device events around `runs` calls after `warmup`, the median per call:
  fwd_ms      gs_meshraster_fwd: key fill, thread-per-triangle pass, wave-per-triangle pass
  resolve_ms  gs_meshraster_resolve
  bwd_ms      gs_meshraster_bwd with a random d rast (includes zeroing d vc)
  topology_ms gs_mesh_topology_build: table fill and insertion of the 3 F half-edges (once per face array, not per view)
  aa_fwd_ms   gs_meshaa_fwd on a 5-channel image (what render_mesh(antialias=True) passes: depth, normal, alpha)
  aa_bwd_ms   gs_meshaa_bwd with a random d out (includes zeroing d vc); aa_pairs counts the blended pairs of the view
  render_fwd_ms / render_bwd_ms   render_mesh(depth, normal, alpha, face) and the backward of sum(depth) + sum(normal): what a user
              calls, with the torch plumbing (view transform, vertex normals, normalisation) included
Counts come from ONE extra forward with the statistics buffer, outside the timed calls: fragments (covered pixel, triangle) and 64-bit
min atomics issued after the plain-load early-z, for the thread pass and the wave pass.  `atomics_per_us` divides the atomics of a
view by fwd_ms: a whole-forward figure (fill and triangle set-up included), not the rate of the atomic unit.  Nothing is compared
with a reference time: the reference's rasterizer is not in its tree.  `--lib` loads another build of the library, e.g. one compiled
with -DMR_SMALL_BOX=8, for the threshold experiment.  Needs a GPU; there is no CPU path.
"""
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


def build_mesh(name, gs, syn, dev):
    if name == "flexicubes96":
        from geosplatting_amd.stage1 import Stage1Model
        grid = gs.FlexiCubes.from_resolution(96, device=dev, random_sdf=False, scale=1.05)
        sdf = grid.vertices.norm(dim=-1) - 0.8
        model = Stage1Model(96, light_resolution=16, device=dev, sdf_init=sdf)
        with torch.no_grad():
            (v, f), _ = model.get_geometry()
        return v.contiguous(), f.contiguous()
    if name == "tsdf512":
        vol = gs.TSDFVolume(512, device=dev)
        R0, R1, R2 = vol.resolution
        ax = [vol.origin[k] + (torch.arange(r, device=dev, dtype=torch.float32) + 0.5) * vol.voxel_size for k, r in enumerate((R0, R1, R2))]
        for i2 in range(R2):                                              # a slab at a time: no second 512^3 temporary
            d = (ax[0][None, :] ** 2 + ax[1][:, None] ** 2 + ax[2][i2] ** 2).sqrt() - 0.6
            vol.volume[i2, :, :, 0] = (d / vol.sdf_trunc).clamp(-1.0, 1.0)
        vol.volume[..., 1] = 1.0
        v, f = vol.extract_mesh()
        del vol
        return v, f
    if name.startswith("ico"):
        v, f = syn.icosphere(int(name[3:]), 0.6)
        return v.to(dev), f.to(dev)
    if name == "plane":
        v = torch.tensor([[-3.0, -3.0, 0.0], [3.0, -3.0, 0.0], [3.0, 3.0, 0.0], [-3.0, 3.0, 0.0]], device=dev)
        return v, torch.tensor([[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 3, 2]], device=dev)      # both windings: one pair survives culling
    raise SystemExit(f"unknown mesh {name}")


def near_clip_section(gs, mr, syn, dev, size, runs=5, warmup=3):
    """rasterize_raw (forward + resolve) on the flexicubes96 mesh with near_clip False and True, alternating in one process, for the
    object-centred view (no crossing face: both take the same code) and for an eye 2 mm inside the wall looking along it"""
    v, f = build_mesh("flexicubes96", gs, syn, dev)
    f32 = f.to(torch.int32).contiguous()
    outside = syn.blender_cameras(8, size, size)[0].to(dev)
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.798], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]], device=dev)
    inside = gs.Camera(c2w, outside.fx, outside.fy, outside.cx, outside.cy, size, size)
    out = {"faces": int(f32.shape[0]), "image": size, "runs": runs}
    for label, cam in (("object_centred", outside), ("inside", inside)):
        intr = (cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width)
        with torch.no_grad():
            vc = mr.to_camera_space(v, cam).contiguous()
        z = vc[f32.long()][..., 2]
        n_in = (z > 1e-2).sum(-1)
        row = {"crossing_faces": int(((n_in > 0) & (n_in < 3) & torch.isfinite(vc[f32.long()]).all(-1).all(-1)).sum())}
        for clip in (False, True):
            kept = {}

            def call():
                kept["rast"] = mr.rasterize_raw(vc, f32, intr, cull="none", near=1e-2, near_clip=clip)

            t = timed(call, runs, warmup)
            row["near_clip" if clip else "plain"] = {"ms": t[0], "min_max": t[1:], "covered_pixels": int((kept["rast"][..., 3] > 0).sum())}
        out[label] = row
        print("near_clip", label, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--near-clip", action="store_true", help="also time near_clip=False against True (flexicubes96, median of 5)")
    ap.add_argument("--meshes", default="flexicubes96,tsdf512,ico3,ico5,ico7,plane")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_bench needs a GPU")
    from geosplatting_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import geosplatting_amd as gs
    from geosplatting_amd import meshrender as mr
    from geosplatting_amd import synthetic as syn
    dev = torch.device("cuda:0")
    cam = syn.blender_cameras(8, a.size, a.size)[0].to(dev)
    lib = _lib.lib()
    results = {"image": a.size, "lib": a.lib or "default", "meshes": {}}
    for name in [m for m in a.meshes.split(",") if m]:
        v, f = build_mesh(name, gs, syn, dev)
        f32 = f.to(torch.int32).contiguous()
        intr = (cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width)
        with torch.no_grad():
            vc = mr.to_camera_space(v, cam).contiguous()
        H, W = cam.height, cam.width
        ws_bytes = lib.gs_meshraster_ws_bytes(f32.shape[0], H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        rast = torch.empty(H, W, 4, device=dev)
        head = (vc.shape[0], f32.shape[0], _lib.ptr(vc), _lib.ptr(f32), *intr, 1e-2)

        def fwd(stats=None):
            _lib.check(lib.gs_meshraster_fwd(*head, 1, _lib.ptr(ws), ws_bytes, _lib.ptr(stats), _lib.stream()), "gs_meshraster_fwd")

        def resolve():
            _lib.check(lib.gs_meshraster_resolve(*head, _lib.ptr(ws), ws_bytes, _lib.ptr(rast), _lib.stream()), "gs_meshraster_resolve")

        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        fwd(stats)
        resolve()
        counts = stats.tolist()
        covered = int((rast[..., 3] > 0).sum())
        d_rast = torch.randn(H, W, 4, device=dev)
        d_vc = torch.empty_like(vc)

        def bwd():
            _lib.check(lib.gs_meshraster_bwd(*head, _lib.ptr(rast), _lib.ptr(d_rast), _lib.ptr(d_vc), _lib.stream()), "gs_meshraster_bwd")

        t_fwd, t_res, t_bwd = timed(fwd, a.runs, a.warmup), timed(resolve, a.runs, a.warmup), timed(bwd, a.runs, a.warmup)
        topo_bytes = lib.gs_mesh_topology_bytes(f32.shape[0])
        topo = torch.empty(topo_bytes, dtype=torch.uint8, device=dev)
        C = 5
        color, d_out = torch.rand(H, W, C, device=dev), torch.randn(H, W, C, device=dev)
        aa_out, d_color = torch.empty_like(color), torch.empty_like(color)
        dbg = torch.empty(H, W, 2, dtype=torch.int32, device=dev)
        aa_head = (*head, 1, _lib.ptr(topo), topo_bytes, C, _lib.ptr(rast), _lib.ptr(color))

        def topology():
            _lib.check(lib.gs_mesh_topology_build(f32.shape[0], _lib.ptr(f32), _lib.ptr(topo), topo_bytes, _lib.stream()),
                       "gs_mesh_topology_build")

        def aa_fwd(debug=None):
            _lib.check(lib.gs_meshaa_fwd(*aa_head, _lib.ptr(aa_out), _lib.ptr(debug), _lib.stream()), "gs_meshaa_fwd")

        def aa_bwd():
            _lib.check(lib.gs_meshaa_bwd(*aa_head, _lib.ptr(d_out), _lib.ptr(d_color), _lib.ptr(d_vc), _lib.stream()), "gs_meshaa_bwd")

        t_topo = timed(topology, a.runs, a.warmup)
        aa_fwd(dbg)
        aa_pairs = int((dbg > 0).sum())
        t_aaf, t_aab = timed(aa_fwd, a.runs, a.warmup), timed(aa_bwd, a.runs, a.warmup)
        vg = v.detach().clone().requires_grad_()
        kept = {}

        def render_fwd():
            kept["maps"] = gs.render_mesh(vg, f, cam)

        def render_bwd():
            maps = gs.render_mesh(vg, f, cam)
            vg.grad = None
            (maps["depth"].sum() + maps["normal"].sum()).backward()

        t_rf = timed(render_fwd, a.runs, a.warmup)
        t_rfb = timed(render_bwd, a.runs, a.warmup)
        atomics = counts[1] + counts[3]
        results["meshes"][name] = {
            "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "covered_pixels": covered,
            "fragments_thread_pass": counts[0], "atomics_thread_pass": counts[1],
            "fragments_wave_pass": counts[2], "atomics_wave_pass": counts[3],
            "atomics_per_view": atomics, "atomics_per_fragment": atomics / max(1, counts[0] + counts[2]),
            "fwd_ms": t_fwd[0], "fwd_ms_min_max": t_fwd[1:], "resolve_ms": t_res[0], "resolve_ms_min_max": t_res[1:],
            "bwd_ms": t_bwd[0], "bwd_ms_min_max": t_bwd[1:], "bwd_float_atomics": 9 * covered,
            "atomics_per_us": atomics / (t_fwd[0] * 1e3),
            "topology_ms": t_topo[0], "topology_ms_min_max": t_topo[1:], "topology_bytes": int(topo_bytes),
            "aa_fwd_ms": t_aaf[0], "aa_fwd_ms_min_max": t_aaf[1:], "aa_bwd_ms": t_aab[0], "aa_bwd_ms_min_max": t_aab[1:],
            "aa_pairs": aa_pairs, "aa_bwd_float_atomics": 6 * aa_pairs,
            "render_fwd_ms": t_rf[0], "render_fwd_plus_bwd_ms": t_rfb[0], "render_bwd_ms": t_rfb[0] - t_rf[0],
        }
        print(name, json.dumps(results["meshes"][name]), flush=True)
        del v, f, f32, vc, ws, rast, d_rast, d_vc, vg, kept, topo, color, d_out, aa_out, d_color, dbg
        torch.cuda.empty_cache()
    if a.near_clip:
        results["near_clip"] = near_clip_section(gs, mr, syn, dev, a.size)
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
