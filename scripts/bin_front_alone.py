"""gs_isect_bin_front alone on the bench views (2 M Gaussians, 800 x 800, tight rectangles, capacity mode as the engine calls it):
time per call from HIP events, the segment-length classes of the tile-first path, and a checksum of the result that two builds of
the library must share.   GEOSPLAT_LIB=<path> python scripts/bin_front_alone.py [level=7] [reps=20] [views=0,3]
Under `rocprofv3 --kernel-trace --stats` the same run gives every binning kernel alone."""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geosplatting_amd._lib as L
if os.environ.get("GEOSPLAT_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["GEOSPLAT_LIB"])
import torch
import geosplatting_amd as gs, geosplatting_amd.synthetic as syn
from geosplatting_amd import front as F
from geosplatting_amd.engine import params_from_scene
from geosplatting_amd.shading import _MODE

dev = torch.device("cuda:0")
level = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
views = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 3]
scene = syn.sphere_scene(level, seed=1, cubemap_res=64, device=dev)
cams = syn.blender_cameras(num=8, width=800, height=800)
p = params_from_scene(scene, dev)
sc, op = p.scales.exp(), torch.sigmoid(p.opacities).squeeze(-1).contiguous()
d = lambda t: t.to(dev, torch.float32).contiguous()
lib = L.lib()
caps = []
if hasattr(lib, "gs_isect_bin_front_classes"):
    buf = (C.c_int * 8)()
    caps = [int(buf[i]) for i in range(lib.gs_isect_bin_front_classes(buf, 8))]


def geometry(c, base, bits, status):
    return F.front_stage(p.means, p.quats, sc, op, p.normals, p.kd, p.ks, d(c.view_matrix), d(c.intrinsic_matrix), d(c.c2w[:, 3]), None, 800, 800,
                         0.1, 1.0, _MODE["pbr"], base, bits, status, records=False, tight_tiles=True)


for i in views:
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    fr = geometry(cams[i], 0, 32, status)
    fr.event.synchronize()
    lo, hi = F.depth_range(fr.host_counts)
    bits, base = F.binning_keys(lo, hi)
    fr = geometry(cams[i], base, bits, status)
    fr.event.synchronize()
    V, I = int(fr.host_counts[0]), int(fr.host_counts[1])
    cap = ((int(I * 1.25) + 65535) // 65536) * 65536
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        state, _, _ = F.bin_stage(fr, cap, status, prepare=False)
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    flat, off = state["flatten_ids"][:I].long(), state["isect_offsets"].long()
    w = torch.arange(I, device=dev) % 1000003 + 1
    check = int((flat * w).sum()) ^ int((off * (torch.arange(off.numel(), device=dev) + 1)).sum())
    tc = fr.tile_counts.cpu().long()
    line = f"view {i}: V={V} I={I} cap={cap} key_bits={bits}  bin_front {times[len(times) // 2]:.1f} us (min {times[0]:.1f})  checksum {check:#x}  status {status.cpu().tolist()}"
    if caps:
        edges = [0] + caps + [1 << 31]
        line += "  classes " + " ".join(f"<={edges[k + 1] if k < len(caps) else 'inf'}: {int(((tc > edges[k]) & (tc <= edges[k + 1])).sum())} tiles / "
                                        f"{int(tc[(tc > edges[k]) & (tc <= edges[k + 1])].sum())} items" for k in range(len(edges) - 1))
    print(line)
