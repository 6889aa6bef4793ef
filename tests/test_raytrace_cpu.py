"""No-GPU checks of the ray queries: the float64 reference (tests/raytrace_ref.py) against hand-computed single-triangle cases, the
fragile cap as a condition on every scene the GPU tests use, argument validation of the C-ABI before the device is touched, and the
refusals of the Python ops.

Fragile shares of the reference alone (rays a float64 evaluation cannot decide for an fp32 kernel, see raytrace_ref), measured with
this file on the committed scenes; the cap is 1 %:
    3 732 rays per mesh: ico2 0.054 %, ico3 0.054 %, grid 0.456 %, bad 0.027 %, and 0 for tri1, tri2, tri3, ico1, dup64 and fan
    shadow scene (640 MGAdapter Gaussians of the bumpy icosphere(2), 8 directions): 0.000 % at offset 1e-5, 0.039 % at 1e-3
(the flat grid's share comes from the axis-parallel rays that start on a grid line and run along a shared edge of every cell they
cross)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import raytrace_ref as ref

FRAGILE_CAP = 0.01


def _one(v, f, o, d, **kw):
    r = ref.trace(np.asarray(v, np.float32), np.asarray(f), np.asarray([o], np.float32), np.asarray([d], np.float32), **kw)
    return {k: x[0] for k, x in r.items()}


UNIT = ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def test_reference_single_triangle_by_hand():
    r = _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1])
    assert r["occluded"] and r["face"] == 0 and r["t"] == 1.0 and np.allclose(r["bary"], [0.5, 0.25, 0.25], atol=1e-15) and not r["fragile"]
    r = _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -4])                                   # t is in units of |d|
    assert r["t"] == 0.25 and r["face"] == 0
    r = _one(*UNIT, [0.5, 0.125, -2.0], [0, 0, 1])                                   # from behind: both sides are tested
    assert r["occluded"] and r["t"] == 2.0 and np.allclose(r["bary"], [0.375, 0.5, 0.125], atol=1e-15)
    r = _one(*UNIT, [0.8, 0.8, 1.0], [0, 0, -1])                                     # outside
    assert not r["occluded"] and r["face"] == -1 and np.isinf(r["t"]) and not r["bary"].any() and not r["fragile"]
    r = _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, 1])                                    # pointing away: t = -1
    assert not r["occluded"] and not r["fragile"]
    r = _one(*UNIT, [1.0, 1.0, 1.0], [-0.75, -0.75, -1.0])                           # oblique, through (0.25, 0.25, 0)
    assert r["t"] == 1.0 and np.allclose(r["bary"], [0.5, 0.25, 0.25], atol=1e-15)


def test_reference_interval_is_strict_and_fragile_at_its_ends():
    assert not _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1], tmax=1.0)["occluded"]      # t == tmax: out
    assert not _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1], tmin=1.0)["occluded"]      # t == tmin: out
    assert _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1], tmax=1.0)["fragile"]
    assert _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1], tmin=0.5, tmax=1.5)["occluded"]
    assert not _one(*UNIT, [0.25, 0.25, 1.0], [0, 0, -1], tmin=0.5, tmax=1.5)["fragile"]


def test_reference_edges_vertices_and_bad_input():
    r = _one(*UNIT, [0.5, 0.0, 1.0], [0, 0, -1])                                     # on an edge: a hit in float64, and fragile
    assert r["occluded"] and r["fragile"]
    assert _one(*UNIT, [0.0, 0.0, 1.0], [0, 0, -1])["fragile"]                       # through a vertex
    assert not _one(*UNIT, [0.5, -1e-3, 1.0], [0, 0, -1])["fragile"]                 # clearly outside
    assert not _one(*UNIT, [0.5, 1e-3, 1.0], [0, 0, -1])["fragile"]                  # clearly inside
    for o, d in (([np.nan, 0.25, 1.0], [0, 0, -1]), ([0.25, 0.25, 1.0], [0, 0, 0]), ([0.25, 0.25, 1.0], [0, np.inf, -1])):
        r = _one(*UNIT, o, d)
        assert not r["occluded"] and r["face"] == -1 and not r["fragile"]
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]]
    r = _one(v, [[0, 1, 1], [3, 1, 2], [0, 1, 2]], [0.25, 0.25, 1.0], [0, 0, -1])    # zero area and NaN faces are never hit
    assert r["face"] == 2 and not r["fragile"]
    r = _one(*UNIT, [0.25, -1.0, 0.0], [0, 1, 0])                                    # in the triangle's plane: det == 0, a miss
    assert not r["occluded"]


def test_reference_closest_and_ties():
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 0, -1], [0, 1, -1]]
    r = _one(v, [[3, 4, 5], [0, 1, 2]], [0.25, 0.25, 1.0], [0, 0, -1])
    assert r["face"] == 1 and r["t"] == 1.0 and not r["fragile"]
    r = _one(v, [[3, 4, 5], [0, 1, 2]], [0.25, 0.25, 1.0], [0, 0, -1], tmin=1.5)      # the nearest hit cut off, not the second
    assert r["face"] == 0 and r["t"] == 2.0
    r = _one(v, [[0, 1, 2], [0, 1, 2], [0, 1, 2]], [0.25, 0.25, 1.0], [0, 0, -1])      # identical faces: the lowest index, not fragile
    assert r["face"] == 0 and not r["fragile"]
    v2 = v[:3] + [[0, 0, 1e-9], [1, 0, 1e-9], [0, 1, 1e-9]]
    assert _one(v2, [[0, 1, 2], [3, 4, 5]], [0.25, 0.25, 1.0], [0, 0, -1])["fragile"]  # two different faces closer than eps_t


def test_expand_forms():
    o = np.zeros((4, 3), np.float32)
    assert ref.expand(o, np.ones((4, 5, 3), np.float32))[2] == 5
    assert ref.expand(o, np.ones((7, 3), np.float32))[0].shape == (28, 3)
    assert ref.expand(o, np.ones((4, 3), np.float32))[2] == 1


@pytest.mark.parametrize("name", ref.MESH_NAMES)
def test_fragile_cap_of_every_scene(name):
    """The condition under which the GPU comparison means something, from the reference alone: at most 1 % of the rays are fragile,
    and the scene does what it is for (most rays hit; the S values and P = 1 occur)."""
    share = ref.fragile_share(name)
    e = ref.expected(name)
    hits = sum(int(x["occluded"].sum()) for x in e) / sum(x["occluded"].size for x in e)
    print(f"{name}: fragile {100 * share:.3f} %, rays {sum(x['fragile'].size for x in e)}, hit share {hits:.2f}")
    assert share <= FRAGILE_CAP
    assert hits > (0.5 if name.startswith("ico") else 0.02)
    S = {ref.expand(b["origins"], b["dirs"])[2] for b in ref.ray_batches(name)}
    assert {1, 3, 64, 65, 130} <= S and any(b["origins"].shape[0] == 1 for b in ref.ray_batches(name))
    if name.startswith("ico"):
        cut, full = e[1], e[0]                                                        # tmin = 1 cuts the nearest hit, not the second
        n = cut["t"].size
        assert ((cut["face"] != full["face"][:n]) & (cut["face"] >= 0)).mean() > 0.5


def test_fragile_cap_of_the_shadow_scene():
    from oracle import mesh_ref
    v, f = ref.mesh("ico2")
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    means, _, _, _, normals = mesh_ref.mesh_to_splats(vt, ft, mesh_ref.vertex_normals(vt, ft))
    pos, nrm = means.numpy()[::ref.SHADOW_STRIDE], normals.numpy()[::ref.SHADOW_STRIDE]
    assert pos.shape[0] == 640
    for offset in (1e-5, 1e-3):
        e = ref.shadow_expected(pos, nrm, offset)
        print(f"shadow offset {offset}: fragile {100 * e['fragile_any'].mean():.3f} %, occluded {e['occluded'].mean():.2f}")
        assert e["fragile_any"].mean() <= FRAGILE_CAP
        assert 0.3 < e["occluded"].mean() < 0.7                                       # half of a closed surface is in its own shadow


# ---- the C-ABI validates before it touches the device --------------------------------------------------------------------------
def _lib_and_dummies():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 16)()                                                          # a host pointer: never dereferenced on these paths
    return lib, C.cast(buf, C.c_void_p), buf


def test_build_argument_validation():
    lib, p, _keep = _lib_and_dummies()
    assert lib.gs_bvh_bytes(0) == 0 and lib.gs_bvh_ws_bytes(0) == 0
    assert lib.gs_bvh_bytes(1) == 32 and lib.gs_bvh_bytes(1280) == 32 * 2559
    assert lib.gs_bvh_bytes((1 << 30) + 1) == 0 and lib.gs_bvh_ws_bytes((1 << 30) + 1) == 0 and lib.gs_bvh_bytes(1 << 30) > 0
    assert lib.gs_bvh_ws_bytes(1280) >= 1280 * (8 + 4) * 2
    rc = lib.gs_bvh_build(3, 0, p, p, p, 32, p, 1 << 20, None)
    assert rc == -1 and b"empty" in lib.gs_last_error()
    rc = lib.gs_bvh_build(3, (1 << 30) + 1, p, p, p, 32, p, 1 << 20, None)
    assert rc == -1 and b"too many faces" in lib.gs_last_error()
    rc = lib.gs_bvh_build(3, 4, p, p, p, 32 * 7, p, 8, None)
    assert rc == -1 and b"workspace" in lib.gs_last_error()
    rc = lib.gs_bvh_build(3, 4, p, p, p, 32, p, lib.gs_bvh_ws_bytes(4), None)
    assert rc == -1 and b"node buffer" in lib.gs_last_error()
    rc = lib.gs_bvh_build(3, 4, None, p, p, 32 * 7, p, lib.gs_bvh_ws_bytes(4), None)
    assert rc == -1 and b"NULL" in lib.gs_last_error()


@pytest.mark.parametrize("entry", ["gs_ray_occluded", "gs_ray_closest"])
def test_query_argument_validation(entry):
    lib, p, _keep = _lib_and_dummies()
    fn = getattr(lib, entry)
    outs = lambda o: (o, None) if entry == "gs_ray_occluded" else (o, o, o, None)
    head = lambda F, P, S: (3, F, p, p, None, P, S, p, p, 1, 0.0, 1.0)
    rc = fn(*head(0, 1, 1), *outs(p))
    assert rc == -1 and b"empty" in lib.gs_last_error()
    rc = fn(*head((1 << 30) + 1, 1, 1), *outs(p))
    assert rc == -1 and b"too many faces" in lib.gs_last_error()
    rc = fn(*head(1, 1, -1), *outs(p))
    assert rc == -1 and b"negative S" in lib.gs_last_error()
    rc = fn(*head(1, 1 << 20, 1 << 12), *outs(p))
    assert rc == -1 and b"too many rays" in lib.gs_last_error()
    rc = fn(*head(1, 1, 1), *outs(None))
    assert rc == -1 and b"null output" in lib.gs_last_error()
    assert fn(*head(1, 0, 5), *outs(None)) == 0                                       # no rays: a no-op


def test_python_ops_refuse_cpu_tensors_empty_meshes_and_bad_shapes():
    import geosplatting_amd as gs
    from geosplatting_amd import raytrace
    from geosplatting_amd._lib import GeoSplatHipError
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2]])
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.MeshBVH(v, f)
    with pytest.raises(ValueError, match=r"empty mesh.*\(0, 3\)"):
        gs.MeshBVH(v, torch.zeros(0, 3, dtype=torch.int64))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.shadow_visibility(None, v, v, v)
    o = torch.zeros(5, 3)
    assert raytrace.ray_layout(o, torch.zeros(5, 7, 3)) == (5, 7, 1)
    assert raytrace.ray_layout(o, torch.zeros(7, 3)) == (5, 7, 0)
    assert raytrace.ray_layout(o, torch.zeros(5, 3)) == (5, 1, 1)
    for bad in (torch.zeros(4, 7, 3), torch.zeros(7, 2), torch.zeros(5, 7, 3, dtype=torch.float64), torch.zeros(3)):
        with pytest.raises(ValueError, match=r"dirs must be.*" + str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")):
            raytrace.ray_layout(o, bad)
    with pytest.raises(ValueError, match=r"origins must be.*\(5, 2\)"):
        raytrace.ray_layout(torch.zeros(5, 2), torch.zeros(5, 3))


def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    """The traversal keeps one integer of state (skip links) and selects axes with conditional moves: a private stack or array
    indexed at run time would live in scratch memory.  The compiler's resource report for gfx950 must show 0 scratch bytes per lane
    for every kernel of csrc/gs_bvh.hip (no GPU needed: hipcc cross-compiles)."""
    import os
    import re
    import shutil
    import subprocess
    from geosplatting_amd import build as B
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, *[f for f in B.FLAGS if f != "-fPIC"], "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(B.CSRC, "gs_bvh.hip"), "-o", str(tmp_path / "gs_bvh.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    report = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, flags=re.S)
    mine = {name: int(scratch) for name, scratch in report if "bvh_" in name}
    print(mine)
    assert len(mine) == 9 and sum("bvh_query_kernel" in n for n in mine) == 4                # five build kernels, four query forms
    assert all(v == 0 for v in mine.values()), mine
