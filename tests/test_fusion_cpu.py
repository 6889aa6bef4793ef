"""No-GPU checks of the depth-fusion feature: the derived marching-cubes table (scripts/make_mc_table.py -> csrc/gs_mc_table.h), the
float64 restatement tests/tsdf_ref.py on an analytic sphere, sphere_cameras and save_obj."""
import math
import os

import numpy as np
import pytest
import torch

from scripts import make_mc_table as mc
from tests import tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    return mc.build_table()


# ------------------------------------------------------------------------------------------------ the table
def test_generator_reproduces_committed_header(table):
    assert open(mc.HEADER).read() == mc.render_header(table)


def test_table_totals(table):
    """The figures a CPU prototype of the same rule gave: a cross-check of the rule, not a remembered table."""
    st = mc.table_stats(table)
    assert st == {"cases": 256, "max_tris": 5, "total_tris": 820, "hist": {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32},
                  "longest_loop": 7}


def test_every_case_uses_exactly_its_sign_changing_edges(table):
    for case in range(256):
        active = {e for e, (lo, hi) in enumerate(mc.EDGE_CORNERS) if ((case >> lo) & 1) != ((case >> hi) & 1)}
        loops = mc.case_loops(case)
        flat = [e for loop in loops for e in loop]
        assert len(flat) == len(set(flat)), case                     # every edge lies in one loop, once
        assert set(flat) == active, case
        assert all(len(loop) >= 3 for loop in loops), case
        used = {e for tri in table[case] for e in tri}
        assert used == active, case
        assert len(table[case]) == sum(len(loop) - 2 for loop in loops) <= mc.MAX_TRIS, case


def test_one_inside_corner_normals_point_away(table):
    for k in range(8):
        (tri,) = table[1 << k]
        n, m, c = mc._normal(tri), mc._edge_mid(tri[0]), mc.corner_offset(k)
        assert sum(n[i] * (m[i] - c[i]) for i in range(3)) > 0, k


def test_random_sign_grid_is_watertight():
    """7^3 cubes, random signs, all weights 1: every half-edge that is not on the grid boundary has exactly one opposite partner and no
    half-edge occurs twice."""
    rng = np.random.default_rng(7)
    res = (8, 8, 8)
    tsdf = rng.choice([-1.0, 1.0], size=8 ** 3) * rng.uniform(0.1, 1.0, size=8 ** 3)
    counts, verts, faces = ref.extract(tsdf, np.ones(8 ** 3), res, (0.0, 0.0, 0.0), 1.0)
    assert counts[2] == 7 ** 3 and counts[1] == len(faces) > 0
    assert faces.max() == counts[0] - 1 and len(np.unique(faces)) == counts[0]
    half = ref.half_edges(faces)
    assert max(half.values()) == 1
    lo, hi = 0.5, 7.5                                                # the boundary of the cube grid (voxel centres)
    for (a, b) in half:
        on_boundary = any((abs(verts[a][ax] - s) < 1e-12 and abs(verts[b][ax] - s) < 1e-12) for ax in range(3) for s in (lo, hi))
        if not on_boundary:
            assert (b, a) in half, (a, b)


# ------------------------------------------------------------------------------------------------ the reference on a sphere
def test_reference_sphere():
    """Sphere r = 0.5, bounds +-0.8, 32^3 voxels, 8 Fibonacci cameras at radius 3 (64^2, 40 degrees).  Measured with this scene:
    max | |v| - r | = 0.061 = 1.2 voxels, mean 0.013; asserted at 1.5 voxels.  The mesh is NOT closed: projective TSDF leaves open
    seams at silhouettes (17 unmatched half-edges here), which is the method."""
    das, vms, Ks = ref.sphere_scene()
    res, origin, vs = (32, 32, 32), (-0.8, -0.8, -0.8), 1.6 / 32
    z = np.zeros(32 ** 3)
    tsdf, weight, fragile, _ = ref.integrate(z, z, das, vms, Ks, res, origin, vs, sdf_trunc=5 * vs)
    assert np.array_equal(weight, np.rint(weight)) and weight.max() <= 8 and weight.min() >= 0
    assert fragile.mean() <= 0.05
    counts, verts, faces = ref.extract(tsdf, weight, res, origin, vs)
    assert counts[0] > 100 and counts[1] > 100
    err = np.abs(np.linalg.norm(verts, axis=1) - 0.5)
    print("sphere: V %d F %d max %.4f (%.2f voxels) mean %.4f fragile %.3f" % (counts[0], counts[1], err.max(), err.max() / vs,
                                                                              err.mean(), fragile.mean()))
    assert err.max() <= 1.5 * vs
    # normals point to free space: outward on the sphere
    tri = verts[faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((n * tri.mean(1)).sum(-1) > 0).mean() > 0.99


# ------------------------------------------------------------------------------------------------ small pieces
def test_sphere_cameras():
    import geosplatting_amd as gs
    g = torch.Generator().manual_seed(3)
    center = (0.1, -0.2, 0.3)
    cams = gs.sphere_cameras(16, 2.5, 80, 60, hfov_degree=60.0, center=center, up=(0.0, 1.0, 0.0), generator=g)
    assert len(cams) == 16
    c = torch.tensor(center)
    for cam in cams:
        R = cam.c2w[:, :3]
        assert torch.allclose(R.norm(dim=0), torch.ones(3), atol=1e-6)
        assert torch.allclose(R.T @ R, torch.eye(3), atol=1e-5)
        eye = cam.c2w[:, 3]
        assert abs(float((eye - c).norm()) - 2.5) < 1e-5
        forward = -R[:, 2]                                           # OpenGL: the camera looks along -z
        assert torch.allclose(forward, (c - eye) / (c - eye).norm(), atol=1e-5)
        assert cam.width == 80 and cam.height == 60 and cam.cx == 40 and cam.cy == 30
        assert abs(cam.fx - 40 / math.tan(math.radians(30))) < 1e-4 and cam.fy == cam.fx
    again = gs.sphere_cameras(16, 2.5, 80, 60, hfov_degree=60.0, center=center, up=(0.0, 1.0, 0.0),
                              generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(a.c2w, b.c2w) for a, b in zip(cams, again))
    # up = z: pitch is the elevation above the xy plane, uniform in its sine
    zc = torch.stack([cam.c2w[2, 3] for cam in gs.sphere_cameras(400, 1.0, 8, 8, generator=torch.Generator().manual_seed(0))])
    assert abs(float(zc.mean())) < 0.1 and float(zc.abs().max()) > 0.9


def test_save_obj_round_trips(tmp_path):
    from geosplatting_amd.fusion import load_obj, save_obj
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.123456789, -2.5e-7, 3e5]])
    f = torch.tensor([[0, 1, 2], [1, 3, 2]])
    path = tmp_path / "m.obj"
    save_obj(path, v, f)
    lines = path.read_text().splitlines()
    assert len(lines) == 6 and all(l.startswith("v ") for l in lines[:4]) and lines[4] == "f 1 2 3" and lines[5] == "f 2 4 3"
    v2, f2 = load_obj(path)
    assert torch.equal(v2, v) and torch.equal(f2, f)


def test_volume_refuses_cpu():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.TSDFVolume(8, device="cpu")
    lib = gs._lib.lib()
    assert lib.gs_tsdf_extract_ws_bytes(0, 4, 4) == 0 and lib.gs_tsdf_extract_ws_bytes(2048, 1024, 1024) == 0
    n = 12 * 10 * 9
    assert 0 < lib.gs_tsdf_extract_ws_bytes(12, 10, 9) <= 8 * n
    assert 0 < lib.gs_tsdf_extract_ws_bytes(512, 512, 512) <= 8 * 512 ** 3
    rc = lib.gs_tsdf_integrate(4, 4, 4, 0.0, 0.0, 0.0, 0.1, 0.5, 0.5, 4.0, 17, None, None, None)
    assert rc == -1 and b"n_views" in lib.gs_last_error()
    rc = lib.gs_tsdf_extract_count(4, 4, 4, None, None, 0, None, None)
    assert rc == -1 and b"workspace" in lib.gs_last_error()
