"""CPU checks of the mesh rasterizer's float64 restatement (tests/meshraster_ref.py) and of the conditions the GPU tests rely on.

The fragile caps are CONDITIONS on the scenes, computed here from the reference alone: a GPU test that leaves fragile pixels out of a
per-pixel comparison is only meaningful while few pixels are fragile.  Measured with this reference (cull='none'): 8 x 16 sphere
1.5 %, 16 x 32 sphere 2.9 %, 48 x 96 sphere (triangles of about 1.4 px: the thread-per-triangle path) 7.9 %.
"""
import numpy as np
import pytest
import torch

from tests import meshraster_ref as ref

CAPS = {(8, 16): 0.05, (16, 32): 0.05, (48, 96): 0.12}
UNIT = (1.0, 1.0, 0.0, 0.0)


def _at_z1(xy):
    xy = np.asarray(xy, dtype=np.float32)
    return np.concatenate((xy, np.ones((xy.shape[0], 1), dtype=np.float32)), 1)


def _coverage_counts(vc, faces, H, W):
    """how many triangles cover each pixel: every triangle rasterized alone"""
    count = np.zeros((H, W), dtype=np.int64)
    for f in faces:
        count += ref.rasterize(vc, np.asarray([f]), UNIT + (H, W))["face"] >= 0
    return count


def test_fan_covers_every_pixel_exactly_once():
    """a square [4, 28]^2 cut into a fan around an off-centre dyadic point: every shared edge passes through pixel centres somewhere"""
    ring = [(4, 4), (12.5, 4), (28, 4), (28, 16.5), (28, 28), (9.5, 28), (4, 28), (4, 20.5)]
    vc = _at_z1([(14.5, 17.5)] + ring)
    faces = [(0, 1 + k, 1 + (k + 1) % len(ring)) for k in range(len(ring))]
    faces[2] = faces[2][::-1]                                                     # winding must not matter
    count = _coverage_counts(vc, faces, 32, 32)
    expect = np.zeros((32, 32), dtype=np.int64)
    expect[4:28, 4:28] = 1                                                        # centres 4.5 .. 27.5: the top-left rule on the square
    assert np.array_equal(count, expect)


def test_grid_covers_every_pixel_exactly_once():
    """a grid of 1.5 px cells on multiples of 1/2 px, alternating diagonals: vertices and edges ON pixel centres"""
    n = 12
    xy = [(3.5 + 1.5 * i, 2.5 + 1.5 * j) for j in range(n + 1) for i in range(n + 1)]
    at = lambda i, j: j * (n + 1) + i
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = at(i, j), at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)] if (i + j) % 2 else [(a, b, c), (b, d, c)]
    count = _coverage_counts(_at_z1(xy), faces, 24, 24)
    ys, xs = np.meshgrid(np.arange(24) + 0.5, np.arange(24) + 0.5, indexing="ij")
    expect = ((xs >= 3.5) & (xs < 21.5) & (ys >= 2.5) & (ys < 20.5)).astype(np.int64)
    assert np.array_equal(count, expect)
    whole = ref.rasterize(_at_z1(xy), np.asarray(faces), UNIT + (24, 24))
    assert np.array_equal(whole["face"] >= 0, expect.astype(bool))


def test_depth_tie_keeps_the_lower_face_and_flags_the_pixel():
    vc = _at_z1([(2, 2), (14, 2), (2, 14), (3, 3), (15, 3), (3, 15)])
    res = ref.rasterize(vc, np.asarray([(3, 4, 5), (0, 1, 2)]), UNIT + (16, 16))
    both = (ref.rasterize(vc, np.asarray([(3, 4, 5)]), UNIT + (16, 16))["face"] >= 0) & \
           (ref.rasterize(vc, np.asarray([(0, 1, 2)]), UNIT + (16, 16))["face"] >= 0)
    assert both.sum() > 20 and np.all(res["face"][both] == 0) and np.all(res["fragile"][both])
    assert np.all(res["depth"][res["face"] >= 0] == 1.0)


def test_dropped_triangles():
    vc = np.array([[1, 1, 1], [9, 1, 1], [1, 9, 1],          # fine
                   [1, 1, 1], [5, 5, 1], [9, 9, 1],          # zero area
                   [1, 1, 0.005], [9, 1, 1], [1, 9, 1],      # a vertex behind near
                   [1, 1, 1], [40000, 1, 1], [1, 9, 1]],     # outside the snap range
                  dtype=np.float32)
    res = ref.rasterize(vc, np.arange(12).reshape(4, 3), UNIT + (16, 16))
    assert res["dropped"].tolist() == [False, True, True, True]
    assert set(np.unique(res["face"])) == {-1, 0}


def test_back_culling_sign_on_an_outward_wound_sphere():
    """the rule of the reference, (camera - centroid) . normal > 0, evaluated in float64 in world space, equals the sign test on the
    snapped screen area for every face that is not edge-on"""
    sc = ref.scene(16, 32)
    nf = sc["n_sphere_faces"]
    vw, faces = sc["vw"].astype(np.float64), sc["faces"][:nf]
    normal = np.cross(vw[faces[:, 1]] - vw[faces[:, 0]], vw[faces[:, 2]] - vw[faces[:, 0]])
    facing = ((np.asarray(ref.EYE) - vw[faces].mean(1)) * normal).sum(-1)
    res = ref.rasterize(sc["vc"], faces, sc["intr"], cull="back")
    clear = np.abs(facing) > 1e-6 * np.linalg.norm(normal, axis=-1)
    assert clear.mean() > 0.95
    assert np.array_equal(~res["dropped"][clear], facing[clear] > 0)
    seen = np.unique(res["face"][res["face"] >= 0])
    assert np.all(facing[seen] > 0)                                               # nothing of the far hemisphere


@pytest.mark.parametrize("lat_long", sorted(CAPS))
def test_fragile_caps(lat_long):
    sc = ref.scene(*lat_long)
    for cull in ("none", "back"):
        res = ref.rasterize(sc["vc"], sc["faces"], sc["intr"], cull=cull)
        share = res["fragile"].mean()
        print(f"sphere {lat_long} cull={cull}: fragile share {share:.4f}")
        assert share <= CAPS[lat_long]
        assert ref.is_candidate(res, res["face"]).all()                           # the reference's own winner is a candidate
    if lat_long == (8, 16):
        nf = len(sc["faces"])
        faces_seen = set(np.unique(res["face"]))
        assert nf - 3 in faces_seen and (nf - 2 in faces_seen or nf - 1 in faces_seen)          # background and quad are in view


def test_reference_autograd_agrees_with_finite_differences():
    sc = ref.scene(8, 16)
    res = ref.rasterize(sc["vc"], sc["faces"], sc["intr"])
    gen = torch.Generator().manual_seed(3)
    up = torch.randn(3, *res["face"].shape, generator=gen, dtype=torch.float64)
    up[:, torch.as_tensor(res["fragile"])] = 0.0
    attr = torch.randn(sc["vc"].shape[0], 3, generator=gen, dtype=torch.float64)
    up_a = torch.randn(*res["face"].shape, 3, generator=gen, dtype=torch.float64)

    def loss(vc):
        p, _, hit = ref.gather_rows(vc, sc["faces"], res["face"])
        rows, _, _ = ref.gather_rows(attr, sc["faces"], res["face"])
        b0, b1, d = ref.values_torch(p, hit, sc["intr"])
        return (up[0] * b0 + up[1] * b1 + up[2] * d).sum() + (up_a * ref.interpolate_torch(rows, b0, b1, hit)).sum()

    vc = torch.as_tensor(sc["vc"], dtype=torch.float64).requires_grad_()
    (g,) = torch.autograd.grad(loss(vc), vc)
    # the values restated in torch are the ones the numpy rasterizer returned
    p, _, hit = ref.gather_rows(vc.detach(), sc["faces"], res["face"])
    b0, b1, d = ref.values_torch(p, hit, sc["intr"])
    assert np.allclose(b0.numpy(), res["b0"], atol=1e-12) and np.allclose(d.numpy(), res["depth"], atol=1e-12)
    direction = torch.randn(vc.shape, generator=gen, dtype=torch.float64)
    h = 1e-6
    fd = (loss(vc.detach() + h * direction) - loss(vc.detach() - h * direction)) / (2 * h)
    assert abs(float(fd) - float((g * direction).sum())) <= 1e-6 * float((g.abs() * direction.abs()).sum())
    # per-pixel contributions scatter back to the same gradient
    p = p.clone().requires_grad_()
    rows, _, _ = ref.gather_rows(attr, sc["faces"], res["face"])
    b0, b1, d = ref.values_torch(p, hit, sc["intr"])
    total = (up[0] * b0 + up[1] * b1 + up[2] * d).sum() + (up_a * ref.interpolate_torch(rows, b0, b1, hit)).sum()
    (gp,) = torch.autograd.grad(total, p)
    _, index, _ = ref.gather_rows(vc.detach(), sc["faces"], res["face"])
    assert torch.allclose(ref.scatter_rows(gp, index, hit, vc.shape), g, rtol=1e-10, atol=1e-12)


def test_ops_refuse_cpu_tensors():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    sc = ref.scene(8, 16)
    vc, faces = torch.as_tensor(sc["vc"]), torch.as_tensor(sc["faces"])
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.rasterize_mesh(vc, faces, sc["intr"])
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.interpolate(vc, torch.zeros(4, 4, 4), faces)
    cam = gs.Camera(torch.as_tensor(sc["c2w"], dtype=torch.float32), *sc["intr"][:4], sc["intr"][5], sc["intr"][4])
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.render_mesh(torch.as_tensor(sc["vw"]), faces, cam)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.visible_faces(torch.as_tensor(sc["vw"]), faces, cam)
