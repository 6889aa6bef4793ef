"""GPU tests of the mesh rasterizer (csrc/gs_meshraster.hip through geosplatting_amd.meshrender) against the float64 / int64 restatement
tests/meshraster_ref.py.

Exact tier.  Vertices at Z = 1 with fx = fy = 1, cx = cy = 0 on multiples of 1/16 px: projection and snapping are exact, every edge
function is an integer, so the face-id map must equal the reference's bit for bit, ties and pixels on edges included.

Perspective tier.  A float32 evaluation may decide a pixel differently from float64 only where a decision is within rounding of its
threshold; those pixels are *fragile* (tests/meshraster_ref.py: within 3/256 px of an edge, or two candidate depths within 2^-16) and
tests/test_meshraster_cpu.py caps their share from the reference alone.  On the other pixels the face is identical and b0, b1 and
the depth are within a budget derived from the arithmetic, in float64 quantities of the winning triangle at that pixel
(eps = 2^-23, a rounding is at most eps / 2 relative):
    D = the largest |coordinate| of a vertex relative to the pixel centre (px),  M = max_i max(|xs_i - cx| + |cx|, |ys_i - cy| + |cy|),
    S = |sum e| = twice the triangle's screen area (px^2),  zmin, zmax = the Z range of its vertices.
  * xs = fma(fx, X / Z, cx): the quotient and the fma round once each, |error| <= eps M; q = xs - centre rounds once more:
    |error of q| <= eps (M + D / 2);
  * e_i = q_a x q_b: two products and a difference, <= 2 eps D^2, plus the inherited 4 D eps (M + D / 2): <= eps (4 D^2 + 4 D M);
  * w_i = e_i / Z_i with the rounded reciprocal (|e_i| <= 2 D^2): <= eps (6 D^2 + 4 D M) / zmin;  N = sum w adds 3 of these and eps |N|
    (inside the triangle the w_i share a sign);  |N| >= S / zmax;
  * b_i = w_i (1 / N), |b_i| <= 1: <= (1 + 3 |b_i|) error(w) / |N| + 2.5 eps, written  4 K + 3 eps  with
        K = eps (6 D^2 + 4 D M) (zmax / zmin) / S;
  * depth = sum e / N: relative error 3 error(e) / S + 3 error(w) / |N| + 3 eps <= 6 K + 3 eps.
Measured on an MI355X: the largest error is 0.036 of the budget for b and 0.022 for the depth, over the three scenes; no face differs
from the reference's, fragile pixels included.

Interpolation takes the kernel's own rast as input, so its budget is that of the sum alone:
    4 eps (|b0 a0| + |b1 a1| + (1 + |b0| + |b1|) |a2|)        (b2 = 1 - b0 - b1 rounds twice, each product once, two sums).
Measured: 0.26 of the budget at most.

Backward.  d attr and d vc are compared per element with torch float64 autograd of the reference at fixed face ids; the bound is
1e-4 of the float64 sum of the absolute per-pixel contributions to that element, the project's contract for gradients.  Upstream
gradients are zero at fragile pixels.  Measured: at most 0.41 of the bound for d vc and 0.40 for d attr (both on the 16 x 32 sphere; 0.15 and 0.04 on the 8 x 16 one).
"""
import functools
import math

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import meshrender
from geosplatting_amd import synthetic as syn
from tests import meshraster_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
CAPS = {(8, 16): 0.05, (16, 32): 0.05, (48, 96): 0.12}
UNIT = (1.0, 1.0, 0.0, 0.0)
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV)


def _rast(vc, faces, intr, **kw):
    return gs.rasterize_mesh(_dev(vc, torch.float32), _dev(faces), intr, **kw)


def _face_map(rast):
    return (rast[..., 3].long() - 1).cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact tier
def _z1(xy):
    xy = np.asarray(xy, dtype=np.float32)
    return np.concatenate((xy, np.ones((xy.shape[0], 1), dtype=np.float32)), 1)


def _grid_case():
    n = 14
    xy = [(3.5 + 1.5 * i, 2.5 + 1.5 * j) for j in range(n + 1) for i in range(n + 1)]
    at = lambda i, j: j * (n + 1) + i
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = at(i, j), at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)] if (i + j) % 2 else [(a, b, c), (b, d, c)]
    return _z1(xy), faces


def _exact_cases():
    cases = {}
    cases["tessellated rectangle, shared edges"] = _grid_case()
    ring = [(4, 4), (12.5, 4), (28, 4), (28, 16.5), (28, 28), (9.5, 28), (4, 28), (4, 20.5)]
    cases["fan, edges through pixel centres"] = (_z1([(14.5, 17.5)] + ring + [(2.5, 2.5), (30.5, 30.5), (2.5, 30.5), (33.5, 3.5)]),
                                                 [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)] + [(9, 10, 11), (9, 12, 10)])
    cases["coplanar overlap, a depth tie"] = (_z1([(2, 2), (14, 2), (2, 14), (3, 3), (15, 3), (3, 15)]), [(3, 4, 5), (0, 1, 2)])
    cases["degenerate"] = (_z1([(1, 1), (5, 5), (9, 9), (1, 1), (9, 1), (1, 9), (4, 4), (4, 4), (9, 2)]),
                           [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    cases["partly and wholly off-screen"] = (_z1([(-7.5, 3), (9, -4.25), (6, 12), (50, 30), (70.5, 33), (58, 70), (-30, -3), (-5, -9),
                                                  (-12, -1), (100, 100), (130, 101), (104, 140), (20, 20), (24, 20), (20, 25)]),
                                             [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14)])
    behind = _z1([(1, 1), (9, 1), (1, 9), (10, 10), (20, 10), (10, 20)])
    behind[0, 2] = 0.005
    cases["behind near"] = (behind, [(0, 1, 2), (3, 4, 5)])
    cases["larger than the thread path's box"] = (_z1([(-10, -20.5), (90, 5), (3.25, 80), (5, 5), (22.0625, 5), (5, 22)]),
                                                  [(0, 1, 2), (3, 4, 5)])
    verts, faces, base = [], [], 0
    for v, f in cases.values():                                                   # everything in one mesh: ties across the cases
        verts.append(v)
        faces += [tuple(base + i for i in t) for t in f]
        base += v.shape[0]
    cases["all together"] = (np.concatenate(verts, 0), faces)
    return cases


EXACT = _exact_cases()


@pytest.mark.parametrize("size", [(64, 64), (37, 53)], ids=["64x64", "37x53"])
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_tier(name, size):
    vc, faces = EXACT[name]
    faces = np.asarray(faces, dtype=np.int64)
    intr = UNIT + size
    for cull in ("none", "back"):
        want = ref.rasterize(vc, faces, intr, cull=cull)
        a = _rast(vc, faces, intr, cull=cull)
        b = _rast(vc, faces, intr, cull=cull)
        assert torch.equal(a, b), "two runs differ"
        got = _face_map(a)
        assert np.array_equal(got, want["face"]), f"{(got != want['face']).sum()} pixels differ"
        r = a.cpu().numpy()
        hit = got >= 0
        assert np.all(r[~hit] == 0.0) and np.all(r[hit][:, 2] == 1.0)             # Z = 1 everywhere: the depth is exact
    assert got.shape == size


def test_int64_and_int32_faces_give_the_same_rast():
    vc, faces = EXACT["all together"]
    f64 = _dev(np.asarray(faces, dtype=np.int64))
    a = gs.rasterize_mesh(_dev(vc), f64, UNIT + (64, 64))
    b = gs.rasterize_mesh(_dev(vc), f64.to(torch.int32), UNIT + (64, 64))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ perspective tier
@functools.lru_cache(maxsize=None)
def _scene(lat_long):
    sc = ref.scene(*lat_long)
    res = ref.rasterize(sc["vc"], sc["faces"], sc["intr"])
    return sc, res


def _budget_terms(sc, res):
    """K [H,W] of the module docstring for the reference's winning triangle at each pixel (inf where empty), and zmax"""
    fx, fy, cx, cy, H, W = sc["intr"]
    xs, ys, zs = ref.project(sc["vc"], sc["intr"])
    tri = sc["faces"][np.maximum(res["face"], 0)]                                  # [H,W,3]
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    qx, qy = xs[tri] - gx[..., None], ys[tri] - gy[..., None]
    D = np.maximum(np.abs(qx), np.abs(qy)).max(-1)
    M = np.maximum(np.abs(xs[tri] - cx) + abs(cx), np.abs(ys[tri] - cy) + abs(cy)).max(-1)
    S = np.abs((qx[..., 1] * qy[..., 2] - qy[..., 1] * qx[..., 2]) + (qx[..., 2] * qy[..., 0] - qy[..., 2] * qx[..., 0]) +
               (qx[..., 0] * qy[..., 1] - qy[..., 0] * qx[..., 1]))
    z = zs[tri]
    K = EPS * (6 * D * D + 4 * D * M) * (z.max(-1) / z.min(-1)) / S
    return np.where(res["face"] >= 0, K, np.inf)


@pytest.mark.parametrize("lat_long", sorted(CAPS), ids=lambda t: f"sphere{t[0]}x{t[1]}")
def test_perspective_tier(lat_long):
    sc, res = _scene(lat_long)
    fragile = res["fragile"]
    assert fragile.mean() <= CAPS[lat_long]
    rast = _rast(sc["vc"], sc["faces"], sc["intr"])
    assert torch.equal(rast, _rast(sc["vc"], sc["faces"], sc["intr"]))
    got = _face_map(rast)
    solid = ~fragile
    print(f"{lat_long}: fragile {fragile.mean():.4f}, faces differing on fragile pixels {(got != res['face'])[fragile].sum()}, "
          f"on the others {(got != res['face'])[solid].sum()}")
    assert np.array_equal(got[solid], res["face"][solid])
    assert ref.is_candidate(res, got)[fragile].all()
    r = rast.cpu().numpy().astype(np.float64)
    K = _budget_terms(sc, res)
    hit = solid & (res["face"] >= 0)
    assert hit.mean() > 0.8
    budget_b = 4 * K + 3 * EPS
    budget_d = res["depth"] * (6 * K + 3 * EPS)
    frac_b = max((np.abs(r[..., 0] - res["b0"]) / budget_b)[hit].max(), (np.abs(r[..., 1] - res["b1"]) / budget_b)[hit].max())
    frac_d = (np.abs(r[..., 2] - res["depth"]) / budget_d)[hit].max()
    print(f"{lat_long}: largest fraction of the budget: b {frac_b:.3f}, depth {frac_d:.3f}")
    assert frac_b <= 1.0 and frac_d <= 1.0
    assert np.all(r[got < 0] == 0.0)


# ------------------------------------------------------------------------------------------------ culling
def _camera(sc):
    fx, fy, cx, cy, H, W = sc["intr"]
    return gs.Camera(_dev(sc["c2w"], torch.float32).contiguous(), fx, fy, cx, cy, W, H)


def test_back_culling_and_visible_faces():
    sc, _ = _scene((16, 32))
    nf = sc["n_sphere_faces"]
    faces = sc["faces"][:nf]
    cam = _camera(sc)
    vw = _dev(sc["vw"], torch.float32)
    vc = meshrender.to_camera_space(vw, cam).cpu().numpy()                          # the float32 positions the kernel rasterizes
    res = ref.rasterize(vc, faces, sc["intr"], cull="back")
    seen = set(gs.visible_faces(vw, _dev(faces), cam, cull="back").tolist())
    solid = set(np.unique(res["face"][~res["fragile"] & (res["face"] >= 0)]).tolist())
    frag_pix = np.flatnonzero(res["fragile"].ravel())
    maybe = set(res["cand_face"][np.isin(res["cand_pix"], frag_pix)].tolist())
    assert solid <= seen <= (solid | maybe), (len(solid - seen), len(seen - solid - maybe))
    v64 = sc["vw"].astype(np.float64)
    normal = np.cross(v64[faces[:, 1]] - v64[faces[:, 0]], v64[faces[:, 2]] - v64[faces[:, 0]])
    facing = ((np.asarray(ref.EYE) - v64[faces].mean(1)) * normal).sum(-1) / np.linalg.norm(normal, axis=-1)
    far = set(np.flatnonzero(facing < -1e-4).tolist())
    assert not (seen & far)
    ids = gs.visible_faces(vw, _dev(faces), cam)
    assert ids.dtype == torch.int64 and torch.equal(ids, ids.unique())


# ------------------------------------------------------------------------------------------------ interpolate
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("kind", ["vertex", "face_vertex"])
def test_interpolate_forward(kind, C):
    sc, res = _scene((8, 16))
    faces = sc["faces"]
    rast = _rast(sc["vc"], faces, sc["intr"])
    gen = torch.Generator().manual_seed(11 + C)
    shape = (sc["vc"].shape[0], C) if kind == "vertex" else (faces.shape[0], 3, C)
    attr = torch.randn(shape, generator=gen)
    out = gs.interpolate(attr.to(DEV), rast, _dev(faces)).cpu().double()
    assert out.shape == (*rast.shape[:2], C)
    r = rast.cpu().double()
    fm = _face_map(rast)
    rows, _, hit = ref.gather_rows(attr.double(), faces, fm)
    want = ref.interpolate_torch(rows, r[..., 0], r[..., 1], hit)
    b0, b1 = r[..., 0:1].abs(), r[..., 1:2].abs()
    budget = 4 * EPS * (b0 * rows[..., 0, :].abs() + b1 * rows[..., 1, :].abs() + (1 + b0 + b1) * rows[..., 2, :].abs())
    frac = ((out - want).abs() / budget)[hit].max()
    print(f"interpolate {kind} C={C}: largest fraction of the budget {float(frac):.3f}")
    assert frac <= 1.0
    assert torch.all(out[~hit] == 0.0)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("kind", ["vertex", "face_vertex"])
@pytest.mark.parametrize("lat_long", [(8, 16), (16, 32)], ids=lambda t: f"sphere{t[0]}x{t[1]}")
def test_backward(lat_long, kind):
    sc, res = _scene(lat_long)
    _check_backward(sc, sc["faces"], res, kind, str(lat_long))


def _check_backward(sc, faces, res, kind, label):
    intr = sc["intr"]
    H, W = intr[4], intr[5]
    C = 3
    gen = torch.Generator().manual_seed(5)
    keep = torch.as_tensor(~res["fragile"])
    up_r = torch.randn(H, W, 3, generator=gen, dtype=torch.float64) * keep[..., None]
    up_a = torch.randn(H, W, C, generator=gen, dtype=torch.float64) * keep[..., None]
    shape = (sc["vc"].shape[0], C) if kind == "vertex" else (faces.shape[0], 3, C)
    attr = torch.randn(shape, generator=gen)

    vc_g = _dev(sc["vc"]).requires_grad_()
    attr_g = attr.to(DEV).requires_grad_()
    rast = gs.rasterize_mesh(vc_g, _dev(faces), intr)
    out = gs.interpolate(attr_g, rast, _dev(faces))
    got = _face_map(rast.detach())
    assert np.array_equal(got[~res["fragile"]], res["face"][~res["fragile"]])
    loss = (rast[..., :3] * up_r.float().to(DEV)).sum() + (out * up_a.float().to(DEV)).sum()
    d_vc, d_attr = torch.autograd.grad(loss, (vc_g, attr_g))

    vc64 = torch.as_tensor(sc["vc"], dtype=torch.float64)
    p, p_index, hit = ref.gather_rows(vc64, faces, res["face"])
    rows, a_index, _ = ref.gather_rows(attr.double(), faces, res["face"])
    p.requires_grad_()
    rows.requires_grad_()
    b0, b1, depth = ref.values_torch(p, hit, intr)
    total = (up_r[..., 0] * b0 + up_r[..., 1] * b1 + up_r[..., 2] * depth).sum() + (up_a * ref.interpolate_torch(rows, b0, b1, hit)).sum()
    gp, ga = torch.autograd.grad(total, (p, rows))
    for name, mine, g, index, tshape in (("d vc", d_vc, gp, p_index, vc64.shape), ("d attr", d_attr, ga, a_index, attr.shape)):
        want = ref.scatter_rows(g, index, hit, tshape)
        scale = ref.scatter_rows(g.abs(), index, hit, tshape)
        err = (mine.cpu().double() - want).abs()
        assert scale.max() > 0
        frac = (err / (1e-4 * scale))[scale > 0].max()
        print(f"{label} {kind} {name}: largest fraction of the bound {float(frac):.4f}")
        assert torch.all(err <= 1e-4 * scale), f"{name}: {float(frac):.3f} of the bound"


# ------------------------------------------------------------------------------------------------ render_mesh
def _sphere_depths(vm, intr, radius):
    """view depth [H,W] of the sphere of `radius` at the world origin along every pixel's ray (nan where the ray misses), float64"""
    fx, fy, cx, cy, H, W = intr
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack(((gx - cx) / fx, (gy - cy) / fy, np.ones_like(gx)), -1)
    c = vm[:3, 3]                                                                   # the world origin in camera space
    a, b, c0 = (d * d).sum(-1), -2.0 * (d * c).sum(-1), float(c @ c) - radius * radius
    disc = b * b - 4 * a * c0
    with np.errstate(invalid="ignore"):
        return np.where(disc > 0, (-b - np.sqrt(disc)) / (2 * a), np.nan)


@pytest.mark.parametrize("normal_type", ["vertex", "flat"])
def test_render_mesh_on_an_icosphere(normal_type):
    radius = 0.5
    v, f = syn.icosphere(3, radius)
    v64 = v.double()
    sc = ref.scene(8, 16)
    cam = _camera(sc)
    intr = sc["intr"]
    vw, fd = v.to(DEV), f.to(DEV)
    maps = gs.render_mesh(vw, fd, cam, normal_type=normal_type)
    assert maps["depth"].shape == (64, 64, 1) and maps["normal"].shape == (64, 64, 3) and maps["alpha"].shape == (64, 64, 1)
    assert maps["face"].shape == (64, 64, 1) and maps["face"].dtype == torch.int64
    vc = meshrender.to_camera_space(vw, cam).cpu().numpy()
    faces = f.numpy()
    res = ref.rasterize(vc, faces, intr, cull="back")
    assert res["fragile"].mean() <= 0.05
    solid = ~res["fragile"]
    hit = solid & (res["face"] >= 0)
    face = maps["face"][..., 0].cpu().numpy()
    assert np.array_equal(face[solid], res["face"][solid])
    assert np.array_equal(maps["alpha"][..., 0].cpu().numpy()[solid], (res["face"] >= 0)[solid].astype(np.float32))
    K = _budget_terms(dict(sc, vc=vc, faces=faces), res)
    zmax = float(vc[:, 2].max())
    depth = maps["depth"][..., 0].cpu().double().numpy()
    # depth = sum b_i Z_i of the kernel's b: three b errors times Z, three products and two sums
    assert np.all((np.abs(depth - res["depth"]) <= 3 * (4 * K + 3 * EPS) * zmax + 4 * EPS * zmax)[hit])
    assert np.all(depth[face < 0] == 0.0)
    normal = maps["normal"].cpu().double()
    hit_t = torch.as_tensor(hit)
    if normal_type == "vertex":
        vn = gs.vertex_normals(vw, fd).cpu().double()
        rows, _, h = ref.gather_rows(vn, faces, res["face"])
        raw = ref.interpolate_torch(rows, torch.as_tensor(res["b0"]), torch.as_tensor(res["b1"]), h)
        length = raw.norm(dim=-1, keepdim=True)
        want = raw / length
        # three b errors on unit normals, the sum, the norm and the division; relative to the interpolated length
        tol = (3 * torch.as_tensor(4 * K + 3 * EPS)[..., None] + 8 * EPS) * 2 / length
        assert torch.all(((normal - want).abs() <= tol)[hit_t])
        assert torch.all(normal[torch.as_tensor(face < 0)] == torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    else:
        e1, e2 = v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]
        n = torch.cross(e1, e2, dim=-1)
        want = (n / n.norm(dim=-1, keepdim=True))[torch.as_tensor(np.maximum(res["face"], 0))]
        # edges are differences of coordinates of size <= radius (eps radius each), the cross product cancels by 1 / sin(angle)
        sin = n.norm(dim=-1) / (e1.norm(dim=-1) * e2.norm(dim=-1))
        tol = float((8 * EPS * radius / torch.minimum(e1.norm(dim=-1), e2.norm(dim=-1)) / sin).max()) + 8 * EPS
        assert torch.all(((normal - want).abs() <= tol)[hit_t])
    # the analytic sphere: the mesh is inscribed, so a covered pixel's depth lies between the ray's depth on the sphere and on the
    # sphere shrunk by the largest facet sagitta
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    la, lb, lc = (b - c).norm(dim=-1), (c - a).norm(dim=-1), (a - b).norm(dim=-1)
    circum = la * lb * lc / (2.0 * torch.cross(b - a, c - a, dim=-1).norm(dim=-1))
    sagitta = radius - math.sqrt(radius * radius - float(circum.max()) ** 2)
    outer = _sphere_depths(sc["vm"], intr, radius)
    inner = _sphere_depths(sc["vm"], intr, radius - sagitta)
    slack = 1e-5                                                                    # fp32 vertices and view matrix, far above the budget
    inside = hit & np.isfinite(inner)
    assert inside.sum() > 500
    assert np.all(depth[inside] >= outer[inside] - slack) and np.all(depth[inside] <= inner[inside] + slack)
    assert np.all(depth[hit] >= outer[hit] - slack)


def test_render_mesh_is_differentiable_and_takes_an_obj(tmp_path):
    v, f = syn.icosphere(2, 0.5)
    from geosplatting_amd import fusion
    fusion.save_obj(tmp_path / "m.obj", v, f)
    v2, f2 = fusion.load_obj(tmp_path / "m.obj")
    sc = ref.scene(8, 16)
    cam = _camera(sc)
    vw = v2.to(DEV).requires_grad_()
    maps = gs.render_mesh(vw, f2.to(DEV), cam)
    (maps["depth"].sum() + maps["normal"][..., 0].sum()).backward()
    assert vw.grad is not None and torch.isfinite(vw.grad).all() and float(vw.grad.abs().sum()) > 0


def test_cpu_tensors_raise():
    from geosplatting_amd._lib import GeoSplatHipError
    sc = ref.scene(8, 16)
    vc, faces = torch.as_tensor(sc["vc"]), torch.as_tensor(sc["faces"])
    with pytest.raises(GeoSplatHipError):
        gs.rasterize_mesh(vc, faces, sc["intr"])
    with pytest.raises(GeoSplatHipError):
        gs.rasterize_mesh(vc.to(DEV), faces, sc["intr"])
    rast = gs.rasterize_mesh(vc.to(DEV), faces.to(DEV), sc["intr"])
    with pytest.raises(GeoSplatHipError):
        gs.interpolate(vc, rast, faces.to(DEV))
    with pytest.raises(GeoSplatHipError):
        gs.render_mesh(torch.as_tensor(sc["vw"]), faces, _camera(sc))
