"""GPU tests of the mesh rasterizer's `near_clip` option (csrc/gs_meshclip_dev.h, gs_meshraster.hip, gs_meshaa.hip through
geosplatting_amd.meshrender) against the float64 / int64 restatement tests/meshclip_ref.py.

Exact tier.  Unit intrinsics, near = 0.5, inside vertices at Z = 1 on multiples of 1/16, outside vertices at Z = 0, -1, -3: the cut
parameter t = 0.5 / (1 - Z) is 1/2, 1/4 or 1/8, every cut, projection and snap is exact in float32, so the face map must equal the
reference's bit for bit for cull 'none' and 'back', and two runs must be identical.

No-change tier.  On meshraster_ref's perspective scenes (no crossing face) `near_clip=True` returns the bits of `near_clip=False`,
from `rasterize_mesh` and from `antialias`.

Perspective tier (meshclip_ref.SCENES).  Off the fragile pixels the face is the reference's; on them it is one of the reference's
candidates; no pixel in the eroded interior of a clipped polygon is empty.  Non-crossing faces keep the budget of
tests/test_gpu_meshraster.py.  The values of a crossing face follow csrc/gs_meshclip_dev.h mc_values; with eps = 2^-23, every
rounding at most eps / 2 relative, first order, in float64 quantities of the face at the pixel (|.| taken term by term):
  * d: dx = ((px + 0.5) - cx) / fx rounds twice: <= eps |dx| (px + 0.5 is exact); e1 = P1 - P0, e2 = P2 - P0: <= eps / 2 each;
  * h = d x e2, e.g. hx = dy e2z - e2y: the product inherits eps + eps / 2 and rounds, the difference rounds:
        <= 2.5 eps H,  H = (|dy e2z| + |e2y|, |e2x| + |dx e2z|, |dx e2y| + |dy e2x|);
  * a = (e1x hx + e1y hy) + e1z hz: each term inherits 2.5 eps H and eps / 2 from e1 and rounds, two sums: <= 4.5 eps A,  A = |e1| . H;
  * nu = P0 . h (P0 is exact): <= 4 eps U,  U = |P0| . H;
  * g = P0 x e1: <= 1.5 eps G,  G = |P0| x |e1| term by term;
  * nv = (dx gx + dy gy) + gz: <= 4 eps V,  V = |dx| Gx + |dy| Gy + Gz;      nt = e2 . g: <= 3.5 eps T,  T = |e2| . G;
  * r = -1 / a: relative 4.5 eps A / |a| + eps / 2;   b1 = nu r, b2 = nv r, depth = nt r round once more:
        |error b1| <= (4 U + 4.5 A |b1|) eps / |a| + eps |b1|,      |error b2| likewise with V,
        |error depth| <= (3.5 T + 4.5 A |depth|) eps / |a| + eps |depth|;
  * b0 = (1 - b1) - b2: <= error b1 + error b2 + eps (|1 - b1| + |b0|) / 2.
Measured on an MI355X, the largest error as a fraction of the budget over the crossing faces' solid pixels (b0, b1, depth), then over
the non-crossing faces' against their own budget (b, depth); no face differed from the reference's, fragile pixels included:
    floor16        0.113  0.160  0.293      0.026  0.015          (fragile share 0.0137)
    floor32        0.141  0.166  0.221      0.019  0.012          (0.0256)
    floor16_37x53  0.103  0.141  0.311      0.020  0.013          (0.0153)
    guard          0.144  0.189  0.201      0.017  0.011          (0.0134)
render_mesh's interpolated depth against rast[..., 2] on crossing faces: 0.052 of its budget.

Backward.  d verts_cam per element against torch float64 autograd of the reference at fixed face ids (the ray / plane form for the
pixels of crossing faces, meshraster_ref.values_torch for the others), upstream gradients zero at fragile pixels; the bound is the
project's gradient contract, 1e-4 of the float64 sum of the absolute per-pixel contributions.  Measured on floor16: at most 0.31 of
the bound over all vertices, 0.0005 on the vertices behind the plane (3 of them receive a gradient).

Antialias.  The debug decisions without their receiving-pixel bits equal meshclip_ref.aa_decisions on the non-fragile pairs; pairs with
a crossing foreground face are 0; at least one pair is "not a silhouette" because of a crossing neighbour.  Measured on floor16: 66
blended pairs, 148 fragile pairs, 192 with a crossing foreground, 5 held back by a crossing neighbour, no decision differing.
"""
import functools
import types

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import meshrender
from tests import meshclip_ref as clip
from tests import meshraster_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
UNIT = (1.0, 1.0, 0.0, 0.0)
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV)


def _rast(vc, faces, intr, **kw):
    return gs.rasterize_mesh(_dev(vc, torch.float32), _dev(faces), intr, near_clip=True, **kw)


def _face_map(rast):
    return (rast[..., 3].long() - 1).cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact tier
def _exact_cases():
    nan = float("nan")
    cases = {}
    # cuts at (12, 34) and (35, 19); the same face with the other winding behind it (equal depth: the lower id wins, or the cull decides)
    cases["one inside"] = ([(10, 4, 1), (2, 30, 0), (40, 26, -1)], [(0, 1, 2), (0, 2, 1)])
    # the clip edge runs along y = 10.5 from x = 16 to x = 32, through pixel centres
    cases["two inside"] = ([(4, 3, 1), (20, 3, 1), (12, 7.5, 0)], [(0, 2, 1)])
    cases["two crossing faces on a crossing edge"] = ([(10, 10, 1), (30, 12, 1), (14, 40, -1), (44, 38, -3)], [(0, 2, 1), (1, 2, 3)])
    # the shared edge runs along y = 20.5 and the clip edge along y = 30.5, both through pixel centres
    cases["crossing beside non-crossing"] = ([(6.5, 20.5, 1), (26.5, 20.5, 1), (16, 8, 1), (16, 10, 0), (26.5, 4.5, 1)],
                                             [(0, 1, 2), (1, 0, 3), (1, 4, 2)])
    cases["wholly behind"] = ([(5, 5, 0), (20, 5, -1), (5, 20, 0.5), (30, 30, 1), (40, 30, 1), (30, 40, 1)], [(0, 1, 2), (3, 4, 5)])
    cases["a NaN vertex"] = ([(nan, 3, 1), (10, 3, 1), (5, 9, 0), (20, 20, 1), (30, 20, 1), (25, 29, -1), (3, nan, 0)],
                             [(0, 1, 2), (3, 4, 5), (3, 4, 6)])
    # sub-triangles (8, 6), (42, 19), (16.5, 33) and wider: beyond the 16 x 16 box of the thread-per-triangle pass
    cases["a large sub-triangle"] = ([(8, 6, 1), (60, 20, -1), (10, 90, -3), (50, 4, 1), (2, 50, 1), (70, 70, 0)], [(0, 2, 1), (3, 5, 4)])
    verts, faces, base = [], [], 0
    for v, f in cases.values():
        verts += v
        faces += [tuple(base + i for i in t) for t in f]
        base += len(v)
    cases["all together"] = (verts, faces)
    return {k: (np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int64)) for k, (v, f) in cases.items()}


EXACT = _exact_cases()
EXACT_MIN_CROSSING_PIXELS = {"wholly behind": 0, "a NaN vertex": 20}


@pytest.mark.parametrize("size", [(64, 64), (37, 53)], ids=["64x64", "37x53"])
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_tier(name, size):
    vc, faces = EXACT[name]
    intr = UNIT + size
    for cull in ("none", "back"):
        want = clip.rasterize(vc, faces, intr, near=0.5, cull=cull)
        a = _rast(vc, faces, intr, cull=cull, near=0.5)
        assert torch.equal(a, _rast(vc, faces, intr, cull=cull, near=0.5)), "two runs differ"
        got = _face_map(a)
        assert np.array_equal(got, want["face"]), f"cull {cull}: {(got != want['face']).sum()} pixels differ"
        r = a.cpu().numpy()
        assert np.all(r[got < 0] == 0.0)
        if cull == "none":
            assert want["crossing"].sum() >= EXACT_MIN_CROSSING_PIXELS.get(name, 50)
    # without the option the crossing faces are dropped whole
    plain = _face_map(gs.rasterize_mesh(_dev(vc), _dev(faces), intr, near=0.5))
    assert not np.isin(plain, np.flatnonzero(want["kind"] == 2)).any()


# ------------------------------------------------------------------------------------------------ no-change tier
@pytest.mark.parametrize("lat_long", [(8, 16), (16, 32)], ids=lambda t: f"sphere{t[0]}x{t[1]}")
def test_nothing_changes_without_a_crossing_face(lat_long):
    sc = ref.scene(*lat_long)
    assert not (clip.classify(sc["vc"], sc["faces"], 1e-2) == 2).any()
    vc, faces = _dev(sc["vc"]), _dev(sc["faces"])
    for cull in ("none", "back"):
        plain = gs.rasterize_mesh(vc, faces, sc["intr"], cull=cull)
        assert torch.equal(gs.rasterize_mesh(vc, faces, sc["intr"], cull=cull, near_clip=True), plain)
        color = torch.rand(*plain.shape[:2], 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
        topo = gs.mesh_edge_topology(faces)
        want = gs.antialias(color, plain, vc, faces, sc["intr"], topology=topo, cull=cull)
        assert torch.equal(gs.antialias(color, plain, vc, faces, sc["intr"], topology=topo, cull=cull, near_clip=True), want)


# ------------------------------------------------------------------------------------------------ perspective tier
def _plain_budget(sc, res):
    """K of tests/test_gpu_meshraster.py for the reference's winning (non-crossing) triangle at each pixel"""
    fx, fy, cx, cy, H, W = sc["intr"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xs, ys, zs = ref.project(sc["vc"], sc["intr"])
        tri = sc["faces"][np.maximum(res["face"], 0)]
        gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
        qx, qy = xs[tri] - gx[..., None], ys[tri] - gy[..., None]
        D = np.maximum(np.abs(qx), np.abs(qy)).max(-1)
        M = np.maximum(np.abs(xs[tri] - cx) + abs(cx), np.abs(ys[tri] - cy) + abs(cy)).max(-1)
        S = np.abs((qx[..., 1] * qy[..., 2] - qy[..., 1] * qx[..., 2]) + (qx[..., 2] * qy[..., 0] - qy[..., 2] * qx[..., 0]) +
                   (qx[..., 0] * qy[..., 1] - qy[..., 0] * qx[..., 1]))
        z = zs[tri]
        return EPS * (6 * D * D + 4 * D * M) * (z.max(-1) / z.min(-1)) / S


def _crossing_budget(sc, res):
    """(budget b0, b1, depth) [H,W] of the module docstring for the reference's winning face at each pixel, taken as a crossing face"""
    fx, fy, cx, cy, H, W = sc["intr"]
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    P = sc["vc"][sc["faces"][np.maximum(res["face"], 0)]].astype(np.float64)                 # [H,W,3,3]
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dx, dy = np.abs((gx - cx) / fx), np.abs((gy - cy) / fy)
    P0 = np.abs(P[..., 0, :])
    e1, e2 = np.abs(P[..., 1, :] - P[..., 0, :]), np.abs(P[..., 2, :] - P[..., 0, :])
    Hx, Hy, Hz = dy * e2[..., 2] + e2[..., 1], e2[..., 0] + dx * e2[..., 2], dx * e2[..., 1] + dy * e2[..., 0]
    A = e1[..., 0] * Hx + e1[..., 1] * Hy + e1[..., 2] * Hz
    U = P0[..., 0] * Hx + P0[..., 1] * Hy + P0[..., 2] * Hz
    Gx = P0[..., 1] * e1[..., 2] + P0[..., 2] * e1[..., 1]
    Gy = P0[..., 2] * e1[..., 0] + P0[..., 0] * e1[..., 2]
    Gz = P0[..., 0] * e1[..., 1] + P0[..., 1] * e1[..., 0]
    V = dx * Gx + dy * Gy + Gz
    T = e2[..., 0] * Gx + e2[..., 1] * Gy + e2[..., 2] * Gz
    # |a| = |d . (e1 x e2)| from the signed quantities
    s1, s2 = P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :]
    n = np.cross(s1, s2)
    a = np.abs((gx - cx) / fx * n[..., 0] + (gy - cy) / fy * n[..., 1] + n[..., 2])
    b0, b1, depth = np.abs(res["b0"]), np.abs(res["b1"]), np.abs(res["depth"])
    b2 = np.abs(1.0 - res["b0"] - res["b1"])
    with np.errstate(divide="ignore", invalid="ignore"):
        err1 = (4 * U + 4.5 * A * b1) * EPS / a + EPS * b1
        err2 = (4 * V + 4.5 * A * b2) * EPS / a + EPS * b2
        errd = (3.5 * T + 4.5 * A * depth) * EPS / a + EPS * depth
        err0 = err1 + err2 + 0.5 * EPS * (np.abs(1.0 - res["b1"]) + b0)
    return err0, err1, errd


@pytest.mark.parametrize("name", clip.SCENES)
def test_perspective_tier(name):
    sc, res = clip.scene(name), clip.scene_result(name)
    fragile = res["fragile"]
    assert fragile.mean() <= clip.FRAGILE_CAP
    rast = _rast(sc["vc"], sc["faces"], sc["intr"], near=sc["near"])
    assert torch.equal(rast, _rast(sc["vc"], sc["faces"], sc["intr"], near=sc["near"]))
    got = _face_map(rast)
    solid = ~fragile
    print(f"{name}: fragile {fragile.mean():.4f}, faces differing on fragile pixels {(got != res['face'])[fragile].sum()}, "
          f"on the others {(got != res['face'])[solid].sum()}")
    assert np.array_equal(got[solid], res["face"][solid])
    assert ref.is_candidate(res, got)[fragile].all()
    assert not (res["interior"] & (got < 0)).any(), "a crack inside a clipped polygon"
    r = rast.cpu().numpy().astype(np.float64)
    assert np.all(r[got < 0] == 0.0)
    cross = solid & res["crossing"]
    plain = solid & (res["face"] >= 0) & ~res["crossing"]
    assert cross.mean() >= 0.04 and plain.mean() >= 0.2
    K = _plain_budget(sc, res)
    frac_b = max((np.abs(r[..., 0] - res["b0"]) / (4 * K + 3 * EPS))[plain].max(), (np.abs(r[..., 1] - res["b1"]) / (4 * K + 3 * EPS))[plain].max())
    with np.errstate(divide="ignore", invalid="ignore"):
        frac_d = (np.abs(r[..., 2] - res["depth"]) / (res["depth"] * (6 * K + 3 * EPS)))[plain].max()
    err0, err1, errd = _crossing_budget(sc, res)
    fc = [(np.abs(r[..., k] - res[key]) / bud)[cross].max() for k, (key, bud) in enumerate((("b0", err0), ("b1", err1), ("depth", errd)))]
    print(f"{name}: largest fraction of the budget: non-crossing b {frac_b:.3f}, depth {frac_d:.3f}; "
          f"crossing b0 {fc[0]:.3f}, b1 {fc[1]:.3f}, depth {fc[2]:.3f}")
    assert frac_b <= 1.0 and frac_d <= 1.0
    assert max(fc) <= 1.0


# ------------------------------------------------------------------------------------------------ backward
def test_backward_reaches_the_vertices_behind_the_plane():
    name = "floor16"
    sc, res = clip.scene(name), clip.scene_result(name)
    intr, faces = sc["intr"], sc["faces"]
    H, W = intr[4], intr[5]
    gen = torch.Generator().manual_seed(5)
    keep = torch.as_tensor(~res["fragile"])
    up = torch.randn(H, W, 3, generator=gen, dtype=torch.float64) * keep[..., None]
    vc_g = _dev(sc["vc"]).requires_grad_()
    rast = gs.rasterize_mesh(vc_g, _dev(faces), intr, near=sc["near"], near_clip=True)
    got = _face_map(rast.detach())
    assert np.array_equal(got[~res["fragile"]], res["face"][~res["fragile"]])
    (d_vc,) = torch.autograd.grad((rast[..., :3] * up.float().to(DEV)).sum(), (vc_g,))

    vc64 = torch.as_tensor(sc["vc"], dtype=torch.float64)
    p, p_index, hit = ref.gather_rows(vc64, faces, res["face"])
    p.requires_grad_()
    cross = torch.as_tensor(res["crossing"])
    safe = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], dtype=torch.float64)
    plain = ref.values_torch(torch.where(cross[..., None, None], safe, p), hit & ~cross, intr)
    clipped = clip.values_torch(p, hit & cross, intr)
    b0, b1, depth = (torch.where(cross, c, q) for c, q in zip(clipped, plain))
    (gp,) = torch.autograd.grad((up[..., 0] * b0 + up[..., 1] * b1 + up[..., 2] * depth).sum(), (p,))
    want = ref.scatter_rows(gp, p_index, hit, vc64.shape)
    scale = ref.scatter_rows(gp.abs(), p_index, hit, vc64.shape)
    err = (d_vc.cpu().double() - want).abs()
    behind = torch.as_tensor(sc["vc"][:, 2] <= np.float32(sc["near"]))
    frac = (err / (1e-4 * scale))[scale > 0].max()
    frac_behind = (err / (1e-4 * scale))[behind[:, None] & (scale > 0)].max()
    print(f"{name} d vc: largest fraction of the bound {float(frac):.4f}, on the vertices behind the plane {float(frac_behind):.4f}; "
          f"{int((behind[:, None] & (scale > 0)).any(-1).sum())} of them receive a gradient")
    assert torch.all(err <= 1e-4 * scale), f"{float(frac):.3f} of the bound"
    assert (d_vc.cpu()[behind].abs().sum(-1) > 0).sum() >= 3
    assert torch.isfinite(d_vc).all()


# ------------------------------------------------------------------------------------------------ antialias
def test_antialias_decisions_next_to_crossing_faces():
    name = "floor16"
    sc, res = clip.scene(name), clip.scene_result(name)
    intr = sc["intr"]
    vc, faces = _dev(sc["vc"]), _dev(sc["faces"]).to(torch.int32)
    rast = gs.rasterize_mesh(vc, faces, intr, near=sc["near"], near_clip=True)
    topo = gs.mesh_edge_topology(faces)
    color = torch.rand(*rast.shape[:2], 3, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    out, dbg = meshrender.antialias_raw(color, rast, vc, faces, intr, topo, near=sc["near"], debug=True, near_clip=True)
    out2, dbg2 = meshrender.antialias_raw(color, rast, vc, faces, intr, topo, near=sc["near"], debug=True, near_clip=True)
    assert torch.equal(out, out2) and torch.equal(dbg, dbg2)
    want = clip.aa_decisions(rast.cpu().numpy(), sc["vc"], sc["faces"], intr, res, near=sc["near"])
    got = dbg.cpu().numpy().astype(np.int64)
    decided = got & ~12                                                             # without the receiving-pixel bits
    solid = ~want["fragile"]
    blocks = want["crossing_blocks"] & solid
    print(f"{name}: {int((want['code'] > 0).sum())} blended pairs, {int(want['fragile'].sum())} fragile pairs, "
          f"{int(want['crossing_fg'].sum())} with a crossing foreground, {int(blocks.sum())} held back by a crossing neighbour, "
          f"decisions differing on solid pairs {int((decided != want['code'])[solid].sum())}")
    assert np.array_equal(decided[solid], want["code"][solid])
    assert want["crossing_fg"].sum() >= 10 and np.all(got[want["crossing_fg"]] == 0)
    assert blocks.sum() >= 1 and np.all(got[blocks] == 0)
    # the same pairs WITHOUT the option blend: there the crossing face is no neighbour
    _, dbg_plain = meshrender.antialias_raw(color, rast, vc, faces, intr, topo, near=sc["near"], debug=True)
    assert (dbg_plain.cpu().numpy()[blocks] != 0).any()
    # the autograd path runs on the same decisions
    c, v = color.clone().requires_grad_(), vc.clone().requires_grad_()
    aa = gs.antialias(c, rast, v, faces, intr, topology=topo, near=sc["near"], near_clip=True)
    assert torch.equal(aa, out)
    gc, gv = torch.autograd.grad((aa * torch.rand_like(aa)).sum(), (c, v))
    assert torch.isfinite(gc).all() and torch.isfinite(gv).all() and float(gv.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ Python layers
def _camera(sc):
    fx, fy, cx, cy, H, W = sc["intr"]
    return gs.Camera(_dev(sc["c2w"], torch.float32).contiguous(), fx, fy, cx, cy, W, H)


@functools.lru_cache(maxsize=None)
def _through_the_camera(name):
    """the scene as the Python layers rasterize it: camera-space positions from to_camera_space in float32"""
    sc = clip.scene(name)
    cam = _camera(sc)
    vw = _dev(sc["vw"], torch.float32)
    vc = meshrender.to_camera_space(vw, cam).cpu().numpy()
    sc = dict(sc, vc=vc)
    return sc, cam, vw, clip.rasterize(vc, sc["faces"], sc["intr"], near=sc["near"])


def test_render_mesh_visible_faces_and_stage3_surface():
    sc, cam, vw, res = _through_the_camera("floor16")
    faces = _dev(sc["faces"])
    assert res["fragile"].mean() <= clip.FRAGILE_CAP
    solid = ~res["fragile"]
    cross = solid & res["crossing"]
    assert cross.mean() >= 0.04
    maps = gs.render_mesh(vw, faces, cam, outputs=("depth", "alpha", "face"), cull="none", near=sc["near"], near_clip=True)
    face = maps["face"][..., 0].cpu().numpy()
    assert np.array_equal(face[solid], res["face"][solid])
    # depth = sum b_i Z_i of the kernel's own b against the kernel's own depth: three b errors times |Z_i|, the depth's error, three
    # products and two sums of the interpolation, and b2 = 1 - b0 - b1 (two more roundings on |Z_2|)
    rast = maps["rast"].cpu().double().numpy()
    depth = maps["depth"][..., 0].cpu().double().numpy()
    err0, err1, errd = _crossing_budget(sc, res)
    Z = np.abs(sc["vc"][sc["faces"][np.maximum(res["face"], 0)]][..., 2].astype(np.float64))
    b = np.stack((np.abs(res["b0"]), np.abs(res["b1"]), np.abs(1 - res["b0"] - res["b1"])), -1)
    budget = err0 * Z[..., 0] + err1 * Z[..., 1] + (err0 + err1 + EPS) * Z[..., 2] + errd + 4 * EPS * (b * Z).sum(-1)
    frac = (np.abs(depth - rast[..., 2]) / budget)[cross].max()
    print(f"render_mesh depth on crossing faces: largest fraction of the budget {frac:.3f}")
    assert frac <= 1.0
    assert np.array_equal(maps["alpha"][..., 0].cpu().numpy()[solid], (res["face"] >= 0)[solid].astype(np.float32))
    # without the option the same call loses every crossing face
    lost = gs.render_mesh(vw, faces, cam, outputs=("face",), cull="none", near=sc["near"])["face"][..., 0].cpu().numpy()
    assert (lost[cross] != res["face"][cross]).all()

    seen = set(gs.visible_faces(vw, faces, cam, near=sc["near"], near_clip=True).tolist())
    wanted = set(np.unique(res["face"][cross]).tolist())
    assert len(wanted) >= 5 and wanted <= seen
    assert not (wanted & set(gs.visible_faces(vw, faces, cam, near=sc["near"]).tolist()))

    # Stage3Model.surface reads only the frozen mesh.  Its near plane is rasterize_mesh's default 0.01: the scene is shrunk tenfold
    # towards the eye, which leaves every projection where it was and puts the same faces across that plane.
    eye = torch.tensor(clip.EYE, device=DEV)
    vw = eye + 0.1 * (vw - eye)
    vc3 = meshrender.to_camera_space(vw, cam).cpu().numpy()
    res3 = clip.rasterize(vc3, sc["faces"], sc["intr"], near=1e-2)
    covered = ~res3["fragile"] & (res3["face"] >= 0)
    model = types.SimpleNamespace(mesh_v=vw, mesh_i=faces)
    positions, mask = gs.Stage3Model.surface(model, cam, near_clip=True)
    assert positions.shape == (*res["face"].shape, 3) and mask.shape == (*res["face"].shape, 1)
    assert (res3["crossing"] & covered).sum() >= 50
    assert bool((mask[..., 0].cpu().numpy()[covered] == 1.0).all()), "a hole in the mask where the reference is covered"
    holes = gs.Stage3Model.surface(model, cam)[1][..., 0].cpu().numpy()
    assert (holes[res3["crossing"] & covered] == 0.0).any()
    # the positions lie on the (shrunk) floor: y within its jitter of -0.012 on the crossing faces
    y = positions[..., 1].cpu().numpy()[res3["crossing"] & covered]
    assert np.all(np.abs(y + 0.012) <= 0.00101)
