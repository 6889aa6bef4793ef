"""GPU tests of the mesh antialias pass (csrc/gs_meshaa.hip through geosplatting_amd.meshrender) against the float64 / exact-integer
restatement tests/meshaa_ref.py.  The restatement takes the device's own rast: the rasterizer has its tests in test_gpu_meshraster.py.

Decisions (which pairs blend, their exit edges, which pixel receives) are read from the DEBUG OUTPUT of the raw call
(meshrender.antialias_raw(..., debug=True): one code per pair at the pair's first pixel) and must equal the restatement's exactly.

Exact tier.  Unit intrinsics, vertices at Z = 1 and Z = 2 on positions whose 256-fold is exact in float32: every snapped integer is the
same on both sides, so every decision must agree, ties and edges through pixel centres included.

Perspective tier.  The checks hold on the pairs that are not *fragile* (tests/meshaa_ref.py); tests/test_meshaa_cpu.py caps their share.
On elements touched by a fragile pair, `out` only has to be finite and inside the range of the colours that can reach it.

Values.  |out - reference| <= 1e-4 kappa max|color| per element, kappa the largest slope factor 1 + |D_par| / |D_perp| over the pairs
that blend into the element: a float32 screen position at <= 64 px carries about 1e-5 px of rounding, the crossing x* amplifies it by
kappa, the rest is margin inside the project's 1e-4 contract.  Elements no pair blends into must equal `color` bit for bit.

Backward.  d color and d verts_cam against float64 autograd of the restatement; |err| <= 1e-4 times the sum over the pairs of
kappa |the pair's contribution to that element| (for d color plus the |upstream gradient| of the element itself, the identity part).
Upstream gradients are zero on the elements of fragile pairs.  The weight |d - 0.5| has a kink at d = 0.5, where the receiving pixel
changes (d = 0.5 itself blends nothing and has no gradient, on both sides); the exact-tier scenes keep 1e-3 away from it unless they
sit on it exactly (tests/test_meshaa_cpu.py).

Measured on an MI355X: no decision differs; values at most 0.0007 of the bound on the exact tier and 0.014 on the perspective tier;
d color at most 0.012 (exact) and 0.23 (perspective), d verts_cam 0.001 and 0.003 of their bounds; the outline test ends at 1.553 px
with the loss at 0.022 of its start.
"""
import functools

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import meshrender
from geosplatting_amd._lib import GeoSplatHipError
from tests import meshaa_ref as aa
from tests import meshraster_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = aa.exact_scenes()
SIZES = [(64, 64), (37, 53)]
PERSPECTIVE = [(8, 16), (12, 24)]                                                 # (tests/test_meshaa_cpu.py caps their fragile share)


def _dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ topology
def _fan_and_sphere():
    _, sphere = ref.uv_sphere(8, 16)
    return {"sphere": sphere,
            "an edge on three faces": np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4), (2, 1, 5)]),
            "degenerate face and an index out of range": np.array([(0, 1, 2), (3, 3, 1), (2, 1, 70000), (4, 4, 4), (1, 0, -5), (70000, 2, 9)])}


@pytest.mark.parametrize("name", sorted(_fan_and_sphere()))
def test_topology(name):
    faces = _fan_and_sphere()[name]
    topo = gs.mesh_edge_topology(_dev(faces))
    assert isinstance(topo, gs.EdgeTopology) and topo.n_faces == faces.shape[0]
    assert topo.neighbours() == aa.topology(faces)
    assert gs.mesh_edge_topology(_dev(faces).to(torch.int32)).neighbours() == aa.topology(faces)


# ------------------------------------------------------------------------------------------------ forward
def _colors(shape, C, seed):
    return torch.rand(*shape, C, generator=torch.Generator().manual_seed(seed)) + 0.25


def _forward_case(vc, faces, intr, C, cull="none", pixel_fragile=None, seed=3):
    """the device's rast, out and decisions, and the restatement's on that rast"""
    H, W = intr[4], intr[5]
    faces = np.asarray(faces, dtype=np.int64)
    v, f = _dev(vc, torch.float32), _dev(faces).to(torch.int32)
    rast = gs.rasterize_mesh(v, f, intr, cull=cull)
    color = _colors((H, W), C, seed)
    topo = gs.mesh_edge_topology(f)
    out, dbg = meshrender.antialias_raw(color.to(DEV), rast, v, f, intr, topo, cull=cull, debug=True)
    again = meshrender.antialias_raw(color.to(DEV), rast, v, f, intr, topo, cull=cull)
    assert torch.equal(out, again), "two forward runs differ"
    assert torch.equal(out, gs.antialias(color.to(DEV), rast, v, _dev(faces), intr, cull=cull)), "the public call differs from the raw one"
    pairs = aa.analyse(rast.cpu().numpy(), vc, faces, intr, cull=cull, pixel_fragile=pixel_fragile)
    want = aa.blend(pairs, color.double(), torch.as_tensor(np.asarray(vc), dtype=torch.float64)[pairs["verts"]], intr)
    return dict(color=color, out=out.cpu(), dbg=dbg.cpu().numpy(), pairs=pairs, want=want, rast=rast)


def _check_forward(case, label):
    color, out, pairs, want = case["color"], case["out"].double(), case["pairs"], case["want"]
    H, W, C = color.shape
    cand = pairs["cand"]
    # decisions, on every pair that is not fragile: blended or not, the exit edge, the foreground and the receiving pixel
    expected = aa.decision_map(pairs, want["code"]).reshape(-1, 2)
    got = case["dbg"].reshape(-1, 2)
    solid = ~cand["fragile"]
    differ = got[cand["first"], cand["axis"]] != expected[cand["first"], cand["axis"]]
    assert not differ[solid].any(), f"{differ[solid].sum()} decisions differ"
    is_cand = np.zeros((H * W, 2), dtype=bool)
    is_cand[cand["first"], cand["axis"]] = True
    assert np.all(got[~is_cand] == 0), "a pair with equal face ids was blended"
    # values: elements that only solid pairs touch
    touched_fragile = torch.zeros(H * W, dtype=torch.bool)
    touched_fragile[torch.as_tensor(np.concatenate((cand["first"][~solid], cand["second"][~solid])))] = True
    kappa = torch.zeros(H * W, dtype=torch.float64)
    if pairs["n"]:
        kappa.scatter_reduce_(0, want["target"], torch.as_tensor(pairs["kappa"]), "amax")
    bound = 1e-4 * kappa[:, None] * float(color.abs().max())
    err = (out - want["out"]).abs().reshape(-1, C)
    ok = ~touched_fragile
    check = ok & (kappa > 0)
    assert check.sum() > 10
    frac = float((err / bound)[check].max())
    print(f"{label}: {pairs['n']} blended pairs ({int((~solid).sum())} of {len(solid)} candidates fragile), "
          f"largest kappa {pairs['kappa'].max():.1f}, largest fraction of the bound {frac:.4f}")
    assert torch.all(err[check] <= bound[check]), f"{frac:.3f} of the bound"
    untouched = ok & (kappa == 0)
    assert torch.equal(case["out"].reshape(-1, C)[untouched], color.reshape(-1, C)[untouched])
    # fragile elements: finite, and inside the range of the pixel's own colour and its four neighbours'
    pad = torch.nn.functional.pad(color.permute(2, 0, 1)[None], (1, 1, 1, 1), mode="replicate")[0].permute(1, 2, 0)
    stack = torch.stack((pad[1:-1, 1:-1], pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]), 0)
    lo, hi = stack.min(0).values.reshape(-1, C), stack.max(0).values.reshape(-1, C)
    o = case["out"].reshape(-1, C)
    assert torch.isfinite(o).all()
    assert torch.all((o >= lo - 1e-6) & (o <= hi + 1e-6)), "an element left the range of the colours around it"


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "37x53"])
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_tier(name, size, C):
    vc, faces = EXACT[name]
    case = _forward_case(vc, faces, aa.UNIT + size, C)
    case["pairs"]["cand"]["fragile"][:] = False                                    # every integer agrees: every pair is compared
    assert case["pairs"]["n"] > 10
    _check_forward(case, f"{name} {size} C={C}")


@functools.lru_cache(maxsize=None)
def _scene(lat_long):
    sc = ref.scene(*lat_long)
    return sc, ref.rasterize(sc["vc"], sc["faces"], sc["intr"])


@pytest.mark.parametrize("lat_long", PERSPECTIVE, ids=lambda t: f"sphere{t[0]}x{t[1]}")
def test_perspective_tier(lat_long):
    sc, res = _scene(lat_long)
    case = _forward_case(sc["vc"], sc["faces"], sc["intr"], 4, pixel_fragile=res["fragile"])
    assert case["pairs"]["n"] > 100
    _check_forward(case, f"sphere {lat_long}")


# ------------------------------------------------------------------------------------------------ backward
def _check_backward(vc, faces, intr, label, pixel_fragile=None, C=3):
    H, W = intr[4], intr[5]
    faces = np.asarray(faces, dtype=np.int64)
    gen = torch.Generator().manual_seed(7)
    color = _colors((H, W), C, 5)
    v_g = _dev(vc, torch.float32).requires_grad_()
    c_g = color.to(DEV).requires_grad_()
    rast = gs.rasterize_mesh(v_g.detach(), _dev(faces), intr)
    pairs = aa.analyse(rast.cpu().numpy(), vc, faces, intr, pixel_fragile=pixel_fragile)
    cand = pairs["cand"]
    keep = torch.ones(H * W, dtype=torch.float64)
    keep[torch.as_tensor(np.concatenate((cand["first"][cand["fragile"]], cand["second"][cand["fragile"]])))] = 0.0
    up = torch.randn(H, W, C, generator=gen, dtype=torch.float64) * keep.reshape(H, W, 1)
    out = gs.antialias(c_g, rast, v_g, _dev(faces), intr)
    d_color, d_vc = torch.autograd.grad((out * up.float().to(DEV)).sum(), (c_g, v_g))

    # the restatement with per-pair copies of everything a pair reads: the gradient of a copy is that pair's own contribution
    vc64 = torch.as_tensor(np.asarray(vc), dtype=torch.float64)
    solid = torch.as_tensor(~pairs["fragile"])
    verts = torch.as_tensor(pairs["verts"])
    pv = vc64[verts].requires_grad_()
    c64 = color.double()
    plain = aa.blend(pairs, c64, pv.detach(), intr)
    flat = c64.reshape(-1, C)
    ident = c64.clone().requires_grad_()
    ct, co = flat[plain["target"]].clone().requires_grad_(), flat[plain["other"]].clone().requires_grad_()
    total = (aa.blend(pairs, ident, pv, intr, pair_colors=(ct, co))["out"] * up).sum()
    g_ident, g_ct, g_co, g_pv = torch.autograd.grad(total, (ident, ct, co, pv))
    kap = torch.as_tensor(pairs["kappa"])
    want_c = g_ident.reshape(-1, C).index_add(0, plain["target"], g_ct).index_add(0, plain["other"], g_co)
    scale_c = g_ident.abs().reshape(-1, C).index_add(0, plain["target"], g_ct.abs() * kap[:, None]).index_add(
        0, plain["other"], g_co.abs() * kap[:, None])
    want_v = torch.zeros_like(vc64).index_add(0, verts.reshape(-1), g_pv.reshape(-1, 3))
    scale_v = torch.zeros_like(vc64).index_add(0, verts.reshape(-1), (g_pv.abs() * kap[:, None, None]).reshape(-1, 3))
    assert float(scale_v.max()) > 0 and int((g_pv.abs().sum((1, 2)) > 0).sum()) > 10
    for name, mine, want, scale in (("d color", d_color.cpu().double().reshape(-1, C), want_c, scale_c),
                                    ("d verts_cam", d_vc.cpu().double(), want_v, scale_v)):
        err = (mine - want).abs()
        frac = float((err / (1e-4 * scale))[scale > 0].max())
        print(f"{label} {name}: largest fraction of the bound {frac:.4f}")
        assert torch.all(err <= 1e-4 * scale), f"{name}: {frac:.3f} of the bound"
    # the entry point overwrites its outputs: a second backward gives the same d color bit for bit
    assert torch.equal(d_color, torch.autograd.grad((gs.antialias(c_g, rast, v_g, _dev(faces), intr) * up.float().to(DEV)).sum(), c_g)[0])


@pytest.mark.parametrize("name", sorted(EXACT))
def test_backward_exact(name):
    vc, faces = EXACT[name]
    _check_backward(vc, faces, aa.UNIT + (64, 64), name)


def test_backward_perspective():
    sc, res = _scene((8, 16))
    _check_backward(sc["vc"], sc["faces"], sc["intr"], "sphere (8, 16)", pixel_fragile=res["fragile"])


def test_moving_a_vertical_edge():
    """One triangle whose right edge x = 20.3 crosses all 64 rows (its ends lie far above and below the image).  Moving that edge by
    delta = 1/64 px moves every row's crossing by delta: sum(alpha) grows by 64 delta = 1, and the gradient says 64 per pixel.
    Rounding: xs and q = xs - centre each round once at magnitude < 32 (2^-20 px together), in both evaluations of all 64 rows; the
    sums are taken in float64."""
    delta = 1.0 / 64.0
    intr = aa.UNIT + (64, 64)
    faces = _dev(np.array([(0, 1, 2)]))

    def alpha_sum(x):
        v = _dev(aa._at([(x, -100.0), (x, 164.0), (-300.0, 32.0)], 1.0), torch.float32).requires_grad_()
        rast = gs.rasterize_mesh(v.detach(), faces, intr)
        alpha = (rast[..., 3:] > 0).float()
        out = gs.antialias(alpha, rast, v, faces, intr)
        assert float(out.detach()[:, 20].min()) > 0.25 and float(out.detach()[:, 20].max()) < 0.35 and torch.all(out[:, 21] == 0)
        (grad,) = torch.autograd.grad(out.sum(), v)
        return float(out.detach().double().sum()), grad.cpu().double()

    s0, g0 = alpha_sum(20.3)
    s1, _ = alpha_sum(20.3 + delta)
    rounding = 2 * 64 * 2.0 ** -20
    print(f"sum(alpha) moved by {s1 - s0:.7f} (64 delta = {64 * delta}), d sum / d x = {float(g0[:2, 0].sum()):.5f}")
    assert abs((s1 - s0) - 64 * delta) <= rounding
    assert abs(float(g0[:2, 0].sum()) - 64.0) <= 64 * 1e-5
    assert torch.all(g0[2] == 0) and float(g0[:2, 1].abs().max()) <= 1e-3


# ------------------------------------------------------------------------------------------------ the public surface
def _camera(sc):
    fx, fy, cx, cy, H, W = sc["intr"]
    return gs.Camera(_dev(sc["c2w"], torch.float32).contiguous(), fx, fy, cx, cy, W, H)


def _sphere():
    sc = ref.scene(8, 16)
    sv, sf = ref.uv_sphere(8, 16, 0.5)
    return sc, _dev(sv, torch.float32), _dev(sf)


def test_render_mesh_without_antialias_is_unchanged():
    sc, v, f = _sphere()
    cam = _camera(sc)
    vn = gs.vertex_normals(v, f)                          # (summed by atomics: computed once, so that two calls can be compared bit for bit)
    a, b = gs.render_mesh(v, f, cam, vertex_normals=vn), gs.render_mesh(v, f, cam, vertex_normals=vn, antialias=False)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_render_mesh_with_antialias():
    sc, v, f = _sphere()
    cam = _camera(sc)
    v.requires_grad_()
    plain = gs.render_mesh(v, f, cam)
    maps = gs.render_mesh(v, f, cam, antialias=True, topology=gs.mesh_edge_topology(f))
    assert torch.equal(maps["rast"], plain["rast"]) and torch.equal(maps["face"], plain["face"])
    assert maps["depth"].shape == (64, 64, 1) and maps["normal"].shape == (64, 64, 3) and maps["alpha"].shape == (64, 64, 1)
    a0, a1 = plain["alpha"][..., 0], maps["alpha"][..., 0]
    changed = a1 != a0
    # the outline: pixels with a 4-neighbour of the other coverage
    pad = torch.nn.functional.pad(a0[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
    outline = (pad[:-2, 1:-1] != a0) | (pad[2:, 1:-1] != a0) | (pad[1:-1, :-2] != a0) | (pad[1:-1, 2:] != a0)
    assert int(changed.sum()) > 40 and torch.all(outline[changed])
    assert torch.all((a1[changed] > 0) & (a1[changed] < 1))
    length = maps["normal"].norm(dim=-1)
    assert torch.all((length - 1).abs() < 1e-5)
    # d alpha / d vertices: only on vertices of faces that own an outline pixel
    (grad,) = torch.autograd.grad(maps["alpha"].sum(), v)
    face = plain["face"][..., 0]
    outline_faces = face[outline & (face >= 0)].unique()
    allowed = torch.zeros(v.shape[0], dtype=torch.bool, device=DEV)
    allowed[f[outline_faces].reshape(-1)] = True
    moved = grad.abs().sum(-1) > 0
    assert int(moved.sum()) > 8 and not bool((moved & ~allowed).any())
    assert torch.isfinite(grad).all()


def test_cpu_tensors_raise():
    sc, v, f = _sphere()
    intr = sc["intr"]
    vc = _dev(ref.scene(8, 16)["vc"][:v.shape[0]], torch.float32)
    rast = gs.rasterize_mesh(vc, f, intr)
    color = torch.rand(64, 64, 2, device=DEV)
    with pytest.raises(GeoSplatHipError):
        gs.mesh_edge_topology(f.cpu())
    with pytest.raises(GeoSplatHipError):
        gs.antialias(color.cpu(), rast, vc, f, intr)
    with pytest.raises(GeoSplatHipError):
        gs.antialias(color, rast.cpu(), vc, f, intr)
    with pytest.raises(GeoSplatHipError):
        gs.antialias(color, rast, vc.cpu(), f, intr)
    with pytest.raises(GeoSplatHipError):
        gs.antialias(color, rast, vc, f[:-1], intr, topology=gs.mesh_edge_topology(f))
    with pytest.raises(GeoSplatHipError):
        gs.render_mesh(v.cpu(), f.cpu(), _camera(sc), antialias=True)


# ------------------------------------------------------------------------------------------------ it moves an outline
def _fit_translation(antialias):
    """the 8 x 16 sphere, a single learnable translation along the camera's x axis in units of one pixel at the sphere's centre, 60
    Adam steps on the silhouette loss against the (antialiased) alpha of the same sphere translated by 1.5 px"""
    sc, v, f = _sphere()
    cam = _camera(sc)
    focal = sc["intr"][0]
    right = torch.as_tensor(sc["c2w"][:3, 0], dtype=torch.float32).to(DEV)            # the camera's x axis in the world (also OpenCV's)
    px = float(sc["vm"][2, 3]) / focal                                              # world length of one pixel at the centre's depth
    topo = gs.mesh_edge_topology(f)
    with torch.no_grad():
        target = gs.render_mesh(v + 1.5 * px * right, f, cam, outputs=("alpha",), antialias=True, topology=topo)["alpha"]
    t = torch.zeros((), device=DEV, requires_grad=True)
    opt = torch.optim.Adam([t], lr=0.1)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        alpha = gs.render_mesh(v + t * px * right, f, cam, outputs=("alpha",), antialias=antialias, topology=topo)["alpha"]
        loss = gs.silhouette_loss(alpha, target)
        losses.append(float(loss))
        if loss.requires_grad:
            loss.backward()
        opt.step()
    return losses, float(t), t.grad


def test_antialias_moves_an_outline():
    losses, t, _ = _fit_translation(True)
    print(f"silhouette loss {losses[0]:.5f} -> {losses[-1]:.5f}, translation {t:.4f} px (target 1.5)")
    assert losses[-1] < 0.25 * losses[0]
    assert abs(t - 1.5) <= 0.25
    # without the pass alpha has no gradient at all: the translation stays exactly where it started
    losses, t, grad = _fit_translation(False)
    assert t == 0.0 and (grad is None or float(grad.abs()) == 0.0)
    assert losses[-1] == losses[0] and losses[0] > 0
