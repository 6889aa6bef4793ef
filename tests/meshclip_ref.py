"""Float64 / int64 restatement of the mesh rasterizer's `near_clip` option (geosplatting_amd/meshrender.py, csrc/gs_meshclip_dev.h): the
classification of faces, the clip of a crossing face against the near plane and the guard band, the values of a crossing face and the
antialias decisions next to crossing faces.  Test infrastructure; it shares no code with the kernels.

How it works.  Every crossing face is clipped in float64 from its float32 vertices (Sutherland-Hodgman, written on Python lists) and
fan-triangulated.  The sub-triangles, with their new vertices rounded to float32, replace the face in an EXPANDED mesh (same order of
faces, so a depth tie still goes to the lower original id); tests/meshraster_ref.py's `rasterize` gives its coverage, candidates and
fragile pixels with its own TOL = 3/256 px, and the sub-triangles are mapped back to their faces.  The values of a crossing face are
then evaluated per FACE with the ray / plane definition:  w_i = d . (P_{i+1} x P_{i+2}),  b_i = w_i / sum w,  depth = det[P0 P1 P2] / sum w,
d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1).

A wider fragile band along some edges.  meshraster_ref's TOL allows for the snap (a vertex moves by up to 0.5/256 px, a flipped snap
by 1/256) and leaves 2/256 px for everything else, which is ample for a vertex on the screen.  A clip vertex on the guard band is
16000 px away, where one float32 rounding is 16000 * 2^-23 = 0.002 px.  An error in t = dA / (dA - dB) moves the cut ALONG its edge
and does not move the edge's line; what moves the line is the rounding of the cut's own coordinates, C = fma(t, B - A, A):
    |error of C| <= (1 - t) error(A) + t error(B) + eps (|C| + |C - A| / 2) + eps |C| / 2      per coordinate
(the difference B - A and the fma round once each; the last term is this reference's own rounding of C to float32; A and B carry an
error when they are cuts of an earlier plane), and on the screen, for xs = fma(fx, X / Z, cx),
    e_v = fx (error(X) / Z + |X| error(Z) / Z^2) + 2 eps |xs - cx|     plus the same in y.
Only the on-screen share matters: along the edge from a to b the line moves by at most (1 - s) e_a + s e_b at parameter s, and s is
confined to where the edge runs through the image (grown by one pixel).  delta_e = the largest such value; an edge with delta_e above
2^-10 px gets a band of TOL + delta_e: the pixels within it are fragile, the face is a candidate there, and the pixel may be empty.
"""
import functools
import math

import numpy as np
import torch

from tests import meshaa_ref as aaref
from tests import meshraster_ref as ref

EPS = 2.0 ** -23
GUARD = 16000.0
WIDEN_FROM = 2.0 ** -10
TOL = ref.TOL
SNAP = ref.SNAP


# ------------------------------------------------------------------------------------------------ classification and clip
def classify(vc, faces, near):
    """per face: 0 dropped (no vertex inside, a non-finite coordinate, an index out of range), 1 all three inside, 2 crossing"""
    vc = np.asarray(vc, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    kind = np.zeros(faces.shape[0], dtype=np.int64)
    for f, t in enumerate(faces):
        if np.any(t < 0) or np.any(t >= vc.shape[0]):
            continue
        P = vc[t]
        inside = int((P[:, 2] > np.float32(near)).sum())
        if inside == 3:
            kind[f] = 1                                     # today's code, which drops it itself when something is not finite
        elif inside > 0 and np.all(np.isfinite(P)):
            kind[f] = 2
    return kind


def _planes(intr, near):
    """(a, b, c, d0, strict): the distance a X + b Y + c Z + d0 is positive inside"""
    fx, fy, cx, cy = (float(np.float32(a)) for a in intr[:4])
    n = float(np.float32(near))
    return [(0.0, 0.0, 1.0, -n, True), (-fx, 0.0, GUARD - cx, 0.0, False), (fx, 0.0, GUARD + cx, 0.0, False),
            (0.0, -fy, GUARD - cy, 0.0, False), (0.0, fy, GUARD + cy, 0.0, False)]


def clip_face(P, intr, near):
    """P [3,3] -> the clipped polygon as a list of (position [3] float64, tag, error [3]): tag 0..2 names an original vertex, -1 a cut;
    error is the bound of the module docstring on the float32 position of a cut.  The face's winding is kept."""
    poly = [(np.asarray(P[k], dtype=np.float64), k, np.zeros(3)) for k in range(3)]
    for a, b, c, d0, strict in _planes(intr, near):
        n = len(poly)
        dist = [a * v[0][0] + b * v[0][1] + c * v[0][2] + d0 for v in poly]
        inside = [(d > 0.0) if strict else (d >= 0.0) for d in dist]
        out = []
        for i in range(n):
            j = (i + 1) % n
            if inside[i]:
                out.append(poly[i])
            if inside[i] != inside[j]:
                s, o = (i, j) if inside[i] else (j, i)
                t = dist[s] / (dist[s] - dist[o])
                C = poly[s][0] + t * (poly[o][0] - poly[s][0])
                err = (1.0 - t) * poly[s][2] + t * poly[o][2] + EPS * (1.5 * np.abs(C) + 0.5 * np.abs(C - poly[s][0]))
                out.append((C, -1, err))
        poly = out
        if len(poly) < 3:
            return []
    return poly


def polygon_area(poly):
    """float64 area of a planar polygon given as a list of positions"""
    total = np.zeros(3)
    for i in range(len(poly)):
        total += np.cross(poly[i], poly[(i + 1) % len(poly)])
    return 0.5 * float(np.linalg.norm(total))


def area_by_enumeration(P, intr, near):
    """The area of face n half-spaces another way: in the face's barycentric plane (u, v), where every clip plane is a line, the region
    is the convex hull of the pairwise intersections of the eight lines (three sides, five planes) that satisfy every constraint."""
    P = np.asarray(P, dtype=np.float64)
    lines = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, -1.0, 1.0)]                    # u >= 0, v >= 0, 1 - u - v >= 0
    for a, b, c, d0, _ in _planes(intr, near):
        d = [a * p[0] + b * p[1] + c * p[2] + d0 for p in P]
        lines.append((d[1] - d[0], d[2] - d[0], d[0]))
    scale = [max(abs(l[0]), abs(l[1]), abs(l[2]), 1e-300) for l in lines]
    pts = []
    for i in range(len(lines)):
        for j in range(i + 1, len(lines)):
            (a1, b1, c1), (a2, b2, c2) = lines[i], lines[j]
            det = a1 * b2 - a2 * b1
            if abs(det) <= 1e-14 * scale[i] * scale[j]:
                continue
            u, v = (b1 * c2 - b2 * c1) / det, (a2 * c1 - a1 * c2) / det
            if all(l[0] * u + l[1] * v + l[2] >= -1e-9 * s for l, s in zip(lines, scale)):
                pts.append((u, v))
    if len(pts) < 3:
        return 0.0
    pts = np.unique(np.round(np.asarray(pts), 12), axis=0)
    if pts.shape[0] < 3:
        return 0.0
    centre = pts.mean(0)
    order = np.argsort(np.arctan2(pts[:, 1] - centre[1], pts[:, 0] - centre[0]))
    q = pts[order]
    shoelace = 0.5 * abs(float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1])))
    return shoelace * float(np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])))


# ------------------------------------------------------------------------------------------------ the expanded mesh
def expand(vc, faces, intr, near):
    """-> dict(kind [F]; polys {f: clip_face(f)}; v [V2,3] float32: vc followed by the cuts; f [F2,3]; sub2face [F2]; ev [V2]: e_v of the
    module docstring in px, 0 for an original vertex).  Dropped faces are left out; non-crossing faces are kept as they are."""
    vc = np.asarray(vc, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    kind = classify(vc, faces, near)
    verts, ev, sub, sub2face, polys = [v for v in vc], [0.0] * vc.shape[0], [], [], {}
    for f, t in enumerate(faces):
        if kind[f] == 1:
            sub.append(tuple(int(i) for i in t))
            sub2face.append(f)
        if kind[f] != 2:
            continue
        poly = clip_face(vc[t].astype(np.float64), intr, near)
        polys[f] = poly
        ids = []
        for C, tag, err in poly:
            if tag >= 0:
                ids.append(int(t[tag]))
                continue
            ids.append(len(verts))
            verts.append(C.astype(np.float32))
            ev.append(_poly_ev((C, tag, err), intr))
        for k in range(1, len(ids) - 1):
            sub.append((ids[0], ids[k], ids[k + 1]))
            sub2face.append(f)
    return dict(kind=kind, polys=polys, v=np.asarray(verts, dtype=np.float32).reshape(-1, 3),
                f=np.asarray(sub, dtype=np.int64).reshape(-1, 3), sub2face=np.asarray(sub2face, dtype=np.int64), ev=np.asarray(ev))


def _on_screen_range(a, b, H, W):
    """Liang-Barsky: the parameter range [s0, s1] of the segment a -> b inside the image grown by one pixel, or None"""
    s0, s1 = 0.0, 1.0
    for p, lo, hi in ((0, -1.0, W + 1.0), (1, -1.0, H + 1.0)):
        d = b[p] - a[p]
        if d == 0.0:
            if a[p] < lo or a[p] > hi:
                return None
            continue
        t0, t1 = (lo - a[p]) / d, (hi - a[p]) / d
        s0, s1 = max(s0, min(t0, t1)), min(s1, max(t0, t1))
        if s0 > s1:
            return None
    return s0, s1


def face_values(P, intr):
    """b0, b1, depth [H,W] float64 of the plane through P [3,3] along every pixel's ray (the ray / plane definition)"""
    fx, fy, cx, cy, H, W = intr
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack(((gx - cx) / fx, (gy - cy) / fy, np.ones_like(gx)), -1)
    P = np.asarray(P, dtype=np.float64)
    w = [(d * np.cross(P[(i + 1) % 3], P[(i + 2) % 3])).sum(-1) for i in range(3)]
    total = (w[0] + w[1]) + w[2]
    det = float(np.dot(P[0], np.cross(P[1], P[2])))
    with np.errstate(divide="ignore", invalid="ignore"):
        return w[0] / total, w[1] / total, det / total


def rasterize(vc, faces, intr, near=1e-2, cull="none"):
    """meshraster_ref.rasterize's result for `near_clip=True` (module docstring), with the faces mapped back, and
      crossing [H,W]     the winner is a crossing face
      kind [F], polys    classification and clipped polygons (expand)
      interior [H,W]     the centre lies in the eroded interior (TOL, or the wider band of its edges) of a crossing face's clipped polygon
                         that is not culled: no rasterizer may leave such a pixel empty, whatever the fan's diagonals are
      widened            number of sub-triangle edges with a band wider than TOL"""
    fx, fy, cx, cy, H, W = intr
    vc = np.asarray(vc, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ex = expand(vc, faces, intr, near)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):           # (vertices at Z = 0 that no kept face uses)
        res = ref.rasterize(ex["v"], ex["f"], intr, near=0.5 * float(np.float32(near)), cull=cull)
    s2f = ex["sub2face"]
    sub_face = res["face"]
    hit = sub_face >= 0
    face = np.where(hit, s2f[np.maximum(sub_face, 0)], -1)
    crossing = hit & (ex["kind"][np.maximum(face, 0)] == 2)
    b0, b1, depth = res["b0"].copy(), res["b1"].copy(), res["depth"].copy()
    for f in np.unique(face[crossing]):
        m = face == f
        v0, v1, vd = face_values(vc[faces[f]], intr)
        b0[m], b1[m], depth[m] = v0[m], v1[m], vd[m]
    fragile = res["fragile"].copy()
    empty_ok = res["empty_ok"].copy()
    cand_pix, cand_face = [res["cand_pix"]], [s2f[res["cand_face"]] if res["cand_face"].size else res["cand_face"]]
    # the wider band of the edges that end far off the screen
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xs, ys, _ = ref.project(ex["v"], intr)
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    widened = 0
    for k in np.flatnonzero(ex["kind"][s2f] == 2):
        t = ex["f"][k]
        for i in range(3):
            ia, ib = int(t[i]), int(t[(i + 1) % 3])
            ea, eb = ex["ev"][ia], ex["ev"][ib]
            if max(ea, eb) <= WIDEN_FROM:
                continue
            a, b = (xs[ia], ys[ia]), (xs[ib], ys[ib])
            rng = _on_screen_range(a, b, H, W)
            if rng is None:
                continue
            d_e = max((1 - s) * ea + s * eb for s in rng)
            if d_e <= WIDEN_FROM:
                continue
            widened += 1
            dx, dy = b[0] - a[0], b[1] - a[1]
            length = math.hypot(dx, dy)
            dist = np.abs(dx * (gy - a[1]) - dy * (gx - a[0])) / length
            s = (dx * (gx - a[0]) + dy * (gy - a[1])) / (length * length)
            pad = (TOL + d_e) / length
            band = (dist < TOL + d_e) & (s > -pad) & (s < 1 + pad)
            fragile |= band
            empty_ok |= band
            pix = np.flatnonzero(band.ravel())
            cand_pix.append(pix)
            cand_face.append(np.full(pix.shape, s2f[k], dtype=np.int64))
    # the eroded interior of the clipped polygons
    fx32, fy32, cx32, cy32 = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    interior = np.zeros((H, W), dtype=bool)
    for f, poly in ex["polys"].items():
        if len(poly) < 3:
            continue
        px = [fx32 * C[0] / C[2] + cx32 for C, _, _ in poly]                       # screen positions of the float64 polygon
        py = [fy32 * C[1] / C[2] + cy32 for C, _, _ in poly]
        area = sum(px[i] * py[(i + 1) % len(poly)] - px[(i + 1) % len(poly)] * py[i] for i in range(len(poly)))
        if area == 0.0 or (cull == "back" and area > 0):
            continue
        sgn = 1.0 if area > 0 else -1.0
        dmin = np.full((H, W), np.inf)
        for i in range(len(poly)):
            j = (i + 1) % len(poly)
            dx, dy = px[j] - px[i], py[j] - py[i]
            length = math.hypot(dx, dy)
            if length == 0.0:
                continue
            # the error of an outline edge's line on the screen: its endpoints' e_v over the part that runs through the image
            ea = _poly_ev(poly[i], intr)
            eb = _poly_ev(poly[j], intr)
            rng = _on_screen_range((px[i], py[i]), (px[j], py[j]), H, W)
            d_e = 0.0 if rng is None else max((1 - s) * ea + s * eb for s in rng)
            dist = sgn * (dx * (gy - py[i]) - dy * (gx - px[i])) / length
            dmin = np.minimum(dmin, dist - (TOL + d_e))
        interior |= dmin >= 0.0
    shape = (H, W)
    valid = np.all((faces >= 0) & (faces < vc.shape[0]), axis=1)
    inside_count = np.where(valid, (vc[np.where(valid[:, None], faces, 0)][:, :, 2] > np.float32(near)).sum(1), 0)
    return dict(inside_count=inside_count, face=face, b0=np.where(hit, b0, 0.0), b1=np.where(hit, b1, 0.0), depth=np.where(hit, depth, 0.0), fragile=fragile,
                empty_ok=empty_ok, cand_pix=np.concatenate(cand_pix), cand_face=np.concatenate(cand_face), crossing=crossing,
                kind=ex["kind"], polys=ex["polys"], interior=interior.reshape(shape), widened=widened, expanded=ex)


def _poly_ev(vertex, intr):
    """e_v in px of one polygon vertex (position, tag, error)"""
    C, tag, err = vertex
    if tag >= 0:
        return 0.0
    fx, fy = float(np.float32(intr[0])), float(np.float32(intr[1]))
    X, Y, Z = C
    return (fx * (err[0] / Z + abs(X) * err[2] / (Z * Z)) + 2 * EPS * abs(fx * X / Z) +
            fy * (err[1] / Z + abs(Y) * err[2] / (Z * Z)) + 2 * EPS * abs(fy * Y / Z))


def crossing_stats(res):
    """-> dict(seen: crossing faces that win at least one pixel, one_inside / two_inside: how many of them have that many vertices
    inside, pixel_share: share of the pixels on crossing faces, max_vertices: the largest clipped polygon among them)"""
    seen = np.unique(res["face"][res["crossing"]])
    # (a vertex inside the near plane can still be cut away by the guard band: the kinds are counted by the near plane alone)
    return dict(seen=len(seen), one_inside=sum(1 for f in seen if res["inside_count"][f] == 1),
                two_inside=sum(1 for f in seen if res["inside_count"][f] == 2), pixel_share=float(res["crossing"].mean()),
                max_vertices=max((len(res["polys"][f]) for f in seen), default=0))


# ------------------------------------------------------------------------------------------------ differentiable values (torch, float64)
def values_torch(p, hit, intr):
    """b0, b1, depth [H,W] (zeros where not hit) of the ray / plane definition as differentiable float64 functions of the per-pixel
    vertex copies p [H,W,3,3] (meshraster_ref.gather_rows): the values of a crossing face"""
    fx, fy, cx, cy, H, W = intr
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    d = torch.stack(((gx - cx) / fx, (gy - cy) / fy, torch.ones_like(gx)), -1)
    w = torch.stack([(d * torch.cross(p[..., (i + 1) % 3, :], p[..., (i + 2) % 3, :], dim=-1)).sum(-1) for i in range(3)], -1)
    det = (p[..., 0, :] * torch.cross(p[..., 1, :], p[..., 2, :], dim=-1)).sum(-1)
    total = torch.where(hit, w.sum(-1), torch.ones((), dtype=torch.float64))
    zero = torch.zeros((), dtype=torch.float64)
    return (torch.where(hit, w[..., 0] / total, zero), torch.where(hit, w[..., 1] / total, zero), torch.where(hit, det / total, zero))


# ------------------------------------------------------------------------------------------------ scenes
EYE = (0.0, 0.0, 0.5)
TARGET = (0.0, -0.5, -0.5)
FOV = 60.0
NEAR = 0.1


def _floor(cells, y, half, seed):
    """a jittered grid of cells x cells quads (two triangles each, both diagonals) on the plane y, x in [-half, half], rows 3 half / cells
    apart in z with one row boundary at z = 0.47, two thirds of the rows in front of it: the floor runs under the eye and behind it,
    and the row in front of that boundary crosses the near plane (which meets the floor near z = 0.45) inside the image"""
    rng = np.random.RandomState(seed)
    n = cells + 1
    step = 2.0 * half / cells
    gx, gz = np.meshgrid(np.linspace(-half, half, n), 0.47 + (np.arange(n) - (2 * cells) // 3) * (3.0 * half / cells), indexing="xy")
    v = np.stack((gx, np.full_like(gx, y), gz), -1).reshape(-1, 3)
    v[:, 0] += rng.uniform(-0.2, 0.2, v.shape[0]) * step
    v[:, 2] += rng.uniform(-0.2, 0.2, v.shape[0]) * step * 1.25
    v[:, 1] += rng.uniform(-0.01, 0.01, v.shape[0])
    at = lambda i, j: j * n + i
    f = []
    for j in range(cells):
        for i in range(cells):
            a, b, c, d = at(i, j), at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)
            f += [(a, d, b), (a, c, d)] if (i + j) % 2 else [(a, c, b), (b, c, d)]       # wound to face up (+y)
    return v.astype(np.float32), np.asarray(f, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def scene(name):
    """The near_clip scenes: 64 x 64 (or 37 x 53) at FOV 60 degrees, the eye at EYE looking at TARGET, near 0.1, over
      'floor16', 'floor32'   a jittered floor grid of 16 x 16 / 32 x 32 cells at y = -0.12 that runs under and behind the eye, and an
                             8 x 16 UV sphere of radius 0.15 standing on it in view (non-crossing faces);
      'floor16_37x53'        'floor16' on a 37 x 53 image;
      'guard'                12 x 12 cells, the sphere, and two triangles with corners at +-40 units, 0.2 below the floor: their clipped
                             polygons reach the guard band.
    -> dict(vw, vc float32, faces int64, intr, c2w, vm, near)"""
    size = (37, 53) if name.endswith("37x53") else (64, 64)
    cells, half = {"floor16": (16, 0.5), "floor32": (32, 1.0), "floor16_37x53": (16, 0.5), "guard": (12, 0.375)}[name]
    fv, ff = _floor(cells, -0.12, half, 7 + cells)
    sv, sf = ref.uv_sphere(8, 16, 0.15)
    sv = sv + np.array([0.1, 0.04, -0.6], dtype=np.float32)
    parts_v, parts_f = [fv, sv], [ff, sf + fv.shape[0]]
    if name == "guard":
        big = np.array([[-40.0, -0.32, -40.0], [40.0, -0.33, -40.5], [40.5, -0.31, 40.0], [-40.0, -0.3, 39.0]], dtype=np.float32)
        base = fv.shape[0] + sv.shape[0]
        parts_v.append(big)
        parts_f.append(np.array([[base, base + 2, base + 1], [base, base + 3, base + 2]], dtype=np.int64))
    vw = np.concatenate(parts_v, 0)
    faces = np.concatenate(parts_f, 0)
    c2w, vm = ref.lookat_view(EYE, TARGET)
    vc = (vw.astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]).astype(np.float32)
    H, W = size
    fl = 0.5 * W / math.tan(math.radians(FOV) * 0.5)
    return dict(vw=vw, vc=vc, faces=faces, intr=(fl, fl, 0.5 * W, 0.5 * H, H, W), c2w=c2w, vm=vm, near=NEAR)


SCENES = ("floor16", "floor32", "floor16_37x53", "guard")
FRAGILE_CAP = 0.05


@functools.lru_cache(maxsize=None)
def scene_result(name, cull="none"):
    sc = scene(name)
    return rasterize(sc["vc"], sc["faces"], sc["intr"], near=sc["near"], cull=cull)


# ------------------------------------------------------------------------------------------------ antialias decisions
class _CrossingFace:
    """the snapped side of a crossing face: whether a sub-triangle survives, and per half-edge i the snapped position of the polygon
    vertex that follows the original vertex i + 2 (None when the guard band removed that vertex)"""

    def __init__(self, poly, intr, cull):
        fx, fy, cx, cy = (float(np.float32(a)) for a in intr[:4])
        self.kept, self.robust, self.follower, self.follower_ev = False, True, [None] * 3, [0.0] * 3
        if len(poly) < 3:
            return
        pos = np.asarray([np.asarray(C, dtype=np.float64).astype(np.float32).astype(np.float64) if tag < 0 else C for C, tag, _ in poly])
        xs, ys = fx * pos[:, 0] / pos[:, 2] + cx, fy * pos[:, 1] / pos[:, 2] + cy
        if not np.all(np.abs(np.concatenate((xs, ys))) * SNAP <= ref.RANGE):
            self.robust = False
            return
        X, Y = np.rint(xs * SNAP).astype(np.int64), np.rint(ys * SNAP).astype(np.int64)
        strong, weak = False, False
        for k in range(1, len(poly) - 1):
            area = int((X[k] - X[0]) * (Y[k + 1] - Y[0]) - (Y[k] - Y[0]) * (X[k + 1] - X[0]))
            if area != 0 and not (cull == "back" and area > 0):
                self.kept = True
            if abs(area) > SNAP * SNAP:                                     # half a pixel of area: no rounding removes or turns it
                strong = strong or not (cull == "back" and area > 0)
            else:
                weak = True
        self.robust = strong or not weak                                    # else a sliver alone decides whether the face counts
        tags = [tag for _, tag, _ in poly]
        for i in range(3):
            want = (i + 2) % 3
            if want in tags:
                m = (tags.index(want) + 1) % len(poly)
                self.follower[i] = (int(X[m]), int(Y[m]), float(xs[m]), float(ys[m]))
                self.follower_ev[i] = _poly_ev(poly[m], intr)


def aa_decisions(rast, vc, faces, intr, res, cull="none", near=1e-2):
    """The antialias decisions with near_clip, on the device's own `rast` [H,W,4] (numpy float32); `res`: rasterize() of the same scene.
    -> dict(code [H,W,2]: 1 + exit edge + 16 (the foreground is the pair's second pixel) of the pairs (p, p + (1,0)) and (p, p + (0,1)),
    0 where the pair blends nothing -- the kernel's debug code without its receiving-pixel bits 4 and 8; fragile [H,W,2];
    crossing_fg [H,W,2]: the foreground face is a crossing face; crossing_blocks [H,W,2]: a crossing neighbour lies on the far side, so
    the edge is not a silhouette).  The foreground, exit edge and silhouette rules are those of tests/meshaa_ref.py."""
    fx, fy, cx, cy, H, W = intr
    rast = np.asarray(rast)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vc, dtype=np.float32)
    V, F = vc.shape[0], faces.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xs, ys, zs = ref.project(vc, intr)
    topo = aaref.topology(faces)
    kind, polys = res["kind"], res["polys"]
    plain, cross = {}, {}

    def plain_face(f):
        if f not in plain:
            plain[f] = aaref._Face([int(v) for v in faces[f]], xs, ys, zs, V, near, cull)
        return plain[f]

    def crossing_face(f):
        if f not in cross:
            cross[f] = _CrossingFace(polys[f], intr, cull)
        return cross[f]

    ids = rast[..., 3]
    fid = np.where((ids >= 1) & (ids <= 2.0 ** 24), ids, 0).astype(np.int64) - 1
    fid[fid >= F] = -1
    depth = rast[..., 2]
    frag = res["fragile"]
    out = {k: np.zeros((H, W, 2), dtype=(np.int64 if k == "code" else bool)) for k in ("code", "fragile", "crossing_fg", "crossing_blocks")}
    for py in range(H):
        for px in range(W):
            for axis, (qx, qy) in enumerate(((px + 1, py), (px, py + 1))):
                if qx >= W or qy >= H or ids[py, px] == ids[qy, qx]:
                    continue
                fragile = bool(frag[py, px] or frag[qy, qx])
                fp, fq = int(fid[py, px]), int(fid[qy, qx])
                code = 0
                if fp >= 0 or fq >= 0:
                    if fq < 0:
                        first = True
                    elif fp < 0:
                        first = False
                    elif depth[py, px] != depth[qy, qx]:
                        first = bool(depth[py, px] < depth[qy, qx])
                    else:
                        first = fp < fq
                    (ax, ay), (bx, by) = ((px, py), (qx, qy)) if first else ((qx, qy), (px, py))
                    f = fp if first else fq
                    if kind[f] == 2:
                        out["crossing_fg"][py, px, axis] = True
                    elif kind[f] == 1 and plain_face(f).kept:
                        T = plain_face(f)
                        sep = []
                        for i in range(3):
                            ea, bias = T.edge(i, ax, ay)
                            eb, _ = T.edge(i, bx, by)
                            if ea + bias >= 0 and eb + bias < 0:
                                sep.append((i, ea, ea - eb))
                        if sep:
                            best = sep[0]
                            for c in sep[1:]:
                                if c[1] * best[2] < best[1] * c[2]:
                                    best = c
                            edge = best[0]
                            fractions = sorted(n / d for _, n, d in sep)
                            fragile = fragile or (len(fractions) > 1 and fractions[1] - fractions[0] < TOL)
                            e1, e2 = (edge + 1) % 3, (edge + 2) % 3
                            x1, y1 = T.X[e1], T.Y[e1]
                            dx, dy = T.X[e2] - x1, T.Y[e2] - y1
                            side = dx * (T.Y[edge] - y1) - dy * (T.X[edge] - x1)
                            v1, v2, vo = int(faces[f][e1]), int(faces[f][e2]), int(faces[f][edge])
                            u1, u2 = (xs[v1], ys[v1]), (xs[v2], ys[v2])
                            if aaref._line_distance((xs[vo], ys[vo]), u1, u2) < TOL:
                                fragile = True
                            silhouette = True
                            for f2, i2 in topo[3 * f + edge]:
                                if kind[f2] == 2:
                                    T2 = crossing_face(f2)
                                    if not T2.robust:
                                        fragile = True
                                    if not T2.kept or T2.follower[i2] is None:
                                        continue
                                    X2, Y2, x2, y2 = T2.follower[i2]
                                    if aaref._line_distance((x2, y2), u1, u2) < TOL + T2.follower_ev[i2]:
                                        fragile = True
                                    if side * (dx * (Y2 - y1) - dy * (X2 - x1)) < 0:
                                        silhouette = False
                                        out["crossing_blocks"][py, px, axis] = True
                                    continue
                                if kind[f2] != 1:
                                    continue
                                T2 = plain_face(f2)
                                o2 = int(faces[f2][i2])
                                if np.isfinite(xs[o2]) and aaref._line_distance((xs[o2], ys[o2]), u1, u2) < TOL:
                                    fragile = True
                                if T2.kept and side * (dx * (T2.Y[i2] - y1) - dy * (T2.X[i2] - x1)) < 0:
                                    silhouette = False
                            if silhouette:
                                code = 1 + edge + (0 if first else 16)
                out["code"][py, px, axis] = code
                out["fragile"][py, px, axis] = fragile
    return out
