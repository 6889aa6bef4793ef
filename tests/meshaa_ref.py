"""Float64 / exact-integer restatement of the mesh antialias pass (geosplatting_amd/meshrender.py `antialias`, csrc/gs_meshaa.hip):
Python integers for the pairs, the foreground, the exit edge and the silhouette test, torch float64 for the weights and the blend, so
that autograd gives the reference gradients.  Test infrastructure; it shares no code with the kernels.

`rast` is an INPUT (the tests hand in the device's own): the rasterizer is not under test here, tests/meshraster_ref.py covers it.

`analyse` returns the blended pairs.  Per pair it also gives
  kappa    1 + |D_par| / |D_perp|, the slope of the exit edge against the pair's axis: an error e in a screen position moves the
           crossing x* by at most kappa e;
  fragile  (TOL = 3/256 px, as in meshraster_ref) one of its two pixels is fragile there, or an opposite vertex deciding the silhouette
           lies within TOL of the edge's line, or the two smallest exit fractions differ by less than TOL;
  code     the decision as the kernel's debug output encodes it: 1 + exit edge + 16 (the foreground is the pair's second pixel); `blend`
           adds 4 (the first pixel receives) or 8 (the second), nothing when the weight is zero.
"""
import numpy as np
import torch

from tests import meshraster_ref as ref

SNAP = ref.SNAP
TOL = ref.TOL


# ------------------------------------------------------------------------------------------------ topology
def topology(faces):
    """dictionary-built: for every half-edge 3 f + i (edge i joins vertices i + 1 and i + 2 of face f) the sorted list of
    (other face, index of its opposite vertex) on the same undirected edge; a half-edge with two equal indices has none"""
    faces = [tuple(int(v) for v in t) for t in np.asarray(faces).reshape(-1, 3)]
    groups = {}
    for f, t in enumerate(faces):
        for i in range(3):
            a, b = t[(i + 1) % 3], t[(i + 2) % 3]
            if a != b:
                groups.setdefault((min(a, b), max(a, b)), []).append((f, i))
    out = []
    for f, t in enumerate(faces):
        for i in range(3):
            a, b = t[(i + 1) % 3], t[(i + 2) % 3]
            out.append(sorted(g for g in groups.get((min(a, b), max(a, b)), []) if g[0] != f) if a != b else [])
    return out


# ------------------------------------------------------------------------------------------------ decisions (integers)
class _Face:
    """the snapped side of one face: kept (not dropped, not culled), integer positions, orientation"""

    def __init__(self, idx, xs, ys, zs, n_vertices, near, cull):
        self.kept = False
        if any(i < 0 or i >= n_vertices for i in idx):
            return
        if not all(np.float32(zs[i]) > np.float32(near) for i in idx):
            return
        sx, sy = [xs[i] * SNAP for i in idx], [ys[i] * SNAP for i in idx]
        if not all(np.isfinite(v) and abs(v) <= ref.RANGE for v in sx + sy):
            return
        self.X, self.Y = [int(np.rint(v)) for v in sx], [int(np.rint(v)) for v in sy]
        X, Y = self.X, self.Y
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if area == 0 or (cull == "back" and area > 0):
            return
        self.sgn = 1 if area > 0 else -1
        self.kept = True

    def edge(self, i, px, py):
        """(E_i at the centre of pixel (px, py), bias_i): positive inside, top-left rule"""
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = self.sgn * (self.X[b] - self.X[a]), self.sgn * (self.Y[b] - self.Y[a])
        e = dx * (SNAP * py + SNAP // 2 - self.Y[a]) - dy * (SNAP * px + SNAP // 2 - self.X[a])
        return e, (0 if (dy < 0 or (dy == 0 and dx > 0)) else -1)


def _line_distance(p, a, b):
    """float64 distance of p from the line through a and b"""
    ex, ey = b[0] - a[0], b[1] - a[1]
    return abs(ex * (p[1] - a[1]) - ey * (p[0] - a[0])) / np.hypot(ex, ey)


def analyse(rast, vc, faces, intr, cull="none", near=1e-2, pixel_fragile=None):
    """rast [H,W,4] float32 (numpy), vc [V,3] float32, faces [F,3] -> dict of arrays over the BLENDED pairs, in raster order of the
    pair's first pixel, horizontal before vertical:
      first, second  pixel indices (second = first + 1 or first + W);  axis 0 horizontal / 1 vertical
      a, b           foreground and other pixel;  s = +1 when a is the first pixel;  face, edge: T and its exit edge
      verts [n,2]    vertex ids of the exit edge's endpoints (vertices edge + 1, edge + 2 of T)
      kappa, fragile, code   (module docstring)
    and 'cand': first, second, axis, fragile, blended of EVERY pair whose face-id channels differ."""
    fx, fy, cx, cy, H, W = intr
    rast = np.asarray(rast)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vc = np.asarray(vc, dtype=np.float32)
    V, F = vc.shape[0], faces.shape[0]
    xs, ys, zs = ref.project(vc, intr)
    topo = topology(faces)
    cache = {}

    def face(f):
        if f not in cache:
            cache[f] = _Face([int(v) for v in faces[f]], xs, ys, zs, V, near, cull)
        return cache[f]

    ids = rast[..., 3]
    fid = np.where((ids >= 1) & (ids <= 2.0 ** 24), ids, 0).astype(np.int64) - 1
    fid[fid >= F] = -1
    depth = rast[..., 2]
    frag = np.zeros((H, W), dtype=bool) if pixel_fragile is None else np.asarray(pixel_fragile)
    out = {k: [] for k in ("first", "second", "axis", "a", "b", "s", "face", "edge", "verts", "kappa", "fragile", "code")}
    cand = {k: [] for k in ("first", "second", "axis", "fragile", "blended")}

    def decide(px, py, qx, qy, axis):
        """-> (the pair's record or None when it blends nothing, fragile)"""
        fragile = bool(frag[py, px] or frag[qy, qx])
        fp, fq = int(fid[py, px]), int(fid[qy, qx])
        if fp < 0 and fq < 0:
            return None, fragile
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
        T = face(f)
        if not T.kept:
            return None, fragile
        # separating edges and their exit fractions, exactly
        sep = []
        for i in range(3):
            ea, bias = T.edge(i, ax, ay)
            eb, _ = T.edge(i, bx, by)
            if ea + bias >= 0 and eb + bias < 0:
                sep.append((i, ea, ea - eb))
        if not sep:
            return None, fragile
        best = sep[0]
        for c in sep[1:]:
            if c[1] * best[2] < best[1] * c[2]:
                best = c
        edge = best[0]
        fractions = sorted(n / d for _, n, d in sep)
        fragile = fragile or (len(fractions) > 1 and fractions[1] - fractions[0] < TOL)
        # silhouette
        e1, e2 = (edge + 1) % 3, (edge + 2) % 3
        x1, y1 = T.X[e1], T.Y[e1]
        dx, dy = T.X[e2] - x1, T.Y[e2] - y1
        side = dx * (T.Y[edge] - y1) - dy * (T.X[edge] - x1)
        v1, v2 = int(faces[f][e1]), int(faces[f][e2])
        u1, u2 = (xs[v1], ys[v1]), (xs[v2], ys[v2])
        vo = int(faces[f][edge])
        if _line_distance((xs[vo], ys[vo]), u1, u2) < TOL:
            fragile = True
        silhouette = True
        for f2, i2 in topo[3 * f + edge]:
            T2 = face(f2)
            o2 = int(faces[f2][i2])
            if 0 <= o2 < V and np.isfinite(xs[o2]) and _line_distance((xs[o2], ys[o2]), u1, u2) < TOL:
                fragile = True
            if not T2.kept:
                continue
            side2 = dx * (T2.Y[i2] - y1) - dy * (T2.X[i2] - x1)
            if side * side2 < 0:
                silhouette = False
        if not silhouette:
            return None, fragile
        ex, ey = u2[0] - u1[0], u2[1] - u1[1]
        par, perp = (ex, ey) if axis == 0 else (ey, ex)
        p, q = py * W + px, qy * W + qx
        return dict(first=p, second=q, axis=axis, a=p if first else q, b=q if first else p, s=1.0 if first else -1.0, face=f, edge=edge,
                    verts=(v1, v2), kappa=1.0 + abs(par) / abs(perp) if perp != 0 else np.inf, code=1 + edge + (0 if first else 16)), fragile

    for py in range(H):
        for px in range(W):
            for axis, (qx, qy) in enumerate(((px + 1, py), (px, py + 1))):
                if qx >= W or qy >= H or ids[py, px] == ids[qy, qx]:
                    continue
                rec, fragile = decide(px, py, qx, qy, axis)
                for k, v in (("first", py * W + px), ("second", qy * W + qx), ("axis", axis), ("fragile", fragile), ("blended", rec is not None)):
                    cand[k].append(v)
                if rec is not None:
                    rec["fragile"] = fragile
                    for k, v in rec.items():
                        out[k].append(v)
    res = {k: np.asarray(v, dtype=(np.float64 if k in ("s", "kappa") else bool if k == "fragile" else np.int64)) for k, v in out.items()}
    res["verts"] = res["verts"].reshape(-1, 2)
    res["n"] = len(out["first"])
    res["shape"] = (H, W)
    # every pair whose face-id channels differ, blended or not, with its fragile flag: what a comparison of decisions has to skip
    res["cand"] = {k: np.asarray(v, dtype=(bool if k in ("fragile", "blended") else np.int64)) for k, v in cand.items()}
    return res


# ------------------------------------------------------------------------------------------------ weights and blend (torch float64)
def blend(pairs, color, pv, intr, pair_colors=None):
    """pairs from `analyse`; color [H,W,C] float64; pv [n,2,3] float64: per-pair copies of the camera-space positions of the exit
    edge's endpoints (vc[pairs['verts']]), so that the gradient with respect to `pv` is every pair's own contribution.
    pair_colors = (ct, co) [n,C]: per-pair copies of the target's and the other pixel's colour, for the same purpose (else gathered).
    -> dict(out [H,W,C], d, w [n], target, other [n] int64 pixel indices, code [n] with the receiving pixel added)"""
    fx, fy, cx, cy, H, W = intr
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    C = color.shape[-1]
    n = pairs["n"]
    if n == 0:
        z = torch.zeros(0, dtype=torch.int64)
        return dict(out=color.clone(), d=torch.zeros(0, dtype=torch.float64), w=torch.zeros(0, dtype=torch.float64), target=z, other=z,
                    code=np.zeros(0, dtype=np.int64))
    a, b = torch.as_tensor(pairs["a"]), torch.as_tensor(pairs["b"])
    horizontal = torch.as_tensor(pairs["axis"] == 0)
    s = torch.as_tensor(pairs["s"])
    pcx = (a % W).double() + 0.5
    pcy = (a // W).double() + 0.5
    qx = fx * pv[..., 0] / pv[..., 2] + cx - pcx[:, None]
    qy = fy * pv[..., 1] / pv[..., 2] + cy - pcy[:, None]
    u = torch.where(horizontal[:, None], qx, qy)
    v = torch.where(horizontal[:, None], qy, qx)
    xstar = (u[:, 0] * v[:, 1] - v[:, 0] * u[:, 1]) / (v[:, 1] - v[:, 0])
    d = torch.clamp(s * xstar, 0.0, 1.0)
    to_b = d.detach() > 0.5
    target, other = torch.where(to_b, b, a), torch.where(to_b, a, b)
    w = torch.where(to_b, d - 0.5, torch.where(d.detach() < 0.5, 0.5 - d, torch.zeros_like(d)))     # d = 0.5 blends nothing
    ct, co = pair_colors if pair_colors is not None else (color.reshape(-1, C)[target], color.reshape(-1, C)[other])
    out = color.reshape(-1, C).index_add(0, target, w[:, None] * (co - ct)).reshape(H, W, C)
    first = torch.as_tensor(pairs["first"])
    recv = torch.where(d.detach() == 0.5, 0, torch.where(target == first, 4, 8))
    return dict(out=out, d=d, w=w, target=target, other=other, code=pairs["code"] + recv.numpy())


def decision_map(pairs, code):
    """int [H,W,2]: the codes of the pairs (p, p + (1,0)) and (p, p + (0,1)) at their first pixel, 0 where nothing blends"""
    H, W = pairs["shape"]
    m = np.zeros((H * W, 2), dtype=np.int64)
    if pairs["n"]:
        m[pairs["first"], pairs["axis"]] = code
    return m.reshape(H, W, 2)


def rast_of(res):
    """a rast [H,W,4] float32 from meshraster_ref.rasterize's result, for the tests that run without a device"""
    hit = res["face"] >= 0
    return np.stack((res["b0"], res["b1"], res["depth"], np.where(hit, res["face"] + 1, 0)), -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ exact-tier scenes
def _at(xy, z):
    """camera-space vertices that project to xy (unit intrinsics) from depth z: exact in float32 for z a power of two"""
    xy = np.asarray(xy, dtype=np.float32)
    return np.concatenate((xy * np.float32(z), np.full((xy.shape[0], 1), z, dtype=np.float32)), 1)


def exact_scenes():
    """name -> (vc [V,3] float32, faces): unit intrinsics (1, 1, 0, 0), vertices at Z = 1 and Z = 2, positions on float32 values whose
    256-fold is computed without rounding, so every snapped integer is the same in float32 and in float64.  The weight has a kink at
    d = 0.5, where the receiving pixel changes: no pair of these scenes comes within 1e-3 of it without sitting on it exactly (with
    dyadic positions, where float32 and float64 both give 0.5), which tests/test_meshaa_cpu.py checks."""
    sc = {}
    sc["square, non-dyadic edges"] = (_at([(10.3, 7.7), (40.6, 9.1), (42.2, 33.3), (8.9, 30.7)], 1.0), [(0, 1, 2), (0, 2, 3)])
    ring = [(6, 5), (19.3, 3.2), (31, 6), (33.7, 17.1), (30, 29), (17.2, 32.4), (5, 28), (3.3, 16.7)]
    sc["fan"] = (_at([(17.4, 16.9)] + ring, 1.0), [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)])
    top = [(4 + 5.3 * k, 6.2 + 0.4 * k) for k in range(6)]
    bot = [(5.1 + 5.3 * k, 17.9 - 0.3 * k) for k in range(6)]
    strip = []
    for k in range(5):
        strip += [(k, 6 + k, 7 + k), (k, 7 + k, k + 1)]
    sc["open strip"] = (_at(top + bot, 1.0), strip)
    sc["two quads, different depths"] = (np.concatenate((_at([(5.2, 4.1), (27.5, 6.3), (26.1, 25.8), (4.4, 24.6)], 1.0),
                                                         _at([(15.7, 14.2), (36.3, 13.1), (35.2, 34.9), (14.6, 33.3)], 2.0)), 0),
                                         [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)])
    sc["coplanar quads, a depth tie"] = (_at([(4, 4), (24, 4), (24, 22), (4, 22), (12.5, 10.25), (33, 11), (32, 30), (13, 29)], 1.0),
                                         [(4, 5, 6), (4, 6, 7), (0, 1, 2), (0, 2, 3)])
    sc["edges through pixel centres"] = (_at([(8.5, 6.5), (30.5, 6.5), (30.5, 28.5), (8.5, 28.5), (3.5, 31.5), (20.5, 48.5), (3.5, 48.5)],
                                             1.0), [(0, 1, 2), (0, 2, 3), (4, 5, 6)])
    return sc


UNIT = (1.0, 1.0, 0.0, 0.0)
