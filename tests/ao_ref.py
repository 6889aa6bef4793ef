"""float64 restatement of gs_ray_ao (include/geosplat_hip.h, "ambient occlusion"), written from the stated semantics and sharing no code
with csrc/gs_ao.hip; the scenes of tests/test_occlusion_cpu.py and tests/test_gpu_occlusion.py.

    o = fl(pos + fl(n * offset)) and d = fl(e_k - o) in float32, operation for operation: they are the INPUTS of the ray test, as the
        origins and directions are in tests/raytrace_ref.py; everything after them is float64
    c = (n . d) / |d|;  the target counts iff c > 0;  w = max(c, 1e-4)
    hit = tests/raytrace_ref.trace(o, d, tmin = 0, tmax = 1)
    vis = sum(w, counting and not hit) / max(sum(w, counting), 1e-6);  0 for a non-finite row

Error of the fp32 kernel, from its arithmetic (u = 2^-24, one rounding):
    n . d       three products and two additions of values bounded by |n|_2 |d|_2 (Cauchy-Schwarz covers the sum of the absolute
                products): (1 + u)^3 - 1 on that bound, under 4 u |n| |d|
    |d|         three squares, two additions, one square root: relative (3 u + u) / 2 + u, under 3 u
    c           the quotient: 4 u |n| + |c| (3 u + u) <= 8 u |n|  since |c| <= |n|:            EPS_C = 8 u |n|
    w           max(c, 1e-4) is 1-Lipschitz:                                                   the same EPS_C
    a sum of S weights with G lanes: a lane adds ceil(S / G) terms one after the other, then log2(G) butterfly levels follow, so a
                term passes through at most A(S, G) = ceil(S / G) - 1 + log2(G) additions:     A u sum(w) + sum(EPS_C)
    vis         num / max(den, 1e-6) with num <= den:  (d_num + vis d_den) / den + u <= 2 (A u den + S EPS_C) / den + u
`budget(S, G)` evaluates that per point; nothing in it is tuned to what the kernel returns.

FRAGILE.  A sample is fragile when |c| <= C_MARGIN |n| with C_MARGIN = 16 u (twice EPS_C: the kernel may decide c > 0 the other
way), or when its ray is fragile by tests/raytrace_ref.py's own rule (`fragile_any`: on an edge or at an end of the segment).
A point is fragile if any of its S samples is.

The share of fragile points grows with S: a ray that crosses a triangle passes within eps_b of one of its edges with a probability of
about 3 eps_b, and eps_b = 4 (20 L M + 6 L^2) u / |det| is 2e-5 .. 4e-5 for the triangles of the bumpy spheres -- with 130 rays per
point, two crossings each, that alone is over 1 % of the points.  The scenes compared against float64 therefore use the meshes
with FEW LARGE faces (eps_b 5e-6: 'tri3', 'fan'); the bumpy spheres serve the bit-for-bit comparisons, which need no float64."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import raytrace_ref as rr

U24 = 2.0 ** -24
C_MARGIN = 16.0 * U24
FRAGILE_CAP = 0.01
OFFSET = 1e-3
SEED = 8          # chosen, from the restatement alone, so that every scene meets FRAGILE_CAP (67 points allow no fragile one at all)


def origins_dirs(positions, normals, targets, offset):
    """float32, operation for operation -> (o [P,3], d [P,S,3])"""
    o = (positions.astype(np.float32) + normals.astype(np.float32) * np.float32(offset)).astype(np.float32)
    d = (targets.astype(np.float32)[None, :, :] - o[:, None, :]).astype(np.float32)
    return o, d


def evaluate(vertices, faces, positions, normals, targets, offset=OFFSET):
    """-> dict(vis [P], hit [P,S] bool, w [P,S], counts [P,S] bool, den [P], eps_w [P], fragile [P], fragile_ray [P,S])"""
    P, S = positions.shape[0], targets.shape[0]
    o, d = origins_dirs(positions, normals, targets, offset)
    finite = np.isfinite(positions).all(1) & np.isfinite(normals).all(1)
    n64, d64 = normals.astype(np.float64), d.astype(np.float64)
    nlen = np.sqrt((n64 ** 2).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (n64[:, None, :] * d64).sum(-1) / np.sqrt((d64 ** 2).sum(-1))
    counts = (c > 0) & finite[:, None]
    w = np.where(counts, np.maximum(c, 1e-4), 0.0)
    tr = rr.trace(vertices, faces, np.ascontiguousarray(np.broadcast_to(o[:, None, :], (P, S, 3))).reshape(-1, 3), d.reshape(-1, 3), 0.0, 1.0)
    hit = tr["occluded"].reshape(P, S)
    fragile_ray = tr["fragile_any"].reshape(P, S)
    num = np.where(counts & ~hit, w, 0.0).sum(1)
    den = w.sum(1)
    vis = np.where(finite, num / np.maximum(den, 1e-6), 0.0)
    with np.errstate(invalid="ignore"):
        fragile_c = np.abs(c) <= C_MARGIN * nlen[:, None]
    fragile = finite & (fragile_c | fragile_ray).any(1)
    return dict(vis=vis, hit=hit, w=w, counts=counts, den=den, eps_w=8.0 * U24 * np.where(finite, nlen, 0.0), fragile=fragile,
                fragile_ray=fragile_ray, finite=finite)


def additions(S, G):
    return math.ceil(S / G) - 1 + int(math.log2(G))


def budget(res, S, G):
    """per point: the bound on |vis_kernel - vis| derived in the module docstring"""
    den = np.maximum(res["den"], 1e-6)
    return 2.0 * (additions(S, G) * U24 * den + S * res["eps_w"]) / den + U24


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
P_VALUES = (1, 67, 1000)
S_VALUES = (1, 5, 128, 130)
LANES = (1, 16, 64)


def mesh_for(P):
    """the mesh of tests/raytrace_ref.py a point count is traced against in float64 (module docstring, FRAGILE)"""
    return {1: "ico2", 67: "fan", 1000: "tri3"}[P]


@functools.lru_cache(maxsize=None)
def scene(P, S):
    """(vertices, faces, positions [P,3], normals [P,3], targets [S,3]) in float32: a quarter of the points on the faces of the mesh
    with their face normals, the others inside and around it with random normals of random length; targets on the sphere of radius 3; from
    67 points on, one row with a NaN."""
    v, f = rr.mesh(mesh_for(P))
    rng = np.random.default_rng(SEED + 1000 * P + S)
    fi = rng.integers(0, f.shape[0], P)
    b = rng.dirichlet((1.0, 1.0, 1.0), P)
    tri = v.astype(np.float64)[f[fi]]
    pos = (tri * b[:, :, None]).sum(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    free = rng.random(P) < 0.75
    if P == 1:
        free[:] = False
    pos = np.where(free[:, None], rng.normal(size=(P, 3)) * 0.8, pos)
    rn = rng.normal(size=(P, 3))
    nrm = np.where(free[:, None], rn / np.linalg.norm(rn, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (P, 1)), nrm)
    tg = rng.normal(size=(S, 3))
    tg = 3.0 * tg / np.linalg.norm(tg, axis=1, keepdims=True)
    pos, nrm, tg = pos.astype(np.float32), nrm.astype(np.float32), tg.astype(np.float32)
    if P >= 67:
        pos[5, 1] = np.nan
    return v, f, pos, nrm, tg


@functools.lru_cache(maxsize=None)
def expected(P, S):
    """evaluate() of scene(P, S): computed once per process and shared (do not modify)"""
    v, f, pos, nrm, tg = scene(P, S)
    return evaluate(v, f, pos, nrm, tg, OFFSET)


# ---- meshes with known answers ---------------------------------------------------------------------------------------------------
def uv_sphere(radius=0.5, center=(0.0, 0.0, 0.0), rings=12, sectors=24):
    """a closed convex triangulated sphere, outward winding -> (vertices fp32, faces int64)"""
    vs = [[0.0, 0.0, radius]]
    for i in range(1, rings):
        th = math.pi * i / rings
        for j in range(sectors):
            ph = 2.0 * math.pi * j / sectors
            vs.append([radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)])
    vs.append([0.0, 0.0, -radius])
    fs = []
    ring = lambda i, j: 1 + (i - 1) * sectors + (j % sectors)
    for j in range(sectors):
        fs.append([0, ring(1, j), ring(1, j + 1)])
        fs.append([len(vs) - 1, ring(rings - 1, j + 1), ring(rings - 1, j)])
    for i in range(1, rings - 1):
        for j in range(sectors):
            a, b, c, d = ring(i, j), ring(i + 1, j), ring(i + 1, j + 1), ring(i, j + 1)
            fs += [[a, b, c], [a, c, d]]
    return (np.asarray(vs) + np.asarray(center)).astype(np.float32), np.asarray(fs, dtype=np.int64)


def closed_box(half=0.5):
    """the 12 faces of the cube [-half, half]^3 -> (vertices fp32, faces int64)"""
    h = half
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)
    return v, f


def sphere_on_plane(radius=0.5, extent=3.0, cells=12):
    """a sphere of `radius` resting on the plane z = 0 (a grid of cells x cells quads over [-extent, extent]^2, normals +z)
    -> (vertices fp32, faces int64, number of sphere faces): the sphere's faces come first"""
    sv, sf = uv_sphere(radius, (0.0, 0.0, radius + 1e-3))
    xs = np.linspace(-extent, extent, cells + 1)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    pv = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], -1).astype(np.float32)
    pf = []
    for i in range(cells):
        for j in range(cells):
            a, b, c, d = i * (cells + 1) + j, (i + 1) * (cells + 1) + j, (i + 1) * (cells + 1) + j + 1, i * (cells + 1) + j + 1
            pf += [[a, b, c], [a, c, d]]
    pf = np.asarray(pf, dtype=np.int64) + sv.shape[0]
    return np.concatenate([sv, pv]), np.concatenate([sf, pf]), sf.shape[0]


def lookat(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3,4] float32, OpenGL convention (x right, y up, -z forward), as Cameras.from_lookat builds it"""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    fwd = target - eye
    right = np.cross(fwd, up)
    up2 = np.cross(right, fwd)
    R = np.stack([right / np.linalg.norm(right), up2 / np.linalg.norm(up2), -fwd / np.linalg.norm(fwd)], -1)
    return np.concatenate([R, eye[:, None]], -1).astype(np.float32)
