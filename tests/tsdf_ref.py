"""Float64 numpy restatement of csrc/gs_tsdf.hip, the yardstick of the fusion tests: projective TSDF integration into a dense
volume (Open3D's uniform-volume update: depth scale 1, no colour, unit weight per observation) and marching cubes over the cubes
whose corners are voxel centres, with the numbering include/geosplat_hip.h fixes.  Also the analytic-sphere scene the tests share.

Layout: voxel n = i0 + R0 (i1 + R1 i2); arrays are flat [R0 * R1 * R2].  Pixel j covers [j, j + 1).
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from scripts.make_mc_table import EDGE_AXIS, EDGE_CORNERS, build_table, corner_offset

EPS = 2.0 ** -23
_TABLE = build_table()


def voxel_indices(res: Sequence[int]) -> np.ndarray:
    R0, R1, R2 = res
    n = np.arange(R0 * R1 * R2)
    return np.stack((n % R0, (n // R0) % R1, n // (R0 * R1)), -1)


def voxel_centres(res, origin, voxel_size) -> np.ndarray:
    return np.asarray(origin, np.float64)[None] + (voxel_indices(res) + 0.5) * float(voxel_size)


def integrate(tsdf: np.ndarray, weight: np.ndarray, depth_alpha: Sequence[np.ndarray], viewmats: np.ndarray, Ks: np.ndarray,
              res, origin, voxel_size: float, sdf_trunc: float, alpha_trunc: float = 0.5, depth_trunc: float = 4.0,
              pixel_margin: float = 2.0 ** -10, sdf_margin: float = 8.0):
    """Integrates the views in order into (tsdf, weight) (float64 copies are returned).  Also returns
      fragile [N] bool : for some view u or v lies within pixel_margin of an integer, or sdf + sdf_trunc within
                         sdf_margin * 2^-23 * (|d| + |z|) of 0 -- a float32 evaluation may decide such a voxel differently
      mag [N]          : max over the contributing views of |d| + S, S = sum_j |R_2j| (|origin_j| + |p_j|) + |t_2|, the magnitude
                         the rounding error of d - z scales with (S >= |z|)"""
    tsdf = np.array(tsdf, np.float64).reshape(-1).copy()
    weight = np.array(weight, np.float64).reshape(-1).copy()
    p = voxel_centres(res, origin, voxel_size)
    fragile = np.zeros(p.shape[0], bool)
    mag = np.zeros(p.shape[0])
    for da, vm, K in zip(depth_alpha, viewmats, Ks):
        da = np.asarray(da)
        H, W = da.shape[:2]
        vm, K = np.asarray(vm, np.float64), np.asarray(K, np.float64)
        pc = p @ vm[:3, :3].T + vm[:3, 3]
        z = pc[:, 2]
        front = z > 0
        zs = np.where(front, z, 1.0)
        u = K[0, 0] * pc[:, 0] / zs + K[0, 2]
        v = K[1, 1] * pc[:, 1] / zs + K[1, 2]
        near_int = (np.abs(u - np.rint(u)) < pixel_margin) | (np.abs(v - np.rint(v)) < pixel_margin)
        fragile |= front & near_int & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
        ok = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        iu = np.clip(np.floor(u), 0, W - 1).astype(np.int64)
        iv = np.clip(np.floor(v), 0, H - 1).astype(np.int64)
        d = da[iv, iu, 0].astype(np.float64)
        a = da[iv, iu, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok &= (a > alpha_trunc) & (d > 0) & (d < depth_trunc)
            d = np.where(ok, d, 0.0)
            sdf = d - z
            fragile |= ok & (np.abs(sdf + sdf_trunc) < sdf_margin * EPS * (np.abs(d) + np.abs(z)))
            ok &= sdf > -sdf_trunc
        val = np.minimum(1.0, sdf / sdf_trunc)
        new = (tsdf * weight + val) / (weight + 1.0)
        tsdf = np.where(ok, new, tsdf)
        weight = np.where(ok, weight + 1.0, weight)
        m = np.abs(d) + (np.abs(p) + np.abs(np.asarray(origin, np.float64))[None]) @ np.abs(vm[2, :3]) + abs(vm[2, 3])
        mag = np.where(ok, np.maximum(mag, m), mag)
    return tsdf, weight, fragile, mag


def tsdf_budget(mag: np.ndarray, weight: np.ndarray, sdf_trunc: float) -> np.ndarray:
    """Bound of |tsdf_fp32 - tsdf_fp64| on a voxel both agree to update (derivation: tests/test_gpu_fusion.py)."""
    return (8.0 * mag / sdf_trunc + 4.0 * weight) * EPS


def extract(tsdf: np.ndarray, weight: np.ndarray, res, origin, voxel_size: float):
    """-> (counts [4] = vertices, triangles, valid cubes, surface cubes; vertices [V,3] float64; faces [F,3] int64).
    A cube is valid iff its eight weights are > 0; a corner is inside iff tsdf < 0; an edge (owned by the voxel at its lower end)
    carries a vertex iff its ends differ in sign and it belongs to a valid cube.  Vertex ids ascend by (owning voxel, axis),
    triangles by (cube, table order)."""
    R0, R1, R2 = res
    t = np.asarray(tsdf).reshape(R2, R1, R0).astype(np.float64)                 # [i2, i1, i0]
    w = np.asarray(weight).reshape(R2, R1, R0)
    with np.errstate(invalid="ignore"):
        inside = t < 0
    C0, C1, C2 = max(R0 - 1, 0), max(R1 - 1, 0), max(R2 - 1, 0)
    valid = np.ones((C2, C1, C0), bool)
    case = np.zeros((C2, C1, C0), np.int64)
    for k in range(8):
        o = corner_offset(k)
        sl = (slice(o[2], o[2] + C2), slice(o[1], o[1] + C1), slice(o[0], o[0] + C0))
        valid &= w[sl] > 0
        case |= inside[sl].astype(np.int64) << k
    surface = valid & (case != 0) & (case != 255)
    # edge flags per owning voxel
    edge = np.zeros((3, R2, R1, R0), bool)
    for c2, c1, c0 in zip(*np.nonzero(surface)):
        cs = case[c2, c1, c0]
        for e, (lo, hi) in enumerate(EDGE_CORNERS):
            if ((cs >> lo) & 1) != ((cs >> hi) & 1):
                o = corner_offset(lo)
                edge[EDGE_AXIS[e], c2 + o[2], c1 + o[1], c0 + o[0]] = True
    flags = edge.reshape(3, -1)                                                  # [axis, n]
    order = flags.T.reshape(-1)                                                  # (n, axis) ascending
    vid = np.cumsum(order) - 1
    vid = np.where(order, vid, -1).reshape(-1, 3)                                # [n, axis]
    n_vert = int(order.sum())
    tf = t.reshape(-1)
    centres = voxel_centres(res, origin, voxel_size)
    verts = np.zeros((n_vert, 3))
    strides = (1, R0, R0 * R1)
    for n, ax in zip(*np.nonzero(vid >= 0)):
        ta, tb = tf[n], tf[n + strides[ax]]
        pos = centres[n].copy()
        pos[ax] += (ta / (ta - tb)) * (centres[n + strides[ax]][ax] - centres[n][ax])
        verts[vid[n, ax]] = pos
    faces = []
    for c2, c1, c0 in zip(*np.nonzero(surface)):                                 # np.nonzero: ascending cube index
        base = c0 + R0 * (c1 + R1 * c2)
        for tri in _TABLE[case[c2, c1, c0]]:
            row = []
            for e in tri:
                o = corner_offset(EDGE_CORNERS[e][0])
                row.append(vid[base + o[0] + R0 * (o[1] + R1 * o[2]), EDGE_AXIS[e]])
            faces.append(row)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    counts = np.array([n_vert, faces.shape[0], int(valid.sum()), int(surface.sum())], np.int64)
    return counts, verts, faces


# ------------------------------------------------------------------------------------------------ the shared analytic scene
def lookat_viewmat(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """world -> camera [4,4], OpenCV convention (x right, y down, z forward)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack((r, d, f))
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = -R @ eye
    return out


def fibonacci_sphere(num: int, radius: float) -> np.ndarray:
    i = np.arange(num) + 0.5
    zc = 1 - 2 * i / num
    phi = i * (np.pi * (3 - np.sqrt(5)))
    rr = np.sqrt(1 - zc * zc)
    return radius * np.stack((rr * np.cos(phi), rr * np.sin(phi), zc), -1)


def pinhole(width: int, height: int, fov_degree: float) -> np.ndarray:
    f = 0.5 * width / np.tan(np.radians(fov_degree) * 0.5)
    return np.array([[f, 0, 0.5 * width], [0, f, 0.5 * height], [0, 0, 1]])


def sphere_depth(viewmat: np.ndarray, K: np.ndarray, width: int, height: int, radius: float, far_hit: bool = False) -> np.ndarray:
    """[H,W,2] float32 (z of the ray hit at the pixel centres, alpha 1; (0, 0) where the ray misses) of the origin-centred sphere.
    far_hit: the exit point (a camera inside the sphere)."""
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    eye = -R.T @ t
    jj, ii = np.meshgrid(np.arange(height) + 0.5, np.arange(width) + 0.5, indexing="ij")
    dirs_c = np.stack(((ii - K[0, 2]) / K[0, 0], (jj - K[1, 2]) / K[1, 1], np.ones_like(ii)), -1)      # z = 1: the ray parameter IS z
    dirs = dirs_c @ R
    a = (dirs * dirs).sum(-1)
    b = 2 * (dirs @ eye)
    c = eye @ eye - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    sq = np.sqrt(np.where(hit, disc, 0.0))
    s = (-b + sq) / (2 * a) if far_hit else (-b - sq) / (2 * a)
    hit &= s > 0
    return np.stack((np.where(hit, s, 0.0), hit.astype(np.float64)), -1).astype(np.float32)


def sphere_scene(num_views: int = 8, size: int = 64, fov_degree: float = 40.0, radius: float = 0.5, cam_radius: float = 3.0):
    """(depth_alpha list of [H,W,2] float32, viewmats [B,4,4] float32, Ks [B,3,3] float32)"""
    K = pinhole(size, size, fov_degree)
    vms = np.stack([lookat_viewmat(e) for e in fibonacci_sphere(num_views, cam_radius)])
    vms32, K32 = vms.astype(np.float32), K.astype(np.float32)
    das = [sphere_depth(vm.astype(np.float64), K32.astype(np.float64), size, size, radius) for vm in vms32]
    return das, vms32, np.repeat(K32[None], num_views, 0)


def half_edges(faces: np.ndarray):
    """Counter of the directed edges of a face list"""
    from collections import Counter
    c = Counter()
    for a, b, d in np.asarray(faces).tolist():
        c[(a, b)] += 1
        c[(b, d)] += 1
        c[(d, a)] += 1
    return c
