"""Float64 / int64 restatement of the mesh rasterizer's semantics (geosplatting_amd/meshrender.py, csrc/gs_meshraster.hip): numpy for
coverage, the winner and the values, torch float64 where autograd is wanted.  Test infrastructure; it shares no code with the kernels.

`rasterize` returns, per pixel, the winning face, b0, b1 and the view depth, the list of *candidate* (pixel, face) pairs, and a
*fragile* mask.  A float32 evaluation may decide a pixel differently from float64 only where a decision is within rounding of its
threshold.  A pixel is fragile when
  * its centre is within TOL = 3/256 px (float64 distance) of an edge of any triangle whose TOL-dilated interior contains it: snapping
    moves a vertex by up to 0.5/256 px and the fp32 error of xs (about 1e-5 px at |xs| <= 64) can flip a snap by one unit; or
  * the two nearest candidate depths at the pixel differ by less than 2^-16 relative.
A face is a candidate at a pixel when its TOL-dilated interior contains the centre; `empty_ok` marks the pixels where no face's
TOL-eroded interior does, i.e. where a float32 rasterizer may leave the pixel empty.
"""
import math

import numpy as np
import torch

SNAP = 256
TOL = 3.0 / 256.0
DEPTH_GAP = 2.0 ** -16
RANGE = 1 << 22


# ------------------------------------------------------------------------------------------------ meshes and scenes
def uv_sphere(n_lat, n_long, radius=0.5):
    """Outward-wound UV sphere: n_lat bands, n_long sectors -> (vertices [V,3] float32, faces [F,3] int64), poles along z."""
    v = [(0.0, 0.0, radius)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_long):
            ph = 2.0 * math.pi * j / n_long
            v.append((radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)))
    v.append((0.0, 0.0, -radius))
    south = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * n_long + (j % n_long)
    f = []
    for j in range(n_long):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_long):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            f.append((a, c, d))
            f.append((a, d, b))
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f, dtype=np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    flip = (n * v[f].mean(1)).sum(-1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v.astype(np.float32), f


def lookat_view(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(c2w [3,4] OpenGL, world->camera [4,4] OpenCV) in float64, the conventions of geosplatting_amd.cameras"""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    fwd = target - eye
    right = np.cross(fwd, up)
    up2 = np.cross(right, fwd)
    R = np.stack((right, up2, -fwd), axis=-1)
    R = R / np.linalg.norm(R, axis=0, keepdims=True)
    c2w = np.concatenate((R, eye[:, None]), axis=1)
    Rcv = np.concatenate((R[:, :1], -R[:, 1:]), axis=1)
    vm = np.eye(4)
    vm[:3, :3] = Rcv.T
    vm[:3, 3] = -Rcv.T @ eye
    return c2w, vm


EYE = (0.3, -0.2, 2.0)
SIZE = 64
FOV = 40.0


def scene(n_lat, n_long, size=SIZE):
    """The test scene: a UV sphere of radius 0.5 at the origin, one background triangle larger than the image at z ~ -0.8 (the
    wave-per-triangle path) and a two-triangle quad that cuts through the sphere (depth intersections), seen from EYE at FOV degrees.
    -> dict(vw world vertices f32, vc camera-space vertices f32, faces int64, intr (fx, fy, cx, cy, H, W), c2w, n_sphere_faces)"""
    sv, sf = uv_sphere(n_lat, n_long, 0.5)
    bg = np.array([[-6.0, -4.0, -0.8], [6.0, -4.1, -0.75], [0.1, 7.0, -0.85]], dtype=np.float32)
    quad = np.array([[-0.9, -0.62, -0.35], [0.85, -0.55, -0.3], [0.8, 0.66, 0.4], [-0.88, 0.6, 0.35]], dtype=np.float32)
    nv = sv.shape[0]
    vw = np.concatenate((sv, bg, quad), 0)
    faces = np.concatenate((sf, np.array([[nv, nv + 1, nv + 2], [nv + 3, nv + 4, nv + 5], [nv + 3, nv + 5, nv + 6]], dtype=np.int64)), 0)
    c2w, vm = lookat_view(EYE)
    vc = (vw.astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]).astype(np.float32)
    f = 0.5 * size / math.tan(math.radians(FOV) * 0.5)
    return dict(vw=vw, vc=vc, faces=faces, intr=(f, f, 0.5 * size, 0.5 * size, size, size), c2w=c2w, vm=vm, n_sphere_faces=sf.shape[0])


# ------------------------------------------------------------------------------------------------ the rasterizer
def project(vc, intr):
    """float64 screen positions of float32 camera-space vertices"""
    fx, fy, cx, cy = (float(np.float32(a)) for a in intr[:4])
    v = np.asarray(vc, dtype=np.float32).astype(np.float64)
    return fx * v[:, 0] / v[:, 2] + cx, fy * v[:, 1] / v[:, 2] + cy, v[:, 2]


def _values(qx, qy, z):
    """qx, qy [3, n] positions relative to the pixel centres, z [3] -> b0, b1, depth (float64)"""
    e0 = qx[1] * qy[2] - qy[1] * qx[2]
    e1 = qx[2] * qy[0] - qy[2] * qx[0]
    e2 = qx[0] * qy[1] - qy[0] * qx[1]
    w0, w1, w2 = e0 / z[0], e1 / z[1], e2 / z[2]
    N = (w0 + w1) + w2
    return w0 / N, w1 / N, ((e0 + e1) + e2) / N


def rasterize(vc, faces, intr, near=1e-2, cull="none"):
    fx, fy, cx, cy, H, W = intr
    xs, ys, zs = project(vc, intr)
    faces = np.asarray(faces, dtype=np.int64)
    X = np.rint(xs * SNAP)
    Y = np.rint(ys * SNAP)
    P = H * W
    best_d = np.full(P, np.inf)                      # winner: smallest float32 depth, then the lower face index
    best_d32 = np.full(P, np.inf, dtype=np.float32)
    best_f = np.full(P, -1, dtype=np.int64)
    best_b0 = np.zeros(P)
    best_b1 = np.zeros(P)
    near1 = np.full(P, np.inf)                       # the two smallest candidate depths (float64), any order of arrival
    near2 = np.full(P, np.inf)
    fragile = np.zeros(P, dtype=bool)
    eroded_any = np.zeros(P, dtype=bool)
    cand_pix, cand_face = [], []
    dropped = np.zeros(faces.shape[0], dtype=bool)
    for f, (i0, i1, i2) in enumerate(faces):
        idx = (i0, i1, i2)
        z = zs[list(idx)]
        if not np.all(np.float32(z) > np.float32(near)):
            dropped[f] = True
            continue
        tx, ty = X[list(idx)], Y[list(idx)]
        if not (np.all(np.isfinite(tx)) and np.all(np.isfinite(ty)) and np.all(np.abs(tx) <= RANGE) and np.all(np.abs(ty) <= RANGE)):
            dropped[f] = True
            continue
        ix = [int(t) for t in tx]
        iy = [int(t) for t in ty]
        area = (ix[1] - ix[0]) * (iy[2] - iy[0]) - (iy[1] - iy[0]) * (ix[2] - ix[0])
        if area == 0 or (cull == "back" and area > 0):
            dropped[f] = True
            continue
        ux, uy = xs[list(idx)], ys[list(idx)]
        x0 = max(int(math.floor(ux.min() - 0.5 - 2 * TOL)), 0)
        x1 = min(int(math.ceil(ux.max() - 0.5 + 2 * TOL)), W - 1)
        y0 = max(int(math.floor(uy.min() - 0.5 - 2 * TOL)), 0)
        y1 = min(int(math.ceil(uy.max() - 0.5 + 2 * TOL)), H - 1)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        px, py = px.ravel(), py.ravel()
        pix = py * W + px
        # integer coverage with the top-left rule
        sx, sy = SNAP * px + SNAP // 2, SNAP * py + SNAP // 2
        inside = np.ones(px.shape, dtype=bool)
        sgn = 1 if area > 0 else -1
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            dx, dy = sgn * (ix[b] - ix[a]), sgn * (iy[b] - iy[a])
            e = dx * (sy - iy[a]) - dy * (sx - ix[a])                   # int64: |d| < 2^24, |s - v| < 2^24
            top_left = dy < 0 or (dy == 0 and dx > 0)
            inside &= (e > 0) | ((e == 0) & top_left)
        # float64 signed distances to the unsnapped edges, positive inside
        qx = ux[:, None] - (px + 0.5)[None, :]
        qy = uy[:, None] - (py + 0.5)[None, :]
        area_f = (ux[1] - ux[0]) * (uy[2] - uy[0]) - (uy[1] - uy[0]) * (ux[2] - ux[0])
        s = 1.0 if area_f > 0 else -1.0
        dmin = np.full(px.shape, np.inf)
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            length = math.hypot(ux[b] - ux[a], uy[b] - uy[a])
            e = s * (qx[a] * qy[b] - qy[a] * qx[b])
            dmin = np.minimum(dmin, e / length if length > 0 else np.full(px.shape, -np.inf))
        dilated = dmin > -TOL
        eroded = dmin >= TOL
        fragile[pix[dilated & ~eroded]] = True
        eroded_any[pix[eroded]] = True
        cand = dilated | inside
        b0, b1, d = _values(qx, qy, z)
        cp, cd = pix[cand], d[cand]
        cand_pix.append(cp)
        cand_face.append(np.full(cp.shape, f, dtype=np.int64))
        lower = cd < near1[cp]
        near2[cp] = np.where(lower, near1[cp], np.minimum(near2[cp], cd))
        near1[cp] = np.where(lower, cd, near1[cp])
        ok = inside & np.isfinite(d) & (d > 0)
        wp, wd = pix[ok], d[ok]
        wd32 = wd.astype(np.float32)
        win = wd32 < best_d32[wp]                                       # faces arrive in ascending order: a tie keeps the lower index
        wp = wp[win]
        best_d32[wp] = wd32[win]
        best_d[wp] = wd[win]
        best_f[wp] = f
        best_b0[wp] = b0[ok][win]
        best_b1[wp] = b1[ok][win]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(near2) & ((near2 - near1) < DEPTH_GAP * np.abs(near1))
    fragile |= close
    hit = best_f >= 0
    shape = (H, W)
    return dict(face=best_f.reshape(shape), b0=np.where(hit, best_b0, 0.0).reshape(shape), b1=np.where(hit, best_b1, 0.0).reshape(shape),
                depth=np.where(hit, best_d, 0.0).reshape(shape), fragile=fragile.reshape(shape), empty_ok=(~eroded_any).reshape(shape),
                cand_pix=np.concatenate(cand_pix) if cand_pix else np.zeros(0, dtype=np.int64),
                cand_face=np.concatenate(cand_face) if cand_face else np.zeros(0, dtype=np.int64), dropped=dropped)


def is_candidate(res, face_map):
    """bool [H,W]: the face a rasterizer reports at each pixel (-1: empty) is one of the reference's candidates there"""
    H, W = face_map.shape
    fm = np.asarray(face_map, dtype=np.int64).ravel()
    nf = int(max(res["cand_face"].max(initial=0), fm.max(initial=0))) + 2
    keys = res["cand_pix"] * nf + res["cand_face"]
    ok = np.isin(np.arange(H * W) * nf + fm, keys)
    ok |= (fm < 0) & res["empty_ok"].ravel()
    return ok.reshape(H, W)


# ------------------------------------------------------------------------------------------------ differentiable values (torch, float64)
def gather_rows(table, faces, face_map):
    """Per-pixel copies of the three rows the pixel's face reads: table [V,C] through the face's vertex indices, or [F,3,C] directly.
    -> (rows [H,W,3,C], index [H,W,3] of each row in table.reshape(-1, C), hit [H,W]).  Taking the gradient with respect to `rows`
    gives every pixel's own contribution; `scatter_rows` sums them (or their absolute values) back into the table."""
    fm = torch.as_tensor(np.asarray(face_map), dtype=torch.int64)
    hit = fm >= 0
    fc = fm.clamp_min(0)
    if table.dim() == 3:
        index = 3 * fc[..., None] + torch.arange(3)
    else:
        index = torch.as_tensor(np.asarray(faces), dtype=torch.int64)[fc]
    return table.reshape(-1, table.shape[-1])[index], index, hit


def scatter_rows(grad_rows, index, hit, shape):
    """sum over the covered pixels of grad_rows [H,W,3,C] into a table of `shape`"""
    C = grad_rows.shape[-1]
    out = torch.zeros(int(np.prod(shape)) // C, C, dtype=grad_rows.dtype)
    out.index_add_(0, index[hit].reshape(-1), grad_rows[hit].reshape(-1, C))
    return out.reshape(shape)


def values_torch(p, hit, intr):
    """b0, b1, depth [H,W] (zeros where not hit) as differentiable float64 functions of the per-pixel vertex copies p [H,W,3,3]"""
    fx, fy, cx, cy, H, W = intr
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    z = p[..., 2]
    xs = fx * p[..., 0] / z + cx
    ys = fy * p[..., 1] / z + cy
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    qx, qy = xs - gx[..., None], ys - gy[..., None]
    e = torch.stack((qx[..., 1] * qy[..., 2] - qy[..., 1] * qx[..., 2], qx[..., 2] * qy[..., 0] - qy[..., 2] * qx[..., 0],
                     qx[..., 0] * qy[..., 1] - qy[..., 0] * qx[..., 1]), -1)
    w = e / z
    N = torch.where(hit, w.sum(-1), torch.ones((), dtype=torch.float64))
    zero = torch.zeros((), dtype=torch.float64)
    return (torch.where(hit, w[..., 0] / N, zero), torch.where(hit, w[..., 1] / N, zero), torch.where(hit, e.sum(-1) / N, zero))


def interpolate_torch(rows, b0, b1, hit):
    """sum_i b_i rows_i with b2 = 1 - b0 - b1 (rows [H,W,3,C]); zeros where not hit"""
    b = torch.stack((b0, b1, 1.0 - b0 - b1), -1)[..., None]
    return torch.where(hit[..., None], (b * rows).sum(-2), torch.zeros((), dtype=rows.dtype))
