"""TEST INFRASTRUCTURE (CPU only): the nearest-neighbour search and the Chamfer backward of csrc/gs_nn.hip restated in numpy.

  nearest_f32 / k_nearest_f32   the semantics of include/geosplat_hip.h, operation for operation in numpy float32 (every numpy float32
                                operation is one round-to-nearest, and numpy never contracts):
                                    dx = q.x - p.x, dy, dz likewise;  d = (dx*dx + dy*dy) + dz*dz
                                and the answer is the lexicographically smallest (d, index) over the set points whose coordinates are
                                all finite; a non-finite query, or a set without a finite point, gives (+inf, -1); the k-nearest form
                                is padded with (+inf, -1).  The GPU must return these BITS and these indices.
  nearest_f64                   the same search in float64 (what scipy's cKDTree is compared with).
  chamfer_bwd_budget            the backward of the Chamfer pair in float64 at GIVEN indices, with a bound per output element.

The bound.  Element c of row j of grad_xyz1 is a sum of n terms: its own term 2 grad1[j] (a[j,c] - b[i,c]) (i = idx1[j] >= 0) and one
term -2 grad2[j'] (b[j',c] - a[j,c]) for every j' with idx2[j'] = j.  In fp32 a term costs two roundings (the difference and the
product; doubling is exact), the own term is stored and every other term arrives by an fp32 atomic add in an order nobody fixes: n - 1
additions, each of which rounds a partial sum whose magnitude is at most the sum S of the magnitudes of the (rounded) terms.  With
u = 2^-24 the error is therefore at most S ((1 + u)^(n + 1) - 1) for ANY order (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2, with the two roundings of a term folded in), plus n 2^-149 for results in the denormals.  The function
returns exactly that, evaluated in float64 on the float64 terms, times 1 + 2^-20 for having used the exact terms instead of the
rounded ones.  grad_xyz2 likewise.  Rows paired with -1 have no own term.
"""
import numpy as np

U24 = 2.0 ** -24
CHUNK = 256


def cloud(n, seed, lattice=4.0, box=1.0):
    """n points uniform in [-box, box]^3, float32; the first quarter snapped to a 1 / lattice lattice (ties, duplicates)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-box, box, (n, 3)).astype(np.float32)
    q = n // 4
    if lattice:
        p[:q] = (np.round(p[:q] * np.float32(lattice)) / np.float32(lattice)).astype(np.float32)
    return p


def _k_nearest(queries, points, k, dtype):
    q = np.asarray(queries, dtype=dtype).reshape(-1, 3)
    p = np.asarray(points, dtype=dtype).reshape(-1, 3)
    N = q.shape[0]
    d_out = np.full((N, k), np.inf, dtype=dtype)
    i_out = np.full((N, k), -1, dtype=np.int32)
    valid = np.isfinite(p).all(-1)
    orig = np.nonzero(valid)[0].astype(np.int32)              # ascending: a stable order over these columns is the index order
    pv = p[valid]
    rows = np.nonzero(np.isfinite(q).all(-1))[0]
    if pv.shape[0] == 0 or rows.size == 0:
        return d_out, i_out
    kk = min(k, pv.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, rows.size, CHUNK):
            r = rows[lo:lo + CHUNK]
            dx = q[r, None, 0] - pv[None, :, 0]
            dy = q[r, None, 1] - pv[None, :, 1]
            dz = q[r, None, 2] - pv[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == dtype
            if k == 1:
                order = np.argmin(d, axis=1)[:, None]         # the first occurrence of the minimum: the lowest index
            else:
                order = np.argsort(d, axis=1, kind="stable")[:, :kk]
            d_out[r, :kk] = np.take_along_axis(d, order, 1)
            i_out[r, :kk] = orig[order]
    return d_out, i_out


def k_nearest_f32(queries, points, k):
    """(d [N,k] float32, idx [N,k] int32): the k lexicographically smallest (d, index) pairs, ascending, padded with (+inf, -1)"""
    return _k_nearest(queries, points, k, np.float32)


def nearest_f32(queries, points):
    d, i = _k_nearest(queries, points, 1, np.float32)
    return d[:, 0], i[:, 0]


def nearest_f64(queries, points):
    d, i = _k_nearest(queries, points, 1, np.float64)
    return d[:, 0], i[:, 0]


def chamfer_bwd_budget(a, b, idx1, idx2, grad1, grad2):
    """(grad_a, bound_a, grad_b, bound_b), float64 [N,3] each: the gradient of sum(grad1 dist1) + sum(grad2 dist2) at the given
    indices and the error bound of the module docstring for an fp32 evaluation with atomics in any order."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g1, g2 = np.asarray(grad1, np.float64), np.asarray(grad2, np.float64)
    ga, gb = np.zeros_like(a64), np.zeros_like(b64)
    sa, sb = np.zeros_like(a64), np.zeros_like(b64)            # sums of magnitudes
    na, nb = np.zeros(a64.shape[0]), np.zeros(b64.shape[0])     # terms per row

    def one_way(x, y, idx, g, gx, gy, sx, sy, nx, ny):
        j = np.nonzero(np.asarray(idx) >= 0)[0]
        i = np.asarray(idx)[j]
        t = 2.0 * g[j, None] * (x[j] - y[i])
        gx[j] += t
        sx[j] += np.abs(t)
        nx[j] += 1
        np.add.at(gy, i, -t)
        np.add.at(sy, i, np.abs(t))
        np.add.at(ny, i, 1)

    one_way(a64, b64, idx1, g1, ga, gb, sa, sb, na, nb)
    one_way(b64, a64, idx2, g2, gb, ga, sb, sa, nb, na)
    grow = lambda n: ((1.0 + U24) ** (n + 1.0) - 1.0) * (1.0 + 2.0 ** -20)
    bound_a = sa * grow(na)[:, None] + na[:, None] * 2.0 ** -149
    bound_b = sb * grow(nb)[:, None] + nb[:, None] * 2.0 ** -149
    return ga, bound_a, gb, bound_b


def fscore(dist_ab, dist_ba, threshold):
    """(chamfer, fscore) of geometric_loss.py's formulae on two squared-distance vectors, float64 of float32 means as torch computes
    them is NOT attempted: plain float64"""
    dab, dba = np.asarray(dist_ab, np.float64), np.asarray(dist_ba, np.float64)
    p_ab, p_ba = float((dab < threshold).mean()), float((dba < threshold).mean())
    return dab.mean() + dba.mean(), 2.0 * p_ab * p_ba / max(p_ab + p_ba, 1e-10)
