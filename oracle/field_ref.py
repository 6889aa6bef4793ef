"""CPU restatement of the hash-grid field encoder -- test infrastructure only.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this; geosplatting_amd never does.

Restates `HashEncoding` with `backend='torch'` (rfstudio/model/components/encoding.py:124-241: __setup__ scalings,
hash_fn, pytorch_fwd, the grad-scaling trick of __call__) and `MLP.__call__` (rfstudio/nn/mlp.py:126-145) in plain
torch, any dtype (float64 for gradient checks).  PINNED by tests/golden/ref_hashgrid.npz, which
scripts/make_golden_field.py produced by executing those reference functions themselves.
(The reference's default `backend='tcnn'` is tinycudann -- CUDA only, absent, different cell convention; it is NOT what
is restated here.)
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch


def level_scalings(num_levels: int = 16, min_res: int = 16, max_res: int = 1024) -> torch.Tensor:
    """encoding.py:124-132 (same torch expression, so the same float32 values)"""
    levels = torch.arange(num_levels)
    growth = np.exp((np.log(max_res) - np.log(min_res)) / (num_levels - 1)) if num_levels > 1 else 1
    return torch.floor(min_res * growth ** levels)


def hash_fn(coords: torch.Tensor, table_size: int, num_levels: int) -> torch.Tensor:
    """encoding.py:168-185; coords [..., L, 3] int32 -> rows of the [L*T, F] table"""
    c = coords * torch.tensor([1, 2654435761, 805459861])
    x = torch.bitwise_xor(torch.bitwise_xor(c[..., 0], c[..., 1]), c[..., 2])
    x = x % table_size
    return x + torch.arange(num_levels) * table_size


def encode(x: torch.Tensor, table: torch.Tensor, scalings: torch.Tensor, log2_T: int) -> torch.Tensor:
    """encoding.py:187-229; x [N,3] in [-1,1] -> [N, L*F]"""
    L = scalings.shape[0]
    T = 2 ** log2_T
    p = x[..., None, :] * 0.5 + 0.5
    scaled = p * scalings.view(-1, 1).to(p.dtype)
    sc = torch.ceil(scaled).to(torch.int32); sf = torch.floor(scaled).to(torch.int32)
    o = scaled - sf
    pick = lambda bx, by, bz: table[hash_fn(torch.stack([(sc if bx else sf)[..., 0], (sc if by else sf)[..., 1],
                                                           (sc if bz else sf)[..., 2]], -1), T, L)]
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    f03 = pick(1, 1, 1) * ox + pick(0, 1, 1) * (1 - ox)
    f12 = pick(1, 0, 1) * ox + pick(0, 0, 1) * (1 - ox)
    f56 = pick(1, 0, 0) * ox + pick(0, 0, 0) * (1 - ox)
    f47 = pick(1, 1, 0) * ox + pick(0, 1, 0) * (1 - ox)
    f0312 = f03 * oy + f12 * (1 - oy)
    f4756 = f47 * oy + f56 * (1 - oy)
    return torch.flatten(f0312 * oz + f4756 * (1 - oz), start_dim=-2)


def mlp(feats: torch.Tensor, weights: Sequence[torch.Tensor], activation: str = "none") -> torch.Tensor:
    """mlp.py:126-145 without bias / skip connections: ReLU between layers, `activation` after the last"""
    x = feats
    for i, w in enumerate(weights):
        x = x @ w.t()
        if i < len(weights) - 1:
            x = torch.relu(x)
        elif activation == "sigmoid":
            x = x.sigmoid()
    return x


def hash_encoding(x, table, scalings, log2_T, weights: Optional[List[torch.Tensor]] = None, activation="none",
                  grad_scaling: Optional[float] = None):
    """encoding.py:231-241: the full HashEncoding.__call__"""
    if grad_scaling is not None:
        x = x * (1 / grad_scaling) + x.detach() * (1 - 1 / grad_scaling)
    f = encode(x, table, scalings, log2_T)
    if grad_scaling is not None:
        f = f * grad_scaling + f.detach() * (1 - grad_scaling)
    return f if weights is None else mlp(f, weights, activation)


# ----------------------------------------------------------------------------- element-wise error budgets (numpy)
# The rest of this file restates csrc/gs_hashgrid.hip's ARITHMETIC (not the reference's): float32 in the kernels' operation
# order (contraction is off there, so numpy's float32 reproduces it), the same quantities in float64, and for every output
# element a bound, in units of 2^-24, on what a correct float32 implementation may differ from the float64 value by.
# tests/test_oracle_cpu.py validates restatement and budgets against float64 autograd through `encode` above;
# tests/test_gpu_field_budget.py holds the kernels to them.
_F32 = np.float32
_P1, _P2 = 2654435761, 805459861
# roundings a table-gradient addend g * (wx * wy * wz * tgs) goes through: three (1 - o), three products of the weight, one by g
TABLE_OWN_ROUNDINGS = 7.0
# roundings of one corner's share of d value / d o[k]: two products and an addition in dotg, two (1 - o), two products; the seven
# additions into do_ (the first lands on zero) and the product by s are charged on the level's sum |share|; one more covers
# the terms of second order
VX_LEVEL_ROUNDINGS = 7.0 + 7.0 + 1.0 + 1.0
# roundings on the path of one corner through the forward: (1 - o), product, addition -- per axis
FWD_ROUNDINGS = 9.0


def _corner_bits():
    b = np.arange(8)
    return (b >> 2) & 1, (b >> 1) & 1, b & 1          # corner index = 4 bx + 2 by + bz: the kernels' loop order


def hash_cells(x, scalings, log2_T):
    """(rows [N, L, 8] int64 within the level, o [N, L, 3] float32): the eight corner rows (corner 4 bx + 2 by + bz, b = 1 the
    ceil corner) and the interpolation offsets of every point and level, in float32 with the kernels' operation order
    (x * 0.5 + 0.5, then * s, ceil, floor, o = scaled - floor); hashed with int64 products and Python's modulo like hash_fn"""
    x = np.asarray(x, _F32).reshape(-1, 3)
    s = np.asarray(scalings, _F32).reshape(-1)
    p = x * _F32(0.5) + _F32(0.5)
    scaled = p[:, None, :] * s[None, :, None]
    c = np.ceil(scaled).astype(np.int64); f = np.floor(scaled).astype(np.int64)
    o = scaled - f.astype(_F32)
    bx, by, bz = _corner_bits()
    cx = np.where(bx, c[..., 0:1], f[..., 0:1]); cy = np.where(by, c[..., 1:2], f[..., 1:2]); cz = np.where(bz, c[..., 2:3], f[..., 2:3])
    rows = (cx ^ (cy * _P1) ^ (cz * _P2)) % (1 << log2_T)
    return rows, o


def _weights(o, dtype):
    """per-axis corner weights [3][N, L, 8]: o for a ceil corner, 1 - o for a floor corner, rounded in `dtype`"""
    o = o.astype(dtype)
    one = dtype(1.0)
    return [np.where(b, o[..., k:k + 1], one - o[..., k:k + 1]) for k, b in enumerate(_corner_bits())]


def _gather(table, rows, log2_T):
    L = rows.shape[1]
    return np.asarray(table, _F32).reshape(-1, 2)[rows + (np.arange(L, dtype=np.int64) << log2_T)[None, :, None]]      # [N, L, 8, 2]


def encode_fwd(x, table, scalings, log2_T):
    """(features float32 [N, 2L] in the kernel's nesting -- x pairs, then y, then z --, the same in float64 with the float32
    offsets as exact constants, budget): budget = FWD_ROUNDINGS * sum over the eight corners of |t| * w"""
    rows, o = hash_cells(x, scalings, log2_T)
    t = _gather(table, rows, log2_T)
    N, L = rows.shape[:2]
    out = []
    for dt in (_F32, np.float64):
        tt = t.astype(dt); oo = o.astype(dt); one = dt(1.0)
        ox, oy, oz = oo[..., 0:1], oo[..., 1:2], oo[..., 2:3]
        fx = lambda by, bz: tt[:, :, 4 + 2 * by + bz] * ox + tt[:, :, 2 * by + bz] * (one - ox)
        z1 = fx(1, 1) * oy + fx(0, 1) * (one - oy)
        z0 = fx(1, 0) * oy + fx(0, 0) * (one - oy)
        out.append((z1 * oz + z0 * (one - oz)).reshape(N, 2 * L))
    w = _weights(o, np.float64)
    bud = FWD_ROUNDINGS * (np.abs(t.astype(np.float64)) * (w[0] * w[1] * w[2])[..., None]).sum(2).reshape(N, 2 * L)
    return out[0], out[1], bud


def fx_exponent(N, gmax, tgs):
    """hg_fx_exponent: e with 8 N gmax |tgs| 2^e < 2^62, the product formed in float32 like the kernel's"""
    v = _F32(8.0) * _F32(N) * _F32(gmax) * _F32(abs(tgs))
    return 62 - int(np.frexp(v)[1])


def encode_bwd_budget(x, table, scalings, log2_T, v_out, tgs, mode, N_for_exponent=None):
    """Gradients of sum(features * v_out) with the offsets taken as exact constants (d o / d x = s / 2), and their budgets.
    mode 'float': the atomic and the float-slab table gradient (order of the additions controlled by nobody);
    mode 'fixed': the 64-bit fixed-point table gradient (order-free).  Returns a dict:
      v_x, v_x_f32, v_x_budget [N, 3]: float64 value, float32 restatement in the kernels' order, budget;
      rows [R]: the table rows (l * T + row) that any corner of any point hits, sorted; every other row is untouched;
      v_table, v_table_f32, v_table_budget, n, abs_sum [R, 2]: float64 sum, float32 restatement (mode 'float': added in point order
        with the slab kernel's products; mode 'fixed': the kernel's integers, so its exact bits), budget, number of non-zero
        contributions and sum |contribution| per element.  An element with n = 0 has budget 0 and must be left exactly alone."""
    assert mode in ("float", "fixed")
    x = np.asarray(x, _F32).reshape(-1, 3)
    s32 = np.asarray(scalings, _F32).reshape(-1)
    N, L = x.shape[0], s32.shape[0]
    T = 1 << log2_T
    g32 = np.asarray(v_out, _F32).reshape(N, L, 2)
    rows, o = hash_cells(x, s32, log2_T)
    t32 = _gather(table, rows, log2_T)
    sign = [np.where(b, 1.0, -1.0) for b in _corner_bits()]
    # ---- v_x: float32 in the kernels' order
    w = _weights(o, _F32)
    dotg = (_F32(0.0) + t32[..., 0] * g32[:, :, None, 0]) + t32[..., 1] * g32[:, :, None, 1]
    other = ((1, 2), (0, 2), (0, 1))
    gx = np.zeros((N, 3), _F32)
    for k in range(3):
        a, b = other[k]
        share = (sign[k].astype(_F32) * w[a]) * w[b] * dotg                      # [N, L, 8]
        d = np.zeros((N, L), _F32)
        for cnr in range(8):
            d = d + share[:, :, cnr]
        for l in range(L):
            gx[:, k] = gx[:, k] + d[:, l] * s32[l] * _F32(0.5)
    # ---- v_x: float64 and budget
    w64 = _weights(o, np.float64)
    t64, g64, s64 = t32.astype(np.float64), g32.astype(np.float64), s32.astype(np.float64)
    dot64 = t64[..., 0] * g64[:, :, None, 0] + t64[..., 1] * g64[:, :, None, 1]
    dabs = np.abs(t64[..., 0] * g64[:, :, None, 0]) + np.abs(t64[..., 1] * g64[:, :, None, 1])
    vx, vxb = np.zeros((N, 3)), np.zeros((N, 3))
    for k in range(3):
        a, b = other[k]
        term = (sign[k] * w64[a] * w64[b] * dot64).sum(2) * s64 * 0.5            # [N, L]
        mag = (w64[a] * w64[b] * dabs).sum(2) * s64 * 0.5
        vx[:, k] = term.sum(1)
        vxb[:, k] = VX_LEVEL_ROUNDINGS * mag.sum(1) + (L - 1) * np.abs(term).sum(1)
    # ---- v_table
    grow = (rows + (np.arange(L, dtype=np.int64) << log2_T)[None, :, None]).reshape(-1)          # [N L 8], point-major
    urows, inv = np.unique(grow, return_inverse=True)
    inv = inv.reshape(-1)
    R = urows.shape[0]
    w3 = (w64[0] * w64[1] * w64[2] * float(tgs))[..., None] * g64[:, :, None, :]                  # contributions [N, L, 8, 2]
    wf = ((w[0] * w[1]) * w[2]) * _F32(tgs)
    c32 = g32[:, :, None, :] * wf[..., None]                                                         # the slab kernels' products
    want, asum, cnt, f32v = np.zeros((R, 2)), np.zeros((R, 2)), np.zeros((R, 2)), np.zeros((R, 2), _F32)
    for q in range(2):
        cq = w3[..., q].reshape(-1)
        want[:, q] = np.bincount(inv, cq, R)
        asum[:, q] = np.bincount(inv, np.abs(cq), R)
        cnt[:, q] = np.bincount(inv, (cq != 0).astype(np.float64), R)
    own = TABLE_OWN_ROUNDINGS * asum
    if mode == "float":
        bud = own + np.maximum(cnt - 1.0, 0.0) * asum
        for q in range(2):
            acc = np.zeros(R, _F32)
            np.add.at(acc, inv, c32[..., q].reshape(-1))
            f32v[:, q] = acc
    else:
        Ne = N if N_for_exponent is None else N_for_exponent
        gmax = np.abs(g32).max(axis=(0, 2)) if N else np.zeros(L, _F32)
        e = np.array([fx_exponent(Ne, gm, tgs) if gm > 0 else 0 for gm in gmax])
        lvl = (urows >> log2_T).astype(np.int64)
        trunc = np.where(gmax[lvl] > 0, np.ldexp(1.0, 24 - e[lvl]), 0.0)[:, None]
        bud = own + cnt * trunc + np.abs(want)
        live = (g32 != 0).any(2)                                                                      # the kernel skips g == (0, 0)
        e_pt = np.broadcast_to(e[None, :, None], rows.shape)
        for q in range(2):
            add = np.trunc(np.ldexp(c32[..., q].astype(np.float64), e_pt)) * live[:, :, None]
            acc = np.zeros(R, np.int64)
            np.add.at(acc, inv, add.reshape(-1).astype(np.int64))
            f32v[:, q] = np.ldexp(acc.astype(np.float64), -e[lvl]).astype(_F32)
    bud = np.where(cnt > 0, bud, 0.0)
    return dict(v_x=vx, v_x_f32=gx, v_x_budget=vxb, rows=urows, v_table=want, v_table_f32=f32v, v_table_budget=bud, n=cnt, abs_sum=asum)


# ---- gs_mlp_wgrad
def wgrad_plan_blocks(N):
    """wgrad_blocks of csrc/gs_hashgrid.hip: 512 points per workgroup (4 waves x 8 trips x 16 points), 1 .. 1024 workgroups"""
    return int(min(max((N + 511) // 512, 1), 1024))


def wgrad_points_per_wave(N, nb):
    """the most points one wave accumulates: trips of 16 points, strided over the 4 nb waves"""
    return 16 * int(-(-N // (64 * nb)))


def wgrad_budget(dY, X, scale, nb):
    """(dW float64 [O, I] = scale * dY^T X, budget): budget = depth * sum_n |dY[n, o] X[n, i]| * |scale| with depth the longest
    chain of additions an element goes through -- the points of one wave (one rounding per accumulate of the matrix unit, nothing
    else assumed about it), 3 for the fold of the four waves, ceil(nb / 32) + 32 for the reduce kernel.  The first addition of each
    of the three chains lands on zero: that slack covers the rounding of the product, of `* scale` and of the final store."""
    dY = np.asarray(dY, np.float64); X = np.asarray(X, np.float64)
    N = dY.shape[0]
    depth = wgrad_points_per_wave(N, nb) + 3 + -(-nb // 32) + 32
    return float(scale) * (dY.T @ X), depth * abs(float(scale)) * (np.abs(dY).T @ np.abs(X))


def wgrad_f32(dY, X, scale, nb):
    """float32 dW with the additions in the launch plan's order (the two points of one matrix instruction in index order)"""
    dY = np.asarray(dY, _F32); X = np.asarray(X, _F32)
    N, O = dY.shape; I = X.shape[1]
    waves = 4 * nb
    trips = -(-N // (waves * 16)) if N else 0
    acc = np.zeros((waves, O, I), _F32)
    pad = trips * waves * 16 - N
    dYp = np.concatenate([dY, np.zeros((pad, O), _F32)]).reshape(trips, waves, 16, O)
    Xp = np.concatenate([X, np.zeros((pad, I), _F32)]).reshape(trips, waves, 16, I)
    for tr in range(trips):
        for u in range(16):
            acc = acc + dYp[tr, :, u, :, None] * Xp[tr, :, u, None, :]
    acc = acc.reshape(nb, 4, O, I)
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    red = np.zeros((32, O, I), _F32)
    for b in range(nb):
        red[b % 32] = red[b % 32] + part[b]
    t = np.zeros((O, I), _F32)
    for q in range(32):
        t = t + red[q]
    return t * _F32(scale)
