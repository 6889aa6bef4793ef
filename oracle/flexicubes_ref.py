"""CPU restatement of the FlexiCubes dual-marching-cubes extraction -- test infrastructure only.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this; geosplatting_amd never does.

Restates `FlexiCubes.dual_marching_cubes` with `grad_func=None` (rfstudio/graphics/_mesh/_flexicubes.py:559-713), its
helpers `_get_case_id` (:459-506), `_identify_surf_edges` (:508-538), `_linear_interp` (:540-557), `_compute_reg_loss`
(:727-741), `_triangulate` (:743-802), `compute_entropy` (:715-725) and the grid of `from_resolution` (:397-457), in
torch of any dtype (float64 for gradient checks; autograd supplies the reference gradients).

The 256-case tables (`_flexicubes.py:36-366`) are NOT taken from the reference: `dmc_patches` / `check_entry` below
derive them from the cube's corner/edge incidence by rule, and scripts/make_golden_flexicubes.py asserts (in the build
container, where the reference is importable) that the derived tables equal the reference's entry for entry.
PINNED by tests/golden/ref_flexicubes.npz, which that script produced by executing the reference extraction itself.

Index formulation (differs from the reference's torch.unique / sort pipeline, produces the same numbering):
  * grid vertex  (i0,i1,i2) -> id  i0 + (R0+1) * (i1 + (R1+1) * i2)   (corner bit 0 moves i0; `from_resolution` :443)
  * a grid edge is keyed (first vertex f, kind): kind 0 = (f, f - s1) [cube edges 8..11, stored high-to-low], kind 1 =
    (f, f + 1) [edges 0,2,4,6], kind 2 = (f, f + s2) [edges 1,3,5,7]; the reference's `unique(dim=0)` order of edge rows
    is exactly ascending slot = 3 f + kind, so the rank of a surface edge is a prefix count over the slots;
  * dual vertices are numbered by (number of patches of the cube, cube id, patch) (:648-664);
  * quads by (flip class, edge rank) (:760-772), the four cubes around an edge in ascending cube id.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

CUBE_EDGES = ((0, 1), (1, 5), (4, 5), (0, 4), (2, 3), (3, 7), (6, 7), (2, 6), (2, 0), (3, 1), (7, 5), (6, 4))   # :18-33


# ------------------------------------------------------------------------------------------------ derived tables
def _components(corners: set) -> List[List[int]]:
    left, out = set(corners), []
    while left:
        seed = min(left)
        comp, frontier = {seed}, [seed]
        while frontier:
            c = frontier.pop()
            for a, b in CUBE_EDGES:
                for p, q in ((a, b), (b, a)):
                    if p == c and q in left and q not in comp:
                        comp.add(q); frontier.append(q)
        left -= comp
        out.append(sorted(comp))
    return out


def dmc_patches(case: int) -> List[List[int]]:
    """Edge groups (one dual vertex each) of a corner-occupancy case.  One patch per connected component of the
    occupied corners, components by their lowest corner, edges ascending -- except the four 'tunnel' cases whose two
    empty corners are opposite ends of a body diagonal, which take the components of the EMPTY corners instead."""
    occ = {c for c in range(8) if case >> c & 1}
    emp = set(range(8)) - occ
    side = occ
    if len(emp) == 2 and sum(emp) == 7 and (min(emp) ^ max(emp)) == 7:
        side = emp
    patches = []
    for comp in _components(side):
        edges = [i for i, (a, b) in enumerate(CUBE_EDGES) if (a in comp) != (b in comp)]
        if edges:
            patches.append(edges)
    return patches


_FACES = [((axis, val), [c for c in range(8) if (c >> axis & 1) == val]) for axis in range(3) for val in (0, 1)]


def check_entry(case: int) -> Optional[Tuple[int, int, int, int]]:
    """(d0, d1, d2, inverted case) for the cases whose 2 or 3 EMPTY corners put a checkerboard on exactly one face
    (`_flexicubes.py:36-78`): the neighbour across that face decides whether both cubes flip to the complement case."""
    emp = [c for c in range(8) if not case >> c & 1]
    if len(emp) not in (2, 3):
        return None
    amb = []
    for (axis, val), fc in _FACES:
        e = [c for c in fc if c in emp]
        if len(e) == 2 and (e[0] ^ e[1]) == (7 ^ (1 << axis)):
            amb.append((axis, val))
    if len(amb) != 1:
        return None
    axis, val = amb[0]
    d = [0, 0, 0]
    d[axis] = 1 if val else -1
    return d[0], d[1], d[2], 255 - case


def tables():
    """(patch edge lists [256][<=4][<=7], num patches [256], check [256,5] as the reference lays it out)"""
    dmc = [dmc_patches(c) for c in range(256)]
    chk = np.zeros((256, 5), dtype=np.int64)
    for c in range(256):
        e = check_entry(c)
        if e is not None:
            chk[c] = (1,) + e
    return dmc, np.array([len(p) for p in dmc], dtype=np.int64), chk


# ------------------------------------------------------------------------------------------------ grid
def grid(res: Tuple[int, int, int], scale: float = 1.0, dtype=torch.float32):
    """`from_resolution` (:397-457): vertices [(R0+1)(R1+1)(R2+1), 3] and cube corner indices [R0 R1 R2, 8]."""
    R0, R1, R2 = res
    a, b, c = np.meshgrid(np.arange(R0 + 1), np.arange(R1 + 1), np.arange(R2 + 1), indexing="ij")
    coords = torch.from_numpy(np.stack((a, b, c), -1).reshape(-1, 3)).float()
    verts = coords / torch.tensor([R0, R1, R2], dtype=torch.long)
    n = np.arange(R0 * R1 * R2)
    base = np.stack((n % R0, (n // R0) % R1, n // (R0 * R1)), -1)[:, None, :]
    corners = np.array([[k & 1, k >> 1 & 1, k >> 2 & 1] for k in range(8)])[None]
    cc = base + corners
    idx = (cc[..., 2] * (1 + R1) + cc[..., 1]) * (1 + R0) + cc[..., 0]
    return ((2 * verts - 1) * scale).to(dtype), torch.from_numpy(idx)


def _interp(sa, sb, xa, xb, sdf_eps):
    w = sa / (sa - sb)                                                   # :551-556
    if sdf_eps is not None:
        w = (1 - sdf_eps) * w + sdf_eps / 2
    return xb * w + xa * (1 - w)


def extract(vertices: torch.Tensor, sdf: torch.Tensor, res, alpha=None, beta=None, gamma=None, *, weight_scale=0.99,
            sdf_eps=None, return_aux: bool = False):
    """vertices [Vg,3], sdf [Vg], raw alpha [C,8] / beta [C,12] / gamma [C,1] (or None) ->
    (mesh vertices [Q+nq,3], faces [4 nq,3] int64, L_dev [K])"""
    R0, R1, R2 = (int(r) for r in res)
    s1, s2 = R0 + 1, (R0 + 1) * (R1 + 1)
    Vg, C = s2 * (R2 + 1), R0 * R1 * R2
    assert vertices.shape == (Vg, 3) and sdf.numel() == Vg
    sdf = sdf.reshape(-1)
    dmc, nvd_t, chk = tables()
    occ = (sdf.detach() < 0).numpy()
    n = np.arange(C)
    origin = (n % R0) + s1 * ((n // R0) % R1) + s2 * (n // (R0 * R1))
    corner_off = np.array([(k & 1) + s1 * (k >> 1 & 1) + s2 * (k >> 2 & 1) for k in range(8)])
    cube_v = origin[:, None] + corner_off[None]                          # [C,8]
    raw = (occ[cube_v] << np.arange(8)).sum(-1)
    surf = (raw > 0) & (raw < 255)
    assert surf.any()
    # ambiguity resolution (:459-506): positions are the C-order unravel of the cube id over `res`
    case = raw.copy()
    prob = surf & (chk[raw, 0] == 1)
    pid = n[prob]
    u = np.stack(np.unravel_index(pid, (R0, R1, R2)), -1)
    adj = u + chk[raw[pid], 1:4]
    ok = (adj >= 0).all(-1) & (adj < np.array([R0, R1, R2])).all(-1)
    adj_id = np.ravel_multi_index(tuple(adj[ok].T), (R0, R1, R2)) if ok.any() else np.zeros(0, dtype=np.int64)
    flip = prob[adj_id]
    case[pid[ok][flip]] = chk[raw[pid[ok][flip]], 4]

    sid = n[surf]                                                        # surface cubes, ascending
    scase = case[sid]
    nvd = nvd_t[scase]
    # grid-edge slots
    edge_first = np.array([max(a, b) if e >= 8 else min(a, b) for e, (a, b) in enumerate(CUBE_EDGES)])
    edge_kind = np.array([0 if e >= 8 else (1 if (a ^ b) == 1 else 2) for e, (a, b) in enumerate(CUBE_EDGES)])
    slot_of = lambda cubes: 3 * (origin[cubes][:, None] + corner_off[edge_first][None]) + edge_kind[None]   # [.,12]
    f_all = np.arange(Vg)
    second = np.stack((f_all - s1, f_all + 1, f_all + s2), -1)            # [Vg,3]
    i0, i1, i2 = f_all % s1, (f_all // s1) % (R1 + 1), f_all // s2
    exists = np.stack((i1 >= 1, i0 < R0, i2 < R2), -1)
    sec_c = np.where(exists, second, 0)
    cross = exists & (occ[f_all][:, None] != occ[sec_c])
    cross_f = cross.reshape(-1)
    rank = np.cumsum(cross_f) - cross_f                                   # rank of a surface edge among surface edges
    E = int(cross_f.sum())
    e_first = np.repeat(f_all, 3)[cross_f]; e_second = second.reshape(-1)[cross_f]

    # dual vertices in reference order (:648-664)
    xs_a, xs_b = vertices[e_first], vertices[e_second]
    s_a, s_b = sdf[e_first], sdf[e_second]
    zero_cross = _interp(s_a[:, None], s_b[:, None], xs_a, xs_b, sdf_eps)

    k_edge, k_vd, k_cube, k_slot, vd_cube, vd_cnt = [], [], [], [], [], []
    vd_base = np.zeros(sid.shape[0], dtype=np.int64)
    total = 0
    for num in range(1, 5):
        sel = np.nonzero(nvd == num)[0]
        if sel.size == 0:
            continue
        vd_base[sel] = total + num * np.arange(sel.size)
        for j, s in enumerate(sel):
            for p, edges in enumerate(dmc[scase[s]]):
                v = total + num * j + p
                vd_cube.append(s); vd_cnt.append(len(edges))
                for e in edges:
                    k_edge.append(e); k_vd.append(v); k_cube.append(s)
        total += num * sel.size
    Q = total
    k_edge, k_vd, k_cube = (np.asarray(a, dtype=np.int64) for a in (k_edge, k_vd, k_cube))
    vd_cube, vd_cnt = np.asarray(vd_cube, dtype=np.int64), np.asarray(vd_cnt, dtype=np.int64)
    k_slot = slot_of(sid[k_cube])[np.arange(k_edge.size), k_edge]
    assert cross_f[k_slot].all()
    k_rank = rank[k_slot]
    dt = vertices.dtype
    if alpha is not None:
        a_act = torch.tanh(alpha[sid]) * weight_scale + 1                 # [N,8]
        ce = np.array(CUBE_EDGES)
        al_a = a_act[k_cube, ce[k_edge, 0]]; al_b = a_act[k_cube, ce[k_edge, 1]]
        ue = _interp((s_a[k_rank] * al_a)[:, None], (s_b[k_rank] * al_b)[:, None], xs_a[k_rank], xs_b[k_rank], sdf_eps)
    else:
        ue = zero_cross[k_rank]
    if beta is not None:
        b_act = torch.tanh(beta[sid]) * weight_scale + 1
        bk = b_act[k_cube, k_edge][:, None]
    else:
        bk = torch.ones(k_edge.size, 1, dtype=dt)
    g_act = (torch.sigmoid(gamma[sid]) * weight_scale + (1 - weight_scale) / 2).reshape(-1) if gamma is not None \
        else torch.ones(sid.size, dtype=dt)
    k_vd_t = torch.from_numpy(k_vd)
    bsum = torch.zeros(Q, 1, dtype=dt).index_add_(0, k_vd_t, bk)
    vd = torch.zeros(Q, 3, dtype=dt).index_add_(0, k_vd_t, ue * bk) / bsum
    dist = (zero_cross[k_rank] - vd[k_vd_t]).norm(dim=-1)                 # :727-741
    mean = torch.zeros(Q, dtype=dt).index_add_(0, k_vd_t, dist) / torch.from_numpy(vd_cnt).to(dt)
    L_dev = (dist - mean[k_vd_t]).abs()
    vd_gamma = g_act[vd_cube]

    # which dual vertex owns (surface cube, cube edge)
    owner = np.zeros((sid.size, 12), dtype=np.int64)
    owner[k_cube, k_edge] = k_vd
    surf_pos = np.full(C, -1, dtype=np.int64); surf_pos[sid] = np.arange(sid.size)

    # quads (:752-772): interior surface edges; the 4 cubes around the edge in ascending cube id
    ef, ek = np.repeat(f_all, 3)[cross_f], np.tile(np.arange(3), Vg)[cross_f]
    j0, j1, j2 = ef % s1, (ef // s1) % (R1 + 1), ef // s2
    interior = np.where(ek == 0, (j0 >= 1) & (j0 < R0) & (j2 >= 1) & (j2 < R2),
                        np.where(ek == 1, (j1 >= 1) & (j1 < R1) & (j2 >= 1) & (j2 < R2),
                                 (j0 >= 1) & (j0 < R0) & (j1 >= 1) & (j1 < R1)))
    eid = np.nonzero(interior)[0]
    # lower vertex of the edge and the cubes touching it
    lo = np.where(ek == 0, ef - s1, ef)
    l0, l1, l2 = lo % s1, (lo // s1) % (R1 + 1), lo // s2
    cid = lambda x, y, z: x + R0 * (y + R1 * z)
    quad_vd = np.zeros((eid.size, 4), dtype=np.int64)
    for q, e in enumerate(eid):
        x, y, z, k = l0[e], l1[e], l2[e], ek[e]
        if k == 1:      # along i0: cubes (x, y-1..y, z-1..z)
            cubes = [cid(x, y - 1, z - 1), cid(x, y, z - 1), cid(x, y - 1, z), cid(x, y, z)]
        elif k == 0:    # along i1: cubes (x-1..x, y, z-1..z)
            cubes = [cid(x - 1, y, z - 1), cid(x, y, z - 1), cid(x - 1, y, z), cid(x, y, z)]
        else:           # along i2: cubes (x-1..x, y-1..y, z)
            cubes = [cid(x - 1, y - 1, z), cid(x, y - 1, z), cid(x - 1, y, z), cid(x, y, z)]
        slot = 3 * ef[e] + k
        for t, c in enumerate(cubes):
            sp = surf_pos[c]
            assert sp >= 0
            ce_slots = slot_of(np.array([c]))[0]
            ee = int(np.nonzero(ce_slots == slot)[0][0])
            quad_vd[q, t] = owner[sp, ee]
    flipm = (sdf.detach()[torch.from_numpy(ef[eid])] > 0).numpy()
    quad_vd = np.concatenate((quad_vd[flipm][:, [0, 1, 3, 2]], quad_vd[~flipm][:, [2, 3, 1, 0]]))
    qt = torch.from_numpy(quad_vd)
    qg = vd_gamma[qt.reshape(-1)].reshape(-1, 4)
    g02 = (qg[:, 0] * qg[:, 2])[:, None]; g13 = (qg[:, 1] * qg[:, 3])[:, None]
    vq = vd[qt.reshape(-1)].reshape(-1, 4, 3)
    v02 = (vq[:, 0] + vq[:, 2]) / 2; v13 = (vq[:, 1] + vq[:, 3]) / 2
    centre = (v02 * g02 + v13 * g13) / ((g02 + g13) + 1e-8)
    nq = quad_vd.shape[0]
    cidx = torch.arange(nq) + Q
    faces = torch.stack((qt[:, [0, 1, 2, 3]], qt[:, [1, 2, 3, 0]], cidx[:, None].expand(nq, 4)), -1).reshape(-1, 3)
    out = (torch.cat((vd, centre)), faces, L_dev)
    if return_aux:
        case8 = np.zeros(C, dtype=np.int64); case8[sid] = scase
        k_first = np.zeros(sid.size, dtype=np.int64)                     # first (patch, edge) row of every surface cube
        if k_cube.size:
            k_first[k_cube[::-1]] = np.arange(k_cube.size)[::-1]
        quad_id = np.full(3 * Vg, -1, dtype=np.int64)
        qslot = 3 * ef[eid] + ek[eid]
        quad_id[np.concatenate((qslot[flipm], qslot[~flipm]))] = np.arange(nq)
        amb = dict(raw=raw[pid], inside=ok, axis_dir=chk[raw[pid], 1:4], complemented=np.zeros(pid.size, dtype=bool))
        amb["complemented"][np.nonzero(ok)[0][flip]] = True
        return out + (dict(case=scase, surf_cubes=sid, num_vd=nvd, Q=Q, E=E, num_quads=nq, num_flipped=int(flipm.sum()),
                           raw=raw, case8=case8, vd_base=vd_base, k_base=k_first, quad_id=quad_id, ambiguous=amb,
                           k_vd=k_vd, k_cube=k_cube, k_edge=k_edge, k_a=e_first[k_rank], k_b=e_second[k_rank],
                           vd_cube=vd_cube, vd_cnt=vd_cnt, quad_vd=quad_vd, cross_first=e_first, cross_second=e_second),)
    return out


def entropy(sdf: torch.Tensor, res) -> torch.Tensor:
    """`compute_entropy` (:715-725): BCE-with-logits across every sign-changing grid edge, both directions."""
    R0, R1, R2 = (int(r) for r in res)
    s1, s2 = R0 + 1, (R0 + 1) * (R1 + 1)
    Vg = s2 * (R2 + 1)
    sdf = sdf.reshape(-1)
    f = np.arange(Vg)
    second = np.stack((f - s1, f + 1, f + s2), -1)
    i0, i1, i2 = f % s1, (f // s1) % (R1 + 1), f // s2
    exists = np.stack((i1 >= 1, i0 < R0, i2 < R2), -1)
    occ = (sdf.detach() < 0).numpy()
    cross = (exists & (occ[f][:, None] != occ[np.where(exists, second, 0)])).reshape(-1)
    a = sdf[torch.from_numpy(np.repeat(f, 3)[cross])]; b = sdf[torch.from_numpy(second.reshape(-1)[cross])]
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    return bce(a, (b > 0).to(sdf.dtype)) + bce(b, (a > 0).to(sdf.dtype))


# ------------------------------------------------------------------------------------------------ per-element error budgets
# Units: 2^-24 (the unit roundoff u of float32).  Every bound is first order in u, computed in float64 from the float64 intermediates.
R_TANH = 2.0        # relative roundings charged to tanhf / expf / log1pf / sqrtf results (libm, not correctly rounded)
FLT_MIN_U = 2.0 ** -126 * 2.0 ** 24          # float32 underflow threshold in units of u: expf / sigmoid flush below it
JUMP = 2.0 ** 25                             # "this factor's sign / direction is not determined": 2 |x| in units of u |x|


def _scatter(n, idx, val):
    return np.bincount(idx, val, n) if idx.size else np.zeros(n)


def _atomic_budget(n, idx, c, ec, m=None):
    """sum of contributions c (own bounds ec, magnitudes m >= |c|: the sizes of the terms a contribution is itself made of) into n
    slots in an order nobody controls: sum ec + (count - 1) sum m; count of non-zero contributions per slot returned too (0 ->
    budget 0: the slot must be exactly +0)"""
    cnt = _scatter(n, idx, ((c != 0) | (ec > 0)).astype(np.float64))     # a zero that is a cancellation (d w / d A at B = 0) counts
    a = _scatter(n, idx, np.abs(c) if m is None else m)
    return np.where(cnt > 0, _scatter(n, idx, ec) + np.maximum(cnt - 1, 0) * a, 0.0), cnt, a


def _tanh_act(raw, ws):
    """activated weight tanh(raw) ws + 1: value, bound, d/d raw = ws (1 - t^2), bound of the derivative (1 - t^2 by its operands)"""
    t = np.tanh(raw)
    act = t * ws + 1
    e_act = np.abs(t * ws) * (R_TANH + 1) + np.abs(act)
    sech = 1 - t * t
    e_sech = t * t * (2 * R_TANH + 1) + np.abs(sech)
    return act, e_act, ws * sech, np.abs(ws) * (e_sech + np.abs(sech))


def extract_budget(vertices, sdf, res, alpha=None, beta=None, gamma=None, *, weight_scale=0.99, sdf_eps=None, v_vertices=None,
                   v_L_dev=None):
    """Float64 reference and first-order float32 error budgets of the extraction, forward and backward, element by element.

    Inputs are float32 arrays (weight_scale / sdf_eps are rounded to float32 first, as the C ABI receives them); the reference is
    float64 autograd of `extract` on them for the cotangents v_vertices [Q + nq, 3] (None: zero) and v_L_dev [K] (None: zero).
    Returns a dict: `aux` (the topology), and for X in out_vertices, L_dev, g_vertices, g_sdf, g_alpha, g_beta, g_gamma (gradients
    of absent weights are left out): X (float64), X_budget, and for the gradients X_n (number of non-zero contributions; 0 means
    budget 0, the element must be exactly +0) and X_abs (sum |contribution|).  `jump` [name] is a boolean mask of the gradient
    elements whose budget holds a charged discontinuity (an L_dev term whose |d_j - mean| or whose distance d_j lies inside its
    own rounding bound, with a non-zero cotangent reaching it): they are compared, but their budget is of the order of the term.

    The bounds follow the kernels' chain of operations (csrc/gs_flexicubes.hip) but assume nothing about the order of the atomics:
    a slot collecting n non-zero contributions c is charged sum(bound of c) + (n - 1) sum |c|.  Differences of computed quantities
    are charged by their operands: ue - vd (beta), v02 - ctr and v13 - ctr (gamma), d_j - mean (L_dev), 1 - tanh^2, 1 - sigmoid."""
    f32 = lambda t: None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float32))
    ws = float(np.float32(weight_scale))
    eps = None if sdf_eps is None else float(np.float32(sdf_eps))
    R0, R1, R2 = (int(r) for r in res)
    Vg, C = (R0 + 1) * (R1 + 1) * (R2 + 1), R0 * R1 * R2
    x32, s32 = f32(vertices).reshape(Vg, 3), f32(sdf).reshape(Vg)
    a32 = None if alpha is None else f32(alpha).reshape(C, 8)
    b32 = None if beta is None else f32(beta).reshape(C, 12)
    g32 = None if gamma is None else f32(gamma).reshape(C, 1)
    leaf = lambda a: None if a is None else torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
    lx, ls, la, lb, lg = leaf(x32), leaf(s32), leaf(a32), leaf(b32), leaf(g32)
    ov, faces, Ld, aux = extract(lx, ls, res, la, lb, lg, weight_scale=ws, sdf_eps=eps, return_aux=True)
    Q, nq, K = aux["Q"], aux["num_quads"], Ld.shape[0]
    cv = np.zeros((Q + nq, 3)) if v_vertices is None else np.asarray(v_vertices, dtype=np.float32).astype(np.float64).reshape(Q + nq, 3)
    cl = np.zeros(K) if v_L_dev is None else np.asarray(v_L_dev, dtype=np.float32).astype(np.float64).reshape(K)
    loss = (ov * torch.from_numpy(cv)).sum() + (Ld * torch.from_numpy(cl)).sum()
    loss.backward()
    gr = lambda t: None if t is None else (np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy())
    out = dict(aux=aux, faces=faces.numpy(), out_vertices=ov.detach().numpy(), L_dev=Ld.detach().numpy(),
               g_vertices=gr(lx), g_sdf=gr(ls))

    # ---- the same chain by hand, in float64, value and bound together; one row per (cube, patch, edge)
    x, s = x32.astype(np.float64), s32.astype(np.float64)
    kq, kc, ke, ka, kb = aux["k_vd"], aux["k_cube"], aux["k_edge"], aux["k_a"], aux["k_b"]
    cube = aux["surf_cubes"][kc]                                         # grid cube id of every row
    ce = np.array(CUBE_EDGES)
    ca, cb = ce[ke, 0], ce[ke, 1]
    xa, xb, sa, sb = x[ka], x[kb], s[ka], s[kb]
    one, zero = np.ones(K), np.zeros(K)
    if a32 is not None:
        aa, e_aa, daa, e_daa = _tanh_act(a32.astype(np.float64)[cube, ca], ws)
        ab, e_ab, dab, e_dab = _tanh_act(a32.astype(np.float64)[cube, cb], ws)
        rA = (e_aa / np.abs(aa)).clip(min=0) + 1, (e_ab / np.abs(ab)).clip(min=0) + 1       # relative bounds of A = sa aa, Bq = sb ab
    else:
        aa = ab = one; e_aa = e_ab = daa = dab = e_daa = e_dab = zero; rA = (zero, zero)
    if b32 is not None:
        bt, e_bt, dbt_raw, e_dbt_raw = _tanh_act(b32.astype(np.float64)[cube, ke], ws)
    else:
        bt = one; e_bt = dbt_raw = e_dbt_raw = zero

    def interp(A, B, rA_, rB_):
        """w = A / (A - B) [(1 - eps) w + eps / 2] with A, B of opposite sign (|A - B| = |A| + |B|): value, bound, bound of 1 - w,
        D = A - B and its relative bound"""
        D = A - B
        rD = (rA_ * np.abs(A) + rB_ * np.abs(B)) / np.abs(D) + 1
        w0 = A / D
        e_w0 = np.abs(w0) * (rA_ + rD + 1)
        if eps is None:
            return w0, e_w0, e_w0 + np.abs(1 - w0), D, rD
        w = (1 - eps) * w0 + eps / 2
        e_w = (1 - eps) * e_w0 + 2 * np.abs((1 - eps) * w0) + eps / 2 + np.abs(w)
        return w, e_w, e_w + np.abs(1 - w), D, rD

    def lerp(w, e_w, e_1w):
        """xb w + xa (1 - w) per component: value and bound"""
        v = xb * w[:, None] + xa * (1 - w)[:, None]
        e = np.abs(xb) * (e_w + np.abs(w))[:, None] + np.abs(xa) * (e_1w + np.abs(1 - w))[:, None] + np.abs(v)
        return v, e

    A, Bq = sa * aa, sb * ab
    w, e_w, e_1w, D, rD = interp(A, Bq, rA[0], rA[1])
    wz, e_wz, e_1wz, Dz, rDz = interp(sa, sb, zero, zero)
    ue, e_ue = lerp(w, e_w, e_1w)
    zc, e_zc = lerp(wz, e_wz, e_1wz)
    cnt = aux["vd_cnt"].astype(np.float64)                                # rows per dual vertex
    sc3 = lambda v: np.stack([_scatter(Q, kq, v[:, c]) for c in range(3)], -1)
    Bs = _scatter(Q, kq, bt)
    e_Bs = _scatter(Q, kq, e_bt) + (cnt - 1) * Bs
    rBs = e_Bs / Bs
    S = sc3(ue * bt[:, None])
    aS = sc3(np.abs(ue * bt[:, None]))
    e_S = sc3(e_ue * bt[:, None] + np.abs(ue) * (e_bt + bt)[:, None]) + (cnt - 1)[:, None] * aS
    vd = S / Bs[:, None]
    e_vd = e_S / Bs[:, None] + np.abs(vd) * (rBs + 1)[:, None]
    z = zc - vd[kq]
    e_z = e_zc + e_vd[kq] + np.abs(z)
    d = np.sqrt((z * z).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(d[:, None] > 0, z / d[:, None], 0.0)
    e_d = (np.abs(nrm) * e_z).sum(-1) + d * (3 + R_TANH)
    e_d = np.where(d > 0, e_d, e_z.sum(-1))
    mean = _scatter(Q, kq, d) / cnt
    e_mean = (_scatter(Q, kq, e_d) + (cnt - 1) * _scatter(Q, kq, d)) / cnt + mean
    df = d - mean[kq]
    e_df = e_d + e_mean[kq] + np.abs(df)
    out["out_vertices_budget"] = np.zeros((Q + nq, 3)); out["out_vertices_budget"][:Q] = e_vd
    out["L_dev_budget"] = e_df
    assert np.allclose(vd, out["out_vertices"][:Q], rtol=1e-12, atol=1e-14) and np.allclose(np.abs(df), out["L_dev"], rtol=1e-9, atol=1e-14)

    # ---- quads: centre, its gradient to the four dual vertices and to gamma
    qv = aux["quad_vd"]                                                  # [nq, 4] dual vertices in winding order
    qcube = aux["surf_cubes"][aux["vd_cube"][qv]] if nq else np.zeros((0, 4), dtype=np.int64)
    if g32 is not None:
        graw = g32.astype(np.float64).reshape(-1)
        sg_all = 1 / (1 + np.exp(-graw))
        e_sg_all = sg_all * (R_TANH + 2) + FLT_MIN_U
        gm_all = sg_all * ws + (1 - ws) / 2
        e_gm_all = (e_sg_all + sg_all) * ws + 2 * (1 - ws) / 2 + gm_all
        gm, e_gm, sg, e_sg = gm_all[qcube], e_gm_all[qcube], sg_all[qcube], e_sg_all[qcube]
    else:
        gm, e_gm = np.ones((nq, 4)), np.zeros((nq, 4)); sg = e_sg = None
    g02, g13 = gm[:, 0] * gm[:, 2], gm[:, 1] * gm[:, 3]
    e_g02 = e_gm[:, 0] * gm[:, 2] + e_gm[:, 2] * gm[:, 0] + g02
    e_g13 = e_gm[:, 1] * gm[:, 3] + e_gm[:, 3] * gm[:, 1] + g13
    wsum = (g02 + g13) + 1e-8
    e_wsum = e_g02 + e_g13 + (g02 + g13) + wsum
    rws = e_wsum / wsum
    vq, e_vq = vd[qv], e_vd[qv]                                          # [nq, 4, 3]
    v02, v13 = (vq[:, 0] + vq[:, 2]) / 2, (vq[:, 1] + vq[:, 3]) / 2
    e_v02 = (e_vq[:, 0] + e_vq[:, 2]) / 2 + np.abs(v02); e_v13 = (e_vq[:, 1] + e_vq[:, 3]) / 2 + np.abs(v13)
    num = v02 * g02[:, None] + v13 * g13[:, None]
    e_num = (e_v02 * g02[:, None] + np.abs(v02) * (e_g02 + g02)[:, None] + e_v13 * g13[:, None] + np.abs(v13) * (e_g13 + g13)[:, None]
             + np.abs(num))
    ctr = num / wsum[:, None]
    e_ctr = e_num / wsum[:, None] + np.abs(ctr) * (rws + 1)[:, None]
    out["out_vertices_budget"][Q:] = e_ctr
    assert np.allclose(ctr, out["out_vertices"][Q:], rtol=1e-12, atol=1e-14)
    go = cv[Q:]                                                          # [nq, 3]
    a02 = go * (g02 / wsum)[:, None] * 0.5; a13 = go * (g13 / wsum)[:, None] * 0.5
    e_a02 = np.abs(go) * ((e_g02 / wsum) + (g02 / wsum) * (rws + 2))[:, None] * 0.5
    e_a13 = np.abs(go) * ((e_g13 / wsum) + (g13 / wsum) * (rws + 2))[:, None] * 0.5
    # dual-vertex scratch: the copied cotangent plus the quads' atomics
    G = cv[:Q].copy(); e_G = np.zeros((Q, 3)); n_G = (cv[:Q] != 0).astype(np.float64); abs_G = np.abs(cv[:Q])
    for t, (a, e_a) in enumerate(((a02, e_a02), (a13, e_a13), (a02, e_a02), (a13, e_a13))):
        for c in range(3):
            G[:, c] += _scatter(Q, qv[:, t], a[:, c]); e_G[:, c] += _scatter(Q, qv[:, t], e_a[:, c])
            n_G[:, c] += _scatter(Q, qv[:, t], (a[:, c] != 0).astype(np.float64)); abs_G[:, c] += _scatter(Q, qv[:, t], np.abs(a[:, c]))
    e_G = e_G + np.maximum(n_G - 1, 0) * abs_G
    if g32 is not None:
        d02 = (go * (v02 - ctr)).sum(-1) / wsum; d13 = (go * (v13 - ctr)).sum(-1) / wsum
        m02 = np.abs(go * (v02 - ctr)).sum(-1) / wsum; m13 = np.abs(go * (v13 - ctr)).sum(-1) / wsum
        e_d02 = (np.abs(go) * (e_v02 + e_ctr + np.abs(v02 - ctr))).sum(-1) / wsum + m02 * (rws + 2 + 2)
        e_d13 = (np.abs(go) * (e_v13 + e_ctr + np.abs(v13 - ctr))).sum(-1) / wsum + m13 * (rws + 2 + 2)
        dsg = sg * (1 - sg)
        e_dsg = e_sg * (1 - sg) + sg * (e_sg + (1 - sg)) + dsg
        cg, e_cg = np.zeros((nq, 4)), np.zeros((nq, 4))
        for t, (dd, e_dd, o) in enumerate(((d02, e_d02, 2), (d13, e_d13, 3), (d02, e_d02, 0), (d13, e_d13, 1))):
            cg[:, t] = dd * gm[:, o] * ws * dsg[:, t]
            e_cg[:, t] = (e_dd * gm[:, o] + np.abs(dd) * e_gm[:, o]) * ws * dsg[:, t] + np.abs(dd * gm[:, o] * ws) * e_dsg[:, t] + 3 * np.abs(cg[:, t])
        bud, n, a = _atomic_budget(C, qcube.reshape(-1), cg.reshape(-1), e_cg.reshape(-1))
        out.update(g_gamma=gr(lg), g_gamma_budget=bud.reshape(C, 1), g_gamma_n=n.reshape(C, 1), g_gamma_abs=a.reshape(C, 1))
        assert np.allclose(_scatter(C, qcube.reshape(-1), cg.reshape(-1)), out["g_gamma"].reshape(-1), rtol=1e-9, atol=1e-300 + 1e-12 * np.abs(cg).max(initial=0))

    # ---- L_dev backward: cotangent of every distance, then of the zero crossings and the dual vertex
    amb_sign = (np.abs(df) <= (e_d + e_mean[kq]) * 2.0 ** -24) & (cl != 0)
    gd_raw = np.sign(df) * cl
    e_gd_raw = np.where(amb_sign, JUMP * np.abs(cl), 0.0)
    ssum = _scatter(Q, kq, gd_raw)
    m_ss = _scatter(Q, kq, np.abs(gd_raw))
    e_ss = _scatter(Q, kq, e_gd_raw) + (cnt - 1) * m_ss
    gd = gd_raw - (ssum / cnt)[kq]
    e_gd = e_gd_raw + (e_ss / cnt + np.abs(ssum / cnt))[kq] + np.abs(gd_raw) + np.abs(ssum / cnt)[kq]
    with np.errstate(divide="ignore", invalid="ignore"):
        e_n = np.where(d[:, None] > 0, (e_z + np.abs(nrm) * e_d[:, None]) / d[:, None], 0.0)
    amb_dir = ((e_n * 2.0 ** -24 >= 0.5).any(-1) | (d == 0)) & ((gd != 0) | (e_gd > 0))
    e_n = np.where(amb_dir[:, None], JUMP, e_n)
    zg = gd[:, None] * nrm
    e_zg = e_gd[:, None] * np.abs(nrm) + np.abs(gd)[:, None] * e_n + 2 * np.abs(zg)
    gv = G - sc3(zg)
    m_gv = np.abs(G) + sc3(np.abs(zg))
    e_gv = e_G + sc3(e_zg) + cnt[:, None] * m_gv
    jump_q = _scatter(Q, kq, (amb_sign | amb_dir).astype(np.float64)) > 0

    # ---- dual vertex = sum(ue bt) / sum(bt): per row
    gvk, e_gvk = gv[kq], e_gv[kq]
    Bk, rBk = Bs[kq], rBs[kq]
    gue = gvk * (bt / Bk)[:, None]
    e_gue = e_gvk * (bt / Bk)[:, None] + np.abs(gvk) * ((e_bt / Bk) + (bt / Bk) * (rBk + 2))[:, None]
    dx = xb - xa
    dw = (gue * dx).sum(-1); m_dw = np.abs(gue * dx).sum(-1)
    ax = np.abs(xa) + np.abs(xb)                                         # sum_c g_c xb_c - sum_c g_c xa_c is a correct order too
    e_dw = (e_gue * np.abs(dx)).sum(-1) + 2 * (np.abs(gue) * ax).sum(-1) + 4 * m_dw
    dwz = (zg * dx).sum(-1); m_dwz = np.abs(zg * dx).sum(-1)
    e_dwz = (e_zg * np.abs(dx)).sum(-1) + 2 * (np.abs(zg) * ax).sum(-1) + 4 * m_dwz
    if eps is not None:
        dw, m_dw, e_dw = dw * (1 - eps), m_dw * (1 - eps), (e_dw + 2 * m_dw) * (1 - eps)
        dwz, m_dwz, e_dwz = dwz * (1 - eps), m_dwz * (1 - eps), (e_dwz + 2 * m_dwz) * (1 - eps)
    den, denz = D * D, Dz * Dz
    r_den, r_denz = 2 * rD + 1, 2 * rDz + 1
    dA = dw * (-Bq) / den; dBq = dw * A / den
    # d w / d A = 1 / D - A / D^2 = -Bq / D^2: charged by the operands of the first form as well
    e_dA = e_dw * np.abs(Bq) / den + m_dw * np.abs(Bq) / den * (rA[1] + r_den + 2) + 2 * m_dw * (np.abs(D) + np.abs(A)) / den
    e_dBq = e_dw * np.abs(A) / den + m_dw * np.abs(A) / den * (rA[0] + r_den + 2)
    za = dwz * (-sb) / denz; zb = dwz * sa / denz
    e_za = e_dwz * np.abs(sb) / denz + m_dwz * np.abs(sb) / denz * (r_denz + 2) + 2 * m_dwz * (np.abs(Dz) + np.abs(sa)) / denz
    e_zb = e_dwz * np.abs(sa) / denz + m_dwz * np.abs(sa) / denz * (r_denz + 2)
    c_sa = dA * aa + za; c_sb = dBq * ab + zb
    e_csa = e_dA * np.abs(aa) + m_dw * np.abs(Bq) / den * (e_aa + np.abs(aa)) + e_za + np.abs(dA * aa) + np.abs(za)
    e_csb = e_dBq * np.abs(ab) + m_dw * np.abs(A) / den * (e_ab + np.abs(ab)) + e_zb + np.abs(dBq * ab) + np.abs(zb)
    idx = np.concatenate((ka, kb))
    m_csa = m_dw * np.abs(Bq * aa) / den + m_dwz * np.abs(sb) / denz; m_csb = m_dw * np.abs(A * ab) / den + m_dwz * np.abs(sa) / denz
    bud, n, a = _atomic_budget(Vg, idx, np.concatenate((c_sa, c_sb)), np.concatenate((e_csa, e_csb)), np.concatenate((m_csa, m_csb)))
    out.update(g_sdf_budget=bud, g_sdf_n=n, g_sdf_abs=a)
    hand_sdf = _scatter(Vg, idx, np.concatenate((c_sa, c_sb)))
    c_va = gue * (1 - w)[:, None] + zg * (1 - wz)[:, None]; c_vb = gue * w[:, None] + zg * wz[:, None]
    e_cva = (e_gue * np.abs(1 - w)[:, None] + np.abs(gue) * (e_1w + np.abs(1 - w))[:, None] + e_zg * np.abs(1 - wz)[:, None]
             + np.abs(zg) * (e_1wz + np.abs(1 - wz))[:, None] + np.abs(gue * (1 - w)[:, None]) + np.abs(zg * (1 - wz)[:, None]))
    e_cvb = (e_gue * np.abs(w)[:, None] + np.abs(gue) * (e_w + np.abs(w))[:, None] + e_zg * np.abs(wz)[:, None]
             + np.abs(zg) * (e_wz + np.abs(wz))[:, None] + np.abs(gue * w[:, None]) + np.abs(zg * wz[:, None]))
    gvb, gvn, gva, hand_v = (np.zeros((Vg, 3)) for _ in range(4))
    for c in range(3):
        cc = np.concatenate((c_va[:, c], c_vb[:, c]))
        mm = np.concatenate((np.abs(gue[:, c] * (1 - w)) + np.abs(zg[:, c] * (1 - wz)), np.abs(gue[:, c] * w) + np.abs(zg[:, c] * wz)))
        gvb[:, c], gvn[:, c], gva[:, c] = _atomic_budget(Vg, idx, cc, np.concatenate((e_cva[:, c], e_cvb[:, c])), mm)
        hand_v[:, c] = _scatter(Vg, idx, cc)
    out.update(g_vertices_budget=gvb, g_vertices_n=gvn, g_vertices_abs=gva)
    tol = lambda v: 1e-10 * max(float(np.abs(v).max(initial=0)), 1e-300)
    assert np.allclose(hand_sdf, out["g_sdf"], rtol=1e-7, atol=tol(np.concatenate((c_sa, c_sb)))), "hand-derived g_sdf != autograd"
    assert np.allclose(hand_v, out["g_vertices"], rtol=1e-7, atol=tol(c_va)), "hand-derived g_vertices != autograd"
    jump = dict(g_sdf=_scatter(Vg, idx, np.tile(jump_q[kq], 2).astype(np.float64)) > 0)
    jump["g_vertices"] = np.repeat(jump["g_sdf"][:, None], 3, 1)
    if b32 is not None:
        dbt = (gvk * (ue - vd[kq])).sum(-1) / Bk
        m_dbt = np.abs(gvk * (ue - vd[kq])).sum(-1) / Bk
        e_dbt = (e_gvk * np.abs(ue - vd[kq]) + np.abs(gvk) * (e_ue + e_vd[kq] + 2 * (np.abs(ue) + np.abs(vd[kq])) + np.abs(ue - vd[kq]))).sum(-1) / Bk + m_dbt * (rBk + 4)
        gb = dbt * dbt_raw
        e_gb = e_dbt * np.abs(dbt_raw) + m_dbt * e_dbt_raw + 2 * np.abs(gb)
        full, fb, fn, fj = (np.zeros((C, 12)) for _ in range(4))
        full[cube, ke] = gb; fb[cube, ke] = e_gb; fn[cube, ke] = (gb != 0) | (e_gb > 0); fj[cube, ke] = jump_q[kq]
        out.update(g_beta=gr(lb), g_beta_budget=np.where(fn > 0, fb, 0.0), g_beta_n=fn, g_beta_abs=np.abs(full))
        jump["g_beta"] = fj > 0
        assert np.allclose(full, out["g_beta"], rtol=1e-7, atol=tol(gb)), "hand-derived g_beta != autograd"
    if a32 is not None:
        flat = np.concatenate((cube * 8 + ca, cube * 8 + cb))
        cga = np.concatenate((dA * sa, dBq * sb)); m_cga = np.concatenate((m_dw * np.abs(Bq * sa) / den, m_dw * np.abs(A * sb) / den))
        e_cga = np.concatenate((e_dA * np.abs(sa) + np.abs(dA * sa), e_dBq * np.abs(sb) + np.abs(dBq * sb)))
        act_b, act_n, act_a = _atomic_budget(8 * C, flat, cga, e_cga, m_cga)     # fixed order in the kernel; charged as if not
        act = _scatter(8 * C, flat, cga)
        _, _, dall, e_dall = _tanh_act(a32.astype(np.float64).reshape(-1), ws)
        ga = act * dall
        e_ga = act_b * np.abs(dall) + act_a * e_dall + 2 * np.abs(ga)
        out.update(g_alpha=gr(la), g_alpha_budget=np.where(act_n > 0, e_ga, 0.0).reshape(C, 8), g_alpha_n=act_n.reshape(C, 8),
                   g_alpha_abs=np.abs(ga).reshape(C, 8))
        jump["g_alpha"] = (_scatter(8 * C, flat, np.tile(jump_q[kq], 2).astype(np.float64)) > 0).reshape(C, 8)
        assert np.allclose(ga.reshape(C, 8), out["g_alpha"], rtol=1e-7, atol=tol(ga)), "hand-derived g_alpha != autograd"
    if g32 is not None:
        jump["g_gamma"] = np.zeros((C, 1), dtype=bool)
    out["jump"] = jump
    return out


def entropy_budget(sdf, res, v_out=1.0):
    """float64 entropy and its gradient for the cotangent v_out, with budgets: dict(entropy, entropy_budget, g_sdf, g_sdf_budget,
    g_sdf_n, g_sdf_abs).  The kernel sums the float32 terms in double: the value's bound is the mean of the terms' own bounds plus
    the final rounding; the gradient is atomics of k (sigmoid(a) - [b > 0]) with sigmoid - 1 charged by its operands."""
    R0, R1, R2 = (int(r) for r in res)
    s32 = np.asarray(sdf, dtype=np.float32).reshape(-1)
    ls = torch.from_numpy(s32.astype(np.float64)).requires_grad_(True)
    ent = entropy(ls, res)
    v = float(np.float32(v_out))
    (ent * v).backward()
    s = s32.astype(np.float64)
    s1, s2 = R0 + 1, (R0 + 1) * (R1 + 1)
    Vg = s2 * (R2 + 1)
    f = np.arange(Vg)
    second = np.stack((f - s1, f + 1, f + s2), -1)
    i0, i1, i2 = f % s1, (f // s1) % (R1 + 1), f // s2
    exists = np.stack((i1 >= 1, i0 < R0, i2 < R2), -1)
    occ = s < 0
    cross = (exists & (occ[f][:, None] != occ[np.where(exists, second, 0)])).reshape(-1)
    ia, ib = np.repeat(f, 3)[cross], second.reshape(-1)[cross]
    E = ia.size
    xs, ts = np.concatenate((s[ia], s[ib])), np.concatenate((s[ib] > 0, s[ia] > 0)).astype(np.float64)
    lin, soft = np.maximum(xs, 0) - xs * ts, np.log1p(np.exp(-np.abs(xs)))
    e_term = np.maximum(xs, 0) + np.abs(xs * ts) + np.abs(lin) + soft * (2 * R_TANH + 1) + (lin + soft)
    val = (lin + soft).sum() / E
    assert abs(val - ent.item()) <= 1e-12 * max(val, 1.0)
    sig = 1 / (1 + np.exp(-xs))
    k = v / E
    c = k * (sig - ts)
    e_c = np.abs(k) * (sig * (R_TANH + 2) + FLT_MIN_U + np.abs(sig - ts)) + 3 * np.abs(c)
    bud, n, a = _atomic_budget(Vg, np.concatenate((ia, ib)), c, e_c)
    g = ls.grad.numpy()
    assert np.allclose(_scatter(Vg, np.concatenate((ia, ib)), c), g, rtol=1e-9, atol=1e-15)
    return dict(entropy=ent.item(), entropy_budget=float(e_term.sum() / E + val), g_sdf=g, g_sdf_budget=bud, g_sdf_n=n, g_sdf_abs=a, E=E)
