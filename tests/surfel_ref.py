"""Dense float64 torch restatement of the 2D Gaussian splatting path (gsplat 1.4 rasterization_2dgs, packed, one camera): the
yardstick of tests/test_surfel_cpu.py and tests/test_gpu_surfels.py.

Every visible Gaussian is evaluated against every pixel whose tile lies in the Gaussian's tile rectangle, in the order (depth, Gaussian
id); there are no per-tile lists.  Gradients come from autograd.  The discrete decisions (culls, alpha < 1/255, the T stop, the branch
of min(w3, w2), the 0.999 clamp, the normal flip, the tile rectangle) are made on the float64 values and detached, and the margin of
each is returned so that a test can leave out what an fp32 evaluation may decide the other way.

composite_pairs is the same compositor arithmetic (_composite_core) on the per-tile lists a binning made, with every per-Gaussian input
broadcast per pixel, so that autograd returns each (Gaussian, pixel) pair's share of a gradient and the size of what was summed: the
yardstick of tests/test_gpu_surfel_budget.py.
"""
import math

import torch

ALPHA_MIN = 1.0 / 255.0
T_STOP = 1e-4
BAND = 1e-5


def quat_rotation(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def sh_basis(deg, d):
    """real SH basis of 3DGS in gsplat's polynomial form, degrees 0..3, at unit directions d [..., 3]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = [torch.full_like(x, 0.2820947917738781)]
    if deg >= 1:
        b += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if deg >= 2:
        z2, t0b, c1, s1 = z * z, -1.092548430592079 * z, x * x - y * y, 2.0 * x * y
        b += [0.5462742152960395 * s1, t0b * y, 0.9461746957575601 * z2 - 0.3153915652525201, t0b * x, 0.5462742152960395 * c1]
        if deg >= 3:
            t0c, t1b = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
            c2, s2 = x * c1 - y * s1, x * s1 + y * c1
            b += [-0.5900435899266435 * s2, t1b * s1, t0c * y, z * (1.865881662950577 * z2 - 1.119528997770346), t0c * x, t1b * c1,
                  -0.5900435899266435 * c2]
    return torch.stack(b, -1)


def sh_colors(deg, means, campos, coeffs):
    d = means - campos
    d = d / d.norm(dim=-1, keepdim=True)
    c = (sh_basis(deg, d)[..., None] * coeffs[:, :(deg + 1) ** 2, :]).sum(-2)
    return (c + 0.5).clamp_min(0.0)


def tile_rect(mx, my, radius, tile_size, tw, th):
    """(x0, y0, x1, y1) half-open tile rectangle of the square means2d +- radius, clamped to the grid"""
    lo = lambda v, n: torch.floor(v).clamp(0, n).long()
    hi = lambda v, n: torch.ceil(v).clamp(0, n).long()
    r = radius / tile_size
    return lo(mx / tile_size - r, tw), lo(my / tile_size - r, th), hi(mx / tile_size + r, tw), hi(my / tile_size + r, th)


def project(means, quats, scales, viewmat, K, W, H, near=0.01, far=1e10, radius_clip=0.0, tile_size=16):
    """Surfel projection of all N Gaussians (dense, no compaction).  Returns a dict of [N, ...] tensors, `valid` and `margin_bad`
    (a cull, the radius rounding or a tile edge is inside the band)."""
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    R = quat_rotation(quats)
    Rc = Rcw @ R
    c = means @ Rcw.T + t
    Hm = torch.stack((scales[:, 0:1] * Rc[:, :, 0], scales[:, 1:2] * Rc[:, :, 1], c), dim=-1)
    M = K @ Hm                                                   # [N,3,3], rows M0, M1, M2
    M0, M1, M2 = M[:, 0], M[:, 1], M[:, 2]
    test = torch.tensor([1.0, 1.0, -1.0], dtype=means.dtype)
    d = (test * M2 * M2).sum(-1)
    dsafe = torch.where(d == 0, torch.ones_like(d), d)
    f = test / dsafe[:, None]
    means2d = torch.stack(((f * M0 * M2).sum(-1), (f * M1 * M2).sum(-1)), dim=-1)
    ext = means2d ** 2 - torch.stack(((f * M0 * M0).sum(-1), (f * M1 * M1).sum(-1)), dim=-1)
    with torch.no_grad():
        pre = 3.0 * torch.sqrt(ext.max(dim=-1).values.clamp_min(1e-4))
        radius = torch.ceil(pre)
        mx, my = means2d[:, 0], means2d[:, 1]
        depth_ok = (c[:, 2] >= near) & (c[:, 2] <= far)
        on = (mx + radius > 0) & (mx - radius < W) & (my + radius > 0) & (my - radius < H)
        valid = depth_ok & (d != 0) & (radius > radius_clip) & on
        flip = (Rc[:, :, 2] * c).sum(-1) > 0
        tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
        rect = torch.stack(tile_rect(mx, my, radius, tile_size, tw, th), dim=-1)
        rect_lo = torch.stack(tile_rect(mx, my, (radius - 1).clamp_min(0), tile_size, tw, th), dim=-1)
        rect_hi = torch.stack(tile_rect(mx, my, radius + 1, tile_size, tw, th), dim=-1)
        rel = lambda a, b: (a - b).abs() <= BAND * torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
        z = c[:, 2]
        cull_bad = rel(z, torch.full_like(z, near)) | rel(z, torch.full_like(z, far)) | (d.abs() <= BAND * (M2 * M2).sum(-1))
        cull_bad |= depth_ok & (rel(mx + radius, torch.zeros_like(mx)) | rel(mx - radius, torch.full_like(mx, W))
                                | rel(my + radius, torch.zeros_like(mx)) | rel(my - radius, torch.full_like(mx, H))
                                | ((mx + radius).abs() <= BAND * radius) | ((my + radius).abs() <= BAND * radius))
        radius_bad = (pre - torch.round(pre)).abs() <= BAND * pre              # ceil may go either way
        edges = torch.stack((mx - radius, mx + radius, my - radius, my + radius), -1) / tile_size
        grid = torch.tensor([tw, tw, th, th], dtype=edges.dtype)
        on_grid = (torch.round(edges) >= 0) & (torch.round(edges) <= grid)     # beyond it the clamp decides, not the rounding
        edge_bad = (on_grid & ((edges - torch.round(edges)).abs() <= BAND * edges.abs().clamp_min(1.0))).any(-1)
    normals = torch.where(flip[:, None], -Rc[:, :, 2], Rc[:, :, 2])
    return dict(M=M, means2d=means2d, depths=c[:, 2], normals=normals, radii=radius.long(), valid=valid, rect=rect, rect_lo=rect_lo,
                rect_hi=rect_hi, cull_bad=cull_bad & depth_ok, radius_bad=radius_bad & valid, edge_bad=edge_bad & valid)


def _composite_core(M, means2d, opacities, colors, normals, member, px, py, depths_channel, distloss, background, taps=None):
    """The compositor's arithmetic on ONE ordered list: dim 0 walks the list front to back, dim 1 the P pixels that share it.  Every
    per-Gaussian tensor carries a pixel axis of length P or 1 (M [L,P|1,3,3], means2d [L,P|1,2], opacities [L,P|1], colors [L,P|1,C],
    normals [L,P|1,3]): with length 1 this is the dense compositor, with length P every (Gaussian, pixel) pair has inputs of its own
    and autograd returns the gradient pair by pair.  member [L,P]: the pair is in the pixel's list.  taps: zero leaves ([L,P], [L,P], [L,P,3]) added
    to alpha where it weighs the pair's own contribution, to alpha where it dims everything behind, and to hu x hv; their gradients
    are dL/dalpha along either route and dL/dz.  Returns flat [P, ...] images, the last active list position per pixel (-1: none), the decision margins and the raw
    branch counts."""
    V, P = member.shape
    dt = M.dtype
    # hu, hv and their cross product cancel for a thin, grazing or close surfel.  The kernels keep the products of these two steps
    # exact (explicit FMAs, a compensated difference of products); so does this, whatever the dtype: formed in float64 and rounded
    # once (a no-op when dt is float64)
    wide, pxw, pyw = M.double(), px.double()[None, :, None], py.double()[None, :, None]
    hu = (pxw * wide[:, :, 2] - wide[:, :, 0]).to(dt)                                        # [L,P,3]
    hv = (pyw * wide[:, :, 2] - wide[:, :, 1]).to(dt)
    z = torch.cross(hu.double(), hv.double(), dim=-1).to(dt)
    if taps is not None:
        z = z + taps[2]
    zz_ok = z[..., 2] != 0
    zz = torch.where(zz_ok, z[..., 2], torch.ones_like(z[..., 2]))
    sx, sy = z[..., 0] / zz, z[..., 1] / zz
    w3 = sx * sx + sy * sy
    w2 = 2.0 * ((means2d[..., 0] - px[None]) ** 2 + (means2d[..., 1] - py[None]) ** 2)
    ray = (w3 < w2).detach()
    sigma = 0.5 * torch.where(ray, w3, w2)
    raw = opacities * torch.exp(-sigma)
    clamped = (raw > 0.999).detach()
    alpha = torch.where(clamped, torch.full_like(raw, 0.999), raw)
    with torch.no_grad():
        contrib = member & zz_ok & (sigma >= 0) & (alpha >= ALPHA_MIN)
        a0 = torch.where(contrib, alpha, torch.zeros_like(alpha))
        Tn = torch.cumprod(1.0 - a0, dim=0)
        active = contrib & (Tn > T_STOP)
        # margins, only where the decision can matter: inside the list and before the pixel has stopped
        T_before0 = torch.cat((torch.ones(1, P, dtype=dt), Tn[:-1]), dim=0) if V > 0 else Tn
        live = member & zz_ok & (T_before0 > T_STOP * (1 + BAND))
        alpha_bad = live & ((alpha - ALPHA_MIN).abs() <= BAND * ALPHA_MIN)
        stop_bad = contrib & (T_before0 > T_STOP) & ((Tn - T_STOP).abs() <= BAND * T_STOP)
        branch_bad = active & ((w3 - w2).abs() <= BAND * torch.maximum(w3, w2))
        clamp_bad = active & ((raw - 0.999).abs() <= BAND)
        pix_bad = (alpha_bad | stop_bad | branch_bad | clamp_bad).any(0)
        pos = torch.arange(V)[:, None].expand(V, P)
        last = torch.where(active, pos, torch.full_like(pos, -1)).max(0).values if V > 0 else torch.full((P,), -1)
    a = torch.where(active, alpha, torch.zeros_like(alpha))
    a_own, a_dim = (a, a) if taps is None else (a + taps[0], a + taps[1])
    Tc = torch.cumprod(1.0 - a_dim, dim=0)
    T_before = torch.cat((torch.ones(1, P, dtype=dt), Tc[:-1]), dim=0) if V > 0 else Tc
    vis = a_own * T_before                                                                   # [L,P]
    T_final = Tc[-1] if V > 0 else torch.ones(P, dtype=dt)
    weigh = lambda t: vis.T @ t[:, 0] if t.shape[1] == 1 else (vis[..., None] * t).sum(0)    # [P,.]
    render, nrm = weigh(colors), weigh(normals)
    out = {}
    if depths_channel:
        d = colors[..., -1]                                                                  # [L,P|1]
        if distloss:
            vd = vis * d
            D_before = torch.cumsum(vd, dim=0) - vd
            out["distort"] = (2.0 * (vd * (1.0 - T_before) - vis * D_before)).sum(0)
        with torch.no_grad():
            med_ok = active & (T_before > 0.5)
            idx = torch.where(med_ok, pos, torch.full_like(pos, -1)).max(0).values if V > 0 else torch.full((P,), -1)
            out["median"] = torch.where(idx >= 0, d.detach().expand(V, P).gather(0, idx.clamp_min(0)[None])[0], torch.zeros(P, dtype=dt)) \
                if V > 0 else torch.zeros(P, dtype=dt)
            out["median_bad"] = (active & ((T_before - 0.5).abs() <= BAND * 0.5)).any(0)
    if background is not None:
        nc = colors.shape[-1] - (1 if depths_channel else 0)
        pad = torch.cat((background[:nc].to(dt), torch.zeros(colors.shape[-1] - nc, dtype=dt)))
        render = render + T_final[:, None] * pad
    counts = dict(n_active=active.sum().item(), n_ray=(active & ray).sum().item(), n_lowpass=(active & ~ray).sum().item(),
                  n_clamped=(active & clamped).sum().item(), n_clamped_ray=(active & clamped & ray).sum().item(),
                  n_clamped_lowpass=(active & clamped & ~ray).sum().item(), n_skipped=(member & zz_ok & (alpha < ALPHA_MIN)).sum().item())
    out.update(render=render, alpha=1.0 - T_final, normals=nrm, pix_bad=pix_bad, last=last, counts=counts, hu=hu.detach(), hv=hv.detach())
    return out


def _abs_cross(a, b):
    """the sizes of the terms of a x b: |a1 b2| + |a2 b1|, ..."""
    a, b = a.abs(), b.abs()
    return torch.stack((a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), dim=-1)


def _branch_report(counts):
    """the branch figures both compositor restatements report, from the raw counts of _composite_core"""
    n_act = counts["n_active"]
    return dict(ray_frac=counts["n_ray"] / max(n_act, 1), lowpass_frac=counts["n_lowpass"] / max(n_act, 1), n_clamped=counts["n_clamped"],
                n_clamped_ray=counts["n_clamped_ray"], n_clamped_lowpass=counts["n_clamped_lowpass"], n_skipped=counts["n_skipped"],
                n_active=n_act)


def _pixel_centres(xs, ys, dt):
    return xs.reshape(-1).to(dt) + 0.5, ys.reshape(-1).to(dt) + 0.5


def composite(M, means2d, opacities, colors, normals, depths_channel, rect, W, H, tile_size=16, distloss=False, background=None,
              order_key=None):
    """Dense compositor over the V Gaussians given (already the visible ones).  colors [V,C]; depths_channel: the last colour channel is
    the depth (distortion and median use it).  order_key [V]: sort key (depth); ties keep the given order.  Returns a dict of images and
    the decision margins."""
    V = M.shape[0]
    order = torch.argsort(order_key.detach(), stable=True) if V > 0 else torch.zeros(0, dtype=torch.long)
    M, means2d, opacities, colors, normals, rect = M[order], means2d[order], opacities[order], colors[order], normals[order], rect[order]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    px, py = _pixel_centres(xs, ys, M.dtype)                                                 # [P]
    tx, ty = xs.reshape(-1) // tile_size, ys.reshape(-1) // tile_size
    in_rect = (tx[None] >= rect[:, 0:1]) & (tx[None] < rect[:, 2:3]) & (ty[None] >= rect[:, 1:2]) & (ty[None] < rect[:, 3:4])   # [V,P]
    co = _composite_core(M[:, None], means2d[:, None], opacities[:, None], colors[:, None], normals[:, None], in_rect, px, py,
                         depths_channel, distloss, background)
    out = {k: co[k].reshape(H, W) for k in ("distort", "median", "median_bad") if k in co}
    out.update(render=co["render"].reshape(H, W, -1), alpha=co["alpha"].reshape(H, W), normals=co["normals"].reshape(H, W, 3),
               pix_bad=co["pix_bad"].reshape(H, W), order=order, **_branch_report(co["counts"]))
    return out


PACKED_COLUMNS = 15          # M 0..8, means2d 9..10, opacity 11, normal 12..14; colours from 15


def composite_pairs(M, means2d, opacities, colors, normals, depths_channel, distloss, background, flatten_ids, offsets, W, H, tile_size,
                    cotangents=(), keep=None):
    """The compositor restated PAIR BY PAIR, on the lists the binning made: tile t composites flatten_ids[offsets[t] : offsets[t+1]] in
    that order (the last tile ends at len(flatten_ids)).  Per tile, every per-Gaussian input is broadcast to an explicit [L, P, ...]
    leaf, _composite_core -- the arithmetic of composite() -- runs on the leaves, and one backward per cotangent set leaves in
    grad[l, p] pixel p's contribution to the gradient of list entry l.  Nothing of the kernel's hand-derived backward is restated.

    Inputs in one dtype (float64: the yardstick; float32: what tests/test_surfel_cpu.py measures the constant from): M [V,3,3] or
    [V,9], means2d [V,2], opacities [V], colors [V,C] (the depth in the last channel if depths_channel), normals [V,3], background [3]
    or None.  cotangents: sets (v_render [H,W,C], v_alpha [H,W], v_normals [H,W,3], v_distort [H,W] or None); each is masked by `keep`
    [H,W] bool, by default the pixels outside this run's own decision bands.

    Returns the images (render, alpha, normals, distort, median; [H,W,...]), last_ids [H,W] (index into flatten_ids of the last active
    entry, -1: none), pix_bad, median_bad, keep, the branch figures of composite(), list_len [tiles] and `grads`: per cotangent set
    (want, B, B_plain), each [V, 15 + C] in the packed layout.  want = sum_p grad[v, p].  B_plain = sum_p |grad[v, p]|: the size of what
    is summed over the pixels, and nothing else.

    B is wider.  B_plain takes each pair's gradient as one exactly known number, and it is not: the restatement's own graph forms it
    from terms of either sign, and when they cancel, the pair's gradient carries the rounding of the terms, not of their small sum.
    Under the sparse cotangents, where one pair is a whole element, the float32 restatement itself then stands at ratios of 10^3 to
    5 * 10^5 of 2^-24 B_plain on 'clamp' and 'outside' (among a few thousand pairs one cancels to a thousandth), whatever the scene.
    B sums, per pair, the sizes of the terms instead, at the four places where the graph adds within a pair:
      (1) the images: an element is the sum of what render, alpha, normals and distort send to it, each a rounded sum of its own:
          |g_render| + |g_alpha| + |g_normals| + |g_distort|, one backward each, in every column;
      (2) dL/dalpha = own + behind: alpha weighs the pair's own contribution (vis = alpha T) and dims everything behind it (T of the
          later entries).  The two are computed apart -- one from this entry's colours, the other a sum over the later entries -- and
          have opposite signs wherever the pair's colour resembles what lies behind.  Every gradient of the pair that runs through
          alpha (M, means2d, opacity) is dL/dalpha times a factor, so its size is scaled by (|own| + |behind|) / |own + behind| >= 1;
      (3) dL/dhu = hv x dL/dz and dL/dhv = dL/dz x hu: each component is a difference of two products, which cancels for a surfel seen
          at a grazing angle: |a1 b2| + |a2 b1| in place of |a1 b2 - a2 b1| (rows M0 and M1 are -dL/dhu and -dL/dhv);
      (4) the row M2 = px dL/dhu + py dL/dhv: |px| size(dL/dhu) + |py| size(dL/dhv).
    The normal and colour columns are vis times the cotangent and get (1) only.  B >= B_plain always; how much wider it is, and how
    the elements stand against B_plain, is reported and capped by the tests (tests.util.SURFEL_PLAIN_P99_KAPPA)."""
    V, dt = M.shape[0], M.dtype
    C = colors.shape[1]
    M = M.reshape(V, 3, 3)
    flatten_ids, offsets = flatten_ids.long().reshape(-1), offsets.long().reshape(-1)
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    assert offsets.numel() == tw * th
    ends = torch.cat((offsets[1:], torch.tensor([flatten_ids.numel()])))
    img = dict(render=torch.zeros(H, W, C, dtype=dt), alpha=torch.zeros(H, W, dtype=dt), normals=torch.zeros(H, W, 3, dtype=dt),
               pix_bad=torch.zeros(H, W, dtype=torch.bool), last_ids=torch.full((H, W), -1, dtype=torch.long))
    if depths_channel:
        img.update(median=torch.zeros(H, W, dtype=dt), median_bad=torch.zeros(H, W, dtype=torch.bool))
        if distloss:
            img["distort"] = torch.zeros(H, W, dtype=dt)
    grads = [tuple(torch.zeros(V, PACKED_COLUMNS + C, dtype=dt) for _ in range(3)) for _ in cotangents]
    counts = {}
    for t in range(tw * th):
        ty, tx = divmod(t, tw)
        ys, xs = torch.meshgrid(torch.arange(ty * tile_size, min((ty + 1) * tile_size, H)),
                                torch.arange(tx * tile_size, min((tx + 1) * tile_size, W)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        px, py = _pixel_centres(xs, ys, dt)
        ids = flatten_ids[offsets[t]:ends[t]]
        L, P = ids.numel(), xs.numel()
        spread = lambda a: a.detach()[ids][:, None].expand(L, P, *a.shape[1:]).clone().requires_grad_(len(cotangents) > 0)
        leaves = dict(M=spread(M), means2d=spread(means2d), opacities=spread(opacities), normals=spread(normals), colors=spread(colors))
        taps = [torch.zeros(L, P, *tail, dtype=dt, requires_grad=len(cotangents) > 0) for tail in ((), (), (3,))]
        co = _composite_core(leaves["M"], leaves["means2d"], leaves["opacities"], leaves["colors"], leaves["normals"],
                             torch.ones(L, P, dtype=torch.bool), px, py, depths_channel, distloss, background, taps)
        for k, v in co["counts"].items():
            counts[k] = counts.get(k, 0) + v
        for k in ("render", "alpha", "normals", "distort", "median", "median_bad", "pix_bad"):
            if k in co:
                img[k][ys, xs] = co[k].detach()
        img["last_ids"][ys, xs] = torch.where(co["last"] >= 0, co["last"] + offsets[t], co["last"])
        kp = (~co["pix_bad"] if keep is None else keep[ys, xs]).to(dt)
        for (want, B, B_plain), (v_render, v_alpha, v_normals, v_distort) in zip(grads, cotangents):
            at = lambda v: v[ys, xs].to(dt) * (kp if v.dim() == 2 else kp[:, None])
            terms = [(co["render"], at(v_render)), (co["alpha"], at(v_alpha)), (co["normals"], at(v_normals))]
            if distloss:
                terms.append((co["distort"], at(v_distort)))
            names = ("M", "means2d", "opacities", "normals", "colors")                           # the packed layout
            whole = torch.zeros(L, P, PACKED_COLUMNS + C, dtype=dt)
            for image, cot in terms:                                                             # (1): one backward per image
                loss = (image * cot).sum()
                if L == 0 or not loss.requires_grad or not bool((cot != 0).any()):
                    continue
                g = torch.autograd.grad(loss, [leaves[k] for k in names] + taps, retain_graph=True, allow_unused=True)
                g = [torch.zeros_like(a) if x is None else x for x, a in zip(g, [leaves[k] for k in names] + taps)]
                g_M, g_means2d, g_opacity, g_normal, g_colors, g_own, g_behind, g_z = g
                total = (g_own + g_behind).abs()                                                 # (2)
                cancel = torch.where(total > 0, (g_own.abs() + g_behind.abs()) / total, torch.ones_like(total))[..., None]
                size_hu, size_hv = _abs_cross(co["hv"], g_z), _abs_cross(g_z, co["hu"])          # (3)
                size_row2 = px[None, :, None].abs() * size_hu + py[None, :, None].abs() * size_hv    # (4)
                sizes = torch.cat((size_hu, size_hv, size_row2, g_means2d.abs(), g_opacity.abs()[..., None]), dim=-1) * cancel
                packed = torch.cat((g_M.reshape(L, P, 9), g_means2d, g_opacity[..., None], g_normal, g_colors), dim=-1)
                whole += packed
                want.index_add_(0, ids, packed.sum(1))
                B.index_add_(0, ids, torch.cat((sizes, g_normal.abs(), g_colors.abs()), dim=-1).sum(1))
            B_plain.index_add_(0, ids, whole.abs().sum(1))
    out = dict(img)
    out.update(keep=~img["pix_bad"] if keep is None else keep, grads=grads, list_len=ends - offsets, **_branch_report(counts))
    return out


def packed_groups(C):
    """(name, first column, end) of the gradients in the packed layout"""
    return (("v_M", 0, 9), ("v_means2d", 9, 11), ("v_opacity", 11, 12), ("v_normal", 12, 15), ("v_colors", 15, 15 + C))


def plain_ratio_medians(err, B_plain, C, eps=2.0 ** -24):
    """per gradient of the packed layout, the median over its elements with B_plain > 0 of err / (eps B_plain): where an
    implementation stands against the plain absolute sum, which composite_pairs' B widens.  A gradient with fewer than 64 such elements reports 0.0: there a handful of pairs,
    each with a cancellation of its own, is the whole sample (the few low-pass pairs of a stack scene in v_means2d)"""
    out = {}
    for name, a, b in packed_groups(C):
        e, p = torch.as_tensor(err)[:, a:b].double(), torch.as_tensor(B_plain)[:, a:b].double()
        out[name] = float((e[p > 0] / (eps * p[p > 0])).median()) if int((p > 0).sum()) >= 64 else 0.0
    return out


def build_lists(rect, depths, tw, th):
    """flatten_ids and tile offsets as the binning makes them, from the tile rectangles [V,4] and depths [V] of the visible Gaussians:
    tile by tile (row-major), each list in the order (depth, index)"""
    order = torch.argsort(depths.detach(), stable=True)
    r = rect[order]
    ids, offsets = [], []
    n = 0
    for ty in range(th):
        for tx in range(tw):
            m = (tx >= r[:, 0]) & (tx < r[:, 2]) & (ty >= r[:, 1]) & (ty < r[:, 3])
            offsets.append(n)
            ids.append(order[m])
            n += int(m.sum())
    return torch.cat(ids) if ids else torch.zeros(0, dtype=torch.long), torch.tensor(offsets, dtype=torch.long)


def depth_to_normal(depth, viewmat, K):
    """gsplat's depth_to_normal on [H,W,1] z-depths -> world normals [H,W,3], zero on the border"""
    H, W = depth.shape[:2]
    dt = depth.dtype
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt) + 0.5, torch.arange(W, dtype=dt) + 0.5, indexing="ij")
    dirs = torch.stack(((xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], torch.ones_like(xs)), -1)
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    P = -(Rcw.T @ t) + depth * (dirs @ Rcw)
    dx = P[2:, 1:-1] - P[:-2, 1:-1]
    dy = P[1:-1, 2:] - P[1:-1, :-2]
    n = torch.cross(dx, dy, dim=-1)
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    out = torch.zeros(H, W, 3, dtype=dt)
    out[1:-1, 1:-1] = n
    return out


def rasterization_2dgs(means, quats, scales, opacities, colors, viewmat, K, W, H, *, near=0.01, far=1e10, radius_clip=0.0, sh_degree=None,
                       tile_size=16, background=None, render_mode="RGB", distloss=False):
    """The whole call on float64 tensors (viewmat [4,4], K [3,3]).  Returns a dict: ids, radii, means2d, depths, ray_transforms (the
    tensor the compositor consumed: retain_grad() is set, its .grad is the compositor's dL/dM), normals_cam, render [H,W,D] (expected
    depth in the ED modes), alpha [H,W], normals [H,W,3] (world), normals_from_depth, distort, median, and the margins: pix_bad [H,W],
    gauss_bad [N] (cull / radius decisions), edge_bad [N] (a tile edge of the square is inside the band: the tile count of that Gaussian
    is undecided, its images are covered by pix_bad), ray_frac / lowpass_frac / n_clamped (_ray / _lowpass) / n_skipped."""
    assert render_mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED")
    depth_channel = render_mode != "RGB"
    pr = project(means, quats, scales, viewmat, K, W, H, near, far, radius_clip, tile_size)
    ids = torch.nonzero(pr["valid"]).reshape(-1)
    M = pr["M"][ids]
    Mc = M.clone()
    if Mc.requires_grad:
        Mc.retain_grad()
    depths = pr["depths"][ids]
    if render_mode in ("D", "ED"):
        cols = depths[:, None]
    else:
        if sh_degree is not None:
            campos = -(viewmat[:3, :3].T @ viewmat[:3, 3])
            cols = sh_colors(sh_degree, means[ids], campos, colors[ids])
        else:
            cols = colors[ids]
        if depth_channel:
            cols = torch.cat((cols, depths[:, None]), dim=-1)
    co = composite(Mc, pr["means2d"][ids], opacities[ids], cols, pr["normals"][ids], depth_channel, pr["rect"][ids], W, H, tile_size,
                   distloss, background, order_key=depths)
    render, alpha = co["render"], co["alpha"]
    nfd = None
    if render_mode in ("ED", "RGB+ED"):
        render = torch.cat((render[..., :-1], render[..., -1:] / alpha[..., None].clamp_min(1e-10)), dim=-1)
        nfd = depth_to_normal(render[..., -1:], viewmat, K)
    # pixels a Gaussian with an undecided cull, radius or tile edge may or may not reach
    with torch.no_grad():
        tw = (W + tile_size - 1) // tile_size
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        tx, ty = xs // tile_size, ys // tile_size
        pix_bad = co["pix_bad"].clone()
        gauss_bad = pr["cull_bad"] | pr["radius_bad"]
        for g in torch.nonzero(pr["cull_bad"] | pr["edge_bad"]).reshape(-1).tolist():
            x0, y0, x1, y1 = pr["rect_hi"][g].tolist()
            pix_bad |= (tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1)
        for g in torch.nonzero(pr["radius_bad"]).reshape(-1).tolist():
            x0, y0, x1, y1 = pr["rect_hi"][g].tolist()
            a0, b0, a1, b1 = pr["rect_lo"][g].tolist()
            hi = (tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1)
            lo = (tx >= a0) & (tx < a1) & (ty >= b0) & (ty < b1)
            pix_bad |= hi & ~lo
    out = dict(co)
    out.update(ids=ids, radii=pr["radii"][ids], means2d=pr["means2d"][ids], depths=depths, ray_transforms=Mc, normals_cam=pr["normals"][ids],
               render=render, alpha=alpha, normals=co["normals"] @ viewmat[:3, :3], normals_from_depth=nfd, pix_bad=pix_bad,
               gauss_bad=gauss_bad, edge_bad=pr["edge_bad"], rect=pr["rect"][ids], colors=cols)
    return out


def fronto_parallel_alpha(delta2, s, f, z, o):
    """closed form for a surfel of scales (s, s) facing the camera on the optical axis at depth z: alpha at squared pixel distance
    delta2 from its centre"""
    return o * math.exp(-0.5 * min(delta2 / (s * f / z) ** 2, 2.0 * delta2))


# ------------------------------------------------------------------------------------------------ the scenes of the GPU tests
def make_scene(name, n=1500, seed=None, min_facing=0.0):
    """Inputs shared by tests/test_surfel_cpu.py (which checks the exclusion caps on the restatement alone) and
    tests/test_gpu_surfels.py: random surfels with anisotropic extents (many thin ones, so that the low-pass branch wins on many
    pixels), opacities from ~0 (always below 1/255) to 1 (the 0.999 clamp), degree-2 SH colours.
    How thin: the compositor reads the ray transform M as fp32, so hu = p.x M2 - M0 carries an absolute error of about
    eps |M0| (eps = 6e-8, |M0| ~ depth * pixel coordinate ~ 200 here), and the surfel coordinate across the thin axis, z / z.z, divides it
    by f * s1.  An error of 1e-5 in that coordinate, i.e. 3e-5 in sigma at the |v| <= 3.3 where alpha >= 1/255, needs f * s1 >= 1.2:
    with f = 60 and extents of 0.1 .. 0.16, a minor-axis factor of 0.15.  Such a surfel is 0.3 .. 0.5 pixels wide at depth 3 -- below
    the 0.7 pixels under which the low-pass branch wins -- and a thinner one cannot meet 1e-4 in fp32 with any kernel.
      'inside'   100 x 75, camera inside the cloud (near plane 0.1): near-plane and frustum culls, surfels on either side of d = 0
      'outside'  64 x 48 from outside"""
    if name == "clamp":
        return make_clamp_scene()
    if name in STACK_SCENES:
        return make_stack_scene(*STACK_SCENES[name])
    from geosplatting_amd.cameras import Camera, lookat_c2w
    from geosplatting_amd.synthetic import random_splats
    seed = {"inside": 3, "outside": 1}[name] if seed is None else seed      # (seeds inside the exclusion caps: test_surfel_cpu.py)
    sp = random_splats(n, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    scales = sp.scales.exp() * torch.cat((0.6 + torch.rand(n, 1, generator=g), 0.15 + 0.8 * torch.rand(n, 1, generator=g) ** 2,
                                          torch.ones(n, 1)), dim=-1)
    u = torch.rand(n, generator=g)
    opac = torch.where(u < 0.15, 0.004 * torch.rand(n, generator=g), torch.where(u > 0.8, torch.ones(n) + 0 * torch.rand(n, generator=g),
                                                                                torch.rand(n, generator=g)))
    sh = torch.cat((torch.rand(n, 1, 3, generator=g) * 2 - 1, 0.3 * torch.randn(n, 8, 3, generator=g)), dim=1)
    if name == "inside":
        W, H, f = 100, 75, 70.0
        eye, target = torch.tensor([0.12, -0.07, -0.35]), torch.tensor([0.0, 0.1, 0.6])
    else:
        W, H, f = 64, 48, 60.0
        eye, target = torch.tensor([1.9, 1.1, -2.2]), torch.tensor([0.0, 0.0, 0.0])
    cam = Camera(lookat_c2w(eye, target, torch.tensor([0.0, 1.0, 0.0])), f, f, W * 0.5, H * 0.5, W, H)
    if min_facing > 0:
        # Surfels seen edge-on are taken out of the view (opacity below 1/255): hu x hv cancels for them, the relative error of alpha
        # and of every gradient of the pair grows with 1 / cos, and under sparse cotangents, where one pair is a whole element, the
        # float32 restatement alone then misses the per-element bound of SURFEL_BUDGET_KAPPA (ratio 296 at |cos| = 0.04).
        to_surfel = sp.means - eye
        facing = (quat_rotation(sp.quats)[:, :, 2] * to_surfel).sum(-1).abs() / to_surfel.norm(dim=-1)
        opac = torch.where(facing < min_facing, torch.full_like(opac, 0.002), opac)
    return dict(means=sp.means, quats=sp.quats, scales=scales, opacities=opac, sh=sh, viewmat=cam.view_matrix, K=cam.intrinsic_matrix,
                W=W, H=H, sh_degree=2, background=torch.tensor([0.3, 0.6, 0.1]), near=0.1 if name == "inside" else 0.01)


def make_clamp_scene():
    """Ten hand-placed surfels on 32 x 32 (2 x 2 tiles, identity view) that force the min(0.999, .) clamp on both branches, which
    the random scenes reach on a handful of contributions only.  With opacity 1 the clamp needs sigma < 1e-3:
      ray branch       one surfel of 40 x 32 pixels (one sigma) at depth 3: w3 < 2e-3 within 0.045 sigma of its centre, about 8 pixels;
      low-pass branch  four surfels 0.3 pixels wide in front of it, each centred 0.01 pixels off a pixel centre along its thin axis,
                       so w2 = 2e-4 there against w3 = 1.1e-3: one clamped pixel each.
    Three half-transparent surfels in front make T < 1 where the clamped ones are reached, one opaque surfel lies behind.  Plain
    [n,3] colours (key 'sh', sh_degree None).  The thin axis keeps f * s1 = 0.6 pixel-depths (the floor derived in make_scene, with
    |M0| ~ 64 here)."""
    W = H = 32
    f = 40.0
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    ray = lambda x, y, z: [(x - W / 2) / f * z, (y - H / 2) / f * z, z]
    means, quats, scales, opac = [], [], [], []

    def add(px, py, z, q, s0, s1, o):
        means.append(ray(px, py, z)); quats.append(q); scales.append([s0, s1, 1.0]); opac.append(o)
    add(12.5, 18.5, 3.0, [0.98, 0.12, -0.1, 0.08], 3.0, 2.4, 1.0)                  # the large one: ray-branch clamp round (12.5, 18.5)
    for (x, y), th in zip(((5, 6), (22, 4), (26, 21), (9, 27)), (0.0, 0.9, -1.3, 2.2)):
        # thin ones, facing the camera (their means2d is then the projected centre) and turned by th in the image plane; the centre lies
        # 0.01 pixels off the centre of pixel (x, y) along the thin axis: low-pass clamp on that pixel
        add(x + 0.5 - 0.01 * math.sin(th), y + 0.5 + 0.01 * math.cos(th), 2.0, [math.cos(th / 2), 0.0, 0.0, math.sin(th / 2)], 0.47, 0.015, 1.0)
    add(11.2, 17.1, 1.5, [0.9, 0.3, 0.1, 0.2], 0.15, 0.1, 0.5)                     # half-transparent, over the clamped pixels
    add(6.3, 6.9, 1.4, [0.7, -0.2, 0.4, 0.1], 0.12, 0.2, 0.35)
    add(24.6, 20.2, 1.6, [0.8, 0.1, -0.3, 0.5], 0.2, 0.08, 0.6)
    add(20.4, 12.7, 4.0, [0.95, 0.2, 0.2, 0.0], 0.6, 0.4, 1.0)                     # behind the large one
    add(16.0, 16.0, 5.0, [1.0, 0.0, 0.0, 0.0], 0.3, 0.3, 0.002)                    # always below 1/255
    n = len(means)
    g = torch.Generator().manual_seed(5)
    return dict(means=torch.tensor(means), quats=torch.tensor(quats), scales=torch.tensor(scales), opacities=torch.tensor(opac),
                sh=torch.rand(n, 3, generator=g), viewmat=torch.eye(4), K=K, W=W, H=H, sh_degree=None,
                background=torch.tensor([0.3, 0.6, 0.1]), near=0.01)


STACK_SCENES = dict(stack256=(256, False), stack257=(257, False), stack600=(600, False), stack_stop=(600, True))
STACK_W, STACK_H = 37, 27


def make_stack_scene(L, stop=False):
    """L surfels that each cover the whole of a 37 x 27 image (identity view, plain [n,3] colours): every tile's list has length
    exactly L at either tile size, so the batch edges of both compositor kernels are hit by construction -- 256 / 257 / 600 are one
    batch, one batch and one record, and three batches of 256 at tile 16; 4, 4 + 1 and 10 batches of 64 at tile 8.  The image is ragged
    at both sizes (3 x 2 tiles of 16 with a last column 5 and a last row 11 pixels wide; 5 x 4 tiles of 8 with 5 and 3).
    Each surfel is 45 .. 60 pixels wide (one sigma), centred within 3 pixels of the image centre, tilted by up to 0.2 rad about a random
    in-plane axis, at a depth of its own in 2 .. 5 (ids are shuffled against the depth order).  Opacity 0.02 (L <= 257: 0.98^257 =
    5.6e-3) or 0.012 (L = 600: 0.988^600 = 7.1e-4): alpha stays between 0.010 and 0.020, far from 1/255, and T above 1e-4 to the
    end of every list, so every pixel's last_ids is the list's last entry.
    stop: 586 such surfels and 14 of opacity 0.9 (below the 0.999 clamp: with it, 1 / (1 - alpha) = 1000 and the float32 restatement
    alone cannot hold the per-element bound of SURFEL_BUDGET_KAPPA): ten 14 pixels wide over the centre of tile (0, 0) of 16, among the
    first 40 of the order -- every pixel of that tile stops in the first batch while its list has three, at the far corner of the image
    they take a tenth each and the walk goes to the end; and two piles of two, 2.5 pixels wide, at mid-depth in tile (1, 1): pixels of
    one tile stop at different depths."""
    W, H, f = STACK_W, STACK_H, 40.0
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    g = torch.Generator().manual_seed(L + (7 if stop else 0))
    rnd = lambda *s: torch.rand(*s, generator=g)
    n = L
    depth_rank = torch.randperm(n, generator=g)                       # id -> place in the depth order
    z = 2.0 + 3.0 * (depth_rank.float() + 0.5) / n
    cx, cy = W / 2 + 6 * rnd(n) - 3, H / 2 + 6 * rnd(n) - 3
    sig = 45.0 + 15.0 * rnd(n, 2)                                     # pixels
    opac = torch.full((n,), 0.012 if L > 257 else 0.02)
    tilt, axis, spin = 0.4 * rnd(n) - 0.2, 6.2831853 * rnd(n), 6.2831853 * rnd(n)
    if stop:
        big = torch.nonzero((depth_rank >= 5) & (depth_rank < 40)).reshape(-1)[:10]
        small = torch.nonzero((depth_rank >= 280) & (depth_rank < 300)).reshape(-1)[:4]
        cx[big], cy[big] = 8.0 + rnd(10) - 0.5, 8.0 + rnd(10) - 0.5
        sig[big] = 14.0
        cx[small], cy[small] = torch.tensor([21.3, 21.4, 27.6, 27.5]), torch.tensor([19.4, 19.5, 22.7, 22.6])
        sig[small] = 2.5
        opac[big], opac[small] = 0.9, 0.9
        tilt[small] = 0.0
    # rotation: spin about z, then a tilt about the in-plane axis (cos axis, sin axis, 0)
    half = lambda ang, ax: torch.cat((torch.cos(ang / 2)[:, None], torch.sin(ang / 2)[:, None] * ax), dim=-1)
    qmul = lambda a, b: torch.stack((a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(-1),
                                     a[:, 0] * b[:, 1] + b[:, 0] * a[:, 1] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                                     a[:, 0] * b[:, 2] + b[:, 0] * a[:, 2] + a[:, 3] * b[:, 1] - a[:, 1] * b[:, 3],
                                     a[:, 0] * b[:, 3] + b[:, 0] * a[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]), dim=-1)
    q_tilt = half(tilt, torch.stack((torch.cos(axis), torch.sin(axis), torch.zeros(n)), dim=-1))
    q_spin = half(spin, torch.tensor([0.0, 0.0, 1.0]).expand(n, 3))
    means = torch.stack(((cx - W / 2) / f * z, (cy - H / 2) / f * z, z), dim=-1)
    scales = torch.cat((sig * z[:, None] / f, torch.ones(n, 1)), dim=-1)
    return dict(means=means, quats=qmul(q_tilt, q_spin), scales=scales, opacities=opac, sh=rnd(n, 3), viewmat=torch.eye(4), K=K, W=W, H=H,
                sh_degree=None, background=torch.tensor([0.3, 0.6, 0.1]), near=0.01)


# (scene, channels C, distloss, tile size, with background) of tests/test_gpu_surfel_budget.py and of the constant's measurement in
# tests/test_surfel_cpu.py: every launchable compositor instantiation (C, DIST) in (3, F), (1, F), (1, T), (4, F), (4, T) meets both
# tile sizes; every stack scene meets both tile sizes and both values of DIST; the colour modes run with and without a background
PAIR_CASES = [
    ("clamp", 3, False, 16, True), ("clamp", 4, True, 8, False), ("clamp", 1, True, 16, False), ("clamp", 1, False, 8, False),
    ("outside", 3, False, 8, False), ("outside", 4, False, 16, True), ("outside", 4, True, 16, True), ("outside", 1, False, 16, False),
    ("outside", 1, True, 8, False), ("outside", 4, False, 8, False),
    ("stack256", 4, True, 16, True), ("stack256", 3, False, 8, True), ("stack256", 1, False, 16, False), ("stack256", 1, True, 8, False),
    ("stack257", 4, True, 8, False), ("stack257", 1, False, 16, False), ("stack257", 3, False, 16, False), ("stack257", 4, False, 8, True),
    ("stack600", 4, True, 16, False), ("stack600", 4, True, 8, True), ("stack600", 3, False, 16, False), ("stack600", 1, True, 8, False),
    ("stack600", 4, False, 8, False), ("stack600", 1, False, 16, False),
    ("stack_stop", 4, True, 16, True), ("stack_stop", 4, False, 8, False), ("stack_stop", 3, False, 16, True), ("stack_stop", 1, True, 8, False),
    ("stack_stop", 1, False, 16, False), ("stack_stop", 3, False, 8, False), ("stack_stop", 4, True, 8, False),
]
PAIR_COTANGENTS = ("dense", "one", "sparse")
PAIR_SCENE_ARGS = dict(outside=dict(n=400, min_facing=0.15))


def pair_one_image(case):
    """which single image the 'one' cotangent of a case of PAIR_CASES drives: alpha, normals and distort in turn over the cases with
    distloss, alpha and normals in turn over the others"""
    peers = [c for c in PAIR_CASES if c[2] == case[2]]
    return (("alpha", "normals", "distort") if case[2] else ("alpha", "normals"))[peers.index(case) % (3 if case[2] else 2)]


def pair_cotangents(kind, H, W, C, distloss, seed, one="normals"):
    """fp32 cotangents (v_render [H,W,C], v_alpha [H,W], v_normals [H,W,3], v_distort [H,W] or None) of the compositor budget tests, in
    the spirit of tests.util.budget_cotangents: 'dense' random signed; 'one' a single image (`one`: alpha, normals or distort), the
    others zero; 'sparse' non-zero on 32 scattered pixels only, so that a pair credited to the wrong pixel or record cannot average
    out"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    cot = [r(H, W, C), r(H, W), r(H, W, 3), r(H, W)]
    if kind == "one":
        assert one in ("alpha", "normals") or (one == "distort" and distloss), one
        which = ("render", "alpha", "normals", "distort").index(one)
        cot = [c if i == which else torch.zeros_like(c) for i, c in enumerate(cot)]
    elif kind == "sparse":
        on = torch.zeros(H * W, dtype=torch.bool)
        on[torch.randperm(H * W, generator=g)[:32]] = True
        on = on.reshape(H, W)
        cot = [c * (on if c.dim() == 2 else on[..., None]) for c in cot]
    else:
        assert kind == "dense", kind
    return cot[0], cot[1], cot[2], (cot[3] if distloss else None)


def pair_scene_inputs(name, C, tile_size):
    """CPU stand-in for what the GPU test takes from the device: the compositor's per-Gaussian inputs of a scene (the restatement's
    projection, rounded to fp32 as the kernels hold them) and the lists built from its tile rectangles.  dict(M, means2d, opacities,
    colors [V,C], normals, depths, flatten_ids, offsets, W, H, background), everything fp32 / long."""
    sc = make_scene(name, **PAIR_SCENE_ARGS.get(name, {}))
    W, H = sc["W"], sc["H"]
    with torch.no_grad():
        pr = project(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["viewmat"].double(), sc["K"].double(), W, H,
                     near=sc["near"], tile_size=tile_size)
        ids = torch.nonzero(pr["valid"]).reshape(-1)
        depths = pr["depths"][ids]
        cols = []
        if C >= 3:
            campos = -(sc["viewmat"][:3, :3].T @ sc["viewmat"][:3, 3]).double()
            cols.append(sh_colors(sc["sh_degree"], sc["means"].double()[ids], campos, sc["sh"].double()[ids]) if sc["sh_degree"] is not None
                        else sc["sh"].double()[ids])
        if C != 3:
            cols.append(depths[:, None])
        tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
        flatten_ids, offsets = build_lists(pr["rect"][ids], depths, tw, th)
    f = lambda a: a.float()
    return dict(M=f(pr["M"][ids]), means2d=f(pr["means2d"][ids]), opacities=sc["opacities"][ids], colors=f(torch.cat(cols, dim=-1)),
                normals=f(pr["normals"][ids]), depths=f(depths), flatten_ids=flatten_ids, offsets=offsets, W=W, H=H,
                background=sc["background"])


def pair_reference(inp, C, distloss, tile_size, with_bg, dtype=torch.float64, keep=None, kinds=PAIR_COTANGENTS, seed=0, one="normals"):
    """composite_pairs on the inputs `inp` (of pair_scene_inputs, or the GPU's own tensors under the same keys) under the cotangents of
    `kinds` (seed: of the random cotangents, one: the image of the 'one' kind; a case of PAIR_CASES passes its index and
    pair_one_image); returns (out, cots): out['grads'][i] belongs to cots[i]"""
    W, H = inp["W"], inp["H"]
    cots = [pair_cotangents(kind, H, W, C, distloss, 3 * seed + i, one) for i, kind in enumerate(kinds)]
    c = lambda a: a.detach().cpu().to(dtype)
    bg = c(inp["background"]) if (with_bg and C >= 3) else None
    out = composite_pairs(c(inp["M"]), c(inp["means2d"]), c(inp["opacities"]), c(inp["colors"]), c(inp["normals"]), C != 3, distloss, bg,
                          inp["flatten_ids"].cpu(), inp["offsets"].cpu(), W, H, tile_size, cotangents=cots, keep=keep)
    return out, cots


def scene_cotangents(H, W, D, seed=11):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    return dict(render=r(H, W, D), alpha=r(H, W), normals=r(H, W, 3), distort=r(H, W))


MODE_CHANNELS = {"RGB": 3, "D": 1, "ED": 1, "RGB+D": 4, "RGB+ED": 4}


def scene_reference(name, render_mode="RGB+ED", distloss=True, tile_size=16, with_background=True, **kw):
    """The restatement of a scene with the gradients of the cotangent-weighted loss; everything float64.  Returns (scene, out,
    cotangents, keep, leaf gradients, densification signal)."""
    sc = make_scene(name, **kw)
    leaves = {k: sc[k].double().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "sh")}
    out = rasterization_2dgs(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves["sh"], sc["viewmat"].double(),
                             sc["K"].double(), sc["W"], sc["H"], sh_degree=sc["sh_degree"],
                             background=sc["background"].double() if with_background else None, render_mode=render_mode,
                             distloss=distloss, near=sc["near"], tile_size=tile_size)
    cot = scene_cotangents(sc["H"], sc["W"], MODE_CHANNELS[render_mode])
    keep = (~out["pix_bad"]).double()
    images = ("render", "alpha", "normals") + (("distort",) if distloss else ())
    loss = sum((out[k] * cot[k] * (keep if out[k].dim() == 2 else keep[..., None])).sum() for k in images)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    vM = out["ray_transforms"].grad
    densify = out["depths"].detach()[:, None] * torch.stack((vM[:, 0, 2], vM[:, 1, 2]), dim=-1)
    out = {k: v.detach() if torch.is_tensor(v) else v for k, v in out.items()}          # (a cached reference does not hold its graph)
    return sc, out, cot, keep, grads, densify


# (scene, render_mode, distloss, tile size, with background) of the call-level cases tests/test_gpu_surfels.py adds to its first three:
# every render mode with distloss off and on where it is allowed; 'outside' in every mode at tile size 8 and in every second one at 16,
# 'clamp' at 16 (the square of its surfel at the image centre ends on x, y = 8 and 24 exactly: with tiles of 8 its tile count is
# undecided and the restatement leaves the whole image out); backgrounds=None in every second case
_CALL_MODES = (("RGB", False), ("D", False), ("D", True), ("ED", False), ("ED", True), ("RGB+D", False), ("RGB+D", True), ("RGB+ED", False),
               ("RGB+ED", True))
CALL_CASES = [("outside", mode, dist, 8, i % 2 == 1) for i, (mode, dist) in enumerate(_CALL_MODES)] + \
    [("outside", mode, dist, 16, i % 4 == 2) for i, (mode, dist) in enumerate(_CALL_MODES) if i % 2 == 0] + \
    [("clamp", mode, dist, 16, i % 2 == 0) for i, (mode, dist) in enumerate(_CALL_MODES)]
CALL_SCENE_ARGS = dict(outside=dict(n=400))
