"""The engine's fused per-view front and tail (csrc/gs_front.hip, gs_isect_bin_front in csrc/gs_sort.hip), as Python stages.

Reference cut: ``RenderableAttrs.splat`` shades every Gaussian (rfstudio/model/geosplat.py:80-122) and hands the colours to
``gsplat.rasterization`` (rfstudio/model/gsplat.py:334-355); autograd then runs the projection backward and the shading backward
one after the other.  ``geosplatting_amd.shade`` + ``geosplatting_amd.rasterization`` keep that call shape.  The step engine does
not need it: ``front_stage`` is ONE launch (projection with the shading fused ahead of it, north star), ``bin_stage`` the binning
from what it leaves behind, ``tail_stage`` ONE launch for the projection + shading backward.  Per visible Gaussian the path holds
one 64-byte record, a 4-byte depth key and an 8-byte tile rectangle -- nothing else.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L

_pinned_pool4 = []           # pinned int64[4] buffers for the asynchronous {V, I, ~min depth bits, max depth bits} read-back


def pinned_counts4() -> Tensor:
    return _pinned_pool4.pop() if _pinned_pool4 else torch.empty(4, dtype=torch.int64).pin_memory()


def release_counts4(t: Tensor) -> None:
    _pinned_pool4.append(t)


def reserve_pinned(n: int) -> None:
    """Pinned buffers cannot be allocated while a stream is capturing: make sure `n` are waiting."""
    while len(_pinned_pool4) < n:
        _pinned_pool4.append(torch.empty(4, dtype=torch.int64).pin_memory())


class Front:
    """What gs_front_fwd left behind for one view; (V, I, depth range) on their way to pinned memory."""
    __slots__ = ("vis", "keys", "rects", "tile_counts", "packed_index", "counts", "host_counts", "event", "whs", "key_bits", "N")


def front_stage(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, normals: Tensor, kd: Tensor, ks: Tensor,
                viewmat: Tensor, K: Tensor, cam_pos: Tensor, env_struct, W: int, H: int, min_roughness: float, max_metallic: float,
                mode: int, key_base: int = 0, key_bits: int = 32, status: Optional[Tensor] = None, tile_size: int = 16,
                eps2d: float = 0.3, near: float = 0.01, far: float = 1e10, radius_clip: float = 0.0, want_packed_index: bool = False,
                records: bool = True, binning: bool = True, tight_tiles: bool = False) -> Front:
    """S1-S3 + A1 (+ A1', A2 count) of one view on the current stream.  `scales` / `opacities` are the activated values
    (rfstudio/model/gsplat.py:336-339).  key_bits 24 needs `status` (int64[4]; word 3 reports a depth outside the key range).
    records=False: geometry only (keys, rectangles, tile counts; env_struct may be None); binning=False: records only.
    tight_tiles: tile rectangles clipped to the {alpha >= 1/255} extents (fewer intersections, identical pixels; not gsplat's `meta`)."""
    lib = L.lib()
    dev = means.device
    N = means.shape[0]
    fr = Front()
    fr.vis = torch.empty(max(N, 1), 16, dtype=torch.float32, device=dev) if records else None
    fr.keys = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if binning else None
    fr.rects = torch.empty(max(N, 1), 2, dtype=torch.int32, device=dev) if binning else None
    fr.counts = torch.empty(4, dtype=torch.int64, device=dev)
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    # (above 8 192 tiles the front kernel keeps no per-tile histogram and the binning derives the offsets from the sorted tile ids)
    fr.tile_counts = torch.empty(tw * th, dtype=torch.int32, device=dev) if (binning and tw * th <= 8192) else None
    fr.packed_index = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if want_packed_index else None
    ws_bytes = lib.gs_front_ws_bytes(N)
    ws = L.workspace(ws_bytes, dev)
    L.check(lib.gs_front_fwd(N, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(normals), L.ptr(kd), L.ptr(ks), L.ptr(viewmat),
                             L.ptr(K), L.ptr(cam_pos), min_roughness, max_metallic, mode, C.byref(env_struct) if env_struct is not None else None, W,
                             H, tile_size, eps2d, near, far, radius_clip, int(key_base) & 0xffffffff, int(key_bits), L.ptr(fr.vis), L.ptr(fr.keys),
                             L.ptr(fr.rects), L.ptr(fr.tile_counts), L.ptr(fr.packed_index), 1 if tight_tiles else 0, L.ptr(fr.counts), L.ptr(status),
                             L.ptr(ws), ws_bytes, L.stream()), "gs_front_fwd")
    fr.host_counts = pinned_counts4()
    fr.host_counts.copy_(fr.counts, non_blocking=True)        # 32 bytes, asynchronous
    fr.event = torch.cuda.Event()
    fr.event.record()
    fr.whs = (W, H, tile_size)
    fr.key_bits = int(key_bits)
    fr.N = N
    return fr


def depth_range(host_counts: Tensor):
    """(min, max) depth bits of a finished view from its pinned counts, or None when nothing was visible."""
    if int(host_counts[0]) <= 0:
        return None
    return 0xffffffff - int(host_counts[2]), int(host_counts[3])


def learn_depth_range(lo: Optional[int], hi: Optional[int], host_counts: Tensor):
    """The depth-bit range (lo, hi) seen so far (None, None: nothing yet), widened by a finished view's pinned counts."""
    rng = depth_range(host_counts)
    if rng is None:
        return lo, hi
    return (rng[0] if lo is None else min(lo, rng[0])), (rng[1] if hi is None else max(hi, rng[1]))


def binning_keys(lo: Optional[int], hi: Optional[int]):
    """(key_bits, key_base) of the binning keys for the depth-bit range (lo, hi) seen so far: 24-bit keys (three depth passes instead
    of four) -- key = depth bits - key_base with half an octave of room below the smallest depth seen -- while the range fits, else
    32-bit keys.  A view outside the range is reported through the status word (word 3)."""
    if lo is None:
        return 32, 0
    base = max(0, lo - (1 << 22))
    if hi - base < (1 << 24) - (1 << 21):
        return 24, base
    return 32, 0


def bin_stage(fr: Front, i_cap: Optional[int], status: Optional[Tensor], prepare: bool = True, binned=None):
    """A2-A4 + the compositor's record stream for a front; exact mode (i_cap None) waits for that view's (V, I) -- the one host
    synchronisation of the forward, as upstream; capacity mode sizes everything by (N, i_cap) and reads the counts on the device.
    Returns (state, V, I) with V / I the sizes the later launches are given (capacities in capacity mode).
    prepare=False: binning only (a geometry-only front); binned=(flatten_ids, isect_offsets) of such an earlier call: record stream only."""
    lib = L.lib()
    W, H, tile_size = fr.whs
    dev = fr.counts.device
    tw, th = (W + tile_size - 1) // tile_size, (H + tile_size - 1) // tile_size
    st = L.stream()
    if i_cap is None:
        fr.event.synchronize()
        V, I = int(fr.host_counts[0]), int(fr.host_counts[1])
        if V < 0 or I < 0 or I >= 2 ** 31:
            raise L.GeoSplatHipError(f"bad intersection count V={V} I={I}")
        counts = None
    else:
        V, I, counts = fr.N, int(i_cap), fr.counts
    if binned is not None:
        flat, offsets = binned
    else:
        flat = torch.empty(max(I, 1), dtype=torch.int32, device=dev)
        offsets = torch.empty(th * tw, dtype=torch.int32, device=dev)
        bin_bytes = lib.gs_isect_bin_front_ws_bytes(V, I, tw, th)
        bin_ws = L.workspace(max(bin_bytes, 1), dev)
        L.check(lib.gs_isect_bin_front(V, L.ptr(fr.keys), L.ptr(fr.rects), L.ptr(fr.tile_counts), L.ptr(counts), I, fr.key_bits, tw, th,
                                       L.ptr(flat), L.ptr(offsets), L.ptr(bin_ws), bin_bytes, L.ptr(status) if counts is not None else None,
                                       st), "gs_isect_bin_front")
    if not prepare:
        return dict(flatten_ids=flat, isect_offsets=offsets, counts=counts, keys=fr.keys, rects=fr.rects, tile_counts=fr.tile_counts), V, I
    rws_bytes = lib.gs_raster_ws_bytes(I, V, W, H, tile_size)
    rws = L.workspace(rws_bytes, dev)
    if counts is None:
        L.check(lib.gs_raster_prepare_vis(W, H, tile_size, 3, V, L.ptr(fr.vis), I, L.ptr(offsets), L.ptr(flat), L.ptr(rws),
                                          rws_bytes, st), "gs_raster_prepare_vis")
    else:
        L.check(lib.gs_raster_prepare_vis_cap(W, H, tile_size, 3, V, L.ptr(fr.vis), I, L.ptr(counts), L.ptr(offsets), L.ptr(flat),
                                              L.ptr(rws), rws_bytes, st), "gs_raster_prepare_vis_cap")
    state = dict(vis_records=fr.vis, flatten_ids=flat, isect_offsets=offsets, raster_ws=rws, counts=counts, keys=fr.keys, rects=fr.rects,
                 tile_counts=fr.tile_counts, packed_index=fr.packed_index)
    return state, V, I


def tail_stage(V: int, counts: Optional[Tensor], means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, normals: Tensor,
               kd: Tensor, ks: Tensor, viewmat: Tensor, K: Tensor, cam_pos: Tensor, env_struct, env_grad_struct, W: int, H: int,
               min_roughness: float, max_metallic: float, mode: int, vis: Tensor, v_packed: Tensor, g_means: Tensor, g_quats: Tensor,
               g_scales: Tensor, g_opacities: Tensor, g_normals: Tensor, g_kd: Tensor, g_ks: Tensor, eps2d: float = 0.3,
               priv: Optional[Tensor] = None) -> None:
    """A7 + S1-S3 backward of one view on the current stream: ADDS into the gradient buffers and the texel gradients.
    `priv`: the zeroed scratch of `tail_priv_alloc` (XCD-private copies of the mid-sized levels; fold with `tail_priv_reduce`)."""
    lib = L.lib()
    L.check(lib.gs_tail_bwd(V, L.ptr(counts), L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(normals), L.ptr(kd),
                            L.ptr(ks), L.ptr(viewmat), L.ptr(K), L.ptr(cam_pos), min_roughness, max_metallic, mode,
                            C.byref(env_struct), W, H, eps2d, L.ptr(vis), L.ptr(v_packed), int(v_packed.shape[1]), L.ptr(g_means),
                            L.ptr(g_quats), L.ptr(g_scales), L.ptr(g_opacities), L.ptr(g_normals), L.ptr(g_kd), L.ptr(g_ks),
                            C.byref(env_grad_struct), L.ptr(priv), 0 if priv is None else priv.numel(), L.stream()), "gs_tail_bwd")


def tail_priv_alloc(env_struct, mode: int, device) -> Optional[Tensor]:
    """Zeroed scratch for the XCD-private texel-gradient copies of one step (None when the pyramid has no mid-sized level)."""
    n = L.lib().gs_tail_priv_ws_bytes(C.byref(env_struct), mode)
    return torch.zeros(n, dtype=torch.uint8, device=device) if n > 0 else None


def tail_priv_reduce(env_struct, env_grad_struct, mode: int, priv: Optional[Tensor]) -> None:
    if priv is not None:
        L.check(L.lib().gs_tail_priv_reduce(C.byref(env_struct), mode, L.ptr(priv), priv.numel(), C.byref(env_grad_struct),
                                            L.stream()), "gs_tail_priv_reduce")


def tail_multi_stage(views, means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, normals: Tensor, kd: Tensor, ks: Tensor,
                     env_struct, env_grad_struct, min_roughness: float, max_metallic: float, mode: int, g_means: Tensor, g_quats: Tensor,
                     g_scales: Tensor, g_opacities: Tensor, g_normals: Tensor, g_kd: Tensor, g_ks: Tensor, accumulate: bool,
                     eps2d: float = 0.3, priv: Optional[Tensor] = None, parts: int = 3) -> None:
    """A7 + S1-S3 backward of SEVERAL views in one call (gs_tail_bwd_multi_parts): `views` = list of
    (viewmat, K, cam_pos, vis_records, v_packed, packed_index, W, H).  accumulate False: the gradient buffers are overwritten.
    parts: 1 = the shading half only, 2 = the projection half only (after the shading half of the same call), 3 = both;
    + 4 = a background launch (the shading half on half of the CUs, beside the compositor of the following views)."""
    lib = L.lib()
    arr = (L.GsTailView * len(views))()
    stride = None
    for i, (vm, K, cp, vis, vp, pidx, W, H) in enumerate(views):
        arr[i].viewmat = vm.data_ptr(); arr[i].K = K.data_ptr(); arr[i].cam_pos = cp.data_ptr()
        arr[i].vis_records = vis.data_ptr(); arr[i].v_packed = vp.data_ptr(); arr[i].packed_index = pidx.data_ptr()
        arr[i].W = int(W); arr[i].H = int(H)
        assert stride in (None, int(vp.shape[1]))
        stride = int(vp.shape[1])
    L.check(lib.gs_tail_bwd_multi_parts(int(parts), means.shape[0], len(views), arr, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities),
                                        L.ptr(normals), L.ptr(kd), L.ptr(ks), min_roughness, max_metallic, mode, C.byref(env_struct), eps2d, stride,
                                        L.ptr(g_means), L.ptr(g_quats), L.ptr(g_scales), L.ptr(g_opacities), L.ptr(g_normals), L.ptr(g_kd),
                                        L.ptr(g_ks), 1 if accumulate else 0, C.byref(env_grad_struct), L.ptr(priv),
                                        0 if priv is None else priv.numel(), L.stream()), "gs_tail_bwd_multi_parts")


# ------------------------------------------------------------------------------------------------------------ both drivers
# engine.RenderStep and the call shape (viewbatch) run the same chain per view: front_stage -> bin_stage -> composite_fwd ->
# composite_bwd -> tail_batch, and share what follows.
def front_streams(dev: torch.device):
    """The two front streams of a device (L.shared_stream): the fronts of consecutive views alternate between them."""
    return [L.shared_stream(dev, "front0"), L.shared_stream(dev, "front1")]


class CameraCache:
    """Device (view matrix, K, position) of cameras, cached by the pose's STORAGE ADDRESS, shape, stride and the intrinsics, checked
    against its version counter and, for a host-resident pose, its 48 bytes (a write that bypasses the version counter cannot return
    stale matrices; a device-resident pose relies on the version counter alone, clear() drops everything).  The entry keeps the pose
    alive, so its address cannot be recycled; `cameras[i]` of a resident dataset -- a new tensor object every step over the same
    storage -- hits.  A hit costs no copy and no synchronisation, also inside a graph capture.  Bounded, oldest entry evicted."""
    MAX_ENTRIES = 4096

    def __init__(self, dev: torch.device):
        self.dev = dev
        self.entries = {}                                   # key -> (pose, version, tensors, fingerprint)

    def get(self, cam, stream: torch.cuda.Stream):
        """A miss builds the tensors on `stream`, the front stream that reads them first -- behind the caller's stream if the pose is
        device-resident (it may still be in flight there) -- and every other front stream waits for them."""
        c2w = cam.c2w
        intr = (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), int(cam.width), int(cam.height))
        host = c2w.device.type == "cpu"
        fp = c2w.detach().numpy().tobytes() if host else None
        key = (c2w.data_ptr(), tuple(c2w.shape), tuple(c2w.stride()), intr)
        hit = self.entries.get(key)
        if hit is not None and hit[1] == c2w._version and hit[3] == fp:
            return hit[2]
        if len(self.entries) >= self.MAX_ENTRIES:
            self.entries.pop(next(iter(self.entries)))
        caller = torch.cuda.current_stream(self.dev)
        if not host and stream != caller:
            stream.wait_stream(caller)
        with torch.cuda.stream(stream):
            tensors = (cam.view_matrix.to(self.dev, torch.float32).contiguous(),
                       cam.intrinsic_matrix.to(self.dev, torch.float32).contiguous(),
                       c2w.detach()[:, 3].to(self.dev, torch.float32).contiguous())
            ev = torch.cuda.Event(); ev.record(stream)
        for f in front_streams(self.dev):
            if f != stream:
                f.wait_event(ev)
        self.entries[key] = (c2w, c2w._version, tensors, fp)
        return tensors

    def clear(self) -> None:
        self.entries.clear()


def texel_grads(env, flat: Optional[Tensor] = None):
    """(g_flat, g_base, g_levels, GsEnvGrad): texel-gradient accumulators of the pyramid `env` in ONE flat buffer -- `flat` (zeroed)
    when its size fits, else zeros on the current stream."""
    sizes = [env.base.numel()] + [l.numel() for l in env.levels]
    if flat is None or flat.numel() != sum(sizes):
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=env.base.device)
    parts = torch.split(flat, sizes)
    g_base = parts[0].view_as(env.base)
    g_levels = [q.view_as(l) for q, l in zip(parts[1:], env.levels)]
    eg = L.GsEnvGrad(); eg.base = g_base.data_ptr()
    for i, g in enumerate(g_levels):
        eg.levels[i] = g.data_ptr()
    return flat, g_base, g_levels, eg


def log_ws(I: int, W: int, H: int, dev: torch.device) -> Tensor:
    """The compositor's cull log of one view (what composite_fwd leaves for composite_bwd), on the current stream."""
    return L.workspace(L.lib().gs_raster_log_ws_bytes(I, W, H, 16), dev)


def composite_fwd(state, V: int, I: int, W: int, H: int, tone: int, exposure: Tensor, log: Tensor):
    """Compositor + tone map (S4 in its epilogue) of a view binned by bin_stage on the current stream -> (img, render, alphas,
    last_ids); it leaves its cull log (stream index + pixel mask of every record that entered a dense batch) in `log` for
    composite_bwd, which then neither culls nor builds masks."""
    dev = state["isect_offsets"].device
    f32 = torch.float32
    render = torch.empty(H, W, 3, dtype=f32, device=dev); alphas = torch.empty(H, W, dtype=f32, device=dev)
    last_ids = torch.empty(H, W, dtype=torch.int32, device=dev); img = torch.empty(H, W, 4, dtype=f32, device=dev)
    rws = state["raster_ws"]
    L.check(L.lib().gs_raster_composite_tone_log(W, H, 16, V, None, I, L.ptr(state["counts"]), L.ptr(state["isect_offsets"]),
                                                 L.ptr(render), L.ptr(alphas), L.ptr(last_ids), tone, L.ptr(exposure), L.ptr(img),
                                                 L.ptr(rws), rws.numel(), L.ptr(log), log.numel(), L.stream()),
            "gs_raster_composite_tone_log")
    return img, render, alphas, last_ids


def composite_bwd(state, V: int, I: int, W: int, H: int, tone: int, exposure: Tensor, render: Tensor, alphas: Tensor,
                  last_ids: Tensor, log: Tensor, v_img: Tensor, g_exp: Tensor) -> None:
    """A6 + S4 backward on the current stream: ADDS into the view's gradient records (state["v_packed"]) and into `g_exp`."""
    rws = state["raster_ws"]
    L.check(L.lib().gs_raster_bwd_tone_log_acc(W, H, 16, V, None, I, L.ptr(state["counts"]), L.ptr(state["isect_offsets"]),
                                               L.ptr(render), L.ptr(alphas), L.ptr(last_ids), tone, L.ptr(exposure), L.ptr(v_img),
                                               L.ptr(state["v_packed"]), L.ptr(g_exp), L.ptr(rws), rws.numel(), L.ptr(log),
                                               log.numel(), L.stream()), "gs_raster_bwd_tone_log_acc")


def smooth_view(state, V: int, I: int, W: int, H: int, kd: Tensor, ks: Tensor, normals: Tensor, bg9: Tensor, gt: Optional[Tensor],
                kinds, weights, loss: Tensor, zero_alphas: Tensor, g_kd: Tensor, g_ks: Tensor, g_normals: Tensor) -> Tensor:
    """The smoothing regularisers of one view on its own binning, on the current stream, AFTER the view's shaded compositor backward
    (rfstudio/model/geosplat.py:881-922: un-shaded renders of kd, (0, ks) and normals * 0.5 + 0.5 over the background): the colours
    in packed-slot order (gs_smooth_gather), ONE D = 9 compositor pair on the view's prepared workspace (D > 3: the colours come from
    `cols`, not from the record stream, which holds the shaded ones), the loss (gs_smooth_loss: ADDS to `loss`), and the fold of the
    D = 9 gradient records (state["v_packed9"], zeroed by the caller) into the view's v_packed and into g_kd / g_ks / g_normals.
    `zero_alphas`: at least H * W zeros (the renders have no alpha cotangent).  Returns the attribute renders [H,W,9]."""
    lib = L.lib()
    dev = kd.device
    st = L.stream()
    counts, vis, offsets, rws = state["counts"], state["vis_records"], state["isect_offsets"], state["raster_ws"]
    cols = torch.empty(max(V, 1), 9, dtype=torch.float32, device=dev)
    L.check(lib.gs_smooth_gather(V, L.ptr(counts), L.ptr(vis), L.ptr(kd), L.ptr(ks), L.ptr(normals), L.ptr(cols), st), "gs_smooth_gather")
    render = torch.empty(H, W, 9, dtype=torch.float32, device=dev)
    alphas = torch.empty(H, W, dtype=torch.float32, device=dev)
    last_ids = torch.empty(H, W, dtype=torch.int32, device=dev)
    if counts is None:
        L.check(lib.gs_raster_composite(W, H, 16, 9, V, L.ptr(cols), L.ptr(bg9), I, L.ptr(offsets), L.ptr(render), L.ptr(alphas),
                                        L.ptr(last_ids), L.ptr(rws), rws.numel(), st), "gs_raster_composite")
    else:
        L.check(lib.gs_raster_composite_cap(W, H, 16, 9, V, L.ptr(cols), L.ptr(bg9), I, L.ptr(counts), L.ptr(offsets), L.ptr(render),
                                            L.ptr(alphas), L.ptr(last_ids), L.ptr(rws), rws.numel(), st), "gs_raster_composite_cap")
    from .loss import smooth_loss_and_grad
    _, v_img = smooth_loss_and_grad(render, gt, kinds, weights, out=loss)
    v9 = state["v_packed9"]
    if counts is None:
        L.check(lib.gs_raster_bwd_acc(W, H, 16, 9, V, L.ptr(cols), L.ptr(bg9), I, L.ptr(offsets), L.ptr(alphas), L.ptr(last_ids), L.ptr(v_img),
                                      L.ptr(zero_alphas), L.ptr(v9), L.ptr(rws), rws.numel(), st), "gs_raster_bwd_acc")
    else:
        L.check(lib.gs_raster_bwd_acc_cap(W, H, 16, 9, V, L.ptr(cols), L.ptr(bg9), I, L.ptr(counts), L.ptr(offsets), L.ptr(alphas),
                                          L.ptr(last_ids), L.ptr(v_img), L.ptr(zero_alphas), L.ptr(v9), L.ptr(rws), rws.numel(),
                                          st), "gs_raster_bwd_acc_cap")
    vp = state["v_packed"]
    L.check(lib.gs_smooth_fold(V, L.ptr(counts), L.ptr(vis), L.ptr(v9), int(v9.shape[1]), L.ptr(vp), int(vp.shape[1]), L.ptr(g_kd),
                               L.ptr(g_ks), L.ptr(g_normals), st), "gs_smooth_fold")
    return render


def tail_schedule(default):
    """Views per tail launch of a backward pass, the last entry repeating: GEOSPLAT_TAIL_BATCH ("3,4,1"), or `default` ("auto")."""
    tb = os.environ.get("GEOSPLAT_TAIL_BATCH", "auto")
    return default if tb == "auto" else [max(1, int(x)) for x in tb.split(",")]


def tail_batch(views, args, accumulate: bool, final: bool, tail: torch.cuda.Stream, proj: torch.cuda.Stream, tail_events=None):
    """tail_multi_stage(views, *args) behind the caller's stream.  A BACKGROUND launch on `tail` (parts 7: half of the CUs, beside
    the compositor of the following views), or the `final` batch of a backward pass: the shading half (parts 1) on `tail`, its
    projection half (parts 2) behind it on `proj` -- a front stream, idle by then -- beside whatever the caller runs next, e.g. the
    prefilter backward, which needs only the texel gradients; `tail_events` then gets (start, end of the shading half, end of the
    projection half).  The per-view tensors are recorded on every stream used; returns those streams."""
    timed = final and tail_events is not None
    ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(tail.device))
    tail.wait_event(ev)
    with torch.cuda.stream(tail):
        if timed:
            t0 = torch.cuda.Event(enable_timing=True); t0.record(tail)
        tail_multi_stage(views, *args, accumulate=accumulate, parts=1 if final else 7)
    used = [tail]
    if final:
        ev_sh = torch.cuda.Event(enable_timing=timed); ev_sh.record(tail)
        proj.wait_event(ev_sh)                              # (v_means: the projection half adds to what the shading half stored)
        with torch.cuda.stream(proj):
            tail_multi_stage(views, *args, accumulate=accumulate, parts=2)
            if timed:
                t2 = torch.cuda.Event(enable_timing=True); t2.record(proj)
                tail_events.append((t0, ev_sh, t2))
        used.append(proj)
    for v in views:
        for t in v[:6]:
            for s in used:
                t.record_stream(s)
    return used


def status_overflow(word: Tensor):
    """Decode a host copy of the device status word {GS_ENOSPC or 0, largest required I, largest required V, depth outside the 24-bit
    key range}: (truncated -- a view was composited from a truncated list, or with clamped keys --, needs_32bit_keys, required_I)."""
    w = word.tolist()
    return w[0] != 0 or w[3] != 0, w[3] != 0, w[1]
