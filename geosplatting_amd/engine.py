"""The render-and-backward step of the path for a batch of views -- the counterpart of
``GeoSplatter.render_report`` (rfstudio/model/geosplat.py:856-927: prefilter once, then a loop of
``attrs.splat`` over the views) followed by the autograd backward the trainer triggers
(rfstudio/optim/optimizer.py:107), with the data-parallel gradient sum of geosplatting_amd.parallel.

Order of work per step (all on the current HIP stream, kernels in libgeosplat_hip.so):
    as_splitsum(cubemap)                                   S5 forward   (once per step)
    for each local view:  shade -> rasterize -> tone-map    S1-S4, A1-A5
                          backward of the same              A6, A7, S1-S3 backward
    prefilter backward with the texel gradients summed over the views   S5 backward (once per step)
    flat-bucket all-reduce over ranks                       RCCL
"""
from __future__ import annotations

import collections
import contextlib
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .cameras import Camera
from .parallel import GradBucket, collectives_active
from . import front as F
from .shading import _MODE, _TONE, RenderableAttrs, _make_env, get_fg_lut
from .splitsum import TextureSplitSum, as_splitsum, as_splitsum_backward, as_splitsum_forward, can_shard_prefilter
from .splats import SplatSet

PARAM_NAMES = ("means", "scales", "quats", "opacities", "normals", "kd", "ks", "cubemap", "exposure")


@dataclass
class PathParams:
    """Leaf tensors of the path (replicated on every rank)."""
    means: Tensor; scales: Tensor; quats: Tensor; opacities: Tensor       # raw Splats fields
    normals: Tensor; kd: Tensor; ks: Tensor                                 # RenderableAttrs
    cubemap: Tensor                                                         # [6,R,R,3]
    exposure: Tensor                                                        # scalar (already exp'ed)

    def named(self) -> Dict[str, Tensor]:
        return {k: getattr(self, k) for k in PARAM_NAMES}

    def shapes(self) -> Dict[str, Sequence[int]]:
        return {k: tuple(v.shape) if v.dim() > 0 else (1,) for k, v in self.named().items()}


def _auto_tail_schedule(n_views: int):
    """Views per tail launch of a step.  A background launch (half of the CUs) works a view off in about half the time the
    compositor needs for one, and the batch before the last has to be done when the last compositor backward ends: the LAST batch
    takes two views, the ones before it up to three (8 views: 3 + 3 + 2; 7: 3 + 2 + 2; 6: 2 + 2 + 2; 5: 3 + 2).  With four views or
    fewer (the strong split over 2 / 4 GPUs) the measured best ends on single views: 4: 2 + 1 + 1 (583 views/s against 571 for
    2 + 2, 552 for one launch), 3: 2 + 1 (519 / 499), 2: 1 + 1 (429 / 418)."""
    if n_views <= 4:
        return {0: [1], 1: [1], 2: [1, 1], 3: [2, 1], 4: [2, 1, 1]}[max(n_views, 0)]
    r, sched = n_views - 2, []
    while r > 0:
        k = 3 if (r >= 3 and r != 4) else min(r, 2)
        sched.append(k)
        r -= k
    return sched + [2]


@dataclass
class Smoothing:
    """The smoothing regularisers of a fused step (rfstudio/model/geosplat.py:881-922; stage1.train_step_fused builds it from the
    model).  Per attribute render -- kd, (0, ks), normals * 0.5 + 0.5, all composited over `background` [3] -- a term kind
    (loss.SMOOTH_NONE / SMOOTH_EDGE / SMOOTH_TV) and its weight, already divided by the global batch size; `gt`: per LOCAL view the
    ground truth blended over that background [H,W,3] (None when no term is edge-aware)."""
    kinds: Tuple[int, int, int]
    weights: Tuple[float, float, float]
    background: Tensor
    gt: Optional[Sequence[Tensor]] = None


@dataclass
class _Geometry:
    """What RenderStep._geometry hands to the records and views phases of a step."""
    scales_act: Tensor; opac_act: Tensor                  # the once-per-step exp / sigmoid activations
    i_cap: Optional[int]                                  # intersection capacity per view; None = exact mode
    key_bits: int; key_base: int                          # binning keys of the step's views
    status: Optional[Tensor]                              # the device status word the fronts report into
    tight: bool                                           # tile rectangles clipped to the {alpha >= 1/255} extents
    early: Dict[int, Tuple[Tensor, Tensor]]               # view index -> (flatten_ids, isect_offsets) binned under the prefilter


@dataclass
class _Views:
    """What RenderStep._views hands to _finish."""
    b: Dict[str, Tensor]                                  # the gradient bucket's segments
    images: Optional[List[Tensor]]
    g_base: Tensor; g_levels: List[Tensor]; g_flat: Tensor   # texel gradients summed over the views (g_flat: all of them)
    env: TextureSplitSum
    sharded: bool; world: int; all_reduce: bool
    main: Optional[torch.cuda.Stream]                     # the caller's stream (capture_views: set at every replay)
    pstream: Optional[torch.cuda.Stream]                  # the per-Gaussian gradients become final on this stream (None: on main)
    tail_job: Optional[dict]                              # the last tail launch, left to _chunked_tail
    smooth_grads: Optional[Tuple[Tensor, Tensor, Tensor]] = None   # kd / ks / normal gradients of the smoothing terms, not yet in `b`
    captured: bool = False                                # recorded into a graph: its tensors live in the graph's private pool


class RenderStep:
    def __init__(self, params: PathParams, min_roughness: float = 0.1, max_metallic: float = 1.0, mode: str = "pbr",
                 tone_type: str = "naive", prefilter: bool = True, fused: bool = True, fg_lut: Optional[Tensor] = None):
        self.p = params
        self.fg_lut = None if fg_lut is None else fg_lut.to(params.means.device, torch.float32).contiguous()   # default: the packaged table
        self.min_roughness, self.max_metallic, self.mode, self.tone_type = min_roughness, max_metallic, mode, tone_type
        self.prefilter = prefilter
        self.fused = fused
        self.bucket = GradBucket(params.shapes(), params.means.device)
        self._static_env: Optional[TextureSplitSum] = None
        self._cameras = F.CameraCache(params.means.device)
        self._side_stream = None
        self._tail_stream = None
        # capacity protocol state (see _geometry / poll_capacity)
        self._use_capacity = os.environ.get("GEOSPLAT_CAPACITY", "1") != "0"
        self._key_lo = self._key_hi = None     # depth-bit range seen so far (asynchronous read-back): sizes the 24-bit binning keys
        self._key32 = os.environ.get("GEOSPLAT_KEY_BITS", "24") == "32"   # forced by a key-range overflow, or by the environment
        self._cap_margin = float(os.environ.get("GEOSPLAT_CAPACITY_MARGIN", "1.25"))   # capacity = margin x the largest count seen
        self._i_cap = None                 # intersection capacity per view; None = exact mode (one (V, I) read-back per view)
        self._status = None                # device int64[4]: {GS_ENOSPC or 0, max required I, max required V, depth outside the 24-bit key range}
        self._status_host = None           # pinned snapshot used by the graph-capture paths (one buffer, refreshed by every replay)
        self._status_event = None
        self._status_pending = collections.deque()   # eager steps: (pinned snapshot of the word, event), one per step, each looked at ONCE
        self._status_pool = []             # pinned int64[4] buffers waiting for reuse
        self.kernel_events = None          # set to a list: (name, start event, end event) around the compositor launches (bench.py)
        self.tail_events = None            # set to a list: (start, end of the shading half, end of the projection half) of the LAST tail launch
        self._seen_counts = []
        self._exact_max_i = 0              # largest intersection count read back by an exact-mode step
        self._pre_group = None
        self.truncated_steps = 0           # steps whose overflow word was seen set (each was composited from a truncated list)
        self.chunked_tails = 0             # steps whose last tail ran in Gaussian-range chunks under their all-reduce (_chunked_tail)
        self._overflow_unreported = False  # an overflow seen by the poll inside __call__ that no caller has been told about yet
        n_fly = int(os.environ.get("GEOSPLAT_STEPS_IN_FLIGHT", "3"))
        self._max_in_flight = max(1, n_fly)
        self._in_flight = collections.deque() if n_fly > 0 else None     # end-of-step events of the steps the GPU has not finished (None: unbounded)
        self.last_smoothing_loss = None    # device scalar: the smoothing terms of the last step's local views (__call__(smoothing=...))
        self.last_attribute_renders = None # with keep_images: that step's attribute renders [H,W,9] per view (tests)

    def _prefilter_group(self):
        """A second communicator for the prefilter exchange (25 MB all-reduce + two rounds of small all-gathers), so that it
        never queues behind the 149 MB per-Gaussian all-reduce on the default one.  Created collectively on first use."""
        import torch.distributed as dist
        if self._pre_group is None:
            self._pre_group = dist.new_group()
        return self._pre_group

    def rebind(self, params: PathParams) -> None:
        """New parameter tensors for the next step (a stage-1 loop extracts a different number of Gaussians every
        iteration): the gradient bucket is re-laid out when a shape changed; streams and camera tensors are kept."""
        self.p = params
        if {k: tuple(v) for k, v in params.shapes().items()} != self.bucket.shapes:
            self.bucket = GradBucket(params.shapes(), params.means.device, comm_stream=self.bucket.comm_stream)

    # ------------------------------------------------------------------------------------------------- fused path
    @property
    def _cam_cache(self):
        """The camera cache's entries as {key: (pose, version, intrinsics, tensors, fingerprint)} (tests read them)."""
        return {k: (e[0], e[1], k[3], e[2], e[3]) for k, e in self._cameras.entries.items()}

    def invalidate_cameras(self) -> None:
        """Forget every cached (view matrix, K, position) triple: for callers that rewrite DEVICE-resident poses behind autograd's back."""
        self._cameras.clear()

    def _activations(self, out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
        """The once-per-step exp / sigmoid activations of the scales and opacities on the current stream (into `out` if given)."""
        p = self.p
        if out is None:
            return p.scales.detach().exp(), torch.sigmoid(p.opacities.detach()).squeeze(-1).contiguous()
        torch.exp(p.scales.detach(), out=out[0])
        torch.sigmoid(p.opacities.detach().squeeze(-1), out=out[1])
        return out

    def _geometry(self, cameras, bin_first: bool, act: Optional[Tuple[Tensor, Tensor]] = None) -> _Geometry:
        """First phase of a step: what does not need the pyramid -- activations, streams, key width -- and, with `bin_first` in
        capacity mode, the GEOMETRY of the first view (projection, keys, binning: gs_front_fwd without records) on a front stream, so
        that it runs UNDER the prefilter forward instead of behind it (the step used to start its first compositor 0.9 ms after the
        prefilter ended).  `act`: the activations, already computed (capture_views)."""
        p = self.p
        dev = p.means.device
        scales_act, opac_act = act if act is not None else self._activations()
        main = torch.cuda.current_stream(dev)
        if self._use_capacity and self._status is None:      # zero-filled on the main stream BEFORE the side streams fork from it
            self._status = torch.zeros(4, dtype=torch.int64, device=dev)
        if self._side_stream is None:
            self._side_stream = F.front_streams(dev)
        # tile rectangles clipped to the {alpha >= 1/255} extents (GEOSPLAT_TIGHT_TILES=0: gsplat's squares): 18 % fewer intersections
        # on the bench scene, identical pixels (gs_front_fwd; the engine never returns gsplat's `meta`)
        tight = os.environ.get("GEOSPLAT_TIGHT_TILES", "1") != "0"
        # binning keys: 24 bits once the depth range of earlier views is known (front.binning_keys); a view outside the range is
        # reported through the status word (poll_capacity) and the engine falls back to 32-bit keys
        i_cap = self._i_cap if self._use_capacity else None
        key_bits, key_base = F.binning_keys(self._key_lo, self._key_hi) if (i_cap is not None and not self._key32) else (32, 0)
        status = self._status if (key_bits == 24 or self._use_capacity) else None
        geo = _Geometry(scales_act, opac_act, i_cap, key_bits, key_base, status, tight, {})
        if bin_first and i_cap is not None and len(cameras) > 0:
            # (the geometry of ONE view: of two, beside the prefilter, costs more than it hides -- 563 against 580 views/s)
            side = self._side_stream[0]
            ev_a = torch.cuda.Event(); ev_a.record(main)
            side.wait_event(ev_a)
            cam_t = self._cameras.get(cameras[0], side)
            with torch.cuda.stream(side):
                fr = self._front(geo, cameras[0], cam_t, None, records=False)
                binned, _, _ = F.bin_stage(fr, i_cap, self._status, prepare=False)
            self._seen_counts.append((fr.host_counts, fr.event))
            geo.early[0] = (binned["flatten_ids"], binned["isect_offsets"])
            for t in (scales_act, opac_act):
                t.record_stream(side)
        return geo

    def _front(self, geo: _Geometry, cam: Camera, cam_t, e, records: bool = True, binning: bool = True) -> F.Front:
        """front_stage of one view on the current stream: records=False: geometry only; binning=False: records only."""
        p = self.p
        keys = (geo.key_base, geo.key_bits, geo.status) if binning else (0, 32, None)
        return F.front_stage(p.means.detach(), p.quats.detach(), geo.scales_act, geo.opac_act, p.normals.detach(), p.kd.detach(),
                             p.ks.detach(), *cam_t, e, cam.width, cam.height, self.min_roughness, self.max_metallic, _MODE[self.mode],
                             *keys, want_packed_index=records, records=records, binning=binning, tight_tiles=geo.tight)

    def _env_args(self, env: TextureSplitSum):
        """(detached pyramid, its GsEnv struct) for the kernels."""
        env_d = TextureSplitSum(env.base.detach(), [l.detach().contiguous() for l in env.levels], env.min_roughness, env.max_roughness)
        return env_d, _make_env(get_fg_lut(self.p.means.device) if self.fg_lut is None else self.fg_lut, env_d)

    def _records(self, cameras, geo: _Geometry, env: TextureSplitSum) -> Dict[int, F.Front]:
        """capture_views: the RECORDS (shading) of the views whose geometry came from the geometry graph, as a graph of their own --
        it needs the pyramid but not the binning, so it replays BESIDE the rest of the geometry graph (projection keys, five radix
        passes, emission: 0.25 ms per view) instead of behind it.  Returns the fronts by view index, for _views."""
        _, e = self._env_args(env)
        cur = torch.cuda.current_stream(self.p.means.device)
        return {j: self._front(geo, cameras[j], self._cameras.get(cameras[j], cur), e, binning=False) for j in sorted(geo.early)}

    def _pyramid(self, sharded: bool, world: int) -> TextureSplitSum:
        """The pyramid of this step: the prefilter forward (sharded over the ranks: splitsum.py), or without the prefilter in the step
        the one filtered once."""
        if not self.prefilter:
            if self._static_env is None:
                self._static_env = as_splitsum_forward(self.p.cubemap)
            return self._static_env
        if sharded:
            import torch.distributed as dist
            return as_splitsum_forward(self.p.cubemap, rank=dist.get_rank(), world=world, group=self._prefilter_group(), sharded=True)
        return as_splitsum_forward(self.p.cubemap)

    def _sharding(self, all_reduce: bool):
        """(world, sharded): S5 sharded over the ranks (each applies 1/world of every level's tiles, all-reduce of the disjoint
        pieces): splitsum.py (collectives_active(): more than one rank, or the one-rank RCCL run of GEOSPLAT_COLLECTIVES_AT_WORLD1=1)"""
        import torch.distributed as dist
        world = dist.get_world_size() if (all_reduce and dist.is_available() and dist.is_initialized()) else 1
        sharded = (self.prefilter and all_reduce and collectives_active() and os.environ.get("GEOSPLAT_SHARD_PREFILTER", "1") != "0"
                   and can_shard_prefilter(int(self.p.cubemap.shape[1]), world))
        return world, sharded

    def _views(self, cameras, upstream, all_reduce, keep_images, geo: _Geometry, env: Optional[TextureSplitSum] = None,
               recs: Optional[Dict[int, F.Front]] = None, smoothing: Optional[Smoothing] = None) -> _Views:
        """Second phase of a step: the zero fill, the pyramid (`env`: already filtered, capture_views) and every view up to its last
        tail launch.  Same arithmetic as the autograd path, driven directly through the C-ABI: every tail launch ADDS into the flat
        gradient bucket, the exp / sigmoid activations of GSplatter.render_rgba (rfstudio/model/gsplat.py:336-339) are applied once
        per step and chained once per step (their Jacobians do not depend on the view), and the prefilter backward runs once on the
        texel gradients summed over the views (_finish).  `recs`: the fronts of _records, by view index.

        HIP streams of a step: two FRONT streams run the memory / latency-bound front of every view (gs_front_fwd, the binning, the
        record stream: ~22 short kernels, none of which fills the chip), the fronts of consecutive views alternating between them
        (one: 638 views/s, two: 690, three: 655); the caller's stream runs the VALU-bound compositor forward / backward -- the step's
        critical path; a tail stream runs the gradient kernels of the views in batches.  In capacity mode nothing makes the host wait,
        so the fronts run as far ahead of the compositor as their inputs allow.

        `smoothing`: after each view's shaded compositor backward, its attribute renders and their regularisers on the main stream
        (F.smooth_view: the view's own binning, a D = 9 compositor pair, gs_smooth_loss, the fold of its gradient records into the
        view's v_packed -- ahead of the tail launch that reads it -- and into per-Gaussian kd / ks / normal scratch, which reaches the
        bucket behind the last tail launch, whose first launch overwrites those rows)."""
        lib = L.lib()
        p = self.p
        dev = p.means.device
        N = p.means.shape[0]
        f32 = torch.float32
        st = L.stream
        mode, tone = _MODE[self.mode], _TONE[self.tone_type]
        world, sharded = self._sharding(all_reduce)
        scales_act, opac_act = geo.scales_act, geo.opac_act
        means, quats = p.means.detach(), p.quats.detach()
        normals, kd, ks = p.normals.detach(), p.kd.detach(), p.ks.detach()
        main = torch.cuda.current_stream(dev)
        sides = self._side_stream
        i_cap, early = geo.i_cap, geo.early
        # ONE fill, issued before the prefilter: the bucket, the activation-gradient accumulators and the texel-gradient accumulators
        # share an allocation
        cres = int(p.cubemap.shape[1])
        tex_res = [cres]
        while tex_res[-1] > 16:
            tex_res.append(tex_res[-1] // 2)
        tex_sizes = [6 * tex_res[-1] * tex_res[-1] * 3] + [6 * r * r * 3 for r in tex_res]        # base map, then the levels
        # (smoothing: kd / ks / normal gradient scratch, the loss scalar and the zero alpha cotangent of the attribute renders)
        sm_sizes = [3 * N, 2 * N, 3 * N, 1, max([c.width * c.height for c in cameras] + [1])] if smoothing is not None else []
        sc = self.bucket.zero_with_scratch([3 * N, N, sum(tex_sizes)] + sm_sizes)
        b = self.bucket.unpack()
        smooth_grads = None
        self.last_smoothing_loss = self.last_attribute_renders = None
        if smoothing is not None:
            smooth_grads = (sc[3].view(N, 3), sc[4].view(N, 2), sc[5].view(N, 3))
            smooth_loss, zero_alphas = sc[6].view(()), sc[7]
            bg9 = smoothing.background.detach().to(dev, f32).reshape(3).repeat(3).contiguous()
            self.last_smoothing_loss = smooth_loss           # sum of the smoothing terms of this step's local views (device scalar)
            self.last_attribute_renders = [] if keep_images else None   # [H,W,9] per view: kd, (0, ks), normals * 0.5 + 0.5 (tests)
        g_scales_act = sc[0].view(N, 3); g_opac_act = sc[1]
        exposure = p.exposure.detach().reshape(1).contiguous()
        if env is None:
            env = self._pyramid(sharded, world)
        env_d, e = self._env_args(env)
        # texel-gradient accumulators: one flat buffer behind the base + level gradients (the sharded prefilter sums them over the
        # ranks in ONE all-reduce).  (Two sets with the first half's prefilter backward under the remaining compositor work were
        # measured: the backward is linear, splitting it doubles it, the overlap does not pay that back.)
        g_flat, g_base, g_levels, eg = F.texel_grads(env_d, sc[2])
        self.last_texel_grads = (g_base, g_levels)           # d loss / d pyramid of this step (summed over the local views): tests read it
        images = []
        tail = self._tail_stream
        if tail is None:
            tail = self._tail_stream = L.shared_stream(dev, "tail")
        for sd in sides:
            sd.wait_stream(main)                             # prefilter pyramid, activations, zeroed buckets
        tail.wait_stream(main)

        # the tails of the views in ONE call per batch of views (gs_tail_bwd_multi_parts: the views of a Gaussian on adjacent lanes, its
        # gradients stored once).  The launches that are not the last run as BACKGROUND launches (parts + 4: half of the CUs) beside the
        # compositor of the following views, and the last one, alone on the GPU, covers 2 views instead of 8 (_auto_tail_schedule).
        tail_sched = F.tail_schedule(_auto_tail_schedule(len(cameras)))
        pending_tails = []
        n_tail_launches = 0
        pstream = None
        # with collectives in the step the LAST tail launch is left to _finish, which runs it in Gaussian-range chunks and sums chunk k
        # over the ranks while chunk k + 1 is still being computed (_chunked_tail)
        n_chunks = max(1, int(os.environ.get("GEOSPLAT_TAIL_CHUNKS", "4")))
        defer_tail = all_reduce and collectives_active() and n_chunks > 1 and N >= 4096
        tail_job = None

        cam_ts = {}

        def start_view(cam, j):                              # S1-S3 + A1; (V, I) travel to the host asynchronously
            side = sides[j % len(sides)]
            cam_t = cam_ts[j] = self._cameras.get(cam, side)
            if recs is not None and j in recs:               # (capture_views: the records graph has run)
                return recs[j], j, side
            with torch.cuda.stream(side):                    # (binned under the prefilter: only the records (shading) are still missing)
                fr = self._front(geo, cam, cam_t, e, binning=j not in early)
            return fr, j, side

        # Capacity protocol (include/geosplat_hip.h): once the engine has seen the intersection counts of a step, the later
        # steps size every per-view buffer by (N, I_cap) and leave (V, I) on the device -- no read-back, no host wait inside
        # the step.  The counts still travel to pinned memory asynchronously; poll_capacity() looks at them (and at the
        # overflow status word) without blocking.
        def bin_view(item):                                  # A2-A4 + record stream on the front stream (exact mode: the host waits for that view's counts)
            fr, j, side = item
            with torch.cuda.stream(side):
                if i_cap is not None:
                    self._seen_counts.append((fr.host_counts, fr.event))
                state, V, I = F.bin_stage(fr, i_cap, self._status, binned=early.get(j))
                if i_cap is None:
                    self._exact_max_i = max(self._exact_max_i, I)
                    self._key_lo, self._key_hi = F.learn_depth_range(self._key_lo, self._key_hi, fr.host_counts)
                    F.release_counts4(fr.host_counts)
                # the packed gradient records of this view, zeroed HERE (front stream, under the compositor of the previous view)
                state["v_packed"] = torch.zeros(max(V, 1), lib.gs_raster_grad_stride(3), dtype=f32, device=dev)
                if smoothing is not None:                    # (the D = 9 pair of the smoothing renders: a second set of records)
                    state["v_packed9"] = torch.zeros(max(V, 1), lib.gs_raster_grad_stride(9), dtype=f32, device=dev)
                ev = torch.cuda.Event(); ev.record(side)
            for t in state.values():
                if isinstance(t, torch.Tensor):
                    t.record_stream(main)
            return state, V, I, ev

        n_views = len(cameras)
        proj = [start_view(cameras[j], j) for j in range(min(2, n_views))]   # prologue: A(0), A(1), B1(0)
        binned = bin_view(proj.pop(0)) if n_views else None
        for i, cam in enumerate(cameras):
            vm, K, cam_pos = cam_ts.pop(i)
            W, H = cam.width, cam.height
            s, V, I, ev = binned
            main.wait_event(ev)
            kev = self.kernel_events
            if kev is not None:
                k0 = torch.cuda.Event(enable_timing=True); k0.record(main)
            log_ws = F.log_ws(I, W, H, dev)
            img, render, alphas, last_ids = F.composite_fwd(s, V, I, W, H, tone, exposure, log_ws)
            if kev is not None:
                k1 = torch.cuda.Event(enable_timing=True); k1.record(main)
                kev.append(("raster_fwd_kernel", k0, k1))
            v_img = upstream(i, img).contiguous()
            if kev is not None:
                k2 = torch.cuda.Event(enable_timing=True); k2.record(main)
            F.composite_bwd(s, V, I, W, H, tone, exposure, render, alphas, last_ids, log_ws, v_img, b["exposure"])
            if kev is not None:
                k3 = torch.cuda.Event(enable_timing=True); k3.record(main)
                kev.append(("raster_bwd_kernel", k2, k3))
            if smoothing is not None:                        # (behind the shaded backward: its tile order lives in the same workspace)
                attr = F.smooth_view(s, V, I, W, H, kd, ks, normals, bg9, None if smoothing.gt is None else smoothing.gt[i],
                                     smoothing.kinds, smoothing.weights, smooth_loss, zero_alphas, *smooth_grads)
                if keep_images:
                    self.last_attribute_renders.append(attr)
            # keep the front streams two views ahead: A(i+2), then B1(i+1) -- AFTER this view's main-stream chain has been enqueued
            # (their ~35 launches cost the host 0.2-0.3 ms; issued first, the compositor stream idled that long per view)
            if i + 2 < n_views:
                proj.append(start_view(cameras[i + 2], i + 2))
            binned = bin_view(proj.pop(0)) if i + 1 < n_views else None
            # gradient tail (A7 + S1-S3 backward: HBM / atomic-rate bound) on the tail stream, beside the compositor of the next views
            pending_tails.append((vm, K, cam_pos, s["vis_records"], s["v_packed"], s["packed_index"], W, H))
            last = i == n_views - 1
            if len(pending_tails) == tail_sched[min(n_tail_launches, len(tail_sched) - 1)] or last:
                targs = (means, quats, scales_act, opac_act, normals, kd, ks, e, eg, self.min_roughness, self.max_metallic, mode,
                         b["means"], b["quats"], g_scales_act, g_opac_act, b["normals"], b["kd"], b["ks"])
                if last and defer_tail:
                    tail_job = dict(targs=(pending_tails,) + targs, accumulate=n_tail_launches > 0, n_chunks=n_chunks)
                else:
                    used = F.tail_batch(pending_tails, targs, n_tail_launches > 0, last, tail, sides[0], self.tail_events)
                    if last:
                        pstream = used[1]
                    n_tail_launches += 1
                    pending_tails = []
            if keep_images:
                images.append(img)
        main.wait_stream(tail)
        if smooth_grads is not None and tail_job is None:
            # the smoothing scratch joins the bucket behind the last tail launch (the first one STORES the kd / ks / normal rows) and
            # ahead of their all-reduce, which starts on pstream (_finish)
            for name, g in zip(("kd", "ks", "normals"), smooth_grads):
                b[name].add_(g)
            if pstream is not None:
                pstream.wait_stream(main)
            smooth_grads = None
        if i_cap is not None:                                # the overflow word follows the step to the host, asynchronously
            if torch.cuda.is_current_stream_capturing():      # a replayed graph refreshes ONE pinned buffer; replay.check() reads it
                if self._status_host is None:
                    self._status_host = torch.zeros(4, dtype=torch.int64).pin_memory()
                self._status_host.copy_(self._status, non_blocking=True)
                self._status_event = torch.cuda.Event(); self._status_event.record()
            else:
                # eager: every step gets its OWN snapshot and clears the word behind it (all of this step's writers are upstream of
                # the main stream here, the next step's fronts fork from it), so that an overflow is attributed to exactly one step
                # however many steps are in flight
                snap = self._status_pool.pop() if self._status_pool else torch.zeros(4, dtype=torch.int64).pin_memory()
                snap.copy_(self._status, non_blocking=True)
                self._status.fill_(0)
                ev_s = torch.cuda.Event(); ev_s.record()
                self._status_pending.append((snap, ev_s))
        # chain the once-per-step activations (behind the projection half of the last tail); the per-Gaussian gradients are then
        # final, so their all-reduce (RCCL on the communication stream) overlaps the prefilter backward
        if tail_job is None:
            with torch.cuda.stream(pstream if pstream is not None else main):
                L.check(lib.gs_activation_chain(N, L.ptr(g_scales_act), L.ptr(scales_act), L.ptr(g_opac_act), L.ptr(opac_act),
                                                L.ptr(b["scales"]), L.ptr(b["opacities"]), st()), "gs_activation_chain")
            if pstream is not None:
                for t in (scales_act, opac_act):
                    t.record_stream(pstream)
        return _Views(b, images if keep_images else None, g_base, g_levels, g_flat, env, sharded, world, all_reduce, main, pstream,
                      tail_job, smooth_grads)

    def _step(self, cameras, upstream, all_reduce, keep_images, smoothing: Optional[Smoothing] = None):
        """One whole step: geometry (the first view binned under the prefilter), views, _finish."""
        geo = self._geometry(cameras, bin_first=self.prefilter)
        return self._finish(self._views(cameras, upstream, all_reduce, keep_images, geo, smoothing=smoothing))

    def _finish(self, ctx: _Views):
        """What follows the views of a step: gradient all-reduce (its per-Gaussian part under the prefilter backward) and the
        prefilter backward on the texel gradients summed over the views (and, sharded, over the ranks)."""
        import torch.distributed as dist
        b, env, main = ctx.b, ctx.env, ctx.main
        pstream = ctx.pstream                                 # the per-Gaussian gradients become final on this stream (None: on main)
        chunked = ctx.tail_job is not None
        if chunked:                                           # last tail in Gaussian-range chunks, each summed over the ranks as it ends
            pstream = self._chunked_tail(ctx)
            main.wait_stream(self._tail_stream)               # the texel gradients are complete behind the last chunk's shading half
        head_stream = pstream if pstream is not None else main
        if ctx.sharded:
            grp = self._prefilter_group()
            dist.all_reduce(ctx.g_flat, op=dist.ReduceOp.SUM, group=grp)         # texel gradients of ALL views: needed by every share
            if not chunked:
                start_head, _ = self.bucket.all_reduce_split("cubemap")
                with torch.cuda.stream(head_stream):
                    start_head()                                # per-Gaussian segments: communication stream, default communicator
            g_cube = as_splitsum_backward(ctx.g_base, ctx.g_levels, min_roughness=env.min_roughness, max_roughness=env.max_roughness,
                                          rank=dist.get_rank(), world=ctx.world, group=grp, sharded=True)
            b["cubemap"].copy_(g_cube)                          # identical on every rank: not reduced again
            if pstream is not None:
                main.wait_stream(pstream)
            self.bucket.all_reduce_names(["exposure"])          # queues behind the head on the communication stream, then joins it
            return b, ctx.images
        start_head, finish = self.bucket.all_reduce_split("cubemap") if ctx.all_reduce else ((lambda: None), (lambda: None))
        if not chunked:
            with torch.cuda.stream(head_stream):
                start_head()
        if self.prefilter:                                      # (the finest level's transposed apply writes the bucket's slice itself)
            as_splitsum_backward(ctx.g_base, ctx.g_levels, min_roughness=env.min_roughness, max_roughness=env.max_roughness,
                                 out=b["cubemap"])
        if pstream is not None:
            main.wait_stream(pstream)
        finish()
        return b, ctx.images

    def _chunked_tail(self, ctx: _Views):
        """The last tail launch of a step with collectives, in `n_chunks` Gaussian ranges: shading half of chunk k on the tail stream,
        its projection half + the activation chain of those rows on a front stream behind it, and -- as soon as they are final -- the
        all-reduce of exactly those rows of the seven per-Gaussian segments on the communication stream (GradBucket.all_reduce_rows),
        while the tail stream already computes chunk k + 1.  The tail kernels index every per-Gaussian array by the Gaussian, so a
        chunk is the same launch on pointers moved to the range's first row.  With one view per rank (BASELINE config 4) the 149 MB
        all-reduce is otherwise fully exposed behind a 0.33 ms tail; here all but the last quarter of it runs under the tail.
        Returns the stream on which the per-Gaussian gradients became final."""
        job = ctx.tail_job
        lib = L.lib()
        b = ctx.b
        self.chunked_tails += 1
        (views, means, quats, scales_act, opac_act, normals, kd, ks, e, eg, mr, mm, mode, g_means, g_quats, g_scales_act, g_opac_act,
         g_normals, g_kd, g_ks) = job["targs"]
        N = means.shape[0]
        C_ = job["n_chunks"]
        bounds = [min(N, ((N * k // C_ + 1023) // 1024) * 1024) for k in range(C_)] + [N]
        tail, pstream = self._tail_stream, self._side_stream[0]
        names = [k for k in PARAM_NAMES if k not in ("cubemap", "exposure")]
        tail.wait_stream(ctx.main)                            # (behind the last compositor backward; a captured views segment: behind its replay)
        for c in range(C_):
            n0, n1 = bounds[c], bounds[c + 1]
            if n1 <= n0:
                continue
            sl = lambda t: t[n0:n1]
            vc = [(vm, K, cp, vis, vp, pidx[n0:n1], W, H) for (vm, K, cp, vis, vp, pidx, W, H) in views]
            args = (vc, sl(means), sl(quats), sl(scales_act), sl(opac_act), sl(normals), sl(kd), sl(ks), e, eg, mr, mm, mode, sl(g_means),
                    sl(g_quats), sl(g_scales_act), sl(g_opac_act), sl(g_normals), sl(g_kd), sl(g_ks))
            with torch.cuda.stream(tail):
                F.tail_multi_stage(*args, accumulate=job["accumulate"], parts=1)
                ev_sh = torch.cuda.Event(); ev_sh.record(tail)
            with torch.cuda.stream(pstream):
                pstream.wait_event(ev_sh)                      # (v_means: the projection half adds to what the shading half stored)
                F.tail_multi_stage(*args, accumulate=job["accumulate"], parts=2)
                L.check(lib.gs_activation_chain(n1 - n0, L.ptr(sl(g_scales_act)), L.ptr(sl(scales_act)), L.ptr(sl(g_opac_act)),
                                                L.ptr(sl(opac_act)), L.ptr(b["scales"][n0:n1]), L.ptr(b["opacities"][n0:n1]), L.stream()),
                        "gs_activation_chain")
                if ctx.smooth_grads is not None:              # the smoothing scratch of these rows, behind this chunk's shading half
                    for name, g in zip(("kd", "ks", "normals"), ctx.smooth_grads):
                        b[name][n0:n1].add_(g[n0:n1])
                ev_c = torch.cuda.Event(); ev_c.record(pstream)
            self.bucket.all_reduce_rows(names, n0, n1, after=ev_c)
        if not ctx.captured:                                  # (a captured segment's tensors live in the graph's private pool)
            for tv in views:
                for t in tv[:6]:
                    t.record_stream(tail); t.record_stream(pstream)
            for t in (scales_act, opac_act, g_scales_act, g_opac_act):
                t.record_stream(tail); t.record_stream(pstream)
        return pstream

    def _capture(self, n_pinned: int, record):
        """What capture() and capture_views() share.  `record(phase)` issues the work to be captured, each graph's share of it under
        `with phase():`.  It runs once eagerly on a side stream -- the allocator warm-up torch.cuda.graph asks for -- and once more
        with every phase() a new graph (the later graphs share the first one's memory pool; phase(own_pool=True): a pool of its own,
        for a graph that replays at the same time as another one).  Returns (what that second run returned,
        the graphs, check): check() synchronises and returns False if a view of the last replay exceeded the capacity OR left the
        depth range of the 24-bit binning keys baked into the graphs; they are then stale and `check.stale` is set."""
        dev = self.p.means.device
        F.reserve_pinned(n_pinned)                             # pinned buffers cannot be allocated while a stream is capturing
        if self._status is None:
            self._status = torch.zeros(4, dtype=torch.int64, device=dev)
        if self._status_host is None:
            self._status_host = torch.zeros(4, dtype=torch.int64).pin_memory()
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(warm):
            record(lambda own_pool=False: contextlib.nullcontext())
        torch.cuda.current_stream(dev).wait_stream(warm)
        torch.cuda.synchronize(dev)
        self.poll_capacity(_internal=True)                    # an overflow of the warm-up step stays pending for the caller's next poll
        graphs = []

        def phase(own_pool: bool = False):
            graphs.append(torch.cuda.CUDAGraph())
            return torch.cuda.graph(graphs[-1], pool=graphs[0].pool() if (len(graphs) > 1 and not own_pool) else None)
        out = record(phase)
        counts = [hc for hc, _ in self._seen_counts]          # refreshed by every replay (D2H copies are graph nodes)
        self._seen_counts = []
        self._status_event = None
        cap = self._i_cap
        status_host = self._status_host

        def check() -> bool:
            torch.cuda.synchronize(dev)
            worst = max([int(hc[1]) for hc in counts] + [0])
            truncated, key32, need_i = F.status_overflow(status_host)
            overflow = truncated or worst > cap
            if overflow:
                check.stale = True
                self.truncated_steps += 1
                self._key32 = self._key32 or key32
                self._exact_max_i = max(self._exact_max_i, worst, need_i)
                self._status.zero_(); status_host.zero_()
            return not overflow
        check.stale = False
        return out, graphs, check

    def capture(self, cameras: List[Camera], upstream: Callable[[int, Tensor], Tensor], keep_images: bool = False,
                smoothing: Optional[Smoothing] = None):
        """One fused step over a FIXED camera list recorded into a HIP graph (torch.cuda.CUDAGraph): possible because in
        capacity mode a step has fixed launch shapes and no host synchronisation.  Returns `replay() -> (grads, images)`:
        the gradients land in this engine's bucket, exactly as after __call__(..., all_reduce=False); the caller reduces
        them over the ranks itself (collectives stay outside the graph).  `upstream` is traced once: it must compute
        d(loss)/d(image) with device-side operations on buffers that keep their addresses (update ground-truth images in
        place between replays).  Parameters are read from the tensors bound at capture time (update them in place).
        replay.check() synchronises and returns False if a view exceeded the capacity OR left the depth range of the 24-bit binning
        keys baked into the graph: the graph is then stale (it would keep replaying with clamped keys, i.e. a wrong depth order) --
        call poll_capacity() and capture() AGAIN before the next replay; a replay after a False check() raises."""
        if smoothing is not None:
            raise NotImplementedError("the smoothing regularisers run on the eager fused step (__call__), not in a captured graph")
        if not (self.fused and self.mode == "pbr"):
            raise RuntimeError("capture() needs the fused path")
        if self._i_cap is None:
            raise RuntimeError("capture() needs a known capacity: run one eager step and poll_capacity(wait=True) first")

        def record(phase):
            with phase():
                return self._step(cameras, upstream, False, keep_images)
        out, (graph,), check = self._capture(2 * len(cameras) + 2, record)

        def replay():
            if check.stale:
                raise RuntimeError("this captured step overflowed its capacity / key range (check() returned False): capture() again")
            graph.replay()
            return out
        replay.check = check
        replay.graph = graph
        return replay

    def capture_views(self, cameras: List[Camera], upstream: Callable[[int, Tensor], Tensor], all_reduce: bool = True,
                      keep_images: bool = False, smoothing: Optional[Smoothing] = None):
        """The VIEWS of a step -- everything between the pyramid and the texel gradients: shading, projection, binning, compositor,
        tone map, upstream and the whole per-view backward -- recorded into one HIP graph, with the prefilter and every collective
        OUTSIDE of it.  This is the shape BASELINE config 4 needs (one view per GPU): a single view is ~45 launches, 2.3-4.5 ms from
        Python depending on the host core against 2.1 ms of kernel time, while the sharded prefilter, the all-reduce of the texel
        gradients and the flat gradient all-reduce (RCCL) cannot be captured together with it.  Returns `step() -> (grads, images)`
        = prefilter forward (eager, sharded over the ranks when all_reduce and world > 1) -> copy into the graph's pyramid buffers ->
        graph replay -> prefilter backward + all-reduces (eager); same results as __call__.  `upstream` as in capture();
        step.check() as replay.check()."""
        if smoothing is not None:
            raise NotImplementedError("the smoothing regularisers run on the eager fused step (__call__), not in a captured graph")
        if not (self.fused and self.mode == "pbr" and self.prefilter):
            raise RuntimeError("capture_views() needs the fused path with the prefilter in the step")
        if self._i_cap is None:
            raise RuntimeError("capture_views() needs a known capacity: run one eager step and poll_capacity(wait=True) first")
        dev = self.p.means.device
        world, sharded = self._sharding(all_reduce)
        first = self._pyramid(sharded, world)
        pyramid = TextureSplitSum(first.base.detach().clone(), [l.detach().clone() for l in first.levels], first.min_roughness,
                                  first.max_roughness)
        slots = [pyramid.base] + list(pyramid.levels)
        # THREE graphs (GEOSPLAT_GEO_GRAPH=0: one).  With one view per GPU the chain front -> binning -> record stream -> compositor ->
        # tail is serial; two pieces of it need less than the whole chain has:
        #   geometry graph: projection, depth keys, binning of the views -- nothing that needs the pyramid -- on its own stream BESIDE the
        #                   eager (sharded) prefilter forward and its all-reduce;
        #   records graph : the shading of those views -- needs the pyramid, NOT the binning -- behind the prefilter, beside whatever is
        #                   left of the geometry graph (0.39 ms of front + binning against 0.1 ms of sharded prefilter at 8 GPUs);
        #   views graph   : record stream, compositor, loss cotangent, compositor backward, background tails -- behind both.
        # The last tail launch and every collective stay eager (_finish): its Gaussian-range chunks are summed over the ranks while the
        # next chunk is computed.
        # The records graph reads the activations, and nothing orders it behind the geometry graph: they are computed on the caller's
        # stream into these buffers BEFORE the geometry graph forks from it, and every graph only reads them.  It also runs while the
        # geometry graph's temporaries are live, so it allocates from a pool of its own; the views graph, which replays behind both,
        # shares the geometry graph's.
        two = os.environ.get("GEOSPLAT_GEO_GRAPH", "1") != "0"
        act = (torch.empty_like(self.p.scales.detach()), torch.empty_like(self.p.opacities.detach().squeeze(-1)))
        self._activations(act)

        def record(phase):                                     # (a captured phase: every forked stream joins before the capture ends)
            geo = recs = None
            if two:
                with phase():
                    geo = self._geometry(cameras, bin_first=True, act=act)
                    for sd in self._side_stream:
                        torch.cuda.current_stream(dev).wait_stream(sd)
                with phase(own_pool=True):
                    recs = self._records(cameras, geo, pyramid)
            with phase():
                if geo is None:
                    geo = self._geometry(cameras, bin_first=False, act=act)
                ctx = self._views(cameras, upstream, all_reduce, keep_images, geo, env=pyramid, recs=recs)
                if ctx.pstream is not None:
                    ctx.main.wait_stream(ctx.pstream)
                    ctx.pstream = None
            return ctx
        # (the geometry and records fronts carry their own count read-backs)
        ctx, graphs, check = self._capture(6 * len(cameras) + 2, record)
        geo_graph, rec_graph, graph = graphs if two else (None, None, graphs[0])
        geo_stream = L.shared_stream(dev, "geo") if two else None
        ctx.main = None
        ctx.captured = True

        def step():
            if check.stale:
                raise RuntimeError("these captured views overflowed their capacity / key range (check() returned False): capture_views() again")
            cur = torch.cuda.current_stream(dev)
            self._activations(act)                             # (read by all three graphs; the previous step's readers joined `cur`)
            if two:
                geo_stream.wait_stream(cur)                    # (the parameters and activations of this step are final on the caller's stream)
                with torch.cuda.stream(geo_stream):
                    geo_graph.replay()
            env = self._pyramid(sharded, world)
            torch._foreach_copy_(slots, [env.base] + list(env.levels))
            if two:
                rec_graph.replay()                             # shading of the views: beside the geometry graph
                cur.wait_stream(geo_stream)
            graph.replay()
            ctx.main = cur
            return self._finish(ctx)
        step.check = check
        step.graph = graph
        step.geo_graph = geo_graph
        step.rec_graph = rec_graph
        return step

    def _throttle(self) -> None:
        """Bound how far the host runs ahead of the GPU.  The step has no host synchronisation, the host enqueues it in 3-5 ms
        against 15 ms on the GPU, and HIP queues without limit: after 400 steps the host was 200 steps ahead and the caching
        allocator -- whose blocks are only reusable once the streams they were recorded on have passed them -- held 186 GiB for
        a step whose live memory is 3.8 GiB (scripts/soak.py).  At most GEOSPLAT_STEPS_IN_FLIGHT (default 3) steps are enqueued
        beyond the one the GPU is working on; the wait polls the event (no blocking call: the step stays clean under
        torch.cuda.set_sync_debug_mode) and never leaves the GPU idle, since one whole step is still queued behind it."""
        if self._in_flight is None:
            return
        import time
        while len(self._in_flight) >= self._max_in_flight:
            ev = self._in_flight[0]
            while not ev.query():
                time.sleep(5e-5)
            self._in_flight.popleft()

    def _note_status(self, word: Tensor):
        """A host copy of the status word of a finished step: a truncated step is counted in `truncated_steps`, and a depth outside
        the 24-bit key range means 32-bit keys from now on.  Returns (truncated, the intersection count it required)."""
        truncated, key32, need_i = F.status_overflow(word)
        if truncated:
            self.truncated_steps += 1
            self._key32 = self._key32 or key32
        return truncated, need_i

    def poll_capacity(self, wait: bool = False, _internal: bool = False) -> bool:
        """Host side of the capacity protocol; never blocks unless `wait`.  Looks at what the earlier steps left in pinned memory:
        the per-view (V, I) counts set / raise the intersection capacity (1.25 x the largest count seen, rounded up to 64 Ki),
        and the overflow word tells whether a view exceeded the capacity it ran with.  Returns False in that case -- that step's
        gradients are incomplete (memory-safe, a truncated view) and the caller should repeat it; the capacity has already been
        raised.  An overflow is never lost: RenderStep.__call__ polls before every step (non-blocking) and, if IT sees the
        word set, counts the step in `truncated_steps` and keeps the fact until the next poll_capacity() of the caller, which
        then returns False.  A trainer that must not consume a truncated step calls poll_capacity(wait=True) before its optimiser
        step (stage1.py does); bench.py reports `truncated_steps`."""
        ok = True
        max_i, self._exact_max_i = self._exact_max_i, 0
        still = []
        for hc, ev in self._seen_counts:                      # front_stage's pinned {V, I, ~min depth bits, max depth bits}
            if wait:
                ev.synchronize()
            if ev.query():
                max_i = max(max_i, int(hc[1]))
                self._key_lo, self._key_hi = F.learn_depth_range(self._key_lo, self._key_hi, hc)
                F.release_counts4(hc)
            else:
                still.append((hc, ev))
        self._seen_counts = still
        while self._status_pending:                           # eager steps, oldest first; each snapshot is inspected exactly once
            snap, ev_s = self._status_pending[0]
            if wait:
                ev_s.synchronize()
            if not ev_s.query():
                break
            self._status_pending.popleft()
            truncated, need_i = self._note_status(snap)
            if truncated:
                ok, max_i = False, max(max_i, need_i)
            self._status_pool.append(snap)
        if self._status_event is not None:                    # the single buffer of a captured step (see capture / capture_views)
            if wait:
                self._status_event.synchronize()
            if self._status_event.query():
                self._status_event = None
                truncated, need_i = self._note_status(self._status_host)
                if truncated:
                    ok, max_i = False, max(max_i, need_i)
                    self._status.zero_(); self._status_host.zero_()
        if self._use_capacity and max_i > 0:
            want = ((int(max_i * self._cap_margin) + 65535) // 65536) * 65536
            if self._i_cap is None or want > self._i_cap or max_i > self._i_cap:
                self._i_cap = max(want, self._i_cap or 0)
        if _internal:
            self._overflow_unreported = self._overflow_unreported or not ok
        elif self._overflow_unreported:
            ok, self._overflow_unreported = False, False
        return ok

    def __call__(self, cameras: List[Camera], upstream: Callable[[int, Tensor], Tensor], all_reduce: bool = True,
                 keep_images: bool = False, smoothing: Optional[Smoothing] = None):
        """Forward + backward for `cameras`; `upstream(i, image)` returns d(loss)/d(image) for local view i.
        Returns (grads dict of views into the flat bucket, images or None).  `smoothing` (fused PBR path only): the smoothing
        regularisers of the local views join the step -- their gradients are in the bucket, their sum in `last_smoothing_loss`."""
        if smoothing is not None and not (self.fused and self.mode == "pbr"):
            raise NotImplementedError("the smoothing regularisers run on the fused PBR step only")
        if self.fused and self.mode == "pbr":
            self._throttle()                                 # first: the step that just left the window has finished, its word is readable
            self.poll_capacity(_internal=True)               # non-blocking: counts / overflow words of the finished steps (an overflow
                                                             # seen here is kept for the caller's next poll_capacity())
            out = self._step(cameras, upstream, all_reduce, keep_images, smoothing)
            if self._in_flight is not None:
                ev = torch.cuda.Event(); ev.record()
                self._in_flight.append(ev)
            return out
        p = self.p
        leaves = {k: v.detach().requires_grad_(True) for k, v in p.named().items()}
        if self.prefilter:
            env = as_splitsum(leaves["cubemap"])
        else:
            if self._static_env is None:
                with torch.no_grad():
                    self._static_env = as_splitsum(p.cubemap)
            env = self._static_env
        # cut the graph at the pyramid so that the prefilter backward runs ONCE with the summed texel gradients
        base_leaf = env.base.detach().requires_grad_(True)
        level_leaves = [l.detach().requires_grad_(True) for l in env.levels]
        env_leaf = TextureSplitSum(base_leaf, level_leaves, env.min_roughness, env.max_roughness)

        class _G:  # raw Splats-like view
            means = leaves["means"]; scales = leaves["scales"]; quats = leaves["quats"]; opacities = leaves["opacities"]
        attrs = RenderableAttrs(kd=leaves["kd"], ks=leaves["ks"], normals=leaves["normals"])
        images = []
        for i, cam in enumerate(cameras):
            img = attrs.splat(_G, [cam], exposure=leaves["exposure"], envmap=env_leaf, min_roughness=self.min_roughness,
                              max_metallic=self.max_metallic, mode=self.mode, tone_type=self.tone_type, fg_lut=self.fg_lut)
            img.backward(upstream(i, img.detach()))
            if keep_images:
                images.append(img.detach())
        if self.prefilter:
            pairs = [(env.base, base_leaf.grad)] + [(l, ll.grad) for l, ll in zip(env.levels, level_leaves)]
            outs = [o for o, g in pairs if g is not None]
            gouts = [g for o, g in pairs if g is not None]
            if outs:
                torch.autograd.backward(outs, gouts)
        grads = {k: leaves[k].grad for k in PARAM_NAMES}
        self.bucket.pack(grads)
        if all_reduce:
            self.bucket.all_reduce()
        return self.bucket.unpack(), (images if keep_images else None)


class MeshStep:
    """mesh -> Gaussians -> render -> backward to the mesh: the geometry half of the reference's stage-1 loop
    (GeoSplatter.get_gaussians_from_mesh, rfstudio/model/geosplat.py:620-672, then render_report) with the
    FlexiCubes extraction and the hash-grid field replaced by explicit leaves:
    `vertices` [V,3] and per-Gaussian `kd` [6F,3] / `ks` [6F,2].  Per step:
        vertex normals -> MGAdapter (HIP, mesh.py) -> RenderStep (fused C-ABI path, per-Gaussian gradient bucket,
        all-reduce at that cut) -> MGAdapter backward -> vertex-normal backward -> d loss / d vertices."""

    def __init__(self, vertices: Tensor, faces: Tensor, kd: Tensor, ks: Tensor, cubemap: Tensor, exposure: Tensor,
                 **render_kwargs):
        from .mesh import mesh_to_splats, vertex_normals
        self._m2s, self._vn = mesh_to_splats, vertex_normals
        self.vertices, self.faces, self.kd, self.ks, self.cubemap, self.exposure = vertices, faces, kd, ks, cubemap, exposure
        self.render_kwargs = render_kwargs
        self.step: Optional[RenderStep] = None

    def __call__(self, cameras: List[Camera], upstream: Callable[[int, Tensor], Tensor], all_reduce: bool = True,
                 keep_images: bool = False):
        v = self.vertices.detach().requires_grad_(True)
        sp, nrm = self._m2s(v, self.faces, self._vn(v, self.faces))
        params = PathParams(sp.means.detach(), sp.scales.detach(), sp.quats.detach(), sp.opacities.detach(), nrm.detach(),
                            self.kd.detach(), self.ks.detach(), self.cubemap.detach(), self.exposure.detach())
        if self.step is None:
            self.step = RenderStep(params, **self.render_kwargs)
        else:
            self.step.rebind(params)
        grads, images = self.step(cameras, upstream, all_reduce=all_reduce, keep_images=keep_images)
        # shading normals == splat colours of the adapter: their gradient rides on `nrm`
        torch.autograd.backward([sp.means, sp.scales, sp.quats, nrm],
                                [grads["means"], grads["scales"], grads["quats"], grads["normals"]])
        out = {"vertices": v.grad, "kd": grads["kd"], "ks": grads["ks"], "cubemap": grads["cubemap"],
               "exposure": grads["exposure"]}
        return out, images


def params_from_scene(scene, device, exposure: float = 1.0) -> PathParams:
    sp: SplatSet = scene.splats
    d = lambda t: t.to(device).contiguous()
    return PathParams(d(sp.means), d(sp.scales), d(sp.quats), d(sp.opacities), d(scene.normals), d(scene.kd),
                      d(scene.ks), d(scene.cubemap), torch.tensor(exposure, dtype=torch.float32, device=device))
