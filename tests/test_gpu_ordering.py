"""Ordering BETWEEN the kernels of a step, under forced stalls.

A step of engine.RenderStep spreads over the caller's stream, two front streams, a tail stream and (capture_views) a `geo` stream,
and the call shape (viewbatch) shares those streams.  A missing stream edge does not fault: it gives a wrong image or gradient
only when one stream happens to run late.  These tests make one stream run late on purpose -- a bounded `torch.cuda._sleep` on it,
from outside the product code (monkeypatched module attributes, the `upstream` callback, the shared `geo` stream) -- and compare
the results with the same run without the stall and with the op-by-op autograd path (GEOSPLAT_SPLAT=ops).  Inside capture() /
capture_views() the stall is recorded into the graph, so the branch structure of the graphs is tested too.  Every run does
three steps with no host synchronisation in between, the parameters changed in place before each step (as an optimizer does),
and every graph replays ONCE per parameter set.
"""
import threading

import pytest
import torch

from geosplatting_amd import _lib as L
from geosplatting_amd import front as F
from geosplatting_amd.cameras import Camera
from tests.util import compare_grads, same_step, small_engine_scene

pytestmark = pytest.mark.gpu

TARGET_MS = 2.0          # one stall
MAX_CYCLES = 5_000_000   # 50 ms even if _sleep counted a 100 MHz clock: a wrong calibration cannot stall for long
N_STEPS = 3


# ----------------------------------------------------------------------------------------------------------------- stalls
@pytest.fixture(scope="module")
def sleep_cycles(cuda):
    """Cycles of torch.cuda._sleep for about TARGET_MS, calibrated with events (the rate of the clock it counts is not assumed)."""
    def timed(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch.cuda._sleep(cycles); b.record()
        b.synchronize()
        return a.elapsed_time(b)
    probe = 200_000
    timed(probe)
    ms = timed(probe)
    cycles = min(MAX_CYCLES, int(probe * TARGET_MS / max(ms, 1e-3)))
    got = timed(cycles)
    print(f"\n _sleep: {probe} cycles {ms:.3f} ms -> {cycles} cycles {got:.3f} ms")
    assert 0.75 * TARGET_MS <= got <= 50.0, (cycles, got)
    return cycles, got


class Stall:
    """A bounded sleep on the current stream.  Eager calls are timed with events on that stream; a call inside a graph capture
    also adds one to a device counter behind the sleep, so that the replays prove the sleep node ran."""

    def __init__(self, cycles_ms, dev):
        self.cycles, self.ms = cycles_ms
        self.events = []
        self.captured = 0
        self.hits = torch.zeros((), dtype=torch.int64, device=dev)

    def __call__(self):
        if torch.cuda.is_current_stream_capturing():
            self.captured += 1
            torch.cuda._sleep(self.cycles)
            self.hits.add_(1)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); torch.cuda._sleep(self.cycles); b.record()
            self.events.append((a, b))

    def check(self, replays):
        """After a synchronisation: every eager stall really stalled its stream, every captured one replayed with its graph."""
        for a, b in self.events:
            assert a.elapsed_time(b) >= 0.5 * self.ms, (a.elapsed_time(b), self.ms)
        assert int(self.hits) == self.captured * replays
        return len(self.events) + self.captured


def _view_index(cams, entries):
    """data_ptr of a camera's device view matrix -> view index, from a camera cache's (pose, (view matrix, K, position)) pairs."""
    by_pose = {id(c.c2w): i for i, c in enumerate(cams)}
    return {t[0].data_ptr(): by_pose[id(c2w)] for c2w, t in entries if id(c2w) in by_pose}


def _install(monkeypatch, point, stall, view_of):
    """Stall the stream of `point` from outside the product: 'front<k>' -- front_stage and bin_stage of view k (view_of() maps a
    view matrix to its view); 'tail<parts>' -- the tail launches with that `parts` value (7: background, 1: shading half of the last
    one on the tail stream, 2: its projection half on a front stream).  'caller' and 'geo' are injected by the runs themselves."""
    if point.startswith("front"):
        k = int(point[5:])
        front_stage, bin_stage, mine = F.front_stage, F.bin_stage, []

        def front_wrap(*a, **kw):
            if view_of().get(a[7].data_ptr()) == k:
                stall()
                fr = front_stage(*a, **kw)
                mine.append(fr)
                return fr
            return front_stage(*a, **kw)

        def bin_wrap(fr, *a, **kw):
            if any(fr is m for m in mine):
                stall()
            return bin_stage(fr, *a, **kw)
        monkeypatch.setattr(F, "front_stage", front_wrap)
        monkeypatch.setattr(F, "bin_stage", bin_wrap)
    elif point.startswith("tail"):
        want = int(point[4:])
        tail_multi_stage = F.tail_multi_stage

        def tail_wrap(*a, parts=3, **kw):
            if parts == want:
                stall()
            return tail_multi_stage(*a, parts=parts, **kw)
        monkeypatch.setattr(F, "tail_multi_stage", tail_wrap)
    else:
        assert point in ("caller", "geo"), point


# ----------------------------------------------------------------------------------------------------------------- scene
@pytest.fixture(scope="module")
def scene(cuda):
    sc, cams, ups = small_engine_scene()
    g = torch.Generator().manual_seed(77)
    n = sc.splats.num
    # the in-place parameter change before every step: an optimizer's update, the same in every run
    nudge = dict(means=2e-3 * torch.randn(n, 3, generator=g), scales=1e-2 * torch.randn(n, 3, generator=g),
                 opacities=5e-2 * torch.randn(n, 1, generator=g))
    return sc, cams, [u.to(cuda) for u in ups], {k: v.to(cuda) for k, v in nudge.items()}


def _nudge(p, nudge):
    """In place, on the caller's stream, no host synchronisation: what an optimizer step does to the parameters."""
    with torch.no_grad():
        p["means"].add_(nudge["means"])
        p["scales"].add_(nudge["scales"])
        p["opacities"].add_(nudge["opacities"].reshape(p["opacities"].shape))
        p["kd"].mul_(0.97)
        p["cubemap"].mul_(1.05)


def _clone(grads, images):
    return {k: v.detach().clone() for k, v in grads.items()}, [im.detach().clone() for im in images]


def _host(out):
    return {k: v.cpu() for k, v in out[0].items()}, [im.cpu() for im in out[1]]


# ----------------------------------------------------------------------------------------------------------------- engine
def _engine_run(cuda, monkeypatch, scene, mode, point=None, stall=None):
    """Three steps of the engine in `mode` (eager | capture | views1 | views0: capture_views with GEOSPLAT_GEO_GRAPH=1 / 0), the
    parameters nudged before each; with `point`, `stall` is injected there.  Returns the three (grads, images) on the host and the
    final parameters."""
    from geosplatting_amd.engine import RenderStep, params_from_scene
    sc, cams, ups, nudge = scene
    if mode.startswith("views"):
        monkeypatch.setenv("GEOSPLAT_GEO_GRAPH", mode[-1])
    step = RenderStep(params_from_scene(sc, cuda, exposure=1.1))
    plain = lambda j, img: ups[j]
    step(cams, plain, all_reduce=False)                               # exact step: learns the capacity and the key range
    torch.cuda.synchronize()
    assert step.poll_capacity(wait=True) and step._i_cap is not None
    upstream = plain
    if point is not None:
        _install(monkeypatch, point, stall, lambda: _view_index(cams, [(e[0], e[3]) for e in step._cam_cache.values()]))
        if point == "caller":                                          # between compositor forward and backward of every view
            def upstream(j, img):
                stall()
                return ups[j]
    if mode == "eager":
        run = lambda: step(cams, upstream, all_reduce=False, keep_images=True)
    elif mode == "capture":
        run = step.capture(cams, upstream, keep_images=True)
    else:
        run = step.capture_views(cams, upstream, all_reduce=False, keep_images=True)
    geo = L.shared_stream(cuda, "geo")
    outs = []
    for _ in range(N_STEPS):
        _nudge(step.p.named(), nudge)
        if point == "geo":
            with torch.cuda.stream(geo):
                stall()
        outs.append(_clone(*run()))                                   # (cloned on the caller's stream)
    torch.cuda.synchronize()
    if mode != "eager":
        assert run.check()
    assert step.poll_capacity(wait=True)
    if point is not None:
        assert stall.check(N_STEPS if mode != "eager" else 0) > 0
    return [_host(o) for o in outs], {k: v.detach().clone() for k, v in step.p.named().items()}


_refs = {}


def _reference(cuda, monkeypatch, scene, mode):
    """The same run without a stall (per mode), and the op-by-op autograd step at the final parameters (once)."""
    if mode not in _refs:
        with monkeypatch.context() as m:
            _refs[mode] = _engine_run(cuda, m, scene, mode)
    if "ops" not in _refs:
        from geosplatting_amd.engine import PathParams, RenderStep
        final = _refs[mode][1]
        with monkeypatch.context() as m:
            m.setenv("GEOSPLAT_SPLAT", "ops")
            ops = RenderStep(PathParams(**{k: v.clone() for k, v in final.items()}), fused=False)
            ups = scene[2]
            _refs["ops"] = (_host(_clone(*ops(scene[1], lambda j, img: ups[j], all_reduce=False, keep_images=True))), final)
    ops, ops_params = _refs["ops"]
    for k, v in _refs[mode][1].items():
        assert torch.equal(v, ops_params[k]), k                       # (the same nudges from the same start in every mode)
    return _refs[mode][0], ops


def _check_engine(got, ref, ops):
    for r, g in zip(ref, got):
        same_step(r, g)
    for a, b in zip(got[-1][1], ops[1]):
        assert torch.equal(a, b)                                      # the engine's images are the op-by-op ones bit for bit
    compare_grads(got[-1][0], ops[0], tol=5e-5)                       # (5e-5: test_gpu_front's engine-vs-ops bar, float atomics)


ENGINE_CASES = ([(m, p) for m in ("eager", "capture", "views1", "views0")
                 for p in ("caller", "front0", "front1", "front3", "tail7", "tail1", "tail2")] + [("views1", "geo")])


@pytest.mark.parametrize("mode,point", ENGINE_CASES)
def test_engine_step_under_a_stalled_stream(cuda, monkeypatch, scene, sleep_cycles, mode, point):
    """One stream of the engine's step runs late: the images must not change and the gradients only by the order of the float
    atomics, in the eager step, in capture() and in both shapes of capture_views().  ('geo': the `geo` stream, on which the geometry
    graph of capture_views() replays, starts late -- the records graph beside it must still see this step's activations.)"""
    ref, ops = _reference(cuda, monkeypatch, scene, mode)
    got, _ = _engine_run(cuda, monkeypatch, scene, mode, point, Stall(sleep_cycles, cuda))
    _check_engine(got, ref, ops)


def test_views_graphs_replayed_once_per_parameter_set(cuda, monkeypatch, scene):
    """capture_views() with single replays and no stall: each step's graphs see that step's parameters (the double replay of
    test_gpu_parallel.py::test_views_segment_captured_in_hip_graph hides a graph that reads the previous step's values)."""
    ref, ops = _reference(cuda, monkeypatch, scene, "eager")
    got, _ = _engine_run(cuda, monkeypatch, scene, "views1")
    _check_engine(got, ref, ops)


# ----------------------------------------------------------------------------------------------------------------- device poses
def _exact_poses(cams, n_steps):
    """Per step, the cameras' poses jittered: rotations on a 2^-12 grid and positions on a 2^-8 grid, so that the view matrix
    (R^T, -R^T t: sums of three products) is exact in float32 and the same on the host and the device whatever the order."""
    g = torch.Generator().manual_seed(31)
    base = torch.stack([c.c2w for c in cams])
    base = torch.cat((torch.round(base[..., :3] * 4096) / 4096, torch.round(base[..., 3:] * 256) / 256), -1)
    jit = [torch.cat((torch.zeros(len(cams), 3, 3), torch.randint(-8, 9, (len(cams), 3, 1), generator=g) / 256), -1)
           for _ in range(n_steps)]
    return base, jit


def _pose_cams(cams, c2w):
    return [Camera(c2w[i], c.fx, c.fy, c.cx, c.cy, c.width, c.height) for i, c in enumerate(cams)]


def test_device_resident_poses_equal_host_poses(cuda, monkeypatch, scene, sleep_cycles):
    """Poses on the device, in new Camera objects every step (every step misses the engine's camera cache), written on the caller's
    stream behind a stall: the fronts that read the camera tensors on the front streams must be ordered behind them.  Images equal
    the same steps with the poses on the host."""
    from geosplatting_amd.engine import RenderStep, params_from_scene
    sc, cams, ups, nudge = scene
    base, jit = _exact_poses(cams, N_STEPS)
    plain = lambda j, img: ups[j]

    def run(device_poses, stall=None):
        step = RenderStep(params_from_scene(sc, cuda, exposure=1.1))
        step(_pose_cams(cams, base), plain, all_reduce=False)
        torch.cuda.synchronize()
        assert step.poll_capacity(wait=True)
        base_d, jit_d = base.to(cuda), [j.to(cuda) for j in jit]
        outs = []
        for k in range(N_STEPS):
            _nudge(step.p.named(), nudge)
            if device_poses:
                stall()
                c2w = base_d + jit_d[k]                               # (behind the stall on the caller's stream)
            else:
                c2w = base + jit[k]
            outs.append(_clone(*step(_pose_cams(cams, c2w), plain, all_reduce=False, keep_images=True)))
        torch.cuda.synchronize()
        assert step.poll_capacity(wait=True)
        return [_host(o) for o in outs]
    want = run(False)
    stall = Stall(sleep_cycles, cuda)
    got = run(True, stall)
    assert stall.check(0) == N_STEPS
    for w, g in zip(want, got):
        same_step(w, g)


def test_device_resident_pose_step_does_not_synchronise(cuda, scene):
    """A capacity-mode step over device-resident poses in new Camera objects (a camera-cache miss per view) issues no host
    synchronisation: the view matrix and K are built without host-to-device copies."""
    from geosplatting_amd.cameras import intrinsic_matrix, view_matrix
    from geosplatting_amd.engine import RenderStep, params_from_scene
    sc, cams, ups, _ = scene
    base, jit = _exact_poses(cams, 1)
    step = RenderStep(params_from_scene(sc, cuda, exposure=1.1))
    step(_pose_cams(cams, base), lambda j, img: ups[j], all_reduce=False)
    torch.cuda.synchronize()
    assert step.poll_capacity(wait=True) and step._i_cap is not None
    c2w = (base + jit[0]).to(cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                           # any synchronising torch call raises
    try:
        vm, K = view_matrix(c2w[0]), intrinsic_matrix(1.0, 2.0, 3.0, 4.0, device=cuda)
        grads, images = step(_pose_cams(cams, c2w), lambda j, img: ups[j], all_reduce=False, keep_images=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert step.poll_capacity(wait=True)
    assert torch.equal(vm.cpu(), view_matrix(c2w[0].cpu())) and torch.equal(K.cpu(), intrinsic_matrix(1.0, 2.0, 3.0, 4.0))
    want = RenderStep(params_from_scene(sc, cuda, exposure=1.1))
    host = _pose_cams(cams, base + jit[0])
    want(host, lambda j, img: ups[j], all_reduce=False)
    wg, wi = want(host, lambda j, img: ups[j], all_reduce=False, keep_images=True)
    torch.cuda.synchronize()
    same_step(_host(_clone(wg, wi)), _host(_clone(grads, images)))


# ----------------------------------------------------------------------------------------------------------------- call shape
def _leaves(sc, cuda):
    d = lambda x: x.clone().to(cuda).requires_grad_(True)
    sp = sc.splats
    return dict(means=d(sp.means), scales=d(sp.scales), quats=d(sp.quats), opacities=d(sp.opacities), normals=d(sc.normals),
                kd=d(sc.kd), ks=d(sc.ks), cubemap=d(sc.cubemap), exposure=torch.tensor(1.1, device=cuda, requires_grad=True))


def _forward(lv, cams, ups, stall=None):
    import geosplatting_amd as gs

    class G:
        means, scales, quats, opacities = lv["means"], lv["scales"], lv["quats"], lv["opacities"]
    attrs = gs.RenderableAttrs(kd=lv["kd"], ks=lv["ks"], normals=lv["normals"])
    env = gs.as_splitsum(lv["cubemap"])
    imgs = [attrs.splat(G, [c], exposure=lv["exposure"], envmap=env, min_roughness=0.1, max_metallic=1.0) for c in cams]
    if stall is not None:
        stall()                                                       # the caller's stream, in the loss
    return imgs, sum((im * u).sum() for im, u in zip(imgs, ups))


def _grads(lv):
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in lv.items()}


_ops_steps = {}


def _ops_reference(cuda, monkeypatch, scene):
    """The op-by-op call shape for the parameters of each of the N_STEPS steps."""
    if not _ops_steps:
        sc, cams, ups, nudge = scene
        lv = _leaves(sc, cuda)
        with monkeypatch.context() as m:
            m.setenv("GEOSPLAT_SPLAT", "ops")
            for k in range(N_STEPS):
                imgs, loss = _forward(lv, cams, ups)
                loss.backward()
                _ops_steps[k] = ([im.detach().clone() for im in imgs], _grads(lv))
                for v in lv.values():
                    v.grad = None
                _nudge(lv, nudge)
        torch.cuda.synchronize()
    return _ops_steps


@pytest.mark.parametrize("point,worker", [("caller", False), ("front1", False), ("tail7", False), ("tail1", False), ("tail2", False),
                                          ("tail1", True)])
def test_call_shape_under_a_stalled_stream(cuda, monkeypatch, scene, sleep_cycles, point, worker):
    """splat() (GEOSPLAT_SPLAT=fused) with one stream late: the caller's stream in the loss, a front of view 1, or a tail launch;
    three steps on the same leaves nudged in place, or (worker) each step's backward on a worker thread while the main thread
    already issues the forward of a second step on other leaves.  Images and gradients equal the op-by-op call shape."""
    import geosplatting_amd as gs
    sc, cams, ups, nudge = scene
    want = _ops_reference(cuda, monkeypatch, scene)
    monkeypatch.setenv("GEOSPLAT_SPLAT", "fused")
    gs.viewbatch.reset()
    warm = _leaves(sc, cuda)
    _forward(warm, cams, ups)[1].backward()                           # the exact first step at this image size: learns the capacity
    torch.cuda.synchronize()
    stall = Stall(sleep_cycles, cuda)
    st = gs.viewbatch._state(cuda)
    _install(monkeypatch, point, stall, lambda: _view_index(cams, [(e[0], e[2]) for e in st.cam_cache.values()]))
    caller = stall if point == "caller" else None
    got = []
    if not worker:
        lv = _leaves(sc, cuda)
        for k in range(N_STEPS):
            imgs, loss = _forward(lv, cams, ups, caller)
            loss.backward()
            got.append(([im.detach().clone() for im in imgs], _grads(lv)))
            for v in lv.values():
                v.grad = None
            _nudge(lv, nudge)
    else:
        lv = _leaves(sc, cuda)
        for k in range(N_STEPS):
            lvB = {n: v.detach().clone().requires_grad_(True) for n, v in lv.items()}
            imgsA, lossA = _forward(lv, cams, ups, caller)
            ev = torch.cuda.Event(); ev.record()
            errors = []

            def work():
                try:
                    with torch.cuda.device(cuda):
                        torch.cuda.current_stream().wait_event(ev)
                        lossA.backward()
                        torch.cuda.current_stream().synchronize()
                except BaseException as e:                             # noqa: BLE001
                    errors.append(e)
            th = threading.Thread(target=work)
            th.start()
            imgsB, lossB = _forward(lvB, cams, ups, caller)            # the next step's forward while this step's backward runs
            th.join()
            assert not errors, errors
            lossB.backward()
            got.append(([im.detach().clone() for im in imgsA], _grads(lv)))
            got.append(([im.detach().clone() for im in imgsB], _grads(lvB)))
            for v in lv.values():
                v.grad = None
            _nudge(lv, nudge)
    torch.cuda.synchronize()
    assert stall.check(0) > 0
    for i, (imgs, grads) in enumerate(got):
        w_imgs, w_grads = want[i // 2 if worker else i]
        for a, b in zip(imgs, w_imgs):
            assert torch.equal(a, b), i
        print(f"\n step {i}")
        compare_grads(grads, w_grads, tol=5e-5)
    gs.viewbatch.reset()
