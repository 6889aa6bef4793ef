"""GPU: the cull-log backward (gs_raster_composite_tone_log + gs_raster_bwd_tone_log_acc, raster_bwd_log_kernel) at the places where
its batch pipeline can break and that the four scenes of tests/test_gpu_raster_budget.py do not pin: the boundaries of the two-ahead
prefetch (logs of 63 .. 193 entries), a batch without a live pixel in front of a live one (the `continue` in front of the first
commit), batches committed in six and more sub-batches, commit instructions that are not full (7 records per atomic instruction), and
one packed gradient record that sixteen waves add into.  Element by element against oracle.raster_bwd_budget with the rule of the budget
file: |got - want| <= util.BUDGET_KAPPA * 2^-24 * budget.

Every scene is one 16 x 16 tile (or 32 x 32 pixels) and at most a few hundred Gaussians.  What a case is FOR is asserted on the oracle's
forward, on the CPU (`_log_model`: which records the forward logs for a quadrant; in the tests on the oracle's compositor fed with the
GPU's projected inputs, which the GPU's forward must equal bit for bit; `premises()` checks the same on the oracle's own projection and
needs no GPU), and the model itself is confirmed against the entry counts the GPU forward wrote.  The cull-log entry points take three colour channels and nothing else (D = 3 is fixed in their
signatures), so "every colour count" is that one; the three tone modes run on the shared-record scene.

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X over the ten cases: 1.44 (kappa = util.BUDGET_KAPPA = 16); -s prints all.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from tests import util
from tests.test_gpu_raster_budget import TILE, _R, _check, _project

pytestmark = pytest.mark.gpu

A_MIN = np.float32(1.0 / 255.0)
BOUNDARY_N = [63, 64, 65, 127, 128, 129, 193]


# ----------------------------------------------------------------------------- scenes (screen space, see util._screen_scene)
def _boundary_scene(n):
    """n small low-opacity splats well inside quadrant 0 of one tile: every one is logged there and nowhere else, no pixel terminates"""
    r = np.random.RandomState(100 + n)
    return util._screen_scene(f"boundary{n}", 16, 16, r.uniform(2.5, 5.0, n), r.uniform(2.5, 5.0, n), r.uniform(0.7, 0.9, n),
                              np.linspace(2.0, 6.0, n)[r.permutation(n)], r.uniform(0.03, 0.05, n), 100 + n)


def _dead_first_scene(n=150):
    """n > 128 nearly opaque splats over the whole tile: every pixel terminates within the first few records, after the forward has
    logged its first TWO dense batches (both are built before anything is composited)"""
    r = np.random.RandomState(7)
    return util._screen_scene("dead_first", 16, 16, r.uniform(7.0, 9.0, n), r.uniform(7.0, 9.0, n), r.uniform(9.0, 11.0, n),
                              np.linspace(2.0, 6.0, n)[r.permutation(n)], np.full(n, 0.97), 7)


def _many_commits_scene(n=64):
    """64 splats that each reach all 256 pixels of the tile without terminating any: 4 096 pairs per quadrant batch"""
    r = np.random.RandomState(8)
    return util._screen_scene("many_commits", 16, 16, r.uniform(7.0, 9.0, n), r.uniform(7.0, 9.0, n), r.uniform(9.0, 11.0, n),
                              np.linspace(2.0, 6.0, n)[r.permutation(n)], r.uniform(0.02, 0.03, n), 8)


SHARED_FILL = [2, 4, 6, 9, 11, 13, 16, 18, 20, 23, 25, 27, 30, 32, 5, 12]          # fillers of the sixteen quadrants (253 in all)


def _shared_scene():
    """32 x 32: one large splat over all four quadrants of all four tiles (sixteen waves add into its record) among small fillers,
    SHARED_FILL[k] of them well inside the k-th quadrant: ragged batches and ragged last commit instructions"""
    r = np.random.RandomState(9)
    u, v = [16.0], [16.0]
    for k, n in enumerate(SHARED_FILL):
        u += list(8 * (k % 4) + r.uniform(2.5, 5.0, n)); v += list(8 * (k // 4) + r.uniform(2.5, 5.0, n))
    n_fill = sum(SHARED_FILL)
    sig = np.concatenate([[14.0], r.uniform(0.7, 0.9, n_fill)])
    z = np.concatenate([[4.0], np.linspace(2.0, 6.0, n_fill)[r.permutation(n_fill)]])
    op = np.concatenate([[0.3], r.uniform(0.03, 0.05, n_fill)])
    return util._screen_scene("shared", 32, 32, np.array(u), np.array(v), sig, z, op, 9)


# ----------------------------------------------------------------------------- the oracle's forward and the log it implies
@functools.lru_cache(maxsize=None)
def _oracle_forward(key):
    kind, arg = key
    sc = dict(boundary=_boundary_scene, dead_first=_dead_first_scene, many_commits=_many_commits_scene, shared=_shared_scene)[kind](*arg)
    m = oracle.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], util.scene_colors(sc, 3), sc["viewmat"], sc["K"],
                             sc["W"], sc["H"], background=None)
    return sc, m


def _quadrant_alpha(sc, m, tile, q):
    """(stream indices of the tile's list, alpha [64 pixels, records] of quadrant q, pixel-inside mask, last_ids of its pixels), fp32"""
    W, H = sc["W"], sc["H"]
    tw = (W + TILE - 1) // TILE
    off = np.asarray(m["isect_offsets"]).reshape(-1).astype(np.int64)
    ends = np.append(off[1:], len(m["flatten_ids"]))
    ty, tx = divmod(tile, tw)
    g = m["flatten_ids"][off[tile]:ends[tile]]
    idx = np.arange(off[tile], ends[tile])
    ys, xs = np.meshgrid(np.arange(8) + ty * TILE + (q >> 1) * 8, np.arange(8) + tx * TILE + (q & 1) * 8, indexing="ij")
    py = (ys.astype(np.float32) + np.float32(0.5)).reshape(-1, 1); px = (xs.astype(np.float32) + np.float32(0.5)).reshape(-1, 1)
    dx = m["means2d"][g, 0][None] - px; dy = m["means2d"][g, 1][None] - py
    ca, cb, cc = m["conics"][g, 0][None], m["conics"][g, 1][None], m["conics"][g, 2][None]
    sig = np.float32(0.5) * ca * dx * dx + np.float32(0.5) * cc * dy * dy + cb * dx * dy
    alpha = np.where(sig >= 0, m["opacities"][g][None] * np.exp(-sig), np.float32(0.0)).astype(np.float32)
    inside = ((ys < H) & (xs < W)).reshape(-1)
    last = m["last_ids"][np.minimum(ys, H - 1), np.minimum(xs, W - 1)].reshape(-1)
    return idx, alpha, inside, last


def _log_model(sc, m, tile, q, n_first=None):
    """Stream indices the forward logs for quadrant q while every pixel of it is still active: the records of the tile's list (the
    first n_first of them) that reach alpha >= 1/255 at some pixel of the quadrant.  The forward's mask is a superset with slack (0.4 %
    in alpha, 0.01 px), so a record whose best pixel lies within 10 % below the threshold would make the model ambiguous: refused."""
    idx, alpha, inside, _ = _quadrant_alpha(sc, m, tile, q)
    best = np.where(inside[:, None], alpha, 0).max(0) if alpha.shape[1] else np.zeros(0, np.float32)
    if n_first is not None:
        idx, best = idx[:n_first], best[:n_first]
    assert not ((best < A_MIN) & (best >= np.float32(0.9) * A_MIN)).any(), "a record within 10 % of the 1/255 threshold"
    return idx[best >= A_MIN]


def _no_termination(m):
    assert float(m["alphas"].max()) < 0.99                         # T_final > 1e-2 everywhere: far from the 1e-4 cut


# ----------------------------------------------------------------------------- GPU side
def _gpu_forward_log(cuda, sc):
    """exact-count GPU forward through the cull-log entry point (tone mode none); returns what the backward needs, the host copies
    for the oracle, and the per-quadrant entry counts of the log"""
    from geosplatting_amd import _lib as L
    R, lib = _R(), L.lib()
    W, H, D = sc["W"], sc["H"], 3
    state, V, I, D_, whs = R._bin_stage(_project(cuda, sc, D))
    st = R._prepare_stage(state, V, I, D_, whs)
    render = torch.empty(H, W, 3, device=cuda); alphas = torch.empty(H, W, device=cuda)
    last = torch.empty(H, W, dtype=torch.int32, device=cuda); img = torch.empty(H, W, 4, device=cuda)
    exposure = torch.tensor([1.3], device=cuda)
    rws = st["raster_ws"]
    log_ws = torch.zeros(lib.gs_raster_log_ws_bytes(L.i64(I), W, H, TILE), dtype=torch.uint8, device=cuda)
    L.check(lib.gs_raster_composite_tone_log(W, H, TILE, V, L.ptr(st["colors"]), L.i64(I), None, L.ptr(st["isect_offsets"]), L.ptr(render),
                                             L.ptr(alphas), L.ptr(last), 0, L.ptr(exposure), L.ptr(img), L.ptr(rws), C.c_size_t(rws.numel()),
                                             L.ptr(log_ws), C.c_size_t(log_ws.numel()), L.stream()), "gs_raster_composite_tone_log")
    torch.cuda.synchronize()
    host = dict(means2d=st["means2d"].cpu().numpy(), conics=st["conics"].cpu().numpy(), opacities=st["opacities"].cpu().numpy(),
                colors=st["colors"].cpu().numpy(), offsets=st["isect_offsets"].cpu().numpy().reshape(-1),
                flatten_ids=st["flatten_ids"].cpu().numpy(), alphas=alphas.cpu().numpy(), last_ids=last.cpu().numpy(),
                render=render.cpu().numpy(), bg=None)
    # the log's layout (csrc/gs_raster.hip carve_log): masks [4 I] u64, indices [4 I] i32, counts [4 tiles] i32, each 256-byte aligned
    a256 = lambda x: (x + 255) & ~255
    n = max(I, 1)
    tiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    at = a256(4 * n * 8) + a256(4 * n * 4)
    counts = log_ws[at:at + 16 * tiles].cpu().numpy().view(np.int32).reshape(tiles, 4)
    return dict(st=st, V=V, I=I, render=render, alphas=alphas, last=last, exposure=exposure, rws=rws, log_ws=log_ws), host, counts


def _oracle_on_gpu_inputs(sc, host):
    """the oracle's compositor forward on the GPU's own projected inputs (what the budget is computed from), in the shape of
    oracle.rasterization()'s result; the GPU's forward must be that forward bit for bit (as in tests/test_gpu_raster_budget.py)"""
    r, a, last, _, _ = oracle.raster_fwd(sc["W"], sc["H"], TILE, host["means2d"], host["conics"], host["opacities"], host["colors"],
                                         host["offsets"], host["flatten_ids"], None)
    assert np.array_equal(last, host["last_ids"]) and np.array_equal(a, host["alphas"])
    assert np.array_equal(r.view(np.int32), host["render"].view(np.int32))
    return dict(means2d=host["means2d"], conics=host["conics"], opacities=host["opacities"], isect_offsets=host["offsets"],
                flatten_ids=host["flatten_ids"], last_ids=last, alphas=a)


def _backward_check(cuda, label, sc, g, host, kinds=("dense", "sparse"), modes=(("none", 0),)):
    from geosplatting_amd import _lib as L
    lib = L.lib()
    W, H, D, V, I, st = sc["W"], sc["H"], 3, g["V"], g["I"], g["st"]
    rgba = np.concatenate([host["render"], host["alphas"][..., None]], -1)
    worst = 0.0
    for tone, mode in modes:
        for kind in kinds:
            vr, va = util.budget_cotangents(kind, H, W, D, seed=70 + mode)
            v_img = np.concatenate([vr, va[..., None]], -1)
            tv = torch.tensor(v_img, device=cuda)
            vp = torch.zeros(V, lib.gs_raster_grad_stride(D), device=cuda)
            v_exp = torch.zeros(1, device=cuda)
            L.check(lib.gs_raster_bwd_tone_log_acc(W, H, TILE, V, L.ptr(st["colors"]), L.i64(I), None, L.ptr(st["isect_offsets"]),
                                                   L.ptr(g["render"]), L.ptr(g["alphas"]), L.ptr(g["last"]), mode, L.ptr(g["exposure"]),
                                                   L.ptr(tv), L.ptr(vp), L.ptr(v_exp), L.ptr(g["rws"]), C.c_size_t(g["rws"].numel()),
                                                   L.ptr(g["log_ws"]), C.c_size_t(g["log_ws"].numel()), L.stream()), "gs_raster_bwd_tone_log_acc")
            torch.cuda.synchronize()
            v_rgba, _ = oracle.tonemap_bwd(rgba, 1.3, v_img, tone)
            worst = max(worst, _check(f"{label} {tone}/{kind}", sc, host, vp, v_rgba[..., :3], v_rgba[..., 3], D, V))
    return worst


# ----------------------------------------------------------------------------- premises alone (what a GPU-less run can check)
def premises():
    """every scene's premise on the oracle's forward; returns a summary per scene (the GPU tests assert the same things)"""
    out = {}
    for n in BOUNDARY_N:
        sc, m = _oracle_forward(("boundary", (n,)))
        _no_termination(m)
        cnt = [len(_log_model(sc, m, 0, q)) for q in range(4)]
        assert cnt == [n, 0, 0, 0], (n, cnt)
        out[f"boundary{n}"] = cnt
    sc, m = _oracle_forward(("dead_first", ()))
    out["dead_first"] = _dead_first_premise(sc, m)
    sc, m = _oracle_forward(("many_commits", ()))
    out["many_commits"] = _many_commits_premise(sc, m)
    sc, m = _oracle_forward(("shared", ()))
    out["shared"] = _shared_premise(sc, m)
    return out


def _dead_first_premise(sc, m):
    """per quadrant: the list is longer than 128, its first 128 records all reach every pixel (the forward builds and logs two dense
    batches of 64 before it composites anything, and logs nothing after every pixel has terminated), and every pixel's last_ids lies in
    front of the 64 entries the backward takes first"""
    off = np.asarray(m["isect_offsets"]).reshape(-1)
    assert len(m["flatten_ids"]) - off[0] > 128
    res = []
    for q in range(4):
        idx, alpha, inside, last = _quadrant_alpha(sc, m, 0, q)
        assert inside.all() and (alpha[:, :128].min() >= np.float32(1.1) * A_MIN)
        log = _log_model(sc, m, 0, q, n_first=128)
        assert len(log) == 128
        assert last.max() < log[-64:].min(), (q, last.max(), log[-64:].min())
        assert last.min() >= log[0]
        res.append((int(last.max()), int(log[-64:].min())))
    return res


def _many_commits_premise(sc, m):
    """per quadrant: 64 logged records, all 64 x 64 pairs live (alpha >= 1/255 with margin, nothing terminated): 4 096 pairs against a
    pair buffer of 790, six sub-batches at least"""
    _no_termination(m)
    res = []
    for q in range(4):
        idx, alpha, inside, last = _quadrant_alpha(sc, m, 0, q)
        assert alpha.shape == (64, 64) and alpha.min() >= np.float32(1.1) * A_MIN and last.min() == idx[-1]
        assert len(_log_model(sc, m, 0, q)) == 64
        res.append(math.ceil(alpha.size / 790))
    assert min(res) >= 6
    return res


def _shared_premise(sc, m):
    """the large splat is logged in all sixteen quadrants; the entry counts are ragged: not all equal, and some leave a
    last commit instruction of fewer than 7 records"""
    _no_termination(m)
    big = int(np.argmin(m["conics"][:, 0]))                         # the large splat's row among the visible Gaussians
    assert m["conics"][big, 0] < 0.1 * np.partition(m["conics"][:, 0], 1)[1]
    counts = np.zeros((4, 4), np.int64)
    for tile in range(4):
        for q in range(4):
            log = _log_model(sc, m, tile, q)
            assert big in m["flatten_ids"][log], (tile, q)
            counts[tile, q] = len(log)
    # quadrant q of tile t is the k-th quadrant of the image in SHARED_FILL's order (rows of 4 quadrants); its log: the fillers + 1
    want = np.array([[SHARED_FILL[4 * (2 * (t >> 1) + (q >> 1)) + 2 * (t & 1) + (q & 1)] + 1 for q in range(4)] for t in range(4)])
    assert np.array_equal(counts, want), (counts, want)
    assert (counts % 7 != 0).sum() >= 12                            # last commit instructions of 1 .. 6 records
    return counts.tolist()


# ----------------------------------------------------------------------------- tests
@pytest.mark.parametrize("n", BOUNDARY_N)
def test_log_bwd_batch_boundaries(cuda, n):
    """a quadrant log of exactly n entries around the 64-entry batches of the two-ahead prefetch; the other three quadrants' logs are
    empty (their waves leave before the loop)"""
    sc = _boundary_scene(n)
    g, host, counts = _gpu_forward_log(cuda, sc)
    m = _oracle_on_gpu_inputs(sc, host)
    _no_termination(m)
    model = [len(_log_model(sc, m, 0, q)) for q in range(4)]
    assert model == [n, 0, 0, 0], model
    assert counts[0].tolist() == model, (counts, model)
    _backward_check(cuda, f"boundary n={n}", sc, g, host)


def test_log_bwd_dead_batch_first(cuda):
    """the first batch the backward takes (log entries 64..127) has no live pixel: `continue`, then the live batch behind it"""
    sc = _dead_first_scene()
    g, host, counts = _gpu_forward_log(cuda, sc)
    _dead_first_premise(sc, _oracle_on_gpu_inputs(sc, host))
    assert counts[0].tolist() == [128] * 4, counts
    _backward_check(cuda, "dead batch first", sc, g, host)


def test_log_bwd_many_commits_per_batch(cuda):
    """4 096 pairs in one batch: six or more sub-batches, each with its own commit (12 records: one full instruction and one of 5)"""
    sc = _many_commits_scene()
    g, host, counts = _gpu_forward_log(cuda, sc)
    _many_commits_premise(sc, _oracle_on_gpu_inputs(sc, host))
    assert counts[0].tolist() == [64] * 4, counts
    _backward_check(cuda, "many commits", sc, g, host)


def test_log_bwd_shared_record_and_commit_tails(cuda):
    """sixteen waves add into one packed record among fillers, ragged batch sizes, under every tone mode"""
    sc = _shared_scene()
    g, host, counts = _gpu_forward_log(cuda, sc)
    model = _shared_premise(sc, _oracle_on_gpu_inputs(sc, host))
    assert counts.tolist() == model, (counts, model)
    _backward_check(cuda, "shared record", sc, g, host, kinds=("dense", "alpha", "sparse"), modes=(("none", 0), ("naive", 1), ("aces", 2)))
