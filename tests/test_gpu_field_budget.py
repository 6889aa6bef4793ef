"""GPU: the hash-grid encoder and the MLP weight gradient (csrc/gs_hashgrid.hip) against oracle/field_ref.py, ELEMENT BY ELEMENT,
within the oracle's error budget (validated against float64 autograd in tests/test_oracle_cpu.py): |got - want| <= kappa * 2^-24 *
budget for every feature, every element of v_x, every element of every table row and every element of dW.  The entry points are
called through the C ABI, so the options the Python wrappers never pass are reached: the atomic kernel (ws = NULL), accumulate = 1,
v_x = NULL, scale != 1, the parts == 1 and parts > 1 stores of the float slab kernel, the fixed-point path at its 4- and 64-slab
limits and its refusal outside them.  Scenes (tests/util.py FIELD_BUDGET_SCENES) interleave uniform points with mesh-order runs
inside one cell, lattice points, x = +-1, points outside [-1, 1], a pile of 500 copies and dead points; cotangents are dense, live on
one level per point, spread over six decades, or zero on the first and last level.

Budgets.  v_x: a running-error bound per level, the levels' bounds plus (L - 1) * sum |level term|.  A table element that collects n
non-zero contributions in an order nobody controls (atomic and float-slab paths): 7 * sum |c| + (n - 1) * sum |c|.  Fixed point
(order-free): 7 * sum |c| + n * 2^-e / 2^-24 + |sum|, e restated from hg_fx_exponent.  An element with n = 0 must be exactly 0, or
keep the pre-filled pattern's bits under accumulate = 1.  On top of a pattern p the test charges n |p| + sum |c| more (float paths:
each addition may round a sum that holds p) or |p| + |sum| (fixed point: one float addition).  dW: depth * sum_n |dY X| |scale| with
depth = points per wave + 3 + ceil(nb / 32) + 32.

Worst ratio |got - want| / (2^-24 budget) seen on an MI355X (kappa = util.FIELD_BUDGET_KAPPA = 4, the smallest power of two that is at
least 4 x the worst figure below):
                                           features    v_x   v_table acc 0   v_table acc 1 (pattern)   N edges v_table / v_x
    gs_hashgrid_fwd                            0.43
    gs_hashgrid_bwd, ws = NULL (atomic)                0.23       0.49              1.00                    0.97 / 0.07
    gs_hashgrid_bwd, float slabs                       0.23       0.49              1.00                    0.97 / 0.07
    gs_hashgrid_bwd_fixed                              0.18       0.84              1.00                    0.97 / 0.07
    gs_mlp_wgrad                               dW: 0.05 (accumulate 0), 0.98 (accumulate 1 over the pattern)
The 1.00 (0.999) and the 0.97 / 0.98 are the pattern cases, and they alone set kappa: an element with a single contribution c on top of
a pattern value p is charged |p| + |c| for one addition whose rounding is at most 2^-24 |p + c| -- the bound is attained when p and c
have the same sign, and cannot be exceeded by correct code.  Over zeros the float paths stay below half a budget; the fixed-point
path's 0.84 (L4_T19 / decades; 0.75 .. 0.80 on the other shapes) is a single addend meeting its own rounding bound.  No regime
stands out.
The CPU side (tests/test_oracle_cpu.py, float32 restatement against float64 autograd on the dyadic scenes, bar kappa / 2): features
0.41, v_x 0.26, v_table float 0.67, v_table fixed 0.98, dW 0.08.

Bits.  The forward, v_x on all three paths (one arithmetic, contraction off) and the fixed-point table gradient (integer sums) were seen
to equal the oracle's float32 / integer restatements bit for bit in every case on the MI355X; the tests assert it.  No kernel bug
showed: hg_hash agrees with Python's modulo on negative cells, the partition of the points among `parts` holds at every N edge, and
the leader fold of the atomic kernel is within budget on the mesh-order runs and the pile.

Whether the tests bite.  Each one-line change below was built into a scratch library (never committed, every address in bounds) and
this module and tests/test_gpu_field.py ("old") were run against it on an MI355X; the first failing element of the first failing
new test is quoted (the unchanged library passes all 112 + 14):
 (a) hashgrid_bwd_x_kernel: do_[1] formed with wy in place of wx -- FAILS 42 cases of test_hashgrid_bwd_within_budget (every slab
     and fixed case; first slab-L16_T10-dense, v_x[1872, 1] got -8235 want 0, ratio 742 902) and 2 of test_hashgrid_bwd_n_boundaries.
     Old: 4 fail (both goldens, the full call, vs float64).
 (b) the same in hashgrid_bwd_kernel only -- FAILS the 30 atomic cases + test_hashgrid_bwd_n_boundaries[atomic] (first
     atomic-L16_T10-dense, the same element and ratio; the cross-path v_x bit comparison fails with it).  Old: all 14 pass -- nothing
     there runs the atomic kernel.
 (c) the leader's fold summing cv[0] for both features -- FAILS the 30 atomic cases + n_boundaries[atomic] (first atomic-L16_T10-dense
     acc0, v_table[1, 1] got 1.419 want -1.215, ratio 404 414).  Old: all pass.
 (d) hashgrid_transpose_kernel swapping the two features of level 1 -- FAILS 39 slab / fixed cases (all but L = 1 and
     L2_T14-level_off, whose cotangent is all zero) and 2 n_boundaries (first slab-L16_T10-dense acc0,
     v_table[1994, 1] got 0.625 want -0.557, ratio 2 337 737).  Old: 5 fail.
 (e) n_hi - 1 as the upper bound of a part of the float slab kernel -- FAILS the 30 slab cases + n_boundaries[slab] (first
     slab-L16_T10-dense acc0, v_table[4654, 0] got 0.114 want 0.655, ratio 395 761).  Old: 2 fail (golden a, the full call: the only
     old tests whose table the fixed-point path refuses).
 (f) hashgrid_bin_kernel building its slab mask from the ceil corner only -- in BOTH phases: changed in phase 2 alone, the queues keep
     entries that nobody wrote and the slab kernel would read point indices from uninitialised memory, which is not run.  FAILS the
     12 fixed cases + n_boundaries[fixed] (first fixed-L16_T15-dense acc0, v_table[21635, 0] got 0 want -9.164, ratio 2 097 152).
     Old: 3 fail (golden b, vs float64, the fixed-point test).
 (g) accumulate ignored in the parts == 1 store -- FAILS the 8 slab cases of L16_T18 and L3_T20 (the only shapes with parts == 1):
     rows no corner reaches lose the pattern's bits.  Old: all pass (accumulate is always 0 there).
 (h) `down` built with exponent e - 1 -- FAILS the 12 fixed cases + n_boundaries[fixed] (first fixed-L16_T15-dense acc0,
     v_table[75663, 1] got -8.689 want -4.345, ratio 2 097 153).  Old: 3 fail.
 (i) the n < N mask dropped from b[u] in mlp_wgrad_kernel -- passes everything, old and new.  The change cannot be observed: a[u]
     keeps its mask, so the product a[u] * b[u] of a point past N is 0 * X[0][c] = 0 for every finite X; the second mask only matters
     for a non-finite X[0], which no test feeds.
 (j) scale not applied under accumulate -- FAILS all 5 test_mlp_wgrad_within_budget cases (first 1-1, N = 2, scale -0.25: dW[0, 0]
     got 1.86811876 want 1.86811952, ratio 6.8 -- small because the pattern dominates that element; 32-32 fails by orders).  Old: all
     pass (scale is always 1 there).

Run with -s to print the ratio of every check.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import field_ref
from tests import util

pytestmark = pytest.mark.gpu

PATHS = ("atomic", "slab", "fixed")
SHAPES = list(util.FIELD_BUDGET_SCENES)
KAPPA = util.FIELD_BUDGET_KAPPA
WORST = {}
_VX_BITS = {}                                   # (shape, kind) -> (path, v_x bytes): the three paths share the arithmetic of v_x


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module's tests: the worst ratio per entry point and gradient over whatever ran (shown with -s)"""
    yield
    print()
    for key in sorted(WORST):
        print(f"    {key[0]:28s} {key[1]:10s} {WORST[key]:7.3f}")


def _record(entry, nm, r):
    WORST[(entry, nm)] = max(WORST.get((entry, nm), 0.0), r)


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = util.field_budget_scene(name)
    util.field_scene_check(sc)
    return sc, util.field_scene_table(sc)


@functools.lru_cache(maxsize=None)
def _pattern(name):
    L, log2_T = util.FIELD_BUDGET_SCENES[name]
    return np.random.RandomState(9).uniform(-2, 2, (L << log2_T, 2)).astype(np.float32)


def _tgs(name, kind):
    return util.FIELD_TGS[(SHAPES.index(name) + util.FIELD_COTANGENTS.index(kind)) % 3]


@functools.lru_cache(maxsize=8)
def _want(name, kind, mode):
    sc, table = _scene(name)
    cot = util.field_budget_cotangents(kind, sc, seed=3)
    return cot, field_ref.encode_bwd_budget(sc["x"], table, sc["scalings"], sc["log2_T"], cot, _tgs(name, kind), mode)


def _fixed_bytes(sc, N):
    from geosplatting_amd import _lib as L
    return int(L.lib().gs_hashgrid_bwd_fixed_ws_bytes(N, sc["L"], 2, sc["log2_T"]))


def _bwd(cuda, path, sc, x, table, cot, tgs, v_table, accumulate, v_x, ws_bytes=None):
    """one launch of the path's entry point through the C ABI; returns the return code"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    N, nl, log2_T = x.shape[0], sc["L"], sc["log2_T"]
    s = (C.c_float * nl)(*[float(v) for v in sc["scalings"]])
    if path == "fixed":
        nbytes = _fixed_bytes(sc, N) if ws_bytes is None else ws_bytes
        fn = lib.gs_hashgrid_bwd_fixed
    else:
        nbytes = int(lib.gs_hashgrid_bwd_ws_bytes(N, nl, 2)) if path == "slab" else 0
        fn = lib.gs_hashgrid_bwd
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda) if nbytes else None
    rc = fn(N, nl, 2, log2_T, s, L.ptr(x), L.ptr(table), L.ptr(cot), L.f32(tgs), L.ptr(v_table), accumulate, L.ptr(v_x), L.ptr(ws),
            C.c_size_t(nbytes), L.stream())
    torch.cuda.synchronize()
    return rc


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32).tobytes()


def _check_table(label, entry, got, b, mode, pattern=None):
    """the whole table gradient: rows no corner reaches are exactly 0 (the pattern's bits), elements without a non-zero contribution
    too (budget 0), every other element within its budget (+ the pattern charge)"""
    g = got.cpu().numpy()
    rows = b["rows"]
    away = np.ones(g.shape[0], bool); away[rows] = False
    want, bud, gt = b["v_table"], b["v_table_budget"], g[rows]
    if pattern is None:
        assert not g[away].any(), label
    else:
        p = pattern[rows]
        assert _bits(g[away]) == _bits(pattern[away]), label
        assert _bits(gt[b["n"] == 0]) == _bits(p[b["n"] == 0]), label
        charge = b["n"] * np.abs(p) + b["abs_sum"] if mode == "float" else np.abs(p) + np.abs(want)
        bud = np.where(b["n"] > 0, bud + charge, 0.0)
        want = want + p
    _record(entry, "v_table", util.assert_within_budget(f"{label} v_table", gt, want, bud, KAPPA))
    return g


def _check_vx(label, entry, v_x, b, dead):
    g = v_x.cpu().numpy()
    assert not g[dead].any() and not b["v_x_budget"][dead].any(), label
    _record(entry, "v_x", util.assert_within_budget(f"{label} v_x", g, b["v_x"], b["v_x_budget"], KAPPA))
    return g


@pytest.mark.parametrize("shape", SHAPES)
def test_hashgrid_fwd_within_budget(cuda, shape):
    """gs_hashgrid_fwd: every feature within budget of the float64 value -- and equal to the float32 restatement bit for bit (the
    kernel's contraction is off; the restatement nests like it: x pairs, then y, then z)"""
    from geosplatting_amd import _lib as L
    sc, table = _scene(shape)
    N, nl = sc["x"].shape[0], sc["L"]
    f32, f64, bud = field_ref.encode_fwd(sc["x"], table, sc["scalings"], sc["log2_T"])
    out = torch.full((N, 2 * nl), 123.0, device=cuda)
    s = (C.c_float * nl)(*[float(v) for v in sc["scalings"]])
    x, t = torch.tensor(sc["x"], device=cuda), torch.tensor(table, device=cuda)
    L.check(L.lib().gs_hashgrid_fwd(N, nl, 2, sc["log2_T"], s, L.ptr(x), L.ptr(t), L.ptr(out), L.stream()), "gs_hashgrid_fwd")
    got = out.cpu().numpy()
    _record("gs_hashgrid_fwd", "features", util.assert_within_budget(f"fwd {shape}", got, f64, bud, KAPPA))
    same = _bits(got) == _bits(f32)
    print(f"  forward {shape}: bits equal the float32 restatement: {same}")
    assert same


@pytest.mark.parametrize("kind", util.FIELD_COTANGENTS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("path", PATHS)
def test_hashgrid_bwd_within_budget(cuda, path, shape, kind):
    """accumulate = 0 over a 123-filled v_table and v_x (every element written, budget-0 elements exactly 0, dead points exactly 0);
    accumulate = 1 with v_x = NULL over a uniform(-2, 2) pattern (untouched elements keep its bits, the others are pattern + gradient
    within budget + charge); fixed: a second accumulate = 0 run with v_x = NULL gives the same bits, the result equals the oracle's
    integer restatement bit for bit, and where the library hands out no workspace the call refuses and leaves v_table alone; the
    v_x of the three paths is bit-identical"""
    from geosplatting_amd import _lib as L
    sc, table_h = _scene(shape)
    N = sc["x"].shape[0]
    mode = "fixed" if path == "fixed" else "float"
    tgs = _tgs(shape, kind)
    x, table = torch.tensor(sc["x"], device=cuda), torch.tensor(table_h, device=cuda)
    entry = f"hashgrid_bwd {path}"
    label = f"{path} {shape}/{kind}"
    if path == "fixed" and _fixed_bytes(sc, N) == 0:
        assert not (15 <= sc["log2_T"] <= 19)
        cot = torch.tensor(util.field_budget_cotangents(kind, sc, seed=3), device=cuda)
        v_table = torch.full_like(table, 123.0)
        with pytest.raises(L.GeoSplatHipError, match="outside the fixed-point path"):
            L.check(_bwd(cuda, path, sc, x, table, cot, tgs, v_table, 0, None, ws_bytes=1 << 20), "gs_hashgrid_bwd_fixed")
        assert bool((v_table == 123.0).all())
        return
    assert path != "fixed" or 15 <= sc["log2_T"] <= 19
    cot_h, b = _want(shape, kind, mode)
    cot = torch.tensor(cot_h, device=cuda)
    dead = sc["regime"] == "dead"
    # accumulate = 0 over garbage
    v_table, v_x = torch.full_like(table, 123.0), torch.full_like(x, 123.0)
    L.check(_bwd(cuda, path, sc, x, table, cot, tgs, v_table, 0, v_x), entry)
    g0 = _check_table(f"{label} acc0", entry + " acc0", v_table, b, mode)
    gx = _check_vx(label, entry, v_x, b, dead)
    first = _VX_BITS.setdefault((shape, kind), (path, _bits(gx)))
    assert first[1] == _bits(gx), f"v_x of {path} and {first[0]} differ"
    assert _bits(gx) == _bits(b["v_x_f32"]), f"{label}: v_x differs from the float32 restatement"      # contraction off: the same bits
    if kind == "level_off":
        lv = np.arange(g0.shape[0]) >> sc["log2_T"]
        assert not g0[(lv == 0) | (lv == sc["L"] - 1)].any()
    # accumulate = 1 over a pattern, no position gradient
    pat = _pattern(shape)
    v_table = torch.tensor(pat, device=cuda)
    L.check(_bwd(cuda, path, sc, x, table, cot, tgs, v_table, 1, None), entry)
    g1 = _check_table(f"{label} acc1", entry + " acc1", v_table, b, mode, pattern=pat)
    if kind == "level_off":
        off = (lv == 0) | (lv == sc["L"] - 1)
        assert _bits(g1[off]) == _bits(pat[off])
    if path == "fixed":
        v_table = torch.full_like(table, 123.0)
        L.check(_bwd(cuda, path, sc, x, table, cot, tgs, v_table, 0, None), entry)
        assert _bits(v_table.cpu().numpy()) == _bits(g0), "fixed point: two runs differ (or v_x = NULL changes v_table)"
        same = _bits(g0[b["rows"]]) == _bits(b["v_table_f32"])
        print(f"  {label}: table bits equal the integer restatement: {same}")
        assert same


@pytest.mark.parametrize("path", PATHS)
def test_hashgrid_bwd_n_boundaries(cuda, path):
    """N around the loops' strides -- 0, 1, the wave, the bin block (1024), PU * blockDim of the slab loops (4096), and an N that
    `parts` does not divide -- on the (16, 2^15) shape with dense cotangents: every element of v_table and v_x"""
    from geosplatting_amd import _lib as L
    full, table_h = _scene("L16_T15")
    table = torch.tensor(table_h, device=cuda)
    mode = "fixed" if path == "fixed" else "float"
    pat = _pattern("L16_T15")
    for N in util.FIELD_N_BOUNDARIES:
        sc = util.field_budget_scene("L16_T15", n=N)
        assert sc["x"].shape[0] == N and np.array_equal(sc["x"], full["x"][:N])
        cot_h = util.field_budget_cotangents("dense", sc, seed=3)
        b = field_ref.encode_bwd_budget(sc["x"], table_h, sc["scalings"], sc["log2_T"], cot_h, 16.0, mode)
        x, cot = torch.tensor(sc["x"], device=cuda).reshape(N, 3), torch.tensor(cot_h, device=cuda).reshape(N, 32)
        v_table, v_x = torch.full_like(table, 123.0), torch.full((N, 3), 123.0, device=cuda)
        L.check(_bwd(cuda, path, sc, x, table, cot, 16.0, v_table, 0, v_x), f"{path} N={N}")
        _check_table(f"{path} N={N}", f"hashgrid_bwd {path} N-edges", v_table, b, mode)
        _check_vx(f"{path} N={N}", f"hashgrid_bwd {path} N-edges", v_x, b, sc["regime"] == "dead")
        if N in (0, 1, 65):
            v_table = torch.tensor(pat, device=cuda)
            L.check(_bwd(cuda, path, sc, x, table, cot, 16.0, v_table, 1, None), f"{path} N={N}")
            _check_table(f"{path} N={N} acc1", f"hashgrid_bwd {path} N-edges", v_table, b, mode, pattern=pat)


@pytest.mark.parametrize("O,I", [(1, 1), (32, 32), (3, 32), (32, 7), (17, 5)])
def test_mlp_wgrad_within_budget(cuda, O, I):
    """gs_mlp_wgrad through the C ABI: N from 1 to past the 1024-workgroup cap, columns of dY and X over six decades, scale 1 and
    -0.25, accumulate = 0 over a 123-filled dW and accumulate = 1 over a pattern (charged |p| + |dW|: one addition) -- every element
    against field_ref.wgrad_budget, and two runs bit-identical"""
    from geosplatting_amd import _lib as L
    lib = L.lib()
    pat = np.random.RandomState(4).uniform(-2, 2, (O, I)).astype(np.float32)
    for N in (1, 2, 15, 16, 17, 511, 512, 513, 4097, 524305):
        r = np.random.RandomState(N + O)
        dY_h = (r.standard_normal((N, O)) * np.logspace(-6, 0, O)).astype(np.float32)
        X_h = (r.standard_normal((N, I)) * np.logspace(0, -6, I)).astype(np.float32)
        nbytes = int(lib.gs_mlp_wgrad_ws_bytes(L.i64(N)))
        nb = nbytes // 4096
        assert nb == field_ref.wgrad_plan_blocks(N) and nb * 4096 == nbytes
        assert (N > 512 * 1024) == (N == 524305) and (nb == 1024) == (N == 524305)
        dY, X = torch.tensor(dY_h, device=cuda), torch.tensor(X_h, device=cuda)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        for scale in (1.0, -0.25):
            want, bud = field_ref.wgrad_budget(dY_h, X_h, scale, nb)
            for accumulate in (0, 1):
                runs = []
                for _ in range(2):
                    ws.fill_(255)                                    # NaN patterns: every partial the reduce reads was written
                    dW = torch.tensor(pat, device=cuda) if accumulate else torch.full((O, I), 123.0, device=cuda)
                    L.check(lib.gs_mlp_wgrad(L.i64(N), O, I, L.ptr(dY), L.ptr(X), L.f32(scale), L.ptr(dW), accumulate, L.ptr(ws),
                                             C.c_size_t(nbytes), L.stream()), "gs_mlp_wgrad")
                    torch.cuda.synchronize()
                    runs.append(dW.cpu().numpy())
                assert _bits(runs[0]) == _bits(runs[1])
                w, bb = (want + pat, bud + np.abs(pat) + np.abs(want)) if accumulate else (want, bud)
                _record(f"gs_mlp_wgrad acc{accumulate}", "dW",
                        util.assert_within_budget(f"wgrad {O}x{I} N={N} scale={scale} acc={accumulate}", runs[0], w, bb, KAPPA))
