"""No-GPU checks of the Monte-Carlo environment shader: the float64 restatement (tests/envshade_ref.py) against hand-worked PCG
values, a direct loop for the pdf tables and a quadrature of the rendering integral; the fragile cap as a condition on every scene the
GPU tests use; argument validation of the C-ABI before the device is touched; the refusals of the Python ops; the kernels' scratch.

Fragile shares of the restatement alone on the committed scenes (points with a sample whose discrete decisions an fp32 rounding may
flip, gradients' decisions included; the cap is 1 %, and one point of 65 is already 1.5 %): 0 of 214, 65 and 1 points in every case of
envshade_ref.CASES at the committed seed."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import envshade_ref as ref

FRAGILE_CAP = 0.01


def test_pcg_known_answers():
    """Worked by hand from the recurrence: out(s) = ((s >> ((s >> 28) + 4)) ^ s) * 277803737, then ^ its own >> 22 (mod 2^32).
    s = 0: shift 4, 0 ^ 0 = 0, product 0 -> 0.
    s = 1: shift 4, (1 >> 4) ^ 1 = 1, product 277803737 = 0x108EF2D9; >> 22 = 0x42 = 66; 277803737 ^ 66 = 277803675.
    s = 2^31: shift 8 + 4 = 12, (2^31 >> 12) ^ 2^31 = 0x80080000; times 277803737 mod 2^32: 0x80000000 * odd = 0x80000000,
      0x00080000 * 0x108EF2D9 = (0x108EF2D9 << 19) mod 2^32 = 0x96C80000; sum 0x16C80000; >> 22 = 0x5B; 0x16C80000 ^ 0x5B = 0x16C8005B.
    LCG: 0 -> 2891336453; 1 -> 747796405 + 2891336453 = 3639132858."""
    assert ref.pcg_out(np.array([0, 1, 1 << 31], np.uint32)).tolist() == [0, 277803675, 0x16C8005B]
    assert ref.pcg_step(np.array([0, 1], np.uint32)).tolist() == [2891336453, 3639132858]
    # the stream of a point: state = out(seed) ^ out(p), two table picks, then the uniforms, sequentially
    lt, bt, u = ref.stream(1, 2, 7, 2)
    s = int(ref.pcg_out(np.uint32(1))) ^ int(ref.pcg_out(np.uint32(1)))              # point 1 with seed 1: state 0
    assert s == 0 and lt[1] == 0 % 7                                                   # out(0) = 0
    s1 = 2891336453
    assert bt[1] == int(ref.pcg_out(np.uint32(s1))) % 7
    s2 = (s1 * 747796405 + 2891336453) % (1 << 32)
    assert u[1, 0, 0] == np.float32((int(ref.pcg_out(np.uint32(s2))) & 0xFFFFFF) / 2.0 ** 24)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and u.shape == (2, 2, 5)
    # jumping 5 k draws ahead in closed form lands on the same state as stepping (what a lane of the kernel does)
    st = np.uint32(12345)
    for _ in range(35):
        st = ref.pcg_step(st)
    mul, inc, cm, ci, k = 1, 0, 747796405, 2891336453, 35
    while k:
        if k & 1:
            mul, inc = (mul * cm) % (1 << 32), (inc * cm + ci) % (1 << 32)
        ci, cm, k = ((cm + 1) * ci) % (1 << 32), (cm * cm) % (1 << 32), k >> 1
    assert int(st) == (12345 * mul + inc) % (1 << 32)


def test_cdf_search_steps_and_picks():
    assert [ref.search_steps(s) for s in (2, 3, 5, 7, 16, 17, 32)] == [1, 2, 3, 4, 5, 5, 6]   # ceil(log2(size - 1)) + 1
    cdf = np.array([0.1, 0.1, 0.6, 1.0], np.float32)                                   # an empty cell is never chosen
    idx, off, width = ref.cdf_pick(cdf, np.array([0.0, 0.05, 0.1, 0.35, 0.6, 0.99, 1.0, 7.0], np.float32))
    assert idx.tolist() == [0, 0, 2, 2, 3, 3, 3, 3]
    assert off[3] == np.float32(0.35) - np.float32(0.1) and width[3] == np.float32(0.6) - np.float32(0.1) and off[1] == np.float32(0.05)
    for size in (5, 7, 16, 32):                                                        # the fixed step count always converges
        rng = np.random.default_rng(size)
        c = np.cumsum(rng.random(size)).astype(np.float32); c /= c[-1]
        x = rng.random(500).astype(np.float32)
        idx, _, _ = ref.cdf_pick(c, x)
        assert np.array_equal(idx, np.searchsorted(c, np.minimum(x, ref.ONE_BELOW), side="right"))


@pytest.mark.parametrize("name", ref.MAPS)
def test_compute_pdf_against_a_direct_loop(name):
    import geosplatting_amd as gs
    light = ref.env_map(name)[0]
    H, W = light.shape[:2]
    env = gs.LatLngEnvMap(torch.from_numpy(light)).compute_pdf_()
    assert env.pdf.shape == (H, W, 3)
    pdf, rows, cols = (t.numpy() for t in env.tables())
    want = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            want[y, x] = max(float(light[y, x].max()), 1e-3) * math.sin((y + 0.5) / H * math.pi)
    want /= want.sum()
    wcols = np.cumsum(want, 1)
    wrows = np.cumsum(wcols[:, -1])
    assert np.allclose(pdf, want, rtol=1e-5, atol=0) and np.allclose(cols, wcols / wcols[:, -1:], rtol=1e-5) and np.allclose(rows, wrows / wrows[-1], rtol=1e-5)
    assert rows[-1] == 1.0 and (cols[:, -1] == 1.0).all() and np.isfinite(env.pdf.numpy()).all()
    assert (pdf[H - 2] > 0).all() and (light[H - 2] == 0).all()                        # the zero row keeps the clamp's share
    assert np.array_equal(env.pdf[..., 1].numpy(), np.repeat(rows[:, None], W, 1))     # rows is kept repeated along the row
    for a, b in zip((pdf, rows, cols), ref.env_map(name)[1:]):                         # the restatement's own tables (numpy fp32)
        assert np.allclose(a, b, rtol=2e-6, atol=1e-9)
    with pytest.raises(ValueError, match=r"\(1, 4, 3\)"):
        gs.LatLngEnvMap(torch.zeros(1, 4, 3))


def test_restatement_is_unbiased():
    """Constant radiance L, no occluder, n_samples_x = 16: the diffuse sum estimates L * integral of cos / pi = L, the specular sum
    L * integral of the specular BSDF over the hemisphere (a 256 x 256 midpoint quadrature in (cos theta, phi) here) -- within 5
    standard errors of the restatement's own per-iteration variance (stratification only lowers it).  Pins the two pdfs, the balance
    heuristic and the 1 / n^2 weight.  Roughness stays above 0.3: the quadrature has to resolve the lobe."""
    n, P, Lc = 16, 8, np.array([0.7, 1.3, 0.4])
    pt = {k: v.copy() for k, v in ref.points(P).items()}
    pt["ks"][:, 1] = np.linspace(0.3, 1.0, P).astype(np.float32)
    lookat_ok = (pt["nrm"] * (ref.CAMERA - pt["pos"])).sum(-1) > 0.1
    assert lookat_ok.sum() >= 4
    light = np.broadcast_to(Lc.astype(np.float32), (16, 32, 3)).copy()
    env = (light,) + ref.compute_pdf(light)
    smp = ref.sample(pt, env, n, 99, ref.perms(n))
    S = 2 * n * n
    out = ref.shade(pt, env, smp, smp["dirs"], np.ones((P, S)), "pbr", 1.0, n)
    # quadrature over the hemisphere of the (unnormalised) normal
    m = 256
    ct = (np.arange(m) + 0.5) / m
    ph = (np.arange(m) + 0.5) / m * 2.0 * np.pi
    ct, ph = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1.0 - ct * ct)
    ps = ref.point_setup(pt)
    for p in np.where(lookat_ok)[0]:
        wi = ps["fu"][p] * (st * np.cos(ph))[..., None] + ps["fv"][p] * (st * np.sin(ph))[..., None] + ps["fw"][p] * ct[..., None]
        ex = lambda k: ref._t(pt[k][p]).expand(m, m, 3)
        lam, spec, *_ = ref.bsdf_terms(ex("pos"), ex("nrm"), ex("kd"), ex("ks"), ref._t(wi), "pbr")
        dw = 2.0 * np.pi / (m * m)
        want_d, want_s = Lc * float(lam.sum()) * dw, Lc * spec.sum((0, 1)).numpy() * dw
        for got, want, terms in ((out["diff"][p], want_d, out["terms"][0][p]), (out["spec"][p], want_s, out["terms"][1][p])):
            pair = (terms[0::2] + terms[1::2]) * (n * n)                               # one estimate per iteration
            se = pair.std(0, ddof=1) / n
            assert (np.abs(got - want) <= 5.0 * se + 1e-3 * np.abs(want)).all(), (p, got, want, se)
        assert np.allclose(want_d, Lc * np.linalg.norm(pt["nrm"][p].astype(np.float64)), rtol=1e-3)


@pytest.mark.parametrize("P,map_name,n", ref.CASES)
def test_fragile_cap_of_every_case(P, map_name, n):
    """The condition under which the GPU comparison means something, from the restatement alone."""
    for bsdf in ref.BSDFS:
        share = ref.fragile_share(P, map_name, n, bsdf)
        _, out = ref.expected(P, map_name, n, bsdf)
        print(f"P={P} {map_name} n={n} {bsdf}: fragile points {100 * share:.2f} %, lit share {out['vis'].mean():.2f}")
        assert share <= FRAGILE_CAP
        assert np.isfinite(out["diff"]).all() and np.isfinite(out["spec"]).all() and np.isfinite(out["resi"]).all()
    assert P == 1 or 0.2 < out["vis"].mean() < 0.8                                      # lit and shadowed samples both occur


def test_scene_covers_what_it_is_for():
    ks = ref.points(214)["ks"]
    assert (ks[:, 1] == np.float32(0.08)).any() and ks[:, 1].max() == 1.0 and ks[:, 1].min() == np.float32(0.08)
    assert (ks[:, 2] == 0).any() and (ks[:, 2] == 1).any() and (ks[:, 0] > 0).any() and (ks[:, 0] == 0).any()
    assert ref.perms(3).shape == (7, 9) and {P for P, _, _ in ref.CASES} == set(ref.POINT_COUNTS)
    assert {m for _, m, _ in ref.CASES} == set(ref.MAPS) and {n for _, _, n in ref.CASES} == set(ref.SAMPLES_X)
    for name in ref.MAPS:
        light = ref.env_map(name)[0]
        assert light.max() > 100 * np.median(light) and (light[light.shape[0] - 2] == 0).all()


# ---- the C-ABI validates before it touches the device --------------------------------------------------------------------------
def _call(entry, **over):
    from geosplatting_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 16)()                                                          # a host pointer: never dereferenced on these paths
    p = C.cast(buf, C.c_void_p)
    a = dict(P=4, mask=p, ro=p, pos=p, nrm=p, view=p, kd=p, ks=p, H=4, W=8, light=p, pdf=p, rows=p, cols=p, T=3, n=2, perms=p, seed=5, bsdf=0,
             shadow=1.0, V=3, F=1, vertices=p, faces=p, bvh=p, lanes=0)
    a.update(over)
    tail = [p] * 3 + [None] * 3 + [None] if entry == "gs_envshade_fwd" else [-1] + [p] * 7 + [None]
    if "tail" in over:
        tail = over["tail"]
    rc = getattr(lib, entry)(*[a[k] for k in ("P", "mask", "ro", "pos", "nrm", "view", "kd", "ks", "H", "W", "light", "pdf", "rows", "cols", "T", "n",
                                              "perms", "seed", "bsdf", "shadow", "V", "F", "vertices", "faces", "bvh", "lanes")], *tail)
    return rc, lib.gs_last_error(), buf


@pytest.mark.parametrize("entry", ["gs_envshade_fwd", "gs_envshade_bwd"])
def test_argument_validation(entry):
    for over, text in ((dict(P=-1), b"negative P"), (dict(H=1), b"H >= 2"), (dict(W=1), b"W >= 2"), (dict(n=0), b"n_samples_x"),
                       (dict(T=0), b"T >= 1"), (dict(seed=1 << 31), b"rnd_seed"), (dict(seed=-1), b"rnd_seed"), (dict(bsdf=3), b"BSDF"),
                       (dict(F=0), b"empty mesh"), (dict(lanes=8), b"lanes_per_point"), (dict(light=None), b"NULL"), (dict(perms=None), b"NULL"),
                       (dict(bvh=None), b"NULL"), (dict(kd=None), b"null point input"), (dict(mask=None), b"null point input")):
        rc, err, _keep = _call(entry, **over)
        assert rc == -1 and text in err, (over, err)
    assert _call(entry, P=0, mask=None, kd=None)[0] == 0                               # no points: a no-op
    none_out = [None] * 3 + [None] * 3 + [None] if entry == "gs_envshade_fwd" else [-1] + [None] * 7 + [None]
    rc, err, _keep = _call(entry, tail=none_out)
    assert rc == -1 and b"null" in err
    if entry == "gs_envshade_fwd":
        rc, err, buf = _call(entry)
        p = C.cast(buf, C.c_void_p)
        rc, err, _keep = _call(entry, tail=[p] * 3 + [p, None, None] + [None])
        assert rc == -1 and b"all three" in err
    else:
        p = C.cast((C.c_float * 4)(), C.c_void_p)
        rc, err, _keep = _call(entry, tail=[99] + [p] * 7 + [None])
        assert rc == -1 and b"merge_rounds" in err


def test_python_ops_refuse_cpu_tensors_and_bad_arguments():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    z = torch.zeros(4, 3)
    light = torch.ones(4, 8, 3)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.env_shade(None, torch.ones(4), z, z, z, torch.zeros(3), z, z, light, light[..., 0], light[:, 0, 0], light[..., 0])
    with pytest.raises(ValueError, match="BSDF"):
        gs.env_shade(None, torch.ones(4), z, z, z, torch.zeros(3), z, z, light, light[..., 0], light[:, 0, 0], light[..., 0], BSDF="glossy")
    with pytest.raises(ValueError, match="at least 1"):
        gs.make_perms(0, "cpu")
    t = gs.make_perms(3, "cpu", tables=5, generator=torch.Generator().manual_seed(1))
    assert t.shape == (5, 9) and t.dtype == torch.int32 and torch.equal(t.sort(-1).values, torch.arange(9, dtype=torch.int32).expand(5, 9))
    from geosplatting_amd import envshade
    with pytest.raises(ValueError, match=r"gb_kd must be.*\(4, 2\)"):
        envshade._rows3("gb_kd", torch.zeros(4, 2), 4)
    with pytest.raises(ValueError, match="has 5 rows, expected 4"):
        envshade._rows3("ro", torch.zeros(1, 1, 5, 3), 4)
    assert envshade._rows3("ro", torch.zeros(1, 1, 5, 3), 5).shape == (5, 3)


def test_splat_mc_refuses_the_denoiser():
    import geosplatting_amd as gs
    attrs = gs.RenderableAttrs(kd=torch.zeros(2, 3), ks=torch.zeros(2, 2), normals=torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match="bilateral denoiser"):
        attrs.splat_mc(None, None, bvh=None, exposure=1.0, positions=torch.zeros(2, 3), envmap=None, min_roughness=0.1, max_metallic=1.0,
                       denoise=True)


def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    """The shadow ray is inlined into the shader with its one integer of traversal state: no private stack, no array indexed at run
    time.  The compiler's resource report for gfx950 must show 0 scratch bytes per lane for every kernel of csrc/gs_envshade.hip."""
    import os
    import re
    import shutil
    import subprocess
    from geosplatting_amd import build as B
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, *[f for f in B.FLAGS if f != "-fPIC"], "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(B.CSRC, "gs_envshade.hip"), "-o", str(tmp_path / "gs_envshade.o")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    report = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, flags=re.S)
    mine = {name: (int(vgprs), int(scratch)) for name, vgprs, scratch in report if "envshade_kernel" in name}
    print(mine)
    assert len(mine) == 9                                                              # 3 arrangements x (forward, forward with the log, backward)
    assert all(scratch == 0 for _, scratch in mine.values()), mine
