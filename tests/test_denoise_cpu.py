"""The bilateral denoiser without a GPU: the float64 restatement (tests/denoise_ref.py) against numbers worked by hand and against
its own transpose; the radius; argument validation of the C-ABI before the device is touched; the refusals of the Python ops; the
kernels' scratch."""
from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from tests import denoise_ref as ref


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _flat3x3(zdz_channels=1):
    col = torch.zeros(1, 3, 3, 1)
    nrm = torch.zeros(1, 3, 3, 3)
    nrm[..., 2] = 1.0
    zdz = torch.full((1, 3, 3, zdz_channels), 2.0)
    if zdz_channels == 2:
        zdz[..., 1] = 0.1
    return col, nrm, zdz


def test_centre_tap_has_weight_one_and_the_window_is_gaussian():
    """sigma = 1: v = 1, R = 7 covers the 3 x 3 image.  Flat guides: w = w_xy = exp(-d2 / 2), so the centre sees 1 + 4 e^-1/2 + 4 e^-1
    and a corner 1 + 2 e^-1/2 + e^-1 + 2 e^-2 + 2 e^-5/2 + e^-4."""
    col, nrm, zdz = _flat3x3()
    col[0, 1, 1, 0] = 1.0                                                              # a delta at the centre
    out, _, sums = ref.forward(col, nrm, zdz, 1.0)
    e = math.exp
    W_centre = 1 + 4 * e(-0.5) + 4 * e(-1.0)
    W_corner = 1 + 2 * e(-0.5) + e(-1.0) + 2 * e(-2.0) + 2 * e(-2.5) + e(-4.0)
    assert sums["W"][0, 1, 1].item() == pytest.approx(W_centre, rel=1e-14)
    assert sums["W"][0, 0, 0].item() == pytest.approx(W_corner, rel=1e-14)
    assert out[0, 1, 1, 0].item() == pytest.approx(1.0 / W_centre, rel=1e-14)          # the centre tap's weight is exactly 1
    assert out[0, 0, 0, 0].item() == pytest.approx(e(-1.0) / W_corner, rel=1e-14)      # the delta is the corner's diagonal tap
    assert sums["N"].min().item() == 9 and sums["N"].max().item() == 9


def test_a_tap_across_a_normal_crease():
    """the pixel right of the centre turns its normal so that the dot product is 0.99: its weight at the centre is e^-1/2 0.99^128"""
    col, nrm, zdz = _flat3x3()
    nrm[0, 1, 2] = torch.tensor([math.sqrt(1 - 0.99 ** 2), 0.0, 0.99])
    col[0, 1, 2, 0] = 1.0
    out, _, sums = ref.forward(col, nrm, zdz, 1.0)
    w = math.exp(-0.5) * float(torch.tensor(0.99, dtype=torch.float32).double()) ** 128
    W = 1 + 3 * math.exp(-0.5) + 4 * math.exp(-1.0) + w
    assert sums["W"][0, 1, 1].item() == pytest.approx(W, rel=1e-6)
    assert out[0, 1, 1, 0].item() == pytest.approx(w / W, rel=1e-6)
    nrm[0, 1, 2] = torch.tensor([1.0, 0.0, 0.0])                                       # a right angle: the clamp 1e-4, and 1e-512 = 0
    assert ref.forward(col, nrm, zdz, 1.0)[0][0, 1, 1, 0].item() == 0.0
    nrm[0, 1, 1] = 0.0                                                                 # a centre without a normal sees nothing: 0 / 1e-4
    out, _, sums = ref.forward(col + 1.0, nrm, zdz, 1.0)
    assert out[0, 1, 1, 0].item() == 0.0 and sums["W"][0, 1, 1].item() == 0.0


@pytest.mark.parametrize("zdz_channels", (1, 2))
def test_a_tap_across_a_depth_step(zdz_channels):
    """the pixel below the centre lies 0.3 deeper.  One channel: dz = z = 2, so w_z = exp(-0.3 / (2 * 1)); two channels: dz = 0.1, so
    w_z = exp(-0.3 / (0.1 * 1)) = e^-3.  Seen from that pixel the centre has the same weight, its own dz being 2.3 or 0.1."""
    col, nrm, zdz = _flat3x3(zdz_channels)
    zdz[0, 2, 1, 0] = 2.3
    col[0, 2, 1, 0] = 1.0
    out, _, sums = ref.forward(col, nrm, zdz, 1.0)
    z23 = float(torch.tensor(2.3, dtype=torch.float32).double())
    step = z23 - 2.0
    dz = 2.0 if zdz_channels == 1 else float(torch.tensor(0.1, dtype=torch.float32).double())
    w = math.exp(-0.5) * math.exp(-step / (dz * 1.0))
    W = 1 + 3 * math.exp(-0.5) + 4 * math.exp(-1.0) + w
    assert out[0, 1, 1, 0].item() == pytest.approx(w / W, rel=1e-12)
    # a diagonal neighbour of the deep pixel, (row 1, column 0): distance sqrt(2) in the denominator; its other taps are flat, at
    # d2 = 1 (three), 2 (one), 4 (one) and 5 (two)
    w_diag = math.exp(-1.0) * math.exp(-step / (dz * math.sqrt(2.0)))
    assert sums["W"][0, 1, 0].item() == pytest.approx(1 + 3 * math.exp(-0.5) + math.exp(-1.0) + w_diag + math.exp(-2.0) + 2 * math.exp(-2.5),
                                                      rel=1e-12)
    # the transposed weight: what the deep pixel gave the centre uses the deep pixel's own dz
    dz_deep = z23 if zdz_channels == 1 else dz
    g = ref.gather(col, None, nrm, zdz, 1.0, transpose=True)
    assert g["S"][0, 1, 1, 0].item() == pytest.approx(math.exp(-0.5) * math.exp(-step / (dz_deep * 1.0)), rel=1e-12)


def test_radius():
    assert [ref.radius(s) for s in (1e-4, 0.4, 0.41, 2.0)] == [3, 3, 5, 11]
    import geosplatting_amd as gs
    assert [gs.filter_radius(s) for s in (1e-4, 0.4, 0.41, 2.0, 4.2, 25.0)] == [3, 3, 5, 11, 23, 127]
    for bad in (0.0, -1.0, float("inf"), float("nan"), 25.3):
        with pytest.raises(ValueError, match="sigma"):
            gs.filter_radius(bad)


@pytest.mark.parametrize("zdz_channels", (1, 2))
def test_backward_is_the_transpose_of_forward(zdz_channels):
    """<g, D c> = <D^T g, c> in float64, with D^T by the restated transposed gather AND by autograd through the forward"""
    col, nrm, zdz, grad = ref.scene(2, 9, 11, 3, zdz_channels, seed=3)
    c = col.double().requires_grad_(True)
    out, _, sums = ref.forward(c, nrm, zdz, 0.5)
    lhs = (grad.double() * out).sum()
    auto, = torch.autograd.grad(lhs, c)
    mine, budget = ref.backward(grad, nrm, zdz, 0.5, sums)
    assert torch.allclose(mine, auto, rtol=1e-12, atol=1e-14)
    assert lhs.item() == pytest.approx((mine * col.double()).sum().item(), rel=1e-12)
    assert (budget > 0).all() and (ref.forward(col, nrm, zdz, 0.5)[1] > 0).all()
    assert (nrm.abs().sum(-1) == 0).any() and (sums["W"] == 0).any()                   # the scene has its zero-normal block


# ---- the C-ABI validates before it touches the device --------------------------------------------------------------------------
def _call(entry, **over):
    from geosplatting_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 16)()                                                           # a host pointer: never dereferenced on these paths
    p = C.cast(buf, C.c_void_p)
    a = dict(B=1, H=4, W=4, C=3, ZC=1, col=p, nrm=p, zdz=p, sigma=2.0, tiled=-1, out=p, wsum=p, grad=p)
    a.update(over)
    keys = (("B", "H", "W", "C", "ZC", "col", "nrm", "zdz", "sigma", "tiled", "out", "wsum") if entry == "gs_denoise_fwd" else
            ("B", "H", "W", "C", "ZC", "nrm", "zdz", "sigma", "tiled", "wsum", "grad", "out"))
    rc = getattr(lib, entry)(*[a[k] for k in keys], None)
    return rc, lib.gs_last_error(), buf


@pytest.mark.parametrize("entry", ["gs_denoise_fwd", "gs_denoise_bwd"])
def test_argument_validation(entry):
    cases = [(dict(B=0), b"at least 1"), (dict(H=0), b"at least 1"), (dict(W=-3), b"at least 1"), (dict(C=0), b"C must be 1..8"),
             (dict(C=9), b"C must be 1..8"), (dict(ZC=0), b"1 or 2 channels"), (dict(ZC=3), b"1 or 2 channels"),
             (dict(sigma=0.0), b"finite and positive"), (dict(sigma=-2.0), b"finite and positive"),
             (dict(sigma=float("nan")), b"finite and positive"), (dict(sigma=float("inf")), b"finite and positive"),
             (dict(sigma=25.3), b"must not exceed 127"), (dict(sigma=1e300), b"must not exceed 127"), (dict(B=65536), b"too large"),
             (dict(H=8 * 65535 + 1), b"too large"), (dict(tiled=2), b"tiled must be"), (dict(tiled=1, sigma=25.0), b"does not fit"),
             (dict(nrm=None), b"null input"), (dict(zdz=None), b"null input"), (dict(out=None), b"null output")]
    cases += [(dict(col=None), b"null input"), (dict(wsum=None), b"null output")] if entry == "gs_denoise_fwd" else \
             [(dict(grad=None), b"null input"), (dict(wsum=None), b"null input")]
    for over, text in cases:
        rc, err, _keep = _call(entry, **over)
        assert rc == -1 and text in err and entry.encode() in err, (over, err)


def test_the_tiled_form_fits_where_the_header_says():
    from geosplatting_amd import _lib
    fits = _lib.lib().gs_denoise_tiled_fits
    assert fits(3, 2.0) == 1 and fits(8, 2.0) == 1 and fits(3, 4.2) == 1               # R = 11 at every C, R = 23 at C = 3
    assert fits(3, 4.6) == 0 and fits(8, 4.2) == 0 and fits(1, 25.0) == 0
    assert fits(0, 2.0) == 0 and fits(9, 2.0) == 0 and fits(3, 0.0) == 0 and fits(3, float("nan")) == 0 and fits(3, 1e300) == 0


# ---- the Python ops refuse before they touch a device ------------------------------------------------------------------------------
def test_bilateral_denoiser_refuses_cpu_tensors_and_bad_shapes():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    col, nrm, zdz = torch.zeros(1, 4, 5, 3), torch.zeros(1, 4, 5, 3), torch.ones(1, 4, 5, 1)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.bilateral_denoiser(col, nrm, zdz, 2.0)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.bilateral_denoiser(col[0], nrm[0], zdz[0], 2.0, tiled=False)
    for args, text in (((torch.zeros(1, 4, 5, 9), nrm, zdz, 2.0), "1..8 channels"), ((col, torch.zeros(1, 4, 5, 2), zdz, 2.0), "nrm must have 3"),
                       ((col, nrm, torch.ones(1, 4, 5, 3), 2.0), "zdz must have 1 or 2"), ((col, nrm, torch.ones(1, 4, 6, 1), 2.0), "share"),
                       ((col.double(), nrm, zdz, 2.0), "float32"), ((col[0, 0], nrm[0, 0], zdz[0, 0], 2.0), "float32 tensor"),
                       ((col[None], nrm[None], zdz[None], 2.0), "float32 tensor"), ((col[:, :0], nrm[:, :0], zdz[:, :0], 2.0), "empty"),
                       ((col, nrm, zdz, 0.0), "sigma"), ((col, nrm, zdz, 26.0), "sigma")):
        with pytest.raises(ValueError, match=text):
            gs.bilateral_denoiser(*args)
    with pytest.raises(ValueError, match="tiled must be"):
        gs.bilateral_denoiser(col, nrm, zdz, 2.0, tiled=1)


def test_splat_mc_deferred_validates_before_touching_a_device():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    kw = dict(bvh=None, exposure=1.0, positions=torch.zeros(4, 4, 3), mask=torch.ones(4, 4, 1), envmap=None, min_roughness=0.1, max_metallic=1.0)
    attrs = gs.RenderableAttrs(kd=torch.zeros(2, 3), ks=torch.zeros(2, 2), normals=torch.zeros(2, 3), occ=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="glossy"):
        attrs.splat_mc_deferred(None, None, mode="glossy", **kw)
    with pytest.raises(ValueError, match="filmic"):
        attrs.splat_mc_deferred(None, None, tone_type="filmic", **kw)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        attrs.splat_mc_deferred(None, None, **kw)
    attrs.occ = None
    with pytest.raises(ValueError, match="needs RenderableAttrs.occ"):
        attrs.splat_mc_deferred(None, None, **kw)


# ---- the kernels' private memory ---------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    """The accumulators are arrays of the template's C entries, fully unrolled: no array is indexed at run time.  The compiler's resource
    report for gfx950 must show 0 scratch bytes per lane for every kernel of csrc/gs_denoise.hip."""
    import os
    import re
    import shutil
    import subprocess
    from geosplatting_amd import build as B
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, *[f for f in B.FLAGS if f != "-fPIC"], "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(B.CSRC, "gs_denoise.hip"), "-o", str(tmp_path / "gs_denoise.o")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    report = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, flags=re.S)
    mine = {name: (int(vgprs), int(scratch)) for name, vgprs, scratch in report if "denoise_kernel" in name}
    print(mine)
    assert len(mine) == 32                                                             # 8 channel counts x (forward, backward) x (tiled, plain)
    assert all(scratch == 0 for _, scratch in mine.values()), mine
