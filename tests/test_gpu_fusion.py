"""GPU tests of depth fusion (csrc/gs_tsdf.hip through geosplatting_amd.fusion) against the float64 restatement tests/tsdf_ref.py.

Integration is compared PER VOXEL.  A float32 evaluation may decide a voxel differently from float64 only where a decision is
within rounding of its threshold; such voxels are *fragile* and left out of the per-element comparison (tsdf_ref.integrate):
  * u or v (float64) within 2^-10 px of an integer, for a view that has the voxel in front of it and within a pixel of its image:
    fp32 u at |u| <= 128 carries about 1e-4 px of error from the camera transform and the (1 ulp) reciprocal, 2^-10 is ten times that;
  * sdf + sdf_trunc within 8 * 2^-23 * (|d| + |z|) of 0.
The alpha and depth thresholds compare float32 data with float32 constants: the same decision in both.  Every test asserts that
at most 5 % of the volume is fragile (the reference alone gives about 3 % with 8 views), so a generous margin cannot hide a failure.

On the other voxels the weight is exact and the tsdf is within

    budget = (8 * mag / sdf_trunc + 4 * w) * 2^-23,     mag = max over the contributing views of |d| + S     (S below)

derived from the arithmetic, not from what the kernel returns (eps = 2^-23 is one ulp of 1, a rounding is at most eps / 2 relative):
  * the voxel centre p_j = origin_j + (i_j + 0.5) voxel_size: a product and a sum, |error| <= eps (|origin_j| + |p_j|);
  * z = R_20 p_0 + R_21 p_1 + R_22 p_2 + t_2: three products and three sums, six roundings of eps / 2, each relative to a partial sum
    bounded by sum_j |R_2j| |p_j| + |t_2|: 3 eps of it; with the inherited error of p, sum_j |R_2j| eps (|origin_j| + |p_j|): at most
    4 eps S with S = sum_j |R_2j| (|origin_j| + |p_j|) + |t_2|.  S, not |z|: the terms cancel when the camera is close to the voxel;
  * sdf = d - z: one rounding, eps (|d| + |z|) / 2;  val = sdf / sdf_trunc (a product with the rounded reciprocal: two roundings,
    eps |val| <= eps (|d| + |z|) / sdf_trunc);  min(1, .) only shrinks an error.
    Sum: (4 S + 1.5 (|d| + |z|)) eps / sdf_trunc <= 5.5 mag eps / sdf_trunc since |z| <= S; written 8 mag eps / sdf_trunc;
  * the running mean (tsdf w + val) rcp(w + 1): a product and a sum on values <= w + 1, then a product with the hardware reciprocal
    (1 ulp, of a small integer): at most 2.5 eps on the new mean, and the errors already in tsdf and val enter with weights w / (w + 1) and 1 / (w + 1),
    so the val errors AVERAGE (<= their maximum) and the step errors add up to 2.5 eps w; written 4 eps w.
This is (8 (|d| + |z|) / sdf_trunc + 4 w) 2^-23 with |z| replaced by S >= |z|, the magnitude the rounding error of z scales with.
Measured on an MI355X: the largest error is 0.03 of the budget in every test; no weight differs, fragile voxels included.
"""
import math

import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd import synthetic as syn
from geosplatting_amd.fusion import camera_matrices
from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu

BOUNDS = ((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8))
RADIUS = 0.5
SIZE = 64
FRAGILE_CAP = 0.05


# ------------------------------------------------------------------------------------------------ scenes
def _camera(eye, target, fov, size, dev):
    c2w = gs.lookat_c2w(torch.tensor(eye, dtype=torch.float32), torch.tensor(target, dtype=torch.float32), torch.tensor([0.0, 0.0, 1.0]))
    f = 0.5 * size / math.tan(math.radians(fov) * 0.5)
    return gs.Camera(c2w.contiguous().to(dev), f, f, 0.5 * size, 0.5 * size, size, size)


def _matrices(cams):
    """the float32 matrices integrate hands to the kernel (elementwise, so the same whatever the batch), on the host"""
    vms, Ks = camera_matrices(cams, cams[0].c2w.device)
    return vms.cpu().numpy(), Ks.cpu().numpy()


def _views(cams, far_hit=()):
    """(depth maps [H,W,2] float32 numpy of the analytic sphere, viewmats, Ks)"""
    vms, Ks = _matrices(cams)
    das = [ref.sphere_depth(vm.astype(np.float64), K.astype(np.float64), c.width, c.height, RADIUS, far_hit=(i in far_hit))
           for i, (vm, K, c) in enumerate(zip(vms, Ks, cams))]
    return das, vms, Ks


class Scene:
    """The analytic sphere seen by `n` Fibonacci cameras at radius 3 (64^2, `fov` degrees) plus, with `awkward`, the cases the kernel
    has branches for.  Built once per module; nothing mutates it."""

    def __init__(self, dev, n=8, fov=40.0, awkward=True):
        cams = [_camera(tuple(float(x) for x in e), (0.0, 0.0, 0.0), fov, SIZE, dev) for e in ref.fibonacci_sphere(n, 3.0)]
        if awkward:
            cams.append(_camera((0.65, 0.6, 0.55), (0.0, 0.0, 0.0), 70.0, SIZE, dev))     # inside the volume: voxels with z <= 0
            cams.append(_camera((3.0, 0.0, 0.0), (3.0, 3.0, 0.5), 40.0, SIZE, dev))       # looks past the volume: every brick culled
        das, self.vms, self.Ks = _views(cams)
        if awkward:
            das[0][20:24, :, 1] = 0.3                                                     # a band below alpha_trunc
            das[1][30:34, 28:36, 0] = 4.0 + np.arange(8, dtype=np.float32)[None] * 0.25  # depths >= depth_trunc (4.0 itself included)
            das[-1][...] = np.array([2.0, 1.0], np.float32)                               # the culled view would count if it were hit
            for da in das[:-1]:
                da[..., 0][da[..., 1] == 0] = np.nan                                      # NaN depth where alpha is 0
        self.cams, self.das = cams, das
        self.das_dev = [torch.from_numpy(d).to(dev) for d in das]

    def reference(self, vol, views=None):
        idx = range(len(self.cams)) if views is None else views
        z = np.zeros(int(np.prod(vol.resolution)))
        return ref.integrate(z, z, [self.das[i] for i in idx], self.vms[list(idx)], self.Ks[list(idx)], vol.resolution,
                             np.float32(vol.origin).astype(np.float64), float(np.float32(vol.voxel_size)),
                             float(np.float32(vol.sdf_trunc)))


@pytest.fixture(scope="module")
def scene(cuda):
    return Scene(cuda)


def _compare(vol, expect, label, n_views):
    tsdf_r, w_r, fragile, mag = expect
    got = vol.volume.reshape(-1, 2).cpu().numpy().astype(np.float64)
    keep = ~fragile
    budget = ref.tsdf_budget(mag, w_r, float(np.float32(vol.sdf_trunc)))
    err = np.abs(got[:, 0] - tsdf_r)
    ratio = (err[keep] / np.maximum(budget[keep], 1e-30)).max()
    print("%s: fragile %.4f, weight mismatches %d (fragile ones %d), max err / budget %.3f, observed voxels %d" % (
        label, fragile.mean(), int((got[keep, 1] != w_r[keep]).sum()), int((got[fragile, 1] != w_r[fragile]).sum()), ratio,
        int((w_r > 0).sum())))
    assert fragile.mean() <= FRAGILE_CAP
    assert (w_r > 0).mean() > 0.2                                    # the scene does observe the volume
    assert np.array_equal(got[keep, 1], w_r[keep])
    assert np.isfinite(got).all()
    assert (err[keep] <= budget[keep]).all()
    # a fragile voxel may differ in the views that are in doubt, never by more than all of them
    assert np.abs(got[fragile, 1] - w_r[fragile]).max(initial=0.0) <= n_views


# ------------------------------------------------------------------------------------------------ 1. integration per voxel
@pytest.mark.parametrize("resolution", [32, (20, 24, 28)], ids=["32", "20x24x28"])
def test_integration_per_voxel(cuda, scene, resolution):
    """32^3 (bricks of 8 x 8 x 4 tile it exactly) and 20 x 24 x 28 (non-cubic, 20 no multiple of the brick's 8: partial bricks): the ten
    views of the scene in one launch -- alpha band, depths past depth_trunc, NaN depth, a camera inside the volume and a culled one."""
    vol = gs.TSDFVolume(resolution, bounds=BOUNDS, device=cuda)
    vol.integrate(scene.das_dev, scene.cams)
    expect = scene.reference(vol)
    _compare(vol, expect, "per-voxel %s" % (resolution,), len(scene.cams))
    w = vol.weight.cpu().numpy()
    assert w.max() <= len(scene.cams) - 1                            # the culled view never counts
    assert vol.tsdf.shape == tuple(reversed(vol.resolution)) and vol.tsdf.data_ptr() == vol.volume.data_ptr()
    # the awkward cases are exercised: the inside camera has voxels behind it, the alpha band and far depths reject voxels
    p = ref.voxel_centres(vol.resolution, vol.origin, vol.voxel_size)
    assert ((p @ scene.vms[8][2, :3] + scene.vms[8][2, 3]) <= 0).any()
    assert ((p @ scene.vms[9][2, :3] + scene.vms[9][2, 3]) > 0).any()    # the culled view fails on its side planes, not only on z


# ------------------------------------------------------------------------------------------------ 2. launch-split invariance
def test_launch_split_is_bit_identical(cuda, scene):
    views = list(range(8))
    vols = []
    for split in ([8], [3, 5], [1] * 8):
        vol = gs.TSDFVolume(32, bounds=BOUNDS, device=cuda)
        lo = 0
        for n in split:
            idx = views[lo:lo + n]
            vol.integrate([scene.das_dev[i] for i in idx], [scene.cams[i] for i in idx])
            lo += n
        vols.append(vol.volume.clone())
    assert torch.equal(vols[0], vols[1]) and torch.equal(vols[0], vols[2])
    assert vols[0][..., 1].max().item() >= 4


def test_twenty_views_split_internally(cuda):
    """20 views = launches of 16 + 4 inside one integrate call, as a [B,H,W,2] tensor.  A 16-degree field of view keeps the voxels
    that a view has in its image, and with them the fragile ones, below the cap (the reference alone: 2.4 %; 5.05 % at 24 degrees)."""
    sc = Scene(cuda, n=20, fov=16.0, awkward=False)
    vol = gs.TSDFVolume(32, bounds=BOUNDS, device=cuda)
    vol.integrate(torch.stack(sc.das_dev), sc.cams)
    _compare(vol, sc.reference(vol), "20 views", 20)
    assert vol.weight.max().item() >= 10


# ------------------------------------------------------------------------------------------------ 3. extraction
def _check_extraction(vol, label):
    v, f = vol.extract_mesh()
    flat = vol.volume.reshape(-1, 2).cpu().numpy()
    origin, vs = np.float32(vol.origin).astype(np.float64), float(np.float32(vol.voxel_size))
    counts, v_ref, f_ref = ref.extract(flat[:, 0], flat[:, 1], vol.resolution, origin, vs)
    print("%s: counts device %s reference %s" % (label, vol.last_counts, counts.tolist()))
    assert list(vol.last_counts) == counts.tolist()
    assert v.shape == (counts[0], 3) and v.dtype == torch.float32 and f.shape == (counts[1], 3) and f.dtype == torch.int64
    fh, vh = f.cpu().numpy(), v.cpu().numpy().astype(np.float64)
    assert np.array_equal(fh, f_ref)                                 # numbering included
    tol = 4 * ref.EPS * (np.abs(v_ref) + vs)
    assert (np.abs(vh - v_ref) <= tol).all(), float((np.abs(vh - v_ref) / tol).max())
    if counts[1]:
        assert fh.min() >= 0 and fh.max() < counts[0] and len(np.unique(fh)) == counts[0]
    return v, f, v_ref


def test_extraction_of_integrated_volume(cuda, scene):
    vol = gs.TSDFVolume(32, bounds=BOUNDS, device=cuda)
    vol.integrate(scene.das_dev, scene.cams)
    v, f, v_ref = _check_extraction(vol, "integrated 32^3")
    assert f.shape[0] > 1000
    # as close to the sphere as the reference's mesh of the same volume (the close-up camera of this scene pulls it past the 1.5
    # voxels of the plain 8-view scene, in both)
    m_ref = np.abs(np.linalg.norm(v_ref, axis=1) - RADIUS).max()
    assert (v.norm(dim=1) - RADIUS).abs().max().item() <= m_ref + 0.01 * vol.voxel_size
    tri = v[f]
    n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    assert ((n * tri.mean(1)).sum(-1) > 0).float().mean().item() > 0.99        # normals toward free space


def test_extraction_of_random_volume(cuda):
    """12 x 10 x 9: 30 % zero weights, random signs, exact zeros (outside), equal neighbours; 1080 voxels = 5 blocks, the last partial"""
    rng = np.random.default_rng(11)
    res = (12, 10, 9)
    n = res[0] * res[1] * res[2]
    t = (rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.05, 1.0, size=n)).astype(np.float32)
    t[rng.random(n) < 0.05] = 0.0
    t[rng.random(n) < 0.02] = -0.0
    eq = np.nonzero(rng.random(n - 1) < 0.1)[0]
    t[eq + 1] = t[eq]
    w = np.where(rng.random(n) < 0.3, 0.0, rng.integers(1, 9, size=n)).astype(np.float32)
    vol = gs.TSDFVolume(res, bounds=((-0.3, 0.1, 1.0), (0.9, 1.1, 1.9)), device=cuda)
    assert vol.resolution == res
    vol.volume.copy_(torch.from_numpy(np.stack((t, w), -1).reshape(res[2], res[1], res[0], 2)))
    _, f, _ = _check_extraction(vol, "random 12x10x9")
    assert f.shape[0] > 50 and 0 < vol.last_counts[2] < 11 * 9 * 8


def test_extraction_of_empty_volume(cuda):
    vol = gs.TSDFVolume((9, 8, 7), bounds=BOUNDS, device=cuda)
    v, f = vol.extract_mesh()
    torch.cuda.synchronize()
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64 and vol.last_counts == (0, 0, 0, 0)
    vol.volume[..., 0] = -1.0                                        # signs but no weights: still nothing
    assert vol.extract_mesh()[1].shape == (0, 3)
    one = gs.TSDFVolume((1, 1, 1), bounds=((0, 0, 0), (1, 1, 1)), device=cuda)
    one.volume[..., 1] = 1.0
    assert one.extract_mesh()[0].shape == (0, 3) and one.last_counts == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 4. end to end
def _sphere_gaussians(dev):
    v, f = syn.icosphere(3, radius=RADIUS)
    v, f = v.to(dev), f.to(dev)
    sp, _ = gs.mesh_to_splats(v, f, gs.vertex_normals(v, f))
    n = sp.means.shape[0]
    return gs.GaussianSet(means=sp.means, scales=sp.scales, quats=sp.quats, opacities=sp.opacities.reshape(n, 1),
                          colors=torch.full((n, 3), 0.5, device=dev), shs=torch.zeros(n, 3, 3, device=dev))


def _end_to_end(model, dev):
    kw = dict(num_views=12, radius=3.0, image_size=128)
    model.train()
    v, f = model.extract_mesh(resolution=48, bounds=BOUNDS, generator=torch.Generator().manual_seed(5), **kw)
    assert model.training                                            # the mode is restored
    assert v.shape[0] > 500 and f.shape[0] > 500 and f.max().item() == v.shape[0] - 1
    # the reference on the very depth maps the model rendered
    cams = [c.to(dev) for c in gs.sphere_cameras(kw["num_views"], kw["radius"], kw["image_size"], kw["image_size"],
                                                 generator=torch.Generator().manual_seed(5))]
    model.eval()
    with torch.no_grad():
        das = [model.render_depth(c).cpu().numpy() for c in cams]
    vms, Ks = _matrices(cams)
    res, vs = (48, 48, 48), float(np.float32(1.6 / 48))
    origin = np.float32(BOUNDS[0]).astype(np.float64)
    z = np.zeros(48 ** 3)
    tsdf, w, _, _ = ref.integrate(z, z, das, vms, Ks, res, origin, vs, float(np.float32(5 * (1.6 / 48))), alpha_trunc=0.5)
    _, v_ref, f_ref = ref.extract(tsdf, w, res, origin, vs)
    m_ref = np.abs(np.linalg.norm(v_ref, axis=1) - RADIUS).max()
    m_dev = (v.norm(dim=1) - RADIUS).abs().max().item()
    print("end to end: device V %d F %d, reference V %d F %d, max | |v| - r | device %.5f reference %.5f (voxel %.5f)" % (
        v.shape[0], f.shape[0], v_ref.shape[0], f_ref.shape[0], m_dev, m_ref, vs))
    assert m_dev <= m_ref + 0.01 * vs
    return v, f


def test_end_to_end_surfel_sphere(cuda, tmp_path):
    model = gs.SurfelModel(gaussians=_sphere_gaussians(cuda), background_color="black")
    v, f = _end_to_end(model, cuda)
    gs.save_obj(tmp_path / "sphere.obj", v, f)
    assert sum(1 for _ in open(tmp_path / "sphere.obj")) == v.shape[0] + f.shape[0]


def test_end_to_end_3dgs_sphere(cuda):
    """GSplatModel in 3DGS mode through the same call: the method is not surfel-only"""
    _end_to_end(gs.GSplatModel(gaussians=_sphere_gaussians(cuda), background_color="black"), cuda)


def test_mesh_from_depth_fusion(cuda, scene):
    """The reference's signature: voxel_size / sdf_trunc given, depth_scale applied"""
    das = [torch.cat((d[..., :1] * 2.0, d[..., 1:]), -1) for d in scene.das_dev[:8]]
    v, f = gs.mesh_from_depth_fusion(das, scene.cams[:8], voxel_size=0.05, sdf_trunc=0.25, depth_scale=2.0, bounds=BOUNDS)
    vol = gs.TSDFVolume(voxel_size=0.05, bounds=BOUNDS, sdf_trunc=0.25, device=cuda)
    assert vol.resolution == (32, 32, 32)
    v2, f2 = vol.integrate(scene.das_dev[:8], scene.cams[:8]).extract_mesh()
    assert torch.equal(f, f2) and torch.equal(v, v2) and f.shape[0] > 1000
