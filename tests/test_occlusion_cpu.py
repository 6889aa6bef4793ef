"""No-GPU checks of the ambient-occlusion map and the shaders on it: the float64 restatement tests/ao_ref.py against known answers,
the fragile cap of every scene the GPU tests use -- asserted from the restatement alone -- and the argument validation of the new
Python surface."""
import numpy as np
import pytest
import torch

import geosplatting_amd as gs
from geosplatting_amd._lib import GeoSplatHipError
from tests import ao_ref


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
def test_ao_known_answers():
    """an isolated convex sphere sees every front-facing target; the floor of a closed box sees none"""
    v, f = ao_ref.uv_sphere(0.5)
    tri = v.astype(np.float64)[f]
    cen = tri.mean(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.all((nrm * cen).sum(1) > 0)                                               # outward winding
    rng = np.random.default_rng(3)
    tg = rng.normal(size=(16, 3))
    tg = (3.0 * tg / np.linalg.norm(tg, axis=1, keepdims=True)).astype(np.float32)
    res = ao_ref.evaluate(v, f, cen[::7].astype(np.float32), nrm[::7].astype(np.float32), tg)
    assert np.all(res["vis"] == 1.0) and not res["hit"][res["counts"]].any()
    bv, bf = ao_ref.closed_box(0.5)
    floor = np.array([[0.1, -0.2, -0.5], [0.0, 0.0, -0.5]], dtype=np.float32)
    up = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    res = ao_ref.evaluate(bv, bf, floor, up, tg)
    assert res["counts"].any(1).all() and np.all(res["vis"] == 0.0)
    bad = floor.copy()
    bad[0, 0] = np.nan
    assert float(ao_ref.evaluate(bv, bf, bad, up, tg)["vis"][0]) == 0.0


# ---- the fragile caps: a condition on the scenes, from the restatements alone ------------------------------------------------------
@pytest.mark.parametrize("P", ao_ref.P_VALUES)
def test_ao_fragile_cap(P):
    for S in ao_ref.S_VALUES:
        res = ao_ref.expected(P, S)
        n = int(res["fragile"].sum())
        print(f"P = {P}, S = {S}: {n} fragile points of {P}, visibility {res['vis'].min():.3f} .. {res['vis'].max():.3f}")
        assert n <= ao_ref.FRAGILE_CAP * P
        if P >= 67:
            assert res["vis"].min() < 0.5 < res["vis"].max() and float(res["vis"][5]) == 0.0


# ---- argument validation without a GPU ---------------------------------------------------------------------------------------------
def _shade_args():
    tex = gs.Texture2D.from_constants((0.1, 0.2, 0.3))
    env = gs.TextureSplitSum(torch.rand(6, 16, 16, 3), [torch.rand(6, r, r, 3) for r in (64, 32, 16)])
    z = torch.zeros(4, 4, 3)
    return (z, z, z[..., :2], torch.zeros(4, 4, 4), tex, tex, torch.zeros(3), env)


def test_shade_pixels_visibility_arguments():
    args = _shade_args()
    for mode in ("ao", "screen"):
        with pytest.raises(ValueError, match="visibility"):
            gs.shade_pixels(*args, occlusion=mode)
        with pytest.raises(ValueError, match="visibility"):
            gs.shade_pixels(*args, occlusion=mode, visibility=torch.ones(4, 5))
        with pytest.raises(GeoSplatHipError, match="GPU only"):
            gs.shade_pixels(*args, occlusion=mode, visibility=torch.ones(4, 4))
    for mode in ("texture", "none"):
        with pytest.raises(ValueError, match="visibility"):
            gs.shade_pixels(*args, occlusion=mode, visibility=torch.ones(4, 4))
    with pytest.raises(ValueError, match="screen"):
        gs.shade_pixels(*args, occlusion="ssao")
    with pytest.raises(ValueError):
        gs.shade_pixels(*args, occlusion="ssao", visibility=torch.ones(4, 4))


def test_occlusion_arguments():
    bvh = gs.MeshBVH.__new__(gs.MeshBVH)                                               # (a real one needs a GPU)
    p = torch.zeros(5, 3)
    with pytest.raises(TypeError):
        gs.ambient_occlusion(None, p, p)
    with pytest.raises(ValueError, match="targets"):
        gs.ambient_occlusion(bvh, p, p, torch.zeros(0, 3))
    with pytest.raises(ValueError, match="targets"):
        gs.ambient_occlusion(bvh, p, p, torch.zeros(4097, 3))
    with pytest.raises(ValueError, match="share"):
        gs.ambient_occlusion(bvh, p, torch.zeros(4, 3), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="lanes"):
        gs.ambient_occlusion(bvh, p, p, torch.zeros(8, 3), lanes=32)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.ambient_occlusion(bvh, p, p, torch.zeros(8, 3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.face_ambient_occlusion(torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]]))
    lib = gs._lib.lib()
    assert lib.gs_ray_ao(3, 1, None, None, None, 0, None, None, 4097, None, 0.0, 0, None, None, None, None) == -1
    assert b"1..4096" in lib.gs_last_error()
    assert lib.gs_ray_ao(3, 1, None, None, None, 0, None, None, 0, None, 0.0, 0, None, None, None, None) == -1
    assert not hasattr(gs, "ssao"), "the screen-space map is not provided"


def test_render_arguments():
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    cam = gs.Camera(torch.from_numpy(ao_ref.lookat((0.0, -2.0, 1.0), (0.0, 0.0, 0.0))), 4.0, 4.0, 2.0, 2.0, 4, 4)
    tex = gs.Texture2D.from_constants((0.1, 0.2, 0.3))
    light = gs.LatLngEnvMap(torch.rand(8, 16, 3))
    with pytest.raises(ValueError, match="render_type"):
        gs.render_mesh_mc(v, f, cam, kd=tex, ks=tex, uvs=None, envmap=light, render_type="shadow")
    with pytest.raises(ValueError, match="transform"):
        gs.render_mesh_mc(v, f, cam, kd=tex, ks=tex, uvs=None, envmap=gs.LatLngEnvMap(torch.rand(8, 16, 3)).rotateZ_(0.3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.render_mesh_mc(v, f, cam, kd=tex, ks=tex, uvs=None, envmap=light)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.render_mesh(v, f, cam, outputs=("ao",))
