"""No-GPU checks behind tests/test_gpu_envmap.py: the float32-against-float64 ratios of the restatement (tests/envmap_ref.py) that fix
KAPPA, the fragile shares of the test inputs, the frame algebra of the two map classes and the Radiance .hdr reader and writer."""
import math

import numpy as np
import pytest
import torch

from geosplatting_amd import envmap as E
from geosplatting_amd.envshade import LatLngEnvMap
from tests import envmap_ref as ref


def _conversion_ratios(k):
    R, H, W, _ = ref.CASES[k]
    x = ref.case_inputs(k)
    out = {}
    for name, fn in (("cube -> lat-long", lambda dt: ref.cube_to_latlng(x["cube"], H, W, x["transform"], x["cot_latlng"], dt)),
                     ("lat-long -> cube", lambda dt: ref.latlng_to_cube(x["latlng"], R, x["cot_cube"], dt))):
        want, got = fn(torch.float64), fn(torch.float32)
        out[name] = (ref.worst_ratio(got["value"], want["value"], want["mag"], name),
                     ref.worst_ratio(got["grad"], want["grad"], want["mag_grad"], name + " gradient"))
    return out


def test_float32_restatement_fixes_kappa():
    forward, texel = {}, {}
    for k in range(len(ref.CASES)):
        for name, (f, t) in _conversion_ratios(k).items():
            forward[name] = max(forward.get(name, 0.0), f)
            texel[name] = max(texel.get(name, 0.0), t)
            print(f"\n  case {ref.CASES[k]} {name}: float32 restatement forward {f:.4f}, texel gradient {t:.4f} of 1e-4 x magnitude", end="")
    s = ref.sample_inputs()
    keep = ~ref.fragile_dirs(s["dirs"], ref.SAMPLE_R)
    cot = s["cot"] * keep[:, None]
    want, got = (ref.sample_cubemap(s["cube"], s["dirs"], cot, dt) for dt in (torch.float64, torch.float32))
    forward["sample"] = ref.worst_ratio(got["value"], want["value"], want["mag"], "sample", keep)
    texel["sample"] = ref.worst_ratio(got["grad"], want["grad"], want["mag_grad"], "sample gradient")
    b = ref.background_inputs()
    for srgb in (True, False):
        want, got = (ref.background(b["cube"], ref.BG["H"], ref.BG["W"], ref.BG["fx"], ref.BG["fy"], ref.BG["cx"], ref.BG["cy"], b["c2w"],
                                    b["transform"], srgb, dt) for dt in (torch.float64, torch.float32))
        forward["background"] = max(forward.get("background", 0.0),
                                    ref.worst_ratio(got["value"], want["value"], want["mag"], "background", ~want["fragile"]))
    worst = max(max(forward.values()), max(texel.values()))
    print(f"\n  forward {forward}\n  texel gradients {texel}\n  worst {worst:.4f} -> KAPPA {ref.smallest_power_of_two_at_least(2 * worst)}")
    assert ref.KAPPA == ref.smallest_power_of_two_at_least(2 * worst)
    assert max(forward.values()) == pytest.approx(ref.MEASURED_FORWARD, rel=0.25)
    assert max(texel.values()) == pytest.approx(ref.MEASURED_TEXEL, rel=0.25)


def test_no_conversion_element_is_fragile():
    gaps = []
    for k, (R, H, W, _) in enumerate(ref.CASES):
        gap = ref.face_gap(ref.latlng_dirs(H, W, ref.case_inputs(k)["transform"], torch.float64), R)
        gaps.append(float(gap.min()))
        assert int((gap < ref.DELTA).sum()) == 0, (ref.CASES[k], float(gap.min()))
    print(f"\n  smallest distance from a face boundary per case, in texels: {gaps}")
    assert min(gaps) > 2 * ref.DELTA


def test_fragile_shares_of_random_directions_and_background():
    s = ref.sample_inputs()
    share = float(ref.fragile_dirs(s["dirs"], ref.SAMPLE_R).float().mean())
    b = ref.background_inputs()
    g = ref.BG
    frag = ref.fragile_dirs(ref.camera_dirs(g["H"], g["W"], g["fx"], g["fy"], g["cx"], g["cy"], b["c2w"], b["transform"], torch.float64), g["R"])
    print(f"\n  fragile: {100 * share:.3f} % of the random directions, {100 * float(frag.float().mean()):.3f} % of the background pixels")
    assert share <= ref.FRAGILE_CAP and float(frag.float().mean()) <= ref.FRAGILE_CAP
    faces = torch.unique(ref.tr._select_face(ref.camera_dirs(g["H"], g["W"], g["fx"], g["fy"], g["cx"], g["cy"], b["c2w"], b["transform"],
                                                            torch.float64)))
    assert faces.numel() >= 2                                             # the background crosses a seam


def test_restatement_keeps_a_constant_map_and_rows_run_y_down():
    """cube -> lat-long -> cube of a constant map is that constant; the lat-long rows run y-down (row 0 looks up)"""
    c = torch.full((6, 8, 8, 3), 0.75, dtype=torch.float64)
    lat = ref.cube_to_latlng(c, 6, 12)["value"]
    assert torch.allclose(lat, torch.full_like(lat, 0.75), atol=1e-14)
    back = ref.latlng_to_cube(lat, 4)["value"]
    assert torch.allclose(back, torch.full_like(back, 0.75), atol=1e-14)
    d = ref.latlng_dirs(6, 12, None, torch.float64).reshape(6, 12, 3)
    assert bool((d[0, :, 1] > 0.8).all()) and bool((d[-1, :, 1] < -0.8).all())
    up = torch.zeros(6, 8, 8, 3, dtype=torch.float64)
    up[2] = 1.0                                                           # face +y
    lat = ref.cube_to_latlng(up, 6, 12)["value"]
    assert float(lat[0].min()) == 1.0 and float(lat[-1].max()) == 0.0


# ------------------------------------------------------------------------------------------------ frames
def test_frame_matrices_and_algebra():
    zy, yz = E.frame_z_up_to_y_up(), E.frame_y_up_to_z_up()
    assert torch.equal(zy, torch.tensor([[0.0, -1, 0], [0, 0, 1], [-1, 0, 0]]))
    assert torch.equal(yz, torch.tensor([[0.0, 0, -1], [-1, 0, 0], [0, 1, 0]]))
    assert torch.equal(yz @ zy, torch.eye(3)) and torch.equal(zy @ yz, torch.eye(3))
    a, b = 0.4, 0.9
    for axis in "xyz":
        Ra, Rb, Rab = E.frame_rotation(axis, a), E.frame_rotation(axis, b), E.frame_rotation(axis, a + b)
        assert torch.allclose(Rb @ Ra, Rab, atol=2e-7)
        assert torch.allclose(Ra @ Ra.T, torch.eye(3), atol=2e-7) and float(torch.linalg.det(Ra)) == pytest.approx(1.0, abs=1e-6)
    c, s = math.cos(a), math.sin(a)
    assert torch.allclose(E.frame_rotation("x", a), torch.tensor([[1.0, 0, 0], [0, c, -s], [0, s, c]]), atol=1e-7)
    assert torch.allclose(E.frame_rotation("y", a), torch.tensor([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]), atol=1e-7)
    assert torch.allclose(E.frame_rotation("z", a), torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), atol=1e-7)


@pytest.mark.parametrize("make", [lambda: E.EnvCubeMap(torch.zeros(6, 2, 2, 3)), lambda: LatLngEnvMap(torch.zeros(2, 4, 3))])
def test_frame_methods_compose_new_at_old(make):
    m = make()
    assert m.transform is None
    m.rotateY_(0.4)
    assert torch.equal(m.transform, E.frame_rotation("y", 0.4))
    m.rotateY_(0.9)
    assert torch.allclose(m.transform, E.frame_rotation("y", 1.3), atol=2e-7)
    m = make()
    m.rotateX_(0.3)
    m.z_up_to_y_up_()                                                     # the later change is applied last: new @ old
    assert torch.equal(m.transform, E.frame_z_up_to_y_up() @ E.frame_rotation("x", 0.3))
    assert not torch.allclose(m.transform, E.frame_rotation("x", 0.3) @ E.frame_z_up_to_y_up())
    m.y_up_to_z_up_()
    assert torch.allclose(m.transform, E.frame_rotation("x", 0.3), atol=1e-7)
    m.rotateZ_(-0.2)
    assert torch.allclose(m.transform, E.frame_rotation("z", -0.2) @ E.frame_rotation("x", 0.3), atol=2e-7)
    twin = m.clone()
    twin.rotateY_(1.0)
    assert torch.allclose(m.transform, E.frame_rotation("z", -0.2) @ E.frame_rotation("x", 0.3), atol=2e-7)   # a clone owns its frame


def test_maps_validate_shapes_and_transforms():
    with pytest.raises(ValueError):
        E.EnvCubeMap(torch.zeros(6, 4, 5, 3))
    with pytest.raises(ValueError):
        E.EnvCubeMap(torch.zeros(6, 4, 4, 3), transform=torch.eye(4))
    with pytest.raises(ValueError):
        LatLngEnvMap(torch.zeros(4, 8, 3), transform=torch.zeros(3))
    with pytest.raises(ValueError, match="without a transform"):
        E.EnvCubeMap(torch.zeros(6, 4, 4, 3), transform=torch.eye(3)).as_splitsum()
    assert torch.equal(E.blend_background(torch.tensor([[0.2, 0.4, 0.6, 0.25]]), torch.tensor([[1.0, 1.0, 0.0]])),
                       torch.tensor([[0.25 * 0.2 + 0.75, 0.25 * 0.4 + 0.75, 0.25 * 0.6]]))


# ------------------------------------------------------------------------------------------------ .hdr
def _hdr_picture():
    g = torch.Generator().manual_seed(7)
    x = torch.rand(9, 21, 3, generator=g) * torch.exp(6.0 * torch.randn(9, 21, 1, generator=g))       # ~ 1e-8 .. 1e8
    x[0, 0] = 0.0
    x[1, 1] = torch.tensor([0.0, 1.0, 255.9 / 256.0])
    x[2, 2] = torch.tensor([0.999999, 0.5, 0.25])                         # the largest channel rounds up to 256 / 256
    return x


def test_hdr_round_trip(tmp_path):
    x = _hdr_picture()
    E.save_hdr(tmp_path / "a.hdr", x)
    y = E.load_hdr(tmp_path / "a.hdr")
    assert y.dtype == torch.float32 and y.shape == x.shape
    bound = x.max(-1, keepdim=True).values.double() * 2.0 ** -8
    assert bool(((y.double() - x.double()).abs() <= bound).all())
    assert torch.equal(y[0, 0], torch.zeros(3))


def _rle_scanline(row):
    """one new-style scanline of rgbe bytes [W,4], built by hand: per channel plane runs (128 + n, value) of equal bytes of length
    >= 3 and literal spans (n, bytes...) otherwise, both at most 127 / 128 long"""
    W = row.shape[0]
    out = bytearray([2, 2, W >> 8, W & 255])
    for c in range(4):
        plane = row[:, c].tolist()
        x = 0
        while x < W:
            run = 1
            while x + run < W and run < 127 and plane[x + run] == plane[x]:
                run += 1
            if run >= 3:
                out += bytes([128 + run, plane[x]])
                x += run
                continue
            start = x
            while x < W and x - start < 128:
                run = 1
                while x + run < W and run < 3 and plane[x + run] == plane[x]:
                    run += 1
                if run >= 3:
                    break
                x += 1
            out += bytes([x - start] + plane[start:x])
    return bytes(out)


def test_hdr_run_length_scanlines_decode_to_the_flat_form(tmp_path):
    rng = np.random.default_rng(3)
    H, W = 5, 40
    rgbe = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    rgbe[:, 5:17] = rgbe[:, 5:6]                                          # long runs in every plane
    rgbe[1, :, 3] = 130                                                   # a whole-row run
    rgbe[2, 20:23, 0] = 9                                                 # a run of exactly three
    rgbe[3, :, :] = 0                                                     # black: exponent 0
    head = b"#?RADIANCE\n# a comment\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n" + f"-Y {H} +X {W}\n".encode()
    (tmp_path / "flat.hdr").write_bytes(head + rgbe.tobytes())
    (tmp_path / "rle.hdr").write_bytes(head + b"".join(_rle_scanline(rgbe[y]) for y in range(H)))
    mixed = b"".join(_rle_scanline(rgbe[y]) if y % 2 else rgbe[y].tobytes() for y in range(H))
    if any(rgbe[y, 0, 0] == 2 and rgbe[y, 0, 1] == 2 for y in range(0, H, 2)):
        pytest.fail("the random flat rows must not look like a run-length header")
    (tmp_path / "mixed.hdr").write_bytes(head + mixed)
    flat, rle, mix = (E.load_hdr(tmp_path / n) for n in ("flat.hdr", "rle.hdr", "mixed.hdr"))
    assert len((tmp_path / "rle.hdr").read_bytes()) < len((tmp_path / "flat.hdr").read_bytes())
    assert torch.equal(flat, rle) and torch.equal(flat, mix)
    want = rgbe[..., :3].astype(np.float64) * np.where(rgbe[..., 3:] > 0, 2.0 ** (rgbe[..., 3:].astype(np.float64) - 136.0), 0.0)
    assert np.array_equal(flat.numpy().astype(np.float64), want.astype(np.float32).astype(np.float64))
    assert float(flat[3].abs().max()) == 0.0


def test_hdr_reader_refuses_what_it_cannot_read(tmp_path):
    (tmp_path / "a.hdr").write_bytes(b"P6\n1 1\n255\n\0\0\0")
    with pytest.raises(ValueError, match="Radiance"):
        E.load_hdr(tmp_path / "a.hdr")
    (tmp_path / "b.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 2\n" + bytes(8))
    with pytest.raises(ValueError, match="truncated"):
        E.load_hdr(tmp_path / "b.hdr")
    (tmp_path / "c.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 2 +X 2\n" + bytes(16))
    with pytest.raises(ValueError, match="orientation"):
        E.load_hdr(tmp_path / "c.hdr")


def test_ops_refuse_cpu_tensors_and_bad_shapes_before_the_device():
    from geosplatting_amd._lib import GeoSplatHipError
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        E.cube_to_latlng(torch.rand(6, 4, 4, 3), 8, 4)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        E.latlng_to_cube(torch.rand(4, 8, 3), 4)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        E.sample_cubemap(torch.rand(6, 4, 4, 3), torch.rand(5, 3))
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        E.EnvCubeMap(torch.rand(6, 4, 4, 3)).as_latlng(8, 4)
    from geosplatting_amd import _lib
    lib = _lib.lib()
    assert lib.gs_env_cube_to_latlng_fwd(4, 1, 8, None, None, None, None) == -1 and b"at least 2" in lib.gs_last_error()
    assert lib.gs_env_cube_to_latlng_bwd(4097, 4, 8, None, None, None, None) == -1 and b"bad R" in lib.gs_last_error()
    assert lib.gs_env_latlng_to_cube_fwd(4, 8, 0, None, None, None) == -1
    assert lib.gs_env_latlng_to_cube_bwd(4, 8, 4, None, None, None) == -1 and b"null" in lib.gs_last_error()
    assert lib.gs_cube_sample_linear_bwd(0, 4, None, 1.0, None, None, None) == 0
    assert lib.gs_cube_sample_linear_bwd(5, 4, None, 1.0, None, None, None) == -1
    assert lib.gs_env_background_fwd(4, 8, 8, None, 0.0, 1.0, 4.0, 4.0, None, None, 1, None, None) == -1
