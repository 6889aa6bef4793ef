"""No GPU: geosplatting_amd.poseopt (CameraPoseDeltas, rot6d) is plain torch."""
import torch

import geosplatting_amd as gs
from geosplatting_amd.poseopt import CameraPoseDeltas, rot6d


def _cams(n=5):
    return gs.orbit_cameras(n, 3.0, 25.0, 97, 61, hfov_degree=55.0)


def test_zero_deltas_are_the_identity():
    """zero deltas return the pose itself: every non-zero entry to the bit, and IEEE-equal throughout (x * 1 + y * 0 + z * 0 turns a
    -0.0 entry of c2w into +0.0, the one thing a product with the identity matrix cannot keep)"""
    p = CameraPoseDeltas(5)
    assert p.deltas.shape == (5, 9) and not p.deltas.any() and p.deltas.requires_grad
    for i, cam in enumerate(_cams()):
        out = p.apply(cam.c2w, i).detach()
        assert out.shape == (3, 4) and torch.equal(out, cam.c2w)
        nz = cam.c2w != 0
        assert torch.equal(out.view(torch.int32)[nz], cam.c2w.view(torch.int32)[nz])
        cam2 = p.camera(cam, i)
        assert torch.equal(cam2.c2w.detach(), cam.c2w) and torch.equal(cam2.view_matrix.detach(), cam.view_matrix)
        assert (cam2.fx, cam2.fy, cam2.cx, cam2.cy, cam2.width, cam2.height) == (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    c44 = torch.cat((_cams()[2].c2w, torch.tensor([[0.0, 0.0, 0.0, 1.0]])))
    assert torch.equal(p.apply(c44, 2).detach(), c44)
    assert torch.equal(rot6d(p.identity), torch.eye(3))


def test_rot6d_is_a_rotation():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(200, 6, generator=g, dtype=torch.float64) * 3.0
    R = rot6d(a)
    assert R.shape == (200, 3, 3)
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    assert float((torch.linalg.det(R) - 1.0).abs().max()) < 1e-12
    # rows: b1 along a1, b2 in the plane of (a1, a2) on a2's side
    assert float((torch.nn.functional.normalize(a[:, :3], dim=-1) - R[:, 0]).abs().max()) < 1e-12
    assert ((R[:, 1] * a[:, 3:]).sum(-1) > 0).all()
    R32 = rot6d(a.float())
    assert float((R32 @ R32.transpose(-1, -2) - torch.eye(3)).abs().max()) < 1e-5


def test_gradient_at_zero_init():
    """a generic loss on the corrected pose: finite everywhere, non-zero in the six slots that move the pose at zero (three
    translations, a1.y, a1.z, a2.z: the six degrees of freedom), and EXACTLY zero in slots 3, 6 and 7 -- d[3] and d[7] scale
    a1 = (1,0,0) and a2 = (0,1,0) along themselves, which the normalisations of rot6d remove, and d[6] moves a2 along b1, which the
    Gram-Schmidt step removes (the semantics are the definition; 'non-zero in all nine slots' cannot hold at exactly zero, and does
    hold a step away from it, checked below)"""
    g = torch.Generator().manual_seed(1)
    cams = _cams()
    w = torch.randn(5, 3, 4, generator=g)
    p = CameraPoseDeltas(5)
    loss = sum((p.apply(c.c2w, i) * w[i]).sum() for i, c in enumerate(cams))
    loss.backward()
    gr = p.deltas.grad
    assert gr.shape == (5, 9) and torch.isfinite(gr).all()
    live = [0, 1, 2, 4, 5, 8]
    assert (gr[:, live] != 0).all()
    assert not gr[:, [3, 6, 7]].any()
    p.random_init_(1e-2, generator=g)
    p.deltas.grad = None
    sum((p.apply(c.c2w, i) * w[i]).sum() for i, c in enumerate(cams)).backward()
    assert torch.isfinite(p.deltas.grad).all() and (p.deltas.grad != 0).all()
    # through the view matrix as the rasterizer receives it
    p.zero_init_()
    assert not p.deltas.any()
    p.deltas.grad = None
    (p.camera(cams[1], 1).view_matrix * torch.randn(4, 4, generator=g)).sum().backward()
    assert (p.deltas.grad[1, live] != 0).all() and not p.deltas.grad[[0, 2, 3, 4]].any()


def test_batch_equals_per_index():
    g = torch.Generator().manual_seed(2)
    cams = _cams()
    p = CameraPoseDeltas(5).random_init_(0.05, generator=g)
    c2w = torch.stack([c.c2w for c in cams])
    idx = torch.tensor([3, 0, 4, 1, 2])
    out = p.apply(c2w[idx], idx).detach()
    assert out.shape == (5, 3, 4)
    for k, i in enumerate(idx.tolist()):
        one = p.apply(cams[i].c2w, i).detach()
        assert float((out[k] - one).abs().max()) <= 1e-6
        R = one[:, :3]
        assert float((R.T @ R - torch.eye(3)).abs().max()) < 1e-5          # still a rigid pose
    # the correction is camera-local: c2w o delta, translation d[:3] along the camera's own axes
    d = p.deltas.detach()
    assert float((out[0][:, 3] - (cams[3].c2w[:, :3] @ d[3, :3] + cams[3].c2w[:, 3])).abs().max()) < 1e-6


def test_random_init_is_seeded_and_state_roundtrips():
    a = CameraPoseDeltas(4).random_init_(0.1, generator=torch.Generator().manual_seed(7))
    b = CameraPoseDeltas(4).random_init_(0.1, generator=torch.Generator().manual_seed(7))
    assert torch.equal(a.deltas, b.deltas) and 0.02 < float(a.deltas.detach().std()) < 0.3
    c = CameraPoseDeltas(4)
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.deltas, a.deltas) and len(c.parameters()) == 1
