"""No-GPU check of the SH restatement the GPU tests measure against (tests/test_gpu_gsplat_modes.py): gsplat's polynomial
("fast") form of the real SH basis equals the classic 3DGS ``eval_sh`` form (coefficients C0..C3) on unit vectors, degrees 0..3,
in float64 -- the two formulations pin each other's constants and signs."""
import numpy as np
import pytest
import torch

from tests.test_gpu_gsplat_modes import sh_basis_fast, sh_colors64

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def eval_sh_classic(deg, sh, dirs):
    """3DGS's eval_sh: sh [..., 3, (deg+1)^2], dirs unit [..., 3]."""
    result = C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        result = result - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3]
        if deg > 1:
            xx, yy, zz = x * x, y * y, z * z
            xy, yz, xz = x * y, y * z, x * z
            result = (result + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
                      + C2[3] * xz * sh[..., 7] + C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                result = (result + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10]
                          + C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
                          + C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + C3[5] * z * (xx - yy) * sh[..., 14]
                          + C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return result


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_fast_form_equals_classic_eval_sh(deg):
    g = torch.Generator().manual_seed(deg)
    n, nb = 4096, (deg + 1) ** 2
    dirs = torch.randn(n, 3, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    coeffs = torch.randn(n, 16, 3, generator=g, dtype=torch.float64)
    fast = (sh_basis_fast(deg, dirs)[..., None] * coeffs[:, :nb]).sum(-2)
    classic = eval_sh_classic(deg, coeffs[:, :nb].transpose(1, 2), dirs)
    assert fast.shape == classic.shape == (n, 3)
    assert float((fast - classic).abs().max()) < 1e-12
    # the GPU tests' helper (unnormalised directions from a camera position, K = 16 rows of which (deg+1)^2 count)
    campos = torch.tensor([0.3, -0.2, 2.0], dtype=torch.float64)
    means = campos + dirs * torch.rand(n, 1, generator=g, dtype=torch.float64).add(0.5)
    assert float((sh_colors64(deg, means, campos, coeffs) - classic).abs().max()) < 1e-12


def test_basis_is_orthonormal():
    """Monte-Carlo check of the normalisation: E[b_i b_j] over the sphere = delta_ij / (4 pi)."""
    g = torch.Generator().manual_seed(7)
    d = torch.randn(400000, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    b = sh_basis_fast(3, d)
    gram = (b.T @ b / d.shape[0] * 4 * np.pi).numpy()
    assert np.abs(gram - np.eye(16)).max() < 0.02
