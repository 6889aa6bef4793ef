"""What the stage-3 tests share: the error budget of the light's (hue, value) round trip and a small export dictionary built by hand."""
import torch

U = 2.0 ** -24                      # float32 unit round-off


def light_budget(L64: torch.Tensor) -> torch.Tensor:
    """Relative float32 error budget of hue * exp(value) around its exact value L (L + 1.00001) / (L + 1), to first order in u:
        hue   = fl(L / fl(L + 1))                       two roundings                                         2 u
        s     = fl(L + fl32(1.00001))                   the constant's rounding (weight <= 1) and the sum's   2 u
        value = fl(log s)                               d log = relative error of s: 2 u absolute, plus the function's error, one
                                                        ulp of the result = 2 u |v|
        e     = fl(exp(value))                          relative error = absolute error of value, 2 u + 2 u |v|, plus one ulp, 2 u
        hue * e                                         one rounding                                          1 u
    in all (7 + 2 |v|) u with v = log(L + 1.00001).  log and exp are taken as faithful to one ulp, which the CPU's vectorised
    routines and the device's math library both document."""
    v = (L64 + 1.00001).log().abs()
    return (7.0 + 2.0 * v) * U


def check_light_round_trip(L: torch.Tensor, got: torch.Tensor) -> float:
    """asserts the round trip of a float32 light L -> got = hue * exp(value); returns the largest error in units of the budget"""
    L64, got64 = L.double().cpu(), got.double().cpu()
    want = L64 * (L64 + 1.00001) / (L64 + 1)
    budget = light_budget(L64)
    worst = float(((got64 - want).abs() / (budget * want)).max())
    assert worst <= 1.0, worst
    # the statement of the parametrisation itself: L is reproduced to 1e-5 / (L + 1) relative, plus the rounding above
    assert bool(((got64 - L64).abs() <= L64 * 1e-5 / (L64 + 1) + budget * want).all())
    return worst


def sample_light(seed: int = 0, shape=(16, 32, 3)) -> torch.Tensor:
    """a seeded light in [0.01, 0.6) with a bright patch of about 20 and a texel at the floor of stage 2's clamp"""
    g = torch.Generator().manual_seed(seed)
    L = torch.rand(*shape, generator=g) * 0.5 + 0.1
    L[3:6, 8:12] += 20.0
    L[0, 0] = 0.01
    return L


def hand_export(n: int = 12, seed: int = 0, log2_hashmap_size: int = 4) -> dict:
    """the keys of `PriorModel.export_model` with n Gaussians on one triangle, built on the CPU (no kernel runs)"""
    from geosplatting_amd.field import HashEncoding
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    enc = HashEncoding([-1, 32, 2], activation="none", max_res=4096, log2_hashmap_size=log2_hashmap_size, grad_scaling=16.0,
                       device="cpu", seed=seed)
    return {"geom_scale": 1.0, "min_roughness": 0.1, "max_metallic": 0.9, "exposure": torch.tensor([0.25]), "latlng": sample_light(seed),
            "means": r(n, 3) - 0.5, "scales": r(n, 3) - 4.0, "quats": r(n, 4), "opacities": r(n, 1), "normals": r(n, 3) - 0.5,
            "kd": r(n, 3), "ks": r(n, 2), "occ": torch.randn(n, 6, generator=g), "ks_enc": enc.state_dict(), "occ_enc": {},
            "mc_positions": r(n, 3) - 0.5, "mc_vertices": torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]),
            "mc_indices": torch.tensor([[0, 1, 2]], dtype=torch.int32), "initial_guess": torch.tensor([0.0, -3.0])}
