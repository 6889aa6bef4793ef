"""No-GPU checks of the antialias restatement tests/meshaa_ref.py: hand-checked cases, the dictionary-built edge topology, and the
condition on the GPU tests' perspective scenes (the share of fragile pairs), computed from the restatement alone with the float64
rasterizer of tests/meshraster_ref.py standing in for the device's rast.

The first hand case.  A vertical edge at x = 10.25 cuts pixel column 10, which covers [10, 11) with its centre at 10.5.
  * Square on the LEFT of the edge: rast leaves column 10 empty, the square covers a quarter of it.  a = column 9, s = +1,
    x* = 10.25 - 9.5 = 0.75, d = 0.75 > 0.5: out[10] += 0.25 (1 - 0).  alpha = 1, 0.25, 0 in columns 9, 10, 11.
  * Square on the RIGHT: rast covers column 10, three quarters of which lie in the square.  a = column 10, s = -1,
    x* = 10.25 - 10.5 = -0.25, d = 0.25 < 0.5: out[10] += 0.25 (0 - 1).  alpha = 0, 0.75, 1 in columns 9, 10, 11.
An empty pixel receives d - 0.5 <= 0.5, so the figure 0.75 belongs to the covered column; both orientations are asserted.
"""
import numpy as np
import pytest
import torch

from tests import meshaa_ref as aa
from tests import meshraster_ref as ref

FRAGILE_CAP = 0.10
PERSPECTIVE = [(8, 16), (12, 24)]                                                 # the scenes of tests/test_gpu_meshaa.py


def _alpha(vc, faces, size, cull="none"):
    intr = aa.UNIT + size
    vc = np.asarray(vc, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64)
    res = ref.rasterize(vc, faces, intr, cull=cull)
    rast = aa.rast_of(res)
    pairs = aa.analyse(rast, vc, faces, intr, cull=cull)
    color = torch.as_tensor((res["face"] >= 0).astype(np.float64))[..., None]
    out = aa.blend(pairs, color, torch.as_tensor(vc, dtype=torch.float64)[pairs["verts"]], intr)
    return out["out"][..., 0].numpy(), pairs, res


def _square(x0, x1):
    return aa._at([(x0, 2), (x1, 2), (x1, 20), (x0, 20)], 1.0), [(0, 1, 2), (0, 2, 3)]


def test_vertical_edge_at_10_25():
    alpha, pairs, res = _alpha(*_square(2.0, 10.25), (24, 16))
    assert np.all(res["face"][2:20, 9] >= 0) and np.all(res["face"][2:20, 10] < 0)
    # (rows 18 and 19: the centre of column 9 lies in the lower-left triangle, whose exit edge is the diagonal, an interior edge)
    assert np.array_equal(alpha[2:18, 9:12], np.tile([1.0, 0.25, 0.0], (16, 1)))
    assert np.all(alpha[18:20, 10] == 0.0)
    alpha, pairs, res = _alpha(*_square(10.25, 14.5), (24, 16))
    assert np.all(res["face"][2:20, 9] < 0) and np.all(res["face"][2:20, 10] >= 0)
    assert np.array_equal(alpha[3:20, 9:12], np.tile([0.0, 0.75, 1.0], (17, 1)))
    # the right edge at 14.5 passes through the centres of column 14, which the fill rule leaves empty: half of it is covered
    # (down to row 15, where the diagonal crosses column 13)
    assert np.array_equal(alpha[2:15, 13:16], np.tile([1.0, 0.5, 0.0], (13, 1)))


def test_interior_edge_blends_nothing():
    alpha, pairs, res = _alpha(*_square(2.0, 14.0), (24, 16))
    inside = res["face"] >= 0
    assert len(np.unique(res["face"][inside])) == 2                               # the diagonal separates the two face ids
    assert np.all(alpha[inside] == 1.0) and np.all(alpha[~inside] == 0.0)         # all edges on pixel boundaries: d = 0.5 everywhere
    assert pairs["n"] > 0 and set(np.unique(res["face"].ravel()[pairs["a"]])) <= {0, 1}
    assert np.all(res["face"].ravel()[pairs["b"]] < 0), "a pair across the diagonal was blended"


def test_open_boundary_blends_and_shared_edge_does_not():
    vc = aa._at([(3.3, 3.2), (10.6, 3.4), (17.7, 3.1), (3.4, 12.7), (10.4, 12.6), (17.6, 12.8)], 1.0)
    faces = [(0, 1, 4), (0, 4, 3), (1, 2, 5), (1, 5, 4)]
    alpha, pairs, res = _alpha(vc, faces, (16, 22))
    assert pairs["n"] > 20 and np.all(res["face"].ravel()[pairs["b"]] < 0)                                      # only the outline blends
    assert np.all((alpha[3:13, 3] > 0) & (alpha[3:13, 3] < 1))                    # left boundary at x ~ 3.3: column 3 partly covered
    assert np.all(alpha[4:12, 5:16] == 1.0)                                       # across the shared edge and the diagonals: untouched


def test_folded_crease_blends():
    # two faces on the edge x = 10.25, both to its left in screen space: the second lies behind the first
    vc = np.concatenate((aa._at([(10.25, 2), (10.25, 20), (2, 11)], 1.0), aa._at([(4, 11)], 2.0)), 0)
    faces = [(0, 1, 2), (1, 0, 3)]
    alpha, pairs, res = _alpha(vc, faces, (24, 16))
    assert aa.topology(faces)[2] == [(1, 2)]                                      # edge 2 of face 0 (vertices 0, 1) is shared
    assert np.all(res["face"][8:14, 9] == 0) and np.all(res["face"][8:14, 10] < 0)
    assert np.array_equal(alpha[8:14, 9:12], np.tile([1.0, 0.25, 0.0], (6, 1)))
    # unfolded, the second face on the right of the edge: an interior edge, nothing blends across it
    vc[3] = aa._at([(15, 11)], 1.0)[0]
    alpha, pairs, res = _alpha(vc, faces, (24, 16))
    assert np.all(alpha[10:12, 8:12] == 1.0)


def _consistent(topo, faces):
    for h, group in enumerate(topo):
        f, i = divmod(h, 3)
        key = {int(faces[f][(i + 1) % 3]), int(faces[f][(i + 2) % 3])}
        for f2, i2 in group:
            assert f2 != f and {int(faces[f2][(i2 + 1) % 3]), int(faces[f2][(i2 + 2) % 3])} == key
            assert (f, i) in topo[3 * f2 + i2]


def test_dictionary_topology():
    _, faces = ref.uv_sphere(8, 16)
    topo = aa.topology(faces)
    assert len(topo) == 3 * faces.shape[0] and all(len(g) == 1 for g in topo)     # closed and manifold
    _consistent(topo, faces)
    fan = np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4), (2, 1, 5)])                   # edge (0, 1) on three faces
    topo = aa.topology(fan)
    assert topo[2] == [(1, 2), (2, 2)] and topo[5] == [(0, 2), (2, 2)] and topo[8] == [(0, 2), (1, 2)]
    assert topo[0] == [(3, 2)] and topo[1] == [] and topo[11] == [(0, 0)]
    _consistent(topo, fan)
    assert aa.topology([(0, 0, 1), (0, 1, 2)])[:3] == [[(1, 2)], [(1, 2)], []]     # a repeated index: the edge (0, 0) is no edge


@pytest.mark.parametrize("lat_long", PERSPECTIVE, ids=lambda t: f"sphere{t[0]}x{t[1]}")
def test_fragile_share_of_the_perspective_scenes(lat_long):
    sc = ref.scene(*lat_long)
    res = ref.rasterize(sc["vc"], sc["faces"], sc["intr"])
    pairs = aa.analyse(aa.rast_of(res), sc["vc"], sc["faces"], sc["intr"], pixel_fragile=res["fragile"])
    share = pairs["fragile"].mean()
    print(f"{lat_long}: {pairs['n']} blended pairs, fragile share {share:.4f}, largest kappa {pairs['kappa'].max():.1f}")
    assert pairs["n"] > 100
    assert share <= FRAGILE_CAP


def test_exact_scenes_blend():
    for name, (vc, faces) in aa.exact_scenes().items():
        alpha, pairs, res = _alpha(vc, faces, (64, 64))
        d = aa.blend(pairs, torch.zeros(64, 64, 1, dtype=torch.float64), torch.as_tensor(vc, dtype=torch.float64)[pairs["verts"]],
                     aa.UNIT + (64, 64))["d"].numpy()
        off = np.abs(d - 0.5)
        print(f"{name}: {pairs['n']} pairs, {(off == 0).sum()} at d = 0.5, the nearest other {off[off > 0].min():.4f}")
        assert off[off > 0].min() > 1e-3, name
        on = off == 0
        assert np.all(np.asarray(vc)[pairs["verts"][on]] * 4 % 1 == 0), name     # exactly 0.5 only between dyadic positions
        assert pairs["n"] > 20, name
        assert np.all(np.isfinite(pairs["kappa"])), name
        edge = (alpha > 0) & (alpha < 1)
        assert edge.sum() > 10 and np.all(alpha >= 0) and np.all(alpha <= 1), name
