"""No-GPU checks of the near_clip reference (tests/meshclip_ref.py) alone: the clip against an independent area computation, and the
conditions that keep tests/test_gpu_meshclip.py from hiding a failure -- the share of fragile pixels (where that test accepts any
candidate face) is capped, and every scene really exercises crossing faces.

Measured with the reference as committed (fragile share, crossing faces that own a pixel with one / two vertices inside, share of
the pixels on crossing faces, largest clipped polygon among them, sub-triangle edges with a widened band):
    floor16        fragile 0.0137   crossing 6 (2 / 4)   pixels 0.237   4 vertices   widened 0
    floor32        fragile 0.0256   crossing 8 (4 / 4)   pixels 0.213   4 vertices   widened 0
    floor16_37x53  fragile 0.0153   crossing 6 (2 / 4)   pixels 0.123   4 vertices   widened 0
    guard          fragile 0.0134   crossing 7 (2 / 5)   pixels 0.381   5 vertices   widened 6
The clipped areas agree with the vertex enumeration to 8e-13 of the face's area.
"""
import numpy as np
import pytest

from tests import meshclip_ref as clip
from tests import meshraster_ref as ref


def test_classification():
    vc = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 0.05], [1, 0, -2], [np.nan, 0, 1], [0, 0, 0.1]], dtype=np.float32)
    faces = [(0, 1, 2), (0, 1, 3), (0, 3, 4), (3, 4, 3), (0, 1, 5), (0, 3, 5), (0, 1, 9), (0, 1, 6)]
    # all inside; two inside; one inside; none; a NaN with all inside (left to the unclipped code, which drops it); a NaN on a
    # crossing face; an index out of range; Z == near is outside
    assert clip.classify(vc, faces, 0.1).tolist() == [1, 2, 2, 0, 1, 0, 0, 2]


@pytest.mark.parametrize("name", clip.SCENES)
def test_clipped_area_against_vertex_enumeration(name):
    sc = clip.scene(name)
    ex = clip.expand(sc["vc"], sc["faces"], sc["intr"], sc["near"])
    assert len(ex["polys"]) >= 5
    worst, sizes = 0.0, set()
    for f, poly in ex["polys"].items():
        P = sc["vc"][sc["faces"][f]].astype(np.float64)
        got = clip.polygon_area([C for C, _, _ in poly]) if poly else 0.0
        want = clip.area_by_enumeration(P, sc["intr"], sc["near"])
        full = clip.polygon_area(list(P))
        assert 0.0 <= got <= full * (1 + 1e-12)
        worst = max(worst, abs(got - want) / full)
        sizes.add(len(poly))
        # the polygon keeps the face's winding: its area vector points along the face's normal
        if poly:
            n = np.cross(P[1] - P[0], P[2] - P[0])
            total = sum(np.cross(poly[i][0], poly[(i + 1) % len(poly)][0]) for i in range(len(poly)))
            assert float(np.dot(total, n)) > 0
            assert all(C[2] >= sc["near"] * (1 - 1e-12) for C, _, _ in poly)
    print(f"{name}: {len(ex['polys'])} crossing faces, polygon sizes {sorted(sizes)}, largest area difference {worst:.2e} of the face")
    assert worst <= 1e-9


def test_a_shared_edge_is_cut_to_the_same_bits():
    """two crossing faces on an edge with one endpoint inside hold the same cut, bit for bit (no guard plane reaches this scene's cuts)"""
    sc = clip.scene("floor16")
    ex = clip.expand(sc["vc"], sc["faces"], sc["intr"], sc["near"])
    inside = sc["vc"][:, 2] > np.float32(sc["near"])
    cuts = {f: {C.tobytes() for C, tag, _ in poly if tag < 0} for f, poly in ex["polys"].items()}
    owners = {}
    for f in ex["polys"]:
        t = sc["faces"][f]
        for i in range(3):
            a, b = int(t[i]), int(t[(i + 1) % 3])
            if inside[a] != inside[b]:
                owners.setdefault((min(a, b), max(a, b)), []).append(f)
    shared = [v for v in owners.values() if len(v) == 2]
    assert len(shared) >= 5
    assert all(cuts[f] & cuts[g] for f, g in shared)


@pytest.mark.parametrize("name", clip.SCENES)
def test_scene_conditions(name):
    res = clip.scene_result(name)
    st = clip.crossing_stats(res)
    share = float(res["fragile"].mean())
    print(f"{name}: fragile {share:.4f}, crossing faces seen {st['seen']} ({st['one_inside']} with one vertex inside, "
          f"{st['two_inside']} with two), {st['pixel_share']:.3f} of the pixels on them, polygons up to {st['max_vertices']} vertices, "
          f"{res['widened']} widened edges")
    assert share <= clip.FRAGILE_CAP
    assert st["seen"] >= 5 and st["one_inside"] >= 1 and st["two_inside"] >= 1
    assert st["pixel_share"] >= 0.05
    if name == "guard":
        assert st["max_vertices"] >= 5 and res["widened"] >= 1
    # the drop-whole rasterizer loses what near_clip adds: the crossing faces own pixels that are empty or further away without it
    sc = clip.scene(name)
    plain = ref.rasterize(sc["vc"], sc["faces"], sc["intr"], near=sc["near"])
    assert not np.isin(plain["face"], np.flatnonzero(res["kind"] == 2)).any()
    solid = ~res["fragile"] & ~plain["fragile"]
    same = (res["face"] == plain["face"]) | res["crossing"]
    assert same[solid].all()
    assert (res["interior"] & ~res["empty_ok"]).sum() > 0 and not (res["interior"] & (res["face"] < 0) & ~res["fragile"]).any()


def test_values_agree_with_the_perspective_form_in_front_of_the_eye():
    """where every vertex has Z > 0 the ray / plane values are meshraster_ref's perspective-correct ones"""
    sc = ref.scene(8, 16)
    res = ref.rasterize(sc["vc"], sc["faces"], sc["intr"])
    for f in np.unique(res["face"][res["face"] >= 0])[::7]:
        m = res["face"] == f
        b0, b1, d = clip.face_values(sc["vc"][sc["faces"][f]], sc["intr"])
        assert np.allclose(b0[m], res["b0"][m], rtol=0, atol=1e-9) and np.allclose(b1[m], res["b1"][m], rtol=0, atol=1e-9)
        assert np.allclose(d[m], res["depth"][m], rtol=1e-10, atol=0)
