"""No-GPU checks of the float64 restatement of the decimation rule (tests/simplify_ref.py), the yardstick of
tests/test_gpu_simplify.py: what the rule does to the small meshes the GPU tests use -- topology kept, placement on the surface, the
link condition, the stall of a mesh that cannot shrink -- and that the per-edge comparison mesh stays clear of every branch threshold.
The figures were measured on this restatement; they are conditions on the inputs of the GPU tests."""
import functools

import numpy as np
import pytest

from tests import simplify_ref as R


@functools.lru_cache(maxsize=None)
def _simplified(name, target):
    v, f = {"icosphere3": lambda: R.icosphere(3), "torus24x12": lambda: R.torus(24, 12), "cube6": lambda: R.cube(6),
            "square8": lambda: R.square(8), "torus4x3": lambda: R.torus(4, 3), "tetrahedron": R.tetrahedron}[name]()
    v2, f2, vmap, info = R.simplify(v, f, target)
    assert R.no_repeats_no_unused(v2, f2) and R.map_is_consistent(f, vmap, f2)
    assert info["rounds"] == len(info["per_round"])
    if not info["stalled"]:
        assert len(f2) in (target - 1, target)
    return v, f, v2, f2, info


def test_meshes_are_what_their_names_say():
    for (v, f), faces, chi, closed in ((R.icosphere(3), 1280, 2, True), (R.torus(24, 12), 576, 0, True), (R.cube(6), 432, 2, True),
                                       (R.square(8), 128, 1, False), (R.torus(6, 3), 36, 0, True), (R.tetrahedron(), 4, 2, True),
                                       (R.strip(7), 7, 1, False)):
        assert len(f) == faces and R.euler(f) == chi and R.is_closed_manifold(f) == closed and R.directed_edges_once(f)
        assert R.no_repeats_no_unused(v, f)
    v, f = R.cube(6)
    assert R.signed_volume(v, f) == pytest.approx(1.0, abs=1e-12) and R.signed_volume(*R.icosphere(3)) > 4.0
    assert R.area(*R.square(8)) == pytest.approx(1.0, abs=1e-12)


def test_sphere_keeps_its_shape():
    _, _, v2, f2, info = _simplified("icosphere3", 320)
    assert len(f2) == 320 and R.is_closed_manifold(f2) and R.euler(f2) == 2 and info["rounds"] == 18 and not info["stalled"]
    radii = np.linalg.norm(v2.astype(np.float64), axis=1)
    print(f"radii [{radii.min():.4f}, {radii.max():.4f}]")
    assert 1.0025 <= radii.min() and radii.max() <= 1.0106            # optimal placement lands outside the sphere, midpoints inside
    centroid = np.linalg.norm(v2.astype(np.float64)[f2].mean(1), axis=1).min()
    v0, f0 = R.icosphere(2)
    regular = np.linalg.norm(v0.astype(np.float64)[f0].mean(1), axis=1).min()
    print(f"smallest centroid radius {centroid:.4f}, icosphere(2) {regular:.4f}, inward deviation ratio {(1 - centroid) / (1 - regular):.3f}")
    assert abs(centroid - 0.9805) < 1e-4 and abs(regular - 0.9822) < 1e-4
    assert R.signed_volume(v2, f2) > 0


def test_torus_keeps_its_genus():
    _, _, v2, f2, info = _simplified("torus24x12", 144)
    assert len(f2) == 144 and R.euler(f2) == 0 and R.is_closed_manifold(f2) and not info["stalled"]


@pytest.mark.parametrize("target", [48, 12])
def test_cube_stays_a_cube(target):
    _, _, v2, f2, info = _simplified("cube6", target)
    assert len(f2) == target and R.is_closed_manifold(f2) and R.euler(f2) == 2
    assert R.signed_volume(v2, f2) == 1.0
    assert float(np.abs(np.abs(v2.astype(np.float64) - 0.5).max(axis=1) - 0.5).max()) == 0.0       # every vertex on the surface
    if target == 12:
        assert len(v2) == 8 and bool(((v2 == 0) | (v2 == 1)).all())   # the corners


def test_flat_square_keeps_its_border():
    _, _, v2, f2, _ = _simplified("square8", 8)
    assert len(f2) == 8 and R.area(v2, f2) == pytest.approx(1.0, abs=1e-12) and R.euler(f2) == 1
    on_border = ((v2[:, :2] == 0) | (v2[:, :2] == 1)).any(axis=1)
    boundary = np.unique([e for e, k in R.edge_faces_count(f2).items() if k == 1])
    assert bool(on_border[boundary].all()) and bool((v2[:, 2] == 0).all())
    corners = {(float(x), float(y)) for x, y, _ in v2 if x in (0, 1) and y in (0, 1)}
    assert corners == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}


def test_link_condition_on_a_three_ring():
    v, f = R.torus(6, 3)
    c = R.edge_costs(v, f, R.initial_quadrics(v, f))
    assert len(c["edges"]) == 54 and int(c["link_fail"].sum()) == 18 and not bool(c["valid"][c["link_fail"]].any())
    ring = {(min(p * 3 + q, p * 3 + (q + 1) % 3), max(p * 3 + q, p * 3 + (q + 1) % 3)) for p in range(6) for q in range(3)}
    assert {tuple(int(x) for x in e) for e in c["edges"][c["link_fail"]]} == ring      # the three edges around the tube, six times


def test_a_mesh_that_cannot_shrink_stalls():
    _, f, v2, f2, info = _simplified("torus4x3", 12)
    assert info["stalled"] and len(f2) == 20 and R.euler(f2) == 0 and info["per_round"][-1][2:] == (0, 0)
    v, f, v2, f2, info = _simplified("tetrahedron", 2)
    assert info["stalled"] and info["rounds"] == 1 and np.array_equal(f2, f) and np.array_equal(v2, v)


def test_per_edge_mesh_is_clear_of_every_threshold():
    """the bumpy icosphere(2) of the per-edge GPU test: no edge near the determinant threshold, the distance limit or min_normal_dot"""
    v, f = R.bumpy_sphere()
    assert v.dtype == np.float32 and len(f) == 320
    c = R.edge_costs(v, f, R.initial_quadrics(v, f))
    det, dist, dot = c["det_ratio"].min() * R.DET_REL, c["dist_ratio"].max(), c["min_dot"].min()
    print(f"smallest |det| / (tr / 3)^3 {det:.2e}, largest |p - mid| / |e| {dist:.3f}, smallest normal dot {dot:.4f}")
    assert len(c["edges"]) == 480 and int(c["near"].sum()) == 0 and bool(c["valid"].all())
    assert abs(det - 4.0e-4) < 0.05e-4 and abs(dist - 0.62) < 0.01 and abs(dot - 0.918) < 0.001
    assert len(np.unique(c["key"] & 0xFFFFFFFF)) == 480 and bool((c["key"] >> 32 == c["cost"].view(np.uint32)).all())


def test_winners_are_independent():
    v, f = R.icosphere(1)
    c = R.edge_costs(v, f, R.initial_quadrics(v, f))
    win, t = R.select_winners(c), c["topology"]
    assert win and [int(c["key"][i]) for i in win] == sorted(int(c["key"][i]) for i in win)
    for i in win:
        closed = set(t.edges[i]) | set(t.nbr[t.edges[i][0]]) | set(t.nbr[t.edges[i][1]])
        assert all(not (set(t.edges[j]) & closed) for j in win if j != i)


def test_union_find_labels():
    v, f = R.strip(5)
    f = np.concatenate((f, R.tetrahedron()[1] + 8))                       # vertex 7 stays unused
    assert R.union_find_labels(f, 12).tolist() == [0] * 7 + [-1] + [8] * 4
