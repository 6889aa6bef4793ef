"""Derive the marching-cubes triangle table of csrc/gs_tsdf.hip and write csrc/gs_mc_table.h.

    python scripts/make_mc_table.py            # rewrites geosplatting_amd/csrc/gs_mc_table.h
    python scripts/make_mc_table.py --check    # exit 1 when the committed header differs

Nothing here is a remembered table: every entry follows from the rule below, and tests/test_fusion_cpu.py checks the
properties that make it a valid one (closed loops over exactly the sign-changing edges, watertight across cubes, outward normals).

Conventions (shared with the kernel and tests/tsdf_ref.py)
  corner k of a cube sits at offset (k & 1, (k >> 1) & 1, (k >> 2) & 1): bit 0 -> axis 0
  edge  e = 4 * axis + j joins EDGE_CORNERS[e] = (lo, hi), hi = lo | (1 << axis); j counts the four lower ends in ascending order
  case  c: bit k set <=> corner k is inside (tsdf < 0)

Rule
  Each of the six faces lists its four corners counter-clockwise as seen from outside the cube.  Every maximal cyclic run of inside
  corners on a face contributes one directed segment, from the edge where the run ends (inside -> outside) to the edge where the
  run starts (outside -> inside).  A face with two diagonal inside corners therefore always separates them, and since the rule sees
  only the face's four signs, the cube on the other side draws the same two segments.  An active edge lies on two faces that
  traverse it in opposite directions, so it has exactly one outgoing and one incoming segment: following the segments gives closed
  loops.  Each loop is fan-triangulated from its smallest edge id whose fan has no diagonal lying in a face of the cube; loops are
  ordered by their smallest edge id.  (A loop that crosses an ambiguous face twice has edges that share that face without being
  joined by a segment; a fan diagonal between two of them lies IN the face, where the neighbouring cube -- same four signs -- may
  draw it again: a half-edge used twice.  With the plain smallest id 18 of the 256 cases have such a diagonal; every loop has a
  root without one.)  The global winding is fixed on the one-inside-corner case: the normal points away from the inside corner
  (toward positive tsdf).
"""
from __future__ import annotations

import os
import sys
from collections import Counter
from typing import Dict, List, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "geosplatting_amd", "csrc", "gs_mc_table.h")

MAX_TRIS = 5


def corner_offset(k: int) -> Tuple[int, int, int]:
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1)


def _edge_corners() -> List[Tuple[int, int]]:
    out = []
    for axis in range(3):
        out += [(lo, lo | (1 << axis)) for lo in range(8) if not lo & (1 << axis)]
    return out


EDGE_CORNERS = _edge_corners()                                  # 12 x (lo, hi)
EDGE_AXIS = [e // 4 for e in range(12)]
_EDGE_OF = {frozenset(c): e for e, c in enumerate(EDGE_CORNERS)}


def _faces() -> List[Tuple[int, int, int, int]]:
    """Corner cycles, counter-clockwise seen from outside: (b, c) = the axes after `a` in cyclic order, so e_b x e_c = e_a and the
    cycle (0,0) (1,0) (1,1) (0,1) in (b, c) turns about +a -- the outward normal of the side at 1; the side at 0 takes the reverse."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            cyc = [(side << a) | (x << b) | (y << c) for x, y in ((0, 0), (1, 0), (1, 1), (0, 1))]
            out.append(tuple(cyc if side == 1 else cyc[::-1]))
    return out


FACES = _faces()


def face_segments(case: int) -> List[Tuple[int, int]]:
    """Directed segments (edge from, edge to) of one case over the six faces."""
    segs = []
    for cyc in FACES:
        inside = [(case >> k) & 1 for k in cyc]
        if sum(inside) in (0, 4):
            continue
        for i in range(4):
            if inside[i] and not inside[i - 1]:                 # a run starts at i (outside -> inside across the edge (i-1, i))
                j = i
                while inside[(j + 1) % 4]:
                    j += 1
                start = _EDGE_OF[frozenset((cyc[i - 1], cyc[i]))]
                end = _EDGE_OF[frozenset((cyc[j % 4], cyc[(j + 1) % 4]))]
                segs.append((end, start))
    return segs


def case_loops(case: int) -> List[List[int]]:
    """Closed loops of edge ids, each rotated to start at its smallest id, ordered by that id."""
    nxt: Dict[int, int] = {}
    for a, b in face_segments(case):
        assert a not in nxt, "an active edge has exactly one outgoing segment"
        nxt[a] = b
    assert sorted(nxt) == sorted(set(nxt.values()))
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop, cur = [], e
        while cur not in seen:
            seen.add(cur)
            loop.append(cur)
            cur = nxt[cur]
        assert cur == e
        loops.append(loop)                                      # starts at its smallest id: edges are visited in ascending order
    return loops


def _edge_mid(e: int) -> Tuple[float, float, float]:
    lo, hi = EDGE_CORNERS[e]
    a, b = corner_offset(lo), corner_offset(hi)
    return tuple(0.5 * (x + y) for x, y in zip(a, b))


def _normal(tri) -> Tuple[float, float, float]:
    p, q, r = (_edge_mid(e) for e in tri)
    u = [q[i] - p[i] for i in range(3)]
    v = [r[i] - p[i] for i in range(3)]
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _edge_faces(e: int) -> frozenset:
    lo, hi = EDGE_CORNERS[e]
    return frozenset(i for i, cyc in enumerate(FACES) if lo in cyc and hi in cyc)


def in_face_diagonals(loop: List[int]) -> List[Tuple[int, int]]:
    """Diagonals of the fan from loop[0] whose two edges share a face of the cube"""
    return [(loop[0], loop[k]) for k in range(2, len(loop) - 1) if _edge_faces(loop[0]) & _edge_faces(loop[k])]


def fan_root(loop: List[int]) -> List[int]:
    """The loop rotated to start at its smallest edge id whose fan has no diagonal in a face"""
    for e in sorted(loop):
        r = loop.index(e)
        rot = loop[r:] + loop[:r]
        if not in_face_diagonals(rot):
            return rot
    raise AssertionError("no fan root without an in-face diagonal: %r" % (loop,))


def _fan(loops: List[List[int]], flip: bool) -> List[Tuple[int, int, int]]:
    tris = []
    for loop in map(fan_root, loops):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i + 1], loop[i]) if flip else (loop[0], loop[i], loop[i + 1]))
    return tris


def _needs_flip() -> bool:
    """Case 1 (corner 0 inside, at the origin): the normal of its single triangle must point away from the origin."""
    (tri,) = _fan(case_loops(1), False)
    n, m = _normal(tri), _edge_mid(tri[0])
    d = sum(n[i] * m[i] for i in range(3))
    assert d != 0
    return d < 0


def build_table() -> List[List[Tuple[int, int, int]]]:
    flip = _needs_flip()
    return [_fan(case_loops(c), flip) for c in range(256)]


def table_stats(table) -> dict:
    hist = Counter(len(t) for t in table)
    return {"cases": len(table), "max_tris": max(hist), "total_tris": sum(len(t) for t in table),
            "hist": dict(sorted(hist.items())), "longest_loop": max((len(l) for c in range(256) for l in case_loops(c)), default=0)}


def render_header(table) -> str:
    st = table_stats(table)
    lines = [
        "// gs_mc_table.h -- marching-cubes triangle table of gs_tsdf.hip.  GENERATED by scripts/make_mc_table.py: do not edit.",
        "// Corner k at offset (k & 1, (k >> 1) & 1, (k >> 2) & 1); edge e = 4 * axis + j joins corner lo = GS_MC_EDGE_LO[e] and",
        "// lo | (1 << axis); case bit k set <=> corner k inside (tsdf < 0).  Normals point toward positive tsdf.",
        "// %d cases, %d triangles, at most %d per case, histogram %s, longest loop %d." % (
            st["cases"], st["total_tris"], st["max_tris"], st["hist"], st["longest_loop"]),
        "#pragma once",
        "",
        "#define GS_MC_MAX_TRIS %d" % MAX_TRIS,
        "",
        "// lower-end corner of every edge",
        "static __constant__ unsigned char GS_MC_EDGE_LO[12] = {%s};" % ", ".join(str(lo) for lo, _ in EDGE_CORNERS),
        "",
        "// triangles per case",
        "static __constant__ unsigned char GS_MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines += ["};", "", "// edge ids of the triangles of every case, three per triangle, -1 padded",
              "static __constant__ signed char GS_MC_TRI[256][%d] = {" % (3 * MAX_TRIS)]
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        lines.append("    {%s},  // %d" % (", ".join("%2d" % e for e in flat), c))
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv) -> int:
    text = render_header(build_table())
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("up to date" if same else "STALE: %s" % HEADER)
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER, table_stats(build_table()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
