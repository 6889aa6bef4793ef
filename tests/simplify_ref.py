"""Float64 numpy restatement of the decimation rule of geosplatting_amd/meshsimplify.py (include/geosplat_hip.h states it): quadric
error metrics run as rounds of independent edge collapses.  Dicts, sets and loops; nothing here is fast.  It also builds the small
meshes the tests use and holds the mesh checks (Euler characteristic, manifoldness, volume) both test files share.

Per edge it also reports how close the edge is to each branch threshold of the rule (`near`), so that a per-element comparison
can leave out the edges whose branch a rounding error may flip."""
import math

import numpy as np

HASH = 0x9E3779B1
DET_REL = 1e-6
DIST_MAX = 2.0


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(level):
    from geosplatting_amd.synthetic import icosphere as ico
    v, f = ico(level)
    return v.numpy().astype(np.float32), f.numpy().astype(np.int64)


def bumpy_sphere(level=2, seed=1):
    """icosphere(level) with r = 0.8 (1 + 0.08 sin 3a + 0.05 cos(4b + 1) + 0.04 sin 5c); a, b, c the dot products with three seeded
    normal vectors; rounded to fp32"""
    v, f = icosphere(level)
    d = np.random.default_rng(seed).standard_normal((3, 3))
    a, b, c = (v.astype(np.float64) @ d.T).T
    r = 0.8 * (1.0 + 0.08 * np.sin(3 * a) + 0.05 * np.cos(4 * b + 1.0) + 0.04 * np.sin(5 * c))
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), f


def torus(nu, nv, R=1.0, r=0.4):
    """nu segments around the axis, nv around the tube; 2 nu nv faces"""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    v = np.stack(((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)), -1).reshape(-1, 3)
    idx = lambda p, q: (p % nu) * nv + (q % nv)
    f = []
    for p in range(nu):
        for q in range(nv):
            f.append((idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)))
            f.append((idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)))
    return v.astype(np.float32), np.array(f, dtype=np.int64)


def square(n=8):
    """flat open unit square of n x n quads in z = 0; 2 n^2 faces, normal +z"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack((i / n, j / n, np.zeros_like(i, dtype=np.float64)), -1).reshape(-1, 3)
    idx = lambda p, q: p * (n + 1) + q
    f = []
    for p in range(n):
        for q in range(n):
            f.append((idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)))
            f.append((idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)))
    return v.astype(np.float32), np.array(f, dtype=np.int64)


def cube(n=6):
    """welded unit cube [0, 1]^3 of n x n quads a side; 12 n^2 faces, outward normals, the vertices in lexicographic (x, y, z) order"""
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(int(round(c * n)) for c in p)
        if key not in index:
            index[key] = len(verts)
            verts.append([c / n for c in key])
        return index[key]

    for axis in range(3):
        for side in (0, 1):
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            for p in range(n):
                for q in range(n):
                    def pt(dp, dq):
                        c = [0.0, 0.0, 0.0]
                        c[axis], c[a1], c[a2] = float(side), (p + dp) / n, (q + dq) / n
                        return vid(c)
                    quad = [pt(0, 0), pt(1, 0), pt(1, 1), pt(0, 1)]           # counter-clockwise seen from +axis
                    if side == 0:
                        quad = quad[::-1]
                    faces.append((quad[0], quad[1], quad[2]))
                    faces.append((quad[0], quad[2], quad[3]))
    v, f = np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return v[order], rank[f]


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)
    return v, f


def strip(n):
    """open strip of n triangles over n + 2 vertices"""
    v = np.stack((np.arange(n + 2) // 2, np.arange(n + 2) % 2, np.zeros(n + 2)), -1).astype(np.float32)
    f = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n)], dtype=np.int64)
    return v, f


# ------------------------------------------------------------------------------------------------ checks
def edge_faces_count(faces):
    count = {}
    for a, b, c in faces:
        for x, y in ((a, b), (b, c), (c, a)):
            key = (min(x, y), max(x, y))
            count[key] = count.get(key, 0) + 1
    return count


def euler(faces):
    faces = np.asarray(faces)
    return len(np.unique(faces)) - len(edge_faces_count(faces)) + len(faces)


def directed_edges_once(faces):
    seen = set()
    for a, b, c in np.asarray(faces):
        for e in ((a, b), (b, c), (c, a)):
            if e in seen:
                return False
            seen.add(e)
    return True


def is_closed_manifold(faces):
    """every edge has two faces, in opposite directions, and the faces of every vertex form one fan"""
    faces = np.asarray(faces)
    if not directed_edges_once(faces) or any(k != 2 for k in edge_faces_count(faces).values()):
        return False
    ring = {}
    for a, b, c in faces:
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            ring.setdefault(x, {})[y] = z                                    # around x: y -> z
    for x, nxt in ring.items():
        start = next(iter(nxt))
        y, steps = nxt[start], 1
        while y != start and steps <= len(nxt):
            if y not in nxt:
                return False
            y, steps = nxt[y], steps + 1
        if y != start or steps != len(nxt):
            return False
    return True


def no_repeats_no_unused(vertices, faces):
    faces = np.asarray(faces)
    distinct = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
    return bool(distinct.all()) and len(np.unique(faces)) == len(vertices) and faces.min() >= 0 and faces.max() < len(vertices)


def signed_volume(vertices, faces):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def area(vertices, faces):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())


def map_is_consistent(faces_in, vertex_map, faces_out):
    """every input face either maps to an output face's vertex set or is degenerate (under the map)"""
    out = {frozenset(int(x) for x in f) for f in np.asarray(faces_out)}
    for f in np.asarray(faces_in):
        m = [int(vertex_map[x]) for x in f]
        if len(set(m)) < 3:
            continue
        if min(m) < 0 or frozenset(m) not in out:
            return False
    return True


def canonical_faces(faces):
    """each face rotated to start at its smallest index, the faces sorted"""
    f = np.asarray(faces)
    k = f.argmin(axis=1)
    r = np.stack([f[np.arange(len(f)), (k + j) % 3] for j in range(3)], 1)
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


def union_find_labels(faces, num_vertices):
    parent = list(range(num_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    used = np.zeros(num_vertices, dtype=bool)
    for a, b, c in np.asarray(faces):
        used[[a, b, c]] = True
        for x, y in ((a, b), (b, c)):
            rx, ry = find(int(x)), find(int(y))
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(x) if used[x] else -1 for x in range(num_vertices)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the rule
class Topology:
    """edges ascending by lo V + hi (the position is the edge index), k faces per edge, the opposite vertices, sorted neighbour
    lists, vertex -> face lists and boundary-vertex flags"""

    def __init__(self, faces, V):
        sides = {}
        for fi, (a, b, c) in enumerate(faces):
            for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
                sides.setdefault((min(x, y), max(x, y)), []).append((fi, int(z)))
        self.edges = sorted(sides, key=lambda e: e[0] * V + e[1])
        self.k = [len(sides[e]) for e in self.edges]
        self.opp = [[z for _, z in sides[e]] for e in self.edges]
        self.edge_face = [[fi for fi, _ in sides[e]] for e in self.edges]
        nbr = [set() for _ in range(V)]
        for u, v in self.edges:
            nbr[u].add(v)
            nbr[v].add(u)
        self.nbr = [sorted(s) for s in nbr]
        self.vf = [[] for _ in range(V)]
        for fi, f in enumerate(faces):
            for x in f:
                self.vf[x].append(fi)
        self.boundary = np.zeros(V, dtype=bool)
        for (u, v), k in zip(self.edges, self.k):
            if k == 1:
                self.boundary[u] = self.boundary[v] = True


def _dot(a, b):
    """in this order and without fused multiply-adds, as the kernel adds it (numpy's dot may not)"""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def plane_quadric(w, n, d):
    h = np.array([n[0], n[1], n[2], d])
    return w * np.outer(h, h)


def initial_quadrics(vertices, faces, boundary_weight=1000.0):
    """[V,4,4] float64: area-weighted face planes plus the boundary planes of one-face edges"""
    P = np.asarray(vertices, dtype=np.float64)
    Q = np.zeros((len(P), 4, 4))
    count = edge_faces_count(faces)
    for a, b, c in faces:
        n = np.cross(P[b] - P[a], P[c] - P[a])
        length = math.sqrt(_dot(n, n))
        if not length > 0.0:
            continue
        n = n / length
        K = plane_quadric(0.5 * length, n, -_dot(n, P[a]))
        for x in (a, b, c):
            Q[x] += K
        for x, y in ((a, b), (b, c), (c, a)):
            if count[(min(x, y), max(x, y))] != 1:
                continue
            e = P[y] - P[x]
            m = np.cross(e, n)
            ml = math.sqrt(_dot(m, m))
            if not (_dot(e, e) > 0.0 and ml > 0.0):
                continue
            m = m / ml
            K = plane_quadric(boundary_weight * _dot(e, e), m, -_dot(m, P[x]))
            Q[x] += K
            Q[y] += K
    return Q


def _cost(Q, p):
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    c = (Q[0, 0] * x * x + 2.0 * Q[0, 1] * x * y + 2.0 * Q[0, 2] * x * z + 2.0 * Q[0, 3] * x + Q[1, 1] * y * y + 2.0 * Q[1, 2] * y * z
         + 2.0 * Q[1, 3] * y + Q[2, 2] * z * z + 2.0 * Q[2, 3] * z + Q[3, 3])
    return 0.0 if c <= 0.0 else c


def _f32(p):
    return np.asarray(p, dtype=np.float64).astype(np.float32).astype(np.float64)


def edge_costs(vertices, faces, Q, min_normal_dot=0.2, topo=None):
    """-> dict of per-edge arrays: edges [E,2], cost [E] f32, position [E,3] f32, valid [E] bool, key [E] int64, k [E],
    budget [E] = |h|^T |Q| |h|, link_fail [E] bool, near [E] bool (an edge within a factor 2 of the determinant threshold, within
    1 % of the distance limit or within 1e-3 of min_normal_dot), and the three margins that decide `near`."""
    P = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    V = len(P)
    t = topo or Topology(faces, V)
    E = len(t.edges)
    out = dict(edges=np.array(t.edges, dtype=np.int32).reshape(E, 2), cost=np.zeros(E, np.float32), position=np.zeros((E, 3), np.float32),
               valid=np.zeros(E, bool), key=np.zeros(E, np.int64), k=np.array(t.k, dtype=np.int32), budget=np.zeros(E),
               link_fail=np.zeros(E, bool), near=np.zeros(E, bool), det_ratio=np.full(E, np.inf), dist_ratio=np.zeros(E),
               min_dot=np.full(E, np.inf))
    for i, (u, v) in enumerate(t.edges):
        Qe = Q[u] + Q[v]
        pu, pv = P[u], P[v]
        mid = 0.5 * (pu + pv)
        e = pv - pu
        elen = math.sqrt(_dot(e, e))
        a00, a01, a02, a11, a12, a22 = Qe[0, 0], Qe[0, 1], Qe[0, 2], Qe[1, 1], Qe[1, 2], Qe[2, 2]
        b0, b1, b2 = -Qe[0, 3], -Qe[1, 3], -Qe[2, 3]
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = a00 * c00 + a01 * c01 + a02 * c02
        tr3 = (a00 + a11 + a22) / 3.0
        thr = DET_REL * (tr3 * tr3 * tr3)
        near = False
        if thr > 0.0:
            out["det_ratio"][i] = abs(det) / thr
            near |= 0.5 < abs(det) / thr < 2.0
        p = None
        if abs(det) > thr:
            s = np.array([(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det, (c02 * b0 + c12 * b1 + c22 * b2) / det])
            d = s - mid
            dist = math.sqrt(_dot(d, d))
            if elen > 0.0:
                out["dist_ratio"][i] = dist / elen
                near |= abs(dist / elen - DIST_MAX) <= 0.01 * DIST_MAX
            if dist <= DIST_MAX * elen:
                p = _f32(s)
        if p is None:
            cands = [pu, pv, _f32(mid)]
            costs = [_cost(Qe, c) for c in cands]
            best = 0
            for j in (1, 2):
                if costs[j] < costs[best]:
                    best = j
            p = cands[best]
        cost = np.float32(_cost(Qe, p))
        h = np.array([abs(p[0]), abs(p[1]), abs(p[2]), 1.0])
        out["budget"][i] = h @ np.abs(Qe) @ h
        out["position"][i] = p.astype(np.float32)
        out["cost"][i] = cost
        out["key"][i] = (int(cost.view(np.uint32)) << 32) | ((i * HASH) & 0xFFFFFFFF)
        k = t.k[i]
        ok = k in (1, 2) and bool(np.isfinite(cost)) and bool(np.isfinite(p).all())
        common = len(set(t.nbr[u]) & set(t.nbr[v]))
        out["link_fail"][i] = k in (1, 2) and common != k
        ok = ok and common == k
        if k == 2 and t.boundary[u] and t.boundary[v]:
            ok = False
        if ok and k == 2:
            oa, ob = t.opp[i]
            if any(oa in faces[fi] and ob in faces[fi] for fi in t.vf[u]):
                ok = False
        if ok:
            for moved, other in ((u, v), (v, u)):
                for fi in t.vf[moved]:
                    f = faces[fi]
                    if other in f:
                        continue
                    p0, p1, p2 = P[f[0]], P[f[1]], P[f[2]]
                    n_old = np.cross(p1 - p0, p2 - p0)
                    r0, r1, r2 = [p if x == moved else P[x] for x in f]
                    n_new = np.cross(r1 - r0, r2 - r0)
                    oo, nn = _dot(n_old, n_old), _dot(n_new, n_new)
                    scale = math.sqrt(oo) * math.sqrt(nn)
                    dot = _dot(n_old, n_new)
                    if scale > 0.0:
                        out["min_dot"][i] = min(out["min_dot"][i], dot / scale)
                        near |= abs(dot / scale - min_normal_dot) <= 1e-3
                    if not nn > 0.0 or not dot > min_normal_dot * scale:
                        ok = False
        out["valid"][i] = ok
        out["near"][i] = near
    out["topology"] = t
    return out


def select_winners(c):
    """edge indices that hold the smallest key over their closed neighbourhood's claims at both endpoints, ascending by key"""
    t = c["topology"]
    claim = {}
    for i in np.nonzero(c["valid"])[0]:
        u, v = t.edges[i]
        key = int(c["key"][i])
        for w in {u, v} | set(t.nbr[u]) | set(t.nbr[v]):
            if key < claim.get(w, 1 << 64):
                claim[w] = key
    win = [int(i) for i in np.nonzero(c["valid"])[0]
           if claim[t.edges[i][0]] == int(c["key"][i]) and claim[t.edges[i][1]] == int(c["key"][i])]
    return sorted(win, key=lambda i: int(c["key"][i]))


def simplify(vertices, faces, target_faces, boundary_weight=1000.0, min_normal_dot=0.2, max_rounds=4096):
    """-> (vertices' [V',3] f32, faces' [F',3] int64, vertex_map [V_in] int64, info)"""
    P = np.array(vertices, dtype=np.float32)
    faces = np.array(faces, dtype=np.int64)
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
    V = len(P)
    Q = initial_quadrics(P, faces, boundary_weight)
    rep = np.arange(V)
    info = dict(rounds=0, stalled=False, per_round=[])
    while len(faces) > target_faces and info["rounds"] < max_rounds:
        c = edge_costs(P, faces, Q, min_normal_dot)
        win = select_winners(c)
        info["rounds"] += 1
        if not win:
            info["stalled"] = True
            info["per_round"].append((len(c["edges"]), int(c["valid"].sum()), 0, 0))
            break
        budget, used, applied = len(faces) - target_faces, 0, []
        for i in win:
            if used + c["k"][i] > budget:
                break
            applied.append(i)
            used += int(c["k"][i])
        if not applied:
            applied = [win[0]]
        info["per_round"].append((len(c["edges"]), int(c["valid"].sum()), len(win), len(applied)))
        remap = np.arange(V)
        for i in applied:
            u, v = c["edges"][i]
            remap[v] = u
            P[u] = c["position"][i]
            Q[u] = Q[u] + Q[v]
        rep = remap[rep]
        faces = remap[faces]
        faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
    used = np.zeros(V, dtype=bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    vertex_map = np.where(used[rep], new[rep], -1).astype(np.int64)
    return P[used], new[faces].astype(np.int64), vertex_map, info
