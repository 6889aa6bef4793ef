// gs_simplify.hip -- mesh decimation by rounds of independent quadric edge collapses, and connected components by min-label
// hooking; include/geosplat_hip.h states the rule, geosplatting_amd/meshsimplify.py rebuilds the index arrays every round (sorts).
//
// Quadrics: a thread per vertex gathers its faces' plane quadrics (and the boundary planes of its one-face sides) through the sorted
//   vertex -> face list, in list order: no float atomics, the same bits every time.  10 doubles a vertex, the upper triangle row-major.
// Edge kernel: a thread per unique edge; float64 throughout, contraction off (the 3 x 3 solve cancels, and the float64 restatement in
//   tests/simplify_ref.py must take the same branches).  Its loops are the two sorted neighbour lists (link condition) and the two face
//   lists (duplicate-face and normal tests); every walk is bounded by its offsets.
// Selection: a valid edge takes atomicMin(claim[w], key) for every w of its closed neighbourhood, a second launch reads claim[u] and
//   claim[v].  Keys are unique (an odd multiplier makes the low word a bijection of the edge index), so the minimum does not depend
//   on the order in which the atomics arrive.
// Components: hook (atomicMin of the smaller root into the larger root's parent) and compress, one pair of launches per call; the
//   caller repeats until `changed` stays 0.  parent[x] <= x always holds, so every walk to a root strictly descends and ends; a walk
//   that reads a stale parent ends at an ancestor that is no longer a root, which only costs another iteration.  No kernel waits for
//   another workgroup.
#include "gs_common.h"

#include <math.h>

#define SD_BLOCK 256
#define SD_MAX_ITEMS (1 << 30)
#define SD_HASH 0x9E3779B1u

struct SdVec { double x, y, z; };
__device__ __forceinline__ SdVec sd_load(const float* __restrict__ p, int i)
{
    return {(double)p[3 * (int64_t)i], (double)p[3 * (int64_t)i + 1], (double)p[3 * (int64_t)i + 2]};
}
__device__ __forceinline__ SdVec sd_sub(SdVec a, SdVec b)
{
#pragma clang fp contract(off)
    return {a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ double sd_dot(SdVec a, SdVec b)
{
#pragma clang fp contract(off)
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ SdVec sd_cross(SdVec a, SdVec b)
{
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// q += w (n, d)(n, d)^T
__device__ __forceinline__ void sd_add_plane(double (&q)[10], double w, SdVec n, double d)
{
#pragma clang fp contract(off)
    q[0] += w * (n.x * n.x); q[1] += w * (n.x * n.y); q[2] += w * (n.x * n.z); q[3] += w * (n.x * d);
    q[4] += w * (n.y * n.y); q[5] += w * (n.y * n.z); q[6] += w * (n.y * d);
    q[7] += w * (n.z * n.z); q[8] += w * (n.z * d);
    q[9] += w * (d * d);
}

// the plane of the side (pa, pb) of a face with unit normal n: through the side, perpendicular to the face
__device__ __forceinline__ void sd_add_boundary(double (&q)[10], double weight, SdVec pa, SdVec pb, SdVec n)
{
#pragma clang fp contract(off)
    const SdVec e = sd_sub(pb, pa);
    const double e2 = sd_dot(e, e);
    const SdVec m = sd_cross(e, n);
    const double ml = sqrt(sd_dot(m, m));
    if (!(e2 > 0.0) || !(ml > 0.0)) return;
    const SdVec mu = {m.x / ml, m.y / ml, m.z / ml};
    sd_add_plane(q, weight * e2, mu, -sd_dot(mu, pa));
}

__global__ void __launch_bounds__(SD_BLOCK) simplify_quadrics_kernel(int V, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                     const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf,
                                                                     const uint8_t* __restrict__ side_boundary, double boundary_weight,
                                                                     double* __restrict__ quadrics)
{
#pragma clang fp contract(off)
    const int v = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (v >= V) return;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = vf_off[v]; t < vf_off[v + 1]; ++t) {
        const int f = vf[t];
        const int idx[3] = {faces[3 * (int64_t)f], faces[3 * (int64_t)f + 1], faces[3 * (int64_t)f + 2]};
        const SdVec p[3] = {sd_load(vertices, idx[0]), sd_load(vertices, idx[1]), sd_load(vertices, idx[2])};
        const SdVec n = sd_cross(sd_sub(p[1], p[0]), sd_sub(p[2], p[0]));
        const double len = sqrt(sd_dot(n, n));
        if (!(len > 0.0)) continue;                                        // a zero-area face has no plane
        const SdVec nu = {n.x / len, n.y / len, n.z / len};
        sd_add_plane(q, 0.5 * len, nu, -sd_dot(nu, p[0]));
#pragma unroll
        for (int j = 0; j < 3; ++j) {                                      // side j joins corner j and corner j + 1
            const int j1 = j == 2 ? 0 : j + 1;
            if ((idx[j] == v || idx[j1] == v) && side_boundary[3 * (int64_t)f + j]) sd_add_boundary(q, boundary_weight, p[j], p[j1], nu);
        }
    }
#pragma unroll
    for (int c = 0; c < 10; ++c) quadrics[10 * (int64_t)v + c] = q[c];
}

__device__ __forceinline__ double sd_cost(const double (&q)[10], double x, double y, double z)
{
#pragma clang fp contract(off)
    const double c = q[0] * x * x + 2.0 * q[1] * x * y + 2.0 * q[2] * x * z + 2.0 * q[3] * x + q[4] * y * y + 2.0 * q[5] * y * z
                     + 2.0 * q[6] * y + q[7] * z * z + 2.0 * q[8] * z + q[9];
    return c <= 0.0 ? 0.0 : c;                                             // (a NaN stays one: the edge is then not valid)
}

struct SdEdges {
    int V, E;
    const float* vertices;
    const double* quadrics;
    const int32_t *faces, *edges, *edge_faces, *edge_opp, *nbr_off, *nbr, *vf_off, *vf;
    const uint8_t* boundary;
    double min_normal_dot;
    float *position, *cost;
    uint8_t* valid;
    int64_t* key;
};

// the faces of `moved` that do not contain `other`, with `moved` at p: false when one of them turns by more than the bound or
// collapses; `pair` counts the faces that contain both oa and ob (asked for the faces of u only)
__device__ __forceinline__ bool sd_faces_ok(const SdEdges& a, int moved, int other, SdVec p, int oa, int ob, int& pair)
{
#pragma clang fp contract(off)
    bool ok = true;
    for (int t = a.vf_off[moved]; t < a.vf_off[moved + 1]; ++t) {
        const int f = a.vf[t];
        const int i0 = a.faces[3 * (int64_t)f], i1 = a.faces[3 * (int64_t)f + 1], i2 = a.faces[3 * (int64_t)f + 2];
        if (oa >= 0 && (i0 == oa || i1 == oa || i2 == oa) && (i0 == ob || i1 == ob || i2 == ob)) ++pair;
        if (i0 == other || i1 == other || i2 == other) continue;
        const SdVec p0 = sd_load(a.vertices, i0), p1 = sd_load(a.vertices, i1), p2 = sd_load(a.vertices, i2);
        const SdVec n_old = sd_cross(sd_sub(p1, p0), sd_sub(p2, p0));
        const SdVec r0 = i0 == moved ? p : p0, r1 = i1 == moved ? p : p1, r2 = i2 == moved ? p : p2;
        const SdVec n_new = sd_cross(sd_sub(r1, r0), sd_sub(r2, r0));
        const double oo = sd_dot(n_old, n_old), nn = sd_dot(n_new, n_new);
        if (!(nn > 0.0) || !(sd_dot(n_old, n_new) > a.min_normal_dot * (sqrt(oo) * sqrt(nn)))) ok = false;
    }
    return ok;
}

__global__ void __launch_bounds__(SD_BLOCK) simplify_edge_kernel(const SdEdges a)
{
#pragma clang fp contract(off)
    const int i = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (i >= a.E) return;
    const int u = a.edges[2 * (int64_t)i], v = a.edges[2 * (int64_t)i + 1];
    double q[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) q[c] = a.quadrics[10 * (int64_t)u + c] + a.quadrics[10 * (int64_t)v + c];
    const SdVec pu = sd_load(a.vertices, u), pv = sd_load(a.vertices, v);
    const SdVec mid = {0.5 * (pu.x + pv.x), 0.5 * (pu.y + pv.y), 0.5 * (pu.z + pv.z)};
    const SdVec e = sd_sub(pv, pu);
    const double elen = sqrt(sd_dot(e, e));
    // p = A^-1 b through the adjugate of the symmetric A
    const double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[4], a12 = q[5], a22 = q[7];
    const double b0 = -q[3], b1 = -q[6], b2 = -q[8];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double tr3 = (a00 + a11 + a22) / 3.0;
    float px = 0.f, py = 0.f, pz = 0.f;
    bool solved = false;
    if (fabs(det) > 1e-6 * (tr3 * tr3 * tr3)) {
        const SdVec s = {(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det, (c02 * b0 + c12 * b1 + c22 * b2) / det};
        const SdVec d = sd_sub(s, mid);
        if (sqrt(sd_dot(d, d)) <= 2.0 * elen) { solved = true; px = (float)s.x; py = (float)s.y; pz = (float)s.z; }
    }
    if (!solved) {                                                          // the cheapest of u, v, mid; the first on a tie
        const float mx = (float)mid.x, my = (float)mid.y, mz = (float)mid.z;
        const double cu = sd_cost(q, pu.x, pu.y, pu.z), cv = sd_cost(q, pv.x, pv.y, pv.z), cm = sd_cost(q, (double)mx, (double)my, (double)mz);
        px = (float)pu.x; py = (float)pu.y; pz = (float)pu.z;
        double best = cu;
        if (cv < best) { best = cv; px = (float)pv.x; py = (float)pv.y; pz = (float)pv.z; }
        if (cm < best) { px = mx; py = my; pz = mz; }
    }
    const SdVec p = {(double)px, (double)py, (double)pz};
    const float cost = (float)sd_cost(q, p.x, p.y, p.z);
    // validity
    const int k = a.edge_faces[i];
    bool ok = (k == 1 || k == 2) && cost >= 0.0f && cost < INFINITY && isfinite(px) && isfinite(py) && isfinite(pz);
    if (ok) {                                                               // link condition: a merge of the two sorted lists
        int iu = a.nbr_off[u], iv = a.nbr_off[v], common = 0;
        const int eu = a.nbr_off[u + 1], ev = a.nbr_off[v + 1];
        while (iu < eu && iv < ev) {
            const int x = a.nbr[iu], y = a.nbr[iv];
            common += x == y;
            iu += x <= y;
            iv += y <= x;
        }
        ok = common == k;
    }
    if (ok && k == 2 && a.boundary[u] && a.boundary[v]) ok = false;         // an interior edge between two boundary vertices
    if (ok) {
        const int oa = k == 2 ? a.edge_opp[2 * (int64_t)i] : -1, ob = k == 2 ? a.edge_opp[2 * (int64_t)i + 1] : -1;
        int pair = 0, unused = 0;
        ok = sd_faces_ok(a, u, v, p, oa, ob, pair) && pair == 0;
        if (ok) ok = sd_faces_ok(a, v, u, p, -1, -1, unused);
    }
    a.position[3 * (int64_t)i] = px; a.position[3 * (int64_t)i + 1] = py; a.position[3 * (int64_t)i + 2] = pz;
    a.cost[i] = cost;
    a.valid[i] = ok ? 1 : 0;
    a.key[i] = (int64_t)(((uint64_t)__float_as_uint(cost) << 32) | (uint64_t)((uint32_t)i * SD_HASH));
}

__global__ void __launch_bounds__(SD_BLOCK) simplify_fill_kernel(unsigned long long* __restrict__ claim, int V)
{
    const int v = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (v < V) claim[v] = ~0ull;
}

__global__ void __launch_bounds__(SD_BLOCK) simplify_claim_kernel(int E, const int32_t* __restrict__ edges, const uint8_t* __restrict__ valid,
                                                                  const int64_t* __restrict__ key, const int32_t* __restrict__ nbr_off,
                                                                  const int32_t* __restrict__ nbr, unsigned long long* __restrict__ claim)
{
    const int i = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (i >= E || !valid[i]) return;
    const unsigned long long k = (unsigned long long)key[i];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int w = edges[2 * (int64_t)i + side];
        atomicMin(&claim[w], k);
        for (int t = nbr_off[w]; t < nbr_off[w + 1]; ++t) atomicMin(&claim[nbr[t]], k);
    }
}

__global__ void __launch_bounds__(SD_BLOCK) simplify_winner_kernel(int E, const int32_t* __restrict__ edges, const uint8_t* __restrict__ valid,
                                                                   const int64_t* __restrict__ key, const unsigned long long* __restrict__ claim,
                                                                   uint8_t* __restrict__ winner)
{
    const int i = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (i >= E) return;
    const unsigned long long k = (unsigned long long)key[i];
    winner[i] = valid[i] && claim[edges[2 * (int64_t)i]] == k && claim[edges[2 * (int64_t)i + 1]] == k;
}

// the selected edges have disjoint endpoints (no endpoint of one lies in the closed neighbourhood of another): plain stores
__global__ void __launch_bounds__(SD_BLOCK) simplify_apply_kernel(int n, const int64_t* __restrict__ selected, const int32_t* __restrict__ edges,
                                                                  const float* __restrict__ position, float* __restrict__ vertices,
                                                                  double* __restrict__ quadrics, int64_t* __restrict__ remap)
{
    const int t = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (t >= n) return;
    const int64_t i = selected[t];
    const int u = edges[2 * i], v = edges[2 * i + 1];
    remap[v] = u;
#pragma unroll
    for (int c = 0; c < 3; ++c) vertices[3 * (int64_t)u + c] = position[3 * i + c];
#pragma unroll
    for (int c = 0; c < 10; ++c) quadrics[10 * (int64_t)u + c] += quadrics[10 * (int64_t)v + c];
}

// ------------------------------------------------------------------------------------------------ components
__device__ __forceinline__ int sd_root(const int32_t* parent, int x)
{
    // parent[y] <= y, and a root has parent[y] == y: the walk strictly descends.  Relaxed atomic loads: other lanes lower these words.
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p < x) {
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

__global__ void __launch_bounds__(SD_BLOCK) components_hook_kernel(int E, const int32_t* __restrict__ edges, int32_t* parent, int32_t* changed)
{
    const int i = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (i >= E) return;
    const int ru = sd_root(parent, edges[2 * (int64_t)i]), rv = sd_root(parent, edges[2 * (int64_t)i + 1]);
    if (ru == rv) return;
    atomicMin(&parent[ru > rv ? ru : rv], ru < rv ? ru : rv);
    __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(SD_BLOCK) components_compress_kernel(int V, int32_t* parent)
{
    const int v = (int)blockIdx.x * SD_BLOCK + (int)threadIdx.x;
    if (v >= V) return;
    const int r = sd_root(parent, v);
    if (r < v) atomicMin(&parent[v], r);                                    // (never raises a parent another lane has lowered further)
}

// ------------------------------------------------------------------------------------------------ entry points
static const char* sd_check(int V, int64_t n)
{
    if (V < 0 || n < 0) return "negative count";
    if (V > SD_MAX_ITEMS || n > SD_MAX_ITEMS) return "more than 2^30 vertices, faces or edges";
    return nullptr;
}

extern "C" int gs_simplify_quadrics(int V, int F, const float* vertices, const int32_t* faces, const int32_t* vf_off, const int32_t* vf,
                                    const uint8_t* side_boundary, double boundary_weight, double* quadrics, void* stream)
{
    const char* msg = sd_check(V, F);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(boundary_weight >= 0.0 && boundary_weight < INFINITY, "boundary_weight must be finite and >= 0");
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(vertices != nullptr && vf_off != nullptr && quadrics != nullptr, "null vertices, vf_off or quadrics");
    GS_CHECK_ARG(F == 0 || (faces != nullptr && vf != nullptr && side_boundary != nullptr), "null faces, vf or side_boundary");
    hipLaunchKernelGGL(simplify_quadrics_kernel, dim3(gs_cdiv(V, SD_BLOCK)), dim3(SD_BLOCK), 0, (hipStream_t)stream, V, vertices, faces, vf_off, vf,
                       side_boundary, boundary_weight, quadrics);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_simplify_edge_costs(int V, int E, const float* vertices, const double* quadrics, const int32_t* faces, const int32_t* edges,
                                      const int32_t* edge_faces, const int32_t* edge_opp, const int32_t* nbr_off, const int32_t* nbr,
                                      const int32_t* vf_off, const int32_t* vf, const uint8_t* boundary, double min_normal_dot, float* position,
                                      float* cost, uint8_t* valid, int64_t* key, void* stream)
{
    const char* msg = sd_check(V, E);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(min_normal_dot >= -1.0 && min_normal_dot < 1.0, "min_normal_dot must be in [-1, 1)");
    if (E == 0) return GS_OK;
    GS_CHECK_ARG(V > 0, "edges without vertices");
    GS_CHECK_ARG(vertices != nullptr && quadrics != nullptr && faces != nullptr && edges != nullptr && edge_faces != nullptr && edge_opp != nullptr,
                 "null vertices, quadrics, faces, edges, edge_faces or edge_opp");
    GS_CHECK_ARG(nbr_off != nullptr && nbr != nullptr && vf_off != nullptr && vf != nullptr && boundary != nullptr, "null list or boundary flags");
    GS_CHECK_ARG(position != nullptr && cost != nullptr && valid != nullptr && key != nullptr, "null output");
    SdEdges a = {};
    a.V = V; a.E = E; a.vertices = vertices; a.quadrics = quadrics; a.faces = faces; a.edges = edges; a.edge_faces = edge_faces; a.edge_opp = edge_opp;
    a.nbr_off = nbr_off; a.nbr = nbr; a.vf_off = vf_off; a.vf = vf; a.boundary = boundary; a.min_normal_dot = min_normal_dot;
    a.position = position; a.cost = cost; a.valid = valid; a.key = key;
    hipLaunchKernelGGL(simplify_edge_kernel, dim3(gs_cdiv(E, SD_BLOCK)), dim3(SD_BLOCK), 0, (hipStream_t)stream, a);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_simplify_select(int V, int E, const int32_t* edges, const uint8_t* valid, const int64_t* key, const int32_t* nbr_off,
                                  const int32_t* nbr, uint64_t* claim, uint8_t* winner, void* stream)
{
    const char* msg = sd_check(V, E);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    if (E == 0) return GS_OK;
    GS_CHECK_ARG(V > 0, "edges without vertices");
    GS_CHECK_ARG(edges != nullptr && valid != nullptr && key != nullptr && nbr_off != nullptr && nbr != nullptr, "null edges, valid, key or list");
    GS_CHECK_ARG(claim != nullptr && winner != nullptr, "null claim or winner");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* c = (unsigned long long*)claim;
    hipLaunchKernelGGL(simplify_fill_kernel, dim3(gs_cdiv(V, SD_BLOCK)), dim3(SD_BLOCK), 0, s, c, V);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(simplify_claim_kernel, dim3(gs_cdiv(E, SD_BLOCK)), dim3(SD_BLOCK), 0, s, E, edges, valid, key, nbr_off, nbr, c);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(simplify_winner_kernel, dim3(gs_cdiv(E, SD_BLOCK)), dim3(SD_BLOCK), 0, s, E, edges, valid, key, (const unsigned long long*)c, winner);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_simplify_apply(int V, int E, int n, const int64_t* selected, const int32_t* edges, const float* position, float* vertices,
                                 double* quadrics, int64_t* remap, void* stream)
{
    const char* msg = sd_check(V, E);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(n >= 0 && n <= E, "more selected edges than edges");
    if (n == 0) return GS_OK;
    GS_CHECK_ARG(selected != nullptr && edges != nullptr && position != nullptr && vertices != nullptr && quadrics != nullptr && remap != nullptr,
                 "null argument");
    hipLaunchKernelGGL(simplify_apply_kernel, dim3(gs_cdiv(n, SD_BLOCK)), dim3(SD_BLOCK), 0, (hipStream_t)stream, n, selected, edges, position, vertices,
                       quadrics, remap);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_components_step(int V, int E, const int32_t* edges, int32_t* parent, int32_t* changed, void* stream)
{
    const char* msg = sd_check(V, E);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(changed != nullptr, "null changed");
    GS_CHECK_ARG(V == 0 || parent != nullptr, "null parent");
    GS_CHECK_ARG(E == 0 || (edges != nullptr && V > 0), "null edges, or edges without vertices");
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(changed, sizeof(int32_t), s));
    if (E > 0) {
        hipLaunchKernelGGL(components_hook_kernel, dim3(gs_cdiv(E, SD_BLOCK)), dim3(SD_BLOCK), 0, s, E, edges, parent, changed);
        GS_CHECK_LAUNCH();
    }
    if (V > 0) {
        hipLaunchKernelGGL(components_compress_kernel, dim3(gs_cdiv(V, SD_BLOCK)), dim3(SD_BLOCK), 0, s, V, parent);
        GS_CHECK_LAUNCH();
    }
    return GS_OK;
}
