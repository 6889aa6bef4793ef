// gs_meshreg.hip -- the mesh-prior regularisers (uniform Laplacian, edge length, normal consistency) on a topology built once;
// include/geosplat_hip.h states the semantics, geosplatting_amd/meshreg.py builds the index arrays.
//
// Forward: one launch over the V + E + P items, a thread each; it writes the item's term, what the backward gathers (the unit
// Laplacian vector of a vertex, the four vertex gradients of a pair) and adds the term to its workgroup's three double sums (a fixed
// butterfly over the wave, the four waves in order).  A one-workgroup pass adds the workgroups' sums, again in a fixed order, and
// divides.  Backward: one launch over the vertices; a vertex gathers its gradient through its neighbour list (Laplacian and edge
// terms: the neighbours of a vertex are its edges) and its list of (pair, role) codes.  No atomics anywhere, so the same inputs give
// the same bits.  A vertex whose lists are longer than MR_LONG (a fan's centre) is skipped by its thread and walked by a whole wave, 64
// entries a trip: both launches carry ceil(NL / 4) extra workgroups for the NL such vertices.
#include "gs_common.h"

#include <math.h>

#define MR_BLOCK 256
#define MR_WAVES (MR_BLOCK / GS_WAVE)
#define MR_LONG 64
#define MR_EPS 1e-8f
#define MR_MAX_ITEMS (1 << 30)

struct MrVec { float x, y, z; };
__device__ __forceinline__ MrVec mr_load(const float* __restrict__ p, int i) { return {p[3 * (int64_t)i], p[3 * (int64_t)i + 1], p[3 * (int64_t)i + 2]}; }
__device__ __forceinline__ void mr_store(float* __restrict__ p, int64_t i, MrVec v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ MrVec operator+(MrVec a, MrVec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ MrVec operator-(MrVec a, MrVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ MrVec operator*(float s, MrVec a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float mr_dot(MrVec a, MrVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// (no contraction: with an FMA the cross product of two equal vectors -- a face with two coincident vertices -- is the rounding error
//  of a product instead of 0, and that residue would be normalised into a direction)
__device__ __forceinline__ MrVec mr_cross(MrVec a, MrVec b)
{
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ MrVec mr_wave_sum(MrVec v) { return {gs_wave_sum(v.x), gs_wave_sum(v.y), gs_wave_sum(v.z)}; }

__device__ __forceinline__ bool mr_is_long(const int32_t* __restrict__ nbr_off, const int32_t* __restrict__ pr_off, int v)
{
    return nbr_off[v + 1] - nbr_off[v] > MR_LONG || pr_off[v + 1] - pr_off[v] > MR_LONG;
}

// the Laplacian term of a vertex from d = sum_j (v - v_j) = deg v - sum_j v_j: summed as differences of neighbouring positions, which
// are nearly exact, where deg v - sum v_j cancels most of its digits on a smooth mesh (and d / |d| is what the backward gathers)
__device__ __forceinline__ float mr_lap_term(MrVec d, MrVec& dir)
{
    const float len = sqrtf(mr_dot(d, d));
    dir = len > 0.0f ? (1.0f / len) * d : MrVec{0.f, 0.f, 0.f};
    return len;
}

// d (1 - cos) / d n of one normal: -(m - cos nh) / |n| with m the other side's unit vector (already negated), under the clamps
__device__ __forceinline__ MrVec mr_cos_grad(MrVec n, float len, float c, MrVec other, float c_other, float s)
{
    // cos = s / (c c_other), s = n . other; d cos / d n = other / (c c_other) - s / (c^2 c_other) d c / d n, d c / d n = n / len where len >= eps
    const float inv = 1.0f / (c * c_other);
    MrVec g = inv * other;
    if (len >= MR_EPS) g = g - (s * inv / (c * len)) * n;
    return {-g.x, -g.y, -g.z};
}

struct MrFwd {
    int V, E, P, NL, item_blocks;
    const float* vertices;
    const int32_t *edges, *pairs, *nbr_off, *nbr, *pr_off, *long_verts;
    float target_length;
    float *terms, *lap_dir, *pair_grad;
    double* partials;
};

__global__ void __launch_bounds__(MR_BLOCK) meshreg_fwd_kernel(const MrFwd a)
{
    __shared__ double s_part[MR_WAVES][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double part[3] = {0.0, 0.0, 0.0};
    if ((int)blockIdx.x < a.item_blocks) {
        const int i = (int)blockIdx.x * MR_BLOCK + tid;
        if (i < a.V) {
            if (!mr_is_long(a.nbr_off, a.pr_off, i)) {
                const int b = a.nbr_off[i], e = a.nbr_off[i + 1];
                const MrVec v = mr_load(a.vertices, i);
                MrVec sum = {0.f, 0.f, 0.f};
                for (int k = b; k < e; ++k) sum = sum + (v - mr_load(a.vertices, a.nbr[k]));
                MrVec dir;
                const float t = mr_lap_term(sum, dir);
                a.terms[i] = t;
                if (a.lap_dir) mr_store(a.lap_dir, i, dir);
                part[0] = (double)t;
            }
        } else if (i < a.V + a.E) {
            const int e = i - a.V;
            const MrVec d = mr_load(a.vertices, a.edges[2 * e]) - mr_load(a.vertices, a.edges[2 * e + 1]);
            const float r = sqrtf(mr_dot(d, d)) - a.target_length, t = r * r;
            a.terms[i] = t;
            part[1] = (double)t;
        } else if (i < a.V + a.E + a.P) {
            const int p = i - a.V - a.E;
            const int4 q = ((const int4*)a.pairs)[p];
            const MrVec v0 = mr_load(a.vertices, q.x);
            const MrVec e = mr_load(a.vertices, q.y) - v0, pa = mr_load(a.vertices, q.z) - v0, pb = mr_load(a.vertices, q.w) - v0;
            const MrVec n0 = mr_cross(e, pa), n1 = mr_cross(e, pb), m1 = {-n1.x, -n1.y, -n1.z};
            const float l0 = sqrtf(mr_dot(n0, n0)), l1 = sqrtf(mr_dot(n1, n1)), c0 = fmaxf(l0, MR_EPS), c1 = fmaxf(l1, MR_EPS);
            const float s = mr_dot(n0, m1), t = 1.0f - s / (c0 * c1);
            a.terms[i] = t;
            part[2] = (double)t;
            if (a.pair_grad) {
                const MrVec g0 = mr_cos_grad(n0, l0, c0, m1, c1, s);                    // d t / d n0
                const MrVec h = mr_cos_grad(m1, l1, c1, n0, c0, s), g1 = {-h.x, -h.y, -h.z};   // d t / d n1 (through m1 = -n1)
                // n0 = e x pa: d e += pa x g0, d pa = g0 x e; likewise n1 = e x pb
                const MrVec ge = mr_cross(pa, g0) + mr_cross(pb, g1), ga = mr_cross(g0, e), gb = mr_cross(g1, e);
                const MrVec gv0 = {-(ge.x + ga.x + gb.x), -(ge.y + ga.y + gb.y), -(ge.z + ga.z + gb.z)};
                const int64_t o = 4 * (int64_t)p;
                mr_store(a.pair_grad, o, gv0); mr_store(a.pair_grad, o + 1, ge); mr_store(a.pair_grad, o + 2, ga); mr_store(a.pair_grad, o + 3, gb);
            }
        }
    } else {
        const int w = ((int)blockIdx.x - a.item_blocks) * MR_WAVES + wave;      // wave-uniform
        if (w < a.NL) {
            const int i = a.long_verts[w], b = a.nbr_off[i], e = a.nbr_off[i + 1];
            const MrVec v = mr_load(a.vertices, i);
            MrVec sum = {0.f, 0.f, 0.f};
            for (int k = b + lane; k < e; k += GS_WAVE) sum = sum + (v - mr_load(a.vertices, a.nbr[k]));
            sum = mr_wave_sum(sum);
            MrVec dir;
            const float t = mr_lap_term(sum, dir);
            if (lane == 0) {
                a.terms[i] = t;
                if (a.lap_dir) mr_store(a.lap_dir, i, dir);
                part[0] = (double)t;
            }
        }
    }
    // the workgroup's three sums: xor butterfly inside each wave, then the waves in order
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part[c] += __shfl_xor(part[c], off, GS_WAVE);
    }
    if (lane == 0) { s_part[wave][0] = part[0]; s_part[wave][1] = part[1]; s_part[wave][2] = part[2]; }
    __syncthreads();
    if (tid < 3) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < MR_WAVES; ++w) t += s_part[w][tid];
        a.partials[3 * (int64_t)blockIdx.x + tid] = t;
    }
}

// out[c] = sum over the rows of partials[:, c] / count[c]: a thread takes every MR_BLOCK-th row, then the same butterfly
__global__ void __launch_bounds__(MR_BLOCK) meshreg_final_kernel(const double* __restrict__ partials, int rows, int V, int E, int P,
                                                                 float* __restrict__ out)
{
    __shared__ double s_part[MR_WAVES][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double part[3] = {0.0, 0.0, 0.0};
    for (int r = tid; r < rows; r += MR_BLOCK) {
        part[0] += partials[3 * (int64_t)r]; part[1] += partials[3 * (int64_t)r + 1]; part[2] += partials[3 * (int64_t)r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part[c] += __shfl_xor(part[c], off, GS_WAVE);
    }
    if (lane == 0) { s_part[wave][0] = part[0]; s_part[wave][1] = part[1]; s_part[wave][2] = part[2]; }
    __syncthreads();
    if (tid < 3) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < MR_WAVES; ++w) t += s_part[w][tid];
        const int n = tid == 0 ? V : tid == 1 ? E : P;
        out[tid] = n > 0 ? (float)(t / (double)n) : 0.0f;
    }
}

struct MrBwd {
    int V, E, P, NL, item_blocks;
    const float* vertices;
    const int32_t *nbr_off, *nbr, *pr_off, *pr, *long_verts;
    float target_length;
    const float *lap_dir, *pair_grad, *out_grad;
    float* grad;
};

// what the neighbour k of the vertex (v, dir) adds: (its unit Laplacian vector, the edge term's gradient at the vertex)
__device__ __forceinline__ void mr_bwd_neighbour(const MrBwd& a, int j, MrVec v, MrVec& lap, MrVec& edge)
{
    lap = lap + mr_load(a.lap_dir, j);
    const MrVec d = v - mr_load(a.vertices, j);
    const float len = sqrtf(mr_dot(d, d));
    if (len > 0.0f) edge = edge + (2.0f * (len - a.target_length) / len) * d;
}

__device__ __forceinline__ void mr_bwd_store(const MrBwd& a, int i, int deg, MrVec lap, MrVec edge, MrVec nc)
{
    const float cl = a.out_grad[0] / (float)a.V, ce = a.E > 0 ? a.out_grad[1] / (float)a.E : 0.0f, cn = a.P > 0 ? a.out_grad[2] / (float)a.P : 0.0f;
    const MrVec gl = (float)deg * mr_load(a.lap_dir, i) - lap;
    mr_store(a.grad, i, cl * gl + ce * edge + cn * nc);
}

__global__ void __launch_bounds__(MR_BLOCK) meshreg_bwd_kernel(const MrBwd a)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    MrVec lap = {0.f, 0.f, 0.f}, edge = lap, nc = lap;
    if ((int)blockIdx.x < a.item_blocks) {
        const int i = (int)blockIdx.x * MR_BLOCK + tid;
        if (i >= a.V || mr_is_long(a.nbr_off, a.pr_off, i)) return;
        const MrVec v = mr_load(a.vertices, i);
        const int b = a.nbr_off[i], e = a.nbr_off[i + 1];
        for (int k = b; k < e; ++k) mr_bwd_neighbour(a, a.nbr[k], v, lap, edge);
        for (int k = a.pr_off[i]; k < a.pr_off[i + 1]; ++k) nc = nc + mr_load(a.pair_grad, a.pr[k]);
        mr_bwd_store(a, i, e - b, lap, edge, nc);
    } else {
        const int w = ((int)blockIdx.x - a.item_blocks) * MR_WAVES + wave;      // wave-uniform
        if (w >= a.NL) return;
        const int i = a.long_verts[w];
        const MrVec v = mr_load(a.vertices, i);
        const int b = a.nbr_off[i], e = a.nbr_off[i + 1];
        for (int k = b + lane; k < e; k += GS_WAVE) mr_bwd_neighbour(a, a.nbr[k], v, lap, edge);
        for (int k = a.pr_off[i] + lane; k < a.pr_off[i + 1]; k += GS_WAVE) nc = nc + mr_load(a.pair_grad, a.pr[k]);
        lap = mr_wave_sum(lap); edge = mr_wave_sum(edge); nc = mr_wave_sum(nc);
        if (lane == 0) mr_bwd_store(a, i, e - b, lap, edge, nc);
    }
}

static const char* mr_check(int V, int E, int P, int NL)
{
    if (V < 0 || E < 0 || P < 0 || NL < 0) return "negative count";
    if ((int64_t)V + E + P > MR_MAX_ITEMS || 4 * (int64_t)P > MR_MAX_ITEMS) return "V + E + P and 4 P must not exceed 2^30";
    if (NL > V) return "more long vertices than vertices";
    return nullptr;
}

extern "C" int gs_meshreg_partial_rows(int V, int E, int P, int NL)
{
    if (mr_check(V, E, P, NL)) return 0;
    return gs_cdiv((int64_t)V + E + P, MR_BLOCK) + gs_cdiv(NL, MR_WAVES);
}

extern "C" int gs_meshreg_fwd(int V, int E, int P, int NL, const float* vertices, const int32_t* edges, const int32_t* pairs, const int32_t* nbr_off,
                              const int32_t* nbr, const int32_t* pr_off, const int32_t* long_verts, float target_length, float* terms, float* lap_dir,
                              float* pair_grad, double* partials, float* out, void* stream)
{
    const char* msg = mr_check(V, E, P, NL);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(out != nullptr, "null output");
    GS_CHECK_ARG(V == 0 || (vertices != nullptr && nbr_off != nullptr && pr_off != nullptr), "null vertices, nbr_off or pr_off");
    GS_CHECK_ARG(E == 0 || (edges != nullptr && nbr != nullptr), "null edges or nbr");
    GS_CHECK_ARG(P == 0 || pairs != nullptr, "null pairs");
    GS_CHECK_ARG(NL == 0 || long_verts != nullptr, "null long_verts");
    GS_CHECK_ARG((lap_dir == nullptr) == (pair_grad == nullptr) || V == 0 || P == 0, "lap_dir and pair_grad: both or none");
    MrFwd a = {};
    a.V = V; a.E = E; a.P = P; a.NL = NL; a.item_blocks = gs_cdiv((int64_t)V + E + P, MR_BLOCK);
    a.vertices = vertices; a.edges = edges; a.pairs = pairs; a.nbr_off = nbr_off; a.nbr = nbr; a.pr_off = pr_off; a.long_verts = long_verts;
    a.target_length = target_length; a.terms = terms; a.lap_dir = lap_dir; a.pair_grad = pair_grad; a.partials = partials;
    const int rows = a.item_blocks + gs_cdiv(NL, MR_WAVES);
    GS_CHECK_ARG(rows == 0 || (terms != nullptr && partials != nullptr), "null terms or partials");
    hipStream_t s = (hipStream_t)stream;
    if (rows > 0) {
        hipLaunchKernelGGL(meshreg_fwd_kernel, dim3(rows), dim3(MR_BLOCK), 0, s, a);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(meshreg_final_kernel, dim3(1), dim3(MR_BLOCK), 0, s, (const double*)partials, rows, V, E, P, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_meshreg_bwd(int V, int E, int P, int NL, const float* vertices, const int32_t* nbr_off, const int32_t* nbr, const int32_t* pr_off,
                              const int32_t* pr, const int32_t* long_verts, float target_length, const float* lap_dir, const float* pair_grad,
                              const float* out_grad, float* grad, void* stream)
{
    const char* msg = mr_check(V, E, P, NL);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(vertices != nullptr && nbr_off != nullptr && pr_off != nullptr && lap_dir != nullptr, "null vertices, nbr_off, pr_off or lap_dir");
    GS_CHECK_ARG(E == 0 || nbr != nullptr, "null nbr");
    GS_CHECK_ARG(P == 0 || (pr != nullptr && pair_grad != nullptr), "null pr or pair_grad");
    GS_CHECK_ARG(NL == 0 || long_verts != nullptr, "null long_verts");
    GS_CHECK_ARG(out_grad != nullptr && grad != nullptr, "null out_grad or grad");
    MrBwd a = {};
    a.V = V; a.E = E; a.P = P; a.NL = NL; a.item_blocks = gs_cdiv(V, MR_BLOCK);
    a.vertices = vertices; a.nbr_off = nbr_off; a.nbr = nbr; a.pr_off = pr_off; a.pr = pr; a.long_verts = long_verts;
    a.target_length = target_length; a.lap_dir = lap_dir; a.pair_grad = pair_grad; a.out_grad = out_grad; a.grad = grad;
    hipLaunchKernelGGL(meshreg_bwd_kernel, dim3(a.item_blocks + gs_cdiv(NL, MR_WAVES)), dim3(MR_BLOCK), 0, (hipStream_t)stream, a);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
