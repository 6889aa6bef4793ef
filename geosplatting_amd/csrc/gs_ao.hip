// gs_ao.hip -- the ambient-occlusion map of the mesh shaders, on the ray routines of gs_bvh_dev.h:
//   gs_ray_ao   cosine-weighted visibility of points towards a shared set of target points: what TriangleMesh.compute_ambient_occlusion
//               (rfstudio/graphics/_mesh/_triangle_mesh.py:616-678) computes per face from 128 depth-peeled views, restated with one
//               shadow segment per (point, target) -- the cameras of the reference become the targets
// The semantics are stated sample by sample in include/geosplat_hip.h; tests/ao_ref.py restates them in float64.
//
// A group of G lanes (1, 16 or 64) owns one point, as envshade_kernel has it: lane l takes the targets k = l, l + G, ...
// and adds them in ascending k; the group is folded with a fixed xor butterfly and one lane stores: no atomics, the same bits every
// run.  The targets are staged once per block in LDS (12 bytes each, at most 48 KB).  Every lane of a block runs every iteration, so
// the shuffles see 64 active lanes.
#include "gs_bvh_dev.h"

// Contraction OFF for the whole file: every value here feeds a comparison (c > 0) or a sum whose bits the tests pin.
#pragma clang fp contract(off)

#define AO_BLOCK 256
#define AO_MAX_TARGETS 4096

struct AoArgs {
    long long V, F;
    const float* vertices;
    const int* faces;
    const BvhNode* nodes;
    long long P;
    const float *pos, *nrm, *targets;
    int S;
    float offset;
    float* vis;
    unsigned char* log_hit;
    float* log_w;
};

template <int G>
__device__ __forceinline__ float ao_group_sum(float v)                                           // fixed order: the same bits every run
{
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool BRUTE>
__device__ __forceinline__ bool ao_segment_hit(const AoArgs& a, const BvhRay& r)
{
    if (!BRUTE) return bvh_any_hit(r, a.V, a.F, a.vertices, a.faces, a.nodes, 0.0f, 1.0f);
    for (long long f = 0; f < a.F; ++f) {
        BvhTri tr;
        float t, b1, b2;
        if (bvh_load_tri(a.vertices, a.faces, a.V, f, tr) && bvh_tri_test(r, tr, 0.0f, 1.0f, t, b1, b2)) return true;
    }
    return false;
}

template <int G, bool BRUTE, bool LOG>
static __global__ void __launch_bounds__(AO_BLOCK) ray_ao_kernel(const AoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_targets[];
    for (int i = threadIdx.x; i < 3 * a.S; i += AO_BLOCK) s_targets[i] = a.targets[i];
    __syncthreads();
    const int sub = (int)threadIdx.x & (G - 1);
    const long long p = ((long long)blockIdx.x * AO_BLOCK + threadIdx.x) / G;
    const bool in_range = p < a.P;
    const long long pc = in_range ? p : 0;
    const float px = a.pos[3 * pc], py = a.pos[3 * pc + 1], pz = a.pos[3 * pc + 2];
    const float nx = a.nrm[3 * pc], ny = a.nrm[3 * pc + 1], nz = a.nrm[3 * pc + 2];
    const bool live = in_range && bvh_finite(px) && bvh_finite(py) && bvh_finite(pz) && bvh_finite(nx) && bvh_finite(ny) && bvh_finite(nz);
    const float ox = px + nx * a.offset, oy = py + ny * a.offset, oz = pz + nz * a.offset;
    float num = 0.0f, den = 0.0f;
    const int iters = (a.S + G - 1) / G;
    for (int it = 0; it < iters; ++it) {
        const int k = it * G + sub;
        if (!(live && k < a.S)) continue;                      // (no wave-wide operation inside the loop)
        const float dx = s_targets[3 * k] - ox, dy = s_targets[3 * k + 1] - oy, dz = s_targets[3 * k + 2] - oz;
        const float c = ((nx * dx + ny * dy) + nz * dz) / sqrtf((dx * dx + dy * dy) + dz * dz);
        const bool counts = c > 0.0f;                           // (a NaN, from a target at the origin itself, does not count)
        const float w = counts ? fmaxf(c, 1e-4f) : 0.0f;
        bool hit = false;
        if (counts || LOG) {
            const BvhRay r = bvh_make_ray(ox, oy, oz, dx, dy, dz);
            if (r.valid) hit = ao_segment_hit<BRUTE>(a, r);
        }
        if (counts) {
            if (!hit) num += w;
            den += w;
        }
        if (LOG) { a.log_hit[p * a.S + k] = hit ? 1 : 0; a.log_w[p * a.S + k] = w; }
    }
    num = ao_group_sum<G>(num);
    den = ao_group_sum<G>(den);
    if (in_range && sub == 0) a.vis[p] = live ? num / fmaxf(den, 1e-6f) : 0.0f;
}

template <int G, bool BRUTE>
static void ao_launch_g(const AoArgs& a, bool log, hipStream_t s)
{
    const dim3 grid(gs_cdiv(a.P, AO_BLOCK / G)), block(AO_BLOCK);
    const size_t lds = (size_t)a.S * 3 * sizeof(float);
    if (log) hipLaunchKernelGGL((ray_ao_kernel<G, BRUTE, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((ray_ao_kernel<G, BRUTE, false>), grid, block, lds, s, a);
}

template <bool BRUTE>
static void ao_launch(const AoArgs& a, int lanes, bool log, hipStream_t s)
{
    if (lanes == 1) ao_launch_g<1, BRUTE>(a, log, s);
    else if (lanes == 16) ao_launch_g<16, BRUTE>(a, log, s);
    else ao_launch_g<64, BRUTE>(a, log, s);
}

// a whole wave per point once every lane has a target; below that the group shrinks with S so that lanes are not left without work
static int ao_default_lanes(int S) { return S >= 64 ? 64 : (S >= 16 ? 16 : 1); }

extern "C" int gs_ray_ao(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int64_t P,
                         const float* positions, const float* normals, int S, const float* targets, float offset, int lanes_per_point,
                         float* vis, uint8_t* log_hit, float* log_w, void* stream)
{
    GS_CHECK_ARG(F >= 1, "empty mesh: F must be at least 1");
    GS_CHECK_ARG(F <= ((int64_t)1 << 30), "too many faces: at most 2^30");
    GS_CHECK_ARG(V >= 1 && V <= 2147483647ll, "bad vertex count");
    GS_CHECK_ARG(P >= 0, "negative P");
    GS_CHECK_ARG(S >= 1 && S <= AO_MAX_TARGETS, "S must be in 1..4096");
    GS_CHECK_ARG(P <= 2147483647ll / S, "too many rays: P S must be below 2^31");
    GS_CHECK_ARG(lanes_per_point == 0 || lanes_per_point == 1 || lanes_per_point == 16 || lanes_per_point == 64,
                 "lanes_per_point must be 0 (default), 1, 16 or 64");
    GS_CHECK_ARG(isfinite(offset), "offset must be finite");
    GS_CHECK_ARG(vertices != nullptr && faces != nullptr && targets != nullptr, "vertices, faces and targets must not be NULL");
    GS_CHECK_ARG(((uintptr_t)bvh & 15) == 0, "node buffer must be 16-byte aligned");
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(positions != nullptr && normals != nullptr && vis != nullptr, "null point input or output");
    const bool log = log_hit != nullptr || log_w != nullptr;
    GS_CHECK_ARG(!log || (log_hit != nullptr && log_w != nullptr), "the sample log needs both buffers");
    AoArgs a = {};
    a.V = V; a.F = F; a.vertices = vertices; a.faces = faces; a.nodes = (const BvhNode*)bvh;
    a.P = P; a.pos = positions; a.nrm = normals; a.targets = targets; a.S = S; a.offset = offset;
    a.vis = vis; a.log_hit = log_hit; a.log_w = log_w;
    const int lanes = lanes_per_point ? lanes_per_point : ao_default_lanes(S);
    if (bvh != nullptr) ao_launch<false>(a, lanes, log, (hipStream_t)stream);
    else ao_launch<true>(a, lanes, log, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
