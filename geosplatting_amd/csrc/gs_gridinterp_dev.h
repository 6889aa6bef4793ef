// gs_gridinterp_dev.h -- the ONE periodic trilinear weight routine of csrc/gs_poisson.hip: the splat, the sample, and both of
// their backward kernels locate a point and weigh its eight nodes through gi_locate / gi_weight / gi_node, so the four directions
// agree bit for bit (the adjoint pair <splat(p, v), g> = <v, sample(g, p)> differs only by the order of its sums).
#pragma once
#include "gs_common.h"

struct GiRes {
    int R[3];                                       // nodes per axis; node i sits at i / R; the last axis is the fastest
};

struct GiCell {
    int lo[3], hi[3];                               // lower node floor(p R) mod R and (lo + 1) mod R
    float f[3];                                     // p R - floor(p R), in [0, 1]
};

// A row takes part iff its three coordinates are finite and |p| < 1024: decided on the floats, before any conversion to an
// integer, so that no input forms an index outside the grid.  p is wrapped to [0, 1] first (p - floor(p): exact for p >= 0, within
// 2^-25 for a tiny negative p, where it gives 1.0 -- which lands on node 0 like p = 1.0 itself), then s = p R in [0, R].
__device__ __forceinline__ bool gi_locate(const float* __restrict__ p3, const GiRes& G, GiCell& c)
{
    const float p[3] = {p3[0], p3[1], p3[2]};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && (fabsf(p[a]) < 1024.0f);                 // NaN and inf fail
    if (!ok) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float w = p[a] - floorf(p[a]);                                       // [0, 1]
        const float s = w * (float)G.R[a];                                         // [0, R]
        const float fl = floorf(s);
        int i = (int)fl;                                                           // 0 .. R: in range by construction
        i = i >= G.R[a] ? i - G.R[a] : i;
        i = i < 0 ? 0 : i;
        c.lo[a] = i;
        c.hi[a] = i + 1 >= G.R[a] ? 0 : i + 1;
        c.f[a] = s - fl;                                                           // exact
    }
    return true;
}

// linear index of corner k (bit 2: axis 0, bit 1: axis 1, bit 0: axis 2 -- the last axis toggles fastest)
__device__ __forceinline__ long long gi_node(const GiCell& c, const GiRes& G, int k)
{
    const int i0 = (k & 4) ? c.hi[0] : c.lo[0], i1 = (k & 2) ? c.hi[1] : c.lo[1], i2 = (k & 1) ? c.hi[2] : c.lo[2];
    return ((long long)i0 * G.R[1] + i1) * G.R[2] + i2;
}

// per-axis weights: lower node 1 - f, upper node f
__device__ __forceinline__ void gi_axis_weights(const GiCell& c, float (&w)[3][2])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) { w[a][0] = 1.0f - c.f[a]; w[a][1] = c.f[a]; }
}

// weight of corner k: (w0 w1) w2, in this order everywhere
__device__ __forceinline__ float gi_weight(const float (&w)[3][2], int k)
{
#pragma clang fp contract(off)
    return (w[0][(k >> 2) & 1] * w[1][(k >> 1) & 1]) * w[2][k & 1];
}

// d weight_k / d p_a = +-R_a times the product of the two other axes' weights (upper node +, lower node -)
__device__ __forceinline__ float gi_dweight(const float (&w)[3][2], const GiRes& G, int k, int a)
{
#pragma clang fp contract(off)
    const int b0 = (k >> 2) & 1, b1 = (k >> 1) & 1, b2 = k & 1;
    const float other = a == 0 ? w[1][b1] * w[2][b2] : a == 1 ? w[0][b0] * w[2][b2] : w[0][b0] * w[1][b1];
    const int up = a == 0 ? b0 : a == 1 ? b1 : b2;
    return (up ? other : -other) * (float)G.R[a];
}
