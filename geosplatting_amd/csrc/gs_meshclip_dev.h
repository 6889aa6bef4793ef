// gs_meshclip_dev.h -- near-plane and guard-band clipping for the mesh rasterizer (gs_meshraster.hip) and its antialias pass
// (gs_meshaa.hip), used only with near_clip.  Semantics in include/geosplat_hip.h; the arithmetic that has to give the same bits
// wherever it is inlined (the cut of an edge, the values of a crossing face) is compiled with contraction off.
//   classification  a vertex is inside iff Z > near (mr_load's comparison).  Three inside: a non-crossing face, mr_load's code.  None
//                   inside or a non-finite coordinate: dropped.  Otherwise a crossing face.
//   clip            Sutherland-Hodgman in camera space against Z > near, then xs <= G, xs >= -G, ys <= G, ys >= -G in homogeneous form
//                   (planes through the eye: nothing is divided by a small Z); at most 8 vertices.  The polygon lives in named
//                   registers: every array index is a compile-time constant after unrolling, a run-time append is a chain of selects.
//   cut             always from the inside endpoint A towards the outside endpoint B:  t = dA / (dA - dB),  C = fma(t, B - A, A) per
//                   coordinate, with d the plane's distance below.  Two faces that share the edge compute the same bits.
//   values          per FACE, from the three original vertices (which may lie behind the eye): mc_values.
#ifndef GS_MESHCLIP_DEV_H
#define GS_MESHCLIP_DEV_H
#include "gs_meshraster_dev.h"

#define MC_GUARD 16000.0f               // G in px: 256 G (1 + a few ulp) stays under MR_RANGE = 2^22 = 256 * 16384
#define MC_MAX_VERTS 8

struct McPoly {
    float x[MC_MAX_VERTS], y[MC_MAX_VERTS], z[MC_MAX_VERTS];
    int tag[MC_MAX_VERTS];              // 0..2: that original vertex of the face; -1: a cut
    int n;
};

__device__ __forceinline__ bool mc_load(const float* __restrict__ vc, const int* __restrict__ faces, long long V, long long f,
                                        float (&P)[3][3])
{
    const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;       // never read outside vc
    const int idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k][0] = vc[3 * (size_t)idx[k] + 0];
        P[k][1] = vc[3 * (size_t)idx[k] + 1];
        P[k][2] = vc[3 * (size_t)idx[k] + 2];
    }
    return true;
}

// 0: dropped (nothing inside, or a non-finite coordinate), 1: all three inside, 2: crossing
__device__ __forceinline__ int mc_kind(const float (&P)[3][3], float near)
{
    int inside = 0;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        finite = finite && fabsf(P[k][0]) <= 3.4028235e38f && fabsf(P[k][1]) <= 3.4028235e38f && fabsf(P[k][2]) <= 3.4028235e38f;
        inside += P[k][2] > near ? 1 : 0;
    }
    if (!finite || inside == 0) return 0;
    return inside == 3 ? 1 : 2;
}

__device__ __forceinline__ bool mc_crossing(const float* __restrict__ vc, const int* __restrict__ faces, long long V, long long f,
                                            const MrCam& cam, float (&P)[3][3])
{
    return mc_load(vc, faces, V, f, P) && mc_kind(P, cam.near) == 2;
}

// the distance of plane PLANE, positive inside:  0  Z - near;  1  (G - cx) Z - fx X;  2  (G + cx) Z + fx X;  3, 4 the same in y
template <int PLANE>
__device__ __forceinline__ float mc_dist(float x, float y, float z, const MrCam& cam)
{
#pragma clang fp contract(off)
    if (PLANE == 0) return z - cam.near;
    if (PLANE == 1) return __builtin_fmaf(-cam.fx, x, (MC_GUARD - cam.cx) * z);
    if (PLANE == 2) return __builtin_fmaf(cam.fx, x, (MC_GUARD + cam.cx) * z);
    if (PLANE == 3) return __builtin_fmaf(-cam.fy, y, (MC_GUARD - cam.cy) * z);
    return __builtin_fmaf(cam.fy, y, (MC_GUARD + cam.cy) * z);
}

__device__ __forceinline__ void mc_put(McPoly& O, float x, float y, float z, int tag)
{
#pragma unroll
    for (int j = 0; j < MC_MAX_VERTS; ++j) {
        const bool here = j == O.n;
        O.x[j] = here ? x : O.x[j];
        O.y[j] = here ? y : O.y[j];
        O.z[j] = here ? z : O.z[j];
        O.tag[j] = here ? tag : O.tag[j];
    }
    O.n += 1;
}

// one Sutherland-Hodgman stage: Q has at most NIN vertices, the result at most NIN + 1 <= MC_MAX_VERTS
template <int PLANE, int NIN>
__device__ __forceinline__ void mc_clip_plane(McPoly& Q, const MrCam& cam)
{
#pragma clang fp contract(off)
    float D[NIN];
    bool in[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        D[i] = mc_dist<PLANE>(Q.x[i], Q.y[i], Q.z[i], cam);
        in[i] = PLANE == 0 ? Q.z[i] > cam.near : D[i] >= 0.0f;                           // (a NaN is outside)
    }
    McPoly O;
#pragma unroll
    for (int j = 0; j < MC_MAX_VERTS; ++j) { O.x[j] = 0.0f; O.y[j] = 0.0f; O.z[j] = 0.0f; O.tag[j] = -1; }
    O.n = 0;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        if (i < Q.n) {
            const int j = i + 1 < NIN ? i + 1 : 0;                                      // (a constant after unrolling)
            const bool wrap = i + 1 >= Q.n;
            const float ax = Q.x[i], ay = Q.y[i], az = Q.z[i], da = D[i];
            const float bx = wrap ? Q.x[0] : Q.x[j], by = wrap ? Q.y[0] : Q.y[j], bz = wrap ? Q.z[0] : Q.z[j];
            const float db = wrap ? D[0] : D[j];
            const bool ia = in[i], ib = wrap ? in[0] : in[j];
            if (ia) mc_put(O, ax, ay, az, Q.tag[i]);
            if (ia != ib) {
                // from the inside endpoint (s) towards the outside one (o)
                const float sx = ia ? ax : bx, sy = ia ? ay : by, sz = ia ? az : bz, ds = ia ? da : db;
                const float ox = ia ? bx : ax, oy = ia ? by : ay, oz = ia ? bz : az, dout = ia ? db : da;
                const float t = ds / (ds - dout);
                mc_put(O, __builtin_fmaf(t, ox - sx, sx), __builtin_fmaf(t, oy - sy, sy), __builtin_fmaf(t, oz - sz, sz), -1);
            }
        }
    }
    Q = O;
}

// the clipped polygon of a crossing face, in the face's winding; Q.n < 3: nothing is left
__device__ __forceinline__ void mc_clip(const float (&P)[3][3], const MrCam& cam, McPoly& Q)
{
#pragma unroll
    for (int j = 0; j < MC_MAX_VERTS; ++j) {
        Q.x[j] = j < 3 ? P[j < 3 ? j : 0][0] : 0.0f;
        Q.y[j] = j < 3 ? P[j < 3 ? j : 0][1] : 0.0f;
        Q.z[j] = j < 3 ? P[j < 3 ? j : 0][2] : 0.0f;
        Q.tag[j] = j < 3 ? j : -1;
    }
    Q.n = 3;
    mc_clip_plane<0, 3>(Q, cam);
    mc_clip_plane<1, 4>(Q, cam);
    mc_clip_plane<2, 5>(Q, cam);
    mc_clip_plane<3, 6>(Q, cam);
    mc_clip_plane<4, 7>(Q, cam);
}

// vertex k of the polygon with a run-time k: a chain of selects
__device__ __forceinline__ void mc_get(const McPoly& Q, int k, float& x, float& y, float& z)
{
    x = Q.x[0]; y = Q.y[0]; z = Q.z[0];
#pragma unroll
    for (int j = 1; j < MC_MAX_VERTS; ++j) {
        x = j == k ? Q.x[j] : x;
        y = j == k ? Q.y[j] : y;
        z = j == k ? Q.z[j] : z;
    }
}

// one vertex of a sub-triangle, projected as mr_load projects
__device__ __forceinline__ void mc_project(float x, float y, float z, const MrCam& cam, MrTri& T, int slot)
{
    T.iz[slot] = 1.0f / z;
    T.xs[slot] = __builtin_fmaf(cam.fx, x / z, cam.cx);
    T.ys[slot] = __builtin_fmaf(cam.fy, y / z, cam.cy);
}

// sub-triangle k (1 <= k, k + 1 < Q.n) of the fan (v0, vk, vk+1)
__device__ __forceinline__ void mc_subtri(const McPoly& Q, int k, const MrCam& cam, MrTri& T)
{
    float x, y, z;
    mc_project(Q.x[0], Q.y[0], Q.z[0], cam, T, 0);
    mc_get(Q, k, x, y, z);
    mc_project(x, y, z, cam, T, 1);
    mc_get(Q, k + 1, x, y, z);
    mc_project(x, y, z, cam, T, 2);
}

// b0, b1 and the view depth of a crossing face at the centre of pixel (px, py): where the ray d = ((px + 0.5 - cx) / fx,
// (py + 0.5 - cy) / fy, 1) meets the plane of P0 P1 P2, solved relative to P0 (the errors then scale with the face's edges, not with
// its distance from the eye).  In this order, every operation rounded once, no contraction:
//   e1 = P1 - P0, e2 = P2 - P0;  h = d x e2;  a = (e1x hx + e1y hy) + e1z hz;  g = P0 x e1;
//   nu = (P0x hx + P0y hy) + P0z hz;  nv = (dx gx + dy gy) + gz;  nt = (e2x gx + e2y gy) + e2z gz;  r = -1 / a;
//   b1 = nu r,  b2 = nv r,  depth = nt r,  b0 = (1 - b1) - b2.
// M (h, e1 x d, e1 x e2)^T / a is the inverse of [e1 e2 -d]: the backward pass uses its rows.
struct McRay {
    float dx, dy, e1[3], e2[3], h[3], a;
};

__device__ __forceinline__ void mc_ray(const float (&P)[3][3], const MrCam& cam, int px, int py, McRay& R)
{
#pragma clang fp contract(off)
    R.dx = ((float)px + 0.5f - cam.cx) / cam.fx;
    R.dy = ((float)py + 0.5f - cam.cy) / cam.fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) { R.e1[k] = P[1][k] - P[0][k]; R.e2[k] = P[2][k] - P[0][k]; }
    R.h[0] = R.dy * R.e2[2] - R.e2[1];
    R.h[1] = R.e2[0] - R.dx * R.e2[2];
    R.h[2] = R.dx * R.e2[1] - R.dy * R.e2[0];
    R.a = (R.e1[0] * R.h[0] + R.e1[1] * R.h[1]) + R.e1[2] * R.h[2];
}

__device__ __forceinline__ void mc_values(const float (&P)[3][3], const MrCam& cam, int px, int py, float& b0, float& b1, float& depth)
{
#pragma clang fp contract(off)
    McRay R;
    mc_ray(P, cam, px, py, R);
    const float g0 = P[0][1] * R.e1[2] - P[0][2] * R.e1[1];
    const float g1 = P[0][2] * R.e1[0] - P[0][0] * R.e1[2];
    const float g2 = P[0][0] * R.e1[1] - P[0][1] * R.e1[0];
    const float nu = (P[0][0] * R.h[0] + P[0][1] * R.h[1]) + P[0][2] * R.h[2];
    const float nv = (R.dx * g0 + R.dy * g1) + g2;
    const float nt = (R.e2[0] * g0 + R.e2[1] * g1) + R.e2[2] * g2;
    const float r = -1.0f / R.a;
    b1 = nu * r;
    const float b2 = nv * r;
    depth = nt * r;
    b0 = (1.0f - b1) - b2;
}

#endif
