// gs_meshraster_dev.h -- device helpers shared by the mesh rasterizer (gs_meshraster.hip) and its antialias pass (gs_meshaa.hip):
// the load, snap, edge set-up, value and cull code.  Both files decide coverage through these, so a face the rasterizer drops or
// culls is dropped or culled by the antialias pass in the same way.
#ifndef GS_MESHRASTER_DEV_H
#define GS_MESHRASTER_DEV_H
#include "gs_common.h"

#define MR_BLOCK 256
#ifndef MR_SMALL_BOX
#define MR_SMALL_BOX 16                 // pass 1 walks boxes of at most MR_SMALL_BOX x MR_SMALL_BOX px
#endif
#define MR_SNAP 256                     // sub-pixel units per pixel
#define MR_RANGE 4194304.0f             // 2^22: snapped coordinates outside +-2^22 drop the triangle
#define MR_EMPTY 0xffffffffffffffffull
#define MR_MAX_BIG_BLOCKS 2048

struct MrCam {
    float fx, fy, cx, cy, near;
    int H, W;
};

// the fp32 side of a triangle: screen positions (unsnapped) and 1 / Z
struct MrTri {
    float xs[3], ys[3], iz[3];
};

// the integer side: edge i runs from vertex i+1 to vertex i+2 (opposite vertex i), oriented so that the inside is positive.
// E_i(px, py) = c[i] + ax[i] (px - x0) + ay[i] (py - y0) at the pixel centre (256 px + 128, 256 py + 128); inside iff E_i + bias[i] >= 0
// with bias 0 on a top or left edge and -1 elsewhere.
struct MrEdges {
    long long c[3], ax[3], ay[3];
    int bias[3];
    int x0, y0, x1, y1;                 // inclusive pixel box, clipped to the image; empty when x1 < x0 or y1 < y0
    bool negative;                      // signed snapped area < 0
};

__device__ __forceinline__ bool mr_load(const float* __restrict__ vc, const int* __restrict__ faces, long long V, long long f,
                                        const MrCam& cam, MrTri& T, float (&P)[3][3])
{
    const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;       // never read outside vc
    const int idx[3] = {i0, i1, i2};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float X = vc[3 * (size_t)idx[k] + 0], Y = vc[3 * (size_t)idx[k] + 1], Z = vc[3 * (size_t)idx[k] + 2];
        P[k][0] = X; P[k][1] = Y; P[k][2] = Z;
        ok = ok && (Z > cam.near);                                                      // (a NaN fails)
        T.iz[k] = 1.0f / Z;
        T.xs[k] = __builtin_fmaf(cam.fx, X / Z, cam.cx);
        T.ys[k] = __builtin_fmaf(cam.fy, Y / Z, cam.cy);
    }
    return ok;
}

// X, Y: the snapped vertex positions in 1/256 px, valid when the result is true
__device__ __forceinline__ bool mr_edges(const MrTri& T, const MrCam& cam, MrEdges& E, int (&X)[3], int (&Y)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sx = T.xs[k] * (float)MR_SNAP, sy = T.ys[k] * (float)MR_SNAP;
        if (!(fabsf(sx) <= MR_RANGE && fabsf(sy) <= MR_RANGE)) return false;            // (a NaN fails)
        X[k] = (int)__builtin_rintf(sx);
        Y[k] = (int)__builtin_rintf(sy);
    }
    const long long area = (long long)(X[1] - X[0]) * (long long)(Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (long long)(X[2] - X[0]);
    if (area == 0) return false;
    E.negative = area < 0;
    const int minx = min(X[0], min(X[1], X[2])), maxx = max(X[0], max(X[1], X[2]));
    const int miny = min(Y[0], min(Y[1], Y[2])), maxy = max(Y[0], max(Y[1], Y[2]));
    // pixel centres 256 p + 128 inside [min, max]: p >= ceil((min - 128) / 256), p <= floor((max - 128) / 256)  (arithmetic shifts)
    E.x0 = max((minx + 127) >> 8, 0);
    E.y0 = max((miny + 127) >> 8, 0);
    E.x1 = min((maxx - 128) >> 8, cam.W - 1);
    E.y1 = min((maxy - 128) >> 8, cam.H - 1);
    if (E.x1 < E.x0 || E.y1 < E.y0) return true;                                       // nothing to walk
    const long long sx = (long long)MR_SNAP * E.x0 + MR_SNAP / 2, sy = (long long)MR_SNAP * E.y0 + MR_SNAP / 2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        long long dx = X[b] - X[a], dy = Y[b] - Y[a];
        if (E.negative) { dx = -dx; dy = -dy; }
        E.c[i] = dx * (sy - Y[a]) - dy * (sx - X[a]);
        E.ax[i] = -dy * MR_SNAP;
        E.ay[i] = dx * MR_SNAP;
        E.bias[i] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;                          // top (y grows downwards) or left edge
    }
    return true;
}

__device__ __forceinline__ bool mr_edges(const MrTri& T, const MrCam& cam, MrEdges& E)
{
    int X[3], Y[3];
    return mr_edges(T, cam, E, X, Y);
}

// b0, b1 and the view depth at the centre of pixel (px, py): unsnapped fp32 edge functions on coordinates relative to the pixel
// centre, e_i = q_{i+1} x q_{i+2};  b_i = e_i / Z_i / N,  depth = (e0 + e1 + e2) / N,  N = sum_j e_j / Z_j.  This is
// lambda_i = e_i / sum e, b_i = (lambda_i / Z_i) / sum_j lambda_j / Z_j, depth = 1 / sum_j lambda_j / Z_j with the common factor
// taken out; nothing is clamped.  With equal Z that are a power of two, N and the sum round alike: coplanar triangles tie exactly.
__device__ __forceinline__ void mr_values(const MrTri& T, int px, int py, float& b0, float& b1, float& depth)
{
    const float pcx = (float)px + 0.5f, pcy = (float)py + 0.5f;
    const float q0x = T.xs[0] - pcx, q0y = T.ys[0] - pcy;
    const float q1x = T.xs[1] - pcx, q1y = T.ys[1] - pcy;
    const float q2x = T.xs[2] - pcx, q2y = T.ys[2] - pcy;
    const float e0 = q1x * q2y - q1y * q2x;
    const float e1 = q2x * q0y - q2y * q0x;
    const float e2 = q0x * q1y - q0y * q1x;
    const float w0 = e0 * T.iz[0], w1 = e1 * T.iz[1], w2 = e2 * T.iz[2];
    const float sum = (e0 + e1) + e2;
    const float N = (w0 + w1) + w2;
    const float rN = 1.0f / N;
    b0 = w0 * rN;
    b1 = w1 * rN;
    depth = sum / N;
}

__device__ __forceinline__ bool mr_culled(const MrEdges& E, int cull)
{
    // cull = 1 ('back') keeps (camera - centroid) . ((v1 - v0) x (v2 - v0)) > 0.  In camera space the eye is the origin and the
    // normal is orthogonal to both edges, so this is -det[v0; v1; v2] > 0, and det = Z0 Z1 Z2 / (fx fy) times the signed screen area
    // (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0): with every Z > near > 0, kept iff the area is negative.
    return cull == 1 && !E.negative;
}

#endif
