// gs_tex2d_dev.h -- the 2-D bilinear lookup of dr.texture (filter_mode='linear', boundary_mode 'wrap' | 'clamp'), shared by the mesh
// shader (gs_meshshade.hip: texture2d, kd / ks) and the lat-long environment resampling (gs_envmap.hip).  Texel centres at
// u W - 0.5; 'wrap' wraps in both axes.
#pragma once
#include "gs_common.h"

struct Tex2Fp {
    bool valid;
    int idx[4];                    // texel indices (not yet times C) of t00, t10, t01, t11
    float fx, fy;
    float su, sv;                  // d x / d u, d y / d v: the texture size, or 0 in a clamped coordinate
};

// Tap selection.  The integer indices are reduced into range in INTEGER arithmetic, after the conversion of a value that was first
// clamped to a finite range: no input produces an address outside the texture.
__device__ __forceinline__ void tex2d_footprint(int W, int H, float u, float v, int boundary, Tex2Fp& fp)
{
    fp.valid = isfinite(u) && isfinite(v);
    if (!fp.valid) { u = 0.0f; v = 0.0f; }
    float x, y;
    bool cx = false, cy = false;
    if (boundary == GS_TEX_WRAP) {
        const float uu = u - floorf(u), vv = v - floorf(v);
        x = uu * (float)W - 0.5f; y = vv * (float)H - 0.5f;
        x = fminf(fmaxf(x, -1.0f), (float)W); y = fminf(fmaxf(y, -1.0f), (float)H);
    } else {                                                         // tex2d_linear_clamp2's coordinates
        x = u * (float)W - 0.5f; y = v * (float)H - 0.5f;
        if (x < 0.0f) { x = 0.0f; cx = true; } else if (x > (float)(W - 1)) { x = (float)(W - 1); cx = true; }
        if (y < 0.0f) { y = 0.0f; cy = true; } else if (y > (float)(H - 1)) { y = (float)(H - 1); cy = true; }
    }
    const int ix0 = (int)floorf(x), iy0 = (int)floorf(y);
    fp.fx = x - (float)ix0; fp.fy = y - (float)iy0;
    int jx0, jx1, jy0, jy1;
    if (boundary == GS_TEX_WRAP) {                                   // ix0 in [-1, W]
        jx0 = (ix0 + W) % W; jx1 = (ix0 + 1 + W) % W;
        jy0 = (iy0 + H) % H; jy1 = (iy0 + 1 + H) % H;
    } else {
        jx0 = min(max(ix0, 0), W - 1); jx1 = min(jx0 + 1, W - 1);
        jy0 = min(max(iy0, 0), H - 1); jy1 = min(jy0 + 1, H - 1);
    }
    fp.idx[0] = jy0 * W + jx0; fp.idx[1] = jy0 * W + jx1; fp.idx[2] = jy1 * W + jx0; fp.idx[3] = jy1 * W + jx1;
    fp.su = cx ? 0.0f : (float)W;
    fp.sv = cy ? 0.0f : (float)H;
}

// value and the derivative of the selected cell's bilinear patch (the forms of tex2d_linear_clamp2)
template <int C>
__device__ __forceinline__ void tex2d_eval(const float* __restrict__ tex, const Tex2Fp& fp, float* out, float* d_du, float* d_dv)
{
    float t[4][C];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) t[i][c] = tex[(size_t)fp.idx[i] * C + c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float top = t[0][c] + fp.fx * (t[1][c] - t[0][c]);
        const float bot = t[2][c] + fp.fx * (t[3][c] - t[2][c]);
        out[c] = fp.valid ? top + fp.fy * (bot - top) : 0.0f;
        d_du[c] = fp.valid ? fp.su * ((t[1][c] - t[0][c]) + fp.fy * ((t[3][c] - t[2][c]) - (t[1][c] - t[0][c]))) : 0.0f;
        d_dv[c] = fp.valid ? fp.sv * (bot - top) : 0.0f;
    }
}

__device__ __forceinline__ void tex2d_weights(const Tex2Fp& fp, float* w)
{
    w[0] = (1.0f - fp.fx) * (1.0f - fp.fy); w[1] = fp.fx * (1.0f - fp.fy);
    w[2] = (1.0f - fp.fx) * fp.fy;          w[3] = fp.fx * fp.fy;
}
