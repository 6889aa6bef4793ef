// gs_smooth.hip -- the smoothing regularisers of the stage-1 trainer on the un-shaded attribute renders
// (rfstudio/model/geosplat.py:881-922; restated in geosplatting_amd/stage1.py as _edge_aware / _tv), value AND gradient in one call.
// The image holds three renders over the background, channel order kd(3), (0, ks)(3), normal * 0.5 + 0.5 (3); each render has its
// own term kind and weight:
//   edge-aware : (|S(r)| * exp(-|S(gt)|)).sum(direction).mean() over 3 H W, S = kornia's normalised Sobel pair (kernel / 8),
//                replicate padding, cross-correlation; gt = the blended ground truth [H,W,3], channel c against channel c
//   TV         : mean((r[y+1] - r[y])^2) over (H-1) W 3 + mean((r[x+1] - r[x])^2) over H (W-1) 3
// One 16x16 tile per block, its 2-pixel halo in LDS with the coordinates clamped (the replicate padding of the forward):
//   the Sobel cotangent sign(S(r)) * exp(-|S(gt)|) of every in-image pixel of the tile + 1-pixel ring, then the transposed stencil
//   gathered per pixel: per axis, the taps of a neighbour that clamp onto this pixel are summed (a border pixel collects the taps
//   that fell outside the image).  d|x|/dx at 0 is 0, as in torch, so flat regions give exact zeros.
// Per block one partial per (render, sum) -- six floats; one block adds the weighted total to the output scalar in double, in a
// fixed order (deterministic).
#include "gs_common.h"
#pragma clang fp contract(off)

#define SM_T 16
#define SM_IN (SM_T + 4)            // tile + 2-pixel halo: the render around the cotangents of the tile + 1-pixel ring
#define SM_G (SM_T + 2)             // tile + 1-pixel ring: where the Sobel cotangents are needed
#define SM_PARTS 6                  // per render: {edge sum or TV y-sum, TV x-sum}

struct SmoothTerms {
    int kind[3];                    // GS_SMOOTH_NONE / _EDGE / _TV per render
    float gscale[3];                // gradient factor: edge w / (3 H W) / 8 (the Sobel normalisation), TV 2 w / N_y
    float gscale_x[3];              // TV only: 2 w / N_x
    int any_edge;
};

// Sobel pair at LDS position (r, c) of a clamped tile, kernel / 8: the two weighted columns (rows) are formed by the same operations,
// so a constant neighbourhood gives exactly 0
__device__ __forceinline__ float sobel_x(const float (*t)[SM_IN + 1], int r, int c)
{
    const float cr = (t[r - 1][c + 1] + 2.0f * t[r][c + 1]) + t[r + 1][c + 1];
    const float cl = (t[r - 1][c - 1] + 2.0f * t[r][c - 1]) + t[r + 1][c - 1];
    return (cr - cl) * 0.125f;
}
__device__ __forceinline__ float sobel_y(const float (*t)[SM_IN + 1], int r, int c)
{
    const float rb = (t[r + 1][c - 1] + 2.0f * t[r + 1][c]) + t[r + 1][c + 1];
    const float rt = (t[r - 1][c - 1] + 2.0f * t[r - 1][c]) + t[r - 1][c + 1];
    return (rb - rt) * 0.125f;
}
__device__ __forceinline__ float sgn0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// weight with which the 3-tap axis kernel {a0, a1, a2} centred on p reads q under replicate padding (clamped taps summed)
__device__ __forceinline__ float tap_weight(int p, int q, int n, float a0, float a1, float a2)
{
    const int um = p - 1 < 0 ? 0 : p - 1, up = p + 1 > n - 1 ? n - 1 : p + 1;
    return (um == q ? a0 : 0.0f) + (p == q ? a1 : 0.0f) + (up == q ? a2 : 0.0f);
}

__device__ __forceinline__ void load_clamped(float (*dst)[SM_IN + 1], const float* __restrict__ src, int stride, int ch, int x0, int y0,
                                             int W, int H)
{
    for (int i = threadIdx.x; i < SM_IN * SM_IN; i += 256) {
        const int r = i / SM_IN, c = i % SM_IN;
        int gy = y0 - 2 + r, gx = x0 - 2 + c;
        gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
        gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
        dst[r][c] = src[((size_t)gy * W + gx) * stride + ch];
    }
}

__global__ void __launch_bounds__(256)
smooth_loss_kernel(int W, int H, const float* __restrict__ img, const float* __restrict__ gt, SmoothTerms t,
                   float* __restrict__ v_img, float* __restrict__ partials)
{
    __shared__ float s_in[SM_IN][SM_IN + 1];
    __shared__ float s_wg[3][2][SM_G][SM_G + 1];        // exp(-|S(gt)|) per GT channel and direction
    __shared__ float s_gx[SM_G][SM_G + 1], s_gy[SM_G][SM_G + 1];
    __shared__ float s_red[4][SM_PARTS];
    const int tid = threadIdx.x, tx = tid % SM_T, ty = tid / SM_T;
    const int x0 = blockIdx.x * SM_T, y0 = blockIdx.y * SM_T;
    const int qx = x0 + tx, qy = y0 + ty;
    const bool inside = qx < W && qy < H;
    const size_t pix = (size_t)qy * W + qx;
    float part[SM_PARTS];
#pragma unroll
    for (int k = 0; k < SM_PARTS; ++k) part[k] = 0.0f;

    if (t.any_edge) {
        for (int c = 0; c < 3; ++c) {
            load_clamped(s_in, gt, 3, c, x0, y0, W, H);
            __syncthreads();
            for (int i = tid; i < SM_G * SM_G; i += 256) {
                const int r = i / SM_G, cc = i % SM_G;
                s_wg[c][0][r][cc] = expf(-fabsf(sobel_x(s_in, r + 1, cc + 1)));
                s_wg[c][1][r][cc] = expf(-fabsf(sobel_y(s_in, r + 1, cc + 1)));
            }
            __syncthreads();
        }
    }
    // per axis: the smoothing taps {1, 2, 1} and the derivative taps {-1, 0, 1} of the neighbours qy - 1 + j (qx - 1 + i)
    float sy[3], dy[3], sx[3], dx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        sy[j] = tap_weight(qy - 1 + j, qy, H, 1.0f, 2.0f, 1.0f); dy[j] = tap_weight(qy - 1 + j, qy, H, -1.0f, 0.0f, 1.0f);
        sx[j] = tap_weight(qx - 1 + j, qx, W, 1.0f, 2.0f, 1.0f); dx[j] = tap_weight(qx - 1 + j, qx, W, -1.0f, 0.0f, 1.0f);
    }

    for (int ch = 0; ch < 9; ++ch) {
        const int im = ch / 3, kind = t.kind[im];           // (block-uniform)
        if (kind == GS_SMOOTH_NONE) {
            if (inside) v_img[pix * 9 + ch] = 0.0f;
            continue;
        }
        load_clamped(s_in, img, 9, ch, x0, y0, W, H);
        __syncthreads();
        float v = 0.0f;
        if (kind == GS_SMOOTH_EDGE) {
            for (int i = tid; i < SM_G * SM_G; i += 256) {
                const int r = i / SM_G, cc = i % SM_G;
                const int py = y0 - 1 + r, px = x0 - 1 + cc;
                float gx = 0.0f, gy = 0.0f;
                if (py >= 0 && py < H && px >= 0 && px < W) {
                    const float ex = sobel_x(s_in, r + 1, cc + 1), ey = sobel_y(s_in, r + 1, cc + 1);
                    const float wx = s_wg[ch % 3][0][r][cc], wy = s_wg[ch % 3][1][r][cc];
                    gx = sgn0(ex) * wx; gy = sgn0(ey) * wy;
                    if (r >= 1 && r <= SM_T && cc >= 1 && cc <= SM_T) part[2 * im] += fabsf(ex) * wx + fabsf(ey) * wy;
                }
                s_gx[r][cc] = gx; s_gy[r][cc] = gy;
            }
            __syncthreads();
            if (inside) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        v += s_gx[ty + j][tx + i] * (sy[j] * dx[i]) + s_gy[ty + j][tx + i] * (dy[j] * sx[i]);
                v *= t.gscale[im];
            }
        } else if (inside) {                                 // TV: forward differences along y and x
            const float r0 = s_in[ty + 2][tx + 2];
            const float dn = qy < H - 1 ? s_in[ty + 3][tx + 2] - r0 : 0.0f, up = qy > 0 ? r0 - s_in[ty + 1][tx + 2] : 0.0f;
            const float rt = qx < W - 1 ? s_in[ty + 2][tx + 3] - r0 : 0.0f, lf = qx > 0 ? r0 - s_in[ty + 2][tx + 1] : 0.0f;
            part[2 * im] += dn * dn;
            part[2 * im + 1] += rt * rt;
            v = (up - dn) * t.gscale[im] + (lf - rt) * t.gscale_x[im];
        }
        if (inside) v_img[pix * 9 + ch] = v;
        __syncthreads();                                     // (s_in / s_gx / s_gy are reused by the next channel)
    }
    const int wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < SM_PARTS; ++k) {
        const float s = gs_wave_sum(part[k]);
        if ((tid & 63) == 0) s_red[wave][k] = s;
    }
    __syncthreads();
    if (tid < SM_PARTS) {
        const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[SM_PARTS * b + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    }
}

struct SmoothNorm { double w[3]; double n0[3], n1[3]; };    // value = sum_im w * (sum0 / n0 + sum1 / n1)  (n = 0: that sum unused)

__global__ void __launch_bounds__(256)
smooth_finalize_kernel(int nblocks, const float* __restrict__ partials, SmoothNorm nrm, float* __restrict__ out)
{
    __shared__ double red[256][SM_PARTS];
    double s[SM_PARTS];
#pragma unroll
    for (int k = 0; k < SM_PARTS; ++k) s[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < SM_PARTS; ++k) s[k] += (double)partials[SM_PARTS * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < SM_PARTS; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int k = 0; k < SM_PARTS; ++k) red[threadIdx.x][k] += red[threadIdx.x + st][k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int im = 0; im < 3; ++im) {
            if (nrm.n0[im] > 0.0) v += nrm.w[im] * red[0][2 * im] / nrm.n0[im];
            if (nrm.n1[im] > 0.0) v += nrm.w[im] * red[0][2 * im + 1] / nrm.n1[im];
        }
        out[0] = (float)((double)out[0] + v);
    }
}

extern "C" size_t gs_smooth_loss_ws_bytes(int W, int H)
{
    if (W <= 0 || H <= 0) return 0;
    return sizeof(float) * SM_PARTS * (size_t)gs_cdiv(W, SM_T) * (size_t)gs_cdiv(H, SM_T);
}

extern "C" int gs_smooth_loss(int W, int H, const float* img, const float* gt_rgb, const int* kinds, const float* weights, float* out,
                              float* v_img, void* ws, size_t ws_bytes, void* stream)
{
    GS_CHECK_ARG(W >= 2 && H >= 2, "W, H must be >= 2");
    GS_CHECK_ARG(kinds != nullptr && weights != nullptr, "kinds / weights (host arrays of 3) must not be NULL");
    GS_CHECK_ARG(img != nullptr && out != nullptr && v_img != nullptr && ws != nullptr, "null argument");
    GS_CHECK_ARG(ws_bytes >= gs_smooth_loss_ws_bytes(W, H), "workspace too small");
    SmoothTerms t;
    SmoothNorm nrm;
    t.any_edge = 0;
    const double px = (double)W * H, ny = 3.0 * (double)(H - 1) * W, nx = 3.0 * (double)H * (W - 1);
    for (int im = 0; im < 3; ++im) {
        GS_CHECK_ARG(kinds[im] >= GS_SMOOTH_NONE && kinds[im] <= GS_SMOOTH_TV, "kind must be GS_SMOOTH_NONE / _EDGE / _TV");
        const double w = (double)weights[im];
        t.kind[im] = kinds[im];
        t.gscale[im] = t.gscale_x[im] = 0.0f;
        nrm.w[im] = w; nrm.n0[im] = nrm.n1[im] = 0.0;
        if (kinds[im] == GS_SMOOTH_EDGE) {
            t.any_edge = 1;
            t.gscale[im] = (float)(w / (3.0 * px) * 0.125);
            nrm.n0[im] = 3.0 * px;
        } else if (kinds[im] == GS_SMOOTH_TV) {
            t.gscale[im] = (float)(2.0 * w / ny);
            t.gscale_x[im] = (float)(2.0 * w / nx);
            nrm.n0[im] = ny; nrm.n1[im] = nx;
        }
    }
    GS_CHECK_ARG(!t.any_edge || gt_rgb != nullptr, "an edge-aware term needs gt_rgb");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(gs_cdiv(W, SM_T), gs_cdiv(H, SM_T));
    float* partials = (float*)ws;
    hipLaunchKernelGGL(smooth_loss_kernel, grid, dim3(256), 0, s, W, H, img, gt_rgb, t, v_img, partials);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(smooth_finalize_kernel, dim3(1), dim3(256), 0, s, (int)(grid.x * grid.y), partials, nrm, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
