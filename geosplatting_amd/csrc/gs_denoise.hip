// gs_denoise.hip -- the edge-avoiding bilateral filter the reference runs on its Monte-Carlo estimates (bilateral_denoiser of
// rfstudio/graphics/_mesh/_optix: ops.py:107-140, c_src/denoising.cu), restated; include/geosplat_hip.h states the semantics.
//
// Both directions are gathers over the (2R+1)^2 window, fy outer and fx inner, one thread per pixel, no atomics.  The backward is the
// forward's loop on other operands (the colour plane holds g / W, the depth denominator takes dz of the tap instead of the centre), so
// one kernel template serves both.  Two forms of that kernel:
//   tiled  a workgroup of 32 x TH pixels (TH = 8, 16 or 32: the height that keeps the most waves on a CU within its 160 KiB of LDS,
//          dn_tile_height) stages its tile plus the R-halo of every operand as planes in LDS once (out-of-image positions as zeros: a
//          zero normal gives the weight clamp(0, 1e-4, 1)^128 = 0 EXACTLY, so such taps add exact zeros and the loops need no bounds
//          test), next to the table of the per-offset factors (w_xy, |offset|) of the whole window;
//   plain  a 32 x 8 tile reading the taps from global memory, with the factors of one window row at a time in LDS -- for any
//          radius whose halo does not fit.
// A tap's weight is one function (`dn_tap_weight`, contraction off, explicit FMAs) and the sums run in the same order, so the two forms
// give the same bits, and so do a C-channel call and calls on its channel slices.
#include "gs_common.h"

#include <math.h>

#define DN_TW 32
#define DN_TH 8
#define DN_TH_MAX 32
#define DN_BLOCK (DN_TW * DN_TH)
#define DN_LDS_LIMIT (160 * 1024)
#define DN_EPS 1e-4f

struct DnArgs {
    int B, H, W, ZC, R;
    int TH;                        // rows of a workgroup's tile (the plain form: DN_TH)
    float inv2v;                   // 1 / (2 sigma^2)
    const float* col;              // forward: col [B,H,W,C]; backward: out_grad
    const float* nrm;
    const float* zdz;
    const float* wsum_in;          // backward: the forward's clamped weight sums [B,H,W]
    float* out;                    // forward: out; backward: col_grad
    float* wsum_out;               // forward only
};

// (w_xy, |offset|) of one window offset: they depend on nothing else, so a workgroup computes each once
__device__ __forceinline__ float2 dn_offset_factors(int fx, int fy, float inv2v)
{
#pragma clang fp contract(off)
    const float d2 = (float)(fx * fx + fy * fy);
    return make_float2(__expf(-(d2 * inv2v)), sqrtf(d2));
}

// w = w_xy w_n w_z of one tap; `dz` is the centre's in forward and the tap's in backward
__device__ __forceinline__ float dn_tap_weight(float2 of, float nx, float ny, float nz, float cnx, float cny, float cnz, float z, float cz, float dz)
{
#pragma clang fp contract(off)
    float c = __builtin_fmaf(nx, cnx, __builtin_fmaf(ny, cny, nz * cnz));
    c = fminf(fmaxf(c, DN_EPS), 1.0f);
    c = c * c; c = c * c; c = c * c; c = c * c; c = c * c; c = c * c; c = c * c;              // ^128
    const float a = fabsf(z - cz) * __builtin_amdgcn_rcpf(fmaxf(dz * of.y, DN_EPS));
    return (of.x * c) * __expf(-a);
}

template <int C, bool BWD, bool TILED>
__global__ void __launch_bounds__(TILED ? DN_TW * DN_TH_MAX : DN_BLOCK) denoise_kernel(const DnArgs a)
{
    extern __shared__ float dn_lds[];
    const int TH = TILED ? a.TH : DN_TH, threads = DN_TW * TH;
    const int tid = (int)threadIdx.x, tx = tid % DN_TW, ty = tid / DN_TW;
    const int x0 = (int)blockIdx.x * DN_TW, y0 = (int)blockIdx.y * TH, b = (int)blockIdx.z;
    const int x = x0 + tx, y = y0 + ty, R = a.R, D = 2 * R + 1, H = a.H, W = a.W, ZC = a.ZC;
    const bool valid = x < W && y < H;
    const int64_t image = (int64_t)b * H * W;
    // window rows that reach the image from any row of this tile: the same for every lane, so the row loop is uniform
    const int fy_lo = -min(R, y0 + TH - 1), fy_hi = min(R, H - 1 - y0);

    float cnx = 0.f, cny = 0.f, cnz = 0.f, cz = 0.f, cdz = 0.f;
    if (valid) {
        const int64_t p = image + (int64_t)y * W + x;
        cnx = a.nrm[p * 3 + 0]; cny = a.nrm[p * 3 + 1]; cnz = a.nrm[p * 3 + 2];
        cz = a.zdz[p * ZC]; cdz = a.zdz[p * ZC + ZC - 1];
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    float wsum = 0.0f;

    if constexpr (TILED) {
        const int HW = DN_TW + 2 * R, HH = TH + 2 * R, plane = HW * HH;
        float* const s_nx = dn_lds, * const s_ny = s_nx + plane, * const s_nz = s_ny + plane, * const s_z = s_nz + plane;
        float* const s_dz = s_z + plane;                                             // backward only
        float* const s_col = s_z + (BWD ? 2 : 1) * plane;                            // C planes
        float2* const s_of = (float2*)(s_col + (size_t)C * plane);                   // (plane counts are even: HW is)
        for (int i = tid; i < plane; i += threads) {
            const int hy = i / HW, hx = i - hy * HW, gy = y0 - R + hy, gx = x0 - R + hx;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int64_t q = image + (int64_t)gy * W + gx;
            s_nx[i] = in ? a.nrm[q * 3 + 0] : 0.0f;
            s_ny[i] = in ? a.nrm[q * 3 + 1] : 0.0f;
            s_nz[i] = in ? a.nrm[q * 3 + 2] : 0.0f;
            s_z[i] = in ? a.zdz[q * ZC] : 0.0f;
            float r = 1.0f;
            if constexpr (BWD) {
                s_dz[i] = in ? a.zdz[q * ZC + ZC - 1] : 0.0f;
                r = in ? 1.0f / a.wsum_in[q] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = in ? a.col[q * C + c] : 0.0f;
                s_col[c * plane + i] = BWD ? v * r : v;
            }
        }
        for (int i = tid; i < D * D; i += threads) {
            const int fy = i / D;
            s_of[i] = dn_offset_factors(i - fy * D - R, fy - R, a.inv2v);
        }
        __syncthreads();
        if (valid) {
            for (int fy = fy_lo; fy <= fy_hi; ++fy) {
                const int row = (ty + R + fy) * HW + tx;                             // + (R + fx) walks the window row
                const float2* const of_row = s_of + (fy + R) * D;
                for (int k = 0; k < D; ++k) {
                    const int i = row + k;
                    const float w = dn_tap_weight(of_row[k], s_nx[i], s_ny[i], s_nz[i], cnx, cny, cnz, s_z[i], cz, BWD ? s_dz[i] : cdz);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = __builtin_fmaf(w, s_col[c * plane + i], acc[c]);
                    wsum += w;
                }
            }
        }
    } else {
        float2* const s_of = (float2*)dn_lds;                                        // one window row: D <= 255 entries
        for (int fy = fy_lo; fy <= fy_hi; ++fy) {
            __syncthreads();                                                         // (the row before is read out)
            if (tid < D) s_of[tid] = dn_offset_factors(tid - R, fy, a.inv2v);
            __syncthreads();
            const int gy = y + fy;
            if (!valid || gy < 0 || gy >= H) continue;
            const int k_lo = max(0, R - x), k_hi = min(D - 1, W - 1 - x + R);
            for (int k = k_lo; k <= k_hi; ++k) {
                const int64_t q = image + (int64_t)gy * W + (x + k - R);
                const float w = dn_tap_weight(s_of[k], a.nrm[q * 3 + 0], a.nrm[q * 3 + 1], a.nrm[q * 3 + 2], cnx, cny, cnz, a.zdz[q * ZC], cz,
                                              BWD ? a.zdz[q * ZC + ZC - 1] : cdz);
                float r = 1.0f;
                if constexpr (BWD) r = 1.0f / a.wsum_in[q];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float v = a.col[q * C + c];
                    acc[c] = __builtin_fmaf(w, BWD ? v * r : v, acc[c]);
                }
                wsum += w;
            }
        }
    }

    if (!valid) return;
    const int64_t p = image + (int64_t)y * W + x;
    if constexpr (BWD) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[p * C + c] = acc[c];
    } else {
        const float wc = fmaxf(wsum, DN_EPS);
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[p * C + c] = acc[c] / wc;
        a.wsum_out[p] = wc;
    }
}

static int dn_radius(double sigma) { return 2 * (int)ceil(2.5 * sigma) + 1; }

// LDS of the tiled form: the halo planes (normal, z, dz, C colours -- the backward's count, so that both directions of one call take
// the same form) and the factor table
static size_t dn_tiled_lds(int C, int R, int TH = DN_TH)
{
    const size_t plane = (size_t)(DN_TW + 2 * R) * (TH + 2 * R), D = 2 * (size_t)R + 1;
    return sizeof(float) * plane * (5 + (size_t)C) + sizeof(float2) * D * D;
}

// the tile height of the tiled form: the one that keeps the most waves resident on a CU (workgroups that fit its LDS x waves of
// each), the lower one on a tie (more workgroups to spread).  Higher tiles stage less halo per pixel AND bring more waves: at R = 11
// a 32 x 8 tile of 8 channels fills the LDS of a CU with one wave per SIMD ("Bilateral denoiser")
static int dn_tile_height(int C, int R)
{
    int best = DN_TH, best_waves = 0;
    for (int th = DN_TH; th <= DN_TH_MAX; th *= 2) {
        const size_t lds = dn_tiled_lds(C, R, th);
        if (lds > DN_LDS_LIMIT) break;
        int waves = (int)(DN_LDS_LIMIT / lds) * (DN_TW * th / GS_WAVE);
        if (waves > 32) waves = 32;
        if (waves > best_waves) { best = th; best_waves = waves; }
    }
    return best;
}

static const char* dn_check(int B, int H, int W, int C, int ZC, double sigma, int tiled)
{
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be at least 1";
    if (C < 1 || C > 8) return "C must be 1..8";
    if (ZC != 1 && ZC != 2) return "zdz must have 1 or 2 channels";
    if (!(sigma > 0.0) || !isfinite(sigma)) return "sigma must be finite and positive";
    if (2.5 * sigma > 64.0 || dn_radius(sigma) > 127) return "sigma too large: the radius 2 ceil(2.5 sigma) + 1 must not exceed 127";
    if (B > 65535 || gs_cdiv(H, DN_TH) > 65535) return "image too large: B and H / 8 must not exceed 65535";
    if (tiled < -1 || tiled > 1) return "tiled must be -1 (pick), 0 (plain) or 1 (tiled)";
    if (tiled == 1 && dn_tiled_lds(C, dn_radius(sigma)) > DN_LDS_LIMIT) return "tiled form: the halo does not fit the LDS at this radius and C";
    return nullptr;
}

template <int C, bool BWD>
static int dn_launch_c(const DnArgs& a, bool tiled, hipStream_t s)
{
    if (tiled) {
        DnArgs t = a;
        t.TH = dn_tile_height(C, a.R);
        const size_t lds = dn_tiled_lds(C, a.R, t.TH);
        if (lds > 64 * 1024)                       // the opt-in for more than 64 KB of dynamic LDS, per device: set on every such launch
            GS_CHECK_HIP(hipFuncSetAttribute((const void*)denoise_kernel<C, BWD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((denoise_kernel<C, BWD, true>), dim3(gs_cdiv(a.W, DN_TW), gs_cdiv(a.H, t.TH), a.B), dim3(DN_TW * t.TH), lds, s, t);
    } else {
        hipLaunchKernelGGL((denoise_kernel<C, BWD, false>), dim3(gs_cdiv(a.W, DN_TW), gs_cdiv(a.H, DN_TH), a.B), dim3(DN_BLOCK),
                           sizeof(float2) * 256, s, a);
    }
    GS_CHECK_LAUNCH();
    return GS_OK;
}

template <bool BWD>
static int dn_launch(int C, const DnArgs& a, bool tiled, hipStream_t s)
{
    switch (C) {
    case 1: return dn_launch_c<1, BWD>(a, tiled, s);
    case 2: return dn_launch_c<2, BWD>(a, tiled, s);
    case 3: return dn_launch_c<3, BWD>(a, tiled, s);
    case 4: return dn_launch_c<4, BWD>(a, tiled, s);
    case 5: return dn_launch_c<5, BWD>(a, tiled, s);
    case 6: return dn_launch_c<6, BWD>(a, tiled, s);
    case 7: return dn_launch_c<7, BWD>(a, tiled, s);
    default: return dn_launch_c<8, BWD>(a, tiled, s);
    }
}

// the form a call takes: the tiled one wherever its halo fits, except for images lower than a tile, whose rows it would mostly stage
// and walk for nothing (the [1,1,N,C] shape)
static bool dn_pick_tiled(int H, int C, int R, int tiled)
{
    if (tiled >= 0) return tiled == 1;
    return H >= DN_TH && dn_tiled_lds(C, R) <= DN_LDS_LIMIT;
}

extern "C" int gs_denoise_tiled_fits(int C, double sigma)
{
    if (C < 1 || C > 8 || !(sigma > 0.0) || !isfinite(sigma) || 2.5 * sigma > 64.0 || dn_radius(sigma) > 127) return 0;
    return dn_tiled_lds(C, dn_radius(sigma)) <= DN_LDS_LIMIT ? 1 : 0;
}

extern "C" int gs_denoise_fwd(int B, int H, int W, int C, int zdz_channels, const float* col, const float* nrm, const float* zdz, double sigma,
                              int tiled, float* out, float* wsum, void* stream)
{
    const char* msg = dn_check(B, H, W, C, zdz_channels, sigma, tiled);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(col != nullptr && nrm != nullptr && zdz != nullptr, "null input");
    GS_CHECK_ARG(out != nullptr && wsum != nullptr, "null output");
    DnArgs a = {};
    a.B = B; a.H = H; a.W = W; a.ZC = zdz_channels; a.TH = DN_TH; a.R = dn_radius(sigma); a.inv2v = (float)(1.0 / (2.0 * sigma * sigma));
    a.col = col; a.nrm = nrm; a.zdz = zdz; a.out = out; a.wsum_out = wsum;
    return dn_launch<false>(C, a, dn_pick_tiled(H, C, a.R, tiled), (hipStream_t)stream);
}

extern "C" int gs_denoise_bwd(int B, int H, int W, int C, int zdz_channels, const float* nrm, const float* zdz, double sigma, int tiled,
                              const float* wsum, const float* out_grad, float* col_grad, void* stream)
{
    const char* msg = dn_check(B, H, W, C, zdz_channels, sigma, tiled);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(nrm != nullptr && zdz != nullptr && wsum != nullptr && out_grad != nullptr, "null input");
    GS_CHECK_ARG(col_grad != nullptr, "null output");
    DnArgs a = {};
    a.B = B; a.H = H; a.W = W; a.ZC = zdz_channels; a.TH = DN_TH; a.R = dn_radius(sigma); a.inv2v = (float)(1.0 / (2.0 * sigma * sigma));
    a.col = out_grad; a.nrm = nrm; a.zdz = zdz; a.wsum_in = wsum; a.out = col_grad;
    return dn_launch<true>(C, a, dn_pick_tiled(H, C, a.R, tiled), (hipStream_t)stream);
}
