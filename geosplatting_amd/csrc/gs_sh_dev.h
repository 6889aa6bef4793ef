// gs_sh_dev.h -- spherical-harmonics colours of one Gaussian, forward and backward (device functions shared by the 3DGS projection
// of gs_project.hip and the surfel projection of gs_surfel.hip).  Every function here sets its own contraction mode, so none depends on the
// mode of the file that includes it.
#pragma once
#include "gs_project_dev.h"

// ---------------------------------------------------------------------------------------------------
// Spherical-harmonics colour of one Gaussian, gsplat 1.4 semantics (rendering.py with sh_degree set, packed, one camera):
//   dir = normalize(mean - campos), campos = inverse(viewmat)[:3, 3] = -R^T t (rigid view matrix),
//   c   = sum_{k < (d+1)^2} basis_k(dir) * coeffs[k, :]   (the real SH basis of 3DGS, gsplat's polynomial "fast" form),
//   rgb = max(c + 0.5, 0).
// Coefficients k >= (d+1)^2 of a row of K are not read.  Degrees 0..3.  A colour, not a sort key: contraction ON here.
__device__ __forceinline__ void sh_campos(const GsCam& cam, float* cp)
{
#pragma clang fp contract(off)           // (as both including files had it: the camera position enters the view direction only)
#pragma unroll
    for (int i = 0; i < 3; ++i) cp[i] = -(cam.R[0 * 3 + i] * cam.t[0] + cam.R[1 * 3 + i] * cam.t[1] + cam.R[2 * 3 + i] * cam.t[2]);
}

template <int DEG>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float* b)
{
#pragma clang fp contract(fast)
    b[0] = 0.2820947917738781f;
    if constexpr (DEG >= 1) {
        b[1] = -0.48860251190292f * y; b[2] = 0.48860251190292f * z; b[3] = -0.48860251190292f * x;
    }
    if constexpr (DEG >= 2) {
        const float z2 = z * z, fTmp0B = -1.092548430592079f * z, fC1 = x * x - y * y, fS1 = 2.f * x * y;
        b[4] = 0.5462742152960395f * fS1;
        b[5] = fTmp0B * y;
        b[6] = 0.9461746957575601f * z2 - 0.3153915652525201f;
        b[7] = fTmp0B * x;
        b[8] = 0.5462742152960395f * fC1;
        if constexpr (DEG >= 3) {
            const float fTmp0C = -2.285228997322329f * z2 + 0.4570457994644658f, fTmp1B = 1.445305721320277f * z;
            const float fC2 = x * fC1 - y * fS1, fS2 = x * fS1 + y * fC1;
            b[9] = -0.5900435899266435f * fS2;
            b[10] = fTmp1B * fS1;
            b[11] = fTmp0C * y;
            b[12] = z * (1.865881662950577f * z2 - 1.119528997770346f);
            b[13] = fTmp0C * x;
            b[14] = fTmp1B * fC1;
            b[15] = -0.5900435899266435f * fC2;
        }
    }
}

// v_xyz += sum_k vb[k] * d basis_k / d(x, y, z)  (x, y, z taken as independent: the normalisation is chained by the caller)
template <int DEG>
__device__ __forceinline__ void sh_basis_vjp(float x, float y, float z, const float* vb, float& vx, float& vy, float& vz)
{
#pragma clang fp contract(fast)
    if constexpr (DEG >= 1) {
        const float C1 = 0.48860251190292f;
        vx += -C1 * vb[3]; vy += -C1 * vb[1]; vz += C1 * vb[2];
    }
    if constexpr (DEG >= 2) {
        const float A = 1.092548430592079f, B = 0.5462742152960395f;
        vx += A * y * vb[4] - A * z * vb[7] + 2.f * B * x * vb[8];
        vy += A * x * vb[4] - A * z * vb[5] - 2.f * B * y * vb[8];
        vz += -A * y * vb[5] + 2.f * 0.9461746957575601f * z * vb[6] - A * x * vb[7];
        if constexpr (DEG >= 3) {
            const float E = -0.5900435899266435f, F = 1.445305721320277f, G = -2.285228997322329f, H0 = 0.4570457994644658f;
            const float xx = x * x, yy = y * y, zz = z * z;
            const float fTmp0C = G * zz + H0;
            vx += E * 6.f * x * y * vb[9] + F * 2.f * y * z * vb[10] + fTmp0C * vb[13] + F * 2.f * x * z * vb[14]
                + E * 3.f * (xx - yy) * vb[15];
            vy += E * 3.f * (xx - yy) * vb[9] + F * 2.f * x * z * vb[10] + fTmp0C * vb[11] - F * 2.f * y * z * vb[14]
                - E * 6.f * x * y * vb[15];
            vz += F * 2.f * x * y * vb[10] + 2.f * G * z * y * vb[11] + (3.f * 1.865881662950577f * zz - 1.119528997770346f) * vb[12]
                + 2.f * G * z * x * vb[13] + F * (xx - yy) * vb[14];
        }
    }
}

// the (d+1)^2 * 3 leading floats of a coefficient row; vec: every row starts 16-byte aligned (K * 3 % 4 == 0, aligned base)
template <int NF>
__device__ __forceinline__ void sh_load_row(const float* __restrict__ row, bool vec, float* co)
{
    if (vec) {
#pragma unroll
        for (int i = 0; i < NF / 4; ++i) {
            const float4 q = *reinterpret_cast<const float4*>(row + 4 * i);
            co[4 * i] = q.x; co[4 * i + 1] = q.y; co[4 * i + 2] = q.z; co[4 * i + 3] = q.w;
        }
#pragma unroll
        for (int i = NF / 4 * 4; i < NF; ++i) co[i] = row[i];
    } else {
#pragma unroll
        for (int i = 0; i < NF; ++i) co[i] = row[i];
    }
}

// dir (unnormalised), its unit vector and 1/|dir|
__device__ __forceinline__ void sh_dir(const GsCam& cam, const float* mean, float& x, float& y, float& z, float& inorm)
{
#pragma clang fp contract(fast)
    float cp[3];
    sh_campos(cam, cp);
    const float dx = mean[0] - cp[0], dy = mean[1] - cp[1], dz = mean[2] - cp[2];
    inorm = rsqrtf(dx * dx + dy * dy + dz * dz);
    x = dx * inorm; y = dy * inorm; z = dz * inorm;
}

template <int DEG>
__device__ __forceinline__ void sh_color_deg(float x, float y, float z, const float* co, float* c)
{
#pragma clang fp contract(fast)
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float b[NB];
    sh_basis<DEG>(x, y, z, b);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float acc = b[0] * co[ch];
#pragma unroll
        for (int k = 1; k < NB; ++k) acc += b[k] * co[3 * k + ch];
        c[ch] = acc;                                      // before the + 0.5 and the clamp
    }
}

template <int DEG>
__device__ __forceinline__ void sh_color_row(const GsCam& cam, const float* mean, const float* __restrict__ row, bool vec, float* rgb)
{
    constexpr int NF = (DEG + 1) * (DEG + 1) * 3;
    float co[NF], c[3];
    sh_load_row<NF>(row, vec, co);
    float x = 0.f, y = 0.f, z = 0.f, inorm = 0.f;
    if constexpr (DEG >= 1) sh_dir(cam, mean, x, y, z, inorm);
    sh_color_deg<DEG>(x, y, z, co, c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = fmaxf(c[ch] + 0.5f, 0.0f);
}

__device__ __forceinline__ bool sh_row_vec(const float* sh_coeffs, int sh_K)
{
    return (sh_K * 3) % 4 == 0 && (reinterpret_cast<uintptr_t>(sh_coeffs) & 15) == 0;
}

__device__ __forceinline__ void sh_color(const GsCam& cam, const float* mean, const float* __restrict__ row, int sh_K, int degree,
                                         float* rgb)
{
    const bool vec = sh_row_vec(row, sh_K);
    switch (degree) {
    case 0:  sh_color_row<0>(cam, mean, row, vec, rgb); break;
    case 1:  sh_color_row<1>(cam, mean, row, vec, rgb); break;
    case 2:  sh_color_row<2>(cam, mean, row, vec, rgb); break;
    default: sh_color_row<3>(cam, mean, row, vec, rgb); break;
    }
}

// Backward of one Gaussian's SH colour: v_rgb = the compositor's colour gradient.  Writes the whole coefficient row
// g_row[K * 3] (basis_k * v_c where the clamp passed -- torch's clamp_min rule, c + 0.5 >= 0 -- zero for k >= (d+1)^2) and adds the
// direction term (chained through the normalisation) to v_mean.  visible == false writes a zero row.
template <int DEG>
__device__ __forceinline__ void sh_color_bwd_row(const GsCam& cam, const float* mean, const float* __restrict__ row, int sh_K, bool vec,
                                                 bool visible, const float* v_rgb, float* __restrict__ g_row, float* v_mean)
{
#pragma clang fp contract(fast)
    constexpr int NB = (DEG + 1) * (DEG + 1), NF = NB * 3;
    float g[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) g[i] = 0.0f;
    if (visible) {
        float co[NF], c[3], b[NB];
        sh_load_row<NF>(row, vec, co);
        float x = 0.f, y = 0.f, z = 0.f, inorm = 0.f;
        if constexpr (DEG >= 1) sh_dir(cam, mean, x, y, z, inorm);
        sh_color_deg<DEG>(x, y, z, co, c);
        sh_basis<DEG>(x, y, z, b);
        float vc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) vc[ch] = (c[ch] + 0.5f >= 0.0f) ? v_rgb[ch] : 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) g[3 * k + ch] = b[k] * vc[ch];
        if constexpr (DEG >= 1) {
            float vb[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) vb[k] = co[3 * k] * vc[0] + co[3 * k + 1] * vc[1] + co[3 * k + 2] * vc[2];
            float vx = 0.f, vy = 0.f, vz = 0.f;
            sh_basis_vjp<DEG>(x, y, z, vb, vx, vy, vz);
            const float dotp = vx * x + vy * y + vz * z;
            v_mean[0] += (vx - dotp * x) * inorm;
            v_mean[1] += (vy - dotp * y) * inorm;
            v_mean[2] += (vz - dotp * z) * inorm;
        }
    }
    const int nf = sh_K * 3;
    if (vec) {
#pragma unroll
        for (int i = 0; i < NF / 4; ++i)
            *reinterpret_cast<float4*>(g_row + 4 * i) = make_float4(g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]);
#pragma unroll
        for (int i = NF / 4 * 4; i < NF; ++i) g_row[i] = g[i];
        int i = NF;
        for (; i < nf && (i & 3); ++i) g_row[i] = 0.0f;
        for (; i + 4 <= nf; i += 4) *reinterpret_cast<float4*>(g_row + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        for (; i < nf; ++i) g_row[i] = 0.0f;
    } else {
#pragma unroll
        for (int i = 0; i < NF; ++i) g_row[i] = g[i];
        for (int i = NF; i < nf; ++i) g_row[i] = 0.0f;
    }
}

__device__ __forceinline__ void sh_color_bwd(const GsCam& cam, const float* mean, const float* __restrict__ row, int sh_K, int degree,
                                             bool visible, const float* v_rgb, float* __restrict__ g_row, float* v_mean)
{
    const bool vec = sh_row_vec(row, sh_K) && (reinterpret_cast<uintptr_t>(g_row) & 15) == 0;
    switch (degree) {
    case 0:  sh_color_bwd_row<0>(cam, mean, row, sh_K, vec, visible, v_rgb, g_row, v_mean); break;
    case 1:  sh_color_bwd_row<1>(cam, mean, row, sh_K, vec, visible, v_rgb, g_row, v_mean); break;
    case 2:  sh_color_bwd_row<2>(cam, mean, row, sh_K, vec, visible, v_rgb, g_row, v_mean); break;
    default: sh_color_bwd_row<3>(cam, mean, row, sh_K, vec, visible, v_rgb, g_row, v_mean); break;
    }
}

// The direction term of sh_color_bwd_row BY ITSELF (gs_project_bwd_view: the gradient of the view matrix needs it apart from v_mean):
// v_dir = d(sum_ch v_rgb[ch] * rgb[ch]) / d(mean - campos), chained through the normalisation; 0 for degree 0.  An evaluation of its
// own -- nothing is shared with sh_color_bwd_row, whose instructions, and so the bits of v_mean and g_row, stay what they are.
template <int DEG>
__device__ __forceinline__ void sh_dir_term_row(const GsCam& cam, const float* mean, const float* __restrict__ row, bool vec,
                                                const float* v_rgb, float* v_dir)
{
#pragma clang fp contract(fast)
    v_dir[0] = v_dir[1] = v_dir[2] = 0.0f;
    if constexpr (DEG >= 1) {
        constexpr int NB = (DEG + 1) * (DEG + 1), NF = NB * 3;
        float co[NF], c[3], vb[NB], vc[3];
        sh_load_row<NF>(row, vec, co);
        float x, y, z, inorm;
        sh_dir(cam, mean, x, y, z, inorm);
        sh_color_deg<DEG>(x, y, z, co, c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) vc[ch] = (c[ch] + 0.5f >= 0.0f) ? v_rgb[ch] : 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) vb[k] = co[3 * k] * vc[0] + co[3 * k + 1] * vc[1] + co[3 * k + 2] * vc[2];
        float vx = 0.f, vy = 0.f, vz = 0.f;
        sh_basis_vjp<DEG>(x, y, z, vb, vx, vy, vz);
        const float dotp = vx * x + vy * y + vz * z;
        v_dir[0] = (vx - dotp * x) * inorm;
        v_dir[1] = (vy - dotp * y) * inorm;
        v_dir[2] = (vz - dotp * z) * inorm;
    }
}

__device__ __forceinline__ void sh_dir_term(const GsCam& cam, const float* mean, const float* __restrict__ row, int sh_K, int degree,
                                            const float* v_rgb, float* v_dir)
{
    const bool vec = sh_row_vec(row, sh_K);
    switch (degree) {
    case 0:  sh_dir_term_row<0>(cam, mean, row, vec, v_rgb, v_dir); break;
    case 1:  sh_dir_term_row<1>(cam, mean, row, vec, v_rgb, v_dir); break;
    case 2:  sh_dir_term_row<2>(cam, mean, row, vec, v_rgb, v_dir); break;
    default: sh_dir_term_row<3>(cam, mean, row, vec, v_rgb, v_dir); break;
    }
}
