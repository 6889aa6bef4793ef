// gs_project.hip -- per-Gaussian stages of the rasterizer half of the path (gfx950):
//   A1  fused projection + cull + anti-alias compensation, packed by a single-pass chained scan
//   A1' opacity*compensation and colour gather (or, for gs_project_fwd_vis_ex, spherical-harmonics colours / 'classic' opacities)
//   A2  tiles-per-Gaussian, inclusive tile cumsum, key/value emission
//   A4  per-tile offsets
//   A7  projection backward + gather backward
// Semantics: gsplat 1.4 `rasterization(packed=True, rasterize_mode='antialiased')` as called by the
// reference at rfstudio/model/gsplat.py:334-355.  All of these stages are
// HBM-bound streaming kernels (44 B in / ~60 B out per Gaussian): one thread per Gaussian, coalesced
// row reads, packed outputs written through an in-launch decoupled look-back scan so that every input
// array is read exactly once.
//
// Floating point: the forward projection is compiled with contraction OFF and spelled in the canonical
// operation order documented in DESIGN.md so that radii / tile ranges / sort keys are bit-exact against
// the CPU oracle.  The backward may contract.
#include "gs_common.h"

#include <stdarg.h>
#include <string.h>

// ---------------------------------------------------------------------------------------------------
// error string (thread-local)
static thread_local char g_err[512] = "";
void gs_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* gs_last_error(void) { return g_err; }
extern "C" int gs_version(void) { return 100; }

#include "gs_project_dev.h"
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------------
// Spherical-harmonics colour of one Gaussian, gsplat 1.4 semantics (rendering.py with sh_degree set, packed, one camera):
//   dir = normalize(mean - campos), campos = inverse(viewmat)[:3, 3] = -R^T t (rigid view matrix),
//   c   = sum_{k < (d+1)^2} basis_k(dir) * coeffs[k, :]   (the real SH basis of 3DGS, gsplat's polynomial "fast" form),
//   rgb = max(c + 0.5, 0).
// Coefficients k >= (d+1)^2 of a row of K are not read.  Degrees 0..3.  A colour, not a sort key: contraction ON here.
__device__ __forceinline__ void sh_campos(const GsCam& cam, float* cp)
{
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

// A1 + A1' (the statements are in gs_project_fwd_body.inc): project_fwd_kernel is the plain instance, project_fwd_ex_kernel<SH, CLASSIC>
// the variants of gs_project_fwd_vis_ex.

__global__ void __launch_bounds__(GS_PROJ_BLOCK)
project_fwd_kernel(int N, const float* __restrict__ means, const float* __restrict__ quats,
                   const float* __restrict__ scales, const float* __restrict__ opacities,
                   const float* __restrict__ colors, int D, const float* __restrict__ viewmat,
                   const float* __restrict__ K, int W, int H, int tile_size, int tile_w, int tile_h,
                   float eps2d, float near_plane, float far_plane, float radius_clip,
                   int32_t* __restrict__ gaussian_ids, int32_t* __restrict__ radii, float* __restrict__ means2d,
                   float* __restrict__ depths, float* __restrict__ conics, float* __restrict__ compensations,
                   float* __restrict__ opacities_packed, float* __restrict__ colors_packed,
                   int32_t* __restrict__ tiles_per_gauss, int64_t* __restrict__ cum_tiles,
                   int32_t* __restrict__ packed_index,
                   unsigned* __restrict__ ctrl, u64* __restrict__ desc, int n_chunks, int64_t* __restrict__ counts, float4* __restrict__ vis)
{
    constexpr bool SH = false, CLASSIC = false;           // the <false, false> instance of project_fwd_ex_kernel
    [[maybe_unused]] const float* const sh_coeffs = nullptr;
    [[maybe_unused]] const int sh_K = 0, sh_degree = -1;
#include "gs_project_fwd_body.inc"
}

template <bool SH, bool CLASSIC>
__global__ void __launch_bounds__(GS_PROJ_BLOCK)
project_fwd_ex_kernel(int N, const float* __restrict__ means, const float* __restrict__ quats,
                      const float* __restrict__ scales, const float* __restrict__ opacities,
                      const float* __restrict__ colors, int D, const float* __restrict__ sh_coeffs, int sh_K, int sh_degree,
                      const float* __restrict__ viewmat,
                      const float* __restrict__ K, int W, int H, int tile_size, int tile_w, int tile_h,
                      float eps2d, float near_plane, float far_plane, float radius_clip,
                      int32_t* __restrict__ gaussian_ids, int32_t* __restrict__ radii, float* __restrict__ means2d,
                      float* __restrict__ depths, float* __restrict__ conics, float* __restrict__ compensations,
                      float* __restrict__ opacities_packed, float* __restrict__ colors_packed,
                      int32_t* __restrict__ tiles_per_gauss, int64_t* __restrict__ cum_tiles,
                      int32_t* __restrict__ packed_index,
                      unsigned* __restrict__ ctrl, u64* __restrict__ desc, int n_chunks, int64_t* __restrict__ counts, float4* __restrict__ vis)
{
#include "gs_project_fwd_body.inc"
}

extern "C" size_t gs_project_ws_bytes(int N)
{
    size_t n_chunks = (size_t)((N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK);
    if (n_chunks == 0) n_chunks = 1;
    return 16 + 4 * n_chunks * sizeof(u64);
}

extern "C" int gs_project_fwd(int N, const float* means, const float* quats, const float* scales,
                              const float* opacities, const float* colors, int D, const float* viewmat,
                              const float* K, int W, int H, int tile_size, float eps2d, float near_plane,
                              float far_plane, float radius_clip, int32_t* gaussian_ids, int32_t* radii,
                              float* means2d, float* depths, float* conics, float* compensations,
                              float* opacities_packed, float* colors_packed, int32_t* tiles_per_gauss,
                              int64_t* cum_tiles, int32_t* packed_index, void* ws, size_t ws_bytes,
                              int64_t* counts, void* stream)
{
    return gs_project_fwd_vis(N, means, quats, scales, opacities, colors, D, viewmat, K, W, H, tile_size, eps2d, near_plane,
                              far_plane, radius_clip, gaussian_ids, radii, means2d, depths, conics, compensations,
                              opacities_packed, colors_packed, tiles_per_gauss, cum_tiles, packed_index, nullptr, ws, ws_bytes,
                              counts, stream);
}

extern "C" int gs_project_fwd_vis(int N, const float* means, const float* quats, const float* scales,
                                  const float* opacities, const float* colors, int D, const float* viewmat,
                                  const float* K, int W, int H, int tile_size, float eps2d, float near_plane,
                                  float far_plane, float radius_clip, int32_t* gaussian_ids, int32_t* radii,
                                  float* means2d, float* depths, float* conics, float* compensations,
                                  float* opacities_packed, float* colors_packed, int32_t* tiles_per_gauss,
                                  int64_t* cum_tiles, int32_t* packed_index, float* vis_records, void* ws, size_t ws_bytes,
                                  int64_t* counts, void* stream)
{
    GS_CHECK_ARG(N >= 0 && W > 0 && H > 0 && tile_size > 0, "bad sizes");
    GS_CHECK_ARG(counts != nullptr && ws != nullptr, "counts/ws must not be NULL");
    GS_CHECK_ARG((colors == nullptr) == (colors_packed == nullptr), "colors and colors_packed go together");
    if (ws_bytes < gs_project_ws_bytes(N)) { gs_set_error("gs_project_fwd: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(ws, gs_project_ws_bytes(N), s));
    GS_CHECK_HIP(gs_zero_async(counts, 2 * sizeof(int64_t), s));
    if (N == 0) return GS_OK;
    const int n_chunks = (N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    unsigned* ctrl = (unsigned*)ws;
    u64* desc = (u64*)((char*)ws + 16);
    hipLaunchKernelGGL(project_fwd_kernel, dim3(n_chunks), dim3(GS_PROJ_BLOCK), 0, s, N, means, quats, scales,
                       opacities, colors, D, viewmat, K, W, H, tile_size, tile_w, tile_h, eps2d, near_plane,
                       far_plane, radius_clip, gaussian_ids, radii, means2d, depths, conics, compensations,
                       opacities_packed, colors_packed, tiles_per_gauss, cum_tiles, packed_index, ctrl, desc,
                       n_chunks, counts, (float4*)vis_records);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// A2 emit: one thread per visible Gaussian.
__global__ void __launch_bounds__(256)
isect_emit_kernel(int V, const float* __restrict__ means2d, const int32_t* __restrict__ radii,
                  const float* __restrict__ depths, const int64_t* __restrict__ cum_tiles, int tile_size,
                  int tile_w, int tile_h, int64_t* __restrict__ isect_ids, int32_t* __restrict__ flatten_ids)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int r = radii[v];
    if (r <= 0) return;
    const float2 m = *reinterpret_cast<const float2*>(means2d + 2 * (size_t)v);
    int x0, y0, x1, y1;
    tile_range_exact(m.x, m.y, r, tile_size, tile_w, tile_h, x0, y0, x1, y1);
    int64_t cur = (v == 0) ? 0 : cum_tiles[v - 1];
    const int64_t depth_enc = (int64_t)(uint32_t)__float_as_int(depths[v]);
    for (int i = y0; i < y1; ++i)
        for (int j = x0; j < x1; ++j) {
            const int64_t tile_id = (int64_t)i * tile_w + j;
            isect_ids[cur] = (tile_id << 32) | depth_enc;
            flatten_ids[cur] = v;
            ++cur;
        }
}

extern "C" int gs_isect_emit(int V, const float* means2d, const int32_t* radii, const float* depths,
                             const int64_t* cum_tiles, int tile_size, int tile_w, int tile_h,
                             int64_t* isect_ids, int32_t* flatten_ids, void* stream)
{
    GS_CHECK_ARG(V >= 0 && tile_size > 0, "bad sizes");
    if (V == 0) return GS_OK;
    hipLaunchKernelGGL(isect_emit_kernel, dim3(gs_cdiv(V, 256)), dim3(256), 0, (hipStream_t)stream, V, means2d,
                       radii, depths, cum_tiles, tile_size, tile_w, tile_h, isect_ids, flatten_ids);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// A4 offsets: offsets[t] = first sorted position whose tile id >= t.
__global__ void __launch_bounds__(256)
isect_offsets_kernel(GsCount nc, const int64_t* __restrict__ ids, int n_tiles, int32_t* __restrict__ offsets)
{
    const int64_t n = gs_count(nc);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0 && i == 0)                                  // (only reachable with a device-side count: the host path memsets)
        for (int t = 0; t < n_tiles; ++t) offsets[t] = 0;
    if (i >= n) return;
    const int cur = (int)(((uint64_t)ids[i]) >> 32);
    if (i == 0) {
        for (int t = 0; t <= cur && t < n_tiles; ++t) offsets[t] = 0;
    } else {
        const int prev = (int)(((uint64_t)ids[i - 1]) >> 32);
        for (int t = prev + 1; t <= cur && t < n_tiles; ++t) offsets[t] = (int32_t)i;
    }
    if (i == n - 1)
        for (int t = cur + 1; t < n_tiles; ++t) offsets[t] = (int32_t)n;
}

// the same from int32 tile ids (gs_isect_bin_tiles_cap)
__global__ void __launch_bounds__(256)
isect_offsets_tiles_kernel(GsCount nc, const int32_t* __restrict__ tiles, int n_tiles, int32_t* __restrict__ offsets)
{
    const int64_t n = gs_count(nc);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0 && i == 0)
        for (int t = 0; t < n_tiles; ++t) offsets[t] = 0;
    if (i >= n) return;
    const int cur = tiles[i];
    if (i == 0) {
        for (int t = 0; t <= cur && t < n_tiles; ++t) offsets[t] = 0;
    } else {
        const int prev = tiles[i - 1];
        for (int t = prev + 1; t <= cur && t < n_tiles; ++t) offsets[t] = (int32_t)i;
    }
    if (i == n - 1)
        for (int t = cur + 1; t < n_tiles; ++t) offsets[t] = (int32_t)n;
}

extern "C" int gs_isect_offsets_tiles_cap(int64_t n_isects_cap, const int64_t* counts_dev, const int32_t* tile_ids_sorted, int n_tiles,
                                          int32_t* offsets, void* stream)
{
    GS_CHECK_ARG(n_isects_cap > 0 && n_tiles > 0 && counts_dev != nullptr && tile_ids_sorted != nullptr, "bad arguments");
    hipLaunchKernelGGL(isect_offsets_tiles_kernel, dim3(gs_cdiv(n_isects_cap, 256)), dim3(256), 0, (hipStream_t)stream,
                       GsCount{ n_isects_cap, (const long long*)counts_dev + 1 }, tile_ids_sorted, n_tiles, offsets);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_isect_offsets(int64_t n_isects, const int64_t* isect_ids_sorted, int n_tiles, int32_t* offsets,
                                void* stream)
{
    GS_CHECK_ARG(n_isects >= 0 && n_tiles > 0, "bad sizes");
    hipStream_t s = (hipStream_t)stream;
    if (n_isects == 0) {
        GS_CHECK_HIP(gs_zero_async(offsets, sizeof(int32_t) * (size_t)n_tiles, s));
        return GS_OK;
    }
    hipLaunchKernelGGL(isect_offsets_kernel, dim3(gs_cdiv(n_isects, 256)), dim3(256), 0, s, GsCount{ n_isects, nullptr },
                       isect_ids_sorted, n_tiles, offsets);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_isect_offsets_cap(int64_t n_isects_cap, const int64_t* counts_dev, const int64_t* isect_ids_sorted, int n_tiles,
                                    int32_t* offsets, void* stream)
{
    GS_CHECK_ARG(n_isects_cap > 0 && n_tiles > 0 && counts_dev != nullptr, "bad sizes");
    hipLaunchKernelGGL(isect_offsets_kernel, dim3(gs_cdiv(n_isects_cap, 256)), dim3(256), 0, (hipStream_t)stream,
                       GsCount{ n_isects_cap, (const long long*)counts_dev + 1 }, isect_ids_sorted, n_tiles, offsets);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// A7: projection backward + gather backward.  One thread per INPUT Gaussian so that the dense [N,*]
// gradients are written coalesced and exactly once (culled Gaussians get zeros, no memset pass); the
// packed slot comes from a binary search in the ascending gaussian_ids list (log2(V) L2-resident probes).
__device__ __forceinline__ int find_slot(const int32_t* __restrict__ gids, int V, int N, int n)
{
    // gids is ascending and holds V of the N indices, so the slot of n lies in [n - (N - V), n]: the search collapses to
    // zero probes when every Gaussian is visible and to log2(N - V + 1) dependent L2 probes otherwise (was log2 V = 21)
    int lo = max(0, n - (N - V)), hi = min(n + 1, V);
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (gids[mid] < n) lo = mid + 1; else hi = mid;
    }
    return (lo < V && gids[lo] == n) ? lo : -1;
}


__global__ void __launch_bounds__(256)
project_bwd_kernel(int N, GsCount vc, int D, const float* __restrict__ means, const float* __restrict__ quats,
                   const float* __restrict__ scales, const float* __restrict__ opacities,
                   const float* __restrict__ viewmat, const float* __restrict__ K, int W, int H, float eps2d,
                   const int32_t* __restrict__ gaussian_ids, const float* __restrict__ conics,
                   const float* __restrict__ compensations, const float* __restrict__ v_packed, int rec_stride,
                   const float* __restrict__ v_depths,
                   float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
                   float* __restrict__ v_opacities, float* __restrict__ v_colors, int accumulate)
{
    constexpr bool SH = false, CLASSIC = false;           // the <false, false> instance of project_bwd_ex_kernel
    [[maybe_unused]] const float* const sh_coeffs = nullptr;
    [[maybe_unused]] float* const g_sh_coeffs = nullptr;
    [[maybe_unused]] const int sh_K = 0, sh_degree = -1;
#include "gs_project_bwd_body.inc"
}

template <bool SH, bool CLASSIC>
__global__ void __launch_bounds__(256)
project_bwd_ex_kernel(int N, GsCount vc, int D, const float* __restrict__ means, const float* __restrict__ quats,
                      const float* __restrict__ scales, const float* __restrict__ opacities,
                      const float* __restrict__ viewmat, const float* __restrict__ K, int W, int H, float eps2d,
                      const int32_t* __restrict__ gaussian_ids, const float* __restrict__ conics,
                      const float* __restrict__ compensations, const float* __restrict__ v_packed, int rec_stride,
                      const float* __restrict__ v_depths, const float* __restrict__ sh_coeffs, int sh_K, int sh_degree,
                      float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
                      float* __restrict__ v_opacities, float* __restrict__ v_colors, float* __restrict__ g_sh_coeffs, int accumulate)
{
#include "gs_project_bwd_body.inc"
}

static int project_bwd_impl(int N, GsCount vc, int D, const float* means, const float* quats, const float* scales,
                            const float* opacities, const float* viewmat, const float* K, int W, int H,
                            float eps2d, const int32_t* gaussian_ids, const float* conics,
                            const float* compensations, const float* v_packed, int rec_stride,
                            const float* v_depths, float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                            int accumulate, void* stream)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(project_bwd_kernel, dim3(gs_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, vc, D, means,
                       quats, scales, opacities, viewmat, K, W, H, eps2d, gaussian_ids, conics, compensations,
                       v_packed, rec_stride > 0 ? rec_stride : ((6 + D) + 15) / 16 * 16, v_depths, v_means, v_quats,
                       v_scales, v_opacities, v_colors, accumulate);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_project_bwd(int N, int V, int D, const float* means, const float* quats, const float* scales,
                              const float* opacities, const float* viewmat, const float* K, int W, int H,
                              float eps2d, const int32_t* gaussian_ids, const float* conics,
                              const float* compensations, const float* v_packed, int rec_stride,
                              const float* v_depths, float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                              int accumulate, void* stream)
{
    GS_CHECK_ARG(N >= 0 && V >= 0 && V <= N, "bad sizes");
    return project_bwd_impl(N, GsCount{ V, nullptr }, D, means, quats, scales, opacities, viewmat, K, W, H, eps2d, gaussian_ids, conics,
                            compensations, v_packed, rec_stride, v_depths, v_means, v_quats, v_scales, v_opacities, v_colors, accumulate,
                            stream);
}

extern "C" int gs_project_bwd_cap(int N, const int64_t* counts_dev, int D, const float* means, const float* quats, const float* scales,
                                  const float* opacities, const float* viewmat, const float* K, int W, int H,
                                  float eps2d, const int32_t* gaussian_ids, const float* conics,
                                  const float* compensations, const float* v_packed, int rec_stride,
                                  const float* v_depths, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                  float* v_colors, int accumulate, void* stream)
{
    GS_CHECK_ARG(N >= 0 && counts_dev != nullptr, "bad sizes");
    return project_bwd_impl(N, GsCount{ N, (const long long*)counts_dev }, D, means, quats, scales, opacities, viewmat, K, W, H, eps2d,
                            gaussian_ids, conics, compensations, v_packed, rec_stride, v_depths, v_means, v_quats, v_scales, v_opacities,
                            v_colors, accumulate, stream);
}

// ---------------------------------------------------------------------------------------------------
// A1 / A7 with spherical-harmonics colours and / or gsplat's 'classic' rasterize mode (include/geosplat_hip.h).
#define GS_PROJ_FLAGS_KNOWN (GS_PROJ_CLASSIC)

static int check_sh_args(int D, const float* colors, const float* sh_coeffs, int sh_K, int sh_degree, int flags)
{
    GS_CHECK_ARG((flags & ~GS_PROJ_FLAGS_KNOWN) == 0, "unknown flags");
    GS_CHECK_ARG(sh_degree >= -1 && sh_degree <= 3, "sh_degree must be -1 (plain colours) or 0..3");
    if (sh_degree >= 0) {
        GS_CHECK_ARG(sh_coeffs != nullptr && colors == nullptr && D == 3, "SH colours: sh_coeffs given, colors NULL, D == 3");
        GS_CHECK_ARG(sh_K >= (sh_degree + 1) * (sh_degree + 1), "sh_K < (sh_degree + 1)^2");
    }
    return GS_OK;
}

extern "C" int gs_project_fwd_vis_ex(int N, const float* means, const float* quats, const float* scales,
                                     const float* opacities, const float* colors, int D, const float* sh_coeffs, int sh_K,
                                     int sh_degree, int flags, const float* viewmat, const float* K, int W, int H, int tile_size,
                                     float eps2d, float near_plane, float far_plane, float radius_clip, int32_t* gaussian_ids,
                                     int32_t* radii, float* means2d, float* depths, float* conics, float* compensations,
                                     float* opacities_packed, float* colors_packed, int32_t* tiles_per_gauss, int64_t* cum_tiles,
                                     int32_t* packed_index, float* vis_records, void* ws, size_t ws_bytes, int64_t* counts,
                                     void* stream)
{
    if (int rc = check_sh_args(D, colors, sh_coeffs, sh_K, sh_degree, flags)) return rc;
    const bool sh = sh_degree >= 0, classic = (flags & GS_PROJ_CLASSIC) != 0;
    if (!sh && !classic)
        return gs_project_fwd_vis(N, means, quats, scales, opacities, colors, D, viewmat, K, W, H, tile_size, eps2d, near_plane,
                                  far_plane, radius_clip, gaussian_ids, radii, means2d, depths, conics, compensations,
                                  opacities_packed, colors_packed, tiles_per_gauss, cum_tiles, packed_index, vis_records, ws,
                                  ws_bytes, counts, stream);
    GS_CHECK_ARG(N >= 0 && W > 0 && H > 0 && tile_size > 0, "bad sizes");
    GS_CHECK_ARG(counts != nullptr && ws != nullptr, "counts/ws must not be NULL");
    if (sh) GS_CHECK_ARG(colors_packed != nullptr, "SH colours need colors_packed [N,3]");
    else    GS_CHECK_ARG((colors == nullptr) == (colors_packed == nullptr), "colors and colors_packed go together");
    if (ws_bytes < gs_project_ws_bytes(N)) { gs_set_error("gs_project_fwd_vis_ex: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(ws, gs_project_ws_bytes(N), s));
    GS_CHECK_HIP(gs_zero_async(counts, 2 * sizeof(int64_t), s));
    if (N == 0) return GS_OK;
    const int n_chunks = (N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    unsigned* ctrl = (unsigned*)ws;
    u64* desc = (u64*)((char*)ws + 16);
    auto kern = sh ? (classic ? project_fwd_ex_kernel<true, true> : project_fwd_ex_kernel<true, false>) : project_fwd_ex_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(GS_PROJ_BLOCK), 0, s, N, means, quats, scales, opacities, colors, D, sh_coeffs,
                       sh_K, sh_degree, viewmat, K, W, H, tile_size, tile_w, tile_h, eps2d, near_plane, far_plane, radius_clip,
                       gaussian_ids, radii, means2d, depths, conics, compensations, opacities_packed, colors_packed, tiles_per_gauss,
                       cum_tiles, packed_index, ctrl, desc, n_chunks, counts, (float4*)vis_records);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_project_bwd_ex(int N, int V, int D, const float* means, const float* quats, const float* scales,
                                 const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                                 const int32_t* gaussian_ids, const float* conics, const float* compensations,
                                 const float* v_packed, int rec_stride, const float* v_depths, const float* sh_coeffs, int sh_K,
                                 int sh_degree, int flags, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                 float* v_colors, float* g_sh_coeffs, int accumulate, void* stream)
{
    if (int rc = check_sh_args(D, nullptr, sh_coeffs, sh_K, sh_degree, flags)) return rc;
    const bool sh = sh_degree >= 0, classic = (flags & GS_PROJ_CLASSIC) != 0;
    if (!sh && !classic)
        return gs_project_bwd(N, V, D, means, quats, scales, opacities, viewmat, K, W, H, eps2d, gaussian_ids, conics, compensations,
                              v_packed, rec_stride, v_depths, v_means, v_quats, v_scales, v_opacities, v_colors, accumulate, stream);
    GS_CHECK_ARG(N >= 0 && V >= 0 && V <= N, "bad sizes");
    if (sh) GS_CHECK_ARG(g_sh_coeffs != nullptr && v_colors == nullptr, "SH colours: g_sh_coeffs given, v_colors NULL");
    if (N == 0) return GS_OK;
    auto kern = sh ? (classic ? project_bwd_ex_kernel<true, true> : project_bwd_ex_kernel<true, false>) : project_bwd_ex_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3(gs_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, GsCount{ V, nullptr }, D, means, quats,
                       scales, opacities, viewmat, K, W, H, eps2d, gaussian_ids, conics, compensations, v_packed,
                       rec_stride > 0 ? rec_stride : ((6 + D) + 15) / 16 * 16, v_depths, sh_coeffs, sh_K, sh_degree, v_means, v_quats,
                       v_scales, v_opacities, v_colors, g_sh_coeffs, accumulate);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
