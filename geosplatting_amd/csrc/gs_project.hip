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

#include "gs_sh_dev.h"

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

static ScanWs project_ws(void* base, int N)
{
    const size_t n_chunks = (size_t)((N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK);
    return scan_ws(base, n_chunks ? n_chunks : 1);
}
extern "C" size_t gs_project_ws_bytes(int N) { return project_ws(nullptr, N).bytes; }

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
    const ScanWs w = project_ws(ws, N);
    if (ws_bytes < w.bytes) { gs_set_error("gs_project_fwd: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(ws, w.bytes, s));
    GS_CHECK_HIP(gs_zero_async(counts, 2 * sizeof(int64_t), s));
    if (N == 0) return GS_OK;
    const int n_chunks = (N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    hipLaunchKernelGGL(project_fwd_kernel, dim3(n_chunks), dim3(GS_PROJ_BLOCK), 0, s, N, means, quats, scales,
                       opacities, colors, D, viewmat, K, W, H, tile_size, tile_w, tile_h, eps2d, near_plane,
                       far_plane, radius_clip, gaussian_ids, radii, means2d, depths, conics, compensations,
                       opacities_packed, colors_packed, tiles_per_gauss, cum_tiles, packed_index, w.ctrl, w.desc,
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
    const ScanWs w = project_ws(ws, N);
    if (ws_bytes < w.bytes) { gs_set_error("gs_project_fwd_vis_ex: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(ws, w.bytes, s));
    GS_CHECK_HIP(gs_zero_async(counts, 2 * sizeof(int64_t), s));
    if (N == 0) return GS_OK;
    const int n_chunks = (N + GS_PROJ_BLOCK - 1) / GS_PROJ_BLOCK;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    auto kern = sh ? (classic ? project_fwd_ex_kernel<true, true> : project_fwd_ex_kernel<true, false>) : project_fwd_ex_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(GS_PROJ_BLOCK), 0, s, N, means, quats, scales, opacities, colors, D, sh_coeffs,
                       sh_K, sh_degree, viewmat, K, W, H, tile_size, tile_w, tile_h, eps2d, near_plane, far_plane, radius_clip,
                       gaussian_ids, radii, means2d, depths, conics, compensations, opacities_packed, colors_packed, tiles_per_gauss,
                       cum_tiles, packed_index, w.ctrl, w.desc, n_chunks, counts, (float4*)vis_records);
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

// ---------------------------------------------------------------------------------------------------
// A7 with the gradient of the view matrix (include/geosplat_hip.h: gs_project_bwd_view).  The per-Gaussian statements are those of
// gs_project_bwd_body.inc -- same thread-per-input-Gaussian mapping, same calls -- written out here because no lane may leave before
// the sum.  Every lane of the workgroup carries twelve numbers, row-major [3][4] = (c_R | c_t), zero unless its Gaussian is visible:
//     c_t = v_mc                       c_R = v_mc m^T + (v_Cc + v_Cc^T) R cov             (mc = R m + t, Cc = R cov R^T)
//     SH, degree >= 1 (dir = m + R^T t):   c_t += R v_dir,   c_R[i][j] += t[i] v_dir[j]
// They come from view_terms_one, an evaluation of the chain OF ITS OWN behind a call that is not inlined: the parameter gradients
// must be the bits of gs_project_bwd_ex, and those depend on how the compiler pairs and contracts the operations of project_bwd_one
// (SLP packing into v_pk_* and the multiply-adds it then can or cannot fuse).  A first version that took v_mc, v_Cc and R cov out of
// the one evaluation changed that pairing and with it the last bits of v_means .. v_scales on the MI355X; behind the call the
// statements below see exactly the operations the other kernels see.  The price is the first two thirds of the chain twice.
// The sum over N is a store-and-sum: fp64 from the wave level up in one fixed tree (gs_wave_sum_f64, then the four waves through LDS
// in wave order), one row of twelve doubles per workgroup in the caller's workspace, and project_view_sum_kernel adds the rows in a
// fixed order and rounds ONCE to fp32.  No float atomics, no arrival order: the same bits every time.
#define GS_VIEW_BLOCK 256
#define GS_VIEW_WAVES (GS_VIEW_BLOCK / 64)
#define GS_VIEW_SUM_LANES 64          // row lanes of the sum kernel: 12 columns x 64 = 768 threads
#define GS_VIEW_SUM_UNROLL 8

struct ViewWs { double* partial; size_t rows, bytes; };
static ViewWs view_ws(void* base, int N)
{
    GsWs w(base, 16);
    ViewWs r;
    r.rows = (size_t)((N + GS_VIEW_BLOCK - 1) / GS_VIEW_BLOCK);
    r.partial = w.take<double>(12 * (r.rows ? r.rows : 1));
    r.bytes = w.bytes();
    return r;
}
extern "C" size_t gs_project_bwd_view_ws_bytes(int N) { return N < 0 ? 0 : view_ws(nullptr, N).bytes; }

struct ViewTerms { float c[12]; };

template <bool SH, bool CLASSIC>
__device__ __noinline__ ViewTerms view_terms_one(const float* __restrict__ viewmat, const float* __restrict__ K, const float* __restrict__ means,
                                                 const float* __restrict__ quats, const float* __restrict__ scales,
                                                 const float* __restrict__ opacities, const float* __restrict__ conics,
                                                 const float* __restrict__ compensations, const float* __restrict__ rec, float v_depth,
                                                 const float* __restrict__ sh_row, int sh_K, int sh_degree, int n, int v, int W, int H,
                                                 float eps2d)
{
#pragma clang fp contract(fast)
    const GsCam cam = load_cam(viewmat, K);
    const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
    const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
    const float scale[3] = { scales[3 * (size_t)n], scales[3 * (size_t)n + 1], scales[3 * (size_t)n + 2] };
    ProjGrad unused;
    ProjViewTerms vt;
    project_bwd_one<true>(cam, mean, q4, scale, CLASSIC ? 0.0f : opacities[n], (float)W, (float)H, eps2d, conics[3 * (size_t)v],
                          conics[3 * (size_t)v + 1], conics[3 * (size_t)v + 2], CLASSIC ? 1.0f : compensations[v], rec[0], rec[1], rec[2],
                          rec[3], rec[4], rec[5], v_depth, unused, &vt);
    ViewTerms o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float s0 = vt.v_Cc[i * 3 + 0] + vt.v_Cc[0 * 3 + i], s1 = vt.v_Cc[i * 3 + 1] + vt.v_Cc[1 * 3 + i],
                    s2 = vt.v_Cc[i * 3 + 2] + vt.v_Cc[2 * 3 + i];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.c[i * 4 + j] = vt.v_mc[i] * mean[j] + (s0 * vt.T1[0 * 3 + j] + s1 * vt.T1[1 * 3 + j] + s2 * vt.T1[2 * 3 + j]);
        o.c[i * 4 + 3] = vt.v_mc[i];
    }
    if constexpr (SH) {
        const float v_rgb[3] = { rec[6], rec[7], rec[8] };
        float vd[3];
        sh_dir_term(cam, mean, sh_row, sh_K, sh_degree, v_rgb, vd);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) o.c[i * 4 + j] += cam.t[i] * vd[j];
            o.c[i * 4 + 3] += cam.R[i * 3 + 0] * vd[0] + cam.R[i * 3 + 1] * vd[1] + cam.R[i * 3 + 2] * vd[2];
        }
    }
    return o;
}

template <bool SH, bool CLASSIC>
__global__ void __launch_bounds__(GS_VIEW_BLOCK)
project_bwd_view_kernel(int N, GsCount vc, int D, const float* __restrict__ means, const float* __restrict__ quats,
                        const float* __restrict__ scales, const float* __restrict__ opacities,
                        const float* __restrict__ viewmat, const float* __restrict__ K, int W, int H, float eps2d,
                        const int32_t* __restrict__ gaussian_ids, const float* __restrict__ conics,
                        const float* __restrict__ compensations, const float* __restrict__ v_packed, int rec_stride,
                        const float* __restrict__ v_depths, const float* __restrict__ sh_coeffs, int sh_K, int sh_degree,
                        float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
                        float* __restrict__ v_opacities, float* __restrict__ v_colors, float* __restrict__ g_sh_coeffs, int accumulate,
                        double* __restrict__ partial)
{
    __shared__ double wave_part[GS_VIEW_WAVES][12];
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    float c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = 0.0f;
    if (n < N) {
        const int V = (int)gs_count(vc);
        const int v = find_slot(gaussian_ids, V, N, n);
        float g_mean[3] = { 0, 0, 0 }, g_quat[4] = { 0, 0, 0, 0 }, g_scale[3] = { 0, 0, 0 }, g_op = 0.0f;
        if (v >= 0) {
            const GsCam cam = load_cam(viewmat, K);
            const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
            const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
            const float scale[3] = { scales[3 * (size_t)n], scales[3 * (size_t)n + 1], scales[3 * (size_t)n + 2] };
            const float* __restrict__ rec = v_packed + (size_t)v * rec_stride;   // {xy(2), conic(3), opacity, colors(D)}
            ProjGrad pg;
            project_bwd_one(cam, mean, q4, scale, CLASSIC ? 0.0f : opacities[n], (float)W, (float)H, eps2d, conics[3 * (size_t)v],
                            conics[3 * (size_t)v + 1], conics[3 * (size_t)v + 2], CLASSIC ? 1.0f : compensations[v], rec[0], rec[1], rec[2],
                            rec[3], rec[4], rec[5], v_depths ? v_depths[v] : 0.0f, pg);
#pragma unroll
            for (int k = 0; k < 3; ++k) { g_mean[k] = pg.mean[k]; g_scale[k] = pg.scale[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) g_quat[k] = pg.quat[k];
            g_op = pg.op;
            if constexpr (SH) {
                const float v_rgb[3] = { rec[6], rec[7], rec[8] };
                sh_color_bwd(cam, mean, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, true, v_rgb,
                             g_sh_coeffs + (size_t)n * sh_K * 3, g_mean);
            }
        } else if constexpr (SH) {
            const GsCam cam = load_cam(viewmat, K);
            const float v_rgb[3] = { 0.f, 0.f, 0.f };
            sh_color_bwd(cam, nullptr, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, false, v_rgb, g_sh_coeffs + (size_t)n * sh_K * 3,
                         g_mean);
        }
        if (accumulate) {
            if (v >= 0) {
                v_means[3 * (size_t)n] += g_mean[0]; v_means[3 * (size_t)n + 1] += g_mean[1]; v_means[3 * (size_t)n + 2] += g_mean[2];
                float4 q = *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n);
                q.x += g_quat[0]; q.y += g_quat[1]; q.z += g_quat[2]; q.w += g_quat[3];
                *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n) = q;
                v_scales[3 * (size_t)n] += g_scale[0]; v_scales[3 * (size_t)n + 1] += g_scale[1]; v_scales[3 * (size_t)n + 2] += g_scale[2];
                v_opacities[n] += g_op;
            }
        } else {
            v_means[3 * (size_t)n] = g_mean[0]; v_means[3 * (size_t)n + 1] = g_mean[1]; v_means[3 * (size_t)n + 2] = g_mean[2];
            *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n) = make_float4(g_quat[0], g_quat[1], g_quat[2], g_quat[3]);
            v_scales[3 * (size_t)n] = g_scale[0]; v_scales[3 * (size_t)n + 1] = g_scale[1]; v_scales[3 * (size_t)n + 2] = g_scale[2];
            v_opacities[n] = g_op;
        }
        if constexpr (!SH) {
            if (v_colors) {
                for (int k = 0; k < D; ++k) v_colors[(size_t)n * D + k] = (v >= 0) ? v_packed[(size_t)v * rec_stride + 6 + k] : 0.0f;
            }
        }
        if (v >= 0) {          // after every store of the parameter gradients: nothing of this reaches the statements above
            const ViewTerms vt = view_terms_one<SH, CLASSIC>(viewmat, K, means, quats, scales, opacities, conics, compensations,
                                                             v_packed + (size_t)v * rec_stride, v_depths ? v_depths[v] : 0.0f,
                                                             SH ? sh_coeffs + (size_t)n * sh_K * 3 : nullptr, sh_K, sh_degree, n, v, W, H,
                                                             eps2d);
#pragma unroll
            for (int k = 0; k < 12; ++k) c[k] = vt.c[k];
        }
    }
    // every lane of the workgroup is here (culled and out-of-range lanes carry zeros)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double s = gs_wave_sum_f64((double)c[k]);
        if (lane == 0) wave_part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double s = wave_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < GS_VIEW_WAVES; ++w) s += wave_part[w][threadIdx.x];
        partial[(size_t)blockIdx.x * 12 + threadIdx.x] = s;
    }
}

// One workgroup of 12 x GS_VIEW_SUM_LANES threads: thread (r, k) adds column k of the rows r, r + 64, r + 128, ... in that order
// (GS_VIEW_SUM_UNROLL independent loads in flight), the 64 row lanes of a column meet in LDS and are added in lane order, and the
// total is rounded once.  The order depends on `rows` alone.  The last row of the 4 x 4 is written as zeros.
__global__ void __launch_bounds__(12 * GS_VIEW_SUM_LANES)
project_view_sum_kernel(const double* __restrict__ partial, long long rows, float* __restrict__ v_viewmat)
{
    __shared__ double lane_part[GS_VIEW_SUM_LANES][12];
    const int k = threadIdx.x % 12, r0 = threadIdx.x / 12;
    double acc = 0.0;
    long long r = r0;
    for (; r + (long long)(GS_VIEW_SUM_UNROLL - 1) * GS_VIEW_SUM_LANES < rows; r += (long long)GS_VIEW_SUM_UNROLL * GS_VIEW_SUM_LANES) {
        double x[GS_VIEW_SUM_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_VIEW_SUM_UNROLL; ++u) x[u] = partial[(size_t)(r + (long long)u * GS_VIEW_SUM_LANES) * 12 + k];
#pragma unroll
        for (int u = 0; u < GS_VIEW_SUM_UNROLL; ++u) acc += x[u];
    }
    for (; r < rows; r += GS_VIEW_SUM_LANES) acc += partial[(size_t)r * 12 + k];
    lane_part[r0][k] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
        double s = 0.0;
        if (threadIdx.x < 12)
            for (int l = 0; l < GS_VIEW_SUM_LANES; ++l) s += lane_part[l][threadIdx.x];
        v_viewmat[threadIdx.x] = (float)s;
    }
}

extern "C" int gs_project_bwd_view(int N, int V, int D, const float* means, const float* quats, const float* scales,
                                   const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                                   const int32_t* gaussian_ids, const float* conics, const float* compensations,
                                   const float* v_packed, int rec_stride, const float* v_depths, const float* sh_coeffs, int sh_K,
                                   int sh_degree, int flags, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                                   float* v_colors, float* g_sh_coeffs, int accumulate, float* v_viewmat, void* ws, size_t ws_bytes,
                                   void* stream)
{
    if (int rc = check_sh_args(D, nullptr, sh_coeffs, sh_K, sh_degree, flags)) return rc;
    const bool sh = sh_degree >= 0, classic = (flags & GS_PROJ_CLASSIC) != 0;
    GS_CHECK_ARG(N >= 0 && V >= 0 && V <= N, "bad sizes");
    GS_CHECK_ARG(v_viewmat != nullptr && ws != nullptr, "v_viewmat/ws must not be NULL");
    if (sh) GS_CHECK_ARG(g_sh_coeffs != nullptr && v_colors == nullptr, "SH colours: g_sh_coeffs given, v_colors NULL");
    const ViewWs w = view_ws(ws, N);
    if (ws_bytes < w.bytes) { gs_set_error("gs_project_bwd_view: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    if (N > 0) {
        auto kern = sh ? (classic ? project_bwd_view_kernel<true, true> : project_bwd_view_kernel<true, false>)
                       : (classic ? project_bwd_view_kernel<false, true> : project_bwd_view_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)w.rows), dim3(GS_VIEW_BLOCK), 0, s, N, GsCount{ V, nullptr }, D, means, quats, scales,
                           opacities, viewmat, K, W, H, eps2d, gaussian_ids, conics, compensations, v_packed,
                           rec_stride > 0 ? rec_stride : ((6 + D) + 15) / 16 * 16, v_depths, sh_coeffs, sh_K, sh_degree, v_means, v_quats,
                           v_scales, v_opacities, v_colors, g_sh_coeffs, accumulate, w.partial);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(project_view_sum_kernel, dim3(1), dim3(12 * GS_VIEW_SUM_LANES), 0, s, w.partial, (long long)w.rows, v_viewmat);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
