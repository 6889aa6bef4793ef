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
