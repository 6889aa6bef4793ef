/*
 * geosplat_hip.h -- C-ABI of libgeosplat_hip.so: the MI355X (gfx950) implementation of the
 * GeoSplatting render-and-backward hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. the PyTorch-ROCm allocator) unless the
 *     parameter is documented "host"; all tensors are contiguous fp32 / int32 / int64 as noted;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream);
 *   - no allocation, no host synchronisation and no exceptions inside; every call returns 0 on success or
 *     a negative GS_E* code, with a message available from gs_last_error() (thread-local);
 *   - data-dependent sizes (V visible Gaussians, I tile intersections) are produced ON THE DEVICE in
 *     `counts[2]`; the caller reads them (one 16-byte copy) before sizing the I-length buffers, exactly
 *     where the reference's upstream performs its own host sync.
 *
 * Reference interfaces replaced (file:line relative to /root/reference):
 *   gs_project_fwd / gs_isect_emit / gs_isect_sort / gs_isect_offsets / gs_raster_fwd
 *        = the stages executed by `gsplat.rasterization(...)` as called at
 *          rfstudio/model/gsplat.py:334-355 (also :240-261, :151-172; rfstudio/model/geosplat.py:276-295)
 *   gs_raster_bwd / gs_project_bwd
 *        = the autograd backward of that call, reached from rfstudio/optim/optimizer.py:107
 *   gs_project_fwd_vis_ex / gs_project_bwd_ex
 *        = the same stages with spherical-harmonics colours and rasterize_mode='classic', as GSplatter calls
 *          gsplat.rasterization (rfstudio/model/gsplat.py:23-36, :209-214, :304-309)
 *   gs_shade_fwd / gs_shade_bwd
 *        = RenderableAttrs.splat arithmetic rfstudio/model/geosplat.py:80-122 including the two
 *          `dr.texture` calls (:93-98 and rfstudio/graphics/_mesh/_texture.py:596-611)
 *   gs_tonemap_fwd / gs_tonemap_bwd
 *        = _tone_mapping_naive / _tone_mapping_aces rfstudio/model/geosplat.py:474-480
 *   gs_cubemap_mip_fwd, gs_cube_sample_linear, gs_diffuse_cubemap_fwd/_bwd, gs_specular_bounds,
 *   gs_specular_cubemap_fwd/_bwd
 *        = the pybind entry points diffuse_cubemap_fwd/bwd, specular_bounds, specular_cubemap_fwd/bwd
 *          (rfstudio/graphics/_mesh/_splitsum/c_src/torch_bindings.cpp:265-271) and _CubeMapMip
 *          (rfstudio/graphics/_mesh/_texture.py:199-226)
 *   gs_env_cube_to_latlng_fwd/_bwd, gs_env_latlng_to_cube_fwd/_bwd, gs_cube_sample_linear_bwd, gs_env_background_fwd
 *        = TextureCubeMap.as_latlng / sample / render and TextureLatLng.as_cubemap (rfstudio/graphics/_mesh/_texture.py:359-377,
 *          :411-465)
 */
#ifndef GEOSPLAT_HIP_H
#define GEOSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK            0
#define GS_EINVAL       -1   /* bad argument */
#define GS_ENOSPC       -2   /* workspace too small */
#define GS_ELAUNCH      -3   /* HIP launch / runtime error */

#define GS_MAX_LEVELS   16   /* maximum mip levels of the split-sum pyramid */
#define GS_MAX_CHANNELS 32   /* maximum colour channels D of the compositor */

/* shading modes of RenderableAttrs.splat (rfstudio/model/geosplat.py:62) */
#define GS_MODE_PBR      0
#define GS_MODE_DIFFUSE  1
#define GS_MODE_SPECULAR 2
/* tone mapping (rfstudio/model/geosplat.py:63) */
#define GS_TONE_NONE     0
#define GS_TONE_NAIVE    1
#define GS_TONE_ACES     2

/* term kinds of gs_smooth_loss */
#define GS_SMOOTH_NONE   0
#define GS_SMOOTH_EDGE   1
#define GS_SMOOTH_TV     2

const char* gs_last_error(void);
int         gs_version(void);

/* ------------------------------------------------------------------ A1 + A1' + A2(count) ---------- */
/* Bytes of scratch gs_project_fwd needs for its single-pass chained scan (zeroed by the call itself). */
size_t gs_project_ws_bytes(int N);

/* Fused projection + cull + anti-alias compensation + packed compaction (ascending Gaussian index)
 * + opacity*compensation + colour gather + tiles-per-Gaussian + inclusive tile cumsum.
 * Packed outputs need capacity N.  counts[0] = V, counts[1] = I (int64).
 * colors / colors_packed may both be NULL (D ignored).  packed_index[N] (nullable) receives the packed
 * slot of every Gaussian or -1.  viewmat: row-major 4x4 world->camera (OpenCV), K: row-major 3x3. */
int gs_project_fwd(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                   const float* colors, int D, const float* viewmat, const float* K, int W, int H, int tile_size,
                   float eps2d, float near_plane, float far_plane, float radius_clip,
                   int32_t* gaussian_ids, int32_t* radii, float* means2d, float* depths, float* conics,
                   float* compensations, float* opacities_packed, float* colors_packed,
                   int32_t* tiles_per_gauss, int64_t* cum_tiles, int32_t* packed_index,
                   void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* The same, additionally writing the compositor's 64-byte per-visible records {mx,my,a/2,b | c/2,opacity,hx,hy | c0,c1,c2,- | pad}
 * (vis_records [N,16] floats, nullable) straight from the projection's registers; gs_raster_prepare_vis then skips its own packing
 * pass.  Colours travel in the record for D <= 3. */
int gs_project_fwd_vis(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                       const float* colors, int D, const float* viewmat, const float* K, int W, int H, int tile_size,
                       float eps2d, float near_plane, float far_plane, float radius_clip,
                       int32_t* gaussian_ids, int32_t* radii, float* means2d, float* depths, float* conics,
                       float* compensations, float* opacities_packed, float* colors_packed,
                       int32_t* tiles_per_gauss, int64_t* cum_tiles, int32_t* packed_index, float* vis_records,
                       void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* gsplat 1.4 `rasterization(..., sh_degree=d, rasterize_mode='classic')`, packed, one camera: the configuration of the reference's
 * GSplatter (rfstudio/model/gsplat.py:23-36; colours assembled at :209-214 and :304-309, trained by
 * rfstudio/trainer/gsplat_trainer.py).  gs_project_fwd_vis plus two options:
 *   sh_degree in 0..3: colours from spherical harmonics.  sh_coeffs [N, sh_K, 3], sh_K >= (sh_degree+1)^2 (coefficients beyond are
 *     ignored), colors must be NULL and D == 3; for every VISIBLE Gaussian, dir = normalize(mean - campos) with
 *     campos = inverse(viewmat)[:3, 3], c = sum_k basis_k(dir) * coeffs[k] (the real SH basis of 3DGS in gsplat's polynomial form),
 *     colors_packed [N,3] (required) and the records receive max(c + 0.5, 0).  sh_degree == -1: plain colours as before.
 *   flags & GS_PROJ_CLASSIC: opacities_packed = opacities[g] (no anti-alias compensation factor); the eps2d blur, radii, culling
 *     and tile counts are unchanged, compensations is still written.
 * With sh_degree == -1 and flags == 0 this is gs_project_fwd_vis. */
#define GS_PROJ_CLASSIC 1
int gs_project_fwd_vis_ex(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                          const float* colors, int D, const float* sh_coeffs, int sh_K, int sh_degree, int flags,
                          const float* viewmat, const float* K, int W, int H, int tile_size,
                          float eps2d, float near_plane, float far_plane, float radius_clip,
                          int32_t* gaussian_ids, int32_t* radii, float* means2d, float* depths, float* conics,
                          float* compensations, float* opacities_packed, float* colors_packed,
                          int32_t* tiles_per_gauss, int64_t* cum_tiles, int32_t* packed_index, float* vis_records,
                          void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* ------------------------------------------------------------------ A2 (emit) ---------------------- */
/* isect_ids[i] = (tile_id << 32) | float_bits(depth), flatten_ids[i] = packed index; emission order =
 * ascending packed index, tiles row-major. */
int gs_isect_emit(int V, const float* means2d, const int32_t* radii, const float* depths,
                  const int64_t* cum_tiles, int tile_size, int tile_w, int tile_h,
                  int64_t* isect_ids, int32_t* flatten_ids, void* stream);

/* ------------------------------------------------------------------ A2 + A3 (depth-major binning) -- */
/* The sorted intersection list straight from the projection outputs, WITHOUT emitting the unsorted keys: the Gaussians are
 * ordered by depth once (V-sized), their intersections are emitted in that order as (tile, index) items and two stable
 * passes over the tile bits finish the (tile | depth | packed index) order -- bit-identical to gs_isect_emit + gs_isect_sort
 * (csrc/gs_sort.hip).  tiles_per_gauss [V] and n_isects (= their sum) come from gs_project_fwd. */
size_t gs_isect_bin_ws_bytes(int V, int64_t n_isects, int tile_w, int tile_h);
int gs_isect_bin(int V, const float* means2d, const int32_t* radii, const float* depths, const int32_t* tiles_per_gauss,
                 int64_t n_isects, int tile_size, int tile_w, int tile_h, int64_t* isect_ids_sorted,
                 int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ A3 ----------------------------- */
size_t gs_sort_ws_bytes(int64_t n_isects, int tile_w, int tile_h);
/* Stable ascending sort of (isect_ids, flatten_ids) over the 32 + tile_bits significant key bits. */
int gs_isect_sort(int64_t n_isects, const int64_t* isect_ids, const int32_t* flatten_ids,
                  int64_t* isect_ids_sorted, int32_t* flatten_ids_sorted, int tile_w, int tile_h,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ A4 ----------------------------- */
/* offsets[t] = first sorted position whose tile id >= t  (t in [0, n_tiles)). */
int gs_isect_offsets(int64_t n_isects, const int64_t* isect_ids_sorted, int n_tiles, int32_t* offsets,
                     void* stream);

/* ------------------------------------------------------------------ A5 / A6 ------------------------ */
/* Bytes of the compositor workspace: the per-intersection record stream in sorted order (48 B each) plus the
 * longest-first tile order.  gs_raster_fwd WRITES it, gs_raster_bwd READS it (keep it alive in between). */
size_t gs_raster_ws_bytes(int64_t n_isects, int V, int W, int H, int tile_size);

/* Front-to-back alpha compositing of the per-tile sorted lists.  colors: packed [V,D]; opacities: packed
 * (already multiplied by the compensation); background: nullable [D].
 * render [H,W,D], alphas [H,W], last_ids [H,W] (index into the sorted list of the last composited entry). */
int gs_raster_fwd(int W, int H, int tile_size, int D, int V, const float* means2d, const float* conics,
                  const float* opacities, const float* colors, const float* background,
                  int64_t n_isects, const int32_t* offsets, const int32_t* flatten_ids,
                  float* render, float* alphas, int32_t* last_ids, void* ws, size_t ws_bytes, void* stream);

/* The two halves of gs_raster_fwd for a caller that spreads a view over several streams: gs_raster_prepare fills
 * the workspace (per-visible records, sorted record stream, tile order: HBM-bound), gs_raster_composite runs the
 * compositor on it (VALU-bound).  gs_raster_fwd == prepare followed by composite on one stream. */
int gs_raster_prepare(int W, int H, int tile_size, int D, int V, const float* means2d, const float* conics,
                      const float* opacities, const float* colors, int64_t n_isects, const int32_t* offsets,
                      const int32_t* flatten_ids, void* ws, size_t ws_bytes, void* stream);
int gs_raster_prepare_vis(int W, int H, int tile_size, int D, int V, const float* vis_records /* gs_project_fwd_vis */,
                          int64_t n_isects, const int32_t* offsets, const int32_t* flatten_ids, void* ws, size_t ws_bytes,
                          void* stream);
int gs_raster_composite(int W, int H, int tile_size, int D, int V, const float* colors, const float* background,
                        int64_t n_isects, const int32_t* offsets, float* render, float* alphas, int32_t* last_ids,
                        const void* ws, size_t ws_bytes, void* stream);

/* Floats per packed per-Gaussian gradient record written by gs_raster_bwd: (6 + D) rounded up to 16. */
int gs_raster_grad_stride(int D);

/* Stored-state backward (uses alphas + last_ids + the workspace of the forward).  The per-visible-Gaussian
 * gradients come out as ONE packed record per Gaussian (one or two cache lines, so the 6+D fp32 atomics of a
 * survivor merge into 1-2 memory-side requests):
 *     v_packed[g*stride + 0..1] = v_means2d   [2..4] = v_conics   [5] = v_opacities   [6..6+D) = v_colors
 * with stride = gs_raster_grad_stride(D); the buffer [V*stride] is zeroed by the call.  colors is only read when
 * D > 3 (for D <= 3 the colours travel inside the record stream). */
int gs_raster_bwd(int W, int H, int tile_size, int D, int V, const float* colors, const float* background,
                  int64_t n_isects, const int32_t* offsets, const float* alphas, const int32_t* last_ids,
                  const float* v_render, const float* v_alphas, float* v_packed, const void* ws, size_t ws_bytes,
                  void* stream);

/* The compositor backward alone: ADDS into a v_packed the caller has zeroed (or that already holds another view's
 * packed gradients of the same visible set); same arguments. */
int gs_raster_bwd_acc(int W, int H, int tile_size, int D, int V, const float* colors, const float* background,
                      int64_t n_isects, const int32_t* offsets, const float* alphas, const int32_t* last_ids,
                      const float* v_render, const float* v_alphas, float* v_packed, const void* ws, size_t ws_bytes,
                      void* stream);

/* ------------------------------------------------------------------ capacity protocol --- */
/* The data-dependent sizes of a view -- V visible Gaussians, I tile intersections -- exist only on the device after
 * gs_project_fwd (counts = {V, I}, int64).  The entry points above take them as host scalars (gsplat's call shape: one
 * read-back per view).  The *_cap variants below take CAPACITIES instead: V_cap (N always suffices) and n_isects_cap size
 * the buffers, the workspaces and the launch grids; every kernel reads the actual count from counts_dev and clamps it to
 * the capacity.  No host synchronisation, fixed launch shapes (capturable in a hipGraph).  If a view needs more than
 * n_isects_cap, gs_isect_bin_cap sets status_dev = {GS_ENOSPC, max required n_isects, max required V} (int64[3], zeroed once by
 * the caller, sticky) and that view is composited from the first n_isects_cap intersections in emission order: memory-safe,
 * wrong image -- the caller polls status_dev at a convenient point (the engine: start of the next step), grows the capacity
 * and repeats the step.  Workspace sizes: the *_ws_bytes functions with the capacities. */
int gs_isect_bin_cap(int V_cap, const float* means2d, const int32_t* radii, const float* depths, const int64_t* counts_dev,
                     int64_t n_isects_cap, int tile_size, int tile_w, int tile_h, int64_t* isect_ids_sorted,
                     int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream);
int gs_isect_offsets_cap(int64_t n_isects_cap, const int64_t* counts_dev, const int64_t* isect_ids_sorted, int n_tiles,
                         int32_t* offsets, void* stream);
/* The pair for a caller that only composites (the step engine never returns `meta`): the binning without the 64-bit isect_ids -- the
 * last pass writes int32 tile ids instead (8 bytes per intersection instead of 12, no depth gather) -- and the tile offsets from
 * those.  flatten_ids_sorted / offsets are bit-identical to gs_isect_bin_cap + gs_isect_offsets_cap. */
int gs_isect_bin_tiles_cap(int V_cap, const float* means2d, const int32_t* radii, const float* depths, const int64_t* counts_dev,
                           int64_t n_isects_cap, int tile_size, int tile_w, int tile_h, int32_t* tile_ids_sorted,
                           int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream);
int gs_isect_offsets_tiles_cap(int64_t n_isects_cap, const int64_t* counts_dev, const int32_t* tile_ids_sorted, int n_tiles,
                               int32_t* offsets, void* stream);
int gs_raster_prepare_vis_cap(int W, int H, int tile_size, int D, int V_cap, const float* vis_records, int64_t n_isects_cap,
                              const int64_t* counts_dev, const int32_t* offsets, const int32_t* flatten_ids, void* ws,
                              size_t ws_bytes, void* stream);
int gs_raster_composite_cap(int W, int H, int tile_size, int D, int V_cap, const float* colors, const float* background,
                            int64_t n_isects_cap, const int64_t* counts_dev, const int32_t* offsets, float* render,
                            float* alphas, int32_t* last_ids, const void* ws, size_t ws_bytes, void* stream);
int gs_raster_bwd_cap(int W, int H, int tile_size, int D, int V_cap, const float* colors, const float* background,
                      int64_t n_isects_cap, const int64_t* counts_dev, const int32_t* offsets, const float* alphas,
                      const int32_t* last_ids, const float* v_render, const float* v_alphas, float* v_packed, const void* ws,
                      size_t ws_bytes, void* stream);
/* gs_raster_bwd_acc with the counts on the device: ADDS into a v_packed [V_cap, stride] the caller has zeroed (the engine
 * zeroes it on its front stream, under the compositor of the previous view). */
int gs_raster_bwd_acc_cap(int W, int H, int tile_size, int D, int V_cap, const float* colors, const float* background,
                          int64_t n_isects_cap, const int64_t* counts_dev, const int32_t* offsets, const float* alphas,
                          const int32_t* last_ids, const float* v_render, const float* v_alphas, float* v_packed, const void* ws,
                          size_t ws_bytes, void* stream);
/* The compositor with S4 (tone mapping, rfstudio/model/geosplat.py:123-133) inside, D = 3 and no background -- what
 * RenderableAttrs.splat runs between `rasterization` and the loss (rfstudio/model/geosplat.py:108-133): the forward also writes
 * image[P,4] = tonemap(render * exposure | alpha) (= gs_tonemap_fwd3 on its outputs, bit-identical), the backward takes the image
 * cotangent v_image[P,4] instead of v_render / v_alphas (= gs_tonemap_bwd3 + gs_raster_bwd_acc) and ADDS the exposure gradient to
 * the device scalar v_exposure.  Two dependent launches fewer per view on the step's critical stream.  counts_dev == NULL: V and
 * n_isects are exact; otherwise they are capacities and {V, I} are read on the device (capacity protocol). */
int gs_raster_composite_tone(int W, int H, int tile_size, int V, const float* colors, int64_t n_isects,
                             const int64_t* counts_dev, const int32_t* offsets, float* render, float* alphas,
                             int32_t* last_ids, int tone_mode, const float* exposure /*device scalar*/, float* image,
                             const void* ws, size_t ws_bytes, void* stream);
int gs_raster_bwd_tone_acc(int W, int H, int tile_size, int V, const float* colors, int64_t n_isects,
                           const int64_t* counts_dev, const int32_t* offsets, const float* render, const float* alphas,
                           const int32_t* last_ids, int tone_mode, const float* exposure, const float* v_image,
                           float* v_packed, float* v_exposure, const void* ws, size_t ws_bytes, void* stream);
/* The same pair with a CULL LOG between them: the forward appends {stream index, pixel mask} of every record that entered one of its
 * dense batches (per tile quadrant, in stream order) to log_ws (gs_raster_log_ws_bytes; written by the forward, read by the backward of
 * the SAME view), and the backward walks that log from its end instead of repeating the forward's cull and ellipse masks.  Same image
 * bit for bit, same gradients up to the order of the float atomics.  The forward also files every tile, by its longest quadrant
 * log, in bucket lists inside `ws` -- the order in which the backward launches its tiles; the lists are cleared by gs_raster_prepare*,
 * so they are used when exactly ONE forward ran on the prepared workspace (otherwise the backward falls back to the forward's order). */
size_t gs_raster_log_ws_bytes(int64_t n_isects, int W, int H, int tile_size);
int gs_raster_composite_tone_log(int W, int H, int tile_size, int V, const float* colors, int64_t n_isects,
                                 const int64_t* counts_dev, const int32_t* offsets, float* render, float* alphas,
                                 int32_t* last_ids, int tone_mode, const float* exposure, float* image, const void* ws,
                                 size_t ws_bytes, void* log_ws, size_t log_bytes, void* stream);
int gs_raster_bwd_tone_log_acc(int W, int H, int tile_size, int V, const float* colors, int64_t n_isects,
                               const int64_t* counts_dev, const int32_t* offsets, const float* render, const float* alphas,
                               const int32_t* last_ids, int tone_mode, const float* exposure, const float* v_image,
                               float* v_packed, float* v_exposure, const void* ws, size_t ws_bytes, const void* log_ws,
                               size_t log_bytes, void* stream);
int gs_project_bwd_cap(int N, const int64_t* counts_dev, int D, const float* means, const float* quats, const float* scales,
                       const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                       const int32_t* gaussian_ids, const float* conics, const float* compensations, const float* v_packed,
                       int rec_stride, const float* v_depths, float* v_means, float* v_quats, float* v_scales,
                       float* v_opacities, float* v_colors, int accumulate, void* stream);

/* Self-test of the compositor's reciprocal (hardware v_rcp_f32 + Newton + Markstein correction, which replaces the IEEE
 * division 1 / (1 - alpha) of gsplat's rasterize_to_pixels backward): *mismatches_dev (device uint64) = number of floats
 * with bit patterns in [lo_bits, hi_bits] whose result differs from the correctly rounded quotient (counted twice, once
 * per packed component).  Test hook; no reference counterpart. */
int gs_selftest_rcp(uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches_dev, void* stream);

/* Self-test of the compositor's canonical exponential exp(-sigma) (one spelled-out operation order instead of gsplat's
 * hardware `__expf`, so that the CPU oracle reproduces it bit for bit): over every float with bit pattern in
 * [lo_bits, hi_bits], out_dev[0] (device uint64) = sum_i bits(result_i) * (2 i + 1) mod 2^64 -- an order-independent checksum the
 * oracle computes from its own copy -- and out_dev[1] = the bit pattern of the largest relative error (a double) against the
 * float64 exponential.  Test hook; no reference counterpart. */
int gs_selftest_exp(uint32_t lo_bits, uint32_t hi_bits, uint64_t* out_dev, void* stream);

/* Self-test of the cube-map edge table (csrc/gs_cube.h): the texel across a face edge is looked up in a 24-entry integer table
 * instead of being re-projected in floating point as oracle/gs_oracle_shade.c defines it; *mismatches_dev (device uint64) = number
 * of (face, edge, position) triples of an R x R face, R <= 2048, for which the two disagree.  Test hook; no reference counterpart. */
int gs_selftest_cube_edges(int R, uint64_t* mismatches_dev, void* stream);

/* ------------------------------------------------------------------ A7 ----------------------------- */
/* Projection backward + gather backward from the packed records of gs_raster_bwd; dense outputs [N,*] are fully
 * written (zeros for culled Gaussians) -- no caller-side zeroing needed -- or, with accumulate != 0, ADDED to
 * v_means / v_quats / v_scales / v_opacities (several views per step share one gradient buffer; v_colors is always
 * written).  v_depths nullable. */
int gs_project_bwd(int N, int V, int D, const float* means, const float* quats, const float* scales,
                   const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                   const int32_t* gaussian_ids, const float* conics, const float* compensations,
                   const float* v_packed, int rec_stride /* 0 = gs_raster_grad_stride(D) */, const float* v_depths,
                   float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                   int accumulate, void* stream);

/* gs_project_bwd for gs_project_fwd_vis_ex's options (the same sh_coeffs / sh_K / sh_degree / flags as the forward):
 *   sh_degree in 0..3: D == 3 (the record's colour gradient), v_colors must be NULL and g_sh_coeffs [N, sh_K, 3] is fully written
 *     (never accumulated): basis_k(dir) * v_c where the clamp passed (c + 0.5 >= 0, torch's clamp_min rule), 0 for k >= (d+1)^2,
 *     for clamped channels and for culled Gaussians; the direction term goes through the normalisation into v_means.
 *   flags & GS_PROJ_CLASSIC: v_opacities = v_opacity_packed, and the compensation contributes no gradient to the covariance.
 * With sh_degree == -1 and flags == 0 this is gs_project_bwd. */
int gs_project_bwd_ex(int N, int V, int D, const float* means, const float* quats, const float* scales,
                      const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                      const int32_t* gaussian_ids, const float* conics, const float* compensations,
                      const float* v_packed, int rec_stride, const float* v_depths, const float* sh_coeffs, int sh_K,
                      int sh_degree, int flags, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                      float* v_colors, float* g_sh_coeffs, int accumulate, void* stream);

/* gs_project_bwd_ex that also returns the gradient of the view matrix (upstream's v_viewmats; camera-pose refinement): plain colours,
 * sh_degree 0..3 and GS_PROJ_CLASSIC in one symbol.  v_means .. g_sh_coeffs are the bits gs_project_bwd_ex writes (or adds, with
 * accumulate != 0).  v_viewmat [16], required: a row-major 4 x 4, ALWAYS a plain write whatever `accumulate` says (a per-view
 * quantity), last row exactly 0; V == 0 (or N == 0) writes 16 zeros.
 *   The function differentiated is the forward as implemented, over the twelve entries R[3][3], t[3] of viewmat it reads:
 *   mc = R m + t, Cc = R cov R^T and, with SH colours of degree >= 1, campos = -R^T t -- NOT inverse(viewmat).  Off the rigid
 *   manifold the two differ; through any rigid parametrisation of the pose they agree, and agree with upstream.  Per visible
 *   Gaussian (v_mc, v_Cc: the chain's cotangents of mc and Cc; v_dir: the SH direction term that also enters v_means):
 *       v_t = v_mc (+ R v_dir),   v_R = v_mc m^T + (v_Cc + v_Cc^T) R cov (+ t v_dir^T);   K has no gradient.
 *   The sum over the Gaussians is bitwise reproducible: fp64 partial sums in one fixed order (one row of 12 doubles per 256
 *   Gaussians in ws, then a second small launch), rounded once to fp32; no float atomics.  Every segment of ws is written before it
 *   is read.  No host wait, no allocation. */
size_t gs_project_bwd_view_ws_bytes(int N);
int gs_project_bwd_view(int N, int V, int D, const float* means, const float* quats, const float* scales,
                        const float* opacities, const float* viewmat, const float* K, int W, int H, float eps2d,
                        const int32_t* gaussian_ids, const float* conics, const float* compensations,
                        const float* v_packed, int rec_stride, const float* v_depths, const float* sh_coeffs, int sh_K,
                        int sh_degree, int flags, float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                        float* v_colors, float* g_sh_coeffs, int accumulate, float* v_viewmat /* [16] */, void* ws, size_t ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------ S1..S3 ------------------------- */
/* Split-sum pyramid description (host struct, device pointers inside). */
typedef struct GsEnv {
    const float* lut;                     /* FG LUT [lut_res, lut_res, 2], row = roughness, col = N.V */
    int          lut_res;
    const float* base;                    /* diffuse irradiance [6, base_res, base_res, 3] */
    int          base_res;
    int          num_levels;              /* L */
    const float* levels[GS_MAX_LEVELS];   /* specular level l: [6, res[l], res[l], 3] */
    int          res[GS_MAX_LEVELS];
    float        min_roughness;           /* TextureSplitSum.min_roughness (0.08) */
    float        max_roughness;           /* TextureSplitSum.max_roughness (0.5)  */
} GsEnv;

typedef struct GsEnvGrad {
    float* base;                          /* [6, base_res, base_res, 3], accumulated into (caller zeroes) */
    float* levels[GS_MAX_LEVELS];
} GsEnvGrad;

/* colors[N,3] = shade(means, normals, kd, ks | cam_pos[3] (device), env). */
int gs_shade_fwd(int N, const float* means, const float* normals, const float* kd, const float* ks,
                 const float* cam_pos, float min_roughness, float max_metallic, int mode,
                 const GsEnv* env /*host*/, float* colors, void* stream);

/* Bytes of the optional workspace of gs_shade_bwd: 8 XCD-private copies of the texel-gradient levels that do
 * not fit LDS (XCD-local atomics stay in L2; device-scope ones are 32-byte write-throughs to the fabric). */
size_t gs_shade_bwd_ws_bytes(const GsEnv* env /*host*/, int mode);
/* launch shape gs_shade_bwd takes for N Gaussians: returns the number of blocks (0 on a bad env), *block_threads the block size;
 * blocks * block_threads < N means persistent blocks that stride over the Gaussians (tests size a grid-stride case by it) */
int gs_shade_bwd_plan_blocks(const GsEnv* env /*host*/, int mode, int N, int* block_threads);

/* Recomputes the forward and chains v_colors[N,3].  v_means/v_normals/v_kd/v_ks are fully written (or added
 * to when accumulate != 0); texel gradients are always ACCUMULATED into env_grad.  ws may be NULL (plain
 * device-scope atomics). */
int gs_shade_bwd(int N, const float* means, const float* normals, const float* kd, const float* ks,
                 const float* cam_pos, float min_roughness, float max_metallic, int mode,
                 const GsEnv* env /*host*/, const float* v_colors,
                 float* v_means, float* v_normals, float* v_kd, float* v_ks,
                 const GsEnvGrad* env_grad /*host*/, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ S4 ----------------------------- */
/* out[P,4] = tonemap(rgba[P,4] * exposure) ; exposure is a DEVICE scalar. */
int gs_tonemap_fwd(int64_t P, int mode, const float* rgba, const float* exposure, float* out, void* stream);
/* The same on the rasterizer's own layout (render [P,3] + alphas [P] -> image [P,4]; backward -> v_render [P,3], v_alphas [P]):
 * no rgba concatenation / strided copies between the compositor and the tone map. */
int gs_tonemap_fwd3(int64_t P, int mode, const float* render, const float* alphas, const float* exposure, float* out, void* stream);
int gs_tonemap_bwd3(int64_t P, int mode, const float* render, const float* alphas, const float* exposure, const float* v_out,
                    float* v_render, float* v_alphas, float* v_exposure, int accumulate, void* stream);
/* v_exposure: device scalar, zeroed by the call (accumulate == 0) then accumulated into. */
int gs_tonemap_bwd(int64_t P, int mode, const float* rgba, const float* exposure, const float* v_out,
                   float* v_rgba, float* v_exposure, int accumulate, void* stream);

/* ------------------------------------------------------------------ S5 ----------------------------- */
int gs_cubemap_mip_fwd(int R, int C, const float* in, float* out, void* stream);
/* n_levels successive gs_cubemap_mip_fwd calls (C = 3) in one launch: outs[k] = [6, R >> (k+1), R >> (k+1), 3], k < n_levels <= 5,
 * R a multiple of 2^n_levels (`outs` is a HOST array of device pointers).  Bit-identical to the chain of single calls
 * (the `while mips[-1].resolution > min_resolution` loop of TextureCubeMap.as_splitsum, rfstudio/graphics/_mesh/_texture.py:536-541). */
int gs_cubemap_mip_chain_fwd(int R, int n_levels, const float* in, float* const* outs, void* stream);
/* out[n,3] = seam-aware bilinear cube lookup of tex[6,R,R,3] at dirs[n,3] (used by the mip backward). */
int gs_cube_sample_linear(int64_t n, const float* tex, int R, const float* dirs, float scale, float* out,
                          void* stream);
/* _CubeMapMip.backward in one call: v_in[6,2R,2R,3] = 0.25 * cube-sample(v_out[6,R,R,3]) at fine texel dirs,
 * ADDED to v_in when accumulate != 0. */
int gs_cubemap_mip_bwd(int R, const float* v_out, float* v_in, int accumulate, void* stream);
int gs_diffuse_cubemap_fwd(int R, const float* cubemap, float* out, void* stream);
int gs_diffuse_cubemap_bwd(int R, const float* v_out, float* v_cubemap, int accumulate, void* stream);
/* bounds[6,R,R,24] (float-encoded ints, layout of the reference: per texel and face xmin, xmax, ymin, ymax of the lobe's texels).
 * gs_specular_bounds is shaped like SpecularBoundsKernel (cubemap.cu:181-244: every texel re-derives the corner directions of every
 * 16x16 tile); gs_specular_bounds_fast gives bit-identical boxes from per-tile / per-4x4-tile-group corner boxes computed once
 * (ws: gs_specular_bounds_ws_bytes(R) bytes of device scratch) and the cached direction table -- ~100x faster, the one the host uses. */
int gs_specular_bounds(int R, float costheta_cutoff, float* bounds, void* stream);
size_t gs_specular_bounds_ws_bytes(int R);
int gs_specular_bounds_fast(int R, float costheta_cutoff, const float* dir_table, float* bounds, void* ws, size_t ws_bytes, void* stream);
/* table[6,R,R,4] = {unit direction xyz, pixel_area}: depends on R only -- compute once, reuse every step. */
int gs_cube_dir_table(int R, float* table, void* stream);
/* out[6,R,R,4] = (sum rgb*w, sum w) */
int gs_specular_cubemap_fwd(int R, const float* cubemap, const float* bounds, const float* dir_table,
                            float roughness, float costheta_cutoff, float* out, void* stream);
/* v_out_rgb[6,R,R,3] = gradient w.r.t. the un-normalised rgb sums; v_cubemap written (or accumulated).  Atomic-free gather:
 * a source texel visits the outputs inside its own box grown by a margin (every texel for R < 64) and keeps those whose box
 * contains it -- the exact adjoint of gs_specular_cubemap_fwd (the reference scatters with atomicAdd, cubemap.cu:300-350). */
int gs_specular_cubemap_bwd(int R, const float* bounds, const float* dir_table, const float* v_out_rgb,
                            float roughness, float costheta_cutoff, float* v_cubemap, int accumulate, void* stream);

/* Tiled pair-weight tables of the specular prefilter (csrc/gs_splitsum_tiles.hip; replaces calling SpecularCubemapFwd/BwdKernel,
 * rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:246-350, with weights recomputed every step).  The pair weights
 * w(o,i) = g(o,i) * pixel_area(i) / 4 depend on (R, roughness, cutoff) only.  Units: a TILE = nb BLOCKS of 8x8 output texels of one
 * face in rows of bw blocks (tiles[n][4] = {face, x0, y0, 0}; block b covers x0 + 8 (b % bw) .., y0 + 8 (b / bw) ..); per
 * (tile, source face, block) -- "slot" (tile * 6 + face) * nb + b -- a list of ROWS, each one weight per lane (= output texel of
 * the block, lane = (y & 7) * 8 + (x & 7)) for the source texel anchor_lane + (dx, dy), anchor = min corner of the lane's lobe box
 * on that face (gs_specular_bounds), descriptor = (dy * pitch + dx) * 16 = the row's byte offset in the staged source rectangle.
 * Row lists are padded to multiples of 8 rows (zero weights); weights are stored in row pairs, [row / 2][lane][2].
 *   gs_specular_tiles_count : row_counts[n_tiles*6*nb] (un-padded), extents[n_tiles*6*nb][4] = {xmin, xmax, ymin, ymax} of the source
 *                             texels a slot's rows can address, *pairs += number of (output, source) pairs.  backward != 0: the
 *                             TRANSPOSED operator as a gather -- lane = source texel, partners = outputs inside the lane's own box
 *                             grown by `margin` texels (margin >= R: every texel of every face) whose box contains the lane's texel:
 *                             the exact adjoint of the forward.
 *   gs_specular_tiles_fill  : desc[rows], weights[rows * 64] (caller zero-fills both; row_begin[slot] = exclusive sum of the padded
 *                             counts; segments as below): g(o,i), the mirror-invariant factor of the weight.
 *   gs_specular_tiles_check : out2[0] = texels whose direction-table entry is not the exact sign-flipped image under the cube's
 *                             seven reflections, out2[1] = lobe boxes that are not the reflected box of the mirrored texel.  Both 0
 *                             <=> tables built for the tiles of ONE octant may be applied with n_mirrors = 8.
 *   gs_specular_tiles_apply : forward  dst[o] = sum_i g(o,i) src[i] scale[i] / sum_i g(o,i) scale[i]      (src = cubemap level [6,R,R,3],
 *                                      scale[6 R^2] = pixel_area / 4)
 *                             backward dst[i] = out_scale[i] sum_o g(o,i) src[o] scale[o]                  (src = d loss / d level,
 *                                      scale = 1 / sum of the pair weights of o, out_scale = pixel_area / 4)
 *                             for the tiles [tile_begin, tile_end) of `tiles` (and their 8 reflections when n_mirrors == 8; one rank's
 *                             share when the prefilter is sharded).  One workgroup of 16 waves per (tile, reflection); 16 / nb waves
 *                             share a block.  segments[n_tiles*6][4] = {x0, y0, rows, pitch} of the source rectangle staged in LDS
 *                             per (tile, face) (pitch 0 = no rows), lds_bytes = max rows * pitch * 16. */
int gs_specular_tiles_count(int R, float roughness, float costheta_cutoff, int backward, int margin, int bw, int nb, const float* bounds,
                            const float* dir_table, const int32_t* tiles, int n_tiles, int32_t* row_counts, int32_t* extents,
                            uint64_t* pairs, void* stream);
int gs_specular_tiles_fill(int R, float roughness, float costheta_cutoff, int backward, int margin, int bw, int nb, const float* bounds,
                           const float* dir_table, const int32_t* tiles, int n_tiles, const int64_t* row_begin,
                           const int32_t* segments, int32_t* desc, float* weights, void* stream);
int gs_specular_tiles_check(int R, const float* bounds, const float* dir_table, uint64_t* out2, void* stream);
int gs_specular_tiles_apply(int R, int backward, int n_mirrors, int margin, int bw, int nb, const float* src, const float* scale,
                            const float* out_scale, const float* bounds, const int32_t* tiles, const int32_t* segments,
                            const int64_t* row_begin, const int32_t* row_counts, const int32_t* desc, const float* weights, float* dst,
                            int tile_begin, int tile_end, size_t lds_bytes, void* stream);

/* The same for SEVERAL levels in one launch (the six specular_cubemap calls of TextureCubeMap.as_splitsum,
 * rfstudio/graphics/_mesh/_texture.py:546-556, or their six backward calls): one entry per level with the arguments of
 * gs_specular_tiles_apply; the levels must not alias (each reads its own src and writes its own dst) and must share n_mirrors.
 * Workgroups are numbered level after level in the order given.  Results are bit-identical to the per-level calls. */
typedef struct GsTileLevel {
    int R, n_mirrors, margin, bw, nb, tile_begin, tile_end, reserved;
    const float* src; const float* scale; const float* out_scale; const float* bounds;
    const int32_t* tiles; const int32_t* segments; const int64_t* row_begin; const int32_t* row_counts; const int32_t* desc;
    const float* weights; float* dst; size_t lds_bytes;
} GsTileLevel;
int gs_specular_tiles_apply_multi(int n_levels, const GsTileLevel* levels, int backward, void* stream);

/* ------------------------------------------------------------------ M1: MGAdapter (mesh -> Gaussians) */
/* rfstudio/model/geosplat.py:378-472 (MGAdapter.make, default ratios): every face -> 6 flat Gaussians (two rings
 * of three).  Output rows are part-major like the reference's Splats.cat: row = part * F + face, N = 6 F.
 *   means[N,3]; scales[N,3] log-scales (third = -10); quats[N,4] wxyz; normals[N,3] interpolated shading normals.
 * faces[F,3] int64 vertex indices; vertices[V,3]; vnormals[V,3].  Opacities are the constant logit(0.99). */
int gs_mgadapter_fwd(int F, const float* vertices, const int64_t* faces, const float* vnormals,
                     float* means, float* scales, float* quats, float* normals, void* stream);
/* v_vertices[V,3], v_vnormals[V,3] are WRITTEN (zeroed by the call, then accumulated with fp32 atomics).
 * v_normals may be NULL (no gradient through the shading normals). */
int gs_mgadapter_bwd(int F, int V, const float* vertices, const int64_t* faces, const float* vnormals,
                     const float* v_means, const float* v_scales, const float* v_quats, const float* v_normals,
                     float* v_vertices, float* v_vnormals, void* stream);

/* compute_vertex_normals_(fix=True), rfstudio/graphics/_mesh/_triangle_mesh.py:588-613: area-weighted vertex normals.
 * raw[V,3] = un-normalised sums (saved for the backward); |raw| <= 1e-10 -> (0,0,1) with zero gradient.
 * bwd: v_raw[V,3] scratch; v_vertices[V,3] written, or accumulated into when accumulate != 0 (so that it can be
 * chained onto gs_mgadapter_bwd's v_vertices). */
int gs_vertex_normals_fwd(int F, int V, const float* vertices, const int64_t* faces, float* raw, float* vnormals,
                          void* stream);
int gs_vertex_normals_bwd(int F, int V, const float* vertices, const int64_t* faces, const float* raw,
                          const float* v_vnormals, float* v_raw, float* v_vertices, int accumulate, void* stream);

/* ------------------------------------------------------------------ L1: loss side (per view) ------- */
/* rfstudio/trainer/geosplat_trainer.py:171-195 for one view, value AND gradient in one call:
 *   x = rgb + (1-alpha) train_bg;  y = lin(gt) mask + (1-mask) train_bg;  mask = gt alpha
 *   loss = ssim_lambda (1 - SSIM(y,x)) + (1 - ssim_lambda) L1(x,y) + mask_weight mean((mask-alpha)^2)
 * SSIM = torchmetrics structural_similarity_index_measure defaults (11x11 Gaussian, sigma 1.5; loss/photometric_loss.py:73-112).
 *   rgb[H,W,3] linear (the path's tone-mapped output), alpha[H,W], gt_rgba[H,W,4] (sRGB colours when gt_is_srgb != 0:
 *   srgb2rgb of graphics/_images.py:287-311 is applied inside), train_bg[H,W,3] (the caller's torch.rand_like),
 *   metric_bg[3] device or NULL (background of the sRGB PSNR metric, :191-195).
 *   out[6] device = {loss, 1-ssim, l1, mask_mse, mse_srgb, psnr_srgb}  (unscaled)
 *   v_rgb[H,W,3], v_alpha[H,W] = grad_scale * d loss / d(rgb, alpha)  (both NULL: value only).
 * W, H must exceed 10.  Deterministic (fixed-order reduction). */
size_t gs_photo_loss_ws_bytes(int W, int H);
int gs_photo_loss(int W, int H, const float* rgb, const float* alpha, const float* gt_rgba, int gt_is_srgb,
                  const float* train_bg, const float* metric_bg, float ssim_lambda, float mask_weight,
                  float grad_scale, float* out, float* v_rgb, float* v_alpha, void* ws, size_t ws_bytes, void* stream);

/* The smoothing regularisers of the stage-1 trainer (rfstudio/model/geosplat.py:881-922; geosplatting_amd/stage1.py _edge_aware /
 * _tv) on the un-shaded attribute renders of one view, value AND gradient in one call:
 *   img[H,W,9]: three renders over the background, channel order kd(3), (0, ks)(3), normal * 0.5 + 0.5 (3);
 *   gt_rgb[H,W,3]: the ground truth blended over the background (NULL when no term is GS_SMOOTH_EDGE);
 *   kinds[3], weights[3] (host): per render GS_SMOOTH_NONE, GS_SMOOTH_EDGE = (|S(r)| exp(-|S(gt)|)).sum(dir).mean() with S the
 *     normalised Sobel pair (kernel / 8, replicate padding, cross-correlation), or GS_SMOOTH_TV = the two mean squared forward
 *     differences, times its weight.
 *   *out (device) += the weighted sum (fixed-order reduction in double: deterministic);  v_img[H,W,9] = d out / d img (written;
 *   0 in the channels of a render without a term).  W, H >= 2; ws: gs_smooth_loss_ws_bytes(W, H) bytes. */
size_t gs_smooth_loss_ws_bytes(int W, int H);
int gs_smooth_loss(int W, int H, const float* img, const float* gt_rgb, const int* kinds, const float* weights, float* out,
                   float* v_img, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ F1: hash-grid encoding --------- */
/* HashEncoding, `backend='torch'` semantics (rfstudio/model/components/encoding.py:187-229): every level hashed,
 * x in [-1,1]^3 -> x/2+1/2, scalings[l] = floor(min_res * growth^l) (host array of L floats, computed by the caller
 * exactly as encoding.py:124-132 does), corners {ceil, floor}, hash = (x ^ y*2654435761 ^ z*805459861) mod 2^log2_T.
 *   x[N,3]; table[L * 2^log2_T, F]; out[N, L*F].  F must be 2 (rfstudio/model/geosplat.py:485-518).
 * bwd: v_table (+)= table_grad_scale * d/dtable (written, or added to when accumulate != 0; table_grad_scale
 *      carries the reference's grad_scaling trick, encoding.py:231-240), v_x[N,3] written (may be NULL). */
int gs_hashgrid_fwd(int N, int L, int F, int log2_T, const float* scalings_host, const float* x, const float* table,
                    float* out, void* stream);
size_t gs_hashgrid_bwd_ws_bytes(int N, int L, int F);         /* level-major copy of v_out */
int gs_hashgrid_bwd(int N, int L, int F, int log2_T, const float* scalings_host, const float* x, const float* table,
                    const float* v_out, float table_grad_scale, float* v_table, int accumulate, float* v_x,
                    void* ws /* with it: atomic-free LDS-slab kernel; NULL: per-point kernel with fp32 atomics */,
                    size_t ws_bytes, void* stream);

/* gs_hashgrid_bwd with the table gradient accumulated in 64-bit FIXED POINT over binned points: deterministic (integer
 * sums), and faster -- LDS float atomics retire one lane per ~3 cycles on gfx950, integer ones 18-30x as many.  One power
 * of two per level, from that level's max |v_out| (reduced on the device), scales the fixed point.  Arguments as
 * gs_hashgrid_bwd; ws: gs_hashgrid_bwd_fixed_ws_bytes(N, L, F, log2_T) bytes (0: table size outside 2^15..2^19 rows). */
size_t gs_hashgrid_bwd_fixed_ws_bytes(int N, int L, int F, int log2_T);
int gs_hashgrid_bwd_fixed(int N, int L, int F, int log2_T, const float* scalings_host, const float* x, const float* table,
                          const float* v_out, float table_grad_scale, float* v_table, int accumulate, float* v_x, void* ws,
                          size_t ws_bytes, void* stream);

/* Weight gradient of one bias-free linear layer of the field's MLPs (rfstudio/nn/mlp.py:126-145; widths <= 32):
 *   dW[O,I] (+)= scale * dY[N,O]^T X[N,I]   (row-major, contiguous; O, I in [1,32]).  fp32 matrix unit, exact f32;
 *   deterministic (partials summed in a fixed order).  ws: gs_mlp_wgrad_ws_bytes(N). */
size_t gs_mlp_wgrad_ws_bytes(int64_t N);
int gs_mlp_wgrad(int64_t N, int O, int I, const float* dY, const float* X, float scale, float* dW, int accumulate,
                 void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ X1: FlexiCubes extraction ------ */
/* FlexiCubes.dual_marching_cubes(grad_func=None) + compute_entropy on the regular grid of FlexiCubes.from_resolution
 * (rfstudio/graphics/_mesh/_flexicubes.py:397-457, 559-713, 715-802; caller rfstudio/model/geosplat.py:751-769).
 * Grid: cube n = i0 + R0 (i1 + R1 i2); grid vertex id = i0 + (R0+1) (i1 + (R1+1) i2); cube corner k adds bit j of k to ij
 * (exactly the `indices` from_resolution builds, which are therefore not passed).
 *   vertices[Vg,3], sdf[Vg]; raw alpha[C,8] / beta[C,12] / gamma[C] or NULL (the tanh / sigmoid * weight_scale
 *   activations of :608-624 are applied inside); sdf_eps < 0 means None.
 * Step 1  gs_flexicubes_count: classifies cubes and grid edges into `ws`, writes counts[8] (device int64) =
 *         {surface cubes N, dual vertices Q, (patch,edge) pairs K, surface edges E, quads, flipped quads, 0, 0}.
 *         The caller reads them (the reference's own .item() syncs) and allocates the outputs.
 * Step 2  gs_flexicubes_fwd: out_vertices[Q + quads, 3] (dual vertices, then one centre vertex per quad),
 *         out_faces[4 * quads, 3] int64, L_dev[K] -- vertex / face / row numbering identical to the reference's.
 * Step 3  gs_flexicubes_bwd: cotangents v_out_vertices[Q+quads,3], v_L_dev[K] (or NULL) -> g_vertices[Vg,3], g_sdf[Vg],
 *         g_alpha[C,8], g_beta[C,12], g_gamma[C] (w.r.t. the RAW weights; NULL iff the weight was NULL), all overwritten.
 *         g_vd_scratch: 3*Q floats.  `ws` must still hold what step 1 left for the same sdf.
 * gs_flexicubes_entropy_fwd/bwd: compute_entropy (:715-725) of the same sdf (needs step 1's `ws`); out[1]; bwd adds
 *         v_out[0] * d/dsdf into g_sdf (overwrites when accumulate == 0). */
size_t gs_flexicubes_ws_bytes(int R0, int R1, int R2);
int gs_flexicubes_count(int R0, int R1, int R2, const float* sdf, void* ws, size_t ws_bytes, int64_t* counts, void* stream);
int gs_flexicubes_fwd(int R0, int R1, int R2, const float* vertices, const float* sdf, const float* alpha,
                      const float* beta, const float* gamma, float weight_scale, float sdf_eps, const void* ws,
                      size_t ws_bytes, int64_t Q, int64_t num_quads, int64_t K, float* out_vertices, int64_t* out_faces,
                      float* L_dev, void* stream);
int gs_flexicubes_bwd(int R0, int R1, int R2, const float* vertices, const float* sdf, const float* alpha,
                      const float* beta, const float* gamma, float weight_scale, float sdf_eps, const void* ws,
                      size_t ws_bytes, int64_t Q, int64_t num_quads, int64_t K, const float* out_vertices,
                      const float* v_out_vertices, const float* v_L_dev, float* g_vd_scratch, float* g_vertices,
                      float* g_sdf, float* g_alpha, float* g_beta, float* g_gamma, void* stream);
int gs_flexicubes_entropy_fwd(int R0, int R1, int R2, const float* sdf, void* ws, size_t ws_bytes, float* out, void* stream);
int gs_flexicubes_entropy_bwd(int R0, int R1, int R2, const float* sdf, const void* ws, size_t ws_bytes, const float* v_out,
                              float* g_sdf, int accumulate, void* stream);

/* ------------------------------------------------------------------ fused front / tail of a view (the engine's path) ---------- */
/* Shading fused AHEAD of the projection (north star; reference semantics rfstudio/model/geosplat.py:80-128 followed by the
 * rasterization call at rfstudio/model/gsplat.py:334-355): one launch projects every Gaussian (gs_project_fwd's arithmetic),
 * shades the visible ones (gs_shade_fwd's arithmetic) and writes, in packed order (ascending Gaussian index),
 *   vis_records [N,16] f32 : {mx, my, a/2, b | c/2, opacity*comp, hx, hy | r, g, b, 0 | comp, bits(Gaussian index), depth, bits(radius)}
 *                            -- gs_raster_prepare_vis(_cap) consumes it as is, gs_tail_bwd reads the fourth quarter;
 *   depth_keys [N] u32     : the binning's depth key.  key_bits == 32: the depth's float bits.  key_bits == 24: bits - key_base,
 *                            valid while key_base <= bits < key_base + 2^24 for every visible Gaussian -- otherwise
 *                            status4[3] is set to 1 (int64[4], caller-zeroed, sticky; words 0..2 as for gs_isect_bin_cap) and the
 *                            key is clamped: memory-safe, wrong order, reported;
 *   tile_rects [N,2] u32   : (x0 | y0 << 16, x1 | y1 << 16), the tile rectangle of gs_project_fwd's tiles_per_gauss;
 *   tile_counts [tiles] u32: intersections per tile (zeroed by the call; nullable, and not written for more than 8 192 tiles):
 *                            gs_isect_bin_front turns them into the tile offsets;
 *   counts4 [4] i64        : {V, I, 0xffffffff - min depth bits, max depth bits} (zeroed by the call).
 * No other per-visible array exists on this path.  Scratch: gs_front_ws_bytes(N), zeroed by the call.
 * tight_tiles != 0: the tile rectangle is gsplat's square intersected with the axis-aligned extent of {alpha >= 1/255} (the extents
 * hx, hy of the record, with which the compositor culls its quadrants anyway): every pixel composites exactly the same Gaussians in
 * the same order, I is smaller (a caller that needs gsplat's `meta` passes 0).
 * Two partial forms (same packed order, same counts): vis_records == NULL = GEOMETRY ONLY (keys, rectangles, tile counts, slots;
 * nothing is shaded, env may be NULL) -- the engine bins its first view with it while the prefilter is still computing the
 * pyramid -- and depth_keys == tile_rects == NULL = records only. */
size_t gs_front_ws_bytes(int N);
int gs_front_fwd(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                 const float* normals, const float* kd, const float* ks, const float* viewmat, const float* K,
                 const float* cam_pos, float min_roughness, float max_metallic, int mode, const GsEnv* env,
                 int W, int H, int tile_size, float eps2d, float near_plane, float far_plane, float radius_clip,
                 uint32_t key_base, int key_bits, float* vis_records, uint32_t* depth_keys, uint32_t* tile_rects,
                 uint32_t* tile_counts, int32_t* packed_index /* [N], nullable: packed slot of every Gaussian or -1 */,
                 int tight_tiles, int64_t* counts4, int64_t* status4, void* ws, size_t ws_bytes, void* stream);
/* Binning from gs_front_fwd's outputs: flatten_ids_sorted in (tile, depth, packed index) order and the tile offsets, bit-identical
 * to gs_isect_bin_tiles_cap + gs_isect_offsets_tiles_cap.  counts_dev == NULL: V_cap / n_isects_cap are the exact counts; otherwise
 * the capacity protocol of gs_isect_bin_cap (status_dev int64[4]).  key_bits as passed to gs_front_fwd.
 * With tile_counts and at most 8 192 tiles the binning is tile first (scatter into the tiles' segments, one workgroup sorts each
 * segment on chip; I * 8 bytes of scratch); gs_isect_bin_front_ws_bytes returns that size for such a grid.  Otherwise (no
 * tile_counts, or a larger grid) it runs radix passes: for a larger grid gs_isect_bin_front_ws_bytes covers them; a caller that
 * withholds tile_counts on a small grid gets GS_ENOSPC unless its scratch is as large as the radix passes need.
 * gs_isect_bin_front_classes: the segment lengths at which the sort changes its path, ascending -- {2048, 8192}: up to the first a
 * 128-thread workgroup sorts the segment in LDS, up to the second a 512-thread workgroup does, a longer one is sorted by a 512-thread
 * workgroup in 8 192-item chunks in LDS with the wide stages of the network in place in global memory; fills at most `max` entries
 * of caps, returns how many lengths there are. */
size_t gs_isect_bin_front_ws_bytes(int V, int64_t n_isects, int tile_w, int tile_h);
int gs_isect_bin_front_classes(int* caps, int max);
int gs_isect_bin_front(int V_cap, const uint32_t* depth_keys, const uint32_t* tile_rects, const uint32_t* tile_counts,
                       const int64_t* counts_dev, int64_t n_isects_cap, int key_bits, int tile_w, int tile_h, int32_t* flatten_ids_sorted,
                       int32_t* isect_offsets, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream);
/* Projection backward fused with the shading backward (gs_project_bwd + gs_shade_bwd in one launch, one thread per VISIBLE
 * Gaussian): reads vis_records and the compositor's gradient records v_packed [V, rec_stride] ({xy, conic(3), opacity, rgb}),
 * ADDS into v_means [N,3], v_quats [N,4], v_scales [N,3] (gradient w.r.t. the scales passed in), v_opacities [N], v_normals,
 * v_kd [N,3], v_ks [N,2] and into the texel gradients env_grad.  counts_dev == NULL: V_cap is the count. */
int gs_tail_bwd(int V_cap, const int64_t* counts_dev, const float* means, const float* quats, const float* scales,
                const float* opacities, const float* normals, const float* kd, const float* ks, const float* viewmat,
                const float* K, const float* cam_pos, float min_roughness, float max_metallic, int mode, const GsEnv* env,
                int W, int H, float eps2d, const float* vis_records, const float* v_packed, int rec_stride,
                float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_normals, float* v_kd, float* v_ks,
                const GsEnvGrad* env_grad, void* priv_ws, size_t priv_ws_bytes, void* stream);
/* The tails of ALL views of a step in one call (two launches: shading half, projection half): up to eight adjacent lanes own one
 * Gaussian, one view each, the 19 parameter gradients are summed over the lanes and stored once (accumulate == 0: plain stores
 * into v_*, every Gaussian written; != 0: added).  Per view: what gs_front_fwd wrote (vis_records, packed_index) and the
 * compositor's v_packed [V, rec_stride].  The gradients of gs_tail_bwd summed over the views, to summation order (the views as a
 * tree, the colour cotangent contracted into the cube fetch: tests/test_gpu_front.py, 1e-5).  More than eight views: further
 * launches add to the first. */
typedef struct GsTailView {
    const float* viewmat; const float* K; const float* cam_pos;            /* device: [4,4], [3,3], [3] */
    const float* vis_records; const float* v_packed; const int32_t* packed_index;
    int W, H;
} GsTailView;
int gs_tail_bwd_multi(int N, int n_views, const GsTailView* views /*host array*/, const float* means, const float* quats,
                      const float* scales, const float* opacities, const float* normals, const float* kd, const float* ks,
                      float min_roughness, float max_metallic, int mode, const GsEnv* env, float eps2d, int rec_stride,
                      float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_normals, float* v_kd, float* v_ks,
                      int accumulate, const GsEnvGrad* env_grad, void* priv_ws, size_t priv_ws_bytes, void* stream);
/* The two halves of gs_tail_bwd_multi as separate calls (bit 0 of `parts`: the S1-S3 shading backward -- writes v_means (its
 * view-direction part), v_normals, v_kd, v_ks and the texel gradients; bit 1: the A7 projection backward -- ADDS its part to
 * v_means, writes v_quats, v_scales, v_opacities), so that the caller can put them on different streams: the projection half has
 * to follow the shading half of the same call (v_means), nothing else orders them.  parts == 3 is gs_tail_bwd_multi.
 * Bit 2 (with bit 0): a BACKGROUND launch -- the shading half on half of the CUs (128 persistent workgroups), for a tail that is
 * not the last of its step and runs beside the compositor of the following views; same results, same order of the sums per
 * Gaussian (texel gradients are float atomics in every form). */
int gs_tail_bwd_multi_parts(int parts, int N, int n_views, const GsTailView* views /*host array*/, const float* means, const float* quats,
                            const float* scales, const float* opacities, const float* normals, const float* kd, const float* ks,
                            float min_roughness, float max_metallic, int mode, const GsEnv* env, float eps2d, int rec_stride,
                            float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_normals, float* v_kd, float* v_ks,
                            int accumulate, const GsEnvGrad* env_grad, void* priv_ws, size_t priv_ws_bytes, void* stream);
/* Optional scratch of gs_tail_bwd / gs_tail_bwd_multi: eight XCD-private copies of the mid-sized specular levels (64^2, 128^2 of a 512^2 pyramid), whose
 * texel atomics then resolve in the XCD's own L2 instead of at the memory side of the fabric.  The caller zeroes priv_ws
 * (gs_tail_priv_ws_bytes) once, every gs_tail_bwd of a step ADDS into it, gs_tail_priv_reduce folds it into env_grad once.
 * priv_ws == NULL: every texel gradient goes straight into env_grad. */
size_t gs_tail_priv_ws_bytes(const GsEnv* env /*host*/, int mode);
int gs_tail_priv_reduce(const GsEnv* env /*host*/, int mode, const void* priv_ws, size_t priv_ws_bytes, const GsEnvGrad* env_grad,
                        void* stream);

/* Chain rule of the per-step activations of GSplatter.render_rgba (rfstudio/model/gsplat.py:336-339: `scales.exp()`,
 * `sigmoid(opacities)`) applied once to gradients accumulated over the views of a step:
 *   v_scales[N,3] = g_scales_act * scales_act,   v_opacities[N] = (g_opac_act * opac_act) * (1 - opac_act). */
/* The attribute renders of the smoothing regularisers on a view the engine has binned (gs_front_fwd's packed slots), D = 9:
 *   gs_smooth_gather: cols[slot, 9] = (kd, 0, ks0, ks1, normal * 0.5 + 0.5) of the Gaussian of every visible slot (its index is in
 *     the slot's vis_records entry) -- the colours gs_raster_composite*(D = 9) reads;
 *   gs_smooth_fold: the compositor's D = 9 gradient records v_packed9 [V, stride9] of the same view: their geometry floats [0..5]
 *     are ADDED to the shaded view's v_packed [V, stride] (same slots), their colour floats to the per-Gaussian v_kd [N,3], v_ks [N,2]
 *     (channel 0 of (0, ks) dropped) and v_normals [N,3] (times 0.5).  Plain read-modify-write: the folds of a step run on one stream.
 * counts_dev == NULL: V_cap is the count; else {V, I} on the device (capacity protocol). */
int gs_smooth_gather(int V_cap, const int64_t* counts_dev, const float* vis_records, const float* kd, const float* ks,
                     const float* normals, float* cols, void* stream);
int gs_smooth_fold(int V_cap, const int64_t* counts_dev, const float* vis_records, const float* v_packed9, int stride9, float* v_packed,
                   int stride, float* v_kd, float* v_ks, float* v_normals, void* stream);

int gs_activation_chain(int64_t N, const float* g_scales_act, const float* scales_act, const float* g_opac_act, const float* opac_act,
                        float* v_scales, float* v_opacities, void* stream);

/* ------------------------------------------------------------------ adaptive density control of the 3DGS trainer ---------- */
/* Splats.densify_and_cull / Splats.cull (rfstudio/graphics/_splats.py:121-175), GSplatter.update_grad_norm
 * (rfstudio/model/gsplat.py:360-374) and the Adam-moment half of ModuleOptimizers.mutate_params (rfstudio/optim/optimizer.py:155-185).
 * The count -> read totals -> fill protocol of the FlexiCubes entry points:
 *
 * gs_densify_stats: for every visible row v, xys_grad_norm[id] += |v_means2d[v]| and vis_counts[id] += 1 with id = gaussian_ids[v].
 *   Ids are unique within a call (packed, one camera): plain read-modify-write.  Ids outside [0, N) are skipped.
 *
 * gs_densify_plan (count): scales[N,3] (log), opacities[N] (logit).  Per Gaussian
 *     scale_max = max_j exp(scales_j),  avg = half_extent * (xys_grad_norm / vis_counts)     (half_extent = 0.5 * max(W, H), host)
 *     high = avg > grad_thresh,  split = high && scale_max > size_thresh,  dup = high && scale_max <= size_thresh
 *     cull = sigmoid(opacity) < alpha_thresh || (scale_thresh >= 0 && scale_max > scale_thresh)     (scale_thresh < 0: None)
 *     selected = !(cull || split)
 *   mode GS_DENSIFY_MODE_CULL is Splats.cull: only `cull` is evaluated (xys_grad_norm / vis_counts may be NULL, num_splits unused).
 *   Leaves the classes and their exclusive ranks over the index order in `ws` and writes
 *   totals[4] (device int64) = {n_selected, n_split, n_dup, N_out = n_selected + num_splits * n_split + n_dup}.
 *   A duplicated Gaussian that is not culled appears twice (kept and copied); a culled one still yields its children or its copy.
 *
 * gs_densify_fill: after the caller has read `totals` and allocated.  `ws` must still hold what the plan left; the fill WRITES its row
 *   map (output row -> source row) into the part of `ws` the plan reserved for it.  Output rows, as
 *   Splats.cat([self[selected], self[splits].split(S).view(-1), self[dups]]): selected rows in index order, then child s of the
 *   split row of rank r at n_selected + s * n_split + r (S-major), then the duplicates in index order.
 *   indices[N_out]: the source index of a selected row, -1 for every new row (what mutate_params consumes).
 *   Every tensor of `table` (host array) is gathered in one launch: dst[N_out, floats_per_row] from src[N, floats_per_row],
 *     GS_DENSIFY_COPY    every row copied bit for bit (quats, colours, SH, opacities)
 *     GS_DENSIFY_MEANS   child rows: R(q / |q|) (exp(scales) o z) + mean with z = randn[S, n_split, 3] (its flat row is the
 *                        child's output row minus n_selected); other rows copied
 *     GS_DENSIFY_SCALES  child rows: log(exp(scales) * (1 / 1.6)); other rows copied
 *     GS_DENSIFY_MOMENT  selected rows copied, every new row 0 (Adam exp_avg / exp_avg_sq)
 *   quats / scales are the SOURCE tensors [N,4] / [N,3]; they and randn may be NULL when no MEANS tensor has children.
 *   The totals are the caller's: rows beyond them are not written and source rows are clamped to [0, N), so totals that do not
 *   belong to the plan in `ws` give wrong rows but touch no memory outside the buffers they size.
 *   Limits: N <= 2^27, num_splits <= 8, N_out * floats_per_row < 2^31, at most GS_DENSIFY_MAX_TENSORS tensors. */
#define GS_DENSIFY_COPY         0
#define GS_DENSIFY_MEANS        1
#define GS_DENSIFY_SCALES       2
#define GS_DENSIFY_MOMENT       3
#define GS_DENSIFY_MODE_DENSIFY 0
#define GS_DENSIFY_MODE_CULL    1
#define GS_DENSIFY_MAX_TENSORS  32
#define GS_DENSIFY_MAX_SPLITS   8
#define GS_DENSIFY_MAX_N        (((int64_t)1) << 27)

typedef struct GsDensifyTensor {
    const float* src;
    float*       dst;
    int          floats_per_row;
    int          kind;
} GsDensifyTensor;

int gs_densify_stats(int V, const int64_t* gaussian_ids, const float* v_means2d, int64_t N, float* xys_grad_norm, float* vis_counts,
                     void* stream);
size_t gs_densify_ws_bytes(int64_t N, int num_splits);
int gs_densify_plan(int64_t N, const float* scales, const float* opacities, const float* xys_grad_norm, const float* vis_counts,
                    float half_extent, float grad_thresh, float size_thresh, float alpha_thresh, float scale_thresh, int num_splits,
                    int mode, void* ws, size_t ws_bytes, int64_t* totals, void* stream);
int gs_densify_fill(int64_t N, int num_splits, void* ws, size_t ws_bytes, int64_t n_selected, int64_t n_split, int64_t n_dup,
                    const GsDensifyTensor* table /*host*/, int n_tensors, const float* quats, const float* scales, const float* randn,
                    int64_t* indices, void* stream);

/* ------------------------------------------------------------------ 2D Gaussian splatting (surfels) -- */
/* gsplat 1.4 `rasterization_2dgs(packed=True)`, one camera, as the reference's GSplatter calls it with rasterize_mode='2dgs'
 * (rfstudio/model/gsplat.py:129-150, :217-238, :312-332).  csrc/gs_surfel.hip.  Only the surfel projection and the ray-splat
 * compositor are new: binning, sort and offsets are gs_isect_bin / gs_isect_offsets on (means2d, radii, depths).
 *
 * gs_surfel_project_fwd: scales [N,3] activated, only [:, :2] are used.  Rc = Rcw R(q), c = Rcw mean + t; culled outside
 * [near, far]; ray transform M = K [s0 Rc[:,0] | s1 Rc[:,1] | c] (rows M0, M1, M2); with test = (1,1,-1), d = sum test M2^2 (culled
 * when 0), f = test / d: means2d = (sum f M0 M2, sum f M1 M2), ext = means2d^2 - (sum f M0^2, sum f M1^2),
 * radius = ceil(3 sqrt(max(1e-4, max(ext)))); culled when radius <= radius_clip or the square means2d +- radius misses the image
 * (gs_project_fwd's inequalities).  normal = Rc[:,2], negated when normal . c > 0 (camera space, facing the camera).
 * Packed outputs (capacity N, ascending Gaussian index): gaussian_ids, radii, means2d [V,2], depths (= c.z), ray_transforms [V,9],
 * normals [V,3], opacities_packed, tiles_per_gauss, colors_packed [V, Dc + depth_channel]: the colours (plain [N,Dc], or, with
 * sh_degree in 0..3, evaluated from sh_coeffs [N,sh_K,3] exactly as gs_project_fwd_vis_ex does; Dc == 3 then) followed by the depth
 * when depth_channel is 1.  1 <= Dc + depth_channel <= 4.  counts = {V, I} (int64) as gs_project_fwd. */
size_t gs_surfel_project_ws_bytes(int N);
int gs_surfel_project_fwd(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                          const float* colors, int Dc, const float* sh_coeffs, int sh_K, int sh_degree, int depth_channel,
                          const float* viewmat, const float* K, int W, int H, int tile_size, float near_plane, float far_plane,
                          float radius_clip, int32_t* gaussian_ids, int32_t* radii, float* means2d, float* depths,
                          float* ray_transforms, float* normals, float* opacities_packed, float* colors_packed,
                          int32_t* tiles_per_gauss, void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* The exact derivative of the above (radii are not differentiable).  The incoming gradients are rows of `stride` floats per visible
 * Gaussian (the columns of gs_surfel_raster_bwd's v_packed, or separate arrays that all have this one row length): v_ray_transforms (9),
 * v_means2d (2), v_depths (1, nullable), v_normals (3), v_opacities (1), v_colors (Dc).  Outputs [N, .], zero for invisible Gaussians:
 * g_means, g_quats, g_scales (third column 0), g_opacities and g_colors [N,Dc] or, with sh_degree >= 0, g_sh [N,sh_K,3]. */
int gs_surfel_project_bwd(int N, int V, int Dc, const float* means, const float* quats, const float* scales,
                          const float* sh_coeffs, int sh_K, int sh_degree, const float* viewmat, const float* K,
                          const int32_t* gaussian_ids, const float* v_ray_transforms, const float* v_means2d,
                          const float* v_depths, const float* v_normals, const float* v_opacities, const float* v_colors,
                          int stride, float* g_means, float* g_quats, float* g_scales, float* g_opacities, float* g_colors,
                          float* g_sh, void* stream);

/* Ray-splat compositor, one tile_size x tile_size tile (8 or 16) per workgroup, front to back over the tile's sorted list.  For the
 * pixel centre p: hu = p.x M2 - M0, hv = p.y M2 - M1, z = hu x hv (skipped when z.z == 0), s = z.xy / z.z, w3 = s.s,
 * w2 = 2 |means2d - p|^2, sigma = min(w3, w2) / 2, alpha = min(0.999, opacity exp(-sigma)); skipped when sigma < 0 or alpha < 1/255;
 * the pixel stops when T (1 - alpha) <= 1e-4.  C = 1, 3 or 4 channels, the last one the depth when depth_channel is 1.
 * render [H,W,C] (+ T background on the first min(3, C - depth_channel) channels), alphas [H,W], render_normals [H,W,3] (camera space),
 * render_median [H,W] (depth of the last Gaussian composited while T > 0.5; 0 without a depth channel), and with distloss
 * render_distort [H,W] = sum 2 (vis d (1 - T) - vis D).  State of the backward: last_ids [H,W] (list index of the last
 * composited entry, -1 for none), final_T [H,W], final_D [H,W] (distloss). */
int gs_surfel_raster_fwd(int W, int H, int tile_size, int C, int depth_channel, int distloss, int V, const float* ray_transforms,
                         const float* means2d, const float* opacities, const float* colors, const float* normals,
                         const float* background, int64_t n_isects, const int32_t* offsets, const int32_t* flatten_ids,
                         float* render, float* alphas, float* render_normals, float* render_distort, float* render_median,
                         int32_t* last_ids, float* final_T, float* final_D, void* stream);

/* Floats per row of v_packed: v_ray_transforms [0..9), v_means2d [9..11), v_opacities [11], v_normals [12..15), v_colors [15..15+C). */
int gs_surfel_grad_stride(void);

/* Stored-state backward, back to front, alpha recomputed.  w3 < w2: the gradient of sigma goes to ray_transforms, else to means2d;
 * an active 0.999 clamp passes none.  v_packed [V, gs_surfel_grad_stride()] is zeroed by the call;
 * v_densify [V,2] = depths[v] * (v_ray_transforms[v][2], v_ray_transforms[v][5]). */
int gs_surfel_raster_bwd(int W, int H, int tile_size, int C, int depth_channel, int distloss, int V, const float* ray_transforms,
                         const float* means2d, const float* opacities, const float* colors, const float* normals,
                         const float* depths, const float* background, int64_t n_isects, const int32_t* offsets,
                         const int32_t* flatten_ids, const int32_t* last_ids, const float* final_T, const float* final_D,
                         const float* v_render, const float* v_alphas, const float* v_normals, const float* v_distort,
                         float* v_packed, float* v_densify, void* stream);

/* ------------------------------------------------------------------ TSDF depth fusion and marching cubes -- */
/* TriangleMesh.from_depth_fusion (rfstudio/graphics/_mesh/_triangle_mesh.py:321-388) as the MeshExport task calls it
 * (tests/model/test_gsplat.py:169-202): Open3D's uniform-volume update with depth scale 1, no colour and unit weight per
 * observation, on a DENSE volume with explicit bounds.  csrc/gs_tsdf.hip.
 *
 * Volume: R0 x R1 x R2 voxels, R0 R1 R2 < 2^31; voxel n = i0 + R0 (i1 + R1 i2); `volume` holds one interleaved (tsdf, weight)
 * float pair per voxel, (0, 0) before the first view; voxel centre = origin + (i + 0.5) voxel_size.
 *
 * gs_tsdf_integrate: up to GS_TSDF_MAX_VIEWS views per call (`views` is a host array; a caller with more views calls again).  Per
 * voxel centre p, over the views in order (viewmat rigid, world -> camera, z forward):
 *     pc = Rwc p + t,  z = pc.z;                         skipped unless z > 0
 *     u = fx pc.x / z + cx,  v = fy pc.y / z + cy;       skipped unless 0 <= u < W and 0 <= v < H
 *     (d, a) = depth_alpha[floor(v), floor(u)]           pixel j covers [j, j + 1): pixel centres at j + 0.5, as the rasterizer has them
 *     skipped unless a > alpha_trunc, and unless d > 0 and d < depth_trunc (a NaN depth skips)
 *     sdf = d - z;                                       skipped unless sdf > -sdf_trunc
 *     val = min(1, sdf / sdf_trunc);  tsdf = (tsdf w + val) / (w + 1);  w += 1
 *   (1 / z and 1 / (w + 1) are the hardware reciprocal, 1 ulp.)
 *   The order of the views per voxel is fixed, so the result does not depend on how the views are split across calls.  A view whose
 *   frustum misses a brick of voxels is skipped for that brick (same result).  No atomics.
 *
 * Extraction: marching cubes over the (R0-1)(R1-1)(R2-1) cubes whose corners are voxel centres; cube (i0,i1,i2) has corner k at
 * i + (k & 1, (k >> 1) & 1, (k >> 2) & 1).  A cube is valid iff its eight weights are > 0; a corner is inside iff tsdf < 0 (exact 0 is
 * outside).  A grid edge is owned by the voxel at its lower end and carries a vertex iff its ends differ in sign and it belongs to
 * at least one valid cube (no unreferenced vertices).  Vertex ids ascend by (owning voxel n, then axis 0, 1, 2); the position is
 * pa + (ta / (ta - tb)) (pb - pa) from the lower end a.  Triangles ascend by (cube linear index, then the order of
 * csrc/gs_mc_table.h, generated by scripts/make_mc_table.py); their normals point toward positive tsdf (free space).
 * The count -> read totals -> fill protocol of the FlexiCubes and densify entry points:
 *   gs_tsdf_extract_ws_bytes  workspace size: 7 bytes per voxel + 16 per 256 voxels (0: resolution out of range)
 *   gs_tsdf_extract_count     classifies into `ws`, writes counts[4] (device int64) = {vertices, triangles, valid cubes, surface cubes}
 *   gs_tsdf_extract_fill      after the caller has read the counts and allocated: vertices [n_vertices,3] float, faces
 *                             [n_triangles,3] int64.  `ws` and `volume` must be what the count saw.  Rows beyond the caller's totals
 *                             are not written; totals of 2^31 or more are an error. */
#define GS_TSDF_MAX_VIEWS 16
typedef struct GsTsdfView {
    const float* depth_alpha;                       /* device [H,W,2]: (depth, alpha) per pixel, what render_depth returns */
    const float* viewmat; const float* K;           /* device: [4,4], [3,3] */
    int W, H;
} GsTsdfView;
int gs_tsdf_integrate(int R0, int R1, int R2, float origin_x, float origin_y, float origin_z, float voxel_size, float sdf_trunc,
                      float alpha_trunc, float depth_trunc, int n_views, const GsTsdfView* views /*host array*/, float* volume,
                      void* stream);
size_t gs_tsdf_extract_ws_bytes(int R0, int R1, int R2);
int gs_tsdf_extract_count(int R0, int R1, int R2, const float* volume, void* ws, size_t ws_bytes, int64_t* counts, void* stream);
int gs_tsdf_extract_fill(int R0, int R1, int R2, float origin_x, float origin_y, float origin_z, float voxel_size, const float* volume,
                         void* ws, size_t ws_bytes, int64_t n_vertices, int64_t n_triangles, float* vertices, int64_t* faces,
                         void* stream);

/* ------------------------------------------------------------------ triangle-mesh rasterizer ------------- */
/* What TriangleMesh.render / visible_faces (rfstudio/graphics/_mesh/_triangle_mesh.py:496-555) get from nvdiffrast's rasterize and
 * interpolate with the NormalShader / DepthShader (antialias = False); a restatement of the semantics.  csrc/gs_meshraster.hip.
 *
 * Inputs: camera-space vertices vc [V,3] (OpenCV, +z forward), faces [F,3] int32 (F <= 2^24), fx fy cx cy, H W, near.
 *   xs = fx X / Z + cx,  ys = fy Y / Z + cy;  pixel j covers [j, j + 1), centre j + 0.5, row 0 on top.
 * Coverage: (xs, ys) are snapped to 1/256 px (rint); the three edge functions are 64-bit integers evaluated at
 *   (256 px + 128, 256 py + 128) and oriented by the sign of the snapped area; a pixel is inside when all three are > 0, or = 0 on a
 *   top or left edge (top-left rule: a pixel on a shared edge belongs to exactly one triangle).  A triangle is DROPPED whole (no
 *   clipping) when its snapped area is 0, any Z <= near, any snapped coordinate is outside +-2^22, or an index is outside [0, V).
 * cull: 0 none; 1 'back' keeps (camera - centroid) . ((v1 - v0) x (v2 - v0)) > 0, which is: snapped signed area
 *   (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) < 0.
 * Values at a covered pixel, from the unsnapped fp32 positions relative to the pixel centre q_i = (xs_i, ys_i) - centre:
 *   e_i = q_{i+1} x q_{i+2},  lambda_i = e_i / sum e (not clamped),  b_i = (lambda_i / Z_i) / sum_j lambda_j / Z_j,
 *   depth = 1 / sum_j lambda_j / Z_j   (evaluated as b_i = e_i / Z_i / N, depth = sum e / N, N = sum_j e_j / Z_j).
 * Depth test: the smallest fp32 depth wins, the lower face index on equal depth; a 64-bit atomic min of (depth bits << 32 | face),
 *   so the result does not depend on launch order.
 *
 *   gs_meshraster_ws_bytes  8 bytes per pixel + 4 per face + 32 (0: sizes out of range)
 *   gs_meshraster_fwd       fills the key buffer in `ws`.  `stats` (optional, device uint64[4], ADDED to) = {fragments and atomics of
 *                           the thread-per-triangle pass, fragments and atomics of the wave-per-triangle pass}
 *   gs_meshraster_resolve   ws -> rast [H,W,4] = (b0, b1, depth, face + 1), zeros where empty
 *   gs_meshraster_bwd       d_rast [H,W,4] (channels 0..2 used) -> d_vc [V,3] (overwritten), face ids fixed; no gradient from coverage
 *   gs_mesh_interp_fwd      out [P,C] = b0 a0 + b1 a1 + (1 - b0 - b1) a2 with a_i = attr[faces[f][i]] (attr [V,C]) or, with
 *                           per_face_vertex, attr[f][i] (attr [F,3,C]); zeros where empty
 *   gs_mesh_interp_bwd      d_out -> d_attr (overwritten; fp32 atomic adds) and d_rast [P,4] = (d b0, d b1, 0, 0) (may be null) */
size_t gs_meshraster_ws_bytes(int64_t F, int H, int W);
int gs_meshraster_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                      float near, int cull, void* ws, size_t ws_bytes, uint64_t* stats, void* stream);
int gs_meshraster_resolve(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H,
                          int W, float near, const void* ws, size_t ws_bytes, float* rast, void* stream);
int gs_meshraster_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                      float near, const float* rast, const float* d_rast, float* d_vc, void* stream);
int gs_mesh_interp_fwd(int64_t P, int C, int64_t F, int64_t V, int per_face_vertex, const float* rast, const int32_t* faces,
                       const float* attr, float* out, void* stream);
int gs_mesh_interp_bwd(int64_t P, int C, int64_t F, int64_t V, int per_face_vertex, const float* rast, const int32_t* faces,
                       const float* attr, const float* d_out, float* d_attr, float* d_rast, void* stream);

/* ------------------------------------------------------------------ near-plane and guard-band clipping --- */
/* The rasterizer above with the faces that cross the near plane CLIPPED instead of dropped (nvdiffrast clips; the reference's scene
 * configurations put the camera inside the mesh).  csrc/gs_meshclip_dev.h, the kernels in csrc/gs_meshraster.hip and gs_meshaa.hip.
 *
 * Classification: a vertex is inside iff Z > near (a NaN fails).  All three inside: a non-crossing face; it takes the code of
 *   gs_meshraster_* and gives its bits (it is still dropped whole when a snapped coordinate leaves +-2^22).  None inside, a non-finite
 *   coordinate or an index outside [0, V): dropped.  Otherwise a crossing face.
 * Clip of a crossing face: Sutherland-Hodgman in camera space against Z > near, then against the guard planes xs <= G, xs >= -G,
 *   ys <= G, ys >= -G with G = 16000 px, in homogeneous form (distances (G - cx) Z - fx X, (G + cx) Z + fx X, (G - cy) Z - fy Y,
 *   (G + cy) Z + fy Y, each one fma of a product; inside when >= 0): at most 8 vertices.  A new vertex is always computed from the
 *   inside endpoint A towards the outside endpoint B:  t = dA / (dA - dB),  C = fma(t, B - A, A) per coordinate, without contraction,
 *   so two faces that share the edge get the same bits and the same snapped vertex.  The polygon (v0 .. vn-1, the face's winding) is
 *   fan-triangulated into (v0, vk, vk+1), at most 6 sub-triangles.
 * Coverage: every sub-triangle is projected (xs = fma(fx, X / Z, cx)), snapped, set up and walked like a triangle above: top-left
 *   rule, cull on the sign of its snapped area, dropped on zero snapped area.  A pixel on an edge shared by two sub-triangles, two
 *   crossing faces, or a crossing and a non-crossing face is covered once.
 * Values of a crossing face, per FACE (not per sub-triangle), from its three original vertices, which may lie behind the eye: where
 *   the ray d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1) meets the plane of P0 P1 P2, solved relative to P0, every operation
 *   rounded once, no contraction:  e1 = P1 - P0, e2 = P2 - P0;  h = d x e2;  a = (e1x hx + e1y hy) + e1z hz;  g = P0 x e1;
 *   nu = (P0x hx + P0y hy) + P0z hz;  nv = (dx gx + dy gy) + gz;  nt = (e2x gx + e2y gy) + e2z gz;  r = -1 / a;
 *   b1 = nu r,  b2 = nv r,  depth = nt r,  b0 = (1 - b1) - b2.  (The same function as w_i = d . (P_{i+1} x P_{i+2}), b_i = w_i / sum w,
 *   depth = det[P0 P1 P2] / sum w.)  The fragment key and the resolve evaluate this one function.  rast[..., 3] = the face id + 1.
 * Depth test, determinism, F <= 2^24: as above.
 * Backward: face ids and the clip fixed.  (b1, b2, depth)^T = -M P0 with M = (h, e1 x d, e1 x e2)^T / a; the gradient of
 *   g0 b0 + g1 b1 + gz depth to vertex m is -b_m ((g1 - g0) h - g0 (e1 x d) + gz (e1 x e2)) / a, for all three original vertices.
 * Antialias: a crossing face with at least one surviving sub-triangle counts as a neighbour in the silhouette test; its side of the
 *   exit edge's line is decided on the snapped position of the polygon vertex that follows the edge's second endpoint (the face's vertex
 *   i + 2 for its half-edge i) in the clipped polygon; it does not count when the guard band removed that endpoint.  A pair whose
 *   foreground face is a crossing face blends nothing (decision 0, no gradient).
 * Not clipped: the far plane; images wider than the guard band (a non-crossing face beyond +-2^22 is still dropped whole).
 *
 *   gs_meshclip_ws_bytes    8 bytes per pixel + 8 per face + 48 (0: sizes out of range)
 *   gs_meshclip_fwd / _resolve / _bwd       the arguments of gs_meshraster_fwd / _resolve / _bwd; `stats` counts the crossing faces'
 *                           fragments and atomics with the wave-per-triangle pass
 *   gs_meshclip_aa_fwd / _bwd               the arguments of gs_meshaa_fwd / _bwd (below), on a rast made by gs_meshclip_* */
size_t gs_meshclip_ws_bytes(int64_t F, int H, int W);
int gs_meshclip_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                    float near, int cull, void* ws, size_t ws_bytes, uint64_t* stats, void* stream);
int gs_meshclip_resolve(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H,
                        int W, float near, const void* ws, size_t ws_bytes, float* rast, void* stream);
int gs_meshclip_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                    float near, const float* rast, const float* d_rast, float* d_vc, void* stream);
int gs_meshclip_aa_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                       float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                       float* out, int32_t* dbg, void* stream);
int gs_meshclip_aa_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                       float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                       const float* d_out, float* d_color, float* d_vc, void* stream);

/* ------------------------------------------------------------------ mesh silhouette antialiasing --------- */
/* What TriangleMesh.render gets from `dr.antialias(rgba, rast, projected, indices)` (_triangle_mesh.py:552-553); a restatement of the
 * semantics, not of nvdiffrast.  csrc/gs_meshaa.hip; faces are loaded, snapped and culled by the rasterizer's own device code.
 *
 * Topology: for every half-edge (f, i) -- edge i of face f runs between its vertices i + 1 and i + 2, opposite vertex i -- the other
 *   half-edges on the same undirected edge, any number of them.  The indices are labels (nothing is read through them); a half-edge
 *   whose two indices are equal has no neighbours.  Depends on `faces` only: build once, reuse across views and steps.
 * Pairs: pixels p and q = p + (1, 0) or p + (0, 1) whose rast[..., 3] differ.  Foreground a: the one with a face and the smaller
 *   rast[..., 2]; an empty pixel loses, the lower face id wins equal depths.  T = the face at a, b = the other pixel.
 * Exit edge: with T's snapped integer edge functions and top-left biases, edge i separates when E_i(a) + bias_i >= 0 and
 *   E_i(b) + bias_i < 0; the exit edge has the smallest E_i(a) / (E_i(a) - E_i(b)) (128-bit cross products), ties to the lower i.
 *   None: the pair blends nothing.
 * Silhouette: the pair blends only if no other face on the exit edge, among those the rasterizer keeps (near, range, area, cull),
 *   has its opposite vertex strictly on the other side of the edge's line from T's (sign of the snapped 64-bit cross product).
 * Weight: q1, q2 = unsnapped fp32 positions of the edge's endpoints relative to a's centre, s = +-1 from a to b;
 *   horizontal pair x* = (q1x q2y - q1y q2x) / (q2y - q1y) (vertical: x and y exchanged);  d = clamp(s x*, 0, 1);
 *   d > 0.5: out[b] += (d - 0.5) (color[a] - color[b]);   d < 0.5: out[a] += (0.5 - d) (color[b] - color[a]).
 *   out = color + the sum over a pixel's (at most four) pairs.  `cull` and `near` must be the rasterizer's.
 *
 *   gs_mesh_topology_bytes  size of the topology object for F faces: at most 60 bytes per half-edge (0: F out of range)
 *   gs_mesh_topology_build  faces [F,3] -> topo.  No workgroup waits on another.
 *   gs_meshaa_fwd           color [H,W,C] -> out [H,W,C]; a gather without atomics: two runs are bit-identical.  dbg (optional,
 *                           int32 [H,W,2]): the decisions of the pairs (p, p + (1,0)) and (p, p + (0,1)): 0 nothing blended, else
 *                           1 + exit edge + 4 (0: zero weight, 1: p receives, 2: the other pixel receives) + 16 (foreground is the other)
 *   gs_meshaa_bwd           d_out -> d_color [H,W,C] and d_vc [V,3] (both overwritten; d_vc may be null): d color is the transpose of
 *                           the blend, d vc goes through d with the decisions and the snap fixed, zero where d is clamped; six fp32
 *                           atomic adds per blended pair.  No gradient to rast. */
size_t gs_mesh_topology_bytes(int64_t F);
int gs_mesh_topology_build(int64_t F, const int32_t* faces, void* topo, size_t topo_bytes, void* stream);
int gs_meshaa_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                  float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color, float* out,
                  int32_t* dbg, void* stream);
int gs_meshaa_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                  float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                  const float* d_out, float* d_color, float* d_vc, void* stream);

/* ------------------------------------------------------------------ mesh shading: 2-D textures, split-sum PBR per pixel ------ */
/* What TriangleMesh.render(cameras, shader=PBRShader(envmap=...)) and PrettyShader(occlusion_type='none') compute per pixel
 * (rfstudio/graphics/shaders.py:44-105, 199-233), on a G-buffer.  csrc/gs_meshshade.hip.
 *
 * 2-D lookup  tex [Ht,Wt,C] fp32, C in 1..4, uv [P,2]; dr.texture(tex[None], uv, filter_mode='linear'), no mip chain.
 *   wrap:  u' = u - floor(u), x = u' Wt - 0.5, ix0 = floor(x) (may be -1), fx = x - ix0, taps at ix0 mod Wt and (ix0 + 1) mod Wt;
 *          y likewise with Ht.
 *   clamp: x = clamp(u Wt - 0.5, 0, Wt - 1), taps ix0 and min(ix0 + 1, Wt - 1) (the FG-LUT lookup, for C channels); the gradient
 *          is 0 in a clamped coordinate.
 *   value: top + fy (bot - top), top = t00 + fx (t10 - t00), bot = t01 + fx (t11 - t01), contraction off.
 *   The uv gradient is the derivative of the selected cell's bilinear patch.  A non-finite uv row gives zeros and no gradient.
 *   Tap indices are reduced into range in integer arithmetic, after the conversion of a value clamped to a finite range.
 * Texture2D.sample(uv) = the wrap lookup at (u (1 - 1/Wt) + 0.5/Wt, v (1 - 1/Ht) + 0.5/Ht) (_texture.py:168-175).
 *
 * Shading  rast [H,W,4] (only rast[..., 3] > 0 is read), position [H,W,3] world space, normal [H,W,3] unit, uv [H,W,2],
 *   kd [kd_h,kd_w,3], ks [ks_h,ks_w,3] = (occlusion, roughness, metallic), cam_pos[3] on the device.  Per covered pixel:
 *     kd, ks = Texture2D.sample(uv);  rough = ks[1], metal = ks[2];  spec = (1 - metal) 0.04 + kd metal;  diff = kd (1 - metal)
 *     wo = safe_normalize(cam_pos - position) ((0,0,1) below 1e-6);  d = n.wo
 *     bend_back_normal: n <- (d > 0 ? n : -n), d <- n.wo, ndv = d;   otherwise ndv = max(d, 1e-4)
 *     fg = LUT(ndv, rough) with clamp;  refl = 2 d n - wo
 *     l_diff = cube(base, n);  l_spec = cube_mip(levels, refl, mip_from_roughness(rough))      (TextureSplitSum.sample)
 *     visibility = max(1 - ks[0], min_visibility) (GS_OCC_TEXTURE) or 1 (GS_OCC_NONE)
 *     colour = (l_diff diff + l_spec (spec fg[0] + fg[1])) visibility
 *   A pixel with rast[..., 3] <= 0, or with a non-finite position, normal or uv, gets colour 0 and no gradient anywhere (the
 *   reference shades empty pixels from face 0 and hides them behind alpha 0).
 *   Gradients: every selection (texel, LUT cell, cube face, mip level, the ndv and visibility clamps, the bend) takes the
 *   derivative of the selected piece; 0 where a clamp is active.
 *
 *   gs_tex2d_fwd      out [P,C]; one thread per sample.
 *   gs_tex2d_bwd      d_uv [P,2] overwritten; d_tex [Ht,Wt,C] ACCUMULATED into (caller zeroes).
 *   gs_meshshade_fwd  color [H,W,3]; one thread per pixel, a gather without atomics: two runs are bit-identical.
 *   gs_meshshade_bwd  d_position, d_normal [H,W,3], d_uv [H,W,2] overwritten without atomics (bit-identical between runs, zero at
 *                     empty pixels); d_kd, d_ks and env_grad (base and every level) ACCUMULATED into (caller zeroes).  Arrays
 *                     that fit the block's LDS budget are summed there and flushed once per block: a 1x1 texture receives at
 *                     most one global atomic per channel and block.
 * All four return GS_EINVAL before touching the device for C outside 1..4, a texture dimension, H or W below 1, an unknown boundary
 * or occlusion mode, or a null required pointer.  P == 0 is a no-op. */
#define GS_TEX_WRAP      0
#define GS_TEX_CLAMP     1
#define GS_OCC_TEXTURE   0
#define GS_OCC_NONE      1
int gs_tex2d_fwd(int64_t P, int Ht, int Wt, int C, int boundary, const float* tex, const float* uv, float* out, void* stream);
int gs_tex2d_bwd(int64_t P, int Ht, int Wt, int C, int boundary, const float* tex, const float* uv, const float* d_out,
                 float* d_uv, float* d_tex, void* stream);
int gs_meshshade_fwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                     int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                     const GsEnv* env /*host*/, int occlusion, float min_visibility, int bend_back_normal, float* color, void* stream);
int gs_meshshade_bwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                     int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                     const GsEnv* env /*host*/, int occlusion, float min_visibility, int bend_back_normal, const float* d_color,
                     float* d_position, float* d_normal, float* d_uv, float* d_kd, float* d_ks, const GsEnvGrad* env_grad /*host*/,
                     void* stream);
/* The same shader with a per-pixel visibility map vis [H,W] (PBRShader(occlusion_type='ao' | 'ssao'), shaders.py:92-104): the
 * per-face values of gs_ray_ao below through the face ids, or any map the caller has.  With v = max(vis[p], min_visibility):
 *     GS_OCC_AO      colour = l_diff diff v + l_spec (spec fg[0] + fg[1])          (the diffuse term alone)
 *     GS_OCC_SCREEN  colour = (l_diff diff + l_spec (spec fg[0] + fg[1])) v
 *   every product rounded once, in this order; ks[0] is not read.  The kernels are those of gs_meshshade_fwd / _bwd, instantiated
 *   for the mode: a map of ones gives the bits of GS_OCC_NONE, forward and backward, in both modes, and GS_OCC_SCREEN's forward is
 *   fl(colour of GS_OCC_NONE * v) to the last bit.  Backward: GS_OCC_SCREEN scales the chain by v.  GS_OCC_AO runs the backward of
 *   GS_OCC_NONE (the same kernel) and a second launch adds the gradient of (v - 1) l_diff diff: to the base texels and the normal
 *   through the diffuse lookup, to kd, to the metallic channel of ks, and to uv; a pixel with v = 1 adds nothing.  vis is a
 *   constant: it receives no gradient, and the min_visibility clamp selects nothing that has one.  GS_EINVAL as above, for another mode or a null vis. */
#define GS_OCC_AO        2
#define GS_OCC_SCREEN    3
int gs_meshshade_vis_fwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                         int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                         const GsEnv* env /*host*/, int occlusion, float min_visibility, int bend_back_normal, const float* vis /*[H,W]*/,
                         float* color, void* stream);
int gs_meshshade_vis_bwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                         int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                         const GsEnv* env /*host*/, int occlusion, float min_visibility, int bend_back_normal, const float* vis /*[H,W]*/,
                         const float* d_color, float* d_position, float* d_normal, float* d_uv, float* d_kd, float* d_ks,
                         const GsEnvGrad* env_grad /*host*/, void* stream);

/* ------------------------------------------------------------------ ray-mesh queries: LBVH, shadow and closest-hit rays ------ */
/* What the reference's OptiX stages get from optix_build_bvh(ctx, vertices, indices, rebuild=1) and from the shadow test of
 * optix_env_shade (rfstudio/graphics/_mesh/_optix/c_src/envsampling/kernel.cu:101-118); a restatement of the semantics.
 * csrc/gs_bvh.hip.  No backward: the reference ignores the shadow boundary gradient (kernel.cu:97-99).
 *
 * Mesh: vertices [V,3] fp32, faces [F,3] int32, 1 <= F <= 2^30 (node indices are int32 and there are 2 F - 1 nodes; the Morton
 *   codes are 30 bits wide and need no limit of their own), V < 2^31.  A face with an index outside [0, V) or with a non-finite
 *   coordinate is INVALID: never hit, and its vertices are in no box.  A zero-area face is never hit.
 * Node buffer (the contract the tests walk): 2 F - 1 nodes of 32 bytes, 16-byte aligned,
 *     struct { float lo[3], hi[3]; int32_t left; int32_t skip; }
 *   Nodes 0 .. F - 2 are internal (node 0 is the root), node F - 1 + i is the leaf of the i-th face in (Morton code, face index)
 *   order; with F = 1 node 0 is that leaf.  Internal: left = left child, and the right child is nodes[left].skip.  Leaf: left =
 *   face index.  skip = the node that follows this node's subtree in depth-first (left before right) order, -1 after the last.
 *   lo / hi = exact min / max over the vertices of the valid faces below the node; (+inf, -inf) when there are none.  The Morton
 *   code of a face: 10 bits per axis of its centroid inside the bounds of the valid faces, x in the highest bit; invalid faces
 *   sort last.  The tree is Karras 2012 over the stably sorted codes, equal codes told apart by their sorted position: two builds
 *   of the same mesh give the same bytes.
 * Ray: origin o, direction d (any length; t is in units of |d|), 0-based ray r = p S + s uses origins[p] and dirs[r]
 *   (dirs_per_point = 1, dirs [P,S,3]) or dirs[s] (dirs_per_point = 0, dirs [S,3] shared by all points).  A ray with a non-finite
 *   origin or a zero or non-finite direction misses everything.
 * Triangle test: Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection" (JCGT 2013): kz = the axis of the largest |d|, kx, ky
 *   the next two (swapped when d[kz] < 0), Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; per vertex A = v - o,
 *   Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz]; U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax in fp32 without
 *   contraction, recomputed in fp64 when one of them is exactly 0.  Hit iff U, V, W are all >= 0 or all <= 0, det = U + V + W != 0,
 *   and tmin < t < tmax (both strict) for t = ((U Az + V Bz) + W Cz) / det with Az = Sz A[kz] -- the fp32 value the kernel computes.
 *   Both sides, no culling.  A ray through a shared edge or vertex hits at least one of the triangles around it.
 *   Barycentrics (b1, b2) = (V, W) / det weigh vertices 1 and 2.
 * gs_ray_occluded: out[r] = 1 iff some face is hit.  gs_ray_closest: the hit with the smallest fp32 t, the lowest face index among
 *   equal t (the rasterizer's depth rule); a miss gives t = +inf, face = -1, bary = 0.  Neither depends on traversal order.
 * bvh = NULL: every ray tests every face with the same device routine.  That form defines the semantics; with a node buffer the
 *   result is the same bit for bit (the box test is conservative).  A traversal visits at most 2 F - 1 nodes and range-checks every
 *   index it reads, so a corrupt node buffer gives misses, not a hang or a fault.
 *
 *   gs_bvh_bytes      32 (2 F - 1) (0: F out of range)          gs_bvh_ws_bytes   build workspace, about 60 bytes per face (0: same)
 *   gs_bvh_build      a full build into `bvh`; rebuilding after the vertices moved is the same call.  No workgroup waits on another.
 * All return GS_EINVAL before touching the device for F < 1 ("empty mesh"), F > 2^30 ("too many faces"), a buffer or workspace that
 * is too small, negative P or S, P S >= 2^31, or a null required pointer.  P S == 0 is a no-op. */
size_t gs_bvh_bytes(int64_t F);
size_t gs_bvh_ws_bytes(int64_t F);
int gs_bvh_build(int64_t V, int64_t F, const float* vertices, const int32_t* faces, void* bvh, size_t bvh_bytes, void* ws,
                 size_t ws_bytes, void* stream);
int gs_ray_occluded(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh /* NULL: brute force */,
                    int64_t P, int S, const float* origins /*[P,3]*/, const float* dirs, int dirs_per_point /* 1: [P,S,3], 0: [S,3] */,
                    float tmin, float tmax, uint8_t* out /*[P,S]*/, void* stream);
int gs_ray_closest(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh /* NULL: brute force */,
                   int64_t P, int S, const float* origins /*[P,3]*/, const float* dirs, int dirs_per_point, float tmin, float tmax,
                   float* t /*[P,S]*/, int32_t* face /*[P,S]*/, float* bary /*[P,S,2]*/, void* stream);

/* ------------------------------------------------------------------ ambient occlusion: rays to targets ------------------------ */
/* The per-face visibility of the reference's mesh shaders.  csrc/gs_ao.hip; tests/ao_ref.py restates it in float64.  Everything
 * below is fp32 with contraction off, every operation rounded once, sums of three products as (a + b) + c.  No backward:
 * TriangleMesh.compute_ambient_occlusion is no_grad and the map is piecewise constant in the geometry.
 *
 * gs_ray_ao: cosine-weighted visibility of P points towards S shared target points; what compute_ambient_occlusion
 *   (rfstudio/graphics/_mesh/_triangle_mesh.py:616-678) computes per face, its cameras being the targets.  The mesh, `bvh` (NULL:
 *   brute force, the same bits) and the segment test are those of gs_ray_occluded.  positions, normals [P,3]; targets [S,3],
 *   1 <= S <= 4096.  Per point:
 *     o = pos + n * offset
 *     per target k:  d = e_k - o (not normalised);  c = ((n.x d.x + n.y d.y) + n.z d.z) / sqrt((d.x^2 + d.y^2) + d.z^2)
 *       the target COUNTS iff c > 0 (a NaN does not), with weight w = max(c, 1e-4)
 *       hit = the ray o + t d meets a face for 0 < t < 1 (gs_ray_occluded with tmin = 0, tmax = 1 on these o and d)
 *       num += w unless hit;  den += w
 *     vis[p] = num / max(den, 1e-6);  0 for a point with a non-finite position or normal, or without a counting target.
 *   Sums: lanes_per_point = G in {1, 16, 64} (0 picks 64 for S >= 64, 16 for S >= 16, else 1) lanes share a point; lane l adds the
 *   targets k = l, l + G, ... in ascending k, then the lanes are combined by v += shfl_xor(v, o) for o = G/2, ..., 1.  No atomics:
 *   the same input and G give the same bits.  G changes the order of the sums only.
 *   log_hit [P,S] uint8 and log_w [P,S] (both or neither; NULL: no log) receive hit and w of every target of a finite point; with
 *   the log, hit is evaluated for the targets that do not count too (w = 0 there).  Rows of a non-finite point are not written.
 *   Against the reference: no 1024^2 pixel quantisation of the test; its depth tolerance of 0.02 becomes `offset` along the normal;
 *   back-facing targets are left out, where the reference counts them as occluded with weight 1e-4.
 *
 * GS_EINVAL before touching the device for S outside its range, sizes out of range, a non-finite offset or a null required
 * pointer.  P == 0 is a no-op. */
int gs_ray_ao(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh /* NULL: brute force */, int64_t P,
              const float* positions /*[P,3]*/, const float* normals /*[P,3]*/, int S, const float* targets /*[S,3]*/, float offset,
              int lanes_per_point, float* vis /*[P]*/, uint8_t* log_hit /*[P,S] or NULL*/, float* log_w /*[P,S] or NULL*/, void* stream);

/* ------------------------------------------------------------------ nearest neighbours: uniform grid, Chamfer backward ---------- */
/* What the reference's geometry metrics get from its brute-force Chamfer kernel (rfstudio/loss/_chamfer) and from Points.k_nearest;
 * a restatement of the semantics, and a semantics of this project's own where the reference leaves it to the hardware.
 * csrc/gs_nn.hip; tests/chamfer_ref.py states the same in numpy.
 *
 * Set: points [M,3] fp32, 1 <= M <= 2^30.  Queries [N,3] fp32, 0 <= N <= 2^30.
 * Distance (to the bit): dx = q.x - p.x, dy, dz likewise; d = (dx*dx + dy*dy) + dz*dz, every operation one fp32 round-to-nearest,
 *   no FMA contraction.  d is the SQUARED distance and is never square-rooted here.
 * Answer (to the bit): the lexicographically smallest pair (d, index) over the set points whose three coordinates are finite -- among
 *   equal d the lowest index into the caller's array, whatever the traversal order.  A set point with a non-finite coordinate is
 *   never returned.  A query with a non-finite coordinate, or a set without a finite point, gives d = +inf, index = -1.  (Two finite
 *   points far enough apart overflow to d = +inf with a valid index.)
 * k-nearest: dist, index [N,k], 1 <= k <= 8: the k smallest pairs in ascending order, padded with (+inf, -1).
 * grid = NULL: every query meets every point through LDS tiles with the same distance routine.  That form defines the semantics; with
 *   a grid the result is the same bit for bit.
 * Grid buffer (opaque): a 256-byte header written on the device, cell starts, and one 16-byte (x, y, z, index bits) record per point
 *   in (cell, index) order.  About M / 4 cells and at most 2^21, per-axis resolution proportional to the extent of the finite points,
 *   one cell along an axis without extent.  The query searches Chebyshev shells of cells around the query's (clamped) cell and stops
 *   after a shell only when the k-th best d is STRICTLY below a conservative lower bound on the fp32 d of every point outside the
 *   searched cube, or when the cube covers the grid: a query far outside the box degrades to a scan of the set.  Every index read
 *   from the buffer is range-checked: a buffer that holds no grid of this set gives wrong answers, not a fault or a hang.
 *
 *   gs_nn_grid_bytes  256 + 4 (cells + 1) + 16 M, rounded (0: M out of range)     gs_nn_ws_bytes  build workspace, about 40 M (0: same)
 *   gs_nn_build       a full build into `grid`; rebuilding after the points moved is the same call.  Nothing is read back and no
 *                     workgroup waits on another.
 *   gs_nn_query       dist [N,k], index [N,k] overwritten.
 *   gs_chamfer_bwd    the backward of (dist1, dist2) = (nearest of xyz1 in xyz2, nearest of xyz2 in xyz1) at the indices of the
 *                     forward: with g = 2 grad1[j] and i = idx1[j], row j of grad_xyz1 gets g (xyz1[j] - xyz2[i]) and row i of
 *                     grad_xyz2 the negative; the other direction likewise.  grad_xyz1 [N1,3] and grad_xyz2 [N2,3] are WRITTEN: every
 *                     row is first overwritten with its own term (plain stores), the scattered terms are then added with fp32 atomics
 *                     in a later launch -- no caller-side zeroing.  A row whose index is -1 (or outside the other set) contributes
 *                     nothing and gets zeros as its own term.
 * All return GS_EINVAL before touching the device for M < 1 ("empty set"), M > 2^30, k outside [1, 8], a buffer or workspace that is too
 * small or not 16-byte aligned, negative N, or a null required pointer.  N == 0 is a no-op. */
size_t gs_nn_grid_bytes(int64_t M);
size_t gs_nn_ws_bytes(int64_t M);
int gs_nn_build(int64_t M, const float* points, void* grid, size_t grid_bytes, void* ws, size_t ws_bytes, void* stream);
int gs_nn_query(int64_t M, const float* points, const void* grid /* NULL: brute force */, int64_t N, const float* queries, int k,
                float* dist /*[N,k]*/, int32_t* index /*[N,k]*/, void* stream);
int gs_chamfer_bwd(int64_t N1, int64_t N2, const float* xyz1, const float* xyz2, const int32_t* idx1 /*[N1]*/,
                   const int32_t* idx2 /*[N2]*/, const float* grad1 /*[N1]*/, const float* grad2 /*[N2]*/, float* grad_xyz1,
                   float* grad_xyz2, void* stream);

/* ------------------------------------------------------------------ Monte-Carlo environment shading on the ray routines --------- */
/* What the reference's stage 2 gets from optix_env_shade (rfstudio/graphics/_mesh/_optix: ops.py, c_src/envsampling/kernel.cu,
 * c_src/bsdf.h); a restatement of the semantics.  csrc/gs_envshade.hip; tests/envshade_ref.py states the same in float64.
 *
 * Points: mask [P], ro (shadow-ray origins), gb_pos, gb_normal, gb_kd, gb_ks [P,3] fp32, one view_pos [3].  gb_ks = (occlusion factor,
 *   roughness, metallic).  Light: light [H,W,3] lat-long radiance and its tables pdf [H,W], rows [H] (CDF over rows), cols [H,W] (CDF
 *   inside each row), H, W >= 2.  perms [T, n^2] int32 (T >= 1 permutations of 0 .. n^2 - 1), n = n_samples_x >= 1, 0 <= rnd_seed < 2^31.
 *   bsdf: 0 pbr, 1 diffuse, 2 white (1 and 2: Lambert only).  Mesh and node buffer as for the ray queries; the node buffer is required.
 * Per point p with mask > 0 (the others get zeros):
 *   stream  state = out(seed) ^ out(p) with out() the PCG output function and the LCG s -> 747796405 s + 2891336453 (mod 2^32); draws
 *     in order: light table = draw % T, bsdf table = draw % T, then per iteration i < n^2 five uniforms (draw & 0xFFFFFF) / 2^24.  Sample
 *     (p, i) has the same numbers however the work is laid out (a lane enters the stream 2 + 5 i draws in).
 *   light sample  (sx, sy) = ((perm % n, perm / n) + (u0, u1)) / n in fp32 without contraction; row from `rows`, column from that row
 *     of `cols` by ceil(log2(size - 1)) + 1 bisection steps on min(x, 0.99999994f), position inside the texel = remainder / width;
 *     direction (sin t sin f, cos t, -sin t cos f), f = (2 u - 1) pi, t = v pi.  Its density: pdf[nearest texel of the direction]
 *     W H / (2 pi^2 max(sin t, 1e-4)); the BSDF's mixture pdf of it is 1 when min(n.wo, n.wi) < 1e-6.
 *   bsdf sample  pDiffuse = (1 - metallic) Y(kd) / (that + Y(Schlick(f0, cos))) (1 when both are 0); u4 < pDiffuse: cosine lobe on the
 *     branchless basis of the unit normal, otherwise the GGX lobe of visible normals (Heitz 2018) at alpha = roughness^2, reflected;
 *     pdf = the mixture, a component added only when its weight exceeds 1e-6; pDiffuse < 1e-4 with the diffuse lobe chosen returns the
 *     normal with pdf 1; a viewer at or below the horizon of the GGX lobe gives the zero direction with pdf 0.
 *   each of the 2 n^2 samples  L = light[nearest texel], diffuse = max(n.wi / pi, 0), specular (pbr only) = F D G / (4 n.wo) with every
 *     cosine clamped to [1e-4, 1 - 1e-4], alpha = clamp(roughness^2, 0.08^2, 1), f0 = (0.04 (1 - m) + kd m)(1 - ks.x), 0 unless n.wo and
 *     n.wi exceed 1e-4; w = 1 / (n^2 max(pdf_light + pdf_bsdf, 1e-4)); vis = 0 if the ray (ro, wi) hits any face for 0 < t < 1e16, else 1;
 *     V = vis shadow_scale + 1 - shadow_scale.  diff += diffuse L V w, spec += specular L V w, resi += (diffuse, mean specular)(1 - V) w.
 * gs_envshade_fwd  diff, spec [P,3], resi [P,2] overwritten, no atomics: the same inputs give the same bits.  log_dirs [P, 2 n^2, 3],
 *   log_pdf_sum, log_vis [P, 2 n^2]: all three or none; slot 2 i is the light sample of iteration i, 2 i + 1 its BSDF sample; only
 *   slots of points with mask > 0 are written.  Without them that code is not compiled into the kernel that runs.
 * gs_envshade_bwd  regenerates the samples from ITS rnd_seed; directions, pdfs and V are constants (no gradient through them, none to
 *   resi).  gb_pos_grad, gb_normal_grad, gb_kd_grad, gb_ks_grad [P,3] overwritten without atomics; light_grad [H,W,3] ACCUMULATED into
 *   on nearest texels (caller zeroes) with float atomics, after merging the adds of a wave that share a texel in up to merge_rounds
 *   leader rounds (-1: default).
 * lanes_per_point: 1 (a thread per point), 16 or 64 lanes share a point's iterations; 0 picks the default.  The arrangement changes
 *   the order of the per-point sums, nothing else.
 * Both return GS_EINVAL before touching the device for negative P, H or W below 2, T or n below 1, a seed outside [0, 2^31), an
 *   unknown bsdf or arrangement, an empty mesh, or a null required pointer.  P == 0 is a no-op. */
int gs_envshade_fwd(int64_t P, const float* mask, const float* ro, const float* gb_pos, const float* gb_normal, const float* view_pos,
                    const float* gb_kd, const float* gb_ks, int H, int W, const float* light, const float* pdf, const float* rows,
                    const float* cols, int T, int n_samples_x, const int32_t* perms, int64_t rnd_seed, int bsdf, float shadow_scale,
                    int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int lanes_per_point, float* diff,
                    float* spec, float* resi, float* log_dirs, float* log_pdf_sum, float* log_vis, void* stream);
int gs_envshade_bwd(int64_t P, const float* mask, const float* ro, const float* gb_pos, const float* gb_normal, const float* view_pos,
                    const float* gb_kd, const float* gb_ks, int H, int W, const float* light, const float* pdf, const float* rows,
                    const float* cols, int T, int n_samples_x, const int32_t* perms, int64_t rnd_seed, int bsdf, float shadow_scale,
                    int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int lanes_per_point,
                    int merge_rounds, const float* diff_grad, const float* spec_grad, float* gb_pos_grad, float* gb_normal_grad,
                    float* gb_kd_grad, float* gb_ks_grad, float* light_grad, void* stream);

/* ------------------------------------------------------------------ bilateral denoiser of the Monte-Carlo estimates ------------- */
/* What the reference's stages 2 and 3 get from bilateral_denoiser (rfstudio/graphics/_mesh/_optix: ops.py:107-140,
 * c_src/denoising.cu); a restatement of the semantics.  csrc/gs_denoise.hip; tests/denoise_ref.py states the same in float64.
 *
 * col [B,H,W,C] with 1 <= C <= 8 (the reference: 3), nrm [B,H,W,3], zdz [B,H,W,zdz_channels] with 1 or 2 channels: z = channel 0, dz = the
 *   last channel (one channel: dz = z), all fp32.  R = 2 ceil(2.5 sigma) + 1 <= 127 and v = sigma^2, sigma a finite positive double.
 * For a centre p and every tap q = p + (fx, fy), |fx|, |fy| <= R, inside the image, fy outer and fx inner:
 *   w = exp(-(fx^2 + fy^2) / (2 v)) * clamp(nrm[q] . nrm[p], 1e-4, 1)^128 * exp(-|z[q] - z[p]| / max(dz[p] sqrt(fx^2 + fy^2), 1e-4))
 * gs_denoise_fwd  wsum[p] = max(sum_q w, 1e-4) and out[p] = sum_q w col[q] / wsum[p] -- the reference's four-channel output and the
 *   division its wrapper applies.  out [B,H,W,C] and wsum [B,H,W] are overwritten.
 * gs_denoise_bwd  col_grad[p] = sum_q w(q<-p) out_grad[q] / wsum[q], with w(q<-p) the weight q gave the tap p: the forward's weight
 *   with dz[q] in the depth denominator.  The gradient reaches col only.  col_grad [B,H,W,C] is overwritten.
 * Both are gathers without atomics: the same inputs give the same bits, a C-channel call gives the bits of calls on its channel slices,
 *   and the two forms agree bit for bit.  tiled: 1 stages the window halo in LDS (GS_EINVAL when it does not fit), 0 reads the taps
 *   from global memory, -1 picks (the tiled form where gs_denoise_tiled_fits, except for H < 8).  gs_denoise_tiled_fits is 1 when the
 *   halo of this C and sigma fits, for both directions alike; it touches no device.
 * Both return GS_EINVAL before touching the device for B, H or W below 1, C outside 1..8, zdz_channels not 1 or 2, sigma not finite and
 *   positive or with R > 127, B or H / 8 above 65535, an unknown form, or a null pointer. */
int gs_denoise_tiled_fits(int C, double sigma);
int gs_denoise_fwd(int B, int H, int W, int C, int zdz_channels, const float* col, const float* nrm, const float* zdz, double sigma,
                   int tiled, float* out, float* wsum, void* stream);
int gs_denoise_bwd(int B, int H, int W, int C, int zdz_channels, const float* nrm, const float* zdz, double sigma, int tiled,
                   const float* wsum, const float* out_grad, float* col_grad, void* stream);

/* ------------------------------------------------------------------ environment resampling, relighting background ------------- */
/* What the reference gets from TextureCubeMap.as_latlng / visualize / sample / render and TextureLatLng.as_cubemap
 * (rfstudio/graphics/_mesh/_texture.py:359-377, :411-465); a restatement of the semantics.  csrc/gs_envmap.hip; tests/envmap_ref.py
 * states the same in float64.
 *
 * cube [6,R,R,3] with 1 <= R <= 4096, latlng [H,W,3] with H, W >= 2 (row 0 is the +y pole: rows run y-DOWN), all fp32.
 * Cube lookups are the seam-aware bilinear lookup of gs_cube_sample_linear (csrc/gs_cube.h: edge taps re-projected onto the
 * neighbouring face, the missing corner tap the mean of the other three, zeros for a zero or non-finite direction; the length of the
 * direction does not matter).  The lat-long lookup is gs_tex2d_fwd's with GS_TEX_WRAP: texel centres at u W - 0.5, wrapped in both axes.
 * transform: DEVICE pointer to 9 floats, row-major [3,3], or NULL for the identity.  linspace(a, b, n)[k] = a + k (b - a) / (n - 1).
 *
 * gs_env_cube_to_latlng_fwd   out[i,j] = cube(T d), d = (sin t sin p, cos t, -sin t cos p) with t = pi linspace(1/H, 1 - 1/H, H)[i]
 *                             (the reference's end points, not the row centres) and p = pi linspace(-1 + 1/W, 1 - 1/W, W)[j].
 * gs_env_cube_to_latlng_bwd   d_cube [6,R,R,3] ADDED to (caller zeroes): the texel gradient of the above for d_out [H,W,3].
 * gs_env_latlng_to_cube_fwd   out[s,y,x] = latlng(tu, tv) with g = linspace(-1 + 1/R, 1 - 1/R, R), v = normalize(face point of
 *                             (s, g[x], g[y])), tu = atan2(v0, -v2) / (2 pi) + 0.5, tv = acos(clamp(v1, -1, 1)) / pi.
 * gs_env_latlng_to_cube_bwd   d_latlng [H,W,3] ADDED to (caller zeroes): the texel gradient of the above for d_out [6,R,R,3].
 * gs_cube_sample_linear_bwd   d_tex [6,R,R,3] ADDED to (caller zeroes): the texel gradient of gs_cube_sample_linear for d_out [n,3]
 *                             (scale as in the forward).  No gradient reaches the directions.
 * gs_env_background_fwd       out[i,j] = cube(T Rc ((0.5 - cx + j) / fx, -(0.5 - cy + i) / fy, -1)) for the [H,W] pixels of a camera;
 *                             c2w: DEVICE pointer to 12 floats, row-major [3,4], OpenGL convention, Rc its rotation.  srgb != 0 applies
 *                             rgb2srgb (c <= 0.0031308 ? 12.92 c : 1.055 c^(1/2.4) - 0.055) per channel, srgb == 0 leaves radiance.
 * One thread per output element, directions in registers.  The forwards are gathers: the same inputs give the same bits.  The
 * backwards recompute the footprint and use float atomics (sums in arrival order).  All return GS_EINVAL before touching the device
 * for R outside 1..4096, H or W below 2 (the background: below 1), H W above 2^28, zero or non-finite intrinsics, or a null required
 * pointer.  n == 0 is a no-op. */
int gs_env_cube_to_latlng_fwd(int R, int H, int W, const float* cube, const float* transform, float* out, void* stream);
int gs_env_cube_to_latlng_bwd(int R, int H, int W, const float* transform, const float* d_out, float* d_cube, void* stream);
int gs_env_latlng_to_cube_fwd(int H, int W, int R, const float* latlng, float* out, void* stream);
int gs_env_latlng_to_cube_bwd(int H, int W, int R, const float* d_out, float* d_latlng, void* stream);
int gs_cube_sample_linear_bwd(int64_t n, int R, const float* dirs, float scale, const float* d_out, float* d_tex, void* stream);
int gs_env_background_fwd(int R, int H, int W, const float* cube, float fx, float fy, float cx, float cy, const float* c2w,
                          const float* transform, int srgb, float* out, void* stream);

/* ------------------------------------------------------------------ mesh-prior regularisers ------------------------------------ */
/* The three mesh regularisers the reference's GeoSplatterPrior deforms a mesh under (rfstudio/model/geosplat_prior.py: a uniform
 * Laplacian term, pytorch3d's mesh_edge_loss and mesh_normal_consistency), on a topology built once; a restatement of the published
 * formulas.  csrc/gs_meshreg.hip; geosplatting_amd/meshreg.py builds the topology; tests/meshreg_ref.py states the same in float64.
 *
 * vertices [V,3] fp32.  edges [E,2] int32 (lo, hi), lo < hi, unique.  pairs [P,4] int32 (v0, v1, a, b): two faces on the side
 * (v0, v1), a and b their opposite vertices.  nbr_off [V+1], nbr [2E]: per vertex its distinct neighbours, ascending (CSR).
 * pr_off [V+1], pr [4P]: per vertex the codes 4 pair + role (role 0..3 = v0, v1, a, b) of its appearances in pairs, ascending (CSR).
 * long_verts [NL]: the vertices with more than 64 neighbours or more than 64 codes, ascending; a wave walks their lists, a lane the
 *   others'.  Every index must be inside its array: the kernels do not check.
 * Terms:  lap_i  = |deg_i v_i - sum_{j in N(i)} v_j|                                  (0 for a vertex without neighbours)
 *         edge_e = (|v_lo - v_hi| - target_length)^2
 *         nc_p   = 1 - (n0 . -n1) / (max(|n0|, 1e-8) max(|n1|, 1e-8)),  n0 = (v1 - v0) x (a - v0),  n1 = (v1 - v0) x (b - v0)
 * gs_meshreg_fwd  terms [V+E+P] (lap, then edge, then nc) and out [3] = (mean lap, mean edge, mean nc; 0 for an empty set) overwritten.
 *   partials: gs_meshreg_partial_rows(V, E, P, NL) x 3 doubles of workspace: a workgroup's sums per term in a fixed order, added by a
 *   final one-workgroup pass in double.  lap_dir [V,3] and pair_grad [P,4,3]: both or none; what the backward gathers (the unit
 *   Laplacian vectors, d nc_p / d (v0, v1, a, b)); a zero-length vector under a norm gives the zero subgradient.
 * gs_meshreg_bwd  grad [V,3] overwritten with out_grad[0] d(mean lap) + out_grad[1] d(mean edge) + out_grad[2] d(mean nc); out_grad: DEVICE
 *   pointer to 3 floats.  A gather per vertex through nbr and pr.
 * No atomics in either: the same inputs give the same bits.  Both return GS_EINVAL before touching the device for a negative count,
 *   V + E + P or 4 P above 2^30, or a null required pointer (an array of a zero count may be null). */
int gs_meshreg_partial_rows(int V, int E, int P, int NL);
int gs_meshreg_fwd(int V, int E, int P, int NL, const float* vertices, const int32_t* edges, const int32_t* pairs, const int32_t* nbr_off,
                   const int32_t* nbr, const int32_t* pr_off, const int32_t* long_verts, float target_length, float* terms, float* lap_dir,
                   float* pair_grad, double* partials, float* out, void* stream);
int gs_meshreg_bwd(int V, int E, int P, int NL, const float* vertices, const int32_t* nbr_off, const int32_t* nbr, const int32_t* pr_off,
                   const int32_t* pr, const int32_t* long_verts, float target_length, const float* lap_dir, const float* pair_grad,
                   const float* out_grad, float* grad, void* stream);

/* ------------------------------------------------------------------ differentiable Poisson surface reconstruction -------------- */
/* TriangleMesh.from_diff_poisson_reconstruction (rfstudio/graphics/_mesh/_triangle_mesh.py:301-319) through Shape-as-Points,
 * rfstudio/graphics/_mesh/_dpsr/ops.py: point_rasterize, grid_interp, the Fourier-space step of DPSR.forward and the vertex normals
 * PSR2Mesh returns; a restatement of the semantics.  csrc/gs_poisson.hip, weights in csrc/gs_gridinterp_dev.h.  The FFTs, the
 * shift / scale step and the means stay with the caller (torch.fft is hipFFT).
 *
 * Grid: [C, R0, R1, R2] float, the LAST axis fastest; every side >= 4, R0 R1 R2 < 2^31; node i sits at i / R per axis of the unit
 * cube and the grid is periodic.  C in [1, 4], N < 2^31.
 * Row rule (splat, sample and both backward kernels): a row takes part iff its three coordinates are finite and |p| < 1024,
 *   decided on the floats before any conversion to an integer.  Other rows add nothing to a grid, read 0 from one and get a zero
 *   gradient.  A finite p outside [0, 1) wraps (the reference raises for p = 1.0).
 * Weights, per axis and in this order: w = p - floor(p);  s = w R;  lo = floor(s) (R -> 0);  hi = (lo + 1) mod R;  f = s - floor(s)
 *   (exact);  lower node 1 - f, upper node f;  corner k (bit 2: axis 0, bit 1: axis 1, bit 0: axis 2) has weight (w0 w1) w2.
 *
 * gs_grid_splat: grid[c, node] = sum over rows and corners of weight * values[n, c].  Bitwise reproducible: every addend
 *   t = fp32(weight * value) enters a 64-bit integer accumulator as rint(t 2^e), e = 62 - exponent(N max|v|) with max|v| reduced
 *   on the device over the rows that take part (no node sum can overflow; an addend is exact to 2^-e), and the node's float is the
 *   sum times 2^-e, rounded once.  Integer sums do not depend on the order.  A NaN or inf VALUE in a row that takes part makes the
 *   whole grid NaN.  ws: gs_grid_splat_ws_bytes = 16 + 8 C R0 R1 R2 (0: out of range); the call clears it.
 * gs_grid_sample_fwd: out[n, c] = sum_k weight_k grid[c, node_k], k = 0..7 in order, fused multiply-adds.
 * gs_grid_sample_bwd: g_points[n, a] = sum_k (d weight_k / d p_a) sum_c cot[n, c] grid[c, node_k]; d weight_k / d p_a = +-R_a times
 *   the two other axes' weights.  A gather per point, no atomics.  The gradient of the sample to its grid is gs_grid_splat(points,
 *   cot); the gradients of the splat are gs_grid_sample_fwd(g_grid, points) to the values and gs_grid_sample_bwd(g_grid, points,
 *   values) to the points.
 *
 * gs_poisson_spectral_fwd: S [3, R0, R1, R2/2+1] complex64 (rfftn of the three splatted normal components) -> Phi [R0, R1, R2/2+1]:
 *     k_a = i if i <= (R_a - 1) / 2 else i - R_a  on axes 0 and 1 (fftfreq: the Nyquist term of an even side is -R/2),  k_2 = i
 *     (rfftfreq: +R/2);  omega_d = fp32(k_d) fp32(2 pi);  G = fp32(exp(-2 sigma^2 |k|^2)) evaluated in float64;
 *     Phi = [sum_d (-i) (G S_d) omega_d] / (-(omega_0^2 + omega_1^2 + omega_2^2) + 1e-6),  d = 0, 1, 2 in order;  Phi(0,0,0) = 0.
 *   IEEE division, no contraction.  _bwd is the adjoint torch's complex autograd expects of a linear map:
 *     g_S_d = conj(c_d) g_Phi,  c_d = -i G omega_d / denominator  (0 at DC).
 *
 * gs_grid_pack_volume: volume[n] = (phi[n], 1): the interleaved volume of gs_tsdf_extract_* called with (R2, R1, R0), whose fastest
 *   axis is then phi's last.  Its vertices come back as (axis 2, axis 1, axis 0); swapping them is a reflection, so the caller also
 *   flips the winding.
 * gs_grid_vertex_normals: vertices [V,3] in NODE units on grid edges (two integer coordinates).  The gradient at a node is the
 *   periodic central difference 0.5 R_a (phi[i + e_a] - phi[i - e_a]); it is interpolated linearly between the edge's two nodes and
 *   normalised (scaled by its largest component first).  A gradient of exactly 0, or a non-finite vertex, gives (0, 0, 0).  Every
 *   index is wrapped: no vertex addresses outside phi. */
size_t gs_grid_splat_ws_bytes(int C, int R0, int R1, int R2);
int gs_grid_splat(int64_t N, int C, int R0, int R1, int R2, const float* points, const float* values, float* grid, void* ws,
                  size_t ws_bytes, void* stream);
int gs_grid_sample_fwd(int64_t N, int C, int R0, int R1, int R2, const float* grid, const float* points, float* out, void* stream);
int gs_grid_sample_bwd(int64_t N, int C, int R0, int R1, int R2, const float* grid, const float* points, const float* cot,
                       float* g_points, void* stream);
int gs_poisson_spectral_fwd(int R0, int R1, int R2, double sigma, const float* S, float* Phi, void* stream);
int gs_poisson_spectral_bwd(int R0, int R1, int R2, double sigma, const float* g_Phi, float* g_S, void* stream);
int gs_grid_pack_volume(int R0, int R1, int R2, const float* phi, float* volume, void* stream);
int gs_grid_vertex_normals(int R0, int R1, int R2, const float* phi, int64_t V, const float* vertices, float* normals, void* stream);

/* ------------------------------------------------------------------ mesh decimation and connected components ------------------- */
/* Garland-Heckbert quadric error metrics run as rounds of independent edge collapses, and the component filter that goes with it:
 * the "cropping and simplifying" the reference leaves to outside tools before its prior flow.  csrc/gs_simplify.hip; the caller
 * (geosplatting_amd/meshsimplify.py) rebuilds the index arrays of a round with sorts, tests/simplify_ref.py restates the rule in
 * float64 numpy.  V, F and E are at most 2^30; every index must be inside its array: the kernels do not check.
 *
 * Index arrays of a round (all int32 unless noted):
 *   faces [F,3]; edges [E,2] the unique undirected sides (lo, hi), ascending by lo V + hi -- the position is the edge index i;
 *   edge_faces [E] the number k of faces of an edge; edge_opp [E,2] the vertices opposite to the edge in its first two faces (-1: none);
 *   nbr_off [V+1], nbr [2E] the neighbours of a vertex, ascending; vf_off [V+1], vf [3F] the faces of a vertex, ascending;
 *   side_boundary [3F] uint8: side j of face f (corner j to corner j + 1) belongs to an edge with one face;
 *   boundary [V] uint8: the vertex is on such an edge.
 *
 * gs_simplify_quadrics  quadrics [V,10] float64 overwritten: the upper triangle, row-major, of the symmetric 4 x 4
 *     Q_v = sum over the faces of v of area (n, d)(n, d)^T  +  sum over its one-face sides of boundary_weight |e|^2 (m, d)(m, d)^T,
 *   n the face's unit normal, d = -n . p0, m the unit vector in the face's plane perpendicular to the side, d = -m . pa.  A zero-area
 *   face adds nothing.  A gather per vertex in list order: no float atomics.
 * gs_simplify_edge_costs  per edge (u, v) = (lo, hi), in float64 without contraction:  Q = Q_u + Q_v, A its upper 3 x 3, b = -Q[:3,3];
 *   p = A^-1 b (adjugate / determinant) is taken when |det A| > 1e-6 (tr A / 3)^3 and |p - mid| <= 2 |e|, otherwise the cheapest of
 *   u, v, fp32(mid) (the first on a tie);  position = fp32(p);  cost = fp32(max(h^T Q h, 0)), h = (position, 1);
 *   key = (bits of cost) << 32 | (i 0x9E3779B1 mod 2^32).
 *   valid: k in {1, 2};  |N(u) n N(v)| = k;  not (k = 2 and both endpoints on the boundary);  no face of u holds both opposite
 *   vertices;  every face with exactly one of u, v keeps a non-zero normal with n_old . n_new > min_normal_dot |n_old| |n_new| when
 *   that vertex moves to position;  cost and position finite.
 * gs_simplify_select  claim [V] uint64 (scratch, overwritten): every valid edge takes the 64-bit atomic minimum of its key into
 *   claim[w] for every w of {u, v} + N(u) + N(v);  winner [E] uint8 = valid and claim[u] == key and claim[v] == key.  Keys are unique,
 *   so the winners do not depend on the launch order, and no endpoint of a winner lies in the closed neighbourhood of another's.
 * gs_simplify_apply  for each of the n selected winners (edge indices, int64):  remap[v] = u,  vertices[u] = position,  Q_u += Q_v.
 *   The caller passes remap as the identity and maps the faces through it.
 * gs_components_step  one hook + compress pass of min-label components over `edges`: parent [V] (the caller starts it as the identity)
 *   keeps parent[x] <= x; an edge whose endpoints have different roots takes the 32-bit atomic minimum of the smaller root into the
 *   larger root's parent and sets *changed (cleared first); then every vertex points at its root.  Repeat until *changed stays 0:
 *   parent[x] is then the smallest vertex index of x's component.  No kernel waits for another workgroup. */
int gs_simplify_quadrics(int V, int F, const float* vertices, const int32_t* faces, const int32_t* vf_off, const int32_t* vf,
                         const uint8_t* side_boundary, double boundary_weight, double* quadrics, void* stream);
int gs_simplify_edge_costs(int V, int E, const float* vertices, const double* quadrics, const int32_t* faces, const int32_t* edges,
                           const int32_t* edge_faces, const int32_t* edge_opp, const int32_t* nbr_off, const int32_t* nbr,
                           const int32_t* vf_off, const int32_t* vf, const uint8_t* boundary, double min_normal_dot, float* position,
                           float* cost, uint8_t* valid, int64_t* key, void* stream);
int gs_simplify_select(int V, int E, const int32_t* edges, const uint8_t* valid, const int64_t* key, const int32_t* nbr_off,
                       const int32_t* nbr, uint64_t* claim, uint8_t* winner, void* stream);
int gs_simplify_apply(int V, int E, int n, const int64_t* selected, const int32_t* edges, const float* position, float* vertices,
                      double* quadrics, int64_t* remap, void* stream);
int gs_components_step(int V, int E, const int32_t* edges, int32_t* parent, int32_t* changed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOSPLAT_HIP_H */
